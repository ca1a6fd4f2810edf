"""Call sequences across features: a long-lived context against a fresh one (include/prt.h, csrc/hip/prt_ctx.h).

Every other test file creates a context, runs one feature's script and closes it.  Here a context lives through uploads, refits, rebuilds,
smoothing topologies, primitive moves, motion snapshots, ray queries, frame changes, filters and refused calls, and at every checkpoint it
must be INDISTINGUISHABLE, bit for bit, from a fresh context brought to the same logical state by the shortest route (Model.fresh).  The
logical state is tracked by `Model` from the calls made, never from read-backs of the context under test.

Both contexts run the code under test, so the last checkpoint of a sequence also compares the render with the CPU oracle on the model's scene:
the tree and the boxes from the numpy mirrors of test_rebuild / test_refit, the normals from test_smooth_normals' mirror, the primitive
records as the model holds them.

A step is a tuple of strings and ints -- ("rebuild", "p11", "none", 4) -- so that a failing random sequence prints as a scripted one.
LIFETIMES is the table of DESIGN.md s4 "What survives what": per piece of context state the calls that create it and what every other call
does to it, with the line of prt.h the entry comes from.  The CPU test at the end replays every sequence on the model alone and asserts that
every (creator, call) pair of the table occurs in one of them with the state really there: made by an accepted call, not dropped or consumed
by anything in between (a checkpoint's own calls included), and followed by a checkpoint."""
import hashlib
import os

import numpy as np
import pytest

from conftest import ROOT
from cases import deform, desc_with, _leaf_root_desc, meshes_of, move_quad, move_sdf, move_sphere, random_rays, _soup, Teapot, TILT, _with
from mirrors import DEFAULT_LEAF, mirror_build, mirror_normals, mirror_refit, mirror_weld, NODE_T
from support import assert_same_render as _assert_same, bytes_flat as _bytes

f32 = np.float32
W, H, FRAMES = Teapot.W, Teapot.H, Teapot.FRAMES
OK, INVALID, NOT_READY, UNSUPPORTED = 0, -1, -4, -5
ADAPT_MIN, ADAPT_MAX, ADAPT_REL = 8, 64, 0.2          # tests/test_adaptive.py MIN, MAX, REL
ADAPT_FRAMES = ADAPT_MAX * 16 + 64                    # ... and its _frames(MAX)
N_RAYS = 130                                          # two waves and a ragged tail
WHOLE = ("whole", W, H)
FRAME_MENU = {"whole": WHOLE, "small": ("whole", 40, 24), "blocks": ("blocks", W, H, 16, 2, 1), "blocks5": ("blocks", W, H, 5, 3, 2),
              "tile_bottom": ("tile", W, H, 0, 1), "tile_top": ("tile", W, H, H - 1, 1)}
FILTER_MENU = ("none", "gaussian", "tent", "box")
POSES = {"rest": None, "p11": 11, "p21": 21}
REFUSALS = ("nan_update", "nan_rebuild", "leaf65", "tile_outside", "radius5", "prim_type", "group_id", "misaligned")
QUERIES = ("q_cast", "q_occluded", "q_pixels")
# the calls that may write a plane (prt.h); every other call must leave its bits alone
WRITES = {"path state": ("render", "adaptive", "frame", "filter"), "framebuffer": ("render", "adaptive", "frame", "filter"),
          "adaptive plane": ("render", "adaptive", "frame", "filter"), "guides": ("guides",), "motion plane": ("guides",),
          "temporal history": ("temporal",)}


def _same(a, b):
    return a is b or (a is not None and b is not None and a.shape == b.shape and np.array_equal(_bytes(a), _bytes(b)))


def _digest(*arrays):
    h = hashlib.sha1()
    for a in arrays:
        h.update(b"-" if a is None else (a if isinstance(a, bytes) else np.ascontiguousarray(a).tobytes()))
        h.update(b"|")
    return h.hexdigest()


def _device_buffer(nbytes):
    import torch
    buf = torch.zeros(nbytes, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    return buf


def _try(fn, *a, **k):
    """("ok", value) or ("refused", code): what the two contexts of a checkpoint must agree on"""
    from conftest import PKG_NAME
    import importlib
    err = importlib.import_module(PKG_NAME).PrtError
    try:
        return ("ok", fn(*a, **k))
    except err as e:
        return ("refused", e.code)


def _agree(a, b, what):
    assert a[0] == b[0], "%s: %s on the long-lived context, %s on the fresh one" % (what, a if a[0] == "refused" else "ok", b if b[0] == "refused" else "ok")
    if a[0] == "refused":
        assert a[1] == b[1], "%s: refused with %s on the long-lived context, %s on the fresh one" % (what, a[1], b[1])
        return
    x, y = a[1], b[1]
    if not isinstance(x, tuple):
        x, y = (x,), (y,)
    for i, (p, q) in enumerate(zip(x, y)):
        if isinstance(p, np.ndarray):
            assert p.shape == q.shape and np.array_equal(_bytes(p), _bytes(q)), "%s: part %d differs between the long-lived and the fresh context" % (what, i)
        else:
            assert p == q, "%s: part %d: %r on the long-lived context, %r on the fresh one" % (what, i, p, q)


# ---- what can be uploaded under one configuration ------------------------------------------------------------------------------------------------

class Scene:
    """one uploadable scene: its desc, the buffers behind it and the primitive records as uploaded; shared, never written to"""

    def __init__(self, prt, key, desc, v0, n0, nodes0, prims0, m0):
        self.prt, self.key, self.desc, self.v0, self.n0, self.nodes0, self.prims0, self.m0 = prt, key, desc, v0, n0, nodes0, prims0, m0
        self.T = 0 if v0 is None else len(v0) // 3
        self._poses = {}
        for a in (v0, n0, nodes0, prims0, m0):
            if a is not None:
                a.setflags(write=False)

    def pose(self, name):
        """(vertices, normals) of a pose: the uploaded ones, or cases.deform of them"""
        if name not in self._poses:
            v, n = (self.v0, self.n0) if POSES[name] is None else deform(self.v0, self.n0, POSES[name])
            v.setflags(write=False)
            n.setflags(write=False)
            self._poses[name] = (v, n)
        return self._poses[name]


def _moved(m0, counts, which):
    """the primitive records in a moved pose: every sphere, SDF primitive and the last quad (test_update_primitives' movers)"""
    m = m0.copy()
    s = 1.0 if which == "mB" else -0.6
    n_sph, n_sdf, n_quad = int(counts[0]), int(counts[1]), int(counts[3])
    for i in range(n_sph):
        move_sphere(m, i, (0.08 * s, -0.05 * s, 0.06 * s), 0.03 * s)
    for i in range(n_sph, n_sph + n_sdf):
        move_sdf(m, i, (-0.06 * s, 0.04 * s, 0.05 * s))
    if n_quad:
        move_quad(m, n_sph + n_sdf + n_quad - 1, (0.02 * s, 0.0, 0.03 * s), TILT, 0.04 * s)
    m.setflags(write=False)
    return m


class Family:
    """one configuration (a scene file of conftest.VARIANTS) and everything a sequence under it chooses from; shared, never written to"""
    _cache = {}

    def __new__(cls, prt, name):
        if name in cls._cache:
            return cls._cache[name]
        self = super().__new__(cls)
        tp = Teapot(prt, seed=None, variant=name)
        self.prt, self.name, self.tp, self.cfg = prt, name, tp, tp.cfg
        self.has_sdf = int(tp.desc.object_count[1]) > 0
        a = prt.scene_arrays(tp.desc)
        m0 = meshes_of(tp.desc)
        self.scenes = {"A": Scene(prt, "A", tp.desc, tp.v0, tp.n0, a["nodes"].view(NODE_T).reshape(-1).copy(), a["primitive_indices"].copy(), m0)}
        for T in (3, 257) + ((6400,) if len(tp.v0) // 3 > 257 else ()):
            v, n = _soup("random", T)
            v[:, :3] = v[:, :3] * f32(1.5) + np.array([0, 1.5, 0], dtype=f32)          # (into the box, in front of the camera)
            d = _leaf_root_desc(prt, tp.desc, v, n)
            self.scenes["S%d" % T] = Scene(prt, "S%d" % T, d, v, n, d._keep[2].view(NODE_T).reshape(-1).copy(), d._keep[3].copy(), m0)
        d = prt.SceneDesc.from_buffer_copy(bytes(tp.desc))                              # the primitives alone
        d.triangle_count, d.bvh_node_count = 0, 0
        self.scenes["N0"] = Scene(prt, "N0", d, None, None, None, None, m0)
        self.meshes = {"m0": m0, "mA": _moved(m0, tp.desc.object_count, "mA"), "mB": _moved(m0, tp.desc.object_count, "mB")}
        orbit = prt.orbit_camera(W, H, d_yaw=0.15, d_pitch=0.05)
        orbit.apertureRadius = tp.cam.apertureRadius
        self.cams = {"default": tp.cam, "orbit": orbit}
        self.envs = {"sky": prt.make_sky(64, 32), "dim": np.ascontiguousarray(prt.make_sky(32, 16) * f32(0.25))}
        self._rays = None
        cls._cache[name] = self
        return self

    def rays(self):
        """130 rays of cases.random_rays through the uploaded scene's root box"""
        if self._rays is None:
            import cast_api
            cast_api.lib()
            self._rays = random_rays(self.prt, cast_api, self.name, n=N_RAYS)
        return self._rays

    def groups(self, scene):
        if not hasattr(scene, "_groups"):
            scene._groups = mirror_weld(scene.v0)
        return scene._groups


class _Dry:
    """in place of a context where the model runs alone: every method is None, which Model._call answers as prt.h says"""
    lib = ctx = None

    def __getattr__(self, name):
        return None


_DRY = _Dry()


# ---- the model -------------------------------------------------------------------------------------------------------------------------------------

class Model:
    """the logical state of a context, from the calls made.  `apply` makes one step on the context and here; `fresh` builds the same state by
    the shortest route"""

    def __init__(self, fam, scene="A"):
        self.fam, self.prt = fam, fam.prt
        self.cam, self.env, self.frame, self.filter = "default", None, WHOLE, "none"
        self.motion = False
        self.history = False
        self.log = []
        self._next_tree = 1
        self._upload(scene)

    # -- state changes ---------------------------------------------------------------------------------------------------------------------------
    def _upload(self, key):
        self.scene = self.fam.scenes[key]
        self.v, self.n = self.scene.v0, self.scene.n0
        self.tree, self.tree_id, self.updated = None, 0, False        # tree: (vertices at the last rebuild, max_leaf), None = as uploaded
        self.smooth = None                                            # (groups, n_groups, weighting, crease)
        self.m = self.scene.m0
        self.snap_tri, self.snap_prim = None, None                    # pending motion snapshots: what they hold
        self.guides_valid = self.motion_valid = False
        self.history = False

    def _frame_changed(self, frame):
        self.frame = frame
        self.guides_valid = self.motion_valid = self.history = False
        self.rendered = self.stats = False

    def _geometry_changed(self):
        self.guides_valid = False

    def _normals_for(self, v, given):
        if given is not None:
            return given
        if self.smooth is None:
            return self.n
        groups, _, weighting, crease = self.smooth
        n = mirror_normals(v, groups, 0 if weighting == "unit" else 1, crease)
        n.setflags(write=False)
        return n

    def _snapshot(self):
        if self.motion and self.snap_tri is None:
            self.snap_tri = dict(tree=self.tree, tree_id=self.tree_id, v=self.v)

    rendered = False
    stats = False
    guides_k = 1

    # -- the frame on a context --------------------------------------------------------------------------------------------------------------------
    @staticmethod
    def _set_frame(r, frame):
        if frame[0] == "whole":
            r.resize(frame[1], frame[2])
        elif frame[0] == "tile":
            r.set_tile(*frame[1:])
        else:
            r.set_row_blocks(*frame[1:])

    def whole(self):
        return self.frame[0] == "whole"

    def frame_rows(self):
        """the global rows of the frame part, in local order"""
        if self.frame[0] == "whole":
            return list(range(self.frame[2]))
        if self.frame[0] == "tile":
            return list(range(self.frame[3], self.frame[3] + self.frame[4]))
        _, _, h, block, parts, part = self.frame
        return [y for y in range(h) if (y // block) % parts == part]

    # -- one step ----------------------------------------------------------------------------------------------------------------------------------
    def expect(self, step):
        """the code prt.h says the step returns in this state"""
        op, T = step[0], self.scene.T
        if op in ("smooth", "update", "rebuild"):
            return OK if T else NOT_READY                                    # (no scene with triangles)
        if op == "filter":
            return UNSUPPORTED if step[1] != "none" and self.fam.has_sdf else OK
        if op in ("denoise", "temporal"):
            return UNSUPPORTED if not self.whole() else NOT_READY if not (self.guides_valid and self.rendered) else OK
        if op == "refuse":
            return INVALID if T or step[1] in ("tile_outside", "radius5", "prim_type", "misaligned") else NOT_READY
        return OK

    def apply(self, r, step):
        """the call on `r`, the code it must return (by prt.h, from the model), and its effect on the model; what prt.h says the call keeps
        must have the bits it had before -- everything, when the call is refused.  r None: the model alone (no device), every call
        answered as prt.h says"""
        self.log.append(step)
        op, args = step[0], step[1:]
        self._want = want = self.expect(step)
        if r is None:
            getattr(self, "_do_" + op)(_DRY, *args)
            return want
        before = self.observe(r)
        getattr(self, "_do_" + op)(r, *args)
        got, self._got = self._got, None
        assert got == want, "%s returned %s, the model says %s (prt.h)\n%s" % (step, got, want, self.replay())
        if got != OK:
            assert r.lib.prt_last_error(r.ctx), "%s was refused without a message\n%s" % (step, self.replay())
        self.check_validity(r, step)
        after = self.observe(r)
        if got == OK and op in ("frame", "filter"):                          # (prt.h: both imply prt_reset)
            for name in ("path state", "framebuffer", "adaptive plane"):
                assert not after[name].view(np.uint8).any(), "%s left the %s as it was: prt.h says it implies a reset\n%s" % (step, name, self.replay())
        for name in before:
            if got != OK:
                assert name in after, "%s was refused and the model dropped the %s\n%s" % (step, name, self.replay())
            if name in after and (got != OK or op not in WRITES[name]):         # (the model says it is still there)
                assert _same(before[name], after[name]), "%s changed the %s, which prt.h says it keeps\n%s" % (step, name, self.replay())
        return got

    def check_validity(self, r, step):
        """what prt.h says is refused in this state is refused, what it says is there is served"""
        for name, read, there in (("guides", r.read_guides, self.guides_valid),
                                  ("motion plane", r.read_motion, self.motion and self.guides_valid and self.motion_valid),
                                  ("temporal history", r.read_history, self.history)):
            t = _try(read)
            want = ("ok",) if there else ("refused", NOT_READY)
            assert t[:len(want)] == want, "after %s the %s should be %s (prt.h): reading it gave %s\n%s" % (
                step, name, "there" if there else "stale or empty", "ok" if t[0] == "ok" else t, self.replay())

    def observe(self, r):
        """the planes the model says are there, as the context holds them"""
        out = {"path state": r.read_state(), "framebuffer": r.read_framebuffer(), "adaptive plane": r.read_adaptive_stats()}
        if self.guides_valid:
            out["guides"] = r.read_guides()
            if self.motion and self.motion_valid:
                out["motion plane"] = r.read_motion()
        if self.history:
            out["temporal history"] = r.read_history()
        return out

    _got = None

    def _call(self, fn, *a, **k):
        if fn is None:                                                      # (the model alone: as prt.h says)
            return self._want == OK
        t = _try(fn, *a, **k)
        self._got = OK if t[0] == "ok" else t[1]
        return self._got == OK

    def replay(self):
        return "family %s, steps so far:\n    %s" % (self.fam.name, ",\n    ".join(repr(s) for s in self.log))

    def _do_upload(self, r, key):
        if self._call(r.upload_scene, self.fam.scenes[key].desc):
            self._upload(key)

    def _do_envmap(self, r, key):
        if self._call(r.upload_envmap, self.fam.envs[key]):
            self.env = key
            self.guides_valid = self.history = False

    def _do_camera(self, r, key):
        if self._call(r.set_camera, self.fam.cams[key]):
            self.cam = key
            self.guides_valid = False

    def _do_frame(self, r, key):
        if self._call(None if r is _DRY else self._set_frame, r, FRAME_MENU[key]):
            self._frame_changed(FRAME_MENU[key])

    def _do_filter(self, r, kind):
        if self._call(r.set_pixel_filter, kind):
            self.filter = kind
            self.guides_valid = False
            self.rendered = self.stats = False

    def _do_smooth(self, r, mode):
        T = self.scene.T
        if mode == "off":
            if self._call(r.set_smooth_normals, None):
                self.smooth = None
        else:
            groups, n_groups = self.fam.groups(self.scene) if T else (np.zeros(0, dtype=np.uint32), 1)
            crease = self.prt.LOADER_CREASE_COS if mode == "unit" else 0.5
            if self._call(r.set_smooth_normals, groups, n_groups, mode, crease):
                self.smooth = (groups, n_groups, mode, crease)

    def _pose(self, pose, normals):
        if not self.scene.T:
            return np.zeros((3, 4), dtype=f32), None
        v, n = self.scene.pose(pose)
        return v, (n if normals == "given" else None)

    def _do_update(self, r, pose, normals):
        v, n = self._pose(pose, normals)
        if self._call(r.update_vertices, v, n):
            self._snapshot()
            self.n = self._normals_for(v, n)
            self.v, self.updated = v, True
            self._geometry_changed()

    def _do_rebuild(self, r, pose, normals, max_leaf):
        v, n = self._pose(pose, normals)
        if self._call(r.rebuild_bvh, v, n, max_leaf):
            self._snapshot()
            self.n = self._normals_for(v, n)
            self.v, self.updated = v, False
            self.tree, self.tree_id = (v, max_leaf if max_leaf else DEFAULT_LEAF), self._next_tree
            self._next_tree += 1
            self._geometry_changed()

    def _do_prims(self, r, key):
        m = self.fam.meshes[key]
        if self._call(r.update_primitives, m):
            if self.motion and self.snap_prim is None:
                self.snap_prim = self.m
            self.m = m
            self._geometry_changed()

    def _do_motion(self, r, on):
        if self._call(r.set_motion, bool(on)) and bool(on) != self.motion:
            self.motion = bool(on)
            self.guides_valid = self.motion_valid = False
            if not on:
                self.snap_tri = self.snap_prim = None

    def _do_render(self, r, frames):
        def go():
            r.reset()
            r.render_frames(self.prt.seed_pairs(frames))
        if self._call(None if r is _DRY else go):
            self.rendered, self.stats = True, False

    def _do_adaptive(self, r):
        def go():
            r.reset()
            t = _try(r.render_adaptive, self.prt.seed_pairs(ADAPT_FRAMES), ADAPT_MIN, ADAPT_MAX, ADAPT_REL)
            assert t[0] == "ok" or t[1] == NOT_READY, t             # (NOT_READY: max_frames ran out, every live pixel did max_frames)
        if self._call(None if r is _DRY else go):
            self.rendered = self.stats = True

    def _do_guides(self, r, samples):
        if self._call(r.render_guides, samples):
            self.guides_valid, self.motion_valid, self.guides_k = True, self.motion, samples
            if self.motion:
                self.snap_tri = self.snap_prim = None

    def _do_denoise(self, r):
        self._call(r.denoise)

    def _do_temporal(self, r):
        if self._call(r.denoise_temporal):
            self.history = True

    def _do_reset_history(self, r):
        if self._call(r.reset_history):
            self.history = False

    def _do_q_cast(self, r):
        self._call(r.cast_rays, self.fam.rays())

    def _do_q_occluded(self, r):
        self._call(r.occluded, self.fam.rays())

    def _do_q_pixels(self, r):
        self._call(r.cast_pixels, self.pixels())

    def pixels(self):
        w, h = self.frame[1], self.frame[2]
        return np.array([[0, 0], [w - 1, 0], [0, h - 1], [w - 1, h - 1], [w // 2, h // 2]], dtype=np.int32)

    def _do_refuse(self, r, kind):
        """one call prt.h documents as refused before anything is written; the model does not change"""
        T = self.scene.T
        bad = np.zeros((3, 4), dtype=f32)
        if T:
            bad = self.v.copy()
            bad[len(bad) // 2, 1] = np.nan
        if kind == "nan_update":
            self._call(r.update_vertices, bad, None)
        elif kind == "nan_rebuild":
            self._call(r.rebuild_bvh, bad, None, 2)
        elif kind == "leaf65":
            self._call(r.rebuild_bvh, self.v if T else bad, None, 65)
        elif kind == "tile_outside":
            self._call(r.set_tile, self.frame[1], self.frame[2], self.frame[2] - 1, 2)
        elif kind == "radius5":
            self._call(r.set_pixel_filter, "box", 5.0)
        elif kind == "prim_type":
            m = self.m.copy()
            m["t"][0] = 8 if m["t"][0] != 8 else 1
            self._call(r.update_primitives, m)
        elif kind == "group_id":
            g = np.zeros(3 * T, dtype=np.uint32)
            if T:
                g[1] = 5
            self._call(r.set_smooth_normals, g, 5)
        elif kind == "misaligned":
            if r is _DRY:
                return
            buf = _device_buffer(len(self.m) * 256 + 16)
            self._call(r.update_primitives, buf.data_ptr() + 4, device=True)
        else:
            raise KeyError(kind)

    # -- the shortest route ------------------------------------------------------------------------------------------------------------------------
    def fresh(self):
        """a new context in this logical state: upload, map, camera, frame, filter, topology, one rebuild, one update, one primitive update, and
        with motion on the geometry of the pending snapshots first, set_motion and a guide render in between"""
        sc, T = self.scene, self.scene.T
        f = self.prt.Renderer(self.fam.cfg, device=0)
        f.upload_scene(sc.desc)
        if self.env is not None:
            f.upload_envmap(self.fam.envs[self.env])
        f.set_camera(self.fam.cams[self.cam])
        self._set_frame(f, self.frame)
        if self.filter != "none":
            f.set_pixel_filter(self.filter)
        if self.smooth is not None:
            f.set_smooth_normals(*self.smooth)
        at = dict(tree_id=0, v=sc.v0, n=sc.n0)

        def to(tree, tree_id, v, force):
            """the tree and the vertices, by at most one rebuild and one update with the final normals"""
            if not T:
                return
            if tree_id != at["tree_id"]:
                f.rebuild_bvh(tree[0], self.n, tree[1])
                at.update(tree_id=tree_id, v=tree[0], n=self.n)
                force = False
            if force or not _same(at["v"], v) or not _same(at["n"], self.n):
                f.update_vertices(v, self.n)
                at.update(v=v, n=self.n)

        if not self.motion:
            to(self.tree, self.tree_id, self.v, self.updated)
            if not _same(self.m, sc.m0):
                f.update_primitives(self.m)
            return f
        pre = self.snap_tri or dict(tree=self.tree, tree_id=self.tree_id, v=self.v)
        to(pre["tree"], pre["tree_id"], pre["v"], self.updated and self.snap_tri is None)
        m_pre = self.m if self.snap_prim is None else self.snap_prim
        if not _same(m_pre, sc.m0):
            f.update_primitives(m_pre)
        f.set_motion(True)
        f.render_guides(1)                                             # (consumes nothing: motion was off until here)
        if self.snap_tri is not None:
            to(self.tree, self.tree_id, self.v, True)
        if self.snap_prim is not None:
            f.update_primitives(self.m)
        return f

    # -- the model's scene for the oracle ----------------------------------------------------------------------------------------------------------
    def oracle_tree(self):
        sc = self.scene
        if self.tree is None:
            nodes, prims = sc.nodes0, sc.prims0
        else:
            nodes, prims = mirror_build(self.tree[0], self.tree[1])[:2]
        if self.updated:
            nodes = mirror_refit(nodes, prims, self.v)
        return nodes, prims

    def oracle_render(self, oracle):
        sc, prt = self.scene, self.prt
        if sc.T:
            nodes, prims = self.oracle_tree()
            base = _with(prt, sc.desc, self.v, self.n, nodes, prims, T=sc.T)
            key = _digest(self.v, self.n, nodes, prims)
        else:
            base, key = sc.desc, "no triangles"
        m = np.ascontiguousarray(self.m)
        desc = desc_with(prt, base, m)
        desc._keep.append(base)
        cam, env = self.fam.cams[self.cam], None if self.env is None else self.fam.envs[self.env]
        key = _digest(self.fam.name.encode(), key.encode(), m, bytes(cam), env, repr(self.frame).encode())
        if key not in _oracle_cache:
            kw = {}
            if self.frame[0] == "tile":
                kw = dict(row0=self.frame[3], rows=self.frame[4])
            elif self.frame[0] == "blocks":
                kw = dict(blocks=self.frame[3:6])
            st, img = oracle.Restatement().render(self.fam.cfg, desc, cam, self.frame[1], self.frame[2], prt.seed_pairs(FRAMES), env=env, threads=8, **kw)
            st.setflags(write=False)
            img.setflags(write=False)
            _oracle_cache[key] = (st, img)
        return _oracle_cache[key]


_oracle_cache = {}


# ---- the checkpoint --------------------------------------------------------------------------------------------------------------------------------

def checkpoint(r, model, oracle=None):
    """`r` against model.fresh(), all by bytes; with `oracle` the render against the CPU oracle on the model's scene as well.  The calls go
    through model.apply on `r`, so the model follows what the checkpoint itself does to the context"""
    prt, what = model.prt, "checkpoint after step %d" % len(model.log)
    try:
        model.check_validity(r, "the last step")
        f = model.fresh()
        try:
            _compare(r, f, model, oracle, what)
        finally:
            f.close()
    except Exception as e:                                               # (a PrtError of the fresh context's route included)
        raise _with_steps(model, e, what + ": ") from None


def _with_steps(model, e, prefix=""):
    """the failure with the steps so far behind it, once: every failure of a sequence can be replayed as a scripted one"""
    msg = "%s%s%s" % (prefix, "" if isinstance(e, AssertionError) else type(e).__name__ + ": ", e)
    return AssertionError(msg if "steps so far" in msg else msg + "\n" + model.replay())


def _compare(r, f, model, oracle, what):
    prt = model.prt
    both = lambda name, *a, **k: (_try(getattr(r, name), *a, **k), _try(getattr(f, name), *a, **k))      # noqa: E731
    log = len(model.log)
    # the render
    model.apply(r, ("render", FRAMES))
    f.reset()
    f.render_frames(prt.seed_pairs(FRAMES))
    state, img = r.read_state(), r.read_framebuffer()
    _agree(("ok", (state, img)), ("ok", (f.read_state(), f.read_framebuffer())), "render_frames")
    if oracle is not None:
        assert model.filter == "none", "the oracle anchor renders without a pixel filter"
        ostate, oimg = model.oracle_render(oracle)
        _assert_same(oracle, ostate, oimg, state, img, "the render against the CPU oracle")
    # one path per pixel
    seeds = prt.seed_pairs(2 * max(model.fam.cfg.max_bounces, 8) + 64)
    r.reset()
    f.reset()
    _agree(*both("render_spp", 1, seeds), "render_spp")
    _agree(*both("read_state"), "render_spp: the path state")
    _agree(*both("read_framebuffer"), "render_spp: the framebuffer")
    # guides and the motion plane
    kept = r.read_guides() if model.guides_valid else None            # (valid guides: what a fresh context renders with as many samples)
    k = model.guides_k if kept is not None else 1
    model.apply(r, ("guides", k))
    f.render_guides(k)
    _agree(*both("read_guides"), "guides")
    if kept is not None:
        assert _same(kept, r.read_guides()), "the guides the context kept are not the guides of this scene, camera, map and frame"
    _agree(*both("read_motion"), "the motion plane")
    # the tree and the normals
    if model.scene.T:
        a, b = both("read_bvh")
        _agree(a, b, "read_bvh")
        _agree(*both("read_bvh_bounds"), "read_bvh_bounds")
        _agree(*both("read_normals"), "read_normals")
    # the ray queries
    rays = model.fam.rays()
    _agree(*both("cast_rays", rays), "cast_rays")
    _agree(*both("occluded", rays), "occluded")
    _agree(*both("cast_pixels", model.pixels()), "cast_pixels")
    # the filters, from an empty history
    model.apply(r, ("reset_history",))
    f.reset_history()
    _agree(*both("denoise"), "denoise")
    t = both("denoise_temporal")
    _agree(*t, "denoise_temporal")
    assert (OK if t[0][0] == "ok" else t[0][1]) == model.expect(("temporal",)), "denoise_temporal: %s, the model says %s" % (t[0][:2] if t[0][0] != "ok" else "ok", model.expect(("temporal",)))
    model.history = t[0][0] == "ok"
    _agree(*both("read_history"), "the history")
    # adaptive sampling
    model.apply(r, ("adaptive",))
    f.reset()
    _try(f.render_adaptive, prt.seed_pairs(ADAPT_FRAMES), ADAPT_MIN, ADAPT_MAX, ADAPT_REL)
    _agree(*both("read_adaptive_stats"), "the adaptive plane")
    _agree(*both("read_state"), "render_adaptive: the path state")
    _agree(*both("read_framebuffer"), "render_adaptive: the framebuffer")
    del model.log[log:]                                                 # (the checkpoint's own calls are not steps of the sequence)


# ---- running a sequence ----------------------------------------------------------------------------------------------------------------------------

CHECK = ("checkpoint",)
CHECK_ORACLE = ("checkpoint", "oracle")


def context(model):
    r = model.prt.Renderer(model.fam.cfg, device=0)
    r.upload_scene(model.scene.desc)
    r.set_camera(model.fam.cams[model.cam])
    r.resize(W, H)
    return r


def with_queries_and_refusals(steps):
    """between every two steps all three kinds of ray query and one refused call, cycled through REFUSALS"""
    out, k = [], 0
    for s in steps:
        out.append(s)
        if s[0] != "checkpoint":
            out += [(q,) for q in QUERIES] + [("refuse", REFUSALS[k % len(REFUSALS)])]
            k += 1
    return out


def run(prt, oracle, family, steps, scene="A"):
    model = Model(Family(prt, family), scene)
    r = context(model)
    try:
        for s in steps:
            if s[0] == "checkpoint":
                checkpoint(r, model, oracle if len(s) > 1 else None)
            else:
                model.apply(r, s)
    except Exception as e:
        raise _with_steps(model, e) from None
    finally:
        r.close()
    return model


# ---- scripted sequences ----------------------------------------------------------------------------------------------------------------------------

SCENE_CHURN = [
    ("update", "p11", "given"), ("rebuild", "p21", "given", 4), ("smooth", "unit"), ("motion", 1), ("update", "p11", "none"), ("q_cast",),
    ("upload", "S3"), CHECK,
    ("upload", "S6400"), ("rebuild", "rest", "given", 4), ("update", "p11", "none"), CHECK,
    ("upload", "A"), ("rebuild", "rest", "given", 0), CHECK_ORACLE,
]
FRAME_CHURN = [
    ("render", FRAMES), ("adaptive",), ("guides", 1), ("temporal",), ("temporal",),
    ("frame", "blocks"), ("adaptive",), ("temporal",), CHECK,
    ("frame", "tile_bottom"), CHECK,
    ("frame", "whole"), CHECK_ORACLE,
]
FILTER_VIEW_MAP = [
    ("filter", "gaussian"), ("render", FRAMES), ("envmap", "sky"), ("camera", "orbit"), ("frame", "small"), ("upload", "S257"), CHECK,
    ("filter", "none"), CHECK_ORACLE,
]
MOTION_ACROSS = [
    ("motion", 1), ("update", "p11", "given"), ("prims", "mA"), ("rebuild", "p21", "none", 4), ("frame", "small"), CHECK,
    ("motion", 0), ("motion", 1), ("update", "rest", "given"), ("prims", "mB"), CHECK,
    ("update", "p21", "none"), ("upload", "A"), CHECK_ORACLE,
]
# a checkpoint's guide render consumes the snapshots; these keep them pending over everything else a context can do in between
SNAPSHOTS_PENDING = [
    ("motion", 1), ("guides", 1), ("update", "p11", "given"), ("update", "p21", "given"), ("prims", "mA"), ("prims", "mB"),
    ("camera", "orbit"), ("envmap", "dim"), ("frame", "blocks5"), ("frame", "whole"), ("filter", "tent"), ("render", 8), ("q_occluded",),
    ("refuse", "nan_update"), ("refuse", "prim_type"), ("smooth", "area"), ("rebuild", "p11", "none", 16), ("filter", "none"), CHECK_ORACLE,
]
# the survival lists of prt.h, call by call: what keeps the guides and the history is followed by a step that needs them
SURVIVAL_LISTS = [
    ("render", 8), ("guides", 2), ("temporal",), ("smooth", "unit"), ("render", 8), ("q_pixels",), ("camera", "orbit"),
    ("guides", 1), ("temporal",), ("update", "p11", "none"), ("prims", "mA"), ("reset_history",),
    ("guides", 1), ("prims", "mB"), ("guides", 1), ("filter", "box"), ("render", 8), ("guides", 1), ("temporal",), ("envmap", "sky"),
    ("adaptive",), ("render", 8), ("guides", 2), ("q_cast",), CHECK, ("guides", 2), ("upload", "S257"), ("filter", "none"), CHECK_ORACLE,
]
SNAPSHOTS_DROPPED = [
    ("motion", 1), ("prims", "mA"), ("guides", 1), ("prims", "mB"), ("motion", 0), ("motion", 1), ("rebuild", "p11", "given", 4),
    ("upload", "A"), ("prims", "mA"), CHECK_ORACLE,
]
# ... and those of the scene's own state: a topology across frame changes, the planes across updates, the history across a rebuild and a
# change of set_motion
SURVIVAL_LISTS_SCENE = [
    ("smooth", "unit"), ("frame", "small"), ("frame", "tile_top"), ("frame", "whole"), ("update", "p11", "none"),
    ("adaptive",), ("update", "p21", "none"), ("guides", 1), ("temporal",), ("rebuild", "p11", "none", 4),
    ("render", 8), ("guides", 1), ("denoise",), ("temporal",), ("motion", 1), CHECK_ORACLE,
]
# snapshots that are really there -- motion on, taken by a rebuild, by an update, by a primitive move -- when the next call arrives
SNAPSHOTS_LIVE = [
    ("motion", 1), ("rebuild", "p11", "given", 4), ("rebuild", "p21", "none", 1), ("prims", "mA"), ("update", "p11", "given"), ("q_cast",), ("q_pixels",),
    ("guides", 1), ("update", "rest", "given"), ("guides", 2), ("rebuild", "p11", "none", 4), ("motion", 0),
    ("motion", 1), ("prims", "mB"), ("upload", "S257"), CHECK, ("rebuild", "rest", "given", 4), ("prims", "mA"), CHECK_ORACLE,
]
SCRIPTED = {
    "survival_lists": ("cornell_coat", SURVIVAL_LISTS),
    "survival_lists_scene": ("cornell_coat", SURVIVAL_LISTS_SCENE),
    "snapshots_live": ("cornell_sdf", SNAPSHOTS_LIVE),
    "snapshots_dropped": ("cornell_sdf", SNAPSHOTS_DROPPED),
    "scene_churn": ("cornell_coat", SCENE_CHURN),
    "frame_churn": ("cornell_quadlight", FRAME_CHURN),
    "filter_view_map": ("cornell_coat", FILTER_VIEW_MAP),
    "motion_across_everything": ("cornell_sdf", MOTION_ACROSS),
    "snapshots_pending": ("cornell_quadlight", SNAPSHOTS_PENDING),
    "scene_churn_with_queries_and_refusals": ("cornell_coat", with_queries_and_refusals(SCENE_CHURN)),
    "frame_churn_with_queries_and_refusals": ("cornell_edge", with_queries_and_refusals(FRAME_CHURN)),
}


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(SCRIPTED))
def test_scripted_sequence(prt, oracle, name):
    family, steps = SCRIPTED[name]
    assert steps[-1] == CHECK_ORACLE, "every scripted sequence ends with an oracle comparison"
    model = run(prt, oracle, family, steps)
    if name.startswith("frame_churn"):
        assert model.frame == WHOLE and model.history, "the history of the last checkpoint's temporal call"


@pytest.mark.gpu
def test_frame_churn_planes_have_the_new_size(prt):
    """after set_row_blocks the history is empty, the adaptive plane has the part's size and reads as the render left it"""
    model = Model(Family(prt, "cornell_quadlight"))
    r = context(model)
    try:
        for s in FRAME_CHURN[:5]:
            model.apply(r, s)
        assert model.history and r.read_history().shape == (H, W, 8)
        model.apply(r, ("frame", "blocks"))
        assert _try(r.read_history) == ("refused", NOT_READY), "the history is empty after set_row_blocks"
        assert not r.read_adaptive_stats().any(), "the adaptive plane of a new frame part is zeros"
        model.apply(r, ("adaptive",))
        model.apply(r, ("temporal",))                                   # (refused: the filter needs the whole frame)
        plane = r.read_adaptive_stats()
    finally:
        r.close()
    assert plane.shape == (16 * W, 2) and plane.any()


@pytest.mark.gpu
def test_checkpoint_and_resume_across_a_change(prt, oracle):
    """read_state after k frames, a rebuild and a primitive update, resize to the same size (zeroes everything), write_state, the remaining
    frames: the path state of an uninterrupted render, and the oracle's resume from the same state bit for bit"""
    k = 10
    seeds = prt.seed_pairs(FRAMES)
    fam = Family(prt, "cornell_edge")

    def first_half(model, r):
        r.reset()
        r.render_frames(seeds[:2 * k])
        model.apply(r, ("rebuild", "p11", "given", 1))
        model.apply(r, ("prims", "mB"))

    model = Model(fam)
    r = context(model)
    first_half(model, r)                                                # (the uploaded scene for k frames, the changed one from there)
    r.render_frames(seeds[2 * k:], first_frame=k + 1)
    want_state, want_img = r.read_state(), r.read_framebuffer()
    r.close()

    model = Model(fam)
    r = context(model)
    r.render_frames(seeds[:2 * k])
    ck, ck_img = r.read_state(), r.read_framebuffer()
    ostate, oimg = oracle.Restatement().render(fam.cfg, model.scene.desc, fam.cams["default"], W, H, seeds[:2 * k], threads=8)
    _assert_same(oracle, ostate, oimg, ck, ck_img, "the first %d frames" % k)
    model.apply(r, ("rebuild", "p11", "given", 1))
    model.apply(r, ("prims", "mB"))
    model.apply(r, ("frame", "whole"))
    assert not r.read_state().view(np.uint8).any() and not r.read_framebuffer().any(), "resize zeroes everything"
    r.write_state(ck)
    assert np.array_equal(_bytes(r.read_framebuffer()), _bytes(ck_img)), "write_state sets the framebuffer as the render left it"
    r.render_frames(seeds[2 * k:], first_frame=k + 1)
    state, img = r.read_state(), r.read_framebuffer()
    r.close()
    _agree(("ok", (want_state, want_img)), ("ok", (state, img)), "resumed against uninterrupted")
    nodes, prims = model.oracle_tree()
    base = _with(prt, model.scene.desc, model.v, model.n, nodes, prims, T=model.scene.T)
    desc = desc_with(prt, base, np.ascontiguousarray(model.m))
    rstate, rimg = oracle.Restatement().render(fam.cfg, desc, fam.cams["default"], W, H, seeds[2 * k:], first_frame=k + 1,
                                               state=np.array(ostate), threads=8)
    _assert_same(oracle, rstate, rimg, state, img, "the oracle resuming from the same state")


# ---- seeded random sequences -----------------------------------------------------------------------------------------------------------------------

SEEDS = {101: "cornell_coat", 202: "cornell_coat", 303: "cornell_sdf", 404: "cornell_quadlight", 505: "cornell_edge"}
N_STEPS = 30
OPS = ("upload", "envmap", "camera", "frame", "filter", "smooth", "update", "rebuild", "prims", "motion", "render", "adaptive", "guides",
       "denoise", "temporal", "reset_history", "refuse") + QUERIES


def generate(seed, family, n=N_STEPS):
    """n steps drawn from OPS with arguments from the small fixed menus, a checkpoint behind every fifth step and the last one.  (The soup of
    6 400 is the scripted scene churn's alone: a checkpoint on its leaf-root upload walks 6 400 triangles per ray and took 8 s.)"""
    rng = np.random.default_rng(seed)
    scenes = ["A", "S3", "S257", "N0"]
    pick = lambda menu: menu[int(rng.integers(len(menu)))]               # noqa: E731
    steps = []
    for i in range(n):
        op = pick(OPS)
        if op == "upload":
            s = (op, pick(scenes))
        elif op == "envmap":
            s = (op, pick(("sky", "dim")))
        elif op == "camera":
            s = (op, pick(("default", "orbit")))
        elif op == "frame":
            s = (op, pick(tuple(FRAME_MENU)))
        elif op == "filter":
            s = (op, pick(FILTER_MENU))
        elif op == "smooth":
            s = (op, pick(("unit", "area", "off")))
        elif op == "update":
            s = (op, pick(tuple(POSES)), pick(("given", "none")))
        elif op == "rebuild":
            s = (op, pick(tuple(POSES)), pick(("given", "none")), int(pick((0, 1, 4, 16))))
        elif op == "prims":
            s = (op, pick(("m0", "mA", "mB")))
        elif op == "motion":
            s = (op, int(pick((0, 1))))
        elif op == "render":
            s = (op, 8)
        elif op == "guides":
            s = (op, int(pick((1, 2))))
        elif op == "refuse":
            s = (op, pick(REFUSALS))
        else:
            s = (op,)
        steps.append(s)
        if i % 5 == 4 or i == n - 1:
            steps.append(CHECK)
    return steps


@pytest.mark.gpu
@pytest.mark.parametrize("seed", list(SEEDS))
def test_random_sequence(prt, oracle, seed):
    steps = generate(seed, SEEDS[seed])
    model = Model(Family(prt, SEEDS[seed]))
    r = context(model)
    try:
        for i, s in enumerate(steps):
            if s[0] != "checkpoint":
                model.apply(r, s)
            else:                                                       # the last checkpoint against the oracle too, where it renders this state
                last = i == len(steps) - 1
                checkpoint(r, model, oracle if last and model.filter == "none" else None)
    except Exception as e:
        raise _with_steps(model, e, "seed %d: " % seed) from None
    finally:
        r.close()


# ---- the lifetime table and the generator (no GPU) -------------------------------------------------------------------------------------------------

# state -> (the calls that create it, {call: (what it does to the state, where prt.h says so)}).  "drops" ends the state's life; "keeps" and
# "reallocates" do not.  DESIGN.md s4 "What survives what" is this table
LIFETIMES = {
    "guides": (("guides",), {
        "upload": ("drops", 421), "camera": ("drops", 421), "envmap": ("drops", 421), "frame": ("drops", 421), "filter": ("drops", 644),
        "update": ("drops", 181), "prims": ("drops", 216), "rebuild": ("drops", 254), "motion": ("drops", 464), "render": ("keeps", 422),
        "smooth": ("keeps", 312), "q_cast": ("keeps", 745), "q_occluded": ("keeps", 745), "q_pixels": ("keeps", 745)}),
    "temporal history": (("temporal",), {
        "upload": ("drops", 549), "envmap": ("drops", 549), "frame": ("drops", 550), "reset_history": ("drops", 550), "render": ("keeps", 549),
        "camera": ("keeps", 549), "filter": ("keeps", 645), "update": ("keeps", 182), "prims": ("keeps", 216), "rebuild": ("keeps", 254),
        "motion": ("keeps", 464), "smooth": ("keeps", 312), "q_cast": ("keeps", 745), "q_occluded": ("keeps", 745), "q_pixels": ("keeps", 745)}),
    "adaptive plane and live list": (("adaptive",), {
        "render": ("drops", 369), "frame": ("drops", 369), "filter": ("drops", 644), "q_cast": ("keeps", 745), "q_occluded": ("keeps", 745),
        "q_pixels": ("keeps", 745), "denoise": ("keeps", 499), "temporal": ("keeps", 548)}),
    "path state and framebuffer": (("render", "adaptive"), {
        "frame": ("drops", 332), "filter": ("drops", 644), "update": ("keeps", 181), "prims": ("keeps", 216), "rebuild": ("keeps", 254),
        "q_cast": ("keeps", 745), "q_occluded": ("keeps", 745), "q_pixels": ("keeps", 745), "denoise": ("keeps", 499), "temporal": ("keeps", 548)}),
    "triangle snapshot": (("update", "rebuild"), {
        "upload": ("drops", 435), "motion": ("drops", 435), "guides": ("drops", 433), "update": ("keeps", 432), "rebuild": ("keeps", 257),
        "prims": ("keeps", 217), "q_cast": ("keeps", 746), "q_occluded": ("keeps", 746), "q_pixels": ("keeps", 746)}),
    "primitive snapshot": (("prims",), {
        "upload": ("drops", 443), "motion": ("drops", 443), "guides": ("drops", 442), "prims": ("keeps", 442), "update": ("keeps", 443),
        "rebuild": ("keeps", 443), "q_cast": ("keeps", 746), "q_occluded": ("keeps", 746), "q_pixels": ("keeps", 746)}),
    "refit and rebuild tables": (("update", "rebuild"), {
        "upload": ("drops", 158), "update": ("keeps", 252), "rebuild": ("reallocates", 259), "prims": ("keeps", 217), "q_cast": ("keeps", 745)}),
    "smoothing topology": (("smooth",), {
        "upload": ("drops", 313), "render": ("keeps", 312), "frame": ("keeps", 312), "camera": ("keeps", 312), "update": ("keeps", 313),
        "rebuild": ("keeps", 313), "prims": ("keeps", 217)}),
    "pixel filter": (("filter",), {"frame": ("keeps", 645), "upload": ("keeps", 645)}),
    "environment map": (("envmap",), {"upload": ("keeps", 329)}),
}


# whether the state is there, by the model
ALIVE = {
    "guides": lambda m: m.guides_valid,
    "temporal history": lambda m: m.history,
    "adaptive plane and live list": lambda m: m.stats,
    "path state and framebuffer": lambda m: m.rendered,
    "triangle snapshot": lambda m: m.snap_tri is not None,
    "primitive snapshot": lambda m: m.snap_prim is not None,
    "refit and rebuild tables": lambda m: m.updated or m.tree is not None,
    "smoothing topology": lambda m: m.smooth is not None,
    "pixel filter": lambda m: m.filter != "none",
    "environment map": lambda m: m.env is not None,
}
# the words a line of prt.h that LIFETIMES cites speaks in: a citation that an edit of the header has moved off its sentence fails
LIFETIME_WORDS = ("keep", "kept", "stale", "survive", "drop", "empt", "zeroed", "consume", "Implies", "implies a reset", "writes none", "writes nothing",
                  "oldest", "pending", "unchanged", "turns it off", "last prt_upload_scene", "swapped in", "refits", "stay as they are")


# the oldest snapshot wins and a second update refits the same tables: a later creating call does not make these anew
KEEPS_ITS_MAKER = ("triangle snapshot", "primitive snapshot", "refit and rebuild tables")


def all_sequences():
    """name -> (family, steps)"""
    out = dict(SCRIPTED)
    out.update({"seed %d" % s: (fam, generate(s, fam)) for s, fam in SEEDS.items()})
    return out


def dry_checkpoint(model):
    """what a checkpoint's own calls do to the state (checkpoint / _compare), on the model alone"""
    n = len(model.log)
    for s in (("render", FRAMES), ("guides", model.guides_k if model.guides_valid else 1), ("reset_history",), ("temporal",), ("adaptive",)):
        model.apply(None, s)
    del model.log[n:]


def exercised_pairs(prt, family, steps):
    """the (state, creator, call) triples of LIFETIMES that the sequence exercises, by the model alone (no device): `creator` was accepted
    and left the state there -- a topology that was set, not turned off or refused on a scene without triangles; a snapshot taken with
    motion on; a history that a temporal call was served --, the state stayed there through every step up to `call`, its own checkpoints'
    guide renders, resets and filters included, `call` was accepted (a set_motion that changes the value), and a checkpoint follows.  Where the
    table says `call` drops the state the model must say so too, and the other way round"""
    model = Model(Family(prt, family))
    live = dict.fromkeys(LIFETIMES)                  # state -> the step name that created it, None while it is not there
    found, waiting = set(), []
    for s in steps:
        if s[0] == "checkpoint":
            found.update(waiting)
            waiting = []
            dry_checkpoint(model)
            for state in live:
                if not ALIVE[state](model):
                    live[state] = None
            continue
        op, motion_before = s[0], model.motion
        accepted = model.apply(None, s) == OK and not (op == "motion" and model.motion == motion_before)
        for state, (creators, table) in LIFETIMES.items():
            was, now = live[state], ALIVE[state](model)
            if was is not None and accepted and op in table:
                assert now == (table[op][0] != "drops"), "%s %s the %s by the table, the model says it is %s" % (s, table[op][0], state, "there" if now else "gone")
                waiting.append((state, was, op))
            if not now:
                live[state] = None
            elif accepted and op in creators and (was is None or state not in KEEPS_ITS_MAKER):
                live[state] = op
    assert not waiting, "a sequence ends with a checkpoint"
    return found


def test_the_generator_is_deterministic_and_covers_the_lifetime_table(prt):
    for seed, fam in SEEDS.items():
        assert generate(seed, fam) == generate(seed, fam)
        assert sum(1 for s in generate(seed, fam) if s[0] == "checkpoint") == N_STEPS // 5
    assert generate(101, "cornell_coat") != generate(202, "cornell_coat")
    seqs = all_sequences()
    used = {s[0] for _, steps in seqs.values() for s in steps}
    assert used >= set(OPS), "operations that never occur: %s" % sorted(set(OPS) - used)
    drawn = {s[0] for seed, fam in SEEDS.items() for s in generate(seed, fam)}
    assert drawn >= set(OPS), "operations the random sequences never draw: %s" % sorted(set(OPS) - drawn)
    refused = {s[1] for _, steps in seqs.values() for s in steps if s[0] == "refuse"}
    assert refused == set(REFUSALS)
    found = set()
    for family, steps in seqs.values():
        assert steps[-1][0] == "checkpoint"
        found |= exercised_pairs(prt, family, steps)
    wanted = {(state, creator, call) for state, (creators, table) in LIFETIMES.items() for creator in creators for call in table}
    assert not wanted - found, "pairs of the lifetime table that no sequence exercises with the state there: %s" % sorted(wanted - found)


def test_the_lifetime_table_cites_sentences_of_the_header():
    header = open(os.path.join(ROOT, "include", "prt.h")).read().split("\n")
    for state, (creators, table) in LIFETIMES.items():
        assert state in ALIVE
        for call, (entry, line) in table.items():
            assert entry in ("keeps", "drops", "reallocates") and call in OPS, (state, call)
            text = header[line - 1]
            assert any(w in text for w in LIFETIME_WORDS), "%s / %s cites prt.h:%d, which says nothing of a lifetime: %r" % (state, call, line, text.strip())


def test_the_lifetime_table_is_the_one_in_the_design_document():
    text = open(os.path.join(ROOT, "DESIGN.md")).read()
    assert "What survives what" in text
    section = text.split("What survives what", 1)[1]
    for state, (creators, table) in LIFETIMES.items():
        row = [ln for ln in section.split("\n") if ln.startswith("| " + state + " |")]
        assert len(row) == 1, "DESIGN.md has no row for %r" % state
        for call, (entry, line) in table.items():
            assert "%s %s (%d)" % (call, entry, line) in row[0], "DESIGN.md, %s: no entry `%s %s (%d)`" % (state, call, entry, line)
