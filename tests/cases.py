"""tests/cases.py -- TEST INFRASTRUCTURE: the inputs and the small drivers that several test files share -- scenes and meshes, moved
primitives, skins and morph targets, synthetic denoiser records, the context / render / read-back helpers, the oracle's inputs of its own and
the codegen tests' listing parser.  A plain module (no fixtures, no hooks, no test); it imports no test module.  The yardsticks the cases
are checked against live in tests/mirrors.py.

Caches here are one per process and shared by every file that asks; what they hold is read-only."""
import ctypes as C
import hashlib
import os
import re
import shutil

import numpy as np
import pytest

from conftest import ROOT, variant_camera, variant_config
from mirrors import NODE_T, MotionCaster, _close, _nrm, _point, camera_basis, centre_dirs, mirror_morph, mirror_morph_raw, mirror_pose, mirror_refit
from support import bytes_flat as _bytes, rodrigues as _rodrigues, variant_case

f32 = np.float32
REFIT_FRAME = (48, 32, 24)          # W, H, frames of tests/test_refit.py, test_rebuild.py and the files built on their Case and Teapot
POSE_FRAME = (32, 24, 48)           # ... of tests/test_pose.py, test_morph.py and test_morph_planes.py (the teapot below)
REFIT, REBUILD = 0, 1
T_TEAPOT = 6320


# ---- scenes and meshes ---------------------------------------------------------------------------------------------------------------------------

def deform(vertices, normals, seed):
    """a scale of y plus a twist about y, float32, from a seed (positions and normals turn together)"""
    rng = np.random.default_rng(seed)
    sy, tw = f32(rng.uniform(0.8, 1.25)), f32(rng.uniform(-0.6, 0.6))
    v, n = np.array(vertices, dtype=f32).reshape(-1, 4), np.array(normals, dtype=f32).reshape(-1, 4)
    ang = tw * v[:, 1]
    c, s = np.cos(ang).astype(f32), np.sin(ang).astype(f32)
    for a in (v, n):
        x, z = a[:, 0].copy(), a[:, 2].copy()
        a[:, 0] = c * x + s * z
        a[:, 2] = c * z - s * x
    v[:, 1] = v[:, 1] * sy
    return v, n


class Case:
    """a scene, its buffers as numpy, a deformation and the desc holding (new vertices, new normals, mirror's nodes); W, H, FRAMES: the frame
    the drivers below render it at"""
    W, H, FRAMES = REFIT_FRAME

    def __init__(self, prt, variant, seed=None, desc=None, scene=None, normals_too=True):
        self.scene, self.cfg, self.cam, self.env = variant_case(prt, variant, self.W, self.H, scene=scene)
        self.desc = desc if desc is not None else self.scene.desc
        a = prt.scene_arrays(self.desc)
        self.v0, self.n0, self.pi = a["vertices"].copy(), a["normals"].copy(), a["primitive_indices"].copy()
        self.nodes0 = a["nodes"].view(NODE_T).copy()
        self.prt = prt
        self.set(*(deform(self.v0, self.n0, seed) if seed is not None else (self.v0, self.n0)), normals_too=normals_too)

    def set(self, v, n, normals_too=True):
        self.v, self.n = np.ascontiguousarray(v, dtype=f32), np.ascontiguousarray(n if normals_too else self.n0, dtype=f32)
        self.nodes = mirror_refit(self.nodes0, self.pi, self.v)
        d = self.prt.SceneDesc.from_buffer_copy(bytes(self.desc))
        d.vertices = self.v.ctypes.data_as(C.c_void_p)
        d.normals = self.n.ctypes.data_as(C.c_void_p)
        d.bvh_nodes = self.nodes.ctypes.data_as(C.c_void_p)
        self.new_desc = d
        return self


def _chain_desc(prt, scene, levels):
    """a caller's chain: every inner node has one single-triangle leaf and the rest of the chain; `levels` pairs nested one in the other (no pair
    has two inner children: the traversal stack needs one entry)"""
    nodes = np.zeros(2 * levels + 1, dtype=NODE_T)
    nodes["bounds"] = np.array([-3, 3, -1, 5, -3, 3], dtype=f32)
    for k in range(levels):
        at = 0 if k == 0 else 2 * k
        nodes[at]["first"], nodes[at]["leaf"] = 2 * k + 1, 0
        nodes[2 * k + 1]["first"], nodes[2 * k + 1]["count"], nodes[2 * k + 1]["leaf"] = k, 1, 1
    nodes[2 * levels]["first"], nodes[2 * levels]["count"], nodes[2 * levels]["leaf"] = levels, 1, 1
    desc = prt.SceneDesc.from_buffer_copy(bytes(scene.desc))
    desc.bvh_nodes = nodes.ctypes.data_as(C.c_void_p)
    desc.bvh_node_count = len(nodes)
    return desc, nodes


def _with(prt, desc, v, n, nodes=None, prims=None, T=None):
    """a copy of `desc` holding the given buffers; the arrays are kept alive on the copy"""
    d = prt.SceneDesc.from_buffer_copy(bytes(desc))
    d._keep = [np.ascontiguousarray(v, dtype=f32), np.ascontiguousarray(n, dtype=f32)]
    d.vertices, d.normals = (a.ctypes.data_as(C.c_void_p) for a in d._keep)
    if nodes is not None:
        nodes, prims = np.ascontiguousarray(nodes), np.ascontiguousarray(prims, dtype=np.uint64)
        d._keep += [nodes, prims]
        d.bvh_nodes, d.bvh_node_count, d.primitive_indices = nodes.ctypes.data_as(C.c_void_p), len(nodes), prims.ctypes.data_as(C.c_void_p)
    if T is not None:
        d.triangle_count = T
    return d


def _leaf_root_desc(prt, desc, v, n):
    """the trivial tree: a leaf root that names every triangle"""
    T = len(v) // 3
    nodes = np.zeros(1, dtype=NODE_T)
    nodes["bounds"] = np.array([-1e3, 1e3] * 3, dtype=f32)
    nodes[0]["count"], nodes[0]["leaf"] = T, 1
    return _with(prt, desc, v, n, nodes, np.arange(T, dtype=np.uint64), T=T)


class Teapot:
    """cornell_coat's scene and buffers, and a deformation of it"""
    W, H, FRAMES = REFIT_FRAME

    def __init__(self, prt, seed=11, variant="cornell_coat"):
        self.prt = prt
        self.scene, self.cfg, self.cam, self.env = variant_case(prt, variant, self.W, self.H)
        self.desc = self.scene.desc
        a = prt.scene_arrays(self.desc)
        self.v0, self.n0 = a["vertices"].copy(), a["normals"].copy()
        self.v, self.n = deform(self.v0, self.n0, seed) if seed is not None else (self.v0, self.n0)


def _soup(kind, T):
    rng = np.random.default_rng(1000 + T)
    v = np.zeros((3 * T, 4), dtype=f32)
    n = np.zeros((3 * T, 4), dtype=f32)
    n[:, 1] = 1
    if kind == "random":
        v[:, :3] = rng.uniform(-1, 1, (3 * T, 3)).astype(f32)
    elif kind == "identical":                      # zero extent on all axes: ordered by index alone
        v[:, :3] = np.tile(np.array([[0, 0, 0.5], [1, 0, 0.5], [0, 1, 0.5]], dtype=f32), (T, 1))
    elif kind == "planar":                         # one zero-extent axis (every triangle spans the same z range)
        v[:, :2] = rng.uniform(-1, 1, (3 * T, 2)).astype(f32)
        v[:, 2] = np.tile(np.array([0.25, 0.25, 0.25], dtype=f32), T)
    elif kind == "clusters":                       # centres at the extent's ends: codes 0 and 1023, the clamp
        tri = np.repeat(np.arange(T), 3)
        off = rng.uniform(0, 1e-3, (3 * T, 3)).astype(f32)
        v[:, :3] = np.where((tri % 2 == 0)[:, None], f32(-100.0) + off, f32(100.0) - off)
        v[0:3, :3] = f32(-100.0)                   # (exact ends: degenerate triangles whose centres ARE lo and hi)
        v[3:6, :3] = f32(100.0)
    return v, n


def callers_tree(prt, oracle):
    """a CALLER'S tree, legal for the reference kernel but unlike anything the builder makes: loose boxes (the whole scene), a leaf of 40
    triangles, two sibling leaves that SHARE triangles (ranges 20..59 and 30..99), 100 of the mesh's triangles referenced in all"""
    import ctypes as C
    scene = prt.HostScene("cornell_coat.json")
    node_t = np.dtype([("bounds", "<f4", 6), ("first", "<u4"), ("count", "<u4"), ("leaf", "u1"), ("_p", "u1", 3)])
    nodes = np.zeros(5, dtype=node_t)
    nodes["bounds"] = np.array([-3, 3, -1, 5, -3, 3], dtype=np.float32)
    nodes[0]["first"], nodes[0]["leaf"] = 1, 0                                   # root: children 1, 2
    nodes[1]["first"], nodes[1]["count"], nodes[1]["leaf"] = 0, 40, 1            # a fat leaf
    nodes[2]["first"], nodes[2]["leaf"] = 3, 0                                   # inner: children 3, 4
    nodes[3]["first"], nodes[3]["count"], nodes[3]["leaf"] = 20, 40, 1
    nodes[4]["first"], nodes[4]["count"], nodes[4]["leaf"] = 30, 70, 1
    desc = prt.SceneDesc.from_buffer_copy(bytes(scene.desc))
    desc.bvh_nodes = nodes.ctypes.data_as(C.c_void_p)
    desc.bvh_node_count = len(nodes)
    return scene, desc, nodes


N_RANDOM = 4096
cast_scenes, cast_ray_sets = {}, {}         # the ray-query scenes and ray sets: computed once, shared, never written to


def scene_of(prt, name):
    if name not in cast_scenes:
        sc = prt.HostScene(name + ".json")
        cast_scenes[name] = (sc, variant_config(sc, name))
    return cast_scenes[name]


def random_rays(prt, emu, name, n=N_RANDOM, seed=20):
    """n rays from uniform points in the root box of the scene's tree, uniform unit directions, tmax = 20"""
    key = (name, n, seed)
    if key not in cast_ray_sets:
        sc, cfg = scene_of(prt, name)
        box = emu.root_box(cfg, sc.desc).astype(np.float64)
        rng = np.random.default_rng(seed)
        o = box[0::2] + rng.uniform(0, 1, (n, 3)) * (box[1::2] - box[0::2])
        d = _nrm(rng.normal(size=(n, 3)))
        r = np.zeros((n, 8), dtype=f32)
        r[:, 0:3], r[:, 3], r[:, 4:7] = o, 20.0, d
        r[:, 4:7] = _nrm(r[:, 4:7].astype(np.float64))                 # unit in float32 as well as it can be
        r.setflags(write=False)
        cast_ray_sets[key] = r
    return cast_ray_sets[key]


def _quad_scene(prt, W, H):
    """a quad emitter with slanted edges 5 units ahead of the default camera, its normal cross(e0, e1) pointing away from the camera (hit_quad
    takes rays with dot(n, dir) > 0); black default environment, no OBJ"""
    cam = prt.default_camera(W, H)
    cam.apertureRadius = 0.0
    P, view, up = (np.array(x[:3], dtype=np.float64) for x in (cam.position, cam.view, cam.up))
    view, up = view / np.linalg.norm(view), up / np.linalg.norm(up)
    h = np.cross(view, up); h /= np.linalg.norm(h)
    v = np.cross(h, view); v /= np.linalg.norm(v)
    c = P + 5.0 * view
    e0 = -0.35 * h + 1.0 * v
    e1 = 1.2 * h + 0.3 * v
    q = [float(x) for x in np.concatenate([c, e0, e1])]
    js = ('{"settings":{"MAX_BOUNCES":4,"MAX_DIFF_BOUNCES":4,"MAX_SPEC_BOUNCES":4,"MAX_TRANS_BOUNCES":4,"MAX_SCATTERING_EVENTS":4,'
          '"MARCHING_STEPS":16,"SHADOW_MARCHING_STEPS":16},"scene":{"spheres":[],"quads":[{"vertices":%s,"material":{"color":[3.0,3.0,3.0],"type":0}}]}}'
          % ("[" + ",".join("%.9g" % x for x in q) + "]"))
    q = np.array(q, dtype=np.float32).astype(np.float64)
    return js, cam, q[:3], q[3:6], q[6:9]


RW, RH = 64, 48


class Rendered:
    """a scene, its vertices, two deformations A (seed 21) and B (seed 11) and the caster's motion plane from the uploaded geometry to B at
    RW x RH: computed once per scene, shared, never written to"""
    _cache = {}

    def __new__(cls, prt, scene_json, **orbit):
        key = (scene_json, tuple(sorted(orbit.items())))
        if key not in cls._cache:
            self = super().__new__(cls)
            self.scene = prt.HostScene(scene_json)
            self.cfg = self.scene.config()
            self.cam = prt.orbit_camera(RW, RH, **orbit) if orbit else prt.default_camera(RW, RH)
            self.cam.apertureRadius = 0.0
            a = prt.scene_arrays(self.scene.desc)
            self.v0, self.n0 = a["vertices"].copy(), a["normals"].copy()
            self.vA, self.nA = deform(self.v0, self.n0, 21)
            self.vB, self.nB = deform(self.v0, self.n0, 11)
            self.env = prt.make_sky(64, 32)
            caster = MotionCaster(self.scene, self.cfg, self.vB)
            self.mesh, tri, u, v, self.mid, self.hit, self.t, self.behind_mirror = caster.first_hits(self.cam, RW, RH)
            v0 = np.asarray(self.v0, dtype=np.float64).reshape(-1, 3, 4)[..., :3]
            self.D = np.where(self.mesh[..., None], _point(v0, tri, u, v) - _point(caster.vtx, tri, u, v), 0.0)
            self.diag = float(np.linalg.norm(caster.vtx.reshape(-1, 3).max(0) - caster.vtx.reshape(-1, 3).min(0)))
            for arr in (self.mesh, self.D, self.mid, self.hit, self.t, self.behind_mirror, self.v0, self.n0, self.vA, self.nA, self.vB, self.nB):
                arr.setflags(write=False)
            cls._cache[key] = self
        return cls._cache[key]

    def context(self, prt, motion=True, part=None, pixel_filter=None):
        r = prt.Renderer(self.cfg, device=0)
        r.upload_scene(self.scene)
        if pixel_filter is not None:
            r.set_pixel_filter(*pixel_filter)
        r.upload_envmap(self.env)
        r.set_camera(self.cam)
        if part is None:
            r.resize(RW, RH)
        elif part[0] == "tile":
            r.set_tile(RW, RH, part[1], part[2])
        else:
            r.set_row_blocks(RW, RH, 16, 2, part[1])
        if motion:
            r.set_motion(True)
        return r

    def check(self, plane, what):
        """the plane of a K = 1 guide render after the geometry went from the uploaded one to B, against the caster; returns the largest
        deviation of D over the matching pixels"""
        m, D = plane[..., 3], plane[..., :3].astype(np.float64)
        assert ((m == 0) | (m == 1)).all(), what
        dev = np.abs(D - self.D).max(-1)
        match = ((m > 0) == self.mesh) & (dev <= 1e-3 * self.diag)
        assert (~match).mean() <= 0.005, "%s: %.2f %% of the pixels differ from the caster" % (what, 100 * (~match).mean())
        assert (D[m == 0] == 0).all(), what
        return float(dev[match].max())


# ---- primitives moved in place -------------------------------------------------------------------------------------------------------------------

def meshes_of(desc):
    import prims_api
    n = int(desc.object_count[7])
    if not n:
        return np.zeros(0, dtype=prims_api.MESH_DTYPE)
    return np.frombuffer((C.c_uint8 * (prims_api.MESH_BYTES * n)).from_address(desc.meshes), dtype=prims_api.MESH_DTYPE).copy()


def desc_with(prt, desc, meshes=None, **fields):
    d = prt.SceneDesc.from_buffer_copy(bytes(desc))
    d._keep = [meshes]
    if meshes is not None:
        d.meshes = meshes.ctypes.data
    for k, v in fields.items():
        if isinstance(v, np.ndarray):
            d._keep.append(v)
            v = v.ctypes.data_as(C.c_void_p)
        setattr(d, k, v)
    return d


def move_sphere(m, i, dpos=(0, 0, 0), dr=0.0):
    m["pos"][i, :3] = (m["pos"][i, :3].astype(np.float64) + dpos).astype(f32)
    m["joker"][i, 0] = f32(m["joker"][i, 0] + dr)


def move_sdf(m, i, dpos):
    m["pos"][i, :3] = (m["pos"][i, :3].astype(np.float64) + dpos).astype(f32)


def move_quad(m, i, dpos=(0, 0, 0), axis=(0.3, 1.0, 0.2), ang=0.0, scale=1.0):
    j = m["joker"][i].astype(np.float64)
    j[0:3] += dpos
    for k in (3, 6, 9):
        j[k:k + 3] = _rodrigues(j[k:k + 3], axis, ang)
    j[3:9] *= scale
    j[12] *= scale * scale
    m["joker"][i] = j.astype(f32)


TILT = (0.3, 1.0, 0.2)


# ---- deformer cases: skins and morph targets over the teapot -------------------------------------------------------------------------------------

def bones(n_bones, seed, amount=0.35):
    """n_bones row-major 3x4 matrices float32 [n_bones, 12]: a rotation by up to `amount` rad about a random axis, a scale near 1, a small shift"""
    rng = np.random.default_rng(seed)
    axis = rng.normal(size=(n_bones, 3))
    axis /= np.linalg.norm(axis, axis=1)[:, None]
    ang = rng.uniform(-amount, amount, n_bones)
    K = np.zeros((n_bones, 3, 3))
    K[:, 0, 1], K[:, 0, 2], K[:, 1, 0], K[:, 1, 2], K[:, 2, 0], K[:, 2, 1] = -axis[:, 2], axis[:, 1], axis[:, 2], -axis[:, 0], -axis[:, 1], axis[:, 0]
    R = np.eye(3)[None] + np.sin(ang)[:, None, None] * K + (1 - np.cos(ang))[:, None, None] * (K @ K)
    M = np.zeros((n_bones, 3, 4))
    M[:, :, :3] = R * rng.uniform(0.9, 1.1, n_bones)[:, None, None]
    M[:, :, 3] = rng.uniform(-0.05, 0.05, (n_bones, 3))
    return np.ascontiguousarray(M.reshape(n_bones, 12), dtype=f32)


def identity(n_bones):
    return np.tile(np.array([1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0], dtype=f32), (n_bones, 1))


def influences(corners, n_bones, seed, rigid=False):
    """(index uint16 [corners, 4], weight float32 [corners, 4]): four random influences with positive weights that sum to about 1, or rigid
    parts -- w = (1, 0, 0, 0), part = triangle index mod min(3, n_bones), the three unused indices random"""
    rng = np.random.default_rng(seed)
    index = rng.integers(0, n_bones, (corners, 4)).astype(np.uint16)
    if rigid:
        index[:, 0] = (np.arange(corners) // 3) % min(3, n_bones)
        weight = np.zeros((corners, 4), dtype=f32)
        weight[:, 0] = 1
        return index, weight
    w = rng.uniform(0.05, 1.0, (corners, 4))
    return index, np.ascontiguousarray(w / w.sum(axis=1)[:, None], dtype=f32)


pose_cache = {}


def teapot(prt):
    """cornell_coat through Case at the deformer tests' frame size (POSE_FRAME): rest pose v0, n0"""
    if "teapot" not in pose_cache:
        case = Case(prt, "cornell_coat")
        case.W, case.H, case.FRAMES = POSE_FRAME
        case.cam = variant_camera(prt, "cornell_coat", case.W, case.H)
        assert len(case.v0) == 3 * T_TEAPOT
        pose_cache["teapot"] = case
    return pose_cache["teapot"]


def skin_case(prt, T, n_bones, rigid=False, seed=5):
    """the first T triangles of the teapot with a skin of n_bones and the frame's matrices; the mirror's pose (computed once, shared, read-only).
    65 536 bones: index 65 535 is used once, by the last corner's heaviest influence"""
    key = ("skin", T, n_bones, rigid, seed)
    if key not in pose_cache:
        case = teapot(prt)
        v0, n0 = case.v0[:3 * T].copy(), case.n0[:3 * T].copy()
        index, weight = influences(3 * T, n_bones, seed, rigid)
        if n_bones == 65536:
            index[index == 65535] = 0
            index[-1, int(np.argmax(weight[-1]))] = 65535
            assert (index == 65535).sum() == 1
        M = bones(n_bones, seed + 1)
        want_v, want_n = mirror_pose(v0, n0, index, weight, M)
        for a in (v0, n0, index, weight, M, want_v, want_n):
            a.setflags(write=False)
        assert np.isfinite(want_v).all() and not np.array_equal(want_v[:, :3], v0[:, :3])
        pose_cache[key] = dict(T=T, n_bones=n_bones, v0=v0, n0=n0, index=index, weight=weight, M=M, v=want_v, n=want_n)
    return pose_cache[key]


def _target(rng, corner, normal_deltas=True):
    corner = np.sort(np.asarray(corner, dtype=np.uint32))
    dp = np.zeros((len(corner), 4), dtype=f32)
    dp[:, :3] = rng.uniform(-0.03, 0.03, (len(corner), 3))
    dp[:, 3] = 5.0                                          # (lane 3 is never looked at)
    dn = None
    if normal_deltas:
        dn = np.zeros((len(corner), 4), dtype=f32)
        dn[:, :3] = rng.uniform(-0.3, 0.3, (len(corner), 3))
    return corner, dp, dn


def target_set(corners, n_targets, seed, fraction=0.05):
    """1 target: a dense one.  3 (and 4: the CPU case): random subsets of `fraction` of the corners, one of them without normal deltas, and a
    dense one last.  257: a handful of entries each, corner 0 listed by all of them, the last corner by the last one.  65 536: only the last has
    an entry, on the last corner.  Weights in [-0.5, 1] without zeros, but for 257 targets, where every seventh is a zero of alternating sign"""
    rng = np.random.default_rng(seed)
    if n_targets == 65536:
        targets = [(np.zeros(0, dtype=np.uint32), np.zeros((0, 4), dtype=f32), None)] * 65535 + [_target(rng, [corners - 1])]
    elif n_targets == 257:
        targets = []
        for t in range(257):
            corner = {0, corners - 1} if t == 256 else {0}
            corner |= set(rng.choice(np.arange(1, corners), size=min(4, corners - 1), replace=False).tolist())
            targets.append(_target(rng, sorted(corner), normal_deltas=(t % 5 != 3)))
    else:
        k = max(1, int(round(fraction * corners)))
        targets = [_target(rng, rng.choice(corners, size=k, replace=False), normal_deltas=(t != 1)) for t in range(n_targets - 1)]
        targets.append(_target(rng, np.arange(corners)))
    weights = rng.uniform(0.1, 1.0, n_targets).astype(f32) * np.where(rng.uniform(size=n_targets) < 0.3, f32(-0.5), f32(1))
    if n_targets == 257:
        weights[0::14], weights[7::14] = 0.0, -0.0
    return targets, np.ascontiguousarray(weights, dtype=f32)


morph_cache = {}


def morph_case(prt, T, n_targets, seed=11):
    """the first T triangles of the teapot as the base, a target set and the frame's weights; the mirror's morph (computed once, shared,
    read-only)"""
    key = (T, n_targets, seed)
    if key not in morph_cache:
        case = teapot(prt)
        v0, n0 = case.v0[:3 * T].copy(), case.n0[:3 * T].copy()
        targets, weights = target_set(3 * T, n_targets, seed)
        raw_p, raw_n = mirror_morph_raw(v0, n0, targets, weights)
        want_v, want_n = mirror_morph(v0, n0, targets, weights)
        for a in (v0, n0, weights, raw_p, raw_n, want_v, want_n) + tuple(x for t in targets for x in t if x is not None):
            a.setflags(write=False)
        assert np.isfinite(want_v).all() and not np.array_equal(want_v[:, :3], v0[:, :3])
        morph_cache[key] = dict(T=T, n_targets=n_targets, v0=v0, n0=n0, targets=targets, weights=weights, raw_p=raw_p, raw_n=raw_n, v=want_v, n=want_n)
    return morph_cache[key]


def fused_case(prt, T, rigid):
    """skin_case(T, 4 bones) posed over morph_case(T, 3 targets): the mirror's arrays"""
    key = ("fused", T, rigid)
    if key not in morph_cache:
        s, m = skin_case(prt, T, 4, rigid), morph_case(prt, T, 3)
        v, n = mirror_pose(m["raw_p"], m["raw_n"], s["index"], s["weight"], s["M"])
        v.setflags(write=False), n.setflags(write=False)
        assert np.isfinite(v).all() and not np.array_equal(v, s["v"])
        morph_cache[key] = dict(s=s, m=m, v=v, n=n)
    return morph_cache[key]


def planted():
    """two triangles, five targets.  Corner 0: no target lists it (-0 coordinates).  Corner 1: every target lists it.  Target 1 has no entries.
    Corner 5, the last one: only the last target lists it.  Target 2 holds NaN deltas and is only ever given a zero weight.  Corner 2: deltas
    that cancel the normal to length 0.  Corner 3: denormal deltas.  Corner 4: a delta that overflows under a large weight"""
    nan = np.nan
    v = np.zeros((6, 4), dtype=f32)
    n = np.zeros((6, 4), dtype=f32)
    v[:, :3] = [[-0.0, 2, -0.0], [0.5, -0.25, 4], [1, 1, 1], [0, -0.0, 1e-45], [3, -2, 1], [0.1, 0.2, 0.3]]
    v[:, 3] = 3.0
    n[:, :3] = [[0, 3, 4], [0, 0, 1], [0.5, 0, 0], [1e-30, 0, 0], [1, 0, 0], [0, 0.6, 0.8]]

    def q(rows):
        a = np.zeros((len(rows), 4), dtype=f32)
        a[:, :3] = rows
        return a
    targets = [(np.array([1, 2, 3], dtype=np.uint32), q([[0.25, 0, 0], [0.125, 0, -1], [1e-42, -2e-44, 1e-45]]), q([[0, 1, 0], [-1, 0, 0], [0, 0, 0]])),
               (np.zeros(0, dtype=np.uint32), np.zeros((0, 4), dtype=f32), None),
               (np.array([1, 3, 4], dtype=np.uint32), q([[nan] * 3] * 3), q([[nan] * 3] * 3)),
               (np.array([1, 4], dtype=np.uint32), q([[0, -0.5, 0], [1e38, 0, 0]]), None),
               (np.array([1, 5], dtype=np.uint32), q([[0, 0, 0.75], [1, 1, 1]]), q([[0.5, 0.5, 0], [0, -0.6, -0.8]]))]
    return v, n, targets


# ---- denoiser worlds: synthetic records ----------------------------------------------------------------------------------------------------------

W0, H0 = 37, 29                          # no multiple of 16, wider than one workgroup
T_DEFAULTS = dict(alpha_color=0.2, alpha_moments=0.2, tau_z=0.05, cos_n=0.9, history_cap=32)


def _unit(v):
    return v / np.linalg.norm(v, axis=-1, keepdims=True)


class World:
    """two rectangles in world space, placed by the default camera of a W0 x H0 frame: `back` faces it at distance 10 and fills the middle
    80 % of its view (the rim misses: cov = 0), `card` stands at distance 3.5, tilted, in front of part of it.  Colours and albedos are
    functions of the world point (of 6 d for a ray that misses), so frames of different cameras show the same world."""

    def __init__(self, prt):
        P, M, Hz, Vt = camera_basis(prt.default_camera(W0, H0))
        view, h, v = M - P, _unit(Hz), _unit(Vt)
        tx, ty = np.linalg.norm(Hz), np.linalg.norm(Vt)
        cn = _unit(-view + 0.45 * h + 0.2 * v)
        cu = _unit(np.cross(cn, v))
        self.surfaces = [(P + 10.0 * view, -view, h, v, 8.0 * tx, 8.0 * ty),
                         (P + 3.5 * view + 0.25 * h - 0.1 * v, cn, cu, np.cross(cn, cu), 0.55, 0.45)]

    @staticmethod
    def colour(X):
        base = 0.7 + 0.2 * np.sin(X @ np.array([[0.9, 0.2, -0.5], [0.3, 1.1, 0.4], [-0.6, 0.5, 0.8]]) + np.array([0.3, 1.7, 2.9]))
        checker = 0.3 * (np.floor(2.2 * X).sum(-1) % 2)
        return base + checker[..., None]

    @staticmethod
    def albedo(X):
        return 0.5 + 0.3 * np.sin(X @ np.array([[0.5, -0.3, 0.2], [0.1, 0.6, -0.4], [0.3, 0.2, 0.7]]) + np.array([1.0, 2.0, 0.5]))

    def records(self, cam, W, H, seed, noise=0.05):
        """(records [H, W, 16] float32, surface [H, W]: 0 none, 1 back, 2 card) of camera `cam`; `seed`: the frame's colour noise, alpha and v"""
        rng = np.random.default_rng(1000 + seed)
        P = camera_basis(cam)[0]
        d = centre_dirs(camera_basis(cam), W, H)
        z = np.full((H, W), np.inf)
        nrm, sid = np.zeros((H, W, 3)), np.zeros((H, W), dtype=np.int64)
        for k, (Cc, n, u, v, hu, hv) in enumerate(self.surfaces):
            with np.errstate(divide="ignore", invalid="ignore"):
                t = ((Cc - P) @ n) / (d @ n)
            X = P + d * t[..., None]
            hit = (t > 1e-6) & (t < z) & (np.abs((X - Cc) @ u) <= hu) & (np.abs((X - Cc) @ v) <= hv)
            z = np.where(hit, t, z)
            nrm = np.where(hit[..., None], np.where(((d @ n) < 0)[..., None], n, -n), nrm)        # the normal faces the ray
            sid = np.where(hit, k + 1, sid)
        cov = sid > 0
        X = np.where(cov[..., None], P + d * np.where(cov, z, 0.0)[..., None], 6.0 * d)
        rec = np.zeros((H, W, 16), dtype=np.float32)
        rec[..., 0:3] = self.colour(X) + rng.uniform(-noise, noise, (H, W, 3))
        rec[..., 3] = rng.uniform(0.0, 1.0, (H, W))
        rec[..., 4:7] = self.albedo(X)
        rec[..., 7] = cov
        rec[..., 8:11] = nrm
        rec[..., 11] = np.where(cov, z, 0.0)
        rec[..., 12] = rng.uniform(0.005, 0.1, (H, W))
        rec[..., 13] = 1.0
        return rec, sid


MOVES = [dict(), dict(d_yaw=0.04, d_pitch=0.012), dict(d_yaw=0.10, d_pitch=0.03, d_radius=0.06), dict(d_yaw=0.13, d_pitch=-0.02, d_radius=-0.03),
         dict(d_yaw=0.06, d_pitch=-0.06, d_radius=0.02)]


def _plain_records(W, H, seed):
    """records of a frame too small for a camera: O(1) colours, unit normals, a depth ramp, one uncovered pixel when there is room"""
    rng = np.random.default_rng(seed)
    rec = np.zeros((H, W, 16), dtype=np.float32)
    rec[..., 0:3] = rng.uniform(0.2, 1.5, (H, W, 3))
    rec[..., 3] = rng.uniform(0.0, 1.0, (H, W))
    rec[..., 4:7] = 0.5 + rng.uniform(-0.05, 0.05, (H, W, 3))
    rec[..., 7] = 1.0
    n = np.array([0.1, 0.2, 1.0]) + rng.uniform(-0.03, 0.03, (H, W, 3))
    rec[..., 8:11] = n / np.linalg.norm(n, axis=-1, keepdims=True)
    rec[..., 11] = 3.0 + 0.05 * np.arange(W)[None, :] + 0.03 * np.arange(H)[:, None]
    if W * H > 2:
        rec[H - 1, W - 1, 7:12] = 0.0
    rec[..., 12] = rng.uniform(0.005, 0.1, (H, W))
    rec[..., 13] = 1.0
    return rec


def _synthetic(W, H, seed=5):
    """records [H, W, 16] no render reliably produces: O(1) colours, two planes of depth meeting at a vertical edge, unit normals, an uncovered
    band, one covered pixel with a zero normal, one pixel with a NaN colour.  Returns (records, (y, x) of the NaN pixel)"""
    rng = np.random.default_rng(seed)
    rec = np.zeros((H, W, 16), dtype=np.float32)
    ys, xs = np.mgrid[0:H, 0:W]
    left = xs < W // 2
    rec[..., 0:3] = rng.uniform(0.2, 1.5, (H, W, 3))
    rec[..., 3] = rng.uniform(0.0, 1.0, (H, W))
    rec[..., 4:7] = np.where(left[..., None], [0.7, 0.6, 0.5], [0.2, 0.5, 0.8]) + rng.uniform(-0.02, 0.02, (H, W, 3))
    rec[..., 7] = 1.0
    nl, nr = np.array([0.1, 0.2, 1.0]), np.array([-0.6, 0.1, 0.8])
    rec[..., 8:11] = np.where(left[..., None], nl / np.linalg.norm(nl), nr / np.linalg.norm(nr))
    rec[..., 11] = np.where(left, 3.0 + 0.02 * xs + 0.01 * ys, 5.0 - 0.03 * xs + 0.015 * ys)
    rec[10:13, :, 4:7] = [0.3, 0.4, 0.6]                 # the band: no hit -- the environment's albedo, no normal, no depth
    rec[10:13, :, 7:12] = 0.0
    rec[20, 7, 8:11] = 0.0                               # covered, but the normals summed to zero
    nan_at = (25, 30)
    rec[25, 30, 0] = np.nan
    rec[..., 12] = rng.uniform(0.005, 0.1, (H, W))
    rec[..., 13] = 1.0
    return rec, nan_at


# ---- shared drivers: contexts, renders, read-backs -----------------------------------------------------------------------------------------------

def pose_context(prt, s, leaf_root=True):
    """a context over the first T triangles of the teapot (rest pose) under a leaf root, or over the whole teapot under its own tree"""
    case = teapot(prt)
    desc = _leaf_root_desc(prt, case.desc, s["v0"], s["n0"]) if leaf_root else case.desc
    assert leaf_root or s["T"] == T_TEAPOT
    r = prt.Renderer(case.cfg, device=0)
    r.upload_scene(desc)
    r.set_camera(case.cam)
    r.resize(case.W, case.H)
    return r


def _skin(r, s, normals=True):
    r.set_skin(s["v0"], s["n0"] if normals else None, s["index"], s["weight"], s["n_bones"])


def pose_scene(r):
    nodes, prims = r.read_bvh()
    return {"bounds": r.read_bvh_bounds(), "nodes": nodes, "prims": prims, "normals": r.read_normals()}


def _everything(prt, r):
    """pose_scene plus the state and the framebuffer of a render of the teapot's FRAMES frames"""
    out = pose_scene(r)
    r.reset()
    r.render_frames(prt.seed_pairs(teapot(prt).FRAMES))
    out["state"], out["framebuffer"] = r.read_state(), r.read_framebuffer()
    return out


def _assert_equal(got, want, what):
    """every array of `want` has its shape and its bytes in `got`"""
    for k in want:
        assert got[k].shape == want[k].shape, "%s: %s has shape %s, expected %s" % (what, k, got[k].shape, want[k].shape)
        bad = np.nonzero(_bytes(got[k]) != _bytes(want[k]))[0]
        assert bad.size == 0, "%s: %s differs in %d of %d bytes, first at byte %d" % (what, k, bad.size, _bytes(want[k]).size, bad[0])


def _refused(prt, call, code=None):
    with pytest.raises(prt.PrtError) as e:
        call()
    assert e.value.code == (prt.PRT_ERR_INVALID_ARGUMENT if code is None else code), e.value
    return e.value


_refit_oracle_cache = {}


def refit_oracle_render(oracle, case, key):
    """the oracle's render of the case's new desc (computed once per key, shared, never written to)"""
    if key not in _refit_oracle_cache:
        st, img = oracle.Restatement().render(case.cfg, case.new_desc, case.cam, case.W, case.H, case.prt.seed_pairs(case.FRAMES), env=case.env, threads=8)
        st.setflags(write=False)
        img.setflags(write=False)
        _refit_oracle_cache[key] = (st, img)
    return _refit_oracle_cache[key]


def refit_context(case, desc=None):
    r = case.prt.Renderer(case.cfg, device=0)
    r.upload_scene(desc if desc is not None else case.desc)
    if case.env is not None:
        r.upload_envmap(case.env)
    r.set_camera(case.cam)
    r.resize(case.W, case.H)
    return r


def refit_render(case, r):
    r.reset()
    r.render_frames(case.prt.seed_pairs(case.FRAMES))
    return r.read_state(), r.read_framebuffer()


def denoise_setup(prt, scene_json, W, H, pinhole=True, env=False):
    scene = prt.HostScene(scene_json)
    cfg = scene.config()
    cam = prt.default_camera(W, H)
    if pinhole:
        cam.apertureRadius = 0.0
    r = prt.Renderer(cfg, device=0)
    r.upload_scene(scene)
    if env:
        r.upload_envmap(prt.make_sky(64, 32))
    r.set_camera(cam)
    r.resize(W, H)
    return scene, cfg, cam, r


def filter_setup(prt, scene_json, W, H, pinhole=False, env=False, cfg_edit=None, text=False):
    scene = prt.HostScene(scene_json, text=text)
    cfg = scene.config()
    if cfg_edit:
        cfg_edit(cfg)
    cam = prt.default_camera(W, H)
    if pinhole:
        cam.apertureRadius = 0.0
    r = prt.Renderer(cfg, device=0)
    r.upload_scene(scene)
    if env:
        r.upload_envmap(prt.make_sky(64, 32))
    r.set_camera(cam)
    r.resize(W, H)
    return scene, cfg, cam, r


def _torch():
    import torch
    return torch


def _export(r):
    """the records of r's frame part: a [rows, width, 16] tensor on cuda:0"""
    torch = _torch()
    t = torch.full((r.rows, r.width, 16), 7.0, dtype=torch.float32, device="cuda:0")
    torch.cuda.synchronize()
    r.export_denoise_inputs(t)
    return t


def _cmp(label, k, what, got, ref, scale, mask, worst):
    got, ref = np.asarray(got, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    if got.ndim == 3:
        scale, mask = scale[..., None], np.broadcast_to(mask[..., None], got.shape)
    if mask.any():
        worst[what] = max(worst.get(what, 0.0), float((np.abs(got - ref) / (1e-4 * np.maximum(scale, 1e-6) * np.ones_like(got)))[mask].max()))
    bad = mask & ~_close(got, ref, scale, rel=1e-4)
    assert not bad.any(), "%s, call %s: %s is more than 1e-4 of its scale from the mirror in %d entries, first at %s" % (
        label, k, what, int(bad.sum()), np.argwhere(bad)[:4].tolist())


# ---- the oracle's inputs of its own: what tests/test_oracle.py checks and tests/golden/make_ref_checks.py generates for --------------------------

EQUALS_SIZE, EQUALS_FRAMES, EQUALS_CAMERA = (45, 27), 70, (-0.3, 0.15, -0.1)      # (d_yaw, d_pitch, d_radius) of the orbit camera
DRAGON_SIZE, DRAGON_FRAMES = (40, 24), 40
NAN_SLABS_SIZE, NAN_SLABS_FRAMES = (33, 21), 60
LIBM_SIZE, LIBM_FRAMES = 48, 768


def _digest(bits):
    bits = np.ascontiguousarray(bits)
    return hashlib.sha256(("%s %s " % (bits.dtype.str, bits.shape)).encode() + bits.tobytes()).hexdigest()


def output_digests(oracle, state, img):
    """SHA-256 of exactly the bits oracle.state_fields_equal (per field) and oracle.images_equal compare"""
    fields = {}
    for f in oracle.STATE_FIELDS:
        x = state[f]
        if f in ("origin", "dir", "mask"):
            x = x[..., :3]
        fields[f] = _digest(oracle.float_bits(x) if x.dtype.kind == "f" else x)
    return {"state": fields, "image": _digest(oracle.float_bits(img))}


def equals_inputs(prt, variant):
    """different size / frame count / camera than the goldens"""
    W, H = EQUALS_SIZE
    scene, cfg, _, env = variant_case(prt, variant, W, H)
    d_yaw, d_pitch, d_radius = EQUALS_CAMERA
    return scene, cfg, prt.orbit_camera(W, H, d_yaw=d_yaw, d_pitch=d_pitch, d_radius=d_radius), env, prt.seed_pairs(EQUALS_FRAMES)


def dragon_inputs(prt):
    prt.ensure_dragon_standin()
    scene = prt.HostScene("cornell_dragon.json")
    return scene, scene.config(), prt.default_camera(*DRAGON_SIZE), prt.seed_pairs(DRAGON_FRAMES)


def nan_slabs_inputs(prt):
    W, H = NAN_SLABS_SIZE
    scene, cfg, _, env = variant_case(prt, "cornell_coat", W, H)
    return scene, cfg, prt.orbit_camera(W, H, d_aperture=-1.0), env, prt.seed_pairs(NAN_SLABS_FRAMES)   # apertureRadius clamps to 0: pinhole


def libm_inputs(prt, std):
    scene, cfg, _, env = variant_case(prt, std, LIBM_SIZE, LIBM_SIZE)
    return scene, cfg, prt.default_camera(LIBM_SIZE, LIBM_SIZE), env, prt.seed_pairs(LIBM_FRAMES)


LIBM_CASES = [("cornell_diffuse", "cornell_diffuse_libm", False, 0), ("cornell_roughcond", "cornell_roughcond_libm", True, 0),
              ("cornell_media_hg", "cornell_media_hg_libm", True, 1)]


# ---- code generation: the headline kernel's listing ----------------------------------------------------------------------------------------------

HIP = os.path.join(ROOT, "photorealistic-rendering-using-opencl_amd", "csrc", "hip")
HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
HEADLINE = "_ZN3prt13render_kernelILj3ELb0ELi6ELb0EEE"        # render_kernel<3, false, 6, false>


def kernel_lines(text, symbol=HEADLINE):
    lines = text.split("\n")
    start = next(i for i, l in enumerate(lines) if l.startswith(symbol) and ":" in l)
    end = next(i for i in range(start + 1, len(lines)) if lines[i].startswith(".Lfunc_end"))
    return [l for l in lines[start:end] if not re.match(r"\s*(;|\.loc|\.file|\.cfi|\.Ltmp)", l)]


def frame_loop(lines):
    """the longest backward-branch span of the kernel"""
    labels = {}
    for i, l in enumerate(lines):
        m = re.match(r"^(\.LBB\d+_\d+):", l)
        if m:
            labels[m.group(1)] = i
    best = (0, 0)
    for i, l in enumerate(lines):
        m = re.search(r"\ss_c?branch\S*\s+(\.LBB\d+_\d+)", l)
        if m and labels.get(m.group(1), i) < i and i - labels[m.group(1)] > best[1] - best[0]:
            best = (labels[m.group(1)], i)
    assert best[1] > best[0], "no loop in the kernel"
    return lines[best[0]:best[1] + 1]
