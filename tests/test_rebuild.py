"""prt_rebuild_bvh: new vertices into the uploaded scene and a new Morton-order tree over all T triangles, built on the device (include/prt.h;
csrc/hip/pt_build.h / .hip), and prt_read_bvh.

`mirror_build` (tests/mirrors.py) restates rules 1 - 8 of prt.h in numpy and Python ints (the integer trie on the sorted keys, boxes by mirror_refit);
pack_scene of the mirror's tree under PRT_PAIR_ORDER=bfs is what every buffer and table must equal, byte for byte.  Every comparison here is
equality of bytes; the one exception is the motion plane, held to what tests/test_motion.py's caster check allows.

CPU tests run the kernels' bodies on the host (tests/emu/build_emu.cpp); GPU tests run the library against oracle/pt_oracle.c."""
import os

import numpy as np
import pytest

from conftest import PKG_NAME, ROOT
from cases import callers_tree, Case, deform, _leaf_root_desc, refit_oracle_render as refit_oracle, Rendered, _soup, Teapot, _with
from mirrors import D_BOUND, DEFAULT_LEAF, mirror_build, mirror_keys, mirror_refit
from support import assert_api, assert_same_render as _assert_same, bytes_flat as _bytes


W, H, FRAMES = Teapot.W, Teapot.H, Teapot.FRAMES
f32 = np.float32
NEW_API = ("prt_rebuild_bvh", "prt_rebuild_bvh_device", "prt_read_bvh")


def test_api_is_declared_exported_and_bound(prt):
    assert_api(NEW_API, prt)
    assert callable(prt.Renderer.rebuild_bvh) and callable(prt.Renderer.read_bvh)
    assert "hip/pt_build.hip" in open(os.path.join(ROOT, PKG_NAME, "build.py")).read()


@pytest.fixture(scope="module")
def build(prt, monkeypatch_module):
    import build_api
    build_api.lib()
    return build_api


@pytest.fixture(scope="module")
def monkeypatch_module():
    """a rebuilt tree is breadth-first: pack_scene of the mirror's tree is asked for that order whatever its size"""
    mp = pytest.MonkeyPatch()
    mp.setenv("PRT_PAIR_ORDER", "bfs")
    yield mp
    mp.undo()


# ---- against the mirror (tests/mirrors.py) -------------------------------------------------------------------------------------------------

_TABLES = ("pairs", "tri_geom", "tri_nrm", "root", "slot_vtx", "level_pairs", "level_first", "node_box", "scalars")


def _assert_tables_equal(got, want, what):
    for k in _TABLES:
        assert got[k].shape == want[k].shape and np.array_equal(_bytes(got[k]), _bytes(want[k])), "%s: %s differs" % (what, k)


def _check_against_the_mirror(prt, build, p, cfg, desc, v, n, max_leaf, what):
    """p (a build_api.Packed, rebuilt with (v, n, max_leaf)) against the mirror and against pack_scene of the mirror's tree"""
    nodes, prims, levels, stack_levels = mirror_build(v, max_leaf if max_leaf else DEFAULT_LEAF)
    got_nodes, got_prims = p.read_bvh()
    assert np.array_equal(got_prims, prims), what + ": primitive_indices differ from the mirror"
    assert got_nodes.shape == nodes.shape and np.array_equal(_bytes(got_nodes), _bytes(nodes)), what + ": nodes differ from the mirror"
    assert (p.n_levels, p.stack_levels) == (levels, stack_levels), what
    want = build.Packed(cfg, _with(prt, desc, v, n, nodes, prims, T=len(prims)))
    _assert_tables_equal(p.get(), want.get(), what)
    return nodes, prims


# ---- CPU: the kernels' bodies on the host ----------------------------------------------------------------------------------------------------

PROTOTYPE = {1: (6319, 20, 18), 4: (2168, 17, 16), 16: (613, 14, 14)}      # max_leaf -> (pairs, levels, stack levels) of the undeformed teapot


@pytest.mark.parametrize("max_leaf", [1, 4, 16])
def test_teapot_equals_the_mirror(prt, build, max_leaf):
    tp = Teapot(prt)
    p = build.Packed(tp.cfg, tp.desc)
    assert p.rebuild(tp.v, tp.n, max_leaf) == 0
    _check_against_the_mirror(prt, build, p, tp.cfg, tp.desc, tp.v, tp.n, max_leaf, "teapot max_leaf %d" % max_leaf)
    assert p.n_slots == 6320 and p.root_is_leaf == 0
    # the undeformed teapot: the shape the rules were prototyped with
    assert p.rebuild(tp.v0, tp.n0, max_leaf) == 0
    assert (p.n_pairs, p.n_levels, p.stack_levels) == PROTOTYPE[max_leaf]
    _check_against_the_mirror(prt, build, p, tp.cfg, tp.desc, tp.v0, tp.n0, max_leaf, "undeformed teapot max_leaf %d" % max_leaf)


def test_max_leaf_zero_is_the_documented_default(prt, build):
    assert ("0 = the library's default (%d)" % DEFAULT_LEAF) in open(os.path.join(ROOT, "include", "prt.h")).read()
    tp = Teapot(prt)
    p, q = build.Packed(tp.cfg, tp.desc), build.Packed(tp.cfg, tp.desc)
    assert p.rebuild(tp.v, tp.n, 0) == 0 and q.rebuild(tp.v, tp.n, DEFAULT_LEAF) == 0
    _assert_tables_equal(p.get(), q.get(), "max_leaf 0")


@pytest.mark.parametrize("max_leaf", [1, 4])
def test_two_triangle_mesh(prt, build, max_leaf):
    tp = Teapot(prt, seed=7, variant="cornell_edge")
    p = build.Packed(tp.cfg, tp.desc)
    assert p.n_tris == 2
    assert p.rebuild(tp.v, tp.n, max_leaf) == 0
    _check_against_the_mirror(prt, build, p, tp.cfg, tp.desc, tp.v, tp.n, max_leaf, "cornell_edge max_leaf %d" % max_leaf)
    if max_leaf == 1:
        assert (p.n_pairs, p.root_is_leaf, p.n_levels, p.stack_levels) == (1, 0, 1, 1), "one pair of two leaves"
        assert np.array_equal(p.get()["pairs"]["meta"], np.array([[0, 1, 1, 1]], dtype=np.uint32))
    else:
        assert (p.n_pairs, p.root_is_leaf, p.root_leaf_first, p.root_leaf_count) == (0, 1, 0, 2), "a leaf root"


SOUPS = [("random", 1, 4), ("random", 4, 4), ("random", 5, 4), ("random", 1, 1), ("random", 2, 1), ("random", 64, 64), ("random", 65, 64),
         ("random", 257, 1), ("random", 257, 4), ("identical", 5, 1), ("identical", 5, 2), ("planar", 40, 2), ("clusters", 24, 1), ("clusters", 24, 4)]


@pytest.mark.parametrize("kind,T,max_leaf", SOUPS)
def test_soups_under_a_leaf_root_upload(prt, build, kind, T, max_leaf):
    tp = Teapot(prt, seed=None)
    v, n = _soup(kind, T)
    desc = _leaf_root_desc(prt, tp.desc, v, n)
    p = build.Packed(tp.cfg, desc)
    assert (p.root_is_leaf, p.n_slots) == (1, T)
    assert p.rebuild(v, None, max_leaf) == 0       # (normals None: carried from the leaf root's slots)
    what = "%s soup of %d, max_leaf %d" % (kind, T, max_leaf)
    nodes, prims = _check_against_the_mirror(prt, build, p, tp.cfg, desc, v, n, max_leaf, what)
    assert sorted(prims.tolist()) == list(range(T)), what + ": every triangle once"
    assert p.root_is_leaf == (1 if T <= max_leaf else 0)
    keys, q = mirror_keys(v)
    if kind == "identical":
        assert (q == 0).all() and [k & 0xFFFFFFFF for k in keys] == list(range(T)), "zero extent: ordered by index alone"
    if kind == "planar":
        assert (q[:, 2] == 0).all() and q[:, 0].max() == 1023
    if kind == "clusters":
        assert set(q.reshape(-1).tolist()) >= {0, 1023} and (q[3] == 1023).all() and (q[0] == 0).all(), "the clamp"


def test_emulator_on_a_rebuilt_scene_equals_the_oracle(prt, oracle, build):
    """the rebuilt tables ARE pack_scene's of the read-back tree (checked table by table); the render emulator packs that tree and runs the
    device's traversal code over it"""
    import emu_api
    tp = Teapot(prt)
    p = build.Packed(tp.cfg, tp.desc)
    assert p.rebuild(tp.v, tp.n, 4) == 0
    nodes, prims = p.read_bvh()
    desc = _with(prt, tp.desc, tp.v, tp.n, nodes, prims)
    _assert_tables_equal(p.get(), build.Packed(tp.cfg, desc).get(), "read-back tree")
    w, h, frames = 24, 16, 12
    cam, seeds = prt.default_camera(w, h), prt.seed_pairs(frames)
    ostate, oimg = oracle.Restatement().render(tp.cfg, desc, cam, w, h, seeds, threads=4)
    state, img = emu_api.render(oracle.PATH_STATE_DTYPE, tp.cfg, desc, cam, w, h, seeds)
    assert not oracle.state_fields_equal(ostate, state.view(oracle.PATH_STATE_DTYPE)) and oracle.images_equal(oimg, img)


def test_update_after_a_rebuild_refits_the_new_topology(prt, build):
    tp = Teapot(prt)
    p = build.Packed(tp.cfg, tp.desc)
    assert p.rebuild(tp.v, tp.n, 2) == 0
    nodes, prims = p.read_bvh()
    v2, n2 = deform(tp.v0, tp.n0, 21)
    assert p.update(v2, n2) == 0
    want_nodes = mirror_refit(nodes, prims, v2)
    got_nodes, got_prims = p.read_bvh()
    assert np.array_equal(got_prims, prims) and np.array_equal(_bytes(got_nodes), _bytes(want_nodes))
    _assert_tables_equal(p.get(), build.Packed(tp.cfg, _with(prt, tp.desc, v2, n2, want_nodes, prims)).get(), "rebuild then update")


def test_the_old_tree_does_not_matter(prt, oracle, build):
    scene, cdesc, keep = callers_tree(prt, oracle)
    tp = Teapot(prt)
    a, b = build.Packed(tp.cfg, cdesc), build.Packed(tp.cfg, tp.desc)
    assert a.n_slots == 150 and b.n_slots == 6320
    before = a.get()
    assert a.rebuild(tp.v, None, 4) == 2, "normals None: no normal record for the unreferenced triangles"
    again = a.get()
    assert all(np.array_equal(_bytes(again[k]), _bytes(before[k])) for k in before), "a refusal wrote something"
    assert a.rebuild(tp.v, tp.n, 4) == 0 and b.rebuild(tp.v, tp.n, 4) == 0
    _assert_tables_equal(a.get(), b.get(), "caller's tree against the builder's")
    assert a.n_slots == 6320


def test_refusals_leave_every_buffer_untouched(prt, build):
    tp = Teapot(prt)
    p = build.Packed(tp.cfg, tp.desc)
    p.set_motion(True)
    assert p.update(tp.v, tp.n) == 0               # (a snapshot is pending)
    before = p.get()
    bad = tp.v.copy()
    bad[len(bad) // 2, 1] = np.inf
    assert p.rebuild(bad, tp.n, 4) == 1
    assert p.rebuild(tp.v, tp.n, 65) == 3
    after = p.get()
    assert all(np.array_equal(_bytes(after[k]), _bytes(before[k])) for k in before)
    assert p.snap_valid == 1


def test_normals_none_carries_trinrm_to_the_new_slots(prt, build):
    tp = Teapot(prt)
    p, q = build.Packed(tp.cfg, tp.desc), build.Packed(tp.cfg, tp.desc)
    assert p.rebuild(tp.v, None, 4) == 0 and q.rebuild(tp.v, tp.n0, 4) == 0
    _assert_tables_equal(p.get(), q.get(), "normals None")
    # ... and again from the rebuilt tree
    v2, _ = deform(tp.v0, tp.n0, 21)
    assert p.rebuild(v2, None, 1) == 0 and q.rebuild(v2, tp.n0, 1) == 0
    _assert_tables_equal(p.get(), q.get(), "normals None, from a rebuilt tree")


def _records_under(build, tp, prt, desc_tree, vertices):
    """TriGeom of `vertices` in the slot order of the tree (nodes, prims)"""
    nodes, prims = desc_tree
    return build.Packed(tp.cfg, _with(prt, tp.desc, vertices, tp.n0, nodes, prims)).get()["tri_geom"]


@pytest.mark.parametrize("pending", [True, False])
def test_motion_snapshot_moves_to_the_new_slot_order(prt, build, pending):
    tp = Teapot(prt)
    vA, nA = deform(tp.v0, tp.n0, 21)
    p = build.Packed(tp.cfg, tp.desc)
    p.set_motion(True)
    if pending:
        assert p.update(vA, nA) == 0               # snapshot: the records of v0; then the geometry is A
        old = tp.v0
    else:
        assert p.update(vA, nA) == 0
        p.consume_snapshot()                       # (a guide render): the geometry is A, nothing pending
        old = vA
    assert p.snap_valid == (1 if pending else 0)
    assert p.rebuild(tp.v, tp.n, 4) == 0
    assert p.snap_valid == 1 and p.n_prev == 6320
    assert np.array_equal(p.get()["prev"], _records_under(build, tp, prt, p.read_bvh(), old)), "the snapshot is not the old vertices under the new tree"
    # a second rebuild before the next guide render keeps measuring from `old`
    assert p.rebuild(vA, nA, 2) == 0
    assert np.array_equal(p.get()["prev"], _records_under(build, tp, prt, p.read_bvh(), old))


def test_motion_snapshot_of_triangles_the_old_tree_did_not_hold(prt, oracle, build):
    scene, cdesc, keep = callers_tree(prt, oracle)
    tp = Teapot(prt)
    p = build.Packed(tp.cfg, cdesc)
    p.set_motion(True)
    assert p.rebuild(tp.v, tp.n, 4) == 0
    nodes, prims = p.read_bvh()
    pi = prt.scene_arrays(tp.desc)["primitive_indices"]
    held = np.isin(prims, pi[:100])                # callers_tree references positions 0 .. 99 of the builder's primitive_indices
    prev = p.get()["prev"]
    assert held.sum() == 100
    assert np.array_equal(prev[held], _records_under(build, tp, prt, (nodes, prims), tp.v0)[held]), "a held triangle: its old record"
    assert np.array_equal(prev[~held], p.get()["tri_geom"][~held]), "an unreferenced triangle: its new record (no motion)"


# ---- GPU --------------------------------------------------------------------------------------------------------------------------------------

_oracle_cache = {}


def _oracle_render(oracle, tp, desc, key):
    if key not in _oracle_cache:
        st, img = oracle.Restatement().render(tp.cfg, desc, tp.cam, W, H, tp.prt.seed_pairs(FRAMES), env=tp.env, threads=8)
        st.setflags(write=False)
        img.setflags(write=False)
        _oracle_cache[key] = (st, img)
    return _oracle_cache[key]


def _context(tp, desc=None):
    r = tp.prt.Renderer(tp.cfg, device=0)
    r.upload_scene(desc if desc is not None else tp.desc)
    if tp.env is not None:
        r.upload_envmap(tp.env)
    r.set_camera(tp.cam)
    r.resize(W, H)
    return r


def _render(tp, r):
    r.reset()
    r.render_frames(tp.prt.seed_pairs(FRAMES))
    return r.read_state(), r.read_framebuffer()


_mirror_cache = {}


def _mirror(v, max_leaf, key):
    if key not in _mirror_cache:
        _mirror_cache[key] = mirror_build(v, max_leaf)[:2]
    return _mirror_cache[key]


def _rebuild_render_check(oracle, tp, v, n, max_leaf, key, device=False, r=None):
    """rebuild, then: read_bvh against the mirror, the render against the oracle on it, read_bvh_bounds against the mirror's boxes"""
    own = r is None
    r = r or _context(tp)
    if device:
        import torch
        r.rebuild_bvh(torch.from_numpy(v).cuda(), torch.from_numpy(n).cuda(), max_leaf)
    else:
        r.rebuild_bvh(v, n, max_leaf)
    nodes, prims = r.read_bvh()
    want_nodes, want_prims = _mirror(v, max_leaf if max_leaf else DEFAULT_LEAF, key)
    assert np.array_equal(prims, want_prims), key + ": primitive_indices differ from the mirror"
    assert nodes.shape == want_nodes.shape and np.array_equal(_bytes(nodes), _bytes(want_nodes)), key + ": read_bvh differs from the mirror"
    state, img = _render(tp, r)
    bounds = r.read_bvh_bounds()
    assert np.array_equal(_bytes(bounds), _bytes(want_nodes["bounds"])), key + ": read_bvh_bounds differs from the mirror"
    _assert_same(oracle, *_oracle_render(oracle, tp, _with(tp.prt, tp.desc, v, n, want_nodes, want_prims, T=len(want_prims)), key), state, img, key)
    if own:
        r.close()
    return state, img


@pytest.mark.gpu
@pytest.mark.parametrize("device", [False, True])
def test_render_after_a_rebuild_matches_the_oracle(prt, oracle, device):
    tp = Teapot(prt)
    r = _context(tp)
    _render(tp, r)
    variant = r.kernel_variant()
    _rebuild_render_check(oracle, tp, tp.v, tp.n, 4, "teapot seed 11 leaf 4", device=device, r=r)
    assert r.kernel_variant() == variant
    r.close()


@pytest.mark.gpu
def test_fresh_upload_of_the_read_back_tree_renders_the_same(prt, oracle):
    tp = Teapot(prt)
    r = _context(tp)
    r.rebuild_bvh(tp.v, tp.n, 2)
    nodes, prims = r.read_bvh()
    state, img = _render(tp, r)
    seeds = prt.seed_pairs(2 * max(tp.cfg.max_bounces, 8) + 64)
    r.reset()
    r.render_spp(1, seeds)
    spp_state, spp_img = r.read_state(), r.read_framebuffer()
    r.close()
    f = _context(tp, _with(prt, tp.desc, tp.v, tp.n, nodes, prims))
    fstate, fimg = _render(tp, f)
    _assert_same(oracle, fstate, fimg, state, img, "fresh upload of the read-back tree")
    f.reset()
    f.render_spp(1, seeds)
    _assert_same(oracle, f.read_state(), f.read_framebuffer(), spp_state, spp_img, "one render_spp after a rebuild")
    fn, fp = f.read_bvh()
    f.close()
    assert np.array_equal(_bytes(fn), _bytes(nodes)) and np.array_equal(fp, prims), "an uploaded tree reads back as uploaded"


@pytest.mark.gpu
def test_update_update_rebuild_update(prt, oracle):
    a, b = Case(prt, "cornell_coat", seed=21), Case(prt, "cornell_coat", seed=11)
    tp = Teapot(prt)
    r = _context(tp)
    r.update_vertices(a.v, a.n)
    _assert_same(oracle, *refit_oracle(oracle, a, "coat seed 21"), *_render(tp, r), "update A")
    r.update_vertices(b.v, b.n)
    _assert_same(oracle, *refit_oracle(oracle, b, "coat seed 11"), *_render(tp, r), "update B")
    _rebuild_render_check(oracle, tp, a.v, a.n, 4, "teapot seed 21 leaf 4", r=r)
    nodes, prims = r.read_bvh()
    r.update_vertices(b.v, b.n)
    want = mirror_refit(nodes, prims, b.v)
    got, _ = r.read_bvh()
    assert np.array_equal(_bytes(got), _bytes(want)), "an update after a rebuild refits the new topology"
    state, img = _render(tp, r)
    r.close()
    _assert_same(oracle, *_oracle_render(oracle, tp, _with(prt, tp.desc, b.v, b.n, want, prims), "seed 11 on seed 21's tree"), state, img, "update after rebuild")


@pytest.mark.gpu
@pytest.mark.parametrize("T,max_leaf", [(3, 4), (257, 4), (257, 1)])
def test_soup_through_a_leaf_root_upload(prt, oracle, T, max_leaf):
    tp = Teapot(prt, seed=None)
    v, n = _soup("random", T)
    v[:, :3] = v[:, :3] * f32(1.5) + np.array([0, 1.5, 0], dtype=f32)        # (into the box, in front of the camera)
    tp.desc = _leaf_root_desc(prt, tp.desc, v, n)
    r = _context(tp)
    assert r.read_bvh()[0]["leaf"][0] == 1
    _rebuild_render_check(oracle, tp, v, n, max_leaf, "soup %d leaf %d" % (T, max_leaf), r=r)
    nodes, _ = r.read_bvh()
    r.close()
    assert bool(nodes[0]["leaf"]) == (T <= max_leaf)


@pytest.mark.gpu
def test_refusals_leave_the_scene_as_it_was(prt, oracle):
    tp = Teapot(prt)
    r = prt.Renderer(tp.cfg, device=0)
    with pytest.raises(prt.PrtError) as e:
        r.rebuild_bvh(tp.v, tp.n)
    assert e.value.code == prt.PRT_ERR_NOT_READY
    with pytest.raises(prt.PrtError) as e:
        r.read_bvh()
    assert e.value.code == prt.PRT_ERR_NOT_READY
    r.close()
    r = _context(tp)
    r.rebuild_bvh(tp.v, tp.n, 4)
    nodes0, prims0 = r.read_bvh()
    state0, img0 = _render(tp, r)
    bad = tp.v.copy()
    bad[len(bad) // 2, 1] = np.nan
    import torch
    for what, call in (("a NaN vertex, host", lambda: r.rebuild_bvh(bad, tp.n, 2)),
                       ("a NaN vertex, device", lambda: r.rebuild_bvh(torch.from_numpy(bad).cuda(), None, 2)),
                       ("max_leaf 65", lambda: r.rebuild_bvh(tp.v0, tp.n0, 65)),
                       ("a misaligned pointer", lambda: r.rebuild_bvh(torch.from_numpy(tp.v0).cuda().data_ptr() + 4, None, 2))):
        with pytest.raises(prt.PrtError) as e:
            call()
        assert e.value.code == prt.PRT_ERR_INVALID_ARGUMENT, what
        nodes, prims = r.read_bvh()
        assert np.array_equal(_bytes(nodes), _bytes(nodes0)) and np.array_equal(prims, prims0), what
        _assert_same(oracle, state0, img0, *_render(tp, r), "after a refused rebuild (%s)" % what)
    assert r.lib.prt_rebuild_bvh(r.ctx, None, None, 4) == prt.PRT_ERR_INVALID_ARGUMENT
    r.close()
    # a caller's tree that references 100 of T triangles: normals None is refused, with normals it comes back with T
    scene, cdesc, keep = callers_tree(prt, oracle)
    r = _context(tp, cdesc)
    state0, img0 = _render(tp, r)
    with pytest.raises(prt.PrtError) as e:
        r.rebuild_bvh(tp.v, None, 4)
    assert e.value.code == prt.PRT_ERR_INVALID_ARGUMENT
    _assert_same(oracle, state0, img0, *_render(tp, r), "after the refused rebuild of the caller's tree")
    _rebuild_render_check(oracle, tp, tp.v, tp.n, 4, "teapot seed 11 leaf 4", r=r)
    r.close()


@pytest.mark.gpu
def test_lifetime(prt, oracle):
    tp = Teapot(prt)
    r = _context(tp)
    r.render_frames(prt.seed_pairs(FRAMES))
    r.render_guides(2)
    r.denoise_temporal(passes=1)
    hist, fb = r.read_history(), r.read_framebuffer()
    r.read_guides()
    r.rebuild_bvh(tp.v, None, 4)
    with pytest.raises(prt.PrtError) as e:
        r.read_guides()
    assert e.value.code == prt.PRT_ERR_NOT_READY
    assert np.array_equal(_bytes(r.read_history()), _bytes(hist)), "the history is kept"
    assert np.array_equal(_bytes(r.read_framebuffer()), _bytes(fb)), "the framebuffer is unchanged until the next render"
    state, img = _render(tp, r)
    r.close()
    nodes, prims = _mirror(tp.v, 4, "teapot seed 11 leaf 4")
    _assert_same(oracle, *_oracle_render(oracle, tp, _with(prt, tp.desc, tp.v, tp.n0, nodes, prims), "seed 11 leaf 4, old normals"), state, img,
                 "normals None: the uploaded normals in the new slots")


@pytest.mark.gpu
def test_motion_plane_after_a_rebuild_matches_the_caster(prt):
    sc = Rendered(prt, "cornell_coat.json")
    r = sc.context(prt)
    r.rebuild_bvh(sc.vB, sc.nB, 4)
    r.render_guides(1)
    plane = r.read_motion()
    # an update, then a rebuild, between two guide renders: still measured from the geometry before the update
    r.update_vertices(sc.v0, sc.n0)
    r.render_guides(1)
    r.update_vertices(sc.vA, sc.nA)
    r.rebuild_bvh(sc.vB, None, 2)
    r.render_guides(1)
    second = r.read_motion()
    r.close()
    worst = sc.check(plane, "coat, one rebuild")
    print("motion plane after a rebuild: largest |D - caster| over the matching pixels %.3e (bound %.3e)" % (worst, D_BOUND))
    assert worst <= D_BOUND, worst
    moving = (plane[..., 3] > 0) & (np.linalg.norm(plane[..., :3], axis=-1) > 0)
    assert moving.mean() >= 0.05
    assert sc.check(second, "coat, update then rebuild") <= D_BOUND


@pytest.mark.gpu
def test_row_block_contexts_that_each_rebuild(prt, oracle):
    tp = Teapot(prt)
    whole = _context(tp)
    whole.rebuild_bvh(tp.v, tp.n, 4)
    state, img = _render(tp, whole)
    whole.close()
    got_state, got_img = np.zeros_like(state).reshape(H, W), np.zeros_like(img)
    for part in range(2):
        rows = [y for y in range(H) if (y // 16) % 2 == part]
        r = _context(tp)
        r.set_row_blocks(W, H, 16, 2, part)
        r.rebuild_bvh(tp.v, tp.n, 4)
        s, i = _render(tp, r)
        r.close()
        got_state[rows], got_img[rows] = s.reshape(len(rows), W), i
    _assert_same(oracle, state, img, got_state.reshape(-1), got_img, "two row-block contexts")


@pytest.mark.gpu
def test_max_leaf_zero_on_the_device(prt):
    tp = Teapot(prt)
    r = _context(tp)
    r.rebuild_bvh(tp.v, tp.n, 0)
    nodes, prims = r.read_bvh()
    r.rebuild_bvh(tp.v, tp.n, DEFAULT_LEAF)
    again, prims2 = r.read_bvh()
    r.close()
    assert np.array_equal(_bytes(nodes), _bytes(again)) and np.array_equal(prims, prims2)
    want_nodes, want_prims = _mirror(tp.v, DEFAULT_LEAF, "teapot seed 11 leaf %d" % DEFAULT_LEAF)
    assert np.array_equal(_bytes(nodes), _bytes(want_nodes)) and np.array_equal(prims, want_prims)
