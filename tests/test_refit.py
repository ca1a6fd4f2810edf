"""prt_update_vertices: new vertices into the uploaded scene, the tree refitted on the device (include/prt.h; csrc/hip/pt_refit.h / .hip).

The contract is the one everything here has: bit-identical to the CPU oracle, which is fed the same refitted buffers in the reference's
layout.  `mirror_refit` (tests/mirrors.py) restates prt.h's box rules in numpy on the CALLER'S tree (children before parents, the comparison form that
fixes the sign of a zero bound); the triangle records are pack_scene's own expressions, so pack_scene of (new vertices, mirror's nodes) is
what every buffer must equal, byte for byte.

CPU tests run the kernels' bodies on the host (tests/emu/refit_emu.cpp); GPU tests run the library against oracle/pt_oracle.c."""
import numpy as np
import pytest

from cases import callers_tree, Case, _chain_desc, refit_context as _context, refit_oracle_render as _oracle_render, refit_render as _render
from mirrors import NODE_T
from support import assert_same_render as _assert_same, bytes_flat as _bytes


FRAMES = Case.FRAMES
f32 = np.float32


@pytest.fixture(scope="module")
def refit():
    import refit_api
    refit_api.lib()
    return refit_api


# ---- what the packed tables hold --------------------------------------------------------------------------------------------------------------

def _node_bounds(got):
    """[n_nodes, 6] from a Packed.get(): every node's box where pack_scene put it (node_box), the root's from `root`"""
    nb = got["node_box"]
    out = np.zeros((len(nb), 6), dtype=f32)
    ok = nb != 0xFFFFFFFF
    out[ok] = got["pairs"]["b"].reshape(-1, 2, 6)[nb[ok] >> 1, nb[ok] & 1]
    out[0] = got["root"]
    return out, ok


def _assert_packed_equal(got, want, want_root, what):
    assert np.array_equal(got["pairs"]["meta"], want["pairs"]["meta"]), what + ": the refit touched NodePair::meta"
    assert np.array_equal(_bytes(got["pairs"]["b"]), _bytes(want["pairs"]["b"])), what + ": pair boxes differ"
    assert np.array_equal(_bytes(got["root"]), _bytes(want_root)), what + ": root box differs"
    assert np.array_equal(got["tri_geom"], want["tri_geom"]), what + ": TriGeom differs"
    assert np.array_equal(got["tri_nrm"], want["tri_nrm"]), what + ": TriNrm differs"


def _plant_zeros(case):
    """in one leaf of at least two triangles: x alternating +0.0 / -0.0 and one shared y (equal coordinates), so that which zero a bound
    keeps, and which of two equal values, depends on the order and the form of the comparisons"""
    leaves = np.nonzero((case.nodes0["leaf"] != 0) & (case.nodes0["count"] >= 2))[0]
    leaf = case.nodes0[leaves[len(leaves) // 2]]
    fv = case.pi[int(leaf["first"]):int(leaf["first"]) + int(leaf["count"])].astype(np.uint32) * np.uint32(3)
    idx = (fv[:, None] + np.arange(3, dtype=np.uint32)[None, :]).reshape(-1)
    v = case.v.copy()
    v[idx, 0] = np.where(np.arange(len(idx)) % 2 == 0, f32(0.0), f32(-0.0))
    v[idx, 1] = f32(0.375)
    v[idx[1::3], 2] = -v[idx[1::3], 2]
    return v


# ---- CPU: the kernels' bodies on the host ----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("variant,order", [("cornell_coat", None), ("cornell_coat", "dfs"), ("cornell_edge", None)])
def test_bodies_equal_the_mirror(prt, refit, monkeypatch, variant, order):
    if order:
        monkeypatch.setenv("PRT_PAIR_ORDER", order)
    case = Case(prt, variant, seed=11)
    case.set(_plant_zeros(case), case.n)
    p = refit.Packed(case.cfg, case.desc)
    assert p.root_is_leaf == int(case.nodes0[0]["leaf"] != 0)
    assert not p.update(case.v, case.n)
    want = refit.Packed(case.cfg, case.new_desc).get()
    _assert_packed_equal(p.get(), want, case.nodes[0]["bounds"], "%s %s" % (variant, order or "default order"))
    if variant == "cornell_edge":
        assert p.root_is_leaf == 1 and p.n_pairs == 0, "cornell_edge is the leaf-root case"
    else:
        assert p.n_pairs == 3114 and p.n_slots == 6320


def test_bodies_tighten_a_callers_loose_tree(prt, oracle, refit):
    """cases.callers_tree with UNCHANGED vertices: a fat leaf, leaves sharing triangles, loose boxes that must come out tight"""
    scene, desc, keep = callers_tree(prt, oracle)
    case = Case(prt, "cornell_coat", desc=desc, scene=scene)
    p = refit.Packed(case.cfg, case.desc)
    before = p.get()
    assert not p.update(case.v, case.n)
    got = p.get()
    _assert_packed_equal(got, refit.Packed(case.cfg, case.new_desc).get(), case.nodes[0]["bounds"], "caller's tree")
    assert np.array_equal(got["tri_geom"], before["tri_geom"]) and np.array_equal(got["tri_nrm"], before["tri_nrm"])
    b = got["pairs"]["b"].reshape(-1, 2, 6)
    loose = np.array([-3, 3, -1, 5, -3, 3], dtype=f32)
    assert (b[:, :, 0::2] > loose[0::2]).all() and (b[:, :, 1::2] < loose[1::2]).all(), "a box stayed loose"
    assert p.n_slots == 40 + 40 + 70


@pytest.mark.parametrize("order", ["bfs", "dfs"])
def test_level_table(prt, refit, monkeypatch, order):
    monkeypatch.setenv("PRT_PAIR_ORDER", order)
    scene = prt.HostScene("cornell_coat.json")
    chain_desc, keep = _chain_desc(prt, scene, 300)
    for desc, levels in ((scene.desc, None), (chain_desc, 300)):
        p = refit.Packed(scene.config(), desc)          # (the chain of more than 256 levels is accepted by the upload's packing)
        g = p.get()
        assert np.array_equal(np.sort(g["level_pairs"]), np.arange(p.n_pairs, dtype=np.uint32)), "every pair in exactly one level"
        lf = g["level_first"].astype(np.int64)
        assert lf[0] == 0 and lf[-1] == p.n_pairs and (np.diff(lf) > 0).all() and len(lf) == p.n_levels + 1
        level = np.zeros(p.n_pairs, dtype=np.int64)
        for l in range(p.n_levels):
            members = g["level_pairs"][lf[l]:lf[l + 1]]
            assert (np.diff(members.astype(np.int64)) > 0).all(), "pair indices ascend within a level"
            level[members] = l
        assert level[0] == 0 and lf[1] == 1
        meta = g["pairs"]["meta"]
        for ch in (0, 1):
            inner = meta[:, 2 * ch + 1] == 0xFFFFFFFF
            assert np.array_equal(level[meta[inner, 2 * ch]], level[inner] + 1), "an inner child's level is its parent's plus 1"
        if levels:
            assert p.n_levels == levels and p.stack_levels == 1 and p.n_levels > 256


def test_bodies_reproduce_the_builders_bounds(prt, refit):
    """the builder's tree with unchanged vertices: its bounds come back by value (== ignores the sign of a zero), and bvh_cost agrees"""
    case = Case(prt, "cornell_coat")
    p = refit.Packed(case.cfg, case.desc)
    assert not p.update(case.v0, case.n0)
    bounds, reached = _node_bounds(p.get())
    reached[0] = True
    assert reached.all()
    assert (bounds == case.nodes0["bounds"]).all()
    assert (case.nodes["bounds"] == case.nodes0["bounds"]).all(), "the mirror disagrees with the builder"
    c0, c1 = prt.bvh_cost(case.nodes0), prt.bvh_cost(case.nodes0, bounds)
    assert c0 == c1 and np.isfinite(c0) and c0 > 1.0
    # a deformed tree costs something else, and the helper is a plain function of its inputs
    moved = Case(prt, "cornell_coat", seed=5)
    assert prt.bvh_cost(moved.nodes) != c0 and prt.bvh_cost(moved.nodes) == prt.bvh_cost(case.nodes0, moved.nodes["bounds"])
    # by hand: a root over two leaves of 2 and 3 triangles
    tiny = np.zeros(3, dtype=NODE_T)
    tiny["bounds"] = [[0, 2, 0, 2, 0, 2], [0, 1, 0, 2, 0, 2], [1, 2, 0, 1, 0, 1]]
    tiny["first"], tiny["count"], tiny["leaf"] = [1, 0, 2], [0, 2, 3], [0, 1, 1]
    assert prt.bvh_cost(tiny) == (24.0 + 2 * 16.0 + 3 * 6.0) / 24.0


def test_update_without_normals_keeps_trinrm(prt, refit):
    case = Case(prt, "cornell_coat", seed=3)
    p = refit.Packed(case.cfg, case.desc)
    before = p.get()
    assert not p.update(case.v, None)
    got = p.get()
    assert np.array_equal(got["tri_nrm"], before["tri_nrm"]) and not np.array_equal(got["tri_geom"], before["tri_geom"])
    # ... and a refusal writes nothing at all
    bad = case.v0.copy()
    bad[7, 2] = np.inf
    assert p.update(bad, case.n0)
    again = p.get()
    assert all(np.array_equal(_bytes(again[k]), _bytes(got[k])) for k in got)


# ---- GPU --------------------------------------------------------------------------------------------------------------------------------------

def _update_render_check(oracle, case, key, device=False):
    r = _context(case)
    if device:
        import torch
        r.update_vertices(torch.from_numpy(case.v).cuda(), torch.from_numpy(case.n).cuda())
    else:
        r.update_vertices(case.v, case.n)
    state, img = _render(case, r)
    bounds = r.read_bvh_bounds()
    r.close()
    ostate, oimg = _oracle_render(oracle, case, key)
    _assert_same(oracle, ostate, oimg, state, img, key)
    assert bounds.shape == (len(case.nodes), 6)
    assert np.array_equal(_bytes(bounds), _bytes(case.nodes["bounds"])), key + ": read_bvh_bounds differs from the mirror"
    return state, img, bounds


@pytest.mark.gpu
def test_render_after_update_matches_the_oracle(prt, oracle):
    _update_render_check(oracle, Case(prt, "cornell_coat", seed=11), "coat seed 11")


@pytest.mark.gpu
def test_device_variant_matches_the_host_variant(prt, oracle):
    case = Case(prt, "cornell_coat", seed=11)
    s1, i1, b1 = _update_render_check(oracle, case, "coat seed 11", device=True)
    s0, i0, b0 = _update_render_check(oracle, case, "coat seed 11")
    assert not oracle.state_fields_equal(s0.view(oracle.PATH_STATE_DTYPE), s1.view(oracle.PATH_STATE_DTYPE)) and oracle.images_equal(i0, i1)
    assert np.array_equal(_bytes(b0), _bytes(b1))


@pytest.mark.gpu
def test_callers_tree_comes_out_tight(prt, oracle):
    scene, desc, keep = callers_tree(prt, oracle)
    case = Case(prt, "cornell_coat", desc=desc, scene=scene)
    r = _context(case)
    assert np.array_equal(r.read_bvh_bounds()[1:], case.nodes0["bounds"][1:]), "before an update: the uploaded bounds"
    r.close()
    assert (case.nodes["bounds"] != case.nodes0["bounds"]).any()
    _update_render_check(oracle, case, "caller's tree")


@pytest.mark.gpu
def test_leaf_root(prt, oracle):
    case = Case(prt, "cornell_edge", seed=7)
    assert case.nodes0[0]["leaf"]
    _update_render_check(oracle, case, "edge seed 7")


@pytest.mark.gpu
def test_depth_first_pair_order(prt, oracle, monkeypatch):
    monkeypatch.setenv("PRT_PAIR_ORDER", "dfs")
    _update_render_check(oracle, Case(prt, "cornell_coat", seed=11), "coat seed 11")


@pytest.mark.gpu
def test_sequence_of_updates(prt, oracle):
    a, b = Case(prt, "cornell_coat", seed=21), Case(prt, "cornell_coat", seed=11)
    r = _context(b)
    fresh_bounds = r.read_bvh_bounds()
    r.update_vertices(a.v, a.n)
    r.update_vertices(b.v, b.n)
    state, img = _render(b, r)
    ostate, oimg = _oracle_render(oracle, b, "coat seed 11")          # (what a fresh context updated with B gives: the tests above)
    _assert_same(oracle, ostate, oimg, state, img, "A then B")
    assert np.array_equal(_bytes(r.read_bvh_bounds()), _bytes(b.nodes["bounds"]))
    r.update_vertices(b.v0, b.n0)
    back = r.read_bvh_bounds()
    r.close()
    assert (back == fresh_bounds).all(), "A, B, then the original vertices: the fresh context's bounds by value"
    assert (back == b.nodes0["bounds"]).all()


@pytest.mark.gpu
def test_refusals_leave_the_scene_as_it_was(prt, oracle):
    case = Case(prt, "cornell_coat", seed=11, normals_too=False)
    r = prt.Renderer(case.cfg, device=0)
    with pytest.raises(prt.PrtError) as e:
        r.update_vertices(case.v, case.n)
    assert e.value.code == prt.PRT_ERR_NOT_READY
    with pytest.raises(prt.PrtError) as e:
        r.read_bvh_bounds()
    assert e.value.code == prt.PRT_ERR_NOT_READY
    r.close()
    r = _context(case)
    bounds0 = r.read_bvh_bounds()
    state0, img0 = _render(case, r)
    bad = case.v.copy()
    bad[len(bad) // 2, 1] = np.nan
    for entry in ("host", "device"):
        with pytest.raises(prt.PrtError) as e:
            if entry == "host":
                r.update_vertices(bad, case.n)
            else:
                import torch
                r.update_vertices(torch.from_numpy(bad).cuda(), None)
        assert e.value.code == prt.PRT_ERR_INVALID_ARGUMENT
        assert np.array_equal(_bytes(r.read_bvh_bounds()), _bytes(bounds0))
        state, img = _render(case, r)
        _assert_same(oracle, state0.view(oracle.PATH_STATE_DTYPE), img0, state, img, "after a refused update (%s)" % entry)
    assert r.lib.prt_update_vertices(r.ctx, None, None) == prt.PRT_ERR_INVALID_ARGUMENT
    # normals == NULL: the uploaded normals stay (and the pointer is not read): the oracle on (new vertices, OLD normals)
    r.update_vertices(case.v, None)
    state, img = _render(case, r)
    r.close()
    assert np.array_equal(case.n, case.n0) and not np.array_equal(case.v, case.v0)
    _assert_same(oracle, *_oracle_render(oracle, case, "coat seed 11, old normals"), state, img, "normals=None")
    # more than 256 levels of pairs: uploads and renders, refused at the update, renders the same afterwards
    chain_desc, keep = _chain_desc(prt, case.scene, 300)
    r = _context(case, chain_desc)
    state0, img0 = _render(case, r)
    with pytest.raises(prt.PrtError) as e:
        r.update_vertices(case.v, None)
    assert e.value.code == prt.PRT_ERR_UNSUPPORTED
    state, img = _render(case, r)
    r.close()
    _assert_same(oracle, state0.view(oracle.PATH_STATE_DTYPE), img0, state, img, "the chain after its refused update")


@pytest.mark.gpu
def test_lifetime(prt, oracle):
    case = Case(prt, "cornell_coat", seed=11)
    r = _context(case)
    r.render_frames(prt.seed_pairs(FRAMES))
    variant = r.kernel_variant()
    r.render_guides(2)
    r.denoise_temporal(passes=1)
    hist, fb = r.read_history(), r.read_framebuffer()
    r.read_guides()
    r.update_vertices(case.v, case.n)
    with pytest.raises(prt.PrtError) as e:
        r.read_guides()
    assert e.value.code == prt.PRT_ERR_NOT_READY
    assert np.array_equal(_bytes(r.read_history()), _bytes(hist)), "the history is kept"
    assert np.array_equal(_bytes(r.read_framebuffer()), _bytes(fb)), "the framebuffer is unchanged until the next render"
    state, img = _render(case, r)
    assert r.kernel_variant() == variant
    r.close()
    _assert_same(oracle, *_oracle_render(oracle, case, "coat seed 11"), state, img, "render after the lifetime checks")
