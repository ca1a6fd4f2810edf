"""prt_bvh_cost / prt_set_rebuild_policy: the SAH cost of the current tree summed on the device in one fixed shape, and the rule that rebuilds a
refitted tree once it costs more than `limit` times the last built one (include/prt.h; csrc/hip/pt_cost.h / .hip).

`mirror_cost` below restates prt.h's formulas in float64 numpy on a table of PAIR_DTYPE records: every pair's term, the terms padded with
zeros to a power of two, s = s[0::2] + s[1::2] until one value is left, then the root's formula.  It shares no code with the bodies.  The
bodies (run on the host by tests/emu/cost_emu.cpp) and the device (through the C ABI) must give its bits.

CPU tests: the bodies against the mirror on packed and refitted golden scenes and on synthetic tables whose sum depends on its order, the
leaf root, and the public numpy helper.  GPU tests: the device against the mirror at every launch shape, prt_bvh_cost as a read-only call,
and the policy against the sequence of calls it stands for -- update, prt_bvh_cost, prt_rebuild_bvh -- made by hand on a second context."""
import ctypes as C
import os
import struct

import numpy as np
import pytest

from conftest import PKG_NAME, ROOT
from cases import (callers_tree, Case, _chain_desc, _leaf_root_desc, morph_case, pose_context, _skin, skin_case, _soup, T_TEAPOT,
                   teapot as posed_teapot)
from support import assert_api, bytes_flat as _bytes

f32, f64 = np.float32, np.float64
INNER = 0xFFFFFFFF
NEW_API = ("prt_bvh_cost", "prt_set_rebuild_policy", "prt_get_rebuild_report")
BLOCK = 256                     # terms a block of the device reduces (pt_cost.h PT_COST_BLOCK)
LIMIT, MAX_LEAF = 1.3, 4        # the policy of the sequence tests


def _bits(x):
    return struct.pack("<d", float(x))


@pytest.fixture(scope="module")
def emu():
    import cost_api
    cost_api.lib()
    return cost_api


@pytest.fixture(scope="module")
def build_emu():
    """tests/emu/build_emu.cpp: update and rebuild on the host -- what the sequence tests plan their frames with"""
    import build_api
    build_api.lib()
    return build_api


# ---- the mirror ------------------------------------------------------------------------------------------------------------------------------

def mirror_area(b):
    """A of boxes [..., 6] = min_x max_x min_y max_y min_z max_z (float32), in float64"""
    b = np.asarray(b, dtype=f32).astype(f64)
    e = b[..., 1::2] - b[..., 0::2]
    d = np.where(e > 0.0, e, 0.0)
    return 2.0 * ((d[..., 0] * d[..., 1] + d[..., 1] * d[..., 2]) + d[..., 2] * d[..., 0])


def mirror_terms(pairs):
    """t_k of every pair of a PAIR_DTYPE table"""
    area = mirror_area(pairs["b"].reshape(-1, 2, 6))
    count = pairs["meta"][:, 1::2]
    with np.errstate(invalid="ignore", over="ignore"):
        w = np.where(count == INNER, 1.0, count.astype(f64)) * area
    w = np.where(count == 0, 0.0, w)
    return w[:, 0] + w[:, 1]


def mirror_sum(terms):
    """the complete binary tree over the index, the terms padded with +0.0 to a power of two"""
    n = 1
    while n < len(terms):
        n *= 2
    s = np.zeros(n, dtype=f64)
    s[:len(terms)] = terms
    while len(s) > 1:
        s = s[0::2] + s[1::2]
    return float(s[0])


def mirror_root(pairs):
    """the root's box by the union rule over pair 0: child 0's box, child 1's merged by the two comparisons of the refit"""
    b0, b1 = pairs["b"][0][:6], pairs["b"][0][6:]
    out = b0.copy()
    out[0::2] = np.where(b1[0::2] < b0[0::2], b1[0::2], b0[0::2])
    out[1::2] = np.where(b1[1::2] > b0[1::2], b1[1::2], b0[1::2])
    return out


def mirror_cost(pairs=None, root=None, leaf_count=None):
    """the cost of a tree with an inner root from its pair table -- or, with leaf_count, of a leaf root of that many triangles with the box root"""
    with np.errstate(invalid="ignore", divide="ignore"):
        if leaf_count is not None:
            a = mirror_area(root)
            return float((f64(leaf_count) * a if leaf_count else f64(0.0)) / a)
        a = mirror_area(mirror_root(pairs))
        return float((a + f64(mirror_sum(mirror_terms(pairs)))) / a)


def mirror_packed(got, root_is_leaf, leaf_count):
    """the cost of an emulator's Packed.get()"""
    return mirror_cost(root=got["root"], leaf_count=leaf_count) if root_is_leaf else mirror_cost(got["pairs"])


def pairs_from_nodes(nodes):
    """the pair table of a REBUILT tree from prt_read_bvh's nodes: the children of pair k are nodes 2k + 1 and 2k + 2 (prt.h rule 6)"""
    n = (len(nodes) - 1) // 2
    pairs = np.zeros(n, dtype=np.dtype([("b", "<f4", 12), ("meta", "<u4", 4)]))
    for ch in (0, 1):
        kid = nodes[1 + ch::2][:n]
        pairs["b"][:, 6 * ch:6 * ch + 6] = kid["bounds"]
        leaf = kid["leaf"] != 0
        pairs["meta"][:, 2 * ch] = np.where(leaf, kid["first"], (kid["first"] - 1) // 2)
        pairs["meta"][:, 2 * ch + 1] = np.where(leaf, kid["count"], INNER)
    return pairs


def mirror_nodes(nodes):
    """the cost of prt_read_bvh's nodes of a rebuilt tree"""
    if nodes[0]["leaf"]:
        return mirror_cost(root=nodes[0]["bounds"], leaf_count=int(nodes[0]["count"]))
    return mirror_cost(pairs_from_nodes(nodes))


# ---- CPU: the bodies on the host -------------------------------------------------------------------------------------------------------------

def test_api_is_declared_exported_and_bound(prt):
    assert_api(NEW_API, prt)
    assert callable(prt.Renderer.bvh_cost) and callable(prt.Renderer.set_rebuild_policy) and callable(prt.Renderer.rebuild_report)
    assert "hip/pt_cost.hip" in open(os.path.join(ROOT, PKG_NAME, "build.py")).read()
    assert C.sizeof(prt._capi.RebuildPolicy) == 8 and C.sizeof(prt._capi.RebuildReport) == 24


@pytest.mark.parametrize("variant,order", [("cornell_coat", None), ("cornell_coat", "dfs"), ("cornell_coat", "bfs"), ("cornell_edge", None)])
def test_bodies_equal_the_mirror(prt, emu, monkeypatch, variant, order):
    """the packed tables of two golden scenes in both pair orders, as packed and after an emulated refit of deformed vertices"""
    if order:
        monkeypatch.setenv("PRT_PAIR_ORDER", order)
    case = Case(prt, variant, seed=11)
    p = emu.Packed(case.cfg, case.desc)
    leaf_count = p.root_leaf_count if p.root_is_leaf else None
    costs = []
    for step in ("as packed", "refitted"):
        if step == "refitted":
            assert not p.update(case.v)
        got = p.get()
        cost, S = p.cost()
        want = mirror_packed(got, p.root_is_leaf, leaf_count)
        assert _bits(cost) == _bits(want), "%s %s, %s: %r differs from the mirror's %r" % (variant, order, step, cost, want)
        if not p.root_is_leaf:
            assert _bits(S) == _bits(mirror_sum(mirror_terms(got["pairs"])))
            assert emu.table_cost(got["pairs"]) == (cost, S), "the two doors disagree"
        costs.append(cost)
    if variant == "cornell_edge":
        assert p.root_is_leaf == 1 and costs == [2.0, 2.0], "cornell_edge is the leaf-root case: the cost of a leaf root is its count"
    else:
        assert p.n_pairs == 3114 and np.isfinite(costs).all() and costs[0] > 1.0 and costs[1] != costs[0]


def test_pair_orders_sum_in_different_orders(prt, emu, monkeypatch):
    """the same tree under the packer's two pair orders: the same terms in another order -- each equals its own mirror (above), and they agree
    to the bound of two orders of summing n non-negative terms"""
    case = Case(prt, "cornell_coat")
    got = {}
    for order in ("bfs", "dfs"):
        monkeypatch.setenv("PRT_PAIR_ORDER", order)
        p = emu.Packed(case.cfg, case.desc)
        got[order] = (p.cost()[0], p.get()["pairs"])
    assert not np.array_equal(got["bfs"][1]["meta"], got["dfs"][1]["meta"]), "the two orders gave one table"
    assert abs(got["bfs"][0] - got["dfs"][0]) <= len(got["bfs"][1]) * 2.0 ** -52 * got["bfs"][0]


def synthetic_table(n_pairs, seed, wide=False):
    """random finite boxes, inner and leaf children mixed, leaf counts of 0, 1 and 64 among others; wide: every pair at a scale of its own out
    of 15 decades, so that the terms (areas) span 30 orders of magnitude"""
    rng = np.random.default_rng(seed)
    pairs = np.zeros(n_pairs, dtype=np.dtype([("b", "<f4", 12), ("meta", "<u4", 4)]))
    scale = 10.0 ** rng.uniform(-7.5, 7.5, (n_pairs, 1, 1)) if wide else np.full((n_pairs, 1, 1), 5.0)
    lo = scale * rng.uniform(-2, 2, (n_pairs, 2, 3))
    ext = scale * rng.uniform(0.25, 1, (n_pairs, 2, 3))
    box = np.zeros((n_pairs, 2, 6))
    box[:, :, 0::2], box[:, :, 1::2] = lo, lo + ext
    pairs["b"] = box.reshape(n_pairs, 12).astype(f32)
    kind = rng.integers(0, 6, (n_pairs, 2))
    count = np.choose(kind, [INNER, 0, 1, 64, rng.integers(2, 64, (n_pairs, 2)), INNER]).astype(np.uint32)
    if n_pairs >= 3:
        count[0], count[1], count[2] = (INNER, 0), (1, 64), (0, 0)         # (every kind at least once; a pair of two empty leaves)
    pairs["meta"][:, 1::2] = count
    pairs["meta"][:, 0::2] = rng.integers(0, n_pairs, (n_pairs, 2))
    if n_pairs >= 3:
        pairs["b"][2] = np.nan                                             # (an empty leaf contributes +0 whatever its box)
    return pairs


def test_synthetic_tables(emu):
    told_apart = 0
    for n_pairs in (1, 2, 3, 63, 64, 65, 255, 256, 257, 1000):
        for wide in (False, True):
            pairs = synthetic_table(n_pairs, 100 + n_pairs, wide)
            terms = mirror_terms(pairs)
            assert np.isfinite(terms).all() and (terms >= 0).all() and not np.signbit(terms).any()
            if n_pairs >= 3:
                assert _bits(terms[2]) == _bits(0.0), "a pair of empty leaves with NaN boxes: +0"
            cost, S = emu.table_cost(pairs)
            want_S = mirror_sum(terms)
            assert _bits(S) == _bits(want_S), "%d pairs%s: S %r differs from the mirror's %r" % (n_pairs, ", wide" if wide else "", S, want_S)
            assert _bits(cost) == _bits(mirror_cost(pairs))
            straight = 0.0
            for t in terms.tolist():
                straight += t
            told_apart += _bits(straight) != _bits(want_S)
            if wide and n_pairs >= 255:
                pos = terms[terms > 0]
                assert pos.max() / pos.min() >= 1e30, "the wide table's terms do not span 30 orders of magnitude"
    assert told_apart >= 1, "a left-to-right sum gives the mirror's bits on every table: the test cannot tell the orders apart"


def test_leaf_root(emu):
    box = np.array([-1, 2, 0, 3, 1, 1.5], dtype=f32)
    for count in (1, 2, 7, 65538):
        cost, S = emu.table_cost(None, root=box, leaf_count=count)
        assert cost == float(count) == mirror_cost(root=box, leaf_count=count) and S == 0.0
    flat = np.array([0, 0, 0, 0, 0, 5], dtype=f32)                     # two zero extents: no area
    assert np.isnan(emu.table_cost(None, root=flat, leaf_count=3)[0]) and np.isnan(mirror_cost(root=flat, leaf_count=3))
    inverted = np.array([1, 0, 3, 0, 1, 2], dtype=f32)                  # max < min on two axes: their extents count as 0
    assert np.isnan(emu.table_cost(None, root=inverted, leaf_count=3)[0])
    assert _bits(emu.table_cost(None, root=box, leaf_count=0)[0]) == _bits(0.0), "an empty leaf root: +0 over its area"
    # an inner root without area: IEEE's NaN or infinity, as the mirror's
    pairs = synthetic_table(2, 5)
    pairs["b"][0] = np.tile(flat, 2)
    pairs["meta"][0] = (0, 1, 1, 1)
    pairs["meta"][1] = (0, 2, 3, 5)
    assert emu.table_cost(pairs)[0] == np.inf == mirror_cost(pairs), "(0 + S) / 0 with S > 0"


@pytest.mark.parametrize("seed", [None, 11])
def test_agreement_with_the_public_helper(prt, emu, seed):
    """bvh_cost(nodes) over the same tree in the reference's layout sums the same non-negative terms in node order: two orders of summing N
    terms differ by at most N * 2^-52 relative, the final division included (derived, not measured)"""
    case = Case(prt, "cornell_coat", seed=seed)
    p = emu.Packed(case.cfg, case.desc)
    if seed is not None:
        assert not p.update(case.v)
    cost = p.cost()[0]
    nodes = case.nodes0 if seed is None else case.nodes
    want = prt.bvh_cost(nodes)
    assert abs(cost - want) <= len(nodes) * 2.0 ** -52 * want, (cost, want)
    assert 2 * p.n_pairs + 1 == len(nodes), "the pair table holds exactly the inner nodes the root reaches"


# ---- GPU -------------------------------------------------------------------------------------------------------------------------------------

W, H, SPP, FRAMES = 16, 16, 4, 24
AMPLITUDES = (0.05, 1.0, 1.05, 0.0)         # of wave(): chosen with the mirror (plan(): two frames stay below the limit, two pass it)
_cache = {}


def teapot(prt):
    """cornell_coat through cases.Case with a camera of this file's frame size"""
    if "teapot" not in _cache:
        from conftest import variant_camera
        case = Case(prt, "cornell_coat")
        case.cam = variant_camera(prt, "cornell_coat", W, H)
        _cache["teapot"] = case
    return _cache["teapot"]


def wave(v0, amp):
    """a sine deformation of amplitude amp: x by the height, z by x (float32, from the rest pose)"""
    v = np.array(v0, dtype=f32)
    v[:, 0] = (v0[:, 0] + amp * np.sin(6.0 * v0[:, 1].astype(f64))).astype(f32)
    v[:, 2] = (v0[:, 2] + amp * np.cos(5.0 * v0[:, 0].astype(f64))).astype(f32)
    return v


def frames_of(prt):
    """the four frames of the sequence tests: (vertices, normals); the third carries its normals (None)"""
    if "frames" not in _cache:
        case = teapot(prt)
        out = [(wave(case.v0, a), None if i == 2 else case.n0) for i, a in enumerate(AMPLITUDES)]
        for v, n in out:
            v.setflags(write=False)
        _cache["frames"] = out
    return _cache["frames"]


def _limit_times(baseline, limit=LIMIT):
    return float(f64(f32(limit)) * f64(baseline))      # prt.h: (double)limit * baseline


def plan(prt, build_emu):
    """the sequence on the host, by the update and rebuild bodies and the mirror: (baseline as uploaded, [(cost, rebuilt, baseline after)])"""
    if "plan" not in _cache:
        case = teapot(prt)
        p = build_emu.Packed(case.cfg, case.desc)
        cost_now = lambda: mirror_packed(p.get(), p.root_is_leaf, p.root_leaf_count)
        first = base = cost_now()
        steps = []
        for v, n in frames_of(prt):
            assert p.update(v, n) == 0
            cost = cost_now()
            rebuilt = cost > _limit_times(base)
            margin = cost / _limit_times(base)
            if rebuilt:
                assert p.rebuild(v, n, MAX_LEAF) == 0
                base = cost_now()
            steps.append((cost, rebuilt, base, margin))
        _cache["plan"] = (first, steps)
    return _cache["plan"]


def assert_plan_is_not_vacuous(steps):
    margins = [s[3] for s in steps]
    assert min(margins) <= 0.95, "no frame stays 5 %% or more below the limit: %r" % (margins,)
    assert max(margins) >= 1.05, "no frame goes 5 %% or more above the limit: %r" % (margins,)
    assert all(abs(m - 1.0) >= 0.05 for m in margins), "a frame within 5 %% of the limit: %r" % (margins,)


def test_the_planned_sequence_crosses_the_limit_both_ways(prt, build_emu):
    first, steps = plan(prt, build_emu)
    assert_plan_is_not_vacuous(steps)
    assert [s[1] for s in steps] == [False, True, False, True]
    assert steps[1][2] != first and steps[0][2] == first, "a rebuild moves the baseline, a refit does not"


def _context(prt, case, desc=None, motion=False, part=None):
    r = prt.Renderer(case.cfg, device=0)
    r.upload_scene(desc if desc is not None else case.desc)
    r.set_camera(case.cam)
    r.resize(W, H)
    if part is not None:
        r.set_row_blocks(W, H, 4, 2, part)
    if motion:
        r.set_motion(True)
    return r


def _seeds(prt):
    if "seeds" not in _cache:
        _cache["seeds"] = prt.seed_pairs(256)
    return _cache["seeds"]


def _everything(prt, r, motion=False):
    """the tree, the normals, a 16 x 16 render of 4 spp and -- with motion -- the motion plane of a guide render"""
    nodes, prims = r.read_bvh()
    out = {"nodes": nodes, "prims": prims, "normals": r.read_normals(), "bounds": r.read_bvh_bounds()}
    r.reset()
    r.render_spp(SPP, _seeds(prt))
    out["state"], out["framebuffer"] = r.read_state(), r.read_framebuffer()
    if motion:
        r.render_guides(1)
        out["motion"] = r.read_motion()
    return out


def _assert_equal(got, want, what):
    assert sorted(got) == sorted(want)
    for k in want:
        assert got[k].shape == want[k].shape and np.array_equal(_bytes(got[k]), _bytes(want[k])), "%s: %s differs" % (what, k)


def _assert_report(r, cost, baseline, rebuilt, rebuilds, what):
    rep = r.rebuild_report()
    assert (_bits(rep["cost"]), _bits(rep["baseline"]), rep["rebuilt"], rep["rebuilds"]) == (_bits(cost), _bits(baseline), rebuilt, rebuilds), \
        "%s: the report %r is not (%r, %r, %r, %r)" % (what, rep, cost, baseline, rebuilt, rebuilds)


def _refused(prt, call, code):
    with pytest.raises(prt.PrtError) as e:
        call()
    assert e.value.code == code, e.value
    return e.value


def _update(r, v, n, device):
    if device:
        import torch
        r.update_vertices(torch.from_numpy(np.array(v)).cuda(), None if n is None else torch.from_numpy(np.array(n)).cuda())
    else:
        r.update_vertices(v, n)


@pytest.mark.gpu
@pytest.mark.parametrize("variant", ["cornell_coat", "cornell_edge"])
def test_device_cost_equals_the_mirror(prt, emu, variant):
    """after the upload, a host update, a device update and a rebuild; cornell_edge: the leaf root, its box as uploaded and then the device's"""
    case = Case(prt, variant, seed=11)
    other = Case(prt, variant, seed=21)
    p = emu.Packed(case.cfg, case.desc)
    leaf_count = p.root_leaf_count if p.root_is_leaf else None
    r = prt.Renderer(case.cfg, device=0)
    r.upload_scene(case.desc)
    want = mirror_packed(p.get(), p.root_is_leaf, leaf_count)
    assert _bits(r.bvh_cost()) == _bits(want), "after the upload: %r, the mirror %r" % (r.bvh_cost(), want)
    for what, c, device in (("a host update", case, False), ("a device update", other, True)):
        assert not p.update(c.v)
        _update(r, c.v, c.n, device)
        want = mirror_packed(p.get(), p.root_is_leaf, leaf_count)
        assert _bits(r.bvh_cost()) == _bits(want), "after %s: %r, the mirror %r" % (what, r.bvh_cost(), want)
        assert _bits(r.bvh_cost()) == _bits(want), "a second call differs"
    for max_leaf in (4, 1, 64):
        r.rebuild_bvh(case.v, case.n, max_leaf)
        nodes, _ = r.read_bvh()
        want = mirror_nodes(nodes)
        assert _bits(r.bvh_cost()) == _bits(want), "after a rebuild, max_leaf %d: %r, the mirror %r" % (max_leaf, r.bvh_cost(), want)
        helper = prt.bvh_cost(nodes)
        assert abs(want - helper) <= len(nodes) * 2.0 ** -52 * helper
    r.close()


@pytest.mark.gpu
def test_cost_of_a_tree_too_deep_to_refit(prt, emu):
    case = Case(prt, "cornell_coat", seed=11)
    desc, keep = _chain_desc(prt, case.scene, 300)
    p = emu.Packed(case.cfg, desc)
    assert p.n_levels == 300 and p.n_pairs == 300
    r = prt.Renderer(case.cfg, device=0)
    r.upload_scene(desc)
    _refused(prt, lambda: r.update_vertices(case.v, None), prt.PRT_ERR_UNSUPPORTED)
    assert _bits(r.bvh_cost()) == _bits(mirror_cost(p.get()["pairs"]))
    r.close()


@pytest.mark.gpu
@pytest.mark.parametrize("T", [2, 3, BLOCK // 4, BLOCK // 4 + 1, BLOCK // 4 + 2, BLOCK, BLOCK + 1, BLOCK + 2, BLOCK * BLOCK + 2])
def test_launch_shapes(prt, T):
    """T - 1 pairs: 1 and 2, a wave less one, a wave, a wave and one, a block less one, a block, a block and one, and the smallest table that
    needs a third level, with a ragged last block on every level"""
    case = teapot(prt)
    v, n = _soup("random", T)
    r = prt.Renderer(case.cfg, device=0)
    r.upload_scene(_leaf_root_desc(prt, case.desc, v, n))
    assert r.bvh_cost() == float(T), "a leaf root over every triangle, its box as uploaded (its area and T times it are exact)"
    r.update_vertices(v, None)
    assert _bits(r.bvh_cost()) == _bits(mirror_nodes(r.read_bvh()[0])), "... and the device's box after a refit"
    assert abs(r.bvh_cost() - T) <= T * 2.0 ** -52
    r.rebuild_bvh(v, None, 1)
    nodes, _ = r.read_bvh()
    assert len(nodes) == 2 * (T - 1) + 1, "max_leaf 1 gives T - 1 pairs"
    want = mirror_nodes(nodes)
    assert _bits(r.bvh_cost()) == _bits(want), "%d pairs: %r, the mirror %r" % (T - 1, r.bvh_cost(), want)
    r.update_vertices((v * f32(0.5)).astype(f32), None)             # (the refit of a rebuilt tree, costed again)
    assert _bits(r.bvh_cost()) == _bits(mirror_nodes(r.read_bvh()[0]))
    r.close()


@pytest.mark.gpu
def test_the_cost_call_is_read_only(prt):
    """two contexts run one sequence with motion on; one of them also asks for the cost wherever something could be disturbed"""
    case = teapot(prt)
    v, n = frames_of(prt)[0]
    got = []
    for ask in (True, False):
        r = _context(prt, case, motion=True)
        r.render_frames(prt.seed_pairs(FRAMES))
        r.render_guides(2)
        r.denoise_temporal(passes=1)
        before = {"framebuffer": r.read_framebuffer(), "state": r.read_state(), "guides": r.read_guides(), "history": r.read_history()}
        if ask:
            cost0 = r.bvh_cost()
            after = {"framebuffer": r.read_framebuffer(), "state": r.read_state(), "guides": r.read_guides(), "history": r.read_history()}
            _assert_equal(after, before, "after prt_bvh_cost")          # (read_guides succeeds: the guides are still valid)
        r.update_vertices(v, n)                                         # a motion snapshot is pending from here on
        if ask:
            assert r.bvh_cost() != cost0
            _refused(prt, r.read_guides, prt.PRT_ERR_NOT_READY)          # (stale since the update, and not revived)
        out = dict(before, history2=r.read_history(), framebuffer2=r.read_framebuffer())
        r.render_frames(prt.seed_pairs(FRAMES), first_frame=FRAMES + 1)
        if ask:
            r.bvh_cost()
        r.render_guides(1)
        out["motion"] = r.read_motion()
        out["state3"], out["framebuffer3"] = r.read_state(), r.read_framebuffer()
        got.append(out)
        r.close()
    _assert_equal(got[0], got[1], "with and without prt_bvh_cost")
    assert (got[0]["motion"][..., 3] > 0).any() and (np.linalg.norm(got[0]["motion"][..., :3], axis=-1) > 0).any(), "the snapshot was not consumed"


@pytest.mark.gpu
@pytest.mark.parametrize("motion", [False, True])
def test_policy_equals_the_manual_sequence(prt, build_emu, motion):
    case = teapot(prt)
    first, steps = plan(prt, build_emu)
    assert_plan_is_not_vacuous(steps)
    a, b = _context(prt, case, motion=motion), _context(prt, case, motion=motion)
    before = _everything(prt, a, motion)
    a.set_rebuild_policy(LIMIT, MAX_LEAF)
    _assert_equal(_everything(prt, a, motion), before, "setting the policy changes no bit of the scene")
    base, rebuilds = b.bvh_cost(), 0
    assert _bits(base) == _bits(first)
    _assert_report(a, base, base, False, 0, "before any update")
    for i, (v, n) in enumerate(frames_of(prt)):
        what = "frame %d (amplitude %g)" % (i, AMPLITUDES[i])
        device = i == 1
        _update(a, v, n, device)
        _update(b, v, n, device)
        cost = b.bvh_cost()
        rebuilt = cost > _limit_times(base)
        if rebuilt:
            if device:
                import torch
                b.rebuild_bvh(torch.from_numpy(np.array(v)).cuda(), None if n is None else torch.from_numpy(np.array(n)).cuda(), MAX_LEAF)
            else:
                b.rebuild_bvh(v, n, MAX_LEAF)
            base, rebuilds = b.bvh_cost(), rebuilds + 1
        _assert_report(a, cost, base, rebuilt, rebuilds, what)
        assert (_bits(cost), rebuilt, _bits(base)) == (_bits(steps[i][0]), steps[i][1], _bits(steps[i][2])), what + ": not what the mirror planned"
        assert a.bvh_node_count == b.bvh_node_count
        _assert_equal(_everything(prt, a, motion), _everything(prt, b, motion), what)
    assert rebuilds == 2
    a.close(), b.close()


@pytest.mark.gpu
@pytest.mark.parametrize("through", ["skin", "morph"])
def test_policy_through_a_pose_and_a_morph(prt, build_emu, through):
    """one frame that triggers, through pose(rebuild=False) on a skin and through morph(rebuild=False): the rebuild is over the posed buffers"""
    case = posed_teapot(prt)
    s = skin_case(prt, T_TEAPOT, 4) if through == "skin" else morph_case(prt, T_TEAPOT, 3)
    p = build_emu.Packed(case.cfg, case.desc)
    first = mirror_packed(p.get(), p.root_is_leaf, p.root_leaf_count)
    assert p.update(s["v"], s["n"]) == 0
    planned = mirror_packed(p.get(), p.root_is_leaf, p.root_leaf_count)
    assert planned >= 1.05 * _limit_times(first), "the frame does not pass the limit by 5 %"
    got = []
    for policy in (True, False):
        r = pose_context(prt, s, leaf_root=False)
        r.set_camera(teapot(prt).cam)
        r.resize(W, H)
        if through == "skin":
            _skin(r, s)
        else:
            r.set_morph_targets(s["v0"], s["n0"], s["targets"])          # (tests/test_morph.py's _set)
        if policy:
            r.set_rebuild_policy(LIMIT, MAX_LEAF)
        nodes_before = r.bvh_node_count
        if through == "skin":
            r.pose(s["M"], rebuild=False)
        else:
            r.morph(s["weights"], rebuild=False)
        if policy:
            rep = r.rebuild_report()
            assert r.bvh_node_count != nodes_before
        else:
            cost, base = r.bvh_cost(), first
            assert _bits(cost) == _bits(planned) and cost > _limit_times(base)
            v, n = r.read_posed() if through == "skin" else r.read_morphed()
            assert np.array_equal(_bytes(v), _bytes(s["v"]))
            r.rebuild_bvh(v, n, MAX_LEAF)
            assert (_bits(rep["cost"]), _bits(rep["baseline"]), rep["rebuilt"], rep["rebuilds"]) == (_bits(cost), _bits(r.bvh_cost()), True, 1)
        got.append(_everything(prt, r))
        r.close()
    _assert_equal(got[0], got[1], "through a " + through)


@pytest.mark.gpu
def test_a_limit_never_reached(prt):
    case = teapot(prt)
    a, b = _context(prt, case), _context(prt, case)
    a.set_rebuild_policy(1e30)
    base = b.bvh_cost()
    for i, (v, n) in enumerate(frames_of(prt)[:2]):
        a.update_vertices(v, n)
        b.update_vertices(v, n)
        _assert_report(a, b.bvh_cost(), base, False, 0, "frame %d" % i)
        _assert_equal(_everything(prt, a), _everything(prt, b), "frame %d under a limit of 1e30" % i)
    a.close(), b.close()


@pytest.mark.gpu
def test_row_block_contexts_under_one_policy(prt):
    case = teapot(prt)

    def run(part):
        r = _context(prt, case, part=part)
        r.set_rebuild_policy(LIMIT, MAX_LEAF)
        reports = []
        for v, n in frames_of(prt)[:2]:
            r.update_vertices(v, n)
            reports.append(r.rebuild_report())
        r.reset()
        r.render_frames(prt.seed_pairs(FRAMES))
        out = reports, r.read_state(), r.read_framebuffer()
        r.close()
        return out
    reports, state, img = run(None)
    assert [rep["rebuilt"] for rep in reports] == [False, True]
    got_state, got_img = np.zeros_like(state).reshape(H, W), np.zeros_like(img)
    for part in range(2):
        rows = [y for y in range(H) if (y // 4) % 2 == part]
        rep, st, im = run(part)
        assert rep == reports, "part %d took other decisions, or saw other costs" % part
        got_state[rows], got_img[rows] = st.reshape(len(rows), W), im
    assert np.array_equal(_bytes(got_state), _bytes(state)) and np.array_equal(_bytes(got_img), _bytes(img)), "two row-block contexts"


@pytest.mark.gpu
def test_refusals_and_lifetime(prt, oracle):
    case = teapot(prt)
    frames = frames_of(prt)
    c_policy = prt._capi.RebuildPolicy
    r = prt.Renderer(case.cfg, device=0)
    _refused(prt, r.bvh_cost, prt.PRT_ERR_NOT_READY)
    _refused(prt, lambda: r.set_rebuild_policy(LIMIT), prt.PRT_ERR_NOT_READY)
    _refused(prt, lambda: r.set_rebuild_policy(None), prt.PRT_ERR_NOT_READY)
    _refused(prt, r.rebuild_report, prt.PRT_ERR_NOT_READY)
    r.close()
    r = _context(prt, case)
    _refused(prt, r.rebuild_report, prt.PRT_ERR_NOT_READY)               # a scene, no policy
    assert r.lib.prt_bvh_cost(r.ctx, None) == prt.PRT_ERR_INVALID_ARGUMENT
    assert r.lib.prt_bvh_cost(None, None) == prt.PRT_ERR_INVALID_ARGUMENT
    r.set_rebuild_policy(LIMIT, MAX_LEAF)
    assert r.lib.prt_get_rebuild_report(r.ctx, None) == prt.PRT_ERR_INVALID_ARGUMENT
    base = r.bvh_cost()
    scene = _everything(prt, r)
    for what, limit, max_leaf in (("a limit below 1", 0.999, 4), ("a NaN limit", float("nan"), 4), ("an infinite limit", float("inf"), 4),
                                  ("a negative limit", -2.0, 4), ("max_leaf 65", 2.0, 65)):
        _refused(prt, lambda: r.set_rebuild_policy(limit, max_leaf), prt.PRT_ERR_INVALID_ARGUMENT)
        _assert_report(r, base, base, False, 0, what)
        _assert_equal(_everything(prt, r), scene, what)
    # ... and the policy in force is still the one of 1.3: frame 0 stays, frame 1 goes
    r.update_vertices(*frames[0])
    assert r.rebuild_report()["rebuilt"] is False
    r.update_vertices(*frames[1])
    rep = r.rebuild_report()
    assert rep["rebuilt"] is True and rep["rebuilds"] == 1 and _bits(rep["baseline"]) == _bits(r.bvh_cost()) != _bits(base)
    # it survives a reset, a resize and a camera change; an explicit rebuild moves the baseline
    r.reset()
    r.resize(W, H)
    r.set_camera(case.cam)
    r.rebuild_bvh(case.v0, case.n0, 1)
    rep = r.rebuild_report()
    assert _bits(rep["baseline"]) == _bits(r.bvh_cost()) and rep["rebuilds"] == 1, "an explicit rebuild moves the baseline"
    r.set_rebuild_policy(1.0)                                              # (limit 1 is the smallest accepted; setting it anew restarts the count)
    _assert_report(r, r.bvh_cost(), r.bvh_cost(), False, 0, "set anew")
    # prt_upload_scene turns it off
    r.upload_scene(case.desc)
    _refused(prt, r.rebuild_report, prt.PRT_ERR_NOT_READY)
    r.update_vertices(*frames[1])
    assert r.bvh_node_count == len(case.nodes0), "an update without a policy rebuilt"
    # None turns it off
    r.set_rebuild_policy(LIMIT)
    r.set_rebuild_policy(None)
    _refused(prt, r.rebuild_report, prt.PRT_ERR_NOT_READY)
    r.close()
    # a caller's tree that references 100 of T triangles, normals None: the update that triggers returns the rebuild's refusal, and the scene
    # is the refitted one -- what a context without a policy holds after the same update
    scene, cdesc, keep = callers_tree(prt, oracle)
    a, b = _context(prt, case, cdesc), _context(prt, case, cdesc)
    a.update_vertices(frames[2][0], None)                                  # (a pose in which the caller's tree is cheap: the baseline)
    b.update_vertices(frames[2][0], None)
    a.set_rebuild_policy(1.0, MAX_LEAF)
    base = b.bvh_cost()
    b.update_vertices(case.v0, None)
    assert b.bvh_cost() >= 1.05 * base, "the caller's tree does not cost 5 % more in the rest pose: nothing would trigger"
    e = _refused(prt, lambda: a.update_vertices(case.v0, None), prt.PRT_ERR_INVALID_ARGUMENT)
    assert "prt_rebuild_bvh" in str(e)
    _assert_report(a, b.bvh_cost(), base, False, 0, "after the refused rebuild")
    _assert_equal(_everything(prt, a), _everything(prt, b), "the refitted scene after the refused rebuild")
    a.update_vertices(case.v0, case.n0)                                    # with normals the same update rebuilds
    assert a.rebuild_report()["rebuilt"] is True and a.bvh_node_count != b.bvh_node_count
    a.close(), b.close()
