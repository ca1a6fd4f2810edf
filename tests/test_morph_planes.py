"""prt_set_morph_targets_layout / prt_get_morph_report: the morph targets as planes of 64 corners per target (include/prt.h
PRT_MORPH_LAYOUT_PLANES; csrc/hip/pt_morph.h / .hip), a second table layout for the same sets with the same bits out.

The yardstick is the float32 numpy mirror of tests/mirrors.py (mirror_morph), which shares no code with either body, and the per-corner layout itself: the plane
body (run on the host by tests/emu/morph_planes_emu.cpp in the kernel's launch shape, over the table the library's own builder makes) and
the device (through the C ABI) must give the mirror's bytes and those of the same set under PRT_MORPH_LAYOUT_CORNERS.

CPU tests: the builder against a numpy restatement written here from the targets' corner lists, the bodies against the mirror on the
teapot and on planted cases -- cases.planted(), and those a plane can get wrong: the two sides of a block boundary, the two halves of the
mask, its first and last bit, a -0 on an unlisted lane, a NaN weight on a plane with one listed lane, 257 planes in one block -- and the
report's arithmetic.  GPU tests: the read-backs through every door at 3, 66, 192, 258 and 18 960 corners (a ragged block; a block and two
lanes; exactly three blocks; a workgroup and a tail; many), the scene after a morph, replacement, lifetime, refusals and row blocks."""
import ctypes as C

import numpy as np
import pytest

from cases import (_assert_equal, _everything, fused_case, identity, morph_case, planted, pose_context as _context, POSE_FRAME, pose_scene as _scene,
                   REBUILD, REFIT, _refused, _skin, T_TEAPOT, teapot)
from mirrors import mirror_morph, mirror_morph_raw, mirror_pose
from support import assert_api, bytes_flat as _bytes

f32 = np.float32
W, H, FRAMES = POSE_FRAME
NAMES = ("prt_set_morph_targets_layout", "prt_get_morph_report")
CORNERS, PLANES = 0, 1


@pytest.fixture(scope="module")
def emu():
    import morph_planes_api
    morph_planes_api.lib()
    return morph_planes_api


@pytest.fixture(scope="module")
def corners_emu():
    import morph_api
    morph_api.lib()
    return morph_api


# ---- the restatement of the table ------------------------------------------------------------------------------------------------------------

def restate_planes(corners, targets, with_normals):
    """(block_first, head [P, 4], plane_p [P, 3, 64], plane_n or None) from the targets' corner lists: a plane per (block, target) with a
    listed corner, sorted by (block, target); +0 on unlisted lanes and for a target without normal deltas"""
    blocks = (corners + 63) // 64
    planes = []
    for t, (corner, dp, dn) in enumerate(targets):
        corner = np.asarray(corner, dtype=np.int64)
        for b in np.unique(corner >> 6):
            sel = (corner >> 6) == b
            lanes = corner[sel] & 63
            mask = sum(1 << int(l) for l in lanes)
            p, n = np.zeros((3, 64), dtype=f32), np.zeros((3, 64), dtype=f32)
            p[:, lanes] = np.asarray(dp, dtype=f32).reshape(-1, 4)[sel, :3].T
            if dn is not None:
                n[:, lanes] = np.asarray(dn, dtype=f32).reshape(-1, 4)[sel, :3].T
            planes.append((int(b), t, mask, p, n))
    planes.sort(key=lambda x: (x[0], x[1]))
    count = np.bincount(np.array([x[0] for x in planes], dtype=np.int64), minlength=blocks)
    block_first = np.concatenate([[0], np.cumsum(count)]).astype(np.uint32)
    head = np.array([[t, 0, m & 0xFFFFFFFF, m >> 32] for _, t, m, _, _ in planes], dtype=np.uint32).reshape(-1, 4)
    plane_p = np.array([x[3] for x in planes], dtype=f32).reshape(-1, 3, 64)
    plane_n = np.array([x[4] for x in planes], dtype=f32).reshape(-1, 3, 64) if with_normals else None
    return block_first, head, plane_p, plane_n


def table_bytes(layout, T, entries, planes, nrm):
    """prt.h's formulas"""
    k = 2 if nrm else 1
    if layout == CORNERS:
        return 4 * (3 * T + 1) + 16 * entries * k
    return 4 * ((3 * T + 63) // 64 + 1) + 16 * planes + 768 * planes * k


def _special_set(prt):
    """86 triangles, 258 corners, 5 blocks: target 1 has no entries, target 2 no normal deltas, and no target lists blocks 1 and 2"""
    m = morph_case(prt, 86, 1)
    dense = m["targets"][0]
    pick = lambda corner: (np.array(corner, dtype=np.uint32), dense[1][corner], dense[2][corner])
    t2 = pick([3, 257])
    return m, [pick([0, 5, 200]), (np.zeros(0, dtype=np.uint32), np.zeros((0, 4), dtype=f32), None), (t2[0], t2[1], None)]


# ---- CPU: the builder ------------------------------------------------------------------------------------------------------------------------

def _check_table(emu, v0, n0, targets, T, what):
    for base_n in (None, n0):
        block_first, head, plane_p, plane_n, entries = emu.table(v0, base_n, targets, T)
        want = restate_planes(3 * T, targets, base_n is not None)
        assert entries == sum(len(t[0]) for t in targets), what
        assert block_first.shape == want[0].shape and np.array_equal(block_first, want[0]), what + ": block_first"
        assert head.shape == want[1].shape and np.array_equal(head, want[1]), what + ": plane_head"
        assert plane_p.shape == want[2].shape and np.array_equal(_bytes(plane_p), _bytes(want[2])), what + ": plane_p"
        assert (plane_n is None) == (base_n is None), what
        if plane_n is not None:
            assert plane_n.shape == want[3].shape and np.array_equal(_bytes(plane_n), _bytes(want[3])), what + ": plane_n"
    return want


@pytest.mark.parametrize("T,n_targets", [(1, 4), (22, 4), (64, 4), (86, 4), (T_TEAPOT, 4), (86, 1), (86, 257), (86, 65536)])
def test_builder_against_a_numpy_restatement(prt, emu, T, n_targets):
    """3, 66, 192, 258 and 18 960 corners; 1, 4, 257 and 65 536 targets (of the last only the last has an entry, on the last corner)"""
    m = morph_case(prt, T, n_targets)
    block_first, head, _, _ = _check_table(emu, m["v0"], m["n0"], m["targets"], T, "T = %d, %d targets" % (T, n_targets))
    assert len(block_first) == (3 * T + 63) // 64 + 1
    if n_targets == 4:
        assert m["targets"][1][2] is None, "a target with d_normal == NULL"
    if n_targets == 65536:
        assert len(head) == 1 and head[0].tolist() == [65535, 0, 2, 0] and block_first.tolist() == [0, 0, 0, 0, 0, 1]      # corner 257: block 4, lane 1
    ragged = 3 * T % 64
    if ragged:                                              # bits of lanes past 3T are 0
        last = head[int(block_first[-2]):]
        assert len(last) and all((int(lo) | int(hi) << 32) >> ragged == 0 for _, _, lo, hi in last)


def test_builder_on_an_empty_target_an_unlisted_block_and_a_target_without_normal_deltas(prt, emu):
    m, targets = _special_set(prt)
    block_first, head, plane_p, plane_n = _check_table(emu, m["v0"], m["n0"], targets, 86, "special")
    assert block_first.tolist() == [0, 2, 2, 2, 3, 4] and head[:, 0].tolist() == [0, 2, 0, 2]
    assert head[0].tolist() == [0, 0, 0x21, 0] and head[3].tolist() == [2, 0, 2, 0] and head[2].tolist() == [0, 0, 1 << 8, 0]
    assert not plane_n[[1, 3]].any() and plane_n[0].any()


# ---- CPU: the bodies -------------------------------------------------------------------------------------------------------------------------

def _check(emu, base_v, base_n, targets, weights, what, corners_emu=None):
    got_v, got_n = emu.morph(base_v, base_n, targets, weights)
    want_v, want_n = mirror_morph(base_v, base_n, targets, weights)
    assert np.array_equal(_bytes(got_v), _bytes(want_v)), what + ": vertices differ from the mirror"
    assert (got_n is None) == (want_n is None) and (got_n is None or np.array_equal(_bytes(got_n), _bytes(want_n))), what + ": normals differ from the mirror"
    if corners_emu is not None:
        ref_v, ref_n = corners_emu.morph(base_v, base_n, targets, weights)
        assert np.array_equal(_bytes(got_v), _bytes(ref_v)), what + ": vertices differ from the per-corner body"
        assert got_n is None or np.array_equal(_bytes(got_n), _bytes(ref_n)), what + ": normals differ from the per-corner body"
    return got_v, got_n


@pytest.mark.parametrize("with_normals", [True, False])
def test_body_equals_the_mirror_on_the_teapot(prt, emu, with_normals):
    """3 targets over random 5 % subsets (one with d_normal = NULL) and a dense one; the sparse ones alone; the dense one alone"""
    m = morph_case(prt, T_TEAPOT, 4)
    n0 = m["n0"] if with_normals else None
    got_v, _ = _check(emu, m["v0"], n0, m["targets"], m["weights"], "teapot, 4 targets")
    assert not got_v[:, 3].any()
    sparse = m["targets"][:3]
    got_v, _ = _check(emu, m["v0"], n0, sparse, m["weights"][:3], "teapot, sparse targets")
    untouched = np.setdiff1d(np.arange(3 * T_TEAPOT), np.concatenate([t[0] for t in sparse]))
    assert len(untouched) > 15000 and np.array_equal(_bytes(got_v[untouched, :3]), _bytes(m["v0"][untouched, :3]))
    _check(emu, m["v0"], n0, m["targets"][3:], m["weights"][3:], "teapot, one dense target")


@pytest.mark.parametrize("rigid", [False, True])
def test_fused_body_equals_the_pose_of_the_raw_morph(prt, emu, rigid):
    f = fused_case(prt, T_TEAPOT, rigid)
    s, m = f["s"], f["m"]
    for with_normals in (True, False):
        got_v, got_n = emu.pose_morphed(m["v0"], m["n0"] if with_normals else None, m["targets"], m["weights"], s["index"], s["weight"], s["M"])
        assert np.array_equal(_bytes(got_v), _bytes(f["v"])), "vertices differ from mirror_pose(mirror_morph_raw)"
        assert got_n is None if not with_normals else np.array_equal(_bytes(got_n), _bytes(f["n"])), "normals differ"
    got_v, got_n = emu.pose_morphed(m["v0"], m["n0"], m["targets"], m["weights"] * 0, s["index"], s["weight"], s["M"])
    assert np.array_equal(_bytes(got_v), _bytes(s["v"])) and np.array_equal(_bytes(got_n), _bytes(s["n"])), "all weights zero: the pose of the base"


def test_planted_cases_of_the_per_corner_layout(emu, corners_emu):
    """cases.planted() with its weight vectors: a -0 weight over NaN deltas, all zero, overflow, negative, a NaN weight"""
    v, n, targets = planted()
    w = np.array([0.5, np.nan, -0.0, 1.0, 1.0], dtype=f32)
    got_v, got_n = _check(emu, v, n, targets, w, "planted", corners_emu)
    assert np.isfinite(got_v).all() and np.isfinite(got_n).all(), "the NaN deltas were used under a zero weight"
    assert np.signbit(got_v[0, 0]) and np.signbit(got_v[0, 2]), "no entry: -0 kept"
    got_v, _ = _check(emu, v, n, targets, np.array([0, -0.0, 0, -0.0, 0], dtype=f32), "all weights zero", corners_emu)
    assert np.array_equal(_bytes(got_v[:, :3]), _bytes(v[:, :3]))
    got_v, _ = _check(emu, v, n, targets, np.array([-0.5, 0, 0, 4.0, -2.0], dtype=f32), "overflow, negative weights", corners_emu)
    assert np.isinf(got_v[4, 0]) and np.isfinite(got_v[[0, 1, 2, 3, 5]]).all()
    got_v, _ = _check(emu, v, n, targets, np.array([np.nan, 0, 0, 1, 1], dtype=f32), "a NaN weight", corners_emu)
    assert np.isnan(got_v[[1, 2, 3], :3]).all() and np.isfinite(got_v[[0, 4, 5]]).all()
    idx = np.zeros((6, 4), dtype=np.uint16)
    bw = np.tile(np.array([1, 0, 0, 0], dtype=f32), (6, 1))
    for base_n in (n, None):
        got = emu.pose_morphed(v, base_n, targets, w, idx, bw, identity(1))
        raw_p, raw_n = mirror_morph_raw(v, base_n, targets, w)
        want = mirror_pose(raw_p, raw_n, idx, bw, identity(1))
        assert np.array_equal(_bytes(got[0]), _bytes(want[0])) and (base_n is None or np.array_equal(_bytes(got[1]), _bytes(want[1])))


def planted_planes(prt):
    """43 triangles, 129 corners: blocks 0 and 1 and one lane of block 2.  Target 0: corners 63 and 64, the two sides of a block boundary.
    Target 1: lanes 31 and 32 of block 1, the two halves of the mask.  Target 2: lanes 0 and 63 of block 0.  Target 3: corner 70 alone; the
    base x of corners 71 and 100, unlisted lanes of planes of block 1, is -0.  Target 4: corner 69 alone, for a NaN weight.  Target 5: corner
    128, the ragged block's only lane"""
    case = teapot(prt)
    v, n = case.v0[:129].copy(), case.n0[:129].copy()
    v[71, 0] = v[100, 0] = -0.0
    rng = np.random.default_rng(3)

    def target(corner):
        dp, dn = np.zeros((len(corner), 4), dtype=f32), np.zeros((len(corner), 4), dtype=f32)
        dp[:, :3], dn[:, :3] = rng.uniform(-0.03, 0.03, (len(corner), 3)), rng.uniform(-0.3, 0.3, (len(corner), 3))
        return np.array(corner, dtype=np.uint32), dp, dn
    return v, n, [target(c) for c in ([63, 64], [95, 96], [0, 63], [70], [69], [128])]


def test_planted_cases_of_the_plane_layout(prt, emu, corners_emu):
    v, n, targets = planted_planes(prt)
    block_first, head, _, _, entries = emu.table(v, n, targets, 43)
    assert block_first.tolist() == [0, 2, 6, 7] and entries == 9
    assert head.tolist() == [[0, 0, 0, 1 << 31], [2, 0, 1, 1 << 31], [0, 0, 1, 0], [1, 0, 1 << 31, 1], [3, 0, 1 << 6, 0], [4, 0, 1 << 5, 0], [5, 0, 1, 0]]
    ones = np.ones(6, dtype=f32)
    for k in range(6):                                       # each target alone: exactly its corners move, by its deltas
        w = np.zeros(6, dtype=f32)
        w[k] = 1
        got_v, got_n = _check(emu, v, n, targets, w, "target %d alone" % k, corners_emu)
        moved = np.flatnonzero((_bytes(got_v[:, :3]).reshape(129, -1) != _bytes(v[:, :3]).reshape(129, -1)).any(axis=1))
        assert moved.tolist() == targets[k][0].tolist(), (k, moved)
        assert np.array_equal(got_v[targets[k][0], :3], v[targets[k][0], :3] + targets[k][1][:, :3])
    got_v, _ = _check(emu, v, n, targets, ones, "all active", corners_emu)
    assert np.signbit(got_v[71, 0]) and got_v[71, 0] == 0 and np.signbit(got_v[100, 0]), "an unlisted lane of a plane of weight 1 keeps its -0"
    w = ones.copy()
    w[4] = np.nan
    got_v, got_n = _check(emu, v, n, targets, w, "a NaN weight on a plane with one listed lane", corners_emu)
    assert np.flatnonzero(np.isnan(got_v).any(axis=1)).tolist() == [69] and np.flatnonzero(np.isnan(got_n).any(axis=1)).tolist() == [69]
    w[4] = np.inf
    got_v, _ = _check(emu, v, n, targets, w, "an infinite weight", corners_emu)
    assert np.flatnonzero(~np.isfinite(got_v).all(axis=1)).tolist() == [69]
    _check(emu, v, None, targets, ones, "no base normals", corners_emu)
    # 257 targets that all list corner 0 (and nothing else): 257 planes in block 0, added in ascending t
    rng = np.random.default_rng(4)
    many = []
    for t in range(257):
        dp, dn = np.zeros((1, 4), dtype=f32), np.zeros((1, 4), dtype=f32)
        dp[0, :3], dn[0, :3] = rng.uniform(-1, 1, 3), rng.uniform(-1, 1, 3)
        many.append((np.zeros(1, dtype=np.uint32), dp, dn if t % 3 else None))
    w = rng.uniform(-1, 1, 257).astype(f32)
    w[5::11] = 0
    assert emu.table(v, n, many, 43)[0].tolist() == [0, 257, 257, 257]
    got_v, _ = _check(emu, v, n, many, w, "257 targets on corner 0", corners_emu)
    assert np.array_equal(_bytes(got_v[1:, :3]), _bytes(v[1:, :3]))
    got_v, _ = _check(emu, v, n, many, w[::-1].copy(), "257 targets on corner 0, other weights", corners_emu)


@pytest.mark.parametrize("T,n_targets", [(86, 4), (T_TEAPOT, 4), (86, 65536), (64, 1)])
def test_report_arithmetic(prt, emu, T, n_targets):
    m = morph_case(prt, T, n_targets)
    entries = sum(len(t[0]) for t in m["targets"])
    planes = len(restate_planes(3 * T, m["targets"], False)[1])
    for base_n in (m["n0"], None):
        for layout in (CORNERS, PLANES):
            rep = emu.report(m["v0"], base_n, m["targets"], T, layout)
            p = planes if layout == PLANES else 0
            assert rep == {"layout": layout, "n_targets": n_targets, "entries": entries, "planes": p,
                           "table_bytes": table_bytes(layout, T, entries, p, base_n is not None)}, (layout, rep)
    if (T, n_targets) == (64, 1):                           # one dense target over three full blocks, with normals
        assert emu.report(m["v0"], m["n0"], m["targets"], T, PLANES)["table_bytes"] == 4 * 4 + 16 * 3 + 1536 * 3
        assert emu.report(m["v0"], m["n0"], m["targets"], T, CORNERS)["table_bytes"] == 4 * 193 + 32 * 192


def test_api_is_declared_exported_and_bound(prt):
    import re
    header = assert_api(NAMES, prt)
    assert re.search(r"#define\s+PRT_MORPH_LAYOUT_CORNERS\s+0u", header) and re.search(r"#define\s+PRT_MORPH_LAYOUT_PLANES\s+1u", header)
    assert C.sizeof(prt._capi.MorphReport) == 32
    assert callable(prt.Renderer.morph_report)


# ---- GPU -------------------------------------------------------------------------------------------------------------------------------------

def _set(r, m, layout="planes", normals=True):
    r.set_morph_targets(m["v0"], m["n0"] if normals else None, m["targets"], layout=layout)


@pytest.mark.gpu
@pytest.mark.parametrize("T,n_targets", [(T, nt) for T in (1, 22, 64, 86, T_TEAPOT) for nt in (1, 3, 257)] + [(86, 65536)])
def test_morphed_buffers_equal_the_mirror_and_the_per_corner_layout_through_both_doors(prt, T, n_targets):
    import torch
    m = morph_case(prt, T, n_targets)
    r = _context(prt, m)
    got = {}
    for layout in ("planes", "corners"):
        for door in ("host", "device"):
            _set(r, m, layout)                                 # (set again: the morphed buffers are new ones)
            assert r.lib.prt_read_morphed(r.ctx, np.zeros(12 * T, dtype=f32).ctypes.data_as(C.c_void_p), None) == prt.PRT_ERR_NOT_READY
            r.morph(m["weights"] if door == "host" else torch.from_numpy(m["weights"].copy()).cuda(), rebuild=(door == "device"), max_leaf=4)
            got[layout, door] = r.read_morphed()
    r.close()
    for door in ("host", "device"):
        v, n = got["planes", door]
        assert np.array_equal(_bytes(v), _bytes(m["v"])), "%s door: morphed vertices differ from the mirror" % door
        assert np.array_equal(_bytes(n), _bytes(m["n"])), "%s door: morphed normals differ from the mirror" % door
        assert np.array_equal(_bytes(v), _bytes(got["corners", door][0])) and np.array_equal(_bytes(n), _bytes(got["corners", door][1])), \
            "%s door: the two layouts differ" % door


@pytest.mark.gpu
@pytest.mark.parametrize("rigid", [True, False])
@pytest.mark.parametrize("T", [1, 22, 86, T_TEAPOT])
def test_posed_buffers_after_pose_morphed_equal_the_mirror(prt, T, rigid):
    import torch
    f = fused_case(prt, T, rigid)
    s, m = f["s"], f["m"]
    r = _context(prt, m)
    _set(r, m)
    for door in ("host", "device"):
        r.set_skin(s["v0"] * 0 + 9, s["n0"] * 0 + 9, s["index"], s["weight"], 4)       # (the skin's rest arrays are not read)
        if door == "host":
            r.pose_morphed(s["M"], m["weights"], rebuild=False)
        else:
            r.pose_morphed(torch.from_numpy(s["M"].copy()).cuda(), torch.from_numpy(m["weights"].copy()).cuda(), rebuild=True, max_leaf=4)
        v, n = r.read_posed()
        assert np.array_equal(_bytes(v), _bytes(f["v"])), "%s door: vertices differ from mirror_pose(mirror_morph_raw)" % door
        assert np.array_equal(_bytes(n), _bytes(f["n"])), "%s door: normals differ" % door
    _refused(prt, lambda: r.read_morphed(), prt.PRT_ERR_NOT_READY)                      # (the set's own buffers were never written)
    r.close()


@pytest.mark.gpu
@pytest.mark.parametrize("fused", [False, True])
@pytest.mark.parametrize("mode", [REFIT, REBUILD])
@pytest.mark.parametrize("mesh", ["86 under a leaf root", "teapot under its tree"])
def test_scene_after_a_morph_equals_an_update_with_the_mirrors_arrays(prt, mode, mesh, fused):
    T = 86 if mesh.startswith("86") else T_TEAPOT
    f = fused_case(prt, T, False)
    s, m = f["s"], f["m"]
    want = f if fused else m
    got = []
    for morphed in (True, False):
        r = _context(prt, m, leaf_root=mesh.startswith("86"))
        if morphed:
            _set(r, m)
            if fused:
                _skin(r, s)
            before = _scene(r)
            assert np.array_equal(_bytes(before["normals"][:, :3]), _bytes(m["n0"][:, :3])), "setting the targets changes nothing by itself"
            if fused:
                r.pose_morphed(s["M"], m["weights"], rebuild=(mode == REBUILD), max_leaf=4)
            else:
                r.morph(m["weights"], rebuild=(mode == REBUILD), max_leaf=4)
        elif mode == REFIT:
            r.update_vertices(want["v"], want["n"])
        else:
            r.rebuild_bvh(want["v"], want["n"], max_leaf=4)
        got.append(_everything(prt, r))
        r.close()
    assert np.array_equal(_bytes(got[0]["normals"]), _bytes(want["n"]))
    _assert_equal(got[0], got[1], "%s, mode %d, fused %s" % (mesh, mode, fused))


def _second_weights(m):
    return np.ascontiguousarray(m["weights"][::-1] * f32(0.5))


@pytest.mark.gpu
def test_replacement_report_and_lifetime(prt, emu):
    m = morph_case(prt, T_TEAPOT, 3)
    w2 = _second_weights(m)
    v2, n2 = mirror_morph(m["v0"], m["n0"], m["targets"], w2)
    case = teapot(prt)

    def fresh(layout, w):
        r = _context(prt, m, leaf_root=False)
        _set(r, m, layout)
        r.morph(w)
        out = _scene(r)
        out["morphed_v"], out["morphed_n"] = r.read_morphed()
        r.close()
        return out

    def now(r):
        out = _scene(r)
        out["morphed_v"], out["morphed_n"] = r.read_morphed()
        return out
    r = _context(prt, m, leaf_root=False)
    _refused(prt, lambda: r.morph_report(), prt.PRT_ERR_NOT_READY)
    # corners -> planes -> corners on one context, each morph equal to a fresh context's
    for step, (layout, w, want) in enumerate((("corners", m["weights"], (m["v"], m["n"])), ("planes", w2, (v2, n2)), ("corners", m["weights"], (m["v"], m["n"])),
                                              ("planes", m["weights"], (m["v"], m["n"])))):
        _set(r, m, layout)
        _refused(prt, lambda: r.read_morphed(), prt.PRT_ERR_NOT_READY)                  # (a new set: nothing morphed yet)
        rep = r.morph_report()
        want_rep = emu.report(m["v0"], m["n0"], m["targets"], T_TEAPOT, PLANES if layout == "planes" else CORNERS)
        assert {k: rep[k] for k in want_rep} == dict(want_rep, layout=layout), (step, rep)
        assert rep["fill"] == (rep["entries"] / (64.0 * rep["planes"]) if layout == "planes" else None)
        r.morph(w)
        got = now(r)
        assert np.array_equal(_bytes(got["morphed_v"]), _bytes(want[0])) and np.array_equal(_bytes(got["morphed_n"]), _bytes(want[1])), step
        _assert_equal(got, fresh(layout, w), "step %d, %s" % (step, layout))
    # an unknown layout is refused: the set in force, the morphed buffers and the report stay
    rep, before = r.morph_report(), now(r)
    _refused(prt, lambda: r.set_morph_targets(m["v0"], m["n0"], m["targets"], layout=2))
    assert r.lib.prt_set_morph_targets_layout(r.ctx, None, 7) == prt.PRT_ERR_INVALID_ARGUMENT, "tested before the NULL test"
    assert r.lib.prt_get_morph_report(r.ctx, None) == prt.PRT_ERR_INVALID_ARGUMENT
    assert r.morph_report() == rep
    _assert_equal(now(r), before, "an unknown layout")
    r.morph(w2)
    assert np.array_equal(_bytes(r.read_morphed()[0]), _bytes(v2)), "the plane set still morphs"
    # NULL through either entry point turns the set off
    assert r.lib.prt_set_morph_targets_layout(r.ctx, None, PLANES) == prt.PRT_OK
    assert r.lib.prt_morph(r.ctx, m["weights"].ctypes.data_as(C.c_void_p), REFIT, 0) == prt.PRT_ERR_NOT_READY
    _refused(prt, lambda: r.morph_report(), prt.PRT_ERR_NOT_READY)
    _set(r, m)
    assert r.lib.prt_set_morph_targets(r.ctx, None) == prt.PRT_OK
    _refused(prt, lambda: r.morph_report(), prt.PRT_ERR_NOT_READY)
    _set(r, m)
    assert r.lib.prt_set_morph_targets_layout(r.ctx, None, CORNERS) == prt.PRT_OK
    assert r.lib.prt_read_morphed(r.ctx, m["v"].copy().ctypes.data_as(C.c_void_p), None) == prt.PRT_ERR_NOT_READY
    # the set survives what the per-corner set survives; prt_upload_scene turns it off
    _set(r, m)
    r.render_frames(prt.seed_pairs(4))
    r.reset()
    r.resize(W + 3, H - 1)
    r.set_camera(case.cam)
    r.set_tile(W, H, 8, 16)
    r.resize(W, H)
    r.update_vertices(v2, n2)
    r.rebuild_bvh(m["v0"], m["n0"], max_leaf=4)
    r.morph(m["weights"])
    v, n = r.read_morphed()
    assert np.array_equal(_bytes(v), _bytes(m["v"])) and np.array_equal(_bytes(n), _bytes(m["n"]))
    assert np.array_equal(_bytes(r.read_normals()), _bytes(m["n"])), "a morph after a rebuild refits the new topology"
    r.upload_scene(case.desc)
    assert r.lib.prt_morph(r.ctx, m["weights"].ctypes.data_as(C.c_void_p), REFIT, 0) == prt.PRT_ERR_NOT_READY
    assert r.lib.prt_get_morph_report(r.ctx, C.byref(prt._capi.MorphReport())) == prt.PRT_ERR_NOT_READY
    r.close()
    r = prt.Renderer(case.cfg, device=0)
    _refused(prt, lambda: _set(r, m), prt.PRT_ERR_NOT_READY)                            # no scene: before the layout is looked at
    assert r.lib.prt_set_morph_targets_layout(r.ctx, None, 7) == prt.PRT_ERR_NOT_READY
    r.close()


@pytest.mark.gpu
def test_refusals_leave_the_scene_the_set_and_a_pending_snapshot_as_they_were(prt):
    import torch
    m = morph_case(prt, T_TEAPOT, 3)
    r = _context(prt, m, leaf_root=False)
    r.set_motion(True)
    _set(r, m)
    r.morph(m["weights"])                                                              # (a snapshot is pending from here on)
    want = _scene(r)
    assert np.array_equal(_bytes(want["normals"]), _bytes(m["n"]))
    dev = torch.zeros(8, dtype=torch.float32, device="cuda")
    dev[1:4] = torch.from_numpy(m["weights"].copy()).cuda()

    def still(what, morphed_too=True):
        _assert_equal(_scene(r), want, what)
        assert r.morph_report()["layout"] == "planes"
        if morphed_too:
            v, n = r.read_morphed()
            assert np.array_equal(_bytes(v), _bytes(m["v"])) and np.array_equal(_bytes(n), _bytes(m["n"])), what + ": the morphed buffers changed"

    _refused(prt, lambda: r.morph(m["weights"], rebuild=2))
    still("an unknown mode")
    assert dev.data_ptr() % 16 == 0
    _refused(prt, lambda: r.morph(dev.data_ptr() + 4))
    still("a misaligned device pointer")
    for what, (t, value) in (("a NaN weight", (0, np.nan)), ("an infinite weight", (2, np.inf))):
        w = m["weights"].copy()
        w[t] = value
        for rebuild in (False, True):
            _refused(prt, lambda: r.morph(w, rebuild=rebuild, max_leaf=4))
            still(what, morphed_too=False)
        v, n = r.read_morphed()
        assert not np.isfinite(v).all(), what + ": prt_read_morphed returns the refused morph"
        assert np.array_equal(_bytes(v), _bytes(mirror_morph(m["v0"], m["n0"], m["targets"], w)[0]))
    # the set still morphs to the same bytes, and the pending snapshot is still the base's: the motion plane equals that of a context that
    # morphed twice and was never refused
    r.morph(m["weights"])
    still("after the refusals")
    r.render_guides(2)
    motion = r.read_motion()
    r.close()
    r = _context(prt, m, leaf_root=False)
    r.set_motion(True)
    _set(r, m)
    r.morph(m["weights"])
    r.morph(m["weights"])
    r.render_guides(2)
    assert motion.any() and np.array_equal(_bytes(motion), _bytes(r.read_motion()))
    r.close()


@pytest.mark.gpu
def test_row_block_contexts_that_each_set_planes_and_morph(prt):
    m = morph_case(prt, T_TEAPOT, 3)

    def run(part):
        r = _context(prt, m, leaf_root=False)
        if part is not None:
            r.set_row_blocks(W, H, 8, 2, part)
        _set(r, m)
        r.morph(m["weights"], rebuild=True, max_leaf=4)
        r.reset()
        r.render_frames(prt.seed_pairs(FRAMES))
        out = r.read_state(), r.read_framebuffer()
        r.close()
        return out
    state, img = run(None)
    got_state, got_img = np.zeros_like(state).reshape(H, W), np.zeros_like(img)
    for part in range(2):
        rows = [y for y in range(H) if (y // 8) % 2 == part]
        st, im = run(part)
        got_state[rows], got_img[rows] = st.reshape(len(rows), W), im
    assert np.array_equal(_bytes(got_state), _bytes(state)) and np.array_equal(_bytes(got_img), _bytes(img)), "two row-block contexts"
