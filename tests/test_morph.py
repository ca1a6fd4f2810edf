"""prt_set_morph_targets / prt_morph / prt_pose_morphed: the mesh morphed on the device from per-frame target weights, alone or in front of
the skin (include/prt.h; csrc/hip/pt_morph.h / .hip).

`mirror_morph_raw` (tests/mirrors.py) restates prt.h's formulas in float32 numpy -- a loop over the targets in ascending t, a target whose weight is zero
skipped, otherwise p[corner_t] = p[corner_t] + w * dp_t as one fancy-indexed statement (a target's corners are distinct) -- and shares no
code with the body.  `mirror_morph` adds prt_morph's output rule; the fused case feeds the raw output to mirror_pose.  The body
(run on the host by tests/emu/morph_emu.cpp, over the table the library's own builder makes) and the device (through the C ABI) must give
its bytes.

CPU tests: the bodies against the mirror on the teapot and on planted cases, the checks of prt_set_morph_targets, the table builder against a
numpy stable sort.  GPU tests: prt_read_morphed / prt_read_posed against the mirror at the sizes where a one-lane-per-corner kernel can go
wrong (3, 66, 258 and 18 960 corners; 1, 3, 257 and 65 536 targets), and the scene after a morph against a second context that was given the
mirror's arrays through prt_update_vertices / prt_rebuild_bvh."""
import ctypes as C

import numpy as np
import pytest

from cases import (_assert_equal, _everything, fused_case, identity, morph_cache as _cache, morph_case, planted, pose_context as _context,
                   POSE_FRAME, pose_scene as _scene, REBUILD, REFIT, _refused, _skin, T_TEAPOT, teapot)
from mirrors import mirror_morph, mirror_morph_raw, mirror_pose
from support import assert_api, bytes_flat as _bytes

f32 = np.float32
W, H, FRAMES = POSE_FRAME
NAMES = ("prt_set_morph_targets", "prt_morph", "prt_morph_device", "prt_pose_morphed", "prt_pose_morphed_device", "prt_read_morphed")


@pytest.fixture(scope="module")
def emu():
    import morph_api
    morph_api.lib()
    return morph_api


# ---- CPU: the bodies on the host -------------------------------------------------------------------------------------------------------------

def _check(emu, base_v, base_n, targets, weights, what):
    got_v, got_n = emu.morph(base_v, base_n, targets, weights)
    want_v, want_n = mirror_morph(base_v, base_n, targets, weights)
    assert np.array_equal(_bytes(got_v), _bytes(want_v)), what + ": vertices differ from the mirror"
    assert (got_n is None) == (want_n is None) and (got_n is None or np.array_equal(_bytes(got_n), _bytes(want_n))), what + ": normals differ from the mirror"
    return got_v, got_n


@pytest.mark.parametrize("with_normals", [True, False])
def test_body_equals_the_mirror_on_the_teapot(prt, emu, with_normals):
    """3 targets over random 5 % subsets (one with d_normal = NULL) and a dense one"""
    m = morph_case(prt, T_TEAPOT, 4)
    assert [len(t[0]) for t in m["targets"]] == [948, 948, 948, 18960] and m["targets"][1][2] is None
    assert emu.check(m["v0"], m["n0"] if with_normals else None, m["targets"], T_TEAPOT) == 0
    got_v, got_n = _check(emu, m["v0"], m["n0"] if with_normals else None, m["targets"], m["weights"], "teapot, 4 targets")
    assert not got_v[:, 3].any()
    if with_normals:
        length = np.linalg.norm(got_n[:, :3].astype(np.float64), axis=1)
        assert np.abs(length - 1).max() < 1e-6 and not got_n[:, 3].any()
    sparse = m["targets"][:3]                                # without the dense target most corners keep their base bits
    got_v, _ = _check(emu, m["v0"], None, sparse, m["weights"][:3], "teapot, sparse targets")
    untouched = np.setdiff1d(np.arange(3 * T_TEAPOT), np.concatenate([t[0] for t in sparse]))
    assert len(untouched) > 15000 and np.array_equal(_bytes(got_v[untouched, :3]), _bytes(m["v0"][untouched, :3]))


@pytest.mark.parametrize("rigid", [False, True])
def test_fused_body_equals_the_pose_of_the_raw_morph(prt, emu, rigid):
    f = fused_case(prt, T_TEAPOT, rigid)
    s, m = f["s"], f["m"]
    for with_normals in (True, False):
        got_v, got_n = emu.pose_morphed(m["v0"], m["n0"] if with_normals else None, m["targets"], m["weights"], s["index"], s["weight"], s["M"])
        assert np.array_equal(_bytes(got_v), _bytes(f["v"])), "vertices differ from mirror_pose(mirror_morph_raw)"
        assert got_n is None if not with_normals else np.array_equal(_bytes(got_n), _bytes(f["n"])), "normals differ"
    # all weights zero: the pose of the base
    got_v, got_n = emu.pose_morphed(m["v0"], m["n0"], m["targets"], m["weights"] * 0, s["index"], s["weight"], s["M"])
    assert np.array_equal(_bytes(got_v), _bytes(s["v"])) and np.array_equal(_bytes(got_n), _bytes(s["n"]))


def test_planted_cases(emu):
    v, n, targets = planted()
    assert emu.check(v, n, targets, 2) == -1, "the NaN deltas are refused by prt_set_morph_targets (the body is run over them all the same)"
    assert emu.check(v, n, targets[:2] + targets[3:], 2) == 0
    w = np.array([0.5, np.nan, -0.0, 1.0, 1.0], dtype=f32)                            # (a NaN weight under a target without entries is harmless)
    got_v, got_n = _check(emu, v, n, targets, w, "planted")
    assert np.isfinite(got_v).all() and np.isfinite(got_n).all(), "the NaN deltas were used under a zero weight"
    assert np.array_equal(_bytes(got_v[0, :3]), _bytes(v[0, :3])) and np.signbit(got_v[0, 0]) and np.signbit(got_v[0, 2]), "no entry: base bits, -0 kept"
    assert np.array_equal(_bytes(got_n[0, :3]), _bytes(np.array([0, 0.6, 0.8], dtype=f32))), "no entry: the base normal renormalised"
    assert not got_v[:, 3].any() and not got_n[:, 3].any()
    assert np.array_equal(got_v[1, :3], np.array([0.625, -0.75, 4.75], dtype=f32)), "a corner every target lists, in ascending t"
    assert not _bytes(got_n[2, :3]).any(), "0.5 + 0.5 * -1: L == 0 keeps n = +0"
    assert got_v[3, 0] != 0 and np.array_equal(_bytes(got_v[3, :3]), _bytes(v[3, :3] + f32(0.5) * targets[0][1][2, :3])), "denormal deltas"
    assert np.array_equal(got_v[5, :3], v[5, :3] + f32(1)) and not _bytes(got_n[5, :3]).any(), "the end of the table"
    # all weights zero, of either sign: every corner keeps its base bits
    got_v, got_n = _check(emu, v, n, targets, np.array([0, -0.0, 0, -0.0, 0], dtype=f32), "all weights zero")
    assert np.array_equal(_bytes(got_v[:, :3]), _bytes(v[:, :3]))
    # a weight that overflows a coordinate is passed on (the refusal is the finite-vertex check's, downstream); negative weights
    got_v, _ = _check(emu, v, n, targets, np.array([-0.5, 0, 0, 4.0, -2.0], dtype=f32), "overflow, negative weights")
    assert np.isinf(got_v[4, 0]) and np.isfinite(got_v[[0, 1, 2, 3, 5]]).all()
    # ... and a NaN weight under a listed target
    got_v, _ = _check(emu, v, n, targets, np.array([np.nan, 0, 0, 1, 1], dtype=f32), "a NaN weight")
    assert np.isnan(got_v[[1, 2, 3], :3]).all() and np.isfinite(got_v[[0, 4, 5]]).all()
    # the fused body over the planted set, and over the set without normals
    idx = np.zeros((6, 4), dtype=np.uint16)
    bw = np.tile(np.array([1, 0, 0, 0], dtype=f32), (6, 1))
    for base_n in (n, None):
        got = emu.pose_morphed(v, base_n, targets, w, idx, bw, identity(1))
        raw_p, raw_n = mirror_morph_raw(v, base_n, targets, w)
        want = mirror_pose(raw_p, raw_n, idx, bw, identity(1))
        assert np.array_equal(_bytes(got[0]), _bytes(want[0])) and (base_n is None or np.array_equal(_bytes(got[1]), _bytes(want[1])))
        assert not np.signbit(got[0][0, 0]), "the pose adds + 0: a -0 becomes +0 there, as in prt_pose"


def test_set_checks(prt, emu):
    INVALID, UNSUPPORTED = prt.PRT_ERR_INVALID_ARGUMENT, prt.PRT_ERR_UNSUPPORTED
    m = morph_case(prt, 22, 3)
    v, n, tg = m["v0"], m["n0"], m["targets"]
    assert emu.check(v, n, tg, 22) == 0 and emu.check(v, None, tg, 22) == 0 and emu.lib().morph_emu_max_targets() == 65536
    assert emu.check(None, n, tg, 22) == INVALID and emu.check(v, n, None, 22, n_targets=3) == INVALID
    assert emu.check(v, n, tg, 22, n_targets=0) == INVALID and emu.check(v, n, tg, 22, n_targets=65537) == INVALID
    empty = (None, None, None)
    assert emu.check(v, n, [tg[0], empty, tg[2]], 22) == 0, "n_entries = 0 needs no arrays"
    assert emu.check(v, n, [(None, tg[0][1], tg[0][2])] + tg[1:], 22, n_entries=[3, 3, 66]) == INVALID
    assert emu.check(v, n, [(tg[0][0], None, tg[0][2])] + tg[1:], 22) == INVALID
    assert emu.check(v, n, [(tg[0][0], tg[0][1], None)] + tg[1:], 22) == 0
    dense = tg[2]
    for bad_corner in ([66], [5, 5], [7, 6], [0, 1, 0xFFFFFFFF]):
        k = len(bad_corner)
        assert emu.check(v, n, [tg[0], tg[1], (np.array(bad_corner, dtype=np.uint32), dense[1][:k], dense[2][:k])], 22) == INVALID, bad_corner
    assert emu.check(v, n, [tg[0], tg[1], (np.array([64, 65], dtype=np.uint32), dense[1][:2], dense[2][:2])], 22) == 0
    for bad in (np.nan, np.inf, -np.inf):
        for lane in range(3):
            for which in ("v", "n", "dp", "dn"):
                a = {"v": v.copy(), "n": n.copy(), "dp": dense[1].copy(), "dn": dense[2].copy()}
                a[which][40, lane] = bad
                assert emu.check(a["v"], a["n"], [tg[0], tg[1], (dense[0], a["dp"], a["dn"])], 22) == INVALID, (which, bad, lane)
    a = {"v": v.copy(), "n": n.copy(), "dp": dense[1].copy(), "dn": dense[2].copy()}
    for x in a.values():
        x[:, 3] = np.nan                                                               # (lane 3 is never looked at)
    assert emu.check(a["v"], a["n"], [tg[0], tg[1], (dense[0], a["dp"], a["dn"])], 22) == 0
    bad_dn = dense[2].copy()
    bad_dn[3, 1] = np.nan
    assert emu.check(v, None, [tg[0], tg[1], (dense[0], dense[1], bad_dn)], 22) == 0, "d_normal is not read when the set has no base normals"
    # more than 2^32 - 1 entries in total: 65 535 targets that all point to the same 65 538 entries are 2^32 + 65 534 (refused before
    # anything is read)
    T = 21846
    big = (np.arange(3 * T, dtype=np.uint32), np.zeros((3 * T, 4), dtype=f32), None)
    base = np.zeros((3 * T, 4), dtype=f32)
    assert emu.check(base, None, [big] * 65536, T) == UNSUPPORTED and emu.check(base, None, [big] * 65535, T) == UNSUPPORTED
    assert emu.check(base, None, [big], T - 1) == INVALID, "more entries than corners"


@pytest.mark.parametrize("n_targets", [1, 4, 257, 65536])
def test_table_builder_against_a_stable_sort(prt, emu, n_targets):
    m = morph_case(prt, 86, n_targets)
    offset, entry_p, entry_n = emu.table(m["v0"], m["n0"], m["targets"], 86)
    corner = np.concatenate([t[0] for t in m["targets"]]).astype(np.int64)
    target = np.concatenate([np.full(len(t[0]), k, dtype=np.uint32) for k, t in enumerate(m["targets"])])
    dp = np.concatenate([t[1] for t in m["targets"]])
    dn = np.concatenate([np.zeros((len(t[0]), 4), dtype=f32) if t[2] is None else t[2] for t in m["targets"]])
    order = np.argsort(corner, kind="stable")
    assert np.array_equal(offset, np.concatenate([[0], np.cumsum(np.bincount(corner, minlength=258))]).astype(np.uint32))
    assert np.array_equal(entry_p.view(np.uint32)[:, 3], target[order]), "entries sorted by (corner, target)"
    assert np.array_equal(_bytes(entry_p[:, :3]), _bytes(dp[order][:, :3])) and np.array_equal(_bytes(entry_n[:, :3]), _bytes(dn[order][:, :3]))
    assert not entry_n[:, 3].any() and emu.table(m["v0"], None, m["targets"], 86)[2] is None


def test_api_is_declared_exported_and_bound(prt):
    assert_api(NAMES, prt)
    assert C.sizeof(prt._capi.MorphTarget) == 32 and C.sizeof(prt._capi.MorphSet) == 32
    for method in ("set_morph_targets", "morph", "pose_morphed", "read_morphed"):
        assert callable(getattr(prt.Renderer, method))


# ---- GPU -------------------------------------------------------------------------------------------------------------------------------------

def _set(r, m, normals=True):
    r.set_morph_targets(m["v0"], m["n0"] if normals else None, m["targets"])


@pytest.mark.gpu
@pytest.mark.parametrize("T,n_targets", [(T, nt) for T in (1, 22, 86, T_TEAPOT) for nt in (1, 3, 257)] + [(86, 65536)])
def test_morphed_buffers_equal_the_mirror_through_both_doors(prt, T, n_targets):
    """3, 66, 258 and 18 960 corners: less than a wave, across a wave, across a block, many blocks"""
    import torch
    m = morph_case(prt, T, n_targets)
    r = _context(prt, m)
    _set(r, m)
    assert r.lib.prt_read_morphed(r.ctx, np.zeros(12 * T, dtype=f32).ctypes.data_as(C.c_void_p), None) == prt.PRT_ERR_NOT_READY
    for door in ("host", "device"):
        r.morph(m["weights"] if door == "host" else torch.from_numpy(m["weights"].copy()).cuda(), rebuild=(door == "device"), max_leaf=4)
        v, n = r.read_morphed()
        assert np.array_equal(_bytes(v), _bytes(m["v"])), "%s door: morphed vertices differ from the mirror" % door
        assert np.array_equal(_bytes(n), _bytes(m["n"])), "%s door: morphed normals differ from the mirror" % door
        _set(r, m)                                             # (set again: the morphed buffers are new ones)
    r.close()


@pytest.mark.gpu
@pytest.mark.parametrize("rigid", [True, False])
@pytest.mark.parametrize("T", [1, 22, 86, T_TEAPOT])
def test_posed_buffers_after_pose_morphed_equal_the_mirror(prt, T, rigid):
    import torch
    f = fused_case(prt, T, rigid)
    s, m = f["s"], f["m"]
    r = _context(prt, m)
    _set(r, m)
    r.set_skin(s["v0"] * 0 + 9, s["n0"] * 0 + 9, s["index"], s["weight"], 4)           # (the skin's rest arrays are not read)
    for door in ("host", "device"):
        if door == "host":
            r.pose_morphed(s["M"], m["weights"], rebuild=False)
        else:
            r.pose_morphed(torch.from_numpy(s["M"].copy()).cuda(), torch.from_numpy(m["weights"].copy()).cuda(), rebuild=True, max_leaf=4)
        v, n = r.read_posed()
        assert np.array_equal(_bytes(v), _bytes(f["v"])), "%s door: vertices differ from mirror_pose(mirror_morph_raw)" % door
        assert np.array_equal(_bytes(n), _bytes(f["n"])), "%s door: normals differ" % door
        r.set_skin(s["v0"] * 0 + 9, s["n0"] * 0 + 9, s["index"], s["weight"], 4)
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


@pytest.mark.gpu
@pytest.mark.parametrize("mode", [REFIT, REBUILD])
def test_zero_weights_over_the_rest_pose_leave_the_scene_of_a_pose(prt, mode):
    f = fused_case(prt, T_TEAPOT, False)
    s, m = f["s"], f["m"]
    got = []
    for morphed in (True, False):
        r = _context(prt, s, leaf_root=False)
        _skin(r, s)
        if morphed:
            _set(r, m)
            r.pose_morphed(s["M"], m["weights"] * 0, rebuild=(mode == REBUILD), max_leaf=4)
        else:
            r.pose(s["M"], rebuild=(mode == REBUILD), max_leaf=4)
        v, n = r.read_posed()
        assert np.array_equal(_bytes(v), _bytes(s["v"])) and np.array_equal(_bytes(n), _bytes(s["n"]))
        got.append(_everything(prt, r))
        r.close()
    _assert_equal(got[0], got[1], "all weights zero, mode %d" % mode)


@pytest.mark.gpu
@pytest.mark.parametrize("mode", [REFIT, REBUILD])
@pytest.mark.parametrize("how", ["smooth normals on", "a set without base normals"])
def test_null_normals_are_passed_on(prt, mode, how):
    """smooth normals on: regenerated from the morphed vertices; a set without base normals: the uploaded ones kept (refit) or carried (rebuild)"""
    m = morph_case(prt, T_TEAPOT, 3)
    groups, n_groups = prt.weld_corners(m["v0"])
    got = []
    for morphed in (True, False):
        r = _context(prt, m, leaf_root=False)
        if how == "smooth normals on":
            r.set_smooth_normals(groups, n_groups)
        if morphed:
            _set(r, m, normals=(how == "smooth normals on"))
            r.morph(m["weights"], rebuild=(mode == REBUILD), max_leaf=4)
            if how != "smooth normals on":
                assert r.read_morphed()[1] is None
                assert r.lib.prt_read_morphed(r.ctx, m["v"].copy().ctypes.data_as(C.c_void_p), m["n"].copy().ctypes.data_as(C.c_void_p)) == prt.PRT_ERR_INVALID_ARGUMENT
        elif mode == REFIT:
            r.update_vertices(m["v"], None)
        else:
            r.rebuild_bvh(m["v"], None, max_leaf=4)
        got.append(_everything(prt, r))
        r.close()
    if how != "smooth normals on":
        assert np.array_equal(_bytes(got[0]["normals"][:, :3]), _bytes(m["n0"][:, :3]))
    else:
        assert not np.array_equal(got[0]["normals"], m["n"]), "regenerated from the morphed faces, not the morphed base normals"
    _assert_equal(got[0], got[1], "%s, mode %d" % (how, mode))


def _second_morph(prt, m):
    key = ("second morph", m["T"], m["n_targets"])
    if key not in _cache:
        w2 = np.ascontiguousarray(m["weights"][::-1] * f32(0.5))
        _cache[key] = (w2,) + mirror_morph(m["v0"], m["n0"], m["targets"], w2)
    return _cache[key]


@pytest.mark.gpu
def test_motion_snapshot_is_the_paths_and_survives_a_refused_morph(prt):
    m = morph_case(prt, T_TEAPOT, 3)
    w2, v2, n2 = _second_morph(prt, m)
    nan = m["weights"].copy()
    nan[1] = np.nan                                            # (a listed target)
    planes = []
    for morphed in (True, False):
        r = _context(prt, m, leaf_root=False)
        r.set_motion(True)
        if morphed:
            _set(r, m)
            r.morph(m["weights"])
            _refused(prt, lambda: r.morph(nan))
            r.morph(w2)
        else:
            r.update_vertices(m["v"], m["n"])
            r.update_vertices(v2, n2)
        r.render_guides(2)
        planes.append((r.read_motion(), r.read_guides()))
        r.close()
    assert planes[0][0].any(), "the mesh moved in front of the camera"
    assert np.array_equal(_bytes(planes[0][0]), _bytes(planes[1][0])) and np.array_equal(_bytes(planes[0][1]), _bytes(planes[1][1]))


@pytest.mark.gpu
def test_refusals_leave_the_scene_and_the_set_as_they_were(prt):
    import torch
    f = fused_case(prt, T_TEAPOT, False)
    s, m = f["s"], f["m"]
    case = teapot(prt)
    r = prt.Renderer(case.cfg, device=0)
    _refused(prt, lambda: _set(r, m), prt.PRT_ERR_NOT_READY)                            # no scene
    r.close()
    r = _context(prt, m, leaf_root=False)
    r.set_motion(True)
    rest = _scene(r)
    _refused(prt, lambda: r.morph(m["weights"]), prt.PRT_ERR_NOT_READY)                 # no set
    _refused(prt, lambda: r.read_morphed(), prt.PRT_ERR_NOT_READY)
    _skin(r, s)
    _refused(prt, lambda: r.pose_morphed(s["M"], m["weights"]), prt.PRT_ERR_NOT_READY)  # a skin, no set
    r.set_skin(None)
    _assert_equal(_scene(r), rest, "a morph without a set")
    _set(r, m)
    _refused(prt, lambda: r.pose_morphed(s["M"], m["weights"]), prt.PRT_ERR_NOT_READY)  # a set, no skin
    r.morph(m["weights"])                                                              # (a snapshot is pending from here on)
    want = _scene(r)
    assert np.array_equal(_bytes(want["normals"]), _bytes(m["n"]))
    dev = torch.zeros(8, dtype=torch.float32, device="cuda")
    dev[1:4] = torch.from_numpy(m["weights"].copy()).cuda()
    dM = torch.from_numpy(s["M"].copy()).cuda()

    def still(what, morphed_too=True):
        _assert_equal(_scene(r), want, what)
        if morphed_too:
            v, n = r.read_morphed()
            assert np.array_equal(_bytes(v), _bytes(m["v"])) and np.array_equal(_bytes(n), _bytes(m["n"])), what + ": the morphed buffers changed"

    _refused(prt, lambda: r.morph(m["weights"], rebuild=2))
    still("an unknown mode")
    _refused(prt, lambda: r.morph(None))
    still("null weights")
    assert dev.data_ptr() % 16 == 0
    _refused(prt, lambda: r.morph(dev.data_ptr() + 4))
    still("a misaligned device pointer")
    _refused(prt, lambda: r.morph(m["weights"], rebuild=True, max_leaf=65))
    still("max_leaf above 64")
    assert r.lib.prt_read_morphed(r.ctx, None, None) == prt.PRT_ERR_INVALID_ARGUMENT
    # the fused doors
    r.set_skin(s["v0"], None, s["index"], s["weight"], 4)
    _refused(prt, lambda: r.pose_morphed(s["M"], m["weights"]))
    still("exactly one of skin and set has normals")
    _skin(r, s)
    _refused(prt, lambda: r.pose_morphed(s["M"], m["weights"], rebuild=2))
    _refused(prt, lambda: r.pose_morphed(None, m["weights"]))
    _refused(prt, lambda: r.pose_morphed(s["M"], None))
    _refused(prt, lambda: r.pose_morphed(dM.data_ptr(), dev.data_ptr() + 4))
    _refused(prt, lambda: r.pose_morphed(dM.data_ptr() + 4, dev.data_ptr()))
    still("the refusals of prt_pose_morphed")
    _refused(prt, lambda: r.read_posed(), prt.PRT_ERR_NOT_READY)                        # (none of them reached the kernel)
    # the refusals of prt_set_morph_targets: the previous set stays in force
    tg = m["targets"]
    dense = tg[2]
    bad_dp, bad_dn, bad_v, bad_n = dense[1].copy(), dense[2].copy(), m["v0"].copy(), m["n0"].copy()
    bad_dp[17, 2], bad_dn[18959, 0], bad_v[5000, 1], bad_n[18959, 2] = np.nan, np.inf, np.inf, -np.inf
    unsorted = tg[0][0].copy()
    unsorted[[3, 4]] = unsorted[[4, 3]]
    past = tg[0][0].copy()
    past[-1] = 3 * T_TEAPOT
    for what, args in (("no targets", (m["v0"], m["n0"], [])), ("65537 targets", (m["v0"], m["n0"], [tg[1]] * 65537)),
                       ("unsorted corners", (m["v0"], m["n0"], [(unsorted, tg[0][1], tg[0][2])] + tg[1:])),
                       ("a corner >= 3T", (m["v0"], m["n0"], [(past, tg[0][1], tg[0][2])] + tg[1:])),
                       ("null d_position", (m["v0"], m["n0"], [(tg[0][0], None, tg[0][2])] + tg[1:])),
                       ("a NaN position delta", (m["v0"], m["n0"], tg[:2] + [(dense[0], bad_dp, dense[2])])),
                       ("an infinite normal delta", (m["v0"], m["n0"], tg[:2] + [(dense[0], dense[1], bad_dn)])),
                       ("an infinite base coordinate", (bad_v, m["n0"], tg)), ("an infinite base normal", (m["v0"], bad_n, tg))):
        _refused(prt, lambda: r.set_morph_targets(*args))
        still(what)
    null_set = prt._capi.MorphSet(None, None, None, 3, 0)
    assert r.lib.prt_set_morph_targets(r.ctx, C.byref(null_set)) == prt.PRT_ERR_INVALID_ARGUMENT
    null_set = prt._capi.MorphSet(m["v0"].ctypes.data_as(C.c_void_p), None, None, 3, 0)
    assert r.lib.prt_set_morph_targets(r.ctx, C.byref(null_set)) == prt.PRT_ERR_INVALID_ARGUMENT
    still("null base or targets")
    # a NaN and an infinite weight under listed targets: refused by the path's finite-vertex check, the scene untouched (the morphed buffers
    # are the refused morph's); a NaN weight under a target without entries is harmless
    for what, (t, value) in (("a NaN weight", (0, np.nan)), ("an infinite weight", (2, np.inf))):
        w = m["weights"].copy()
        w[t] = value
        for rebuild in (False, True):
            _refused(prt, lambda: r.morph(w, rebuild=rebuild, max_leaf=4))
            still(what, morphed_too=False)
            _refused(prt, lambda: r.pose_morphed(s["M"], w, rebuild=rebuild, max_leaf=4))
            still(what, morphed_too=False)
        v, n = r.read_morphed()
        assert not np.isfinite(v).all(), what + ": prt_read_morphed returns the refused morph"
        assert np.array_equal(_bytes(v), _bytes(mirror_morph(m["v0"], m["n0"], tg, w)[0]))
    # the previous set still morphs to the same bytes, and the pending snapshot is still the base's: the motion plane equals that of a
    # context that morphed twice and was never refused
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
    # a NaN weight under a target without entries
    empty = (np.zeros(0, dtype=np.uint32), np.zeros((0, 4), dtype=f32), None)
    r.set_morph_targets(m["v0"], m["n0"], tg + [empty])
    r.morph(np.concatenate([m["weights"], [np.nan]]).astype(f32))
    v, n = r.read_morphed()
    assert np.array_equal(_bytes(v), _bytes(m["v"])) and np.array_equal(_bytes(n), _bytes(m["n"]))
    r.close()


@pytest.mark.gpu
def test_lifetime(prt):
    """the set survives reset, resize, prt_set_tile, camera changes, an update, a rebuild, poses and morphs, and prt_set_skin in both directions;
    prt_upload_scene turns it off"""
    f = fused_case(prt, T_TEAPOT, False)
    s, m = f["s"], f["m"]
    w2, v2, n2 = _second_morph(prt, m)
    case = teapot(prt)
    r = _context(prt, m, leaf_root=False)
    _set(r, m)
    r.render_frames(prt.seed_pairs(4))
    r.reset()
    r.resize(W + 3, H - 1)
    r.set_camera(case.cam)
    r.set_tile(W, H, 8, 16)
    r.resize(W, H)
    r.update_vertices(v2, n2)
    r.rebuild_bvh(m["v0"], m["n0"], max_leaf=4)
    _skin(r, s)
    r.pose(s["M"])
    r.morph(w2)
    r.pose_morphed(s["M"], m["weights"])
    r.set_skin(None)                                           # (the set stays in force)
    r.morph(m["weights"])
    v, n = r.read_morphed()
    assert np.array_equal(_bytes(v), _bytes(m["v"])) and np.array_equal(_bytes(n), _bytes(m["n"]))
    assert np.array_equal(_bytes(r.read_normals()), _bytes(m["n"])), "a morph after a rebuild refits the new topology"
    _skin(r, s)
    r.set_morph_targets(None)                                  # (... and the skin does when the set goes)
    _refused(prt, lambda: r.morph(m["weights"]), prt.PRT_ERR_NOT_READY)
    _refused(prt, lambda: r.read_morphed(), prt.PRT_ERR_NOT_READY)
    r.pose(s["M"])
    assert np.array_equal(_bytes(r.read_posed()[0]), _bytes(s["v"]))
    _set(r, m)
    r.upload_scene(case.desc)
    assert r.lib.prt_morph(r.ctx, m["weights"].ctypes.data_as(C.c_void_p), REFIT, 0) == prt.PRT_ERR_NOT_READY
    assert r.lib.prt_read_morphed(r.ctx, v.ctypes.data_as(C.c_void_p), None) == prt.PRT_ERR_NOT_READY
    assert np.array_equal(_bytes(r.read_normals()[:, :3]), _bytes(m["n0"][:, :3]))
    r.close()


@pytest.mark.gpu
def test_row_block_contexts_that_each_morph(prt):
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
