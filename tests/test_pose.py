"""prt_set_skin / prt_pose: the mesh posed on the device from per-frame bone matrices (include/prt.h; csrc/hip/pt_pose.h / .hip).

`mirror_pose` (tests/mirrors.py) restates prt.h's formulas in float32 numpy -- every operation rounded to f32, the blend summed left to right from +0 with
np.where(w != 0, w * m, 0) -- and shares no code with the body.  The body (run on the host by tests/emu/pose_emu.cpp) and the device (through
the C ABI) must give its bytes.

CPU tests: the body against the mirror on the teapot and on planted cases, the checks of prt_set_skin.  GPU tests: prt_read_posed against
the mirror at the sizes where a one-lane-per-corner kernel can go wrong (3, 66, 258 and 18 960 corners; 1, 4, 257 and 65 536 bones), and the
scene after a pose against a second context that was given the mirror's arrays through prt_update_vertices / prt_rebuild_bvh -- the path
tests/test_refit.py and tests/test_rebuild.py pin to the CPU oracle."""
import ctypes as C

import numpy as np
import pytest

from cases import (_assert_equal, bones, _everything, identity, pose_cache as _cache, pose_context as _context, POSE_FRAME, pose_scene as _scene,
                   REBUILD, REFIT, _refused, _skin, skin_case, T_TEAPOT, teapot)
from mirrors import mirror_pose
from support import bytes_flat as _bytes

f32 = np.float32
W, H, FRAMES = POSE_FRAME


@pytest.fixture(scope="module")
def emu():
    import pose_api
    pose_api.lib()
    return pose_api


# ---- CPU: the body on the host ---------------------------------------------------------------------------------------------------------------

def _check(emu, rest_v, rest_n, index, weight, M, what):
    got_v, got_n = emu.pose(rest_v, rest_n, index, weight, M)
    want_v, want_n = mirror_pose(rest_v, rest_n, index, weight, M)
    assert np.array_equal(_bytes(got_v), _bytes(want_v)), what + ": vertices differ from the mirror"
    assert (got_n is None) == (want_n is None) and (got_n is None or np.array_equal(_bytes(got_n), _bytes(want_n))), what + ": normals differ from the mirror"
    return got_v, got_n


@pytest.mark.parametrize("rigid", [False, True])
@pytest.mark.parametrize("with_normals", [True, False])
def test_body_equals_the_mirror_on_the_teapot(prt, emu, rigid, with_normals):
    s = skin_case(prt, T_TEAPOT, 3, rigid)
    assert emu.check(s["v0"], s["n0"], s["index"], s["weight"], 3)
    got_v, got_n = _check(emu, s["v0"], s["n0"] if with_normals else None, s["index"], s["weight"], s["M"], "teapot, 3 bones")
    assert not got_v[:, 3].any()
    if with_normals:
        length = np.linalg.norm(got_n[:, :3].astype(np.float64), axis=1)
        assert np.abs(length - 1).max() < 1e-6 and not got_n[:, 3].any()
    if rigid:                                                  # a rigid part costs one matrix: the others may hold anything
        M = s["M"].copy()
        part = (np.arange(3 * T_TEAPOT) // 3) % 3
        one = part == 1
        only = emu.pose(s["v0"][one], None, s["index"][one] * 0 + 1, s["weight"][one], np.where(np.arange(3)[:, None] == 1, M, np.nan))[0]
        assert np.array_equal(_bytes(only), _bytes(got_v[one]))


def test_identity_matrices_give_rest_plus_zero(prt, emu):
    """((1*x + 0*y) + 0*z) + 0: a -0 coordinate becomes +0, everything else keeps its bits; lane 3 is 0 whatever the rest pose holds there"""
    s = skin_case(prt, T_TEAPOT, 3, True)
    v0 = s["v0"].copy()
    v0[7, 0], v0[8, 1], v0[9, 2], v0[:, 3] = -0.0, -0.0, -0.0, 3.0
    got_v, got_n = _check(emu, v0, s["n0"], s["index"], s["weight"], identity(3), "identity")
    assert np.array_equal(_bytes(got_v[:, :3]), _bytes(v0[:, :3] + f32(0.0)))
    assert not np.array_equal(_bytes(got_v[:, :3]), _bytes(v0[:, :3])) and not got_v[:, 3].any()
    s4 = skin_case(prt, T_TEAPOT, 3, False)                    # four influences of the identity: weights that sum to 1 only approximately
    _check(emu, v0, s["n0"], s4["index"], s4["weight"], identity(3), "identity, 4 influences")


def planted():
    """two triangles, four bones; bone 2 is NaN throughout and only ever named under a zero weight, bone 3 is the identity"""
    nan = np.nan
    M = np.array([[1, 0, 0, 0.5, 0, 1, 0, 0, 0, 0, 1, -0.25],
                  [0, -1, 0, 0, 1, 0, 0, 0, 0, 0, 1, 0],
                  [nan] * 12,
                  [1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0]], dtype=f32)
    v = np.zeros((6, 4), dtype=f32)
    n = np.zeros((6, 4), dtype=f32)
    v[:, :3] = [[1, 2, 3], [0.5, -0.25, 4], [1, 1, 1], [1e-42, -2e-44, 1e-45], [3, -2, 1], [0.1, 0.2, 0.3]]
    n[:, :3] = [[0, 1, 0], [0, 0, 1], [0.6, 0.8, 0], [1e-42, 0, 0], [1, 0, 0], [0, 0.6, 0.8]]
    index = np.array([[0, 1, 2, 2], [0, 2, 1, 2], [0, 0, 2, 2], [3, 2, 2, 2], [1, 0, 2, 2], [0, 1, 0, 1]], dtype=np.uint16)
    weight = np.array([[0, -0.0, 0, -0.0],          # all weights zero: to the origin
                       [1, -0.0, 0, 0],             # a -0 weight beside the NaN matrix
                       [0.5, -0.5, 0, 0],           # the same bone with +w and -w: A == 0, the normal has length 0
                       [1, 0, 0, 0],                # denormal coordinates
                       [-0.75, 1.5, 0, -0.0],       # negative weights
                       [0.25, 0.25, 0.25, 0.25]], dtype=f32)
    return v, n, index, weight, M


def test_planted_cases(emu):
    v, n, index, weight, M = planted()
    assert emu.check(v, n, index, weight, 4) and not emu.check(v, n, index, weight, 3)
    got_v, got_n = _check(emu, v, n, index, weight, M, "planted")
    assert np.isfinite(got_v).all() and np.isfinite(got_n).all(), "the NaN matrix was read under a zero weight"
    assert not _bytes(got_v[0]).any() and not _bytes(got_n[0]).any(), "all weights zero: +0 everywhere"
    assert not _bytes(got_n[2]).any() and not _bytes(got_v[2]).any(), "A == 0: L == 0 keeps n' = +0"
    assert np.array_equal(_bytes(got_v[3, :3]), _bytes(v[3, :3] + f32(0))) and got_v[3, 0] != 0, "denormals pass through the identity rotation"
    assert np.array_equal(_bytes(got_n[3, :3]), _bytes(n[3, :3])), "a normal whose square underflows: L == 0 keeps n'"
    # a matrix that overflows is passed on (the refusal is the finite-vertex check's, downstream)
    big = M.copy()
    big[0, 0] = big[0, 1] = 3e38
    got_v, got_n = _check(emu, v, n, index, weight, big, "overflow")
    assert not np.isfinite(got_v[4, 0]) and np.isfinite(got_v[0]).all()
    # ... and a NaN matrix under a non-zero weight
    index2 = index.copy()
    index2[1, 0] = 2
    got_v, _ = _check(emu, v, n, index2, weight, M, "NaN under a weight")
    assert np.isnan(got_v[1, :3]).all() and np.isfinite(got_v[[0, 2, 3, 4, 5]]).all()


def test_skin_checks(prt, emu):
    s = skin_case(prt, 22, 4)
    ok = (s["v0"], s["n0"], s["index"], s["weight"], 4)
    assert emu.check(*ok) and emu.check(s["v0"], None, s["index"], s["weight"], 4) and emu.lib().pose_emu_max_bones() == 65536
    assert not emu.check(*ok[:4], 0) and not emu.check(*ok[:4], 65537) and not emu.check(*ok[:4], 3)
    assert emu.check(s["v0"], s["n0"], s["index"] * 0 + 65535, s["weight"], 65536)
    for which, lanes in ((0, 3), (1, 3), (3, 4)):
        for bad in (np.nan, np.inf, -np.inf):
            for lane in range(lanes):
                a = [x.copy() if x is not None and not isinstance(x, int) else x for x in ok]
                a[which][40, lane] = bad
                assert not emu.check(*a), (which, bad, lane)
    a = [x.copy() if not isinstance(x, int) else x for x in ok]
    a[0][:, 3], a[1][:, 3] = np.nan, np.inf                    # (lane 3 of the rest pose is never looked at)
    assert emu.check(*a)
    a = [x.copy() if not isinstance(x, int) else x for x in ok]
    a[2][65, 3], a[3][65, 3] = 4, 0.0                          # an index >= n_bones is refused even under a zero weight
    assert not emu.check(*a)
    assert emu.check(s["v0"], s["n0"], s["index"], -s["weight"] * 3, 4), "weights may be negative and need not sum to 1"


# ---- GPU -------------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.gpu
@pytest.mark.parametrize("T,n_bones", [(T, nb) for T in (1, 22, 86, T_TEAPOT) for nb in (1, 4, 257)] + [(86, 65536)])
def test_posed_buffers_equal_the_mirror_through_both_doors(prt, T, n_bones):
    """3, 66, 258 and 18 960 corners: less than a wave, across a wave, across a block, many blocks; the table of 1, 4, 257 and 65 536 bones read
    through the vector cache (no LDS staging: no threshold to straddle)"""
    import torch
    s = skin_case(prt, T, n_bones, rigid=(n_bones == 257))
    r = _context(prt, s)
    _skin(r, s)
    assert r.lib.prt_read_posed(r.ctx, np.zeros(12 * T, dtype=f32).ctypes.data_as(C.c_void_p), None) == prt.PRT_ERR_NOT_READY
    for door in ("host", "device"):
        r.pose(s["M"] if door == "host" else torch.from_numpy(s["M"].copy()).cuda(), rebuild=(door == "device"), max_leaf=4)
        v, n = r.read_posed()
        assert np.array_equal(_bytes(v), _bytes(s["v"])), "%s door: posed vertices differ from the mirror" % door
        assert np.array_equal(_bytes(n), _bytes(s["n"])), "%s door: posed normals differ from the mirror" % door
        _skin(r, s)                                            # (set again: the posed buffers are new ones)
    r.close()


@pytest.mark.gpu
@pytest.mark.parametrize("mode", [REFIT, REBUILD])
@pytest.mark.parametrize("mesh", ["86 under a leaf root", "teapot under its tree"])
def test_scene_after_a_pose_equals_an_update_with_the_mirrors_arrays(prt, mode, mesh):
    s = skin_case(prt, 86 if mesh.startswith("86") else T_TEAPOT, 4)
    got = []
    for posed in (True, False):
        r = _context(prt, s, leaf_root=mesh.startswith("86"))
        if posed:
            _skin(r, s)
            before = _scene(r)
            assert np.array_equal(_bytes(before["normals"][:, :3]), _bytes(s["n0"][:, :3])), "setting the skin changes nothing by itself"
            r.pose(s["M"], rebuild=(mode == REBUILD), max_leaf=4)
        elif mode == REFIT:
            r.update_vertices(s["v"], s["n"])
        else:
            r.rebuild_bvh(s["v"], s["n"], max_leaf=4)
        got.append(_everything(prt, r))
        r.close()
    assert np.array_equal(_bytes(got[0]["normals"]), _bytes(s["n"]))
    _assert_equal(got[0], got[1], "%s, mode %d" % (mesh, mode))


@pytest.mark.gpu
@pytest.mark.parametrize("mode", [REFIT, REBUILD])
@pytest.mark.parametrize("how", ["smooth normals on", "a skin without rest normals"])
def test_null_normals_are_passed_on(prt, mode, how):
    """smooth normals on: regenerated from the posed vertices; a skin without rest normals: the rest pose's kept (refit) or carried (rebuild)"""
    s = skin_case(prt, T_TEAPOT, 4)
    groups, n_groups = prt.weld_corners(s["v0"])
    got = []
    for posed in (True, False):
        r = _context(prt, s, leaf_root=False)
        if how == "smooth normals on":
            r.set_smooth_normals(groups, n_groups)
        if posed:
            _skin(r, s, normals=(how == "smooth normals on"))
            r.pose(s["M"], rebuild=(mode == REBUILD), max_leaf=4)
        elif mode == REFIT:
            r.update_vertices(s["v"], None)
        else:
            r.rebuild_bvh(s["v"], None, max_leaf=4)
        got.append(_everything(prt, r))
        r.close()
    if how != "smooth normals on":
        assert np.array_equal(_bytes(got[0]["normals"][:, :3]), _bytes(s["n0"][:, :3]))
    else:
        assert not np.array_equal(got[0]["normals"], s["n"]), "regenerated from the posed faces, not the posed rest normals"
    _assert_equal(got[0], got[1], "%s, mode %d" % (how, mode))


def _second_pose(prt, s):
    M2 = bones(s["n_bones"], 77)
    key = ("second pose", s["T"], s["n_bones"])
    if key not in _cache:
        _cache[key] = mirror_pose(s["v0"], s["n0"], s["index"], s["weight"], M2)
    return (M2,) + _cache[key]


@pytest.mark.gpu
def test_motion_snapshot_is_the_paths_and_survives_a_refused_pose(prt):
    s = skin_case(prt, T_TEAPOT, 4)
    M2, v2, n2 = _second_pose(prt, s)
    nan = s["M"].copy()
    nan[2, 5] = np.nan
    planes = []
    for posed in (True, False):
        r = _context(prt, s, leaf_root=False)
        r.set_motion(True)
        if posed:
            _skin(r, s)
            r.pose(s["M"])
            _refused(prt, lambda: r.pose(nan))
            r.pose(M2)
        else:
            r.update_vertices(s["v"], s["n"])
            r.update_vertices(v2, n2)
        r.render_guides(2)
        planes.append((r.read_motion(), r.read_guides()))
        r.close()
    assert planes[0][0].any(), "the mesh moved in front of the camera"
    assert np.array_equal(_bytes(planes[0][0]), _bytes(planes[1][0])) and np.array_equal(_bytes(planes[0][1]), _bytes(planes[1][1]))


@pytest.mark.gpu
def test_refusals_leave_the_scene_and_the_skin_as_they_were(prt):
    import torch
    s = skin_case(prt, T_TEAPOT, 4)
    case = teapot(prt)
    r = prt.Renderer(case.cfg, device=0)
    skin = prt._capi.Skin(*[a.ctypes.data_as(C.c_void_p) for a in (s["v0"], s["n0"], s["index"], s["weight"])], 4, 0)
    assert r.lib.prt_set_skin(r.ctx, C.byref(skin)) == prt.PRT_ERR_NOT_READY, "no scene"
    r.close()
    r = _context(prt, s, leaf_root=False)
    r.set_motion(True)
    rest = _scene(r)
    _refused(prt, lambda: r.pose(s["M"]), prt.PRT_ERR_NOT_READY)                        # no skin
    _refused(prt, lambda: r.read_posed(), prt.PRT_ERR_NOT_READY)
    _assert_equal(_scene(r), rest, "a pose without a skin")
    _skin(r, s)
    r.pose(s["M"])                                                                     # (a snapshot is pending from here on)
    want = _scene(r)
    assert np.array_equal(_bytes(want["normals"]), _bytes(s["n"]))
    dev = torch.zeros(12 * 4 + 4, dtype=torch.float32, device="cuda")
    dev[1:49] = torch.from_numpy(s["M"].reshape(-1).copy()).cuda()

    def still(what, posed_too=True):
        _assert_equal(_scene(r), want, what)
        if posed_too:
            v, n = r.read_posed()
            assert np.array_equal(_bytes(v), _bytes(s["v"])) and np.array_equal(_bytes(n), _bytes(s["n"])), what + ": the posed buffers changed"

    _refused(prt, lambda: r.pose(s["M"], rebuild=2))
    still("an unknown mode")
    _refused(prt, lambda: r.pose(None))
    still("null matrices")
    assert dev.data_ptr() % 16 == 0
    _refused(prt, lambda: r.pose(dev.data_ptr() + 4))
    still("a misaligned device pointer")
    _refused(prt, lambda: r.pose(s["M"], rebuild=True, max_leaf=65))
    still("max_leaf above 64", posed_too=False)
    assert r.lib.prt_read_posed(r.ctx, None, None) == prt.PRT_ERR_INVALID_ARGUMENT
    # the refusals of prt_set_skin: the previous skin stays in force
    bad_index = s["index"].copy()
    bad_index[1000, 2] = 4
    bad_index_w0 = s["index"].copy()
    bad_index_w0[1000, 0] = 4
    w0 = s["weight"].copy()
    w0[1000, 0] = 0
    bad_w, bad_v, bad_n = s["weight"].copy(), s["v0"].copy(), s["n0"].copy()
    bad_w[17, 3], bad_v[5000, 1], bad_n[18959, 2] = np.nan, np.inf, -np.inf
    for what, args in (("n_bones 0", (s["v0"], s["n0"], s["index"], s["weight"], 0)), ("n_bones 65537", (s["v0"], s["n0"], s["index"], s["weight"], 65537)),
                       ("an index >= n_bones", (s["v0"], s["n0"], bad_index, s["weight"], 4)),
                       ("an index >= n_bones under a zero weight", (s["v0"], s["n0"], bad_index_w0, w0, 4)),
                       ("a NaN weight", (s["v0"], s["n0"], s["index"], bad_w, 4)), ("an infinite rest coordinate", (bad_v, s["n0"], s["index"], s["weight"], 4)),
                       ("an infinite rest normal", (s["v0"], bad_n, s["index"], s["weight"], 4))):
        _refused(prt, lambda: r.set_skin(*args))
        still(what)
    for missing in (0, 2, 3):
        p = [a.ctypes.data_as(C.c_void_p) for a in (s["v0"], s["n0"], s["index"], s["weight"])]
        p[missing] = None
        assert r.lib.prt_set_skin(r.ctx, C.byref(prt._capi.Skin(*p, 4, 0))) == prt.PRT_ERR_INVALID_ARGUMENT
    # a NaN matrix under a non-zero weight and a matrix that overflows: refused by the path's finite-vertex check, the scene untouched (the
    # posed buffers are the refused pose's)
    for what, (row, col, value) in (("a NaN matrix", (1, 3, np.nan)), ("a matrix that overflows", (3, slice(0, 4), 3e38))):
        M = s["M"].copy()
        M[row, col] = value
        for rebuild in (False, True):
            _refused(prt, lambda: r.pose(M, rebuild=rebuild, max_leaf=4))
            still(what, posed_too=False)
        v, n = r.read_posed()
        assert not np.isfinite(v).all(), what + ": prt_read_posed returns the refused pose"
        assert np.array_equal(_bytes(v), _bytes(mirror_pose(s["v0"], s["n0"], s["index"], s["weight"], M)[0]))
    # the previous skin still poses to the same bytes, and the pending snapshot is still the rest pose's: the motion plane equals that of a
    # context that posed twice and was never refused
    r.pose(s["M"])
    still("after the refusals")
    r.render_guides(2)
    motion = r.read_motion()
    r.close()
    r = _context(prt, s, leaf_root=False)
    r.set_motion(True)
    _skin(r, s)
    r.pose(s["M"])
    r.pose(s["M"])
    r.render_guides(2)
    assert motion.any() and np.array_equal(_bytes(motion), _bytes(r.read_motion()))
    r.close()


@pytest.mark.gpu
def test_lifetime(prt):
    """the skin survives reset, resize, prt_set_tile, camera changes, an update, a rebuild and poses; prt_upload_scene turns it off"""
    s = skin_case(prt, T_TEAPOT, 4)
    M2, v2, n2 = _second_pose(prt, s)
    case = teapot(prt)
    r = _context(prt, s, leaf_root=False)
    _skin(r, s)
    r.render_frames(prt.seed_pairs(4))
    r.reset()
    r.resize(W + 3, H - 1)
    r.set_camera(case.cam)
    r.set_tile(W, H, 8, 16)
    r.resize(W, H)
    r.update_vertices(v2, n2)
    r.rebuild_bvh(s["v0"], s["n0"], max_leaf=4)
    r.pose(M2)
    r.pose(s["M"])
    v, n = r.read_posed()
    assert np.array_equal(_bytes(v), _bytes(s["v"])) and np.array_equal(_bytes(n), _bytes(s["n"]))
    assert np.array_equal(_bytes(r.read_normals()), _bytes(s["n"])), "a pose after a rebuild refits the new topology"
    r.set_skin(None)
    _refused(prt, lambda: r.pose(s["M"]), prt.PRT_ERR_NOT_READY)
    _skin(r, s)
    r.upload_scene(case.desc)
    assert r.lib.prt_pose(r.ctx, s["M"].ctypes.data_as(C.c_void_p), REFIT, 0) == prt.PRT_ERR_NOT_READY
    assert r.lib.prt_read_posed(r.ctx, v.ctypes.data_as(C.c_void_p), None) == prt.PRT_ERR_NOT_READY
    assert np.array_equal(_bytes(r.read_normals()[:, :3]), _bytes(s["n0"][:, :3]))
    r.close()


@pytest.mark.gpu
def test_row_block_contexts_that_each_pose(prt):
    s = skin_case(prt, T_TEAPOT, 4)

    def run(part):
        r = _context(prt, s, leaf_root=False)
        if part is not None:
            r.set_row_blocks(W, H, 8, 2, part)
        _skin(r, s)
        r.pose(s["M"], rebuild=True, max_leaf=4)
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
