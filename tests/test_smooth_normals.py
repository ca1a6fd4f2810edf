"""prt_set_smooth_normals: smooth shading normals regenerated on the device from new vertices (include/prt.h; csrc/hip/pt_normals.h / .hip).

`mirror_normals` (tests/mirrors.py) restates prt.h's formulas in float32 numpy (every operation rounded to f32, the sum of a corner taken member by
member in ascending corner order); the kernels' bodies (run on the host by tests/emu/normals_emu.cpp) and the device (through the C ABI)
must give its bytes.  The mirror finds a group's members with a stable argsort of its own, not with the library's table builder.

CPU tests: the weld, the bodies, the loader equivalence, the group table.  GPU tests: the kernels against the mirror, composition with
explicit normals, the render against the CPU oracle, lifetime and refusals."""
import ctypes as C

import numpy as np
import pytest

from cases import Case, _leaf_root_desc, refit_context as _context, refit_render as _render
from mirrors import AREA, LOADER_CREASE_COS, mirror_faces, mirror_normals, mirror_weld, UNIT
from support import assert_same_render as _assert_same, bytes_flat as _bytes

f32 = np.float32
W, H, FRAMES = Case.W, Case.H, Case.FRAMES


@pytest.fixture(scope="module")
def emu():
    import normals_api
    normals_api.lib()
    return normals_api


# ---- meshes ----------------------------------------------------------------------------------------------------------------------------------

_cache = {}


def teapot(prt):
    """cornell_coat through cases.Case: rest pose (v0, n0) and the deformed pose of seed 11 (v), with the weld of the rest pose"""
    if "teapot" not in _cache:
        case = Case(prt, "cornell_coat", seed=11)
        groups, n_groups = mirror_weld(case.v0)
        _cache["teapot"] = (case, groups, n_groups)
    return _cache["teapot"]


def teapot_mirror(prt, weighting, crease):
    """the mirror's normals of the deformed teapot (computed once per setting, shared, never written to)"""
    key = ("teapot mirror", weighting, crease)
    if key not in _cache:
        case, groups, _ = teapot(prt)
        _cache[key] = mirror_normals(case.v, groups, weighting, crease)
        _cache[key].setflags(write=False)
    return _cache[key]


def quads(tris):
    """[T, 3, 3] positions -> float32 [3T, 4]"""
    t = np.asarray(tris, dtype=f32).reshape(-1, 3)
    v = np.zeros((len(t), 4), dtype=f32)
    v[:, :3] = t
    return v


def fan(valence=300, wobble=0.0):
    """a closed fan around one apex: triangle i = (apex, ring[i], ring[i + 1]); the apex's group has `valence` members"""
    ang = (np.arange(valence + 1) % valence).astype(np.float64) * (2 * np.pi / valence)
    ring = np.stack([np.cos(ang), 0.15 * np.sin(3 * ang) + wobble * np.cos(5 * ang), np.sin(ang)], axis=1)
    apex = np.array([0.0, 0.8, 0.0])
    return quads([[apex, ring[i], ring[i + 1]] for i in range(valence)])


def cube():
    """a unit cube, 12 triangles, outward winding"""
    p = np.array([[x, y, z] for x in (0, 1) for y in (0, 1) for z in (0, 1)], dtype=f32)
    faces = [(0, 1, 3, 2), (4, 6, 7, 5), (0, 4, 5, 1), (2, 3, 7, 6), (0, 2, 6, 4), (1, 5, 7, 3)]
    return quads([[p[a], p[b], p[c]] for q in faces for a, b, c in ((q[0], q[1], q[2]), (q[0], q[2], q[3]))])


def random_soup(T, seed):
    rng = np.random.default_rng(seed)
    return quads(rng.uniform(-1, 1, (T, 3, 3)))


def _check(emu, v, groups, n_groups, weighting, crease, what):
    got, face = emu.generate(v, groups, n_groups, weighting, crease)
    want = mirror_normals(v, groups, weighting, crease)
    r, l, f = mirror_faces(v)
    assert np.array_equal(_bytes(face[:, :3]), _bytes(f)) and np.array_equal(_bytes(face[:, 3]), _bytes(l)), what + ": face records differ"
    assert np.array_equal(_bytes(got), _bytes(want)), what + ": normals differ from the mirror"
    return got, f


# ---- CPU: prt_weld_corners -------------------------------------------------------------------------------------------------------------------

def test_weld_equals_a_numpy_weld_on_the_teapot(prt, emu):
    case, groups, n_groups = teapot(prt)
    got, n = prt.weld_corners(case.v0)
    assert n == n_groups == 3201 and case.v0.shape == (3 * 6320, 4)
    assert got.dtype == np.uint32 and np.array_equal(got, groups)
    assert got[0] == 0 and (np.diff(np.maximum.accumulate(got)) <= 1).all(), "ids by first appearance"
    valence = np.bincount(got)
    assert valence.min() == 2 and valence.max() == 40
    assert (mirror_faces(case.v0)[1] > 0).all() and (mirror_faces(case.v)[1] > 0).all(), "no degenerate face"


def test_weld_joins_the_two_zeros(prt):
    v = quads([[[0.0, 1, 2], [1, 0, 0], [0, 0, 1]], [[-0.0, 1, 2], [1, -0.0, 0], [5, 5, 5]]])
    assert np.signbit(v[3, 0]) and np.signbit(v[4, 1])
    got, n = prt.weld_corners(v)
    assert got.tolist() == [0, 1, 2, 0, 1, 3] and n == 4


def test_weld_refusals(prt):
    lib = prt.load_library()
    v = random_soup(2, 1)
    g, n = np.zeros(6, dtype=np.uint32), C.c_uint32(0)
    pv, pg = v.ctypes.data_as(C.c_void_p), g.ctypes.data_as(C.c_void_p)
    assert lib.prt_weld_corners(pv, 2, pg, C.byref(n)) == prt.PRT_OK and n.value == 6
    assert lib.prt_weld_corners(None, 2, pg, C.byref(n)) == prt.PRT_ERR_INVALID_ARGUMENT
    assert lib.prt_weld_corners(pv, 2, None, C.byref(n)) == prt.PRT_ERR_INVALID_ARGUMENT
    assert lib.prt_weld_corners(pv, 2, pg, None) == prt.PRT_ERR_INVALID_ARGUMENT
    assert lib.prt_weld_corners(pv, 0, pg, C.byref(n)) == prt.PRT_ERR_INVALID_ARGUMENT
    for bad in (np.nan, np.inf, -np.inf):
        for lane in range(3):
            w = v.copy()
            w[4, lane] = bad
            with pytest.raises(prt.PrtError) as e:
                prt.weld_corners(w)
            assert e.value.code == prt.PRT_ERR_INVALID_ARGUMENT
    w = v.copy()
    w[:, 3] = np.nan                                           # (lane 3 is never looked at)
    assert prt.weld_corners(w)[1] == 6


# ---- CPU: the kernels' bodies on the host ----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("crease", [-2.0, LOADER_CREASE_COS, 0.5])
@pytest.mark.parametrize("weighting", [UNIT, AREA])
@pytest.mark.parametrize("pose", ["rest", "deformed"])
def test_bodies_equal_the_mirror_on_the_teapot(prt, emu, pose, weighting, crease):
    case, groups, n_groups = teapot(prt)
    v = case.v0 if pose == "rest" else case.v
    got, f = _check(emu, v, groups, n_groups, weighting, crease, "teapot %s %d %g" % (pose, weighting, crease))
    length = np.linalg.norm(got[:, :3].astype(np.float64), axis=1)
    assert np.abs(length - 1).max() < 1e-6 and (got[:, 3] == 0).all()
    if crease == 0.5:
        assert not np.array_equal(got, mirror_normals(v, groups, weighting, -2.0)), "the crease test changes nothing on the teapot?"


@pytest.mark.parametrize("weighting", [UNIT, AREA])
def test_bodies_on_a_closed_fan_of_valence_300(prt, emu, weighting):
    v = fan(300)
    groups, n_groups = prt.weld_corners(v)
    assert n_groups == 301 and np.bincount(groups).max() == 300
    got, f = _check(emu, v, groups, n_groups, weighting, LOADER_CREASE_COS, "fan")
    apex = got[0::3]
    assert np.array_equal(_bytes(apex), _bytes(np.tile(apex[:1], (300, 1)))), "every apex corner sums the same members in the same order"


def test_bodies_on_a_soup_of_single_corner_groups(emu):
    """Every corner in a group of its own: the sum is the corner's own face alone.  AREA: s = r_i and L = l_i by the same expression, so the
    normal is r_i / l_i = f_i, bit for bit, on every face.  UNIT: s = f_i and the normal is f_i / L with L = sqrtf(f_i . f_i), which rounds to
    exactly 1 on every axis-aligned face and on most others -- there the normal is f_i's own bits -- and is one or two ulps from 1 on the rest,
    where the normal is f_i divided by that L (what the mirror says, byte for byte).  The first 12 triangles are a cube's, the rest random."""
    v = np.concatenate([cube(), random_soup(117, 3)])
    T = len(v) // 3
    groups = np.arange(3 * T, dtype=np.uint32)
    got, f = _check(emu, v, groups, 3 * T, AREA, LOADER_CREASE_COS, "soup, area")
    fi = f[np.arange(3 * T) // 3]
    assert np.array_equal(_bytes(got[:, :3]), _bytes(fi)), "area weighting: every normal equals f_i"
    got, f = _check(emu, v, groups, 3 * T, UNIT, LOADER_CREASE_COS, "soup, unit")
    L = np.sqrt((fi[:, 0] * fi[:, 0] + fi[:, 1] * fi[:, 1]) + fi[:, 2] * fi[:, 2])
    exact = L == 1
    assert exact[:36].all() and exact.mean() > 0.5
    assert np.array_equal(_bytes(got[exact, :3]), _bytes(fi[exact])), "L == 1: every normal equals f_i"
    assert np.abs(got[:, :3] - fi).max() <= 2 * np.finfo(f32).eps, "elsewhere: f_i divided by an L next to 1"


def test_bodies_on_a_welded_cube_with_a_crease(prt, emu):
    v = cube()
    groups, n_groups = prt.weld_corners(v)
    assert n_groups == 8
    for weighting in (UNIT, AREA):
        got, f = _check(emu, v, groups, n_groups, weighting, 0.5, "cube")
        assert np.array_equal(_bytes(got[:, :3]), _bytes(f[np.arange(36) // 3])), "every corner keeps its face's normal exactly"
    smooth, _ = _check(emu, v, groups, n_groups, UNIT, -2.0, "cube without a crease")
    assert not np.array_equal(smooth[:, :3], f[np.arange(36) // 3])


def test_bodies_on_a_zero_area_face(prt, emu):
    a, b, c, d = [0, 0, 0], [1, 0, 0], [0, 1, 0], [0.5, 0.5, 0.25]
    v = quads([[a, b, c], [b, b, c], [b, d, c], [a, a, a]])          # face 1: two corners coincide; face 3: a point
    groups, n_groups = prt.weld_corners(v)
    r, l, f = mirror_faces(v)
    assert l[1] == 0 and l[3] == 0 and not f[1].any()
    for weighting in (UNIT, AREA):
        for crease in (-2.0, LOADER_CREASE_COS, 0.5):
            got, _ = _check(emu, v, groups, n_groups, weighting, crease, "zero-area face")
            assert np.isfinite(got).all()
    alone = np.arange(12, dtype=np.uint32)
    got, _ = _check(emu, v, alone, 12, UNIT, LOADER_CREASE_COS, "zero-area face alone")
    assert not got[3:6].any() and not got[9:12].any(), "L == 0: the normal is f_i, here zero"


def test_bodies_on_two_coincident_faces_of_opposite_winding(prt, emu):
    a, b, c = [0.25, 0, 0], [1, 0.5, 0], [0, 1, 0.75]
    v = quads([[a, b, c], [a, c, b]])
    groups, n_groups = prt.weld_corners(v)
    assert n_groups == 3
    got, f = _check(emu, v, groups, n_groups, UNIT, -2.0, "coincident faces")
    assert np.array_equal(_bytes(f[0]), _bytes(-f[1]))
    assert np.array_equal(_bytes(got[:, :3]), _bytes(f[np.arange(6) // 3])), "the sum is zero: each corner keeps its own f_i"
    _check(emu, v, groups, n_groups, AREA, -2.0, "coincident faces, area")


def test_bodies_on_one_triangle(prt, emu):
    v = quads([[[0.1, 0.2, 0.3], [1.5, 0.25, -0.5], [0.4, 1.75, 0.6]]])
    groups, n_groups = prt.weld_corners(v)
    assert n_groups == 3
    for weighting in (UNIT, AREA):
        _check(emu, v, groups, n_groups, weighting, LOADER_CREASE_COS, "T = 1")


def test_nan_and_overflow_go_through_the_formulas(emu):
    v = quads([[[0, 0, 0], [3e38, 0, 0], [0, 3e38, 0]], [[0, 0, 0], [0, 3e38, 0], [0, 0, 1]], [[0, 0, 0], [1, 0, 0], [0, 1, 0]]])
    groups = mirror_weld(v)[0]
    for weighting in (UNIT, AREA):
        _check(emu, v, groups, int(groups.max()) + 1, weighting, LOADER_CREASE_COS, "overflow")


# ---- CPU: the loader's rule ------------------------------------------------------------------------------------------------------------------

def test_bodies_reproduce_the_loaders_smooth_normals(prt, emu, tmp_path):
    """an OBJ without vn (a 12 x 12 grid bent over a cylinder, closed by a pole vertex above it) through HostScene, whose loader applies
    smooth_missing_normals; the bodies on the loaded vertices with prt_weld_corners' groups, UNIT and the loader's crease give desc.normals"""
    N = 12
    pts = []
    for i in range(N + 1):
        for j in range(N + 1):
            a = 0.9 * np.pi * j / N
            pts.append((0.7 * np.cos(a), 0.7 * np.sin(a) + 0.01 * i * j, 1.5 * i / N - 0.75))
    pole = len(pts)
    pts.append((0.0, 1.9, 0.0))
    idx = lambda i, j: i * (N + 1) + j
    faces = []
    for i in range(N):
        for j in range(N):
            faces += [(idx(i, j), idx(i, j + 1), idx(i + 1, j + 1)), (idx(i, j), idx(i + 1, j + 1), idx(i + 1, j))]
    faces += [(pole, idx(0, j + 1), idx(0, j)) for j in range(N)] + [(pole, idx(N, j), idx(N, j + 1)) for j in range(N)]
    (tmp_path / "bent.obj").write_text("o bent\n" + "".join("v %r %r %r\n" % tuple(float(x) for x in p) for p in pts) + "".join("f %d %d %d\n" % (a + 1, b + 1, c + 1) for a, b, c in faces))
    text = '{"scene":{"obj":{"path":"bent.obj","material":{"type":1}},"spheres":[{"pos":[0,3,0],"radius":0.5,"material":{"color":[5,5,5],"type":0}}]}}'
    scene = prt.HostScene(text, models_dir=str(tmp_path) + "/", text=True)
    a = prt.scene_arrays(scene.desc)
    v, n = a["vertices"].copy(), a["normals"].copy()
    assert len(v) == 3 * len(faces) == 3 * (2 * N * N + 2 * N)
    groups, n_groups = prt.weld_corners(v)
    assert n_groups == len(pts) and np.bincount(groups).max() == 2 * N
    got, f = _check(emu, v, groups, n_groups, UNIT, LOADER_CREASE_COS, "bent grid")
    assert np.array_equal(_bytes(got[:, :3]), _bytes(n[:, :3])), "the bodies differ from the loader's smooth_missing_normals"
    assert not np.array_equal(got[:, :3], f[np.arange(len(v)) // 3]), "the mesh is smooth somewhere"


# ---- CPU: the group table --------------------------------------------------------------------------------------------------------------------

def test_group_table(prt, emu):
    case, groups, n_groups = teapot(prt)
    spread = (groups.astype(np.uint64) * 3 + 2).astype(np.uint32)              # ids with gaps: 3g + 2 of 3 n_groups + 5
    for g, n in ((groups, n_groups), (spread, 3 * n_groups + 5), (np.zeros(9, dtype=np.uint32), 1), (np.arange(9, dtype=np.uint32)[::-1].copy(), 9)):
        first, member = emu.table(g, n)
        T = len(g) // 3
        assert first[0] == 0 and first[-1] == 3 * T and len(first) == n + 1 and (np.diff(first.astype(np.int64)) >= 0).all()
        count = np.bincount(g, minlength=n)
        assert np.array_equal(np.diff(first.astype(np.int64)), count), "a group's span is its corner count; an unused id's is empty"
        corners = np.argsort(g, kind="stable")                                 # ascending corner order within a group
        assert np.array_equal(member, (corners // 3).astype(np.uint32)), "members: the faces of the group's corners, ascending"
        seen = np.zeros(3 * T, dtype=np.int64)
        for grp in np.unique(g)[:50]:
            mine = np.nonzero(g == grp)[0]
            assert np.array_equal(member[first[grp]:first[grp + 1]], mine // 3)
            seen[mine] += 1
        assert seen.max() == 1, "every corner appears exactly once"
    assert emu.table(np.array([0, 1, 2], dtype=np.uint32), 2) is None, "an id >= n_groups is refused"
    assert emu.generate(quads([[[0, 0, 0], [1, 0, 0], [0, 1, 0]]]), np.array([0, 1, 2], dtype=np.uint32), 2, UNIT, 0.0) is None


# ---- GPU --------------------------------------------------------------------------------------------------------------------------------------

def _soup_case(prt, v_rest):
    """cornell_coat's configuration around a soup uploaded under a leaf root that names every triangle"""
    case, _, _ = teapot(prt)
    n = np.zeros_like(v_rest)
    n[:, 1] = 1
    return case, _leaf_root_desc(prt, case.desc, v_rest, n)


@pytest.mark.gpu
@pytest.mark.parametrize("mesh,weighting,crease", [("teapot", "unit", LOADER_CREASE_COS), ("teapot", "area", -2.0), ("fan", "unit", LOADER_CREASE_COS),
                                                   ("fan", "area", LOADER_CREASE_COS), ("one", "unit", LOADER_CREASE_COS), ("one", "area", 0.5)])
def test_kernels_equal_the_mirror(prt, mesh, weighting, crease):
    """T = 1, 300 and 6 320: one partial block, a block edge inside the apex group's span, many blocks"""
    w = {"unit": UNIT, "area": AREA}[weighting]
    if mesh == "teapot":
        case, groups, n_groups = teapot(prt)
        desc, v, want = case.desc, case.v, teapot_mirror(prt, w, crease)
    else:
        rest = fan(300) if mesh == "fan" else quads([[[0.1, 0.2, 0.3], [1.5, 0.25, -0.5], [0.4, 1.75, 0.6]]])
        v = fan(300, wobble=0.07) if mesh == "fan" else quads([[[0.1, 0.3, 0.3], [1.25, 0.25, -0.5], [0.4, 1.5, 0.7]]])
        case, desc = _soup_case(prt, rest)
        groups, n_groups = prt.weld_corners(rest)
        want = mirror_normals(v, groups, w, crease)
    r = _context(case, desc)
    r.set_smooth_normals(groups, n_groups, weighting, crease)
    r.update_vertices(v, None)
    got = r.read_normals()
    r.close()
    assert got.shape == want.shape and np.array_equal(_bytes(got), _bytes(want)), "%s: the device's normals differ from the mirror" % mesh


@pytest.mark.gpu
def test_host_and_device_variants_agree(prt, oracle):
    import torch
    case, groups, n_groups = teapot(prt)
    out = []
    for device in (False, True):
        r = _context(case)
        r.set_smooth_normals(groups, n_groups)
        r.update_vertices(torch.from_numpy(case.v).cuda() if device else case.v, None)
        out.append((r.read_normals(),) + _render(case, r))
        r.close()
    assert np.array_equal(_bytes(out[0][0]), _bytes(out[1][0]))
    assert np.array_equal(_bytes(out[0][0]), _bytes(teapot_mirror(prt, UNIT, LOADER_CREASE_COS)))
    _assert_same(oracle, out[0][1].view(oracle.PATH_STATE_DTYPE), out[0][2], out[1][1], out[1][2], "numpy against torch")


def _everything(case, r):
    state, img = _render(case, r)
    r.render_guides(2)
    return {"state": state, "framebuffer": img, "guides": r.read_guides(), "bounds": r.read_bvh_bounds(), "normals": r.read_normals()}


def _assert_everything_equal(got, want, what):
    for k in want:
        assert got[k].shape == want[k].shape and np.array_equal(_bytes(got[k]), _bytes(want[k])), "%s: %s differs" % (what, k)


@pytest.mark.gpu
@pytest.mark.parametrize("how", ["update", "rebuild", "rebuild from a leaf root"])
def test_generated_normals_compose_as_explicit_ones(prt, how):
    case, groups, n_groups = teapot(prt)
    generated = teapot_mirror(prt, UNIT, LOADER_CREASE_COS)
    desc = _leaf_root_desc(prt, case.desc, case.v0, case.n0) if how == "rebuild from a leaf root" else case.desc
    got = []
    for smooth in (True, False):
        r = _context(case, desc)
        if smooth:
            r.set_smooth_normals(groups, n_groups)
        n = None if smooth else generated
        if how == "update":
            r.update_vertices(case.v, n)
        else:
            r.rebuild_bvh(case.v, n, max_leaf=4)
        got.append(_everything(case, r))
        r.close()
    assert np.array_equal(_bytes(got[0]["normals"]), _bytes(generated))
    _assert_everything_equal(got[0], got[1], how)


@pytest.mark.gpu
def test_rebuild_with_null_normals_under_a_partial_tree(prt):
    """a tree that references only some triangles: a rebuild with NULL normals is refused without the topology (there is no record to carry
    for the rest) and accepted with it (there is a normal for every corner)"""
    case, groups, n_groups = teapot(prt)
    T = len(case.v0) // 3
    desc = _leaf_root_desc(prt, case.desc, case.v0, case.n0)
    keep = desc._keep[2].copy()
    keep[0]["count"] = 100                                     # (the leaf root names 100 of the T triangles)
    desc._keep.append(keep)
    desc.bvh_nodes = keep.ctypes.data_as(C.c_void_p)
    r = _context(case, desc)
    rest = r.read_normals()
    assert rest[:300].any() and not rest[300:].any(), "a triangle no slot holds reads as zeros"
    with pytest.raises(prt.PrtError) as e:
        r.rebuild_bvh(case.v, None, max_leaf=4)
    assert e.value.code == prt.PRT_ERR_INVALID_ARGUMENT
    r.set_smooth_normals(groups, n_groups)
    r.rebuild_bvh(case.v, None, max_leaf=4)
    got = r.read_normals()
    r.close()
    assert len(got) == 3 * T and np.array_equal(_bytes(got), _bytes(teapot_mirror(prt, UNIT, LOADER_CREASE_COS)))


_oracle_cache = {}


@pytest.mark.gpu
def test_render_after_an_update_with_generated_normals_matches_the_oracle(prt, oracle):
    """the generated normals reach the render kernels: the oracle on a desc holding (v, mirror normals, mirror_refit nodes)"""
    case, groups, n_groups = teapot(prt)
    want = Case(prt, "cornell_coat", seed=11)
    want.set(case.v, teapot_mirror(prt, UNIT, LOADER_CREASE_COS))
    r = _context(case)
    r.set_smooth_normals(groups, n_groups)
    r.update_vertices(case.v, None)
    state, img = _render(case, r)
    bounds = r.read_bvh_bounds()
    r.close()
    ostate, oimg = oracle.Restatement().render(want.cfg, want.new_desc, want.cam, W, H, prt.seed_pairs(FRAMES), env=want.env, threads=8)
    _assert_same(oracle, ostate, oimg, state, img, "update with generated normals")
    assert np.array_equal(_bytes(bounds), _bytes(want.nodes["bounds"]))


@pytest.mark.gpu
def test_it_matters(prt):
    """on the deformed teapot the guides' normal plane differs between smooth on and off; on, it is a fresh upload's of (v, mirror normals)"""
    case, groups, n_groups = teapot(prt)
    fresh = Case(prt, "cornell_coat", seed=11)
    fresh.set(case.v, teapot_mirror(prt, UNIT, LOADER_CREASE_COS))
    planes = {}
    for which in ("on", "off", "fresh"):
        r = _context(case, fresh.new_desc if which == "fresh" else None)
        if which == "on":
            r.set_smooth_normals(groups, n_groups)
        if which != "fresh":
            r.update_vertices(case.v, None)
        r.render_guides(2)
        planes[which] = r.read_guides()
        r.close()
    assert np.array_equal(_bytes(planes["on"]), _bytes(planes["fresh"]))
    differ = (planes["on"][..., 4:7] != planes["off"][..., 4:7]).any(axis=-1)
    assert differ.mean() > 0.02, "the rest pose's normals are as good as the regenerated ones?"
    assert np.array_equal(_bytes(planes["on"][..., 7]), _bytes(planes["off"][..., 7])), "depth is geometry: the same either way"


@pytest.mark.gpu
@pytest.mark.parametrize("how", ["never set", "set, then turned off"])
def test_off_is_off(prt, how):
    """today's bytes: an update keeps the uploaded normals, a rebuild carries them, whatever was set and unset before"""
    case, groups, n_groups = teapot(prt)
    key = "off reference"
    if key not in _cache:
        r = _context(case)
        r.update_vertices(case.v, case.n0)                     # (explicitly the uploaded normals: what NULL keeps)
        a = _everything(case, r)
        r.rebuild_bvh(case.v0, case.n0, max_leaf=4)
        _cache[key] = (a, _everything(case, r))
        r.close()
    r = _context(case)
    if how != "never set":
        r.set_smooth_normals(groups, n_groups, "area", 0.5)
        r.set_smooth_normals(None)
    assert np.array_equal(_bytes(r.read_normals()[:, :3]), _bytes(case.n0[:, :3])), "before any update: the uploaded normals"
    r.update_vertices(case.v, None)
    a = _everything(case, r)
    assert np.array_equal(_bytes(a["normals"][:, :3]), _bytes(case.n0[:, :3])) and not a["normals"][:, 3].any()
    r.rebuild_bvh(case.v0, None, max_leaf=4)
    b = _everything(case, r)
    r.close()
    _assert_everything_equal(a, _cache[key][0], how + ", update")
    _assert_everything_equal(b, _cache[key][1], how + ", rebuild")


@pytest.mark.gpu
def test_refusals_leave_the_topology_in_force(prt):
    case, groups, n_groups = teapot(prt)
    want = teapot_mirror(prt, UNIT, LOADER_CREASE_COS)
    r = prt.Renderer(case.cfg, device=0)
    out = np.zeros(4, dtype=f32)
    assert r.lib.prt_set_smooth_normals(r.ctx, groups.ctypes.data_as(C.c_void_p), n_groups, 0, C.c_float(0.0)) == prt.PRT_ERR_NOT_READY
    assert r.lib.prt_read_normals(r.ctx, out.ctypes.data_as(C.c_void_p)) == prt.PRT_ERR_NOT_READY
    r.close()
    r = _context(case)
    assert r.lib.prt_read_normals(r.ctx, None) == prt.PRT_ERR_INVALID_ARGUMENT
    r.set_smooth_normals(groups, n_groups)
    bad_id = groups.copy()
    bad_id[len(bad_id) // 2] = n_groups
    for args in ((bad_id, n_groups, "unit", LOADER_CREASE_COS), (groups, 0, "unit", LOADER_CREASE_COS), (groups, n_groups, 2, LOADER_CREASE_COS),
                 (groups, n_groups, "area", np.nan), (groups, n_groups, "area", np.inf)):
        with pytest.raises(prt.PrtError) as e:
            r.set_smooth_normals(*args)
        assert e.value.code == prt.PRT_ERR_INVALID_ARGUMENT
    r.update_vertices(case.v, None)
    assert np.array_equal(_bytes(r.read_normals()), _bytes(want)), "the previous topology is still the one in force"
    # a non-finite vertex: records and normals unchanged
    bounds = r.read_bvh_bounds()
    bad = case.v0.copy()
    bad[1234, 2] = np.inf
    for call in (lambda: r.update_vertices(bad, None), lambda: r.rebuild_bvh(bad, None, 4)):
        with pytest.raises(prt.PrtError) as e:
            call()
        assert e.value.code == prt.PRT_ERR_INVALID_ARGUMENT
        assert np.array_equal(_bytes(r.read_normals()), _bytes(want)) and np.array_equal(_bytes(r.read_bvh_bounds()), _bytes(bounds))
    # prt_upload_scene turns it off
    r.upload_scene(case.desc)
    r.update_vertices(case.v, None)
    assert np.array_equal(_bytes(r.read_normals()[:, :3]), _bytes(case.n0[:, :3]))
    r.close()


@pytest.mark.gpu
def test_lifetime(prt, oracle):
    """the topology survives reset, resize, camera changes, updates and rebuilds; histories, path state and framebuffer survive an update
    with generated normals as any update"""
    case, groups, n_groups = teapot(prt)
    want = teapot_mirror(prt, UNIT, LOADER_CREASE_COS)
    r = _context(case)
    r.set_smooth_normals(groups, n_groups)
    assert np.array_equal(_bytes(r.read_normals()[:, :3]), _bytes(case.n0[:, :3])), "setting it changes nothing by itself"
    r.render_frames(prt.seed_pairs(FRAMES))
    r.render_guides(2)
    r.denoise_temporal(passes=1)
    hist, fb, state, guides = r.read_history(), r.read_framebuffer(), r.read_state(), r.read_guides()
    r.set_smooth_normals(groups, n_groups)                     # (again: the records, guides and histories keep their bits)
    assert np.array_equal(_bytes(r.read_guides()), _bytes(guides))
    r.update_vertices(case.v, None)
    with pytest.raises(prt.PrtError) as e:
        r.read_guides()
    assert e.value.code == prt.PRT_ERR_NOT_READY
    assert np.array_equal(_bytes(r.read_history()), _bytes(hist)), "the history is kept"
    assert np.array_equal(_bytes(r.read_framebuffer()), _bytes(fb)) and np.array_equal(_bytes(r.read_state()), _bytes(state))
    r.reset()
    r.resize(W + 3, H - 1)
    r.set_camera(case.cam)
    r.set_tile(W, H, 8, 16)
    r.resize(W, H)
    r.update_vertices(case.v0, None)
    r.rebuild_bvh(case.v, None, max_leaf=4)
    assert np.array_equal(_bytes(r.read_normals()), _bytes(want))
    r.update_vertices(case.v, None)
    assert np.array_equal(_bytes(r.read_normals()), _bytes(want)), "an update after a rebuild refits the new topology with generated normals"
    r.close()


@pytest.mark.gpu
def test_row_block_contexts_that_each_update(prt, oracle):
    case, groups, n_groups = teapot(prt)

    def run(part):
        r = _context(case)
        if part is not None:
            r.set_row_blocks(W, H, 16, 2, part)
        r.set_smooth_normals(groups, n_groups)
        r.update_vertices(case.v, None)
        out = _render(case, r)
        r.close()
        return out
    state, img = run(None)
    got_state, got_img = np.zeros_like(state).reshape(H, W), np.zeros_like(img)
    for part in range(2):
        rows = [y for y in range(H) if (y // 16) % 2 == part]
        s, i = run(part)
        got_state[rows], got_img[rows] = s.reshape(len(rows), W), i
    _assert_same(oracle, state.view(oracle.PATH_STATE_DTYPE), img, got_state.reshape(-1), got_img, "two row-block contexts")
