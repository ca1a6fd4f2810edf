"""Environment-map importance sampling (prt_config::env_importance_sampling), function by function and per pixel block.

The reference does not have the mode, so nothing here is pinned to it: the tables (prt_env_cdf = build_env_cdf), the search, env_sample, env_pdf and
env_lookup (prt_selftest_fn fn 13 / 14) are compared with float64 numpy statements of the same formulas; the estimator is compared with the
default mode -- which IS pinned to the reference bit for bit -- on 8 x 8 block means of small frames ("Environment importance sampling,
function by function").  Every function-level test runs on the host compilation of the device code (tests/emu) without a GPU and has a `gpu` twin
that asserts device output == host output bit for bit and then runs the same checks on the device output."""
import functools
import json
import time

import numpy as np
import pytest

import support                          # (its import puts tests/emu, where emu_api lives, on the path)
import emu_api

F32 = np.float32
PI = np.pi


# ---- the maps ---------------------------------------------------------------------------------------------------------------------------
def _block_map(ci, cj, w=64, h=32):
    """constant 1 with a 3 x 3 block of 200 centred on column ci, row cj (columns wrap; rows outside the map are dropped)"""
    m = np.ones((h, w, 3), dtype=F32)
    for dj in (-1, 0, 1):
        for di in (-1, 0, 1):
            if 0 <= cj + dj < h:
                m[cj + dj, (ci + di) % w] = 200.0
    return m


@functools.lru_cache(maxsize=None)
def _maps():
    rng = np.random.RandomState(20261019)
    maps = {}
    for w, h in ((1, 1), (2, 1), (4, 2), (5, 3)):                     # the sizes fn 11 is tested at
        maps["rand%dx%d" % (w, h)] = rng.uniform(0.1, 4.0, (h, w, 3)).astype(F32)
    m = rng.uniform(0.1, 4.0, (5, 7, 3)).astype(F32)
    m[:, :3] = 0.0
    maps["black7x5"] = m
    maps["const"] = np.ones((32, 64, 3), dtype=F32)
    maps["seam0"] = _block_map(0, 8)                                   # the block straddles the seam
    maps["seam63"] = _block_map(63, 8)
    maps["pole"] = _block_map(20, 0)
    return maps


MAPS = ("rand1x1", "rand2x1", "rand4x2", "rand5x3", "black7x5", "const", "seam0", "seam63", "pole")
BIG = ("const", "seam0", "seam63", "pole")                             # the 64 x 32 maps


def cdf_mirror(rgb):
    """prt.h's statement of prt_env_cdf in float64 numpy, rounded to float32 at the end"""
    a = rgb.astype(np.float64)
    h, w = a.shape[:2]
    lum = (0.2126 * a[..., 0] + 0.7152 * a[..., 1]) + 0.0722 * a[..., 2]
    lum = np.where((lum > 0.0) & (lum < 1e30), lum, 0.0)
    m = np.zeros_like(lum)
    jj, ii = np.arange(h), np.arange(w)
    for dj in (-1, 0, 1):
        for di in (-1, 0, 1):
            m = np.maximum(m, lum[np.clip(jj + dj, 0, h - 1)][:, (ii + di) % w])       # rows clamp, columns wrap
    st = np.sin(PI * (jj + 0.5) / h)
    f = m * st[:, None]
    total = f.sum()
    floor = 0.05 * total / (w * h) if total > 0.0 else 1.0
    f = f + (floor * st * (PI / 2.0))[:, None]
    row_sum = f.sum(axis=1)
    rows = np.concatenate([[0.0], np.cumsum(row_sum)]) / row_sum.sum()
    cols = np.concatenate([np.zeros((h, 1)), np.cumsum(f, axis=1)], axis=1) / row_sum[:, None]
    rows[h] = 1.0
    cols[:, w] = 1.0
    return rows.astype(F32), cols.astype(F32)


def _ulps(a, b):
    """distance in float32 ulps of non-negative float32 arrays"""
    return np.abs(a.view(np.int32).astype(np.int64) - b.view(np.int32).astype(np.int64))


@functools.lru_cache(maxsize=None)
def _tables(name):
    return support.pkg().env_cdf(_maps()[name])


# ---- tables -----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", MAPS)
def test_tables_match_the_stated_density(prt, name):
    """prt_env_cdf == the float64 mirror of prt.h's formula within 1 float32 ulp (the summation order); 0 .. 1, strictly increasing: no bin of
    these maps is empty, the black columns of the 7 x 5 map included (the floor)"""
    env = _maps()[name]
    h, w = env.shape[:2]
    rows, cols = prt.env_cdf(env)
    mrows, mcols = cdf_mirror(env)
    assert rows.shape == (h + 1,) and cols.shape == (h, w + 1)
    assert _ulps(rows, mrows).max() <= 1 and _ulps(cols, mcols).max() <= 1, (name, int(_ulps(rows, mrows).max()), int(_ulps(cols, mcols).max()))
    assert rows[0] == 0.0 and rows[h] == 1.0 and (cols[:, 0] == 0.0).all() and (cols[:, w] == 1.0).all()
    assert (np.diff(rows) > 0).all() and (np.diff(cols, axis=1) > 0).all(), name
    if name == "black7x5":                                            # columns 0 and 2 have a lit neighbour, column 1 has the floor alone
        width = np.diff(cols, axis=1)
        assert (width[:, :3] > 0).all() and (width[:, 1] < 0.2 * width[:, 4]).all()
    if name in ("seam0", "seam63"):                                   # the block's neighbourhood maximum reaches across the seam
        c = 0 if name == "seam0" else 63
        width = np.diff(cols[8].astype(np.float64))
        heavy = sorted(int(i) for i in np.argsort(width)[-5:])
        assert heavy == sorted((c + d) % 64 for d in (-2, -1, 0, 1, 2)), (name, heavy)


def test_tables_of_a_large_map_with_one_hot_texel_have_no_empty_bin(prt):
    """2048 x 1024 constant 1 with one texel at 1e5: every bin of both tables keeps a positive float32 width"""
    env = np.ones((1024, 2048, 3), dtype=F32)
    env[300, 1000] = 1e5
    rows, cols = prt.env_cdf(env)
    assert rows[0] == 0.0 and rows[-1] == 1.0 and (np.diff(rows) > 0).all()
    assert (cols[:, 0] == 0.0).all() and (cols[:, -1] == 1.0).all() and (np.diff(cols, axis=1) > 0).all()


def test_env_cdf_refuses_bad_arguments(prt):
    import ctypes as C
    lib = prt.load_library()
    buf = np.zeros(16, dtype=F32)
    p = buf.ctypes.data_as(C.c_void_p)
    assert lib.prt_env_cdf(None, 1, 1, p, p) != 0 and lib.prt_env_cdf(p, 0, 1, p, p) != 0 and lib.prt_env_cdf(p, 1, 1, None, p) != 0


# ---- the cases of fn 13 / fn 14 -----------------------------------------------------------------------------------------------------------
def _below(x):
    return np.nextafter(x.astype(F32), F32(-1.0))


def _cases(cols):
    c = np.zeros((len(cols[0]), 32), dtype=F32)
    for k, col in enumerate(cols):
        c[:, k] = col
    return c


@functools.lru_cache(maxsize=None)
def _search_cases(name):
    """xi on a 257 x 257 grid; 0, 1 - 2^-24, every table entry and its float32 neighbour below"""
    rows, cols = _tables(name)
    h, w = cols.shape[0], cols.shape[1] - 1
    g = (np.arange(257) / 257.0).astype(F32)
    top = F32(1.0 - 2.0 ** -24)
    edge0 = np.concatenate([[F32(0.0), top], rows, _below(rows)]).astype(F32)
    edge0 = edge0[(edge0 >= 0.0) & (edge0 < 1.0)]
    x0 = [np.repeat(g, 257), np.repeat(edge0, 17)]
    x1 = [np.tile(g, 257), np.tile(g[::16][:17], len(edge0))]
    for j in range(h):                                                 # the column table of row j: xi0 in the middle of the row's bin
        e = np.concatenate([[F32(0.0), top], cols[j], _below(cols[j])]).astype(F32)
        e = e[(e >= 0.0) & (e < 1.0)]
        mid = F32(0.5 * (float(rows[j]) + float(rows[j + 1])))
        x0.append(np.full(len(e), mid, dtype=F32))
        x1.append(e)
    return _cases([np.concatenate(x0), np.concatenate(x1)])


@functools.lru_cache(maxsize=None)
def _trip_cases(name):
    """per texel a grid of interior points (fractions 0.02 .. 0.98, the bin midpoint among them): xi = c0 + f (c1 - c0).  Returns (cases,
    midpoint mask)"""
    rows, cols = _tables(name)
    h, w = cols.shape[0], cols.shape[1] - 1
    fr = np.array([0.02, 0.25, 0.5, 0.75, 0.98]) if w * h > 64 else np.concatenate([np.linspace(0.02, 0.98, 32), [0.5]])
    r64, c64 = rows.astype(np.float64), cols.astype(np.float64)
    J, I, FV, FU = np.meshgrid(np.arange(h), np.arange(w), fr, fr, indexing="ij")
    xi0 = (r64[J] + FV * (r64[J + 1] - r64[J])).astype(F32)
    xi1 = (c64[J, I] + FU * (c64[J, I + 1] - c64[J, I])).astype(F32)
    return _cases([xi0.ravel(), xi1.ravel()]), ((FV == 0.5) & (FU == 0.5)).ravel()


@functools.lru_cache(maxsize=None)
def _grid_cases(name):
    """fn 14: directions at an 8 x 8 midpoint grid inside every texel.  Returns (cases, sin(theta) float64, texel area du dv)"""
    h, w = _maps()[name].shape[:2]
    u = (np.arange(8 * w) + 0.5) / (8.0 * w)
    v = (np.arange(8 * h) + 0.5) / (8.0 * h)
    V, U = np.meshgrid(v, u, indexing="ij")
    phi, theta = (U - 0.5) * 2.0 * PI, V * PI
    d = np.stack([np.sin(theta) * np.cos(phi), np.cos(theta), np.sin(theta) * np.sin(phi)], axis=-1).reshape(-1, 3)
    return _cases([d[:, 0], d[:, 1], d[:, 2]]), np.sin(theta).ravel(), 1.0 / (64.0 * w * h)


@functools.lru_cache(maxsize=None)
def _host(fn, name, kind):
    cases = {"search": lambda: _search_cases(name), "trip": lambda: _trip_cases(name)[0], "grid": lambda: _grid_cases(name)[0]}[kind]()
    out = emu_api.selftest_env(fn, _maps()[name], cases)
    out.setflags(write=False)
    return out


def _device(prt, fn, name, cases):
    scene = prt.HostScene("cornell_open.json")
    cfg = scene.config()
    cfg.env_importance_sampling = 1
    r = prt.Renderer(cfg, device=0)
    try:
        r.upload_envmap(_maps()[name])
        return r.selftest_fn(fn, np.zeros(80, dtype=F32), cases)
    finally:
        r.close()
        scene.close()


def _same_bits(dev, host, what):
    bad = np.argwhere(dev.view(np.uint32) != host.view(np.uint32))
    assert not len(bad), "%s: device != host compilation at %d values, first (case, word) %s: %r vs %r" % (
        what, len(bad), bad[0].tolist(), dev[tuple(bad[0])], host[tuple(bad[0])])


def _ij(out):
    return out[:, 4].copy().view(np.uint32).astype(np.int64), out[:, 5].copy().view(np.uint32).astype(np.int64)


def _reference(name, cases):
    """float64: from the float32 tables, the search (searchsorted) and env_sample's formulas.  Returns i, j, d [n, 3], pdf, sin(theta), (u w, v h)"""
    rows, cols = _tables(name)
    h, w = cols.shape[0], cols.shape[1] - 1
    xi0, xi1 = cases[:, 0], cases[:, 1]
    j = np.searchsorted(rows, xi0, side="right").astype(np.int64) - 1
    i = np.zeros_like(j)
    for row in range(h):
        sel = j == row
        i[sel] = np.searchsorted(cols[row], xi1[sel], side="right") - 1
    r0, r1 = rows[j].astype(np.float64), rows[j + 1].astype(np.float64)
    c0, c1 = cols[j, i].astype(np.float64), cols[j, i + 1].astype(np.float64)
    fv, fu = (xi0.astype(np.float64) - r0) / (r1 - r0), (xi1.astype(np.float64) - c0) / (c1 - c0)
    uw, vh = i + fu, j + fv
    phi, theta = (uw / w - 0.5) * 2.0 * PI, vh / h * PI
    d = np.stack([np.sin(theta) * np.cos(phi), np.cos(theta), np.sin(theta) * np.sin(phi)], axis=-1)
    with np.errstate(divide="ignore"):
        pdf = (r1 - r0) * (c1 - c0) * w * h / (2.0 * PI * PI * np.sin(theta))
    return i, j, d, pdf, np.sin(theta), (uw, vh)


# ---- search, direction, density ---------------------------------------------------------------------------------------------------------
def check_search(name, cases, out):
    """the texel fn 13 chose == searchsorted(table, xi, 'right') - 1 on the float32 tables, the column in the row of the chosen j; direction
    within 4e-6 per component and density within 2e-5 (where sin(theta) >= 0.05) of the float64 formulas on those tables"""
    i, j, d, pdf, st, _ = _reference(name, cases)
    di, dj = _ij(out)
    bad = np.flatnonzero((di != i) | (dj != j))
    assert not len(bad), (name, len(bad), cases[bad[0], :2].tolist(), (int(di[bad[0]]), int(dj[bad[0]])), (int(i[bad[0]]), int(j[bad[0]])))
    err = np.abs(out[:, 0:3].astype(np.float64) - d).max()
    assert err <= 4e-6, (name, err)
    p = out[:, 3].astype(np.float64)
    assert np.isfinite(p).all() and (p >= 0.0).all(), name
    far = st >= 0.05
    rel = np.abs(p[far] / pdf[far] - 1.0).max() if far.any() else 0.0
    print("%s: %d cases, direction error %.2e, density error %.2e over %d cases off the poles" % (name, len(cases), err, rel, int(far.sum())))
    assert rel <= 2e-5, (name, rel)


@pytest.mark.parametrize("name", MAPS)
def test_search_direction_and_density(prt, name):
    check_search(name, _search_cases(name), _host(13, name, "search"))


@pytest.mark.gpu
@pytest.mark.parametrize("name", MAPS)
def test_gpu_search_direction_and_density(prt, name):
    dev = _device(prt, 13, name, _search_cases(name))
    _same_bits(dev, _host(13, name, "search"), name)
    check_search(name, _search_cases(name), dev)


# ---- round trip -------------------------------------------------------------------------------------------------------------------------
def check_round_trip(name, cases, mid, out):
    """samples whose (u w, v h) are at least 0.01 inside their texel (at least 95 % of the cases): env_pdf(d) == the sample's pdf within 2e-5,
    d maps back to the texel the search chose, and at bin midpoints env_lookup(d) is that texel within 4e-5 max(map)"""
    env = _maps()[name]
    h, w = env.shape[:2]
    i, j, d, pdf, st, (uw, vh) = _reference(name, cases)
    di, dj = _ij(out)
    assert (di == i).all() and (dj == j).all(), name
    fu, fv = uw - np.floor(uw), vh - np.floor(vh)
    inside = (fu >= 0.01) & (fu <= 0.99) & (fv >= 0.01) & (fv <= 0.99)
    assert inside.mean() >= 0.95, (name, inside.mean())
    p, q = out[:, 3].astype(np.float64), out[:, 6].astype(np.float64)
    assert np.isfinite(p).all() and np.isfinite(q).all() and (p > 0).all() and (q >= 0).all(), name
    rel = np.abs(q[inside] / p[inside] - 1.0)
    dd = out[:, 0:3].astype(np.float64)
    bu = (np.arctan2(dd[:, 2], dd[:, 0]) / (2.0 * PI) + 0.5) * w
    bv = np.arccos(np.clip(dd[:, 1], -1.0, 1.0)) / PI * h
    back = (np.floor(bu).astype(np.int64) == i) & (np.floor(bv).astype(np.int64) == j)
    assert back[inside].all(), (name, int((~back[inside]).sum()))
    worst = int(np.argmax(rel))
    print("%s: %d cases, %.1f %% inside, env_pdf(d) / pdf - 1 at most %.2e (sin(theta) there %.3f)" % (
        name, len(cases), 100.0 * inside.mean(), rel.max(), st[inside][worst]))
    assert rel.max() <= 2e-5, (name, rel.max(), st[inside][worst])
    look = out[mid, 7:10].astype(np.float64)
    texel = env[j[mid], i[mid]].astype(np.float64)
    assert mid.sum() == w * h and np.abs(look - texel).max() <= 4e-5 * float(env.max()), (name, np.abs(look - texel).max())


@pytest.mark.parametrize("name", MAPS)
def test_round_trip(prt, name):
    cases, mid = _trip_cases(name)
    check_round_trip(name, cases, mid, _host(13, name, "trip"))


@pytest.mark.gpu
@pytest.mark.parametrize("name", MAPS)
def test_gpu_round_trip(prt, name):
    cases, mid = _trip_cases(name)
    dev = _device(prt, 13, name, cases)
    _same_bits(dev, _host(13, name, "trip"), name)
    check_round_trip(name, cases, mid, dev)


# ---- normalisation and positivity through fn 14 ------------------------------------------------------------------------------------------
def check_normalisation(name, out, st, area):
    """sum of env_pdf 2 pi^2 sin(theta) du dv over an 8 x 8 midpoint grid per texel == 1 within 1e-4 (the integrand is constant per texel in
    (u, v): the midpoint rule is exact up to rounding), and env_pdf > 0 wherever env_lookup is"""
    p = out[:, 0].astype(np.float64)
    assert np.isfinite(p).all() and (p >= 0).all(), name
    total = float((p * 2.0 * PI * PI * st * area).sum())
    print("%s: integral of env_pdf over the sphere %.7f" % (name, total))
    assert abs(total - 1.0) <= 1e-4, (name, total)
    lit = (out[:, 1:4] > 0).any(axis=1)
    assert lit.any() and (p[lit] > 0).all(), (name, int((p[lit] <= 0).sum()))


@pytest.mark.parametrize("name", BIG + ("black7x5",))
def test_density_integrates_to_one_and_covers_the_lookup(prt, name):
    cases, st, area = _grid_cases(name)
    check_normalisation(name, _host(14, name, "grid"), st, area)


@pytest.mark.gpu
@pytest.mark.parametrize("name", BIG + ("black7x5",))
def test_gpu_density_integrates_to_one_and_covers_the_lookup(prt, name):
    cases, st, area = _grid_cases(name)
    dev = _device(prt, 14, name, cases)
    _same_bits(dev, _host(14, name, "grid"), name)
    check_normalisation(name, dev, st, area)


@pytest.mark.gpu
def test_gpu_env_selftest_needs_the_tables(prt):
    """fn 13 / 14 without a map uploaded under the mode: PRT_ERR_INVALID_ARGUMENT"""
    scene = prt.HostScene("cornell_open.json")
    for mode, upload in ((1, False), (0, True)):
        cfg = scene.config()
        cfg.env_importance_sampling = mode
        r = prt.Renderer(cfg, device=0)
        if upload:
            r.upload_envmap(_maps()["const"])
        for fn in (13, 14):
            with pytest.raises(prt.PrtError) as ei:
                r.selftest_fn(fn, np.zeros(80, dtype=F32), np.zeros((3, 32), dtype=F32))
            assert ei.value.code == prt.PRT_ERR_INVALID_ARGUMENT and "fn 13 / 14" in str(ei.value)
        r.close()
    scene.close()


# ---- the estimator, per 8 x 8 block against the default mode -----------------------------------------------------------------------------
W, H, R = 64, 48, 32
CAPS = {"MAX_BOUNCES": 12, "MAX_DIFF_BOUNCES": 6, "MAX_SPEC_BOUNCES": 12, "MAX_TRANS_BOUNCES": 12, "MAX_SCATTERING_EVENTS": 12, "MARCHING_STEPS": 128,
        "SHADOW_MARCHING_STEPS": 64}
LIGHT = {"pos": [0.0, 3.0, 0.0], "radius": 0.25, "material": {"color": [8.0, 8.0, 8.0], "type": 0}}     # without a light nothing takes the MIS branch
GROUND = {"vertices": [0.0, 0.0, 0.0, 8.0, 0.0, 0.0, 0.0, 0.0, 8.0], "material": {"color": [0.5, 0.5, 0.5]}}


def _scene_json(spheres, **caps):
    return json.dumps({"settings": dict(CAPS, **caps), "scene": {"spheres": [LIGHT] + spheres, "quads": [GROUND]}})


SPHERES_A = [{"pos": [-1.2, 0.5, 0.3], "radius": 0.5, "material": {"color": [0.7, 0.7, 0.7], "type": 1}},                               # diffuse
             {"pos": [0.0, 0.5, 0.6], "radius": 0.5, "material": {"color": [0.9, 0.8, 0.6], "type": 10, "dist": 2, "roughness": 0.3}},   # GGX rough conductor
             {"pos": [1.2, 0.5, 0.3], "radius": 0.5, "material": {"color": [0.9, 0.9, 0.9], "type": 4, "roughness": 0.15}}]              # coat
SPHERES_B = [{"pos": [-0.8, 0.6, 0.5], "radius": 0.6, "material": {"color": [1.0, 1.0, 1.0], "type": 11, "dist": 2, "roughness": 0.2}},  # rough dielectric
             {"pos": [0.9, 0.6, 0.3], "radius": 0.6, "material": {"color": [0.95, 0.95, 0.95], "type": 2}}]                              # smooth mirror


def _scene(prt, which):
    if which == "a":
        return prt.HostScene(_scene_json(SPHERES_A), text=True)
    if which == "a_cap":                                               # one diffuse bounce: every diffuse vertex fills the cap
        return prt.HostScene(_scene_json(SPHERES_A, MAX_DIFF_BOUNCES=1), text=True)
    if which == "b":
        return prt.HostScene(_scene_json(SPHERES_B), text=True)
    return prt.HostScene("cornell_open.json")                          # (c): the teapot mesh -- the shadow ray from the vertex walks the tree with tmax = inf


def _sky(prt, which):
    return {"sky": lambda: prt.make_sky(64, 32), "seam": lambda: _maps()["seam0"], "pole": lambda: _maps()["pole"], "const": lambda: _maps()["const"]}[which]()


def block_means(prt, which, sky, mode, spp, first, backend="gpu"):
    """R independent renders of `spp` complete paths per pixel -> float64 [R, H / 8, W / 8, 3] of 8 x 8 block means, and the variants that ran.
    Render k takes the seed pairs of frames first + k n .. first + (k + 1) n - 1, n = 13 spp (no path has more than 13 segments under these caps:
    the ranges are disjoint).  "N spp" renders, not a fixed number of frames: after n frames a pixel is usually in the middle of a path that `samples` already
    counts, and the default mode -- which looks the map up one segment later than the mode under test -- loses more to that than the mode does: a
    difference of 0.35 % at 256 frames that is the truncation's, not the estimator's"""
    scene = _scene(prt, which)
    cfg = scene.config()
    cfg.env_importance_sampling = mode
    cam = prt.default_camera(W, H)
    env = _sky(prt, sky)
    out = np.zeros((R, H // 8, W // 8, 3))
    ran = set()
    n = 13 * spp
    bad = 0
    r = None
    if backend == "gpu":
        r = prt.Renderer(cfg, device=0)
        r.upload_scene(scene); r.upload_envmap(env); r.set_camera(cam); r.resize(W, H)
    for k in range(R):
        seeds = prt.seed_pairs(n, first_frame=first + k * n)
        if r is not None:
            if k:
                r.reset()
            r.render_spp(spp, seeds)
            img, samples = r.read_framebuffer(), r.read_state()["samples"]
            ran.add(r.kernel_variant())
        else:
            st, img = emu_api.render(np.dtype(prt._capi.PATH_STATE_DTYPE), cfg, scene.desc, cam, W, H, seeds, env=env, spp_limit=spp)
            samples = st["samples"]
            ran.add(emu_api.last_variant())
        assert (samples == spp).all(), (which, sky, mode, k)
        # (a pixel that is not finite counts as black, in either mode, as in test_gpu_parity's convergence test: the default mode -- the
        # reference's arithmetic -- has one in a few hundred thousand under the block maps, and the spread of the renders sees it)
        a = np.nan_to_num(img[..., :3].astype(np.float64), nan=0.0, posinf=0.0, neginf=0.0)
        bad += int((~np.isfinite(img[..., :3])).any(axis=-1).sum())
        out[k] = a.reshape(H // 8, 8, W // 8, 8, 3).mean(axis=(1, 3))
    if r is not None:
        r.close()
    scene.close()
    assert bad <= 8, (which, sky, mode, bad)
    return out, ran


def block_verdict(b0, b1, label):
    """z = (m1 - m0) / sqrt(e0^2 + e1^2) per block and channel, the standard errors from the spread of the R renders; over the blocks whose
    mean is above 5 % of the image mean.  Returns what the assertions need (and prints it)"""
    m0, m1 = b0.mean(axis=0), b1.mean(axis=0)
    e0, e1 = b0.std(axis=0, ddof=1) / np.sqrt(len(b0)), b1.std(axis=0, ddof=1) / np.sqrt(len(b1))
    counted = m0 > 0.05 * m0.mean(axis=(0, 1))
    e = np.sqrt(e0 ** 2 + e1 ** 2)[counted]
    with np.errstate(divide="ignore", invalid="ignore"):             # (a block of sky pixels under a constant map: no spread, and no difference)
        z = np.where(e > 0, (m1 - m0)[counted] / e, np.where((m1 - m0)[counted] == 0, 0.0, np.inf))
    e_rel = e / m0[counted]
    ratio = m1[counted] / m0[counted] - 1.0
    v = {"n": int(counted.sum()), "max_z": float(np.abs(z).max()), "mean_z": float(abs(z.mean()) * np.sqrt(z.size)),
         "resolved": float((e_rel <= 0.02).mean()), "ratio_excess": float((np.abs(ratio) - (5.0 * e_rel + 0.002)).max()),
         "worst_ratio": float(ratio[np.argmax(np.abs(z))]), "e90": float(np.quantile(e_rel, 0.9))}
    print("%s: %d blocks counted, max |z| %.2f, |mean z| sqrt(n) %.2f, %.1f %% of them resolved to 2 %% (90 %% to %.2f %%), worst block m1 / m0 - 1 = %+.4f" % (
        label, v["n"], v["max_z"], v["mean_z"], 100.0 * v["resolved"], 100.0 * v["e90"], v["worst_ratio"]))
    return v


def assert_same_expectation(v, label):
    assert v["resolved"] >= 0.90, (label, v)                          # (a test that passes through being insensitive is no test)
    assert v["max_z"] < 5.0, (label, v)
    assert v["mean_z"] < 5.0, (label, v)
    assert v["ratio_excess"] < 0.0, (label, v)


# Paths per pixel and render (R = 32 renders each): chosen on the host compilation so that the combined standard error of a block is at most 2 % for
# 90 % of the counted blocks in the comparison AND between two independent default-mode sets, which pass the same assertions (DESIGN.md has the
# figures).  Under the block maps the default mode finds the block by BSDF sampling alone: twice the paths.  The cap case's ground is lit by the
# small light only (dark and noisy): 1024.
SPP = {"sky": 96, "seam": 192, "pole": 192, "const": 1024}
COMBOS = [(s, m) for s in ("a", "b", "c") for m in ("sky", "seam", "pole")]
_sets = {}


def _set(prt, which, sky, mode, second=False):
    """the R renders of one scene, map and mode (computed once); second: an independent set (the seed pairs after the first set's)"""
    key = (which, sky, mode, second)
    if key not in _sets:
        spp = SPP[sky]
        t = time.time()
        b, ran = block_means(prt, which, sky, mode, spp, 1 + (R * 13 * spp if second else 0))
        print("%s / %s, mode %d%s: %d x %d paths per pixel in %.2f s; %s" % (which, sky, mode, ", second set" if second else "", R, spp, time.time() - t, sorted(ran)))
        # the variant names the mode in every launch of a mode-1 render, and in none of the default's
        assert ran and all(("env_importance_sampling" in v) == bool(mode) for v in ran), ran
        b.setflags(write=False)
        _sets[key] = b
    return _sets[key]


@pytest.mark.gpu
@pytest.mark.parametrize("which,sky", COMBOS)
def test_gpu_block_means_match_the_default_mode(prt, which, sky):
    """8 x 8 block means of a 64 x 48 frame, mode on against the default mode: per block and channel z = (m1 - m0) / sqrt(e0^2 + e1^2) with the
    standard errors from R = 32 independent renders.  Over the blocks above 5 % of the image mean: max |z| < 5, |mean z| sqrt(n) < 5 (a small bias of
    one sign everywhere), |m1 / m0 - 1| < 5 e_rel + 0.002 -- and at least 90 % of those blocks resolved to 2 %.  (a): diffuse, GGX conductor and coat
    spheres on a grey ground; (b): rough dielectric and mirror; (c): cornell_open with its teapot mesh; each under a sky with a sun, a 3 x 3 block
    of 200 across the map's seam and one on the pole row"""
    v = block_verdict(_set(prt, which, sky, 0), _set(prt, which, sky, 1), "%s / %s, mode on vs default" % (which, sky))
    assert_same_expectation(v, (which, sky))


@pytest.mark.gpu
@pytest.mark.parametrize("sky", ("sky", "seam", "pole"))
def test_gpu_block_statistic_is_calibrated(prt, sky):
    """two independent default-mode sets pass the same assertions against each other at the same counts (scene (a))"""
    v = block_verdict(_set(prt, "a", sky, 0), _set(prt, "a", sky, 0, second=True), "a / %s, default vs default" % sky)
    assert_same_expectation(v, ("a", sky, "calibration"))


@pytest.mark.gpu
def test_gpu_block_means_match_the_default_mode_at_a_bounce_cap(prt):
    """scene (a) with MAX_DIFF_BOUNCES = 1 under the constant map.  In the default mode a vertex that fills a cap resets the path at the end of its
    segment, so the BSDF-sampled ray that escapes from it is never looked up: diffuse and glossy surfaces get no sky light at all.  The mode must
    do the same (lane_back: no map sample and no escaped-ray term at a vertex whose counters reset the path) -- before that the spheres' blocks
    were off by z = 80"""
    v = block_verdict(_set(prt, "a_cap", "const", 0), _set(prt, "a_cap", "const", 1), "a with MAX_DIFF_BOUNCES = 1 / const, mode on vs default")
    assert_same_expectation(v, "cap")
