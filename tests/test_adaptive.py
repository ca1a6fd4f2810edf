"""Adaptive sampling (prt_render_adaptive, include/prt.h): every pixel renders paths until the standard error of its mean luminance is below
rel_err x max(mean, abs_floor), between min_spp and max_spp paths.  The contract checked here: a pixel frozen after k paths is bit for bit the
same pixel of prt_render_spp(k); the freeze decision is the documented float32 arithmetic, which the host repeats in numpy; no schedule
(wave-count build, pixel mapping, launch length, run-ahead, pacing, live-pixel lists, streams, row blocks) changes a bit."""
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from conftest import ROOT, variant_camera
from support import bytes_rows as _bytes, pkg as _pkg, variant_case

PKG = os.path.join(ROOT, "photorealistic-rendering-using-opencl_amd")
HIP = os.path.join(PKG, "csrc", "hip")
HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"


# ---- the convergence test on the host (no GPU) -----------------------------------------------------------------------------------------

def _conv(l, s2, n, rel_err, abs_floor):
    c, se, m = _pkg().adaptive_converged(np.float32(l), np.float32(s2), n, rel_err, abs_floor)
    return bool(c), float(se), float(m)


def test_convergence_helper_zero_variance():
    # four paths of luminance 0.5: l = 2, s2 = 4 x 0.25 = 1, m = 0.5, v = (1 - 2 x 0.5) / 12 = 0
    c, se, m = _conv(2.0, 1.0, 4, 0.01, 0.0)
    assert c and se == 0.0 and m == 0.5
    assert not _conv(2.0, 1.0, 4, 0.0, 0.0)[0]           # rel_err = 0 never converges (strict: 0 < 0 is false)
    # six paths of the same luminance c (the light seen directly): the plane's recurrence, and s2 - l m rounds below zero; v is held at 0
    c, l, s2 = np.float32(0.5118216), np.float32(0), np.float32(0)
    for _ in range(6):
        lum = l + c
        y = lum - l
        l, s2 = lum, s2 + y * y
    assert s2 - l * (l / np.float32(6)) < 0
    conv, se, _ = _conv(l, s2, 6, 0.0, 0.0)
    assert not conv and se == 0.0                          # rel_err = 0 still never converges
    assert _conv(l, s2, 6, 1e-6, 0.0)[0]


def test_convergence_helper_dark_pixel_under_the_floor():
    # l = 0 after two paths with increments +0.1, -0.1: s2 = 0.02, m = 0, v = 0.02 / 2 = 0.01 -> standard error 0.1
    assert _conv(0.0, 0.02, 2, 0.2, 1.0)[0]               # t = 0.2 x max(0, 1) = 0.2: 0.01 < 0.04
    assert not _conv(0.0, 0.02, 2, 0.2, 0.25)[0]          # t = 0.05: 0.01 < 0.0025 fails
    assert not _conv(0.0, 0.0, 2, 1e30, 0.0)[0]           # a black pixel without a floor: t = 0, never converged


def test_convergence_helper_at_min_spp():
    # n = 2, increments 0 and 1: l = 1, s2 = 1, m = 0.5, v = (1 - 0.5) / 2 = 0.25, t = rel_err x 0.5
    assert not _conv(1.0, 1.0, 2, 1.0, 0.0)[0]            # t^2 = 0.25: strict
    assert _conv(1.0, 1.0, 2, 1.01, 0.0)[0]
    c, se, m = _conv(1.0, 1.0, 2, 1.0, 0.0)
    assert se == 0.5 and m == 0.5


def test_convergence_helper_is_float32_in_the_documented_order():
    rng = np.random.default_rng(7)
    n = rng.integers(2, 5000, 4000).astype(np.uint32)
    l = (rng.random(4000) * n).astype(np.float32)
    s2 = (l * rng.random(4000) * 3).astype(np.float32)
    c, _, _ = _pkg().adaptive_converged(l, s2, n, 0.05, 0.01)
    f = np.float32
    m = np.array([f(a) / f(b) for a, b in zip(l, n)], dtype=f)
    v = np.array([max((f(s) - f(a) * f(mm)) / (f(b) * f(b - 1)), f(0)) for a, s, b, mm in zip(l, s2, n, m)], dtype=f)
    t = np.array([f(0.05) * max(f(mm), f(0.01)) for mm in m], dtype=f)
    assert (c == (v < t * t)).all()
    acc = rng.random((100, 4)).astype(np.float32)
    lum = _pkg().adaptive_luminance(acc)
    assert lum.dtype == np.float32
    assert all(lum[k] == (f(0.2126) * acc[k, 0] + f(0.7152) * acc[k, 1]) + f(0.0722) * acc[k, 2] for k in range(100))


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="no hipcc")
def test_adaptive_build_keeps_uniform_loads_scalar(tmp_path):
    """the adaptive build of the headline set (render_kernel_adaptive) within the bounds tests/test_codegen.py holds render_kernel to"""
    out = tmp_path / "light_diff.s"
    cmd = [HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=off", "-fno-fast-math", "-fno-slp-vectorize", "-S",
           "--cuda-device-only", "-I" + os.path.join(ROOT, "include"), "-I" + HIP, "-o", str(out), os.path.join(HIP, "pt_inst_light_diff.hip")]
    subprocess.run(cmd, check=True, capture_output=True, timeout=1800)
    kernels, cur = {}, None
    for line in out.read_text().split("\n"):
        m = re.match(r"^(_ZN3prt22render_kernel_adaptive\w+):", line)
        if m:
            cur = m.group(1)
            kernels[cur] = [0, 0]
        elif line.startswith(".Lfunc_end"):
            cur = None
        elif cur:
            m = re.match(r"\s+s_load_dword(x(\d+))?\s", line)
            if m:
                kernels[cur][0] += int(m.group(2) or 1)
            elif re.match(r"\s+global_load", line):
                kernels[cur][1] += 1
    assert len(kernels) == 2, kernels                          # medium off / on, one wave-count build
    for k, (scalar_dw, vector) in kernels.items():
        assert scalar_dw >= 240 and vector <= 45, (k, scalar_dw, vector)


# ---- on the GPU ------------------------------------------------------------------------------------------------------------------------

def _setup(prt, variant, W, H):
    scene, cfg, cam, env = variant_case(prt, variant, W, H)
    r = prt.Renderer(cfg, device=0)
    r.upload_scene(scene)
    if env is not None:
        r.upload_envmap(env)
    r.set_camera(cam)
    r.resize(W, H)
    return scene, cfg, cam, env, r


def _bits(img):
    return np.ascontiguousarray(img).view(np.uint32).reshape(-1, 4)


def _same_pixels(a, b, mask, what):
    (sa, ia), (sb, ib) = a, b
    bad = np.nonzero(mask & ~((_bytes(sa) == _bytes(sb)).all(1) & (_bits(ia) == _bits(ib)).all(1)))[0]
    assert bad.size == 0, "%s: %d pixels differ, first %s" % (what, bad.size, bad[:8])


def _frames(spp):
    return spp * 16 + 64


MIN, MAX, REL = 8, 64, 0.2          # (at 0.05 nearly every coat pixel needs more than 64 paths: the test would see one count)


def _adaptive(r, seeds, min_spp=MIN, max_spp=MAX, rel_err=REL, abs_floor=0.0):
    r.reset()
    used = r.render_adaptive(seeds, min_spp, max_spp, rel_err, abs_floor)
    return r.read_state(), r.read_framebuffer().reshape(-1, 4), used


def _spp(r, seeds, k):
    r.reset()
    r.render_spp(k, seeds)
    return r.read_state(), r.read_framebuffer().reshape(-1, 4)


@pytest.mark.gpu
@pytest.mark.parametrize("variant", ["cornell_coat", "cornell_roughdiel", "cornell_media"])
def test_each_pixel_equals_the_spp_render_of_its_own_count(prt, oracle, variant):
    W, H = 64, 48
    scene, cfg, cam, env, r = _setup(prt, variant, W, H)
    seeds = prt.seed_pairs(_frames(MAX))
    state, img, used = _adaptive(r, seeds)
    assert "adaptive" in r.kernel_variant(), r.kernel_variant()
    k = state["samples"]
    assert (state["reset"] != 0).all() and ((k >= MIN) & (k <= MAX)).all()
    ks = np.unique(k)
    assert len(ks) >= 3 and (k < MAX).any(), ks                 # not vacuous: pixels stopped at different counts
    for kk in ks:
        _same_pixels((state, img), _spp(r, seeds, int(kk)), k == kk, "%s: pixels of %d paths vs prt_render_spp(%d)" % (variant, kk, kk))
    # the CPU restatement of the reference under the "N spp" rule, for the smallest count
    k0 = int(ks[0])
    ostate, oimg = oracle.Restatement().render(cfg, scene.desc, cam, W, H, seeds, env=env, spp_limit=k0, threads=16)
    mask = k == k0
    bad = oracle.state_fields_equal(ostate[mask], state.view(oracle.PATH_STATE_DTYPE)[mask])
    assert not bad, "%s: %d-path pixels vs the oracle: %s" % (variant, k0, bad)
    assert (_bits(oimg.reshape(-1, 4))[mask] == _bits(img)[mask]).all()
    r.close()


@pytest.mark.gpu
def test_freeze_rule_is_the_documented_arithmetic(prt):
    """l is the float32 luminance of acc bit for bit; and, from renders that never converge (rel_err 0) with max_spp = j for every j, the host
    finds each pixel's count of the adaptive render: the first j whose plane passes the test in numpy float32, else max_spp"""
    W, H = 64, 48
    scene, cfg, cam, env, r = _setup(prt, "cornell_coat", W, H)
    seeds = prt.seed_pairs(_frames(MAX))
    state, img, _ = _adaptive(r, seeds)
    plane = r.read_adaptive_stats()
    lum = prt.adaptive_luminance(state["acc"])
    assert (lum.view(np.uint32) == plane[:, 0].view(np.uint32)).all()
    k = state["samples"].astype(np.int64)
    first = np.full(W * H, MAX, dtype=np.int64)
    for j in range(MIN, MAX + 1):
        sj, ij, _ = _adaptive(r, seeds, MIN, j, 0.0)
        assert (sj["samples"] == j).all()
        pj = r.read_adaptive_stats()
        conv, _, _ = prt.adaptive_converged(pj[:, 0], pj[:, 1], np.full(W * H, j, np.uint32), REL, 0.0)
        first = np.where((first == MAX) & conv & (j < MAX), j, first)
    assert (first == k).all(), np.nonzero(first != k)[0][:8]
    r.close()


@pytest.mark.gpu
def test_ends_of_the_range(prt):
    W, H = 64, 48
    scene, cfg, cam, env, r = _setup(prt, "cornell_roughdiel", W, H)
    seeds = prt.seed_pairs(_frames(MAX))
    all_px = np.ones(W * H, bool)
    s0, i0, _ = _adaptive(r, seeds, MIN, MAX, 0.0)                # never converges: the "N spp" render of max_spp
    _same_pixels((s0, i0), _spp(r, seeds, MAX), all_px, "rel_err 0 vs prt_render_spp(max_spp)")
    s1, i1, _ = _adaptive(r, seeds, MIN, MAX, 1e30, 1.0)          # converges at once: min_spp
    assert (s1["samples"] == MIN).all()
    _same_pixels((s1, i1), _spp(r, seeds, MIN), all_px, "huge rel_err vs prt_render_spp(min_spp)")
    r.close()


@pytest.mark.gpu
def test_schedules_change_no_bit(prt, monkeypatch):
    W, H = 96, 64
    seeds = prt.seed_pairs(_frames(MAX))
    scene, cfg, cam, env, r = _setup(prt, "cornell_coat", W, H)
    r.set_option("compact", 0)
    ref = _adaptive(r, seeds)[:2]
    assert r.adaptive_report().list_launches == 0
    cases = [("waves", 5), ("waves", 6), ("scatter", 0), ("scatter", 1), ("frames_per_launch", 3), ("run_ahead", 0), ("run_ahead", 1),
             ("pace", 0), ("pace", 1), ("compact", 0), ("compact", 1)]
    all_px = np.ones(W * H, bool)
    lists = 0
    for name, value in cases:
        r.set_option("compact", 1)
        r.set_option("frames_per_launch", 16)               # short launches: the live pixels drop below the list threshold early
        r.set_option(name, value)
        got = _adaptive(r, seeds)[:2]
        _same_pixels(ref, got, all_px, "adaptive under %s=%s" % (name, value))
        rep = r.adaptive_report()
        lists += rep.list_launches
        if name == "compact" and value == 1:
            assert rep.list_builds >= 1 and rep.list_launches >= 1 and 0 < rep.list_live_lanes <= rep.list_lanes, \
                (rep.list_builds, rep.list_launches, rep.list_live_lanes, rep.list_lanes)
        for n, v in (("waves", 0), ("scatter", -1), ("run_ahead", 1), ("pace", 1)):
            r.set_option(n, v)
    assert lists > 0
    r.close()
    for streams in ("1", "2"):
        monkeypatch.setenv("PRT_STREAMS", streams)
        scene, cfg, cam, env, r = _setup(prt, "cornell_coat", W, H)
        r.set_option("frames_per_launch", 16)
        got = _adaptive(r, seeds)[:2]
        assert r.stats().concurrent == int(streams)
        _same_pixels(ref, got, all_px, "adaptive with PRT_STREAMS=%s" % streams)
        r.close()


@pytest.mark.gpu
def test_live_list_past_one_scan_run_and_with_a_ragged_tail(prt, monkeypatch):
    """331 x 199 = 65 869 pixels: 1 030 wave counts, so each of live_scan_kernel's 1 024 threads sums a run of two and the threads above 514
    have empty runs; the last wave of live_count / live_write has 13 pixels; neither side is a multiple of the 8 x 8 tile.  Lists from the first
    freeze on (compact_below 100), on a context whose list buffers were sized for a smaller frame before"""
    W, H = 331, 199
    assert (W * H + 63) // 64 == 1030 and W * H % 64 == 13
    seeds = prt.seed_pairs(_frames(MAX))
    all_px = np.ones(W * H, bool)
    scene, cfg, cam, env, r = _setup(prt, "cornell_coat", W, H)
    r.set_option("compact", 0)
    ref = _adaptive(r, seeds)[:2]
    assert r.adaptive_report().list_launches == 0
    assert len(np.unique(ref[0]["samples"])) >= 3, np.unique(ref[0]["samples"])
    r.close()
    for streams in ("1", "2"):
        monkeypatch.setenv("PRT_STREAMS", streams)
        scene, cfg, cam, env, r = _setup(prt, "cornell_coat", 64, 48)
        for name, value in (("compact", 1), ("compact_below", 100), ("frames_per_launch", 16)):
            r.set_option(name, value)
        _adaptive(r, seeds)                                   # allocates the list and its wave counts for 3 072 pixels
        assert r.adaptive_report().list_builds >= 1
        r.resize(W, H)
        r.set_camera(variant_camera(prt, "cornell_coat", W, H))
        got = _adaptive(r, seeds)[:2]
        assert r.stats().concurrent == int(streams)
        _same_pixels(ref, got, all_px, "lists from the first freeze on, PRT_STREAMS=%s, after a 64 x 48 render on the same context" % streams)
        rep = r.adaptive_report()
        assert rep.list_builds >= 2 and rep.list_launches >= 1 and 0 < rep.list_live_lanes <= rep.list_lanes, \
            (rep.list_builds, rep.list_launches, rep.list_live_lanes, rep.list_lanes)
        r.close()


@pytest.mark.gpu
def test_schedules_change_no_bit_through_the_big_tree(prt, monkeypatch):
    """the 871 k-triangle stand-in on a strip of its 1080p frame (rows through the mesh): tiles and lists, tile order on and off"""
    W, H, row0, rows = 1920, 1080, 500, 24
    prt.ensure_dragon_standin()
    scene = prt.HostScene("cornell_dragon.json")
    seeds = prt.seed_pairs(_frames(8))
    out = []
    for compact, order in ((0, 1), (1, 1), (1, 0)):
        r = prt.Renderer(scene.config(), device=0)
        r.upload_scene(scene)
        r.set_camera(prt.default_camera(W, H))
        r.set_tile(W, H, row0, rows)
        r.set_option("compact", compact)
        r.set_option("tile_order", order)
        r.set_option("frames_per_launch", 4)
        r.render_adaptive(seeds, 2, 8, 0.1, 0.01)
        out.append((r.read_state(), r.read_framebuffer().reshape(-1, 4)))
        if compact:
            assert r.adaptive_report().list_launches > 0
        r.close()
    k = out[0][0]["samples"]
    assert len(np.unique(k)) >= 2, np.unique(k)
    for j in (1, 2):
        _same_pixels(out[0], out[j], np.ones(W * rows, bool), "big tree, schedule %d" % j)


@pytest.mark.gpu
def test_row_blocks_together_are_the_frame(prt):
    W, H, B = 64, 48, 8
    seeds = prt.seed_pairs(_frames(MAX))
    scene, cfg, cam, env, r = _setup(prt, "cornell_coat", W, H)
    full_s, full_i, _ = _adaptive(r, seeds)
    r.close()
    full_s, full_i = full_s.reshape(H, W), full_i.reshape(H, W, 4)
    for part in (0, 1):
        scene, cfg, cam, env, r = _setup(prt, "cornell_coat", W, H)
        r.set_row_blocks(W, H, B, 2, part)
        r.render_adaptive(seeds, MIN, MAX, REL)
        own = [y for y in range(H) if (y // B) % 2 == part]
        _same_pixels((full_s[own].reshape(-1), full_i[own].reshape(-1, 4)), (r.read_state(), r.read_framebuffer().reshape(-1, 4)),
                     np.ones(len(own) * W, bool), "row blocks part %d" % part)
        r.close()


@pytest.mark.gpu
def test_converged_pixels_are_within_their_error_of_a_long_render(prt):
    W, H, lo, hi, rel = 128, 96, 16, 2048, 0.1          # (at 0.05 the coat frame takes 1 413 paths per pixel on average: too close to 2 048)
    scene, cfg, cam, env, r = _setup(prt, "cornell_coat", W, H)
    r.render_adaptive(prt.seed_pairs(_frames(hi)), lo, hi, rel, 0.0)
    st = r.read_state()
    plane = r.read_adaptive_stats()
    n = st["samples"]
    conv, se, m = prt.adaptive_converged(plane[:, 0], plane[:, 1], n, rel, 0.0)
    by_conv = n < hi
    assert by_conv.sum() > 0.2 * W * H and n.mean() < 0.5 * hi, (by_conv.sum(), n.mean())
    assert conv[by_conv].all()
    r.reset()
    r.render_spp(8192, prt.seed_pairs(_frames(8192), first_frame=1000003))      # an independent reference: other seeds
    ref = prt.adaptive_luminance(r.read_framebuffer().reshape(-1, 4)).astype(np.float64)
    off = np.abs(m.astype(np.float64) - ref) > 3.0 * se.astype(np.float64)
    frac = off[by_conv].mean()
    assert frac <= 0.05, frac
    r.close()


@pytest.mark.gpu
def test_refused_combinations(prt):
    W, H = 32, 24
    scene, cfg, cam, env, r = _setup(prt, "cornell_coat", W, H)
    seeds = prt.seed_pairs(_frames(16))
    for args, code in (((1, 16, 0.1, 0.0), prt.PRT_ERR_INVALID_ARGUMENT), ((17, 16, 0.1, 0.0), prt.PRT_ERR_INVALID_ARGUMENT),
                       ((2, 16, -0.1, 0.0), prt.PRT_ERR_INVALID_ARGUMENT), ((2, 16, float("nan"), 0.0), prt.PRT_ERR_INVALID_ARGUMENT),
                       ((2, 16, 0.1, -1.0), prt.PRT_ERR_INVALID_ARGUMENT), ((2, 16, 0.1, float("nan")), prt.PRT_ERR_INVALID_ARGUMENT)):
        with pytest.raises(prt.PrtError) as e:
            r.render_adaptive(seeds, *args)
        assert e.value.code == code, (args, e.value.code)
    r.render_adaptive(seeds, 2, 16, 0.1)
    with pytest.raises(prt.PrtError) as e:                      # not freshly reset
        r.render_adaptive(seeds, 2, 16, 0.1)
    assert e.value.code == prt.PRT_ERR_NOT_READY
    r.reset()
    with pytest.raises(prt.PrtError, match="max_frames") as e:   # the frame budget runs out
        r.render_adaptive(prt.seed_pairs(12), 8, 16, 0.0)
    assert e.value.code == prt.PRT_ERR_NOT_READY
    st = r.read_state()
    assert (st["samples"] < 16).any()
    r.reset()
    assert r.render_adaptive(seeds, 2, 16, 0.1) > 0              # usable again after a reset
    r.close()
    # a debug view overwrites acc
    vs = prt.HostScene("cornell_mixed.json")
    vcfg = vs.config()
    vcfg.view_option = 1
    rv = prt.Renderer(vcfg, device=0)
    rv.upload_scene(vs)
    rv.set_camera(prt.default_camera(W, H))
    rv.resize(W, H)
    with pytest.raises(prt.PrtError) as e:
        rv.render_adaptive(seeds, 2, 16, 0.1)
    assert e.value.code == prt.PRT_ERR_UNSUPPORTED
    rv.close()


@pytest.mark.gpu
def test_cli_renders_adaptively(prt, tmp_path):
    exe = os.path.join(PKG, "prt_render")
    out, spp_map = tmp_path / "a.png", tmp_path / "spp.pfm"
    r = subprocess.run([exe, "-scene", os.path.join(ROOT, "scenes", "cornell_coat.json"), "-models", os.path.join(ROOT, "scenes", "models") + "/",
                        "-width", "64", "-height", "48", "-spp", "256", "-min-spp", "16", "-adaptive", "0.2", "-out", str(out),
                        "-spp-map", str(spp_map)], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr
    assert "adaptive:" in r.stdout and out.stat().st_size > 0
    raw = spp_map.read_bytes()
    data = np.frombuffer(raw[raw.index(b"-1.0\n") + 5:], dtype=np.float32).reshape(48, 64, 3)
    assert data.min() >= 16 and data.max() <= 256 and data.min() < data.max()
