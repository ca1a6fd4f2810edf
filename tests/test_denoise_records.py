"""Denoising a frame rendered in parts, from gathered records (prt_export_denoise_inputs, prt_denoise_records, prt_denoise_records_temporal,
prt_reset_records_history; include/prt.h).  The contract checked here: the records are the words of the framebuffer and the guides plus the
stats variance; the filter over the records of any split of the frame -- row blocks, row tiles, exported part by part -- gives the bits of
prt_denoise / prt_denoise_temporal on one whole-frame context, on a context that has no scene at all; mixed records fall back to the spatial
variance; the filter is prt.h's formulas on synthetic records (an uncovered band, a zero normal, a NaN colour); refused inputs; the calls
write nothing of the context's own frame."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from conftest import ROOT
from cases import denoise_setup as _setup, _export, _synthetic, _torch
from mirrors import denoise_ref, spatial_variance, stats_variance
from support import assert_api, bits as _bits, pkg as _pkg, to_device as _to_device

PKG = os.path.join(ROOT, "photorealistic-rendering-using-opencl_amd")
HIP = os.path.join(PKG, "csrc", "hip")
HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
NEW_API = ("prt_export_denoise_inputs", "prt_denoise_records", "prt_denoise_records_temporal", "prt_reset_records_history")


# ---- no GPU --------------------------------------------------------------------------------------------------------------------------------

def test_api_is_declared_exported_and_bound():
    header = assert_api(NEW_API)
    assert re.search(r"#define\s+PRT_DENOISE_RECORD_FLOATS\s+16\b", header)
    assert _pkg()._capi.DENOISE_RECORD_FLOATS == 16
    for name in ("export_denoise_inputs", "denoise_records", "denoise_records_temporal", "reset_records_history"):
        assert callable(getattr(_pkg().Renderer, name)), name


def test_records_kernels_have_no_scratch():
    cmd = [HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=off", "-fno-fast-math", "-fno-slp-vectorize", "-c",
           "--cuda-device-only", "-I" + os.path.join(ROOT, "include"), "-I" + HIP, "-Rpass-analysis=kernel-resource-usage", "-o", os.devnull,
           os.path.join(HIP, "pt_records.hip")]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stderr[-4000:]
    kernels, lds, cur = {}, {}, None
    for line in r.stderr.splitlines():
        m = re.search(r"Function Name: (\S+)", line)
        if m:
            cur = m.group(1)
        m = re.search(r"ScratchSize \[bytes/lane\]: (\d+)", line)
        if m and cur:
            kernels[cur] = int(m.group(1))
        m = re.search(r"LDS Size \[bytes/block\]: (\d+)", line)
        if m and cur:
            lds[cur] = int(m.group(1))
    names = " ".join(kernels)
    for k in ("rec_export_kernel", "rec_import_kernel"):
        assert k in names, kernels
    assert len(kernels) == 2, kernels
    assert all(v == 0 for v in kernels.values()), kernels
    assert all(v == 0 for v in lds.values()), lds


# ---- on the GPU ------------------------------------------------------------------------------------------------------------------------------

W1, H1 = 100, 70                        # no multiple of 8 or 16; the 62 rows and columns five passes reach cross every edge of the frame
SOURCES, PASSES = ("stats", "spatial"), (1, 5)
# ("blocks", block_rows, n_parts) | ("tiles", cuts)
SPLITS = [("blocks", 8, 2), ("blocks", 8, 3), ("tiles", (0, 40, 70)), ("tiles", (0, 24, 50, 70)), ("tiles", (0, 1, 70))]


def _split_parts(split, H):
    """[(how to set the part on a Renderer, its global rows)]"""
    if split[0] == "blocks":
        _, b, n = split
        return [(("blocks", b, n, k), [y for y in range(H) if (y // b) % n == k]) for k in range(n)]
    cuts = split[1]
    return [(("tile", a, e - a), list(range(a, e))) for a, e in zip(cuts[:-1], cuts[1:])]


def _set_part(r, W, H, how):
    if how[0] == "blocks":
        r.set_row_blocks(W, H, how[1], how[2], how[3])
    else:
        r.set_tile(W, H, how[1], how[2])


def _gathered(r, W, H, split, render):
    """render(r, part index) every part of `split` on context r, export it and scatter the rows: the [H, W, 16] records on cuda:0"""
    torch = _torch()
    full = torch.zeros((H, W, 16), dtype=torch.float32, device="cuda:0")
    for k, (how, rows) in enumerate(_split_parts(split, H)):
        _set_part(r, W, H, how)
        assert r.rows == len(rows)
        render(r, k)
        full[torch.as_tensor(rows, dtype=torch.long, device="cuda:0")] = _export(r)
    torch.cuda.synchronize()
    return full


def _adaptive16(prt):
    seeds = prt.seed_pairs(16 * 64 + 64)

    def render(r, k):
        r.reset()
        r.render_adaptive(seeds, 16, 16, 0.0)
        r.render_guides(4)
    return render


@pytest.fixture(scope="module")
def whole(prt):
    """the whole-frame context's picture: what every split must reproduce.  Computed once, never changed"""
    scene, cfg, cam, r = _setup(prt, "cornell_mixed.json", W1, H1, pinhole=False)
    _adaptive16(prt)(r, 0)
    doc = {"cfg": cfg, "fb": r.read_framebuffer(), "guides": r.read_guides(), "stats": r.read_adaptive_stats().reshape(H1, W1, 2),
           "n": r.read_state()["samples"].reshape(H1, W1), "records": _export(r).cpu().numpy(),
           "out": {(s, p): r.denoise(var_source=s, passes=p) for s in SOURCES for p in PASSES},
           "out8": r.denoise(tonemap=True)}
    import importlib
    par = importlib.import_module("photorealistic-rendering-using-opencl_amd.parallel")
    doc["rank0"] = par.denoise_on_rank0(r, H1, W1, 1, None, passes=5, var_source="stats").cpu().numpy()      # one rank: the same path, no collective
    r.close()
    for v in doc.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return doc


def _check_all(prt, rec_ctx, records, whole):
    torch = _torch()
    for (s, p), want in whole["out"].items():
        host = rec_ctx.denoise_records(records, W1, H1, var_source=s, passes=p)
        assert (_bits(host) == _bits(want)).all(), (s, p, "host")
        dev = torch.zeros((H1, W1, 4), dtype=torch.float32, device="cuda:0")
        torch.cuda.synchronize()
        assert rec_ctx.denoise_records(records, W1, H1, var_source=s, passes=p, out=dev) is dev
        assert (_bits(dev.cpu().numpy()) == _bits(want)).all(), (s, p, "device")
    assert (rec_ctx.denoise_records(records, W1, H1, tonemap=True) == whole["out8"]).all()


@pytest.mark.gpu
def test_whole_frame_records_are_the_planes_and_give_the_bits(prt, whole):
    rec = whole["records"]
    assert rec.shape == (H1, W1, 16)
    assert (_bits(rec[..., 0:4]) == _bits(whole["fb"])).all()
    assert (_bits(rec[..., 4:12]) == _bits(whole["guides"])).all()
    v = stats_variance(whole["stats"][..., 0], whole["stats"][..., 1], whole["n"])
    assert (np.abs(rec[..., 12] - v) <= 1e-6 * np.abs(v)).all()
    assert (whole["n"] >= 2).all() and (v > 0).any()
    assert (rec[..., 13] == 1.0).all() and (_bits(rec[..., 14:16]) == 0).all()
    assert (_bits(whole["rank0"]) == _bits(whole["out"][("stats", 5)])).all()
    rc = prt.Renderer(whole["cfg"], device=0)                       # no scene, no camera, no frame
    records = _to_device(rec)
    _check_all(prt, rc, records, whole)
    # all three outputs of one call, and NULL params = the defaults
    torch = _torch()
    dev = torch.zeros((H1, W1, 4), dtype=torch.float32, device="cuda:0")
    torch.cuda.synchronize()
    host, host8 = np.zeros((H1, W1, 4), dtype=np.float32), np.zeros((H1, W1, 4), dtype=np.uint8)
    assert rc.lib.prt_denoise_records(rc.ctx, None, W1, H1, C.c_void_p(records.data_ptr()), C.c_void_p(dev.data_ptr()),
                                      host.ctypes.data_as(C.c_void_p), host8.ctypes.data_as(C.c_void_p)) == 0
    want = whole["out"][("stats", 5)]                               # auto = stats: every record has them
    assert (_bits(host) == _bits(want)).all() and (_bits(dev.cpu().numpy()) == _bits(want)).all() and (host8 == whole["out8"]).all()
    assert rc.lib.prt_denoise_records(rc.ctx, None, W1, H1, C.c_void_p(records.data_ptr()), None, None, None) == 0
    rc.close()


@pytest.mark.gpu
@pytest.mark.parametrize("split", SPLITS, ids=lambda s: "%s-%s" % (s[0], "x".join(str(v) for v in (s[1:] if s[0] == "blocks" else s[1]))))
def test_split_equals_whole_bit_for_bit(prt, whole, split):
    scene, cfg, cam, r = _setup(prt, "cornell_mixed.json", W1, H1, pinhole=False)
    records = _gathered(r, W1, H1, split, _adaptive16(prt))
    r.close()
    assert (_bits(records.cpu().numpy()) == _bits(whole["records"])).all()
    rc = prt.Renderer(cfg, device=0)
    _check_all(prt, rc, records, whole)
    rc.close()


@pytest.mark.gpu
def test_mixed_stats_fall_back_to_spatial(prt, whole):
    scene, cfg, cam, r = _setup(prt, "cornell_mixed.json", W1, H1, pinhole=False)
    seeds = prt.seed_pairs(16 * 64 + 64)

    def render(r, k):
        r.reset()
        if k == 0:
            r.render_spp(16, seeds)
        else:
            r.render_adaptive(seeds, 16, 16, 0.0)
        r.render_guides(4)
    records = _gathered(r, W1, H1, ("blocks", 8, 2), render)
    r.close()
    rec = records.cpu().numpy()
    rows0 = [y for y in range(H1) if (y // 8) % 2 == 0]
    rows1 = [y for y in range(H1) if (y // 8) % 2 == 1]
    assert (rec[rows0][..., 13] == 0.0).all() and (_bits(rec[rows0][..., 12]) == 0).all() and (rec[rows1][..., 13] == 1.0).all()
    assert (_bits(rec[..., 0:12]) == _bits(whole["records"][..., 0:12])).all()       # "16 spp" is the same picture either way
    rc = prt.Renderer(cfg, device=0)
    with pytest.raises(prt.PrtError) as e:
        rc.denoise_records(records, W1, H1, var_source="stats")
    assert e.value.code == prt.PRT_ERR_NOT_READY
    for p in PASSES:
        assert (_bits(rc.denoise_records(records, W1, H1, var_source="auto", passes=p)) == _bits(whole["out"][("spatial", p)])).all(), p
    rc.close()


@pytest.mark.gpu
@pytest.mark.parametrize("feedback,adaptive", [("atrous", False), ("integrated", True)])
def test_temporal_split_equals_whole(prt, feedback, adaptive):
    W, H, F = 68, 44, 4
    scene, cfg, cam0, rw = _setup(prt, "cornell_mixed.json", W, H, pinhole=False)
    rp = _setup(prt, "cornell_mixed.json", W, H, pinhole=False)[3]
    rc, fresh = prt.Renderer(cfg, device=0), prt.Renderer(cfg, device=0)
    n = 2 * 64 + 64                              # frames of seeds per displayed frame (test_denoise's spp * 64 + 64)

    def frame(k):
        """frame k of the orbit: (camera, the whole-frame context rendered, the records of the two 8-row block parts)"""
        cam = prt.orbit_camera(W, H, d_yaw=0.02 * k) if k else prt.default_camera(W, H)
        seeds = prt.seed_pairs(n, first_frame=1 + k * n)

        def render(r, part):
            r.set_camera(cam)
            r.reset()
            if adaptive:
                r.render_adaptive(seeds, 2, 2, 0.0)
            else:
                r.render_spp(2, seeds)
            r.render_guides(4)
        render(rw, 0)
        return cam, _gathered(rp, W, H, ("blocks", 8, 2), render)

    kw = dict(feedback=feedback)
    for k in range(F):
        cam, records = frame(k)
        want = rw.denoise_temporal(**kw)
        got = rc.denoise_records_temporal(records, W, H, cam, **kw)
        assert (_bits(got) == _bits(want)).all(), k
        assert (_bits(rc.read_records_history(W, H)) == _bits(rw.read_history())).all(), k
    # an emptied history: the next frame is a fresh context's
    cam, records = frame(F)
    first = fresh.denoise_records_temporal(records, W, H, cam, **kw)
    with_history = rc.denoise_records_temporal(records, W, H, cam, **kw)
    assert (_bits(with_history) != _bits(first)).any()
    rc.reset_records_history()
    assert (_bits(rc.denoise_records_temporal(records, W, H, cam, **kw)) == _bits(first)).all()
    # ... and so does a call with another size (the first H - 4 rows of the same records are a frame too)
    rc.denoise_records_temporal(records, W, H, cam, **kw)
    rc.denoise_records_temporal(records, W, H - 4, cam, **kw)
    assert (_bits(rc.denoise_records_temporal(records, W, H, cam, **kw)) == _bits(first)).all()
    # the device output of the temporal call
    torch = _torch()
    dev = torch.zeros((H, W, 4), dtype=torch.float32, device="cuda:0")
    torch.cuda.synchronize()
    fresh.reset_records_history()
    fresh.denoise_records_temporal(records, W, H, cam, out=dev, **kw)
    assert (_bits(dev.cpu().numpy()) == _bits(first)).all()
    for r in (rw, rp, rc, fresh):
        r.close()


@pytest.mark.gpu
def test_synthetic_records_equal_the_formulas(prt):
    W, H = 40, 33
    rec, (ny, nx) = _synthetic(W, H)
    records = _to_device(rec)
    rc = prt.Renderer(prt.HostScene("cornell_coat.json").config(), device=0)
    fin = np.ones((H, W), dtype=bool)
    fin[ny, nx] = False
    variances = {"stats": rec[..., 12].astype(np.float64), "spatial": spatial_variance(rec[..., 0:3].astype(np.float64))}
    for source, v in variances.items():
        for passes in PASSES:
            got = rc.denoise_records(records, W, H, var_source=source, passes=passes)
            assert np.isfinite(got[fin]).all(), (source, passes)
            assert (_bits(got[ny, nx]) == _bits(rec[ny, nx, 0:4])).all(), (source, passes)           # the NaN pixel keeps its colour words
            assert (_bits(got[..., 3]) == _bits(rec[..., 3])).all(), (source, passes)               # alpha is the records'
            assert (_bits(rc.denoise_records(records, W, H, var_source=source, passes=passes)) == _bits(got)).all()
            ref = denoise_ref(rec[..., 0:4], rec[..., 4:12], v, passes=passes)
            err = np.abs(got[fin] - ref[fin]).max()
            bound = 1e-4 * np.abs(ref[fin]).max()
            print("synthetic records: %s, %d passes: max error %.3e (bound %.3e)" % (source, passes, err, bound))
            assert err <= bound, (source, passes, err)
    assert (_bits(rc.denoise_records(records, W, H)) == _bits(rc.denoise_records(records, W, H, var_source="stats"))).all()       # auto
    rc.close()


@pytest.mark.gpu
def test_refusals_and_read_only(prt):
    W, H = 32, 24
    torch = _torch()
    scene = prt.HostScene("cornell_coat.json")
    cfg = scene.config()
    cam = prt.default_camera(W, H)
    seeds = prt.seed_pairs(16 * 16 + 64)
    big, _ = _synthetic(W1, H1, seed=9)
    big_dev = _to_device(big)
    buf = torch.zeros((H, W, 16), dtype=torch.float32, device="cuda:0")
    torch.cuda.synchronize()

    def code(fn, *a, **k):
        with pytest.raises(prt.PrtError) as e:
            fn(*a, **k)
        return e.value.code

    # prt_export_denoise_inputs
    r = prt.Renderer(cfg, device=0)
    assert code(r.export_denoise_inputs, buf.data_ptr()) == prt.PRT_ERR_INVALID_ARGUMENT          # a context without a size
    r.upload_scene(scene); r.set_camera(cam)
    r.set_row_blocks(W, H, 4, 2, 1)
    assert r.rows == 12
    assert code(r.export_denoise_inputs, 0) == prt.PRT_ERR_INVALID_ARGUMENT                       # a null pointer
    assert code(r.export_denoise_inputs, buf) == prt.PRT_ERR_NOT_READY                            # no guides
    r.render_guides(2)
    assert code(r.export_denoise_inputs, buf) == prt.PRT_ERR_NOT_READY                            # nothing rendered since the reset
    r.render_adaptive(seeds, 2, 16, 0.1)
    r.export_denoise_inputs(buf)
    assert (buf[12:] == 0).all().item() and (buf[:12, :, 13] == 1.0).all().item()                  # this part's 12 rows and no more
    # prt_denoise_records on that row-block context: its own frame is left alone
    state, fb, st, g = r.read_state(), r.read_framebuffer(), r.read_adaptive_stats(), r.read_guides()
    out = r.denoise_records(big_dev, W1, H1)
    r.denoise_records_temporal(big_dev, W1, H1, prt.default_camera(W1, H1))
    r.denoise_records(big_dev, W1, H1, var_source="spatial", tonemap=True)
    assert out.shape == (H1, W1, 4)
    assert (r.read_state().view(np.uint8) == state.view(np.uint8)).all()
    assert (_bits(r.read_framebuffer()) == _bits(fb)).all() and (_bits(r.read_adaptive_stats()) == _bits(st)).all()
    assert (_bits(r.read_guides()) == _bits(g)).all()
    assert code(r.read_history) == prt.PRT_ERR_NOT_READY                                            # its own history: still empty
    assert code(r.denoise) == prt.PRT_ERR_UNSUPPORTED                                               # prt_denoise keeps its refusal
    again = torch.zeros_like(buf)
    torch.cuda.synchronize()
    r.export_denoise_inputs(again)
    assert (_bits(again.cpu().numpy()) == _bits(buf.cpu().numpy())).all()
    # a whole-frame context with a history of its own: the record calls and the record history are another matter
    r.resize(W, H)
    r.render_spp(4, seeds); r.render_guides(2)
    r.denoise_temporal()
    hist = r.read_history()
    r.denoise_records_temporal(big_dev, W1, H1, prt.default_camera(W1, H1))
    r.denoise_records(big_dev, W1, H1)
    r.reset_records_history()
    assert (_bits(r.read_history()) == _bits(hist)).all()
    # prt_denoise_records' arguments
    assert code(r.denoise_records, big_dev.data_ptr(), 0, H1) == prt.PRT_ERR_INVALID_ARGUMENT
    assert code(r.denoise_records, big_dev.data_ptr(), W1, -1) == prt.PRT_ERR_INVALID_ARGUMENT
    assert code(r.denoise_records, 0, W1, H1) == prt.PRT_ERR_INVALID_ARGUMENT
    nan = float("nan")
    for kw in (dict(passes=0), dict(passes=9), dict(sigma_l=-1.0), dict(sigma_n=nan), dict(sigma_z=0.0), dict(sigma_a=-0.1)):
        assert code(r.denoise_records, big_dev, W1, H1, **kw) == prt.PRT_ERR_INVALID_ARGUMENT, kw
        assert code(r.denoise_records_temporal, big_dev, W1, H1, cam, **kw) == prt.PRT_ERR_INVALID_ARGUMENT, kw
    for kw in (dict(alpha_color=1.1), dict(alpha_moments=nan), dict(tau_z=0.0), dict(cos_n=1.01), dict(history_cap=0)):
        assert code(r.denoise_records_temporal, big_dev, W1, H1, cam, **kw) == prt.PRT_ERR_INVALID_ARGUMENT, kw
    assert code(r.denoise_records_temporal, big_dev, W1, H1, None) == prt.PRT_ERR_INVALID_ARGUMENT    # a null camera
    assert code(r.denoise_records_temporal, 0, W1, H1, cam) == prt.PRT_ERR_INVALID_ARGUMENT
    p = prt.DenoiseParams(5, 3, 3.0, 128.0, 1.0, 0.1)                                               # unknown var_source
    assert r.lib.prt_denoise_records(r.ctx, C.byref(p), W1, H1, C.c_void_p(big_dev.data_ptr()), None, None, None) == prt.PRT_ERR_INVALID_ARGUMENT
    with pytest.raises(ValueError):
        r.denoise_records(big_dev, W1, H1 + 1)                                                       # a tensor smaller than the frame
    with pytest.raises(ValueError):
        r.export_denoise_inputs(buf[:5])
    r.close()
    # a debug view is not a picture to filter
    vcfg = scene.config()
    vcfg.view_option = 1
    rv = prt.Renderer(vcfg, device=0)
    rv.upload_scene(scene); rv.set_camera(cam); rv.resize(W, H)
    rv.render_guides(1); rv.render_spp(16, seeds)
    assert code(rv.export_denoise_inputs, buf) == prt.PRT_ERR_UNSUPPORTED
    rv.close()
