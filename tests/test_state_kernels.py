"""The small kernels every result passes through (csrc/hip/pt_kernels.hip), on synthetic data at ragged frame sizes: no scene, no rendering.

  state_to_rtd / rtd_to_state   prt_read_state / prt_write_state: which parts of the 112-byte record are carried, bit for bit, and the framebuffer
                                prt_write_state derives (acc / (float)samples, zero where samples == 0)
  count_kernel                  prt_query_counts against integer sums, past the 2048 x 256-thread grid (a second, ragged trip of the stride loop)
  tonemap_kernel                prt_tonemap_rgba8 against a float32 mirror of the kernel's own order of operations, byte for byte, on whole frames,
                                tiles and row blocks (the vignette needs the GLOBAL row) and on the special inputs

The frames: 1x1, 63x1 / 65x1 (either side of a wave), 257x3 (either side of a 256-thread block, three rows), 331x199 (ragged, 258 blocks),
1031x509 (524 779 pixels: 491 past the count kernel's grid)."""
import ctypes as C
import os

import numpy as np
import pytest

from conftest import ROOT
from support import bytes_rows as _bytes

F = np.float32
U32 = np.uint32
FLT_MIN = F(1.1754944e-38)


def _ctx(prt):
    return prt.Renderer(prt.HostScene("cornell_diffuse.json").config(), device=0)


def _u32(a):
    return np.ascontiguousarray(a).view(U32)


def _block_rows(H, B, n_parts, part):
    """the global rows of a row-block part, in its framebuffer's order (prt_set_row_blocks: block b belongs to part b % n_parts)"""
    return np.array([y for y in range(H) if (y // B) % n_parts == part])


# ---- 1. state pack / unpack -----------------------------------------------------------------------------------------------------------------

U16_EDGES = [0, 1, 0x7fff, 0xffff]
TOTAL_EDGES = [0, 1, 0x7f800001, 0x80000000, 0xffffffff]          # (0x7f800001: a signalling NaN when held as a float, as the planes hold it)
SAMPLES_EDGES = [0, 1, 1 << 24, (1 << 24) + 1, 0xffffffff]
FLAG_EDGES = [0, 1, 2, 255]
# +-0, denormals, +-inf, NaNs (quiet, and negative with a payload), +-FLT_MAX, FLT_MIN, 1
FLOAT_EDGES = np.array([0x00000000, 0x80000000, 0x00000001, 0x807fffff, 0x7f800000, 0xff800000, 0x7fc00000, 0xffc00001,
                        0x7f7fffff, 0xff7fffff, 0x00800000, 0x3f800000], dtype=U32)
CARRIED_VEC3 = ("origin", "dir", "mask")
CARRIED_BITS = ("time", "dist", "total", "samples", "diff", "spec", "trans", "scatters")


def synthetic_state(prt, n, seed):
    """n records: every byte non-zero first (so origin[3], dir[3], mask[3] and the pads are), then every field drawn from arbitrary bit patterns
    (acc: finite values of any magnitude and sign), a quarter of each field's entries replaced by its edge values, and edge combinations
    planted at fixed indices, the first and the last pixel among them"""
    rng = np.random.default_rng(seed)
    st = rng.integers(1, 256, (n, 112), dtype=np.uint8).view(np.dtype(prt.PATH_STATE_DTYPE)).reshape(n)

    def mixed(values, edges, shape):
        e = np.asarray(edges, dtype=values.dtype)
        return np.where(rng.random(shape) < 0.25, e[rng.integers(0, len(e), shape)], values)

    for name in CARRIED_VEC3:
        st[name].view(U32)[:, :3] = mixed(rng.integers(0, 1 << 32, (n, 3), dtype=U32), FLOAT_EDGES, (n, 3))
    for name in ("time", "dist"):
        st[name].view(U32)[:] = mixed(rng.integers(0, 1 << 32, n, dtype=U32), FLOAT_EDGES, n)
    acc = (np.exp(rng.uniform(-60, 60, (n, 4))) * rng.choice([-1.0, 1.0], (n, 4))).astype(F)
    st["acc"].view(U32)[:] = mixed(acc.view(U32), FLOAT_EDGES, (n, 4))
    st["total"] = mixed(rng.integers(0, 1 << 32, n, dtype=U32), TOTAL_EDGES, n)
    small = rng.integers(1, 5000, n, dtype=U32)
    st["samples"] = mixed(np.where(rng.random(n) < 0.5, small, rng.integers(0, 1 << 32, n, dtype=U32)), SAMPLES_EDGES, n)
    for name in ("diff", "spec", "trans", "scatters"):
        st[name] = mixed(rng.integers(0, 1 << 16, n, dtype=np.uint16), U16_EDGES, n)
    for name in ("was_specular", "reset"):
        st[name] = np.asarray(FLAG_EDGES, dtype=np.uint8)[rng.integers(0, 4, n)]
    planted = sorted({i for i in (0, 1, 2, 62, 63, 64, 65, 255, 256, 257, n // 2, n - 2, n - 1) if 0 <= i < n})
    for j, p in enumerate(planted):
        st["diff"][p] = U16_EDGES[(j + 3) % 4]
        st["spec"][p] = U16_EDGES[(j + j // 4) % 4]
        st["trans"][p] = U16_EDGES[(j + 2) % 4]
        st["scatters"][p] = U16_EDGES[(j + 1 + j // 2) % 4]
        st["total"][p] = TOTAL_EDGES[(j + 2) % 5]
        st["samples"][p] = SAMPLES_EDGES[(j + 3) % 5]
        st["was_specular"][p] = FLAG_EDGES[(j + 2) % 4]
        st["reset"][p] = FLAG_EDGES[(j + 3) % 4]
        st["acc"].view(U32)[p] = FLOAT_EDGES[(4 * j + 8 + np.arange(4)) % len(FLOAT_EDGES)]      # (j = 0: +-FLT_MAX, FLT_MIN, 1 over 2^24 + 1 paths)
        st["mask"].view(U32)[p, :3] = FLOAT_EDGES[(3 * j + np.arange(3)) % len(FLOAT_EDGES)]
    if n > 3:                                     # quotients that are denormal: tiny sums over the largest count
        st["acc"][3] = np.array([1e-30, -1e-30, 1e-32, 5e-35], dtype=F)          # / 2^32: 2.3e-40 ... 1.2e-44 (8 ulp of the denormals)
        st["samples"][3] = 0xffffffff
    return st


def carried_record(prt, st):
    """what prt_read_state returns after prt_write_state(st), by include/prt.h: the carried fields' bits, the flags as 0 / 1, zeros elsewhere"""
    want = np.zeros(st.size, dtype=np.dtype(prt.PATH_STATE_DTYPE))
    for name in CARRIED_VEC3:
        want[name].view(U32)[:, :3] = st[name].view(U32)[:, :3]
    want["acc"].view(U32)[:] = st["acc"].view(U32)
    for name in ("time", "dist"):
        want[name].view(U32)[:] = st[name].view(U32)
    for name in ("total", "samples", "diff", "spec", "trans", "scatters"):
        want[name] = st[name]
    for name in ("was_specular", "reset"):
        want[name] = (st[name] != 0).astype(np.uint8)
    return want


def derived_framebuffer(st):
    """acc / (float)samples in numpy float32, +0.0 where samples == 0"""
    with np.errstate(all="ignore"):
        q = st["acc"] / st["samples"].astype(F)[:, None]
    q[st["samples"] == 0] = F(0.0)
    return q


def _roundtrip(prt, r, seed, what):
    import torch
    n = r.rows * r.width
    st = synthetic_state(prt, n, seed)
    sent = st.copy()
    r.write_state(st)
    assert (_bytes(st) == _bytes(sent)).all(), what + ": prt_write_state changed its input"
    got = r.read_state()
    want = carried_record(prt, st)
    for name in CARRIED_VEC3 + ("acc",) + CARRIED_BITS + ("was_specular", "reset"):
        a, b = np.ascontiguousarray(got[name]), np.ascontiguousarray(want[name])
        bad = np.flatnonzero((a.view(np.uint8).reshape(n, -1) != b.view(np.uint8).reshape(n, -1)).any(1))
        assert bad.size == 0, "%s: %s differs at %d pixels, first %s: got %r, want %r (sent %r)" % (
            what, name, bad.size, bad[:8], got[name][bad[0]], want[name][bad[0]], st[name][bad[0]])
    bad = np.argwhere(_bytes(got) != _bytes(want))                  # the rest: origin[3], dir[3], mask[3] and the pads are zero
    assert bad.size == 0, "%s: %d bytes that are not carried are not zero, first (pixel, byte) %s" % (what, len(bad), bad[:8].tolist())
    # the framebuffer prt_write_state derives
    q = derived_framebuffer(st)
    fb = r.read_framebuffer().reshape(-1, 4)
    nan = np.isnan(q)
    assert np.isnan(fb[nan]).all(), what + ": a NaN quotient is not NaN in the framebuffer"
    bad = np.flatnonzero(((_u32(fb) != _u32(q)) & ~nan).any(1))
    assert bad.size == 0, "%s: framebuffer differs from acc / (float)samples at %d pixels, first %s: got %r, want %r (acc %r, samples %d)" % (
        what, bad.size, bad[:8], fb[bad[0]], q[bad[0]], st["acc"][bad[0]], st["samples"][bad[0]])
    assert n < 4 or ((q[3] != 0) & (np.abs(q[3]) < FLT_MIN)).all()          # (the planted denormal quotients are denormal)
    none = st["samples"] == 0
    assert (_u32(fb)[none] == 0).all(), what + ": samples == 0 is not +0.0 in all four channels"
    # reading changes nothing, and the device-to-device copy is the same picture
    assert (_bytes(r.read_state()) == _bytes(got)).all(), what + ": a second prt_read_state differs"
    t = torch.empty((r.rows, r.width, 4), dtype=torch.float32, device="cuda:0")
    torch.cuda.synchronize()
    r.copy_framebuffer_to_device(t.data_ptr())
    assert (_u32(t.cpu().numpy()).reshape(-1, 4) == _u32(fb)).all(), what + ": prt_copy_framebuffer_to_device differs from prt_read_framebuffer"
    return st, q


def test_synthetic_state_has_every_edge(prt):
    """the generator itself (no GPU): the edge values the round trip is meant to see are in the records"""
    for n in (1, 63, 65):
        st = synthetic_state(prt, n, 100 + n)
        assert (_bytes(st)[:, 40:48] != 0).all() and (_bytes(st)[:, 104:112] != 0).all() and (_bytes(st)[:, 93:96] != 0).all()
        assert (_u32(st["origin"])[:, 3] != 0).all() and (_u32(st["dir"])[:, 3] != 0).all() and (_u32(st["mask"])[:, 3] != 0).all()
        assert st["diff"][0] == 0xffff and st["total"][0] == 0x7f800001 and st["samples"][0] == (1 << 24) + 1 and st["reset"][0] == 255
    st = synthetic_state(prt, 331 * 199, 5)
    for name in ("diff", "spec", "trans", "scatters"):
        assert set(U16_EDGES) <= set(st[name].tolist())
    assert set(TOTAL_EDGES) <= set(st["total"].tolist()) and set(SAMPLES_EDGES) <= set(st["samples"].tolist())
    assert set(FLAG_EDGES) == set(st["was_specular"].tolist()) == set(st["reset"].tolist())
    assert len({(int(a), int(b)) for a, b in zip(st["diff"][:4096], st["spec"][:4096])} & {(x, y) for x in U16_EDGES for y in U16_EDGES}) == 16
    for name in ("origin", "dir", "mask", "acc"):
        assert set(FLOAT_EDGES.tolist()) <= set(_u32(st[name]).reshape(-1).tolist()), name
    assert ((st["samples"] == 0) & (_u32(st["acc"]) != 0).all(1)).any() and ((st["samples"] == 0) & ~np.isfinite(st["acc"]).all(1)).any()
    q = derived_framebuffer(st)
    assert ((q != 0) & (np.abs(q) < FLT_MIN)).any() and np.isnan(q).any() and np.isinf(q).any() and (_u32(q) == 0x80000000).any()


@pytest.mark.gpu
@pytest.mark.parametrize("W,H", [(1, 1), (63, 1), (65, 1), (257, 3), (331, 199)])
def test_state_roundtrip_on_synthetic_records(prt, W, H):
    r = _ctx(prt)
    r.resize(W, H)
    _roundtrip(prt, r, 1000 * W + H, "%d x %d" % (W, H))
    r.close()


@pytest.mark.gpu
def test_state_roundtrip_on_a_tile_and_on_row_blocks(prt):
    W, H = 331, 199
    r = _ctx(prt)
    r.set_tile(W, H, 120, 40)
    assert r.rows == 40
    _roundtrip(prt, r, 21, "tile rows 120..159 of %d x %d" % (W, H))
    for part in range(3):
        r.set_row_blocks(W, H, 8, 3, part)
        assert r.rows == len(_block_rows(H, 8, 3, part))
        _roundtrip(prt, r, 30 + part, "row blocks of 8, part %d of 3 of %d x %d" % (part, W, H))
    r.close()


# ---- 2. counts ------------------------------------------------------------------------------------------------------------------------------

def counts_state(prt, n, seed):
    """samples over the whole uint32 range (the sum passes 2^32), acc.w an integer-valued float below 2^24 (count_kernel's precondition),
    reset mixed; the counts around each spp of the test planted with reset set and clear"""
    rng = np.random.default_rng(seed)
    st = np.zeros(n, dtype=np.dtype(prt.PATH_STATE_DTYPE))
    st["samples"] = rng.integers(0, 1 << 32, n, dtype=U32)
    st["acc"][:, 3] = rng.integers(0, 1 << 24, n).astype(F)
    st["acc"][:, :3] = rng.random((n, 3)).astype(F)
    st["reset"] = np.where(rng.random(n) < 0.6, np.asarray([1, 2, 255], dtype=np.uint8)[rng.integers(0, 3, n)], 0)
    edges = [0, 1, 2, 6, 7, 8, 0xfffffffe, 0xffffffff]
    at = np.linspace(0, n - 1, 2 * len(edges)).astype(np.int64)            # the first and the last pixel among them
    st["samples"][at] = np.repeat(np.asarray(edges, dtype=U32), 2)
    st["reset"][at] = np.tile(np.asarray([1, 0], dtype=np.uint8), len(edges))
    st["acc"][at[::3], 3] = F((1 << 24) - 1)
    return st


@pytest.mark.gpu
@pytest.mark.parametrize("W,H", [(65, 1), (331, 199), (1031, 509)])
def test_counts_equal_integer_sums(prt, W, H):
    n = W * H
    st = counts_state(prt, n, 7 * W + H)
    samples = int(st["samples"].astype(np.uint64).sum())
    segments = int(st["acc"][:, 3].astype(np.uint64).sum())
    assert samples >= 1 << 32 and (st["acc"][:, 3] == np.floor(st["acc"][:, 3])).all() and st["acc"][:, 3].max() < 1 << 24
    median = int(np.sort(st["samples"])[n // 2])                 # a count that occurs: the rule's >= is on its edge
    r = _ctx(prt)
    r.resize(W, H)
    r.write_state(st)                                            # uploaded once, queried for every spp
    for spp in (0, 1, 7, median, 0xffffffff):
        frozen = int(((st["reset"] != 0) & (st["samples"] >= spp)).sum()) if spp > 0 else 0
        if spp == median:
            assert 10 * frozen >= n and 10 * (n - frozen) >= n, (frozen, n)
        elif spp:
            assert 0 < frozen < n
        c = r.counts(spp)
        assert (c.samples, c.segments, c.finished_pixels) == (samples, segments, frozen), (W, H, spp)
    r.close()


# ---- 3. tonemap -----------------------------------------------------------------------------------------------------------------------------

_probe_lib = []


def _prt_pow(x, y):
    """prt_pow of include/prt_detmath.h, evaluated on the host by the probe tests/test_detmath.py binds (fn 7); the device's is held to it there"""
    if not _probe_lib:
        lib = C.CDLL(os.path.join(ROOT, "oracle", "libdetmath_probe.so"))
        lib.detmath_probe.argtypes = [C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int]
        _probe_lib.append(lib)
    x = np.ascontiguousarray(x, dtype=F)
    y = np.ascontiguousarray(np.broadcast_to(F(y), x.shape), dtype=F)
    out = np.zeros_like(x)
    _probe_lib[0].detmath_probe(7, x.ctypes.data, y.ctypes.data, out.ctypes.data, x.size)
    return out


def _fmax32(a, b):           # prt_fmax: a NaN operand is ignored
    a, b = np.broadcast_arrays(np.asarray(a, dtype=F), np.asarray(b, dtype=F))
    return np.where(np.isnan(b), a, np.where(np.isnan(a), b, np.where(a < b, b, a)))


def _fmin32(a, b):
    a, b = np.broadcast_arrays(np.asarray(a, dtype=F), np.asarray(b, dtype=F))
    return np.where(np.isnan(b), a, np.where(np.isnan(a), b, np.where(b < a, b, a)))


def _curve32(x):             # filmic_reinhard_curve: (T2 * T2 + 1) * x * x, left to right
    q = F(57.25) * x * x
    return q / (q + x + F(56.25))


def _smoothstep32(e0, e1, x):
    t = _fmin32(_fmax32((x - e0) / (e1 - e0), F(0.0)), F(1.0))
    return t * t * (F(3.0) - F(2.0) * t)


def tonemap_mirror32(fb, W, full_height, global_rows):
    """tonemap_kernel operation by operation in numpy float32 (the library is built without contraction, so the order fixes the bits).
    fb: [rows, W, >= 3] float32, row k being row global_rows[k] of a frame full_height high.  Returns uint8 [rows, W, 3]"""
    fb = np.asarray(fb, dtype=F).reshape(len(global_rows), W, -1)
    with np.errstate(all="ignore"):
        px = F(1.0) - F(2.0) * (np.arange(W).astype(F) + F(0.5)) / F(W)
        py = F(1.0) - F(2.0) * (np.asarray(global_rows).astype(F) + F(0.5)) / F(full_height)
        vig = F(1.25) / (F(1.1) + F(1.1) * ((px * px)[None, :] + (py * py)[:, None]))
        vig = vig * vig
        vig = F(0.75) + _smoothstep32(F(0.1), F(1.1), vig) * F(0.25)
        v = fb[..., :3] * vig[..., None]
        v = _curve32(F(1.0) * v) / _curve32(F(1.2))
        v = _smoothstep32(F(-0.025), F(1.0), v)
        v = _prt_pow(v, F(1.0) / F(2.2))
        v = _fmin32(_fmax32(v, F(0.0)), F(1.0))
        out = np.rint(v * F(255.0))
    assert out.dtype == F and vig.dtype == F
    return out.astype(np.uint8)


def tonemap_formula64(fb, W, H):
    """shaders/tonemapper.glsl in float64 on a whole frame (the formula of test_tonemap_matches_the_reference_shader_and_cli_writes_png)"""
    fb = np.asarray(fb, dtype=np.float64).reshape(H, W, -1)
    yy, xx = np.mgrid[0:H, 0:W]
    px, py = 1 - 2 * (xx + 0.5) / W, 1 - 2 * (yy + 0.5) / H
    vig = (1.25 / (1.1 + 1.1 * (px * px + py * py))) ** 2
    sm = lambda e0, e1, x: (lambda t: t * t * (3 - 2 * t))(np.clip((x - e0) / (e1 - e0), 0, 1))
    vig = 0.75 + 0.25 * sm(0.1, 1.1, vig)
    curve = lambda x: (57.25 * x * x) / (57.25 * x * x + x + 56.25)
    col = curve(fb[..., :3] * vig[..., None]) / curve(1.2)
    return np.rint(np.clip(sm(-0.025, 1.0, col) ** (1 / 2.2), 0, 1) * 255)


def tonemap_inputs(W, H, seed=3):
    """finite log-uniform triples in [1e-4, 50], about 5 % negated"""
    rng = np.random.default_rng(seed)
    x = np.exp(rng.uniform(np.log(1e-4), np.log(50.0), (H, W, 3)))
    return np.where(rng.random((H, W, 3)) < 0.05, -x, x).astype(F)


# nan, +-inf and every value whose 57.25 x^2 overflows float32 map to 0 (black, where the float64 formula says 255 for the large ones)
SPECIALS_TO_ZERO = np.array([np.nan, np.inf, -np.inf, 3e18, 1e19, 3.4e38, -1e19], dtype=F)
SPECIALS = np.concatenate([np.array([0.0, -0.0, 1e-45], dtype=F), SPECIALS_TO_ZERO, np.array([1.0, 1.2], dtype=F)])

FULL_W, FULL_H = 331, 199
_full = {}


def _full_frame():
    """the 331 x 199 picture and its mirror, computed once"""
    if not _full:
        _full["fb"] = tonemap_inputs(FULL_W, FULL_H)
        _full["want"] = tonemap_mirror32(_full["fb"], FULL_W, FULL_H, np.arange(FULL_H))
        _full["fb"].setflags(write=False)
        _full["want"].setflags(write=False)
    return _full["fb"], _full["want"]


def test_float32_mirror_agrees_with_the_float64_formula(oracle):
    fb, got = _full_frame()
    assert fb.size >= 100000 and np.isfinite(fb).all() and 0.03 < (fb < 0).mean() < 0.07
    want = tonemap_formula64(fb, FULL_W, FULL_H)
    assert np.abs(got.astype(np.float64) - want).max() <= 1
    assert len(np.unique(got)) >= 200, len(np.unique(got))             # the inputs are not saturated
    # a part of the frame is those rows of the whole
    rows = _block_rows(FULL_H, 8, 3, 0)
    assert len(rows) == 71 and rows[-1] == 198
    assert (tonemap_mirror32(fb[rows], FULL_W, FULL_H, rows) == got[rows]).all()
    # ... and taking the tile at row 120 for one at row 0 is far from subtle
    assert (tonemap_mirror32(fb[120:160], FULL_W, FULL_H, np.arange(40)) != got[120:160]).mean() > 0.1


def test_float32_mirror_on_the_special_inputs(oracle):
    """at the centre of a 1 x 1 frame: the float32 transform takes NaN, +-inf and the overflowing values to 0 (include/prt.h says so), a zero of
    either sign and a denormal to the byte of 0.0, and 1.0 / 1.2 to what the float64 formula gives"""
    one = lambda x: tonemap_mirror32(np.full((1, 1, 3), x, dtype=F), 1, 1, [0])[0, 0]
    assert all((one(x) == 0).all() for x in SPECIALS_TO_ZERO)
    zero = one(F(0.0))
    assert (zero > 0).all() and (one(F(-0.0)) == zero).all() and (one(F(1e-45)) == zero).all()
    for x in (0.0, 1.0, 1.2):
        assert np.abs(one(F(x)).astype(np.float64) - tonemap_formula64(np.full((1, 1, 3), x), 1, 1)[0, 0]).max() <= 1
    assert (tonemap_formula64(np.full((1, 1, 3), 1e19), 1, 1) == 255).all()      # where float64 and the shader's float32 part ways


def _inject(prt, r, fb):
    """the framebuffer through prt_write_state: samples = 1 and acc = fb, so the derived acc / 1.0f is fb exactly"""
    n = r.rows * r.width
    fb = np.asarray(fb, dtype=F).reshape(n, 3)
    st = np.zeros(n, dtype=np.dtype(prt.PATH_STATE_DTYPE))
    st["acc"][:, :3] = fb
    st["acc"][:, 3] = 1.0
    st["samples"] = 1
    st["reset"] = 1
    r.write_state(st)
    got = r.read_framebuffer().reshape(n, 4)[:, :3]
    assert ((_u32(got) == _u32(fb)) | (np.isnan(got) & np.isnan(fb))).all()


def _assert_tonemap(prt, r, fb, full_height, global_rows, what):
    _inject(prt, r, fb)
    got = r.tonemap_rgba8()
    want = tonemap_mirror32(fb, r.width, full_height, global_rows)
    assert got.shape == (len(global_rows), r.width, 4)
    bad = np.argwhere(got[..., :3] != want)
    assert bad.size == 0, "%s: %d of %d bytes differ from the float32 mirror, first (row, x, channel) %s: got %s, want %s" % (
        what, len(bad), want.size, bad[:4].tolist(), got[..., :3][tuple(bad[:4].T)], want[tuple(bad[:4].T)])
    assert (got[..., 3] == 255).all(), what + ": alpha"
    return want


TONEMAP_FRAMES = [("whole", None), ("tile", (0, 1)), ("tile", (120, 40)), ("tile", (198, 1)), ("blocks", 0), ("blocks", 1), ("blocks", 2)]


@pytest.mark.gpu
@pytest.mark.parametrize("kind,arg", TONEMAP_FRAMES, ids=["whole", "tile0+1", "tile120+40", "tile198+1", "blocks0", "blocks1", "blocks2"])
def test_tonemap_equals_the_float32_mirror_whole_and_split(prt, oracle, kind, arg):
    fb, whole = _full_frame()
    W, H = FULL_W, FULL_H
    r = _ctx(prt)
    if kind == "whole":
        r.resize(W, H)
        rows = np.arange(H)
    elif kind == "tile":
        r.set_tile(W, H, arg[0], arg[1])
        rows = np.arange(arg[0], arg[0] + arg[1])
    else:
        r.set_row_blocks(W, H, 8, 3, arg)
        rows = _block_rows(H, 8, 3, arg)
    assert r.rows == len(rows)
    want = _assert_tonemap(prt, r, fb[rows], H, rows, "%d x %d %s %s" % (W, H, kind, arg))
    assert (want == whole[rows]).all()                  # the part's picture is those rows of the whole frame's
    r.close()


@pytest.mark.gpu
def test_tonemap_equals_the_float32_mirror_on_small_frames_and_special_inputs(prt, oracle):
    r = _ctx(prt)
    for W, H in ((1, 1), (257, 3)):
        r.resize(W, H)
        _assert_tonemap(prt, r, tonemap_inputs(W, H, seed=W), H, np.arange(H), "%d x %d" % (W, H))
    # one row of the special inputs, each in every channel
    n = len(SPECIALS)
    row = np.stack([np.roll(SPECIALS, -k) for k in (0, 1, 5)], axis=1).reshape(1, n, 3)
    r.resize(n, 1)
    _assert_tonemap(prt, r, row, 1, [0], "special inputs, one row")
    # ... and at the centre of a 1 x 1 frame, where test_float32_mirror_on_the_special_inputs says what the mirror gives
    r.resize(1, 1)
    for k in range(0, n, 3):
        want = _assert_tonemap(prt, r, SPECIALS[k:k + 3].reshape(1, 1, 3), 1, [0], "special inputs %s at the centre" % SPECIALS[k:k + 3])
        assert (want.reshape(3)[np.isin(_u32(SPECIALS[k:k + 3]), _u32(SPECIALS_TO_ZERO))] == 0).all()
    r.close()
