"""The exact fast paths of csrc/hip/pt_device.h (hw_recip, hw_sqrt, out_of_unit_range) choose between the fast expression and the IEEE one
per WAVE on the device: one lane outside the fast range sends the whole wave through the IEEE expression.  The exhaustive checks
(prt_selftest_math fn 17 - 19, tests/test_gpu_parity.py) walk the bit patterns in order, so almost all of their waves are entirely
inside or entirely outside the range; here every wave (64 consecutive inputs) MIXES in-range normals with zeros, subnormals, the
values at and beyond both range edges, infinities and NaNs, next to waves that are entirely in and entirely out of range.
Expectation: numpy's float32 1/x and sqrt(x) (correctly rounded IEEE), compared as words; NaN lanes by NaN-ness, like the selftests."""
import numpy as np
import pytest

WAVE, GROUPS = 64, 16
F = np.float32
INF, NAN = F(np.inf), F(np.nan)


def _around(v):
    v = F(v)
    return [np.nextafter(v, F(0)), v, np.nextafter(v, INF if v > 0 else -INF)]


def _signed(vals):
    vals = [F(v) for v in vals]
    return vals + [F(-v) for v in vals]


RECIP_OUT = _signed([0.0, 1e-45, 1e-40, 1.1754942e-38, 2.0 ** -126, np.nextafter(F(2.0 ** -125), F(0)), 2.0 ** 126, np.nextafter(F(2.0 ** 126), INF),
                     2.0 ** 127, 3.4028235e38, INF]) + [NAN]
RECIP_EDGE_IN = _signed([2.0 ** -125, np.nextafter(F(2.0 ** -125), INF), np.nextafter(F(2.0 ** 126), F(0))])
SQRT_OUT = _signed([0.0, 1e-45, 1e-40, 1.1754942e-38, np.nextafter(F(2.0 ** -100), F(0)), 2.0 ** 100, np.nextafter(F(2.0 ** 100), INF), 3.4028235e38, INF]) + \
    [NAN, F(-1.0), F(-2.0 ** -100), F(-2.0 ** 99), F(-3.5)]
SQRT_EDGE_IN = [F(2.0 ** -100), np.nextafter(F(2.0 ** -100), INF), np.nextafter(F(2.0 ** 100), F(0))]


def _mixed(rng, normals, out_vals, edge_in):
    """64 x 16 inputs: group 0 entirely in range (edges included), group 1 entirely out of range, groups 2 .. 15 in-range values with 1, 2, 3, ...
    out-of-range ones at random lanes (group 2: a single lane), every out-of-range value used"""
    x = normals(WAVE * GROUPS).astype(F).reshape(GROUPS, WAVE)
    x[0, :len(edge_in)] = edge_in
    x[1] = np.resize(np.array(out_vals, dtype=F), WAVE)
    pool = list(out_vals)
    for g in range(2, GROUPS):
        lanes = rng.choice(WAVE, size=min(WAVE - 8, (g - 1) * (g - 1)), replace=False)
        for k, lane in enumerate(lanes):
            x[g, lane] = pool[(g * 7 + k) % len(pool)]
        rest = [l for l in range(WAVE) if l not in set(lanes)]
        x[g, rest[0]] = edge_in[g % len(edge_in)]                  # an in-range edge value beside them
    return x.reshape(-1)


def _same(dev, want):
    return (dev.view(np.uint32) == want.view(np.uint32)) | (np.isnan(dev) & np.isnan(want))


@pytest.fixture(scope="module")
def renderer(prt):
    scene = prt.HostScene("cornell_diffuse.json")
    r = prt.Renderer(scene.config(), device=0)
    yield r
    r.close()


def _report(name, x, dev, want, ok):
    bad = np.flatnonzero(~ok)
    return "%s differs at %d of %d inputs, e.g. lane %d of group %d: x=%r device=%r expected=%r" % (
        name, bad.size, x.size, bad[0] % WAVE, bad[0] // WAVE, x[bad[0]], dev[bad[0]], want[bad[0]]) if bad.size else ""


@pytest.mark.gpu
def test_reciprocal_in_waves_that_mix_fast_and_slow_lanes(renderer):
    rng = np.random.default_rng(17)
    x = _mixed(rng, lambda n: (np.exp(rng.uniform(-80, 80, n)) * rng.choice([-1.0, 1.0], n)), RECIP_OUT, RECIP_EDGE_IN)
    e = (x.view(np.uint32) >> 23) & 0xff
    in_range = ((e >= 2) & (e <= 252)).reshape(GROUPS, WAVE)
    assert in_range[0].all() and not in_range[1].any() and all(0 < in_range[g].sum() < WAVE for g in range(2, GROUPS))
    with np.errstate(all="ignore"):
        want = (F(1.0) / x).astype(F)
    dev = renderer.selftest_math(22, x, np.zeros_like(x))
    ok = _same(dev, want)
    assert ok.all(), _report("hw_recip", x, dev, want, ok)


@pytest.mark.gpu
def test_square_root_in_waves_that_mix_fast_and_slow_lanes(renderer):
    rng = np.random.default_rng(19)
    x = _mixed(rng, lambda n: np.exp(rng.uniform(-65, 65, n)), SQRT_OUT, SQRT_EDGE_IN)
    e = (x.view(np.uint32) >> 23) & 0x1ff
    in_range = ((e >= 27) & (e < 227)).reshape(GROUPS, WAVE)
    assert in_range[0].all() and not in_range[1].any() and all(0 < in_range[g].sum() < WAVE for g in range(2, GROUPS))
    with np.errstate(all="ignore"):
        want = np.sqrt(x).astype(F)
    dev = renderer.selftest_math(23, x, np.zeros_like(x))
    ok = _same(dev, want)
    assert ok.all(), _report("hw_sqrt", x, dev, want, ok)


@pytest.mark.gpu
@pytest.mark.parametrize("divisors", [(1.0,), (0.7531,), (2.0 ** 41,), (1e-20,), (3.0, 2.0 ** 41), (0.7531, 1e-20, 16777215.0, 2.0 ** -41)],
                         ids=["valid_u", "valid_u_odd", "no_u_large", "no_u_small", "mixed_two", "mixed_four"])
def test_quad_range_test_in_waves_that_mix_fast_and_slow_lanes(renderer, divisors):
    """out_of_unit_range(x, c, u) against the reference's `l = x / c; l < 0 || l > 1` in float32: x near 0, near c, below 2^-100 and NaN, with a
    divisor that has a valid u (2^-40 <= c <= 2^40), one that has none, and both kinds within a wave"""
    rng = np.random.default_rng(18)
    n = WAVE * GROUPS
    c = np.array([divisors[k % len(divisors)] for k in rng.integers(0, len(divisors), n)], dtype=F)
    x = (rng.uniform(-0.25, 1.25, n) * c.astype(np.float64)).astype(F).reshape(GROUPS, WAVE)          # fast lanes: ordinary quotients
    cg = c.reshape(GROUPS, WAVE)
    tiny = _signed([0.0, 1e-45, 1e-40, 1.1754944e-38, 1e-35, 7.0e-31, np.nextafter(F(2.0 ** -100), F(0))]) + [NAN]       # below 2^-100, or NaN: the divide
    near = lambda cv: _around(cv) + [F(cv) * (F(1.0) + F(2.0 ** -23)), F(cv) * F(2.0), np.nextafter(F(2.0) * F(cv), F(0))] + _signed([2.0 ** -100, np.nextafter(F(2.0 ** -100), INF)]) + [INF, -INF]
    x[1] = np.resize(np.array(tiny, dtype=F), WAVE)                                                     # group 1: every lane takes the divide
    for g in range(2, GROUPS):
        lanes = rng.choice(WAVE, size=min(WAVE - 8, (g - 1) * (g - 1)), replace=False)
        for k, lane in enumerate(lanes):
            x[g, lane] = tiny[(g * 5 + k) % len(tiny)]
        rest = [l for l in range(WAVE) if l not in set(lanes)]
        for k, lane in enumerate(rest[:len(rest) // 2]):                                              # and the fast lanes sit on the edges of [0, c]
            vals = near(cg[g, lane])
            x[g, lane] = vals[(g + k) % len(vals)]
    vals0 = near(cg[0, 0])
    for lane in range(WAVE // 2):                                                                     # group 0 keeps clear of the divide where c has a valid u
        x[0, lane] = near(cg[0, lane])[lane % len(vals0)]
    x = x.reshape(-1)
    with np.errstate(all="ignore"):
        l = (x / c).astype(F)
        want = ((l < 0) | (l > 1)).astype(F)
    valid_u = (c >= F(2.0 ** -40)) & (c <= F(2.0 ** 40))
    slow = (~(np.abs(x) >= F(2.0 ** -100)) | ~valid_u).reshape(GROUPS, WAVE)
    assert slow[1].all()
    if valid_u.all():
        assert not slow[0].any() and all(0 < slow[g].sum() < WAVE for g in range(2, GROUPS))
    elif valid_u.any():
        assert all(0 < slow[g].sum() < WAVE for g in range(GROUPS) if g != 1)
    else:
        assert slow.all()
    dev = renderer.selftest_math(24, x, c)
    ok = dev == want
    assert ok.all(), _report("out_of_unit_range (c in %r)" % (divisors,), x, dev, want, ok)
