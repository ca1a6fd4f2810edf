"""Temporal reprojection and the a-trous filter on synthetic records (prt_denoise_records_temporal, prt_denoise_records,
prt_read_records_history; include/prt.h).  Rendered frames decide which branches of tm_reproject_kernel run; here the frames are made in
numpy -- a back rectangle, a tilted card in front of it, an uncovered rim, seen consistently from any camera -- and go in as records, so
every branch is there on purpose: the n >= 4 switch of the variance, history_cap reached, alpha = 1, every temporal and a-trous parameter
away from its default, reprojection outside and half outside the frame, pixels the card uncovers, points behind the previous camera,
depth / normal rejections of some of the four taps, non-finite history colours, frames of one row, one column and one pixel, a-trous steps
larger than the frame.  After every call the record history read back and the picture are compared with the float64 mirrors of
tests/mirrors.py -- temporal_ref, denoise_ref -- (the previous history fed to the mirror is the device's own).  Every scenario also runs without a GPU,
the mirror standing in for the device, to assert that the branch it is named for holds enough pixels clear of every threshold."""
import numpy as np
import pytest

from cases import H0, MOVES, _plain_records, _synthetic, T_DEFAULTS, _unit, W0, World
from mirrors import camera_basis, centre_dirs, _close, denoise_ref, lum, project, spatial_variance, temporal_ref
from support import assert_api, bits as _bits, pkg as _pkg, to_device as _to_device

NEW_API = ("prt_read_records_history",)


# ---- no GPU --------------------------------------------------------------------------------------------------------------------------------

def test_api_is_declared_exported_and_bound():
    assert_api(NEW_API)
    assert callable(getattr(_pkg().Renderer, "read_records_history"))


# ---- the synthetic world ---------------------------------------------------------------------------------------------------------------------

def _geometry(rec, cam, cam_prev):
    """where the mirror projects every pixel of `rec` (camera cam) in the previous camera: x', y', dot(e, f), and the coverage"""
    H, W = rec.shape[:2]
    g = rec[..., 4:12].astype(np.float64)
    cov = g[..., 3] > 0
    B, Bp = camera_basis(cam), camera_basis(cam_prev)
    d = centre_dirs(B, W, H)
    e = np.where(cov[..., None], B[0] + d * g[..., 7][..., None] - Bp[0], d)
    with np.errstate(all="ignore"):
        xp, yp, ef = project(Bp, e, W, H)
    return xp, yp, ef, cov


def _taps_hit(mask, xp, yp, ok):
    """pixels (of `ok`) one of whose 2x2 taps at (x', y') lies on `mask` with a bilinear weight above 1e-6"""
    H, W = mask.shape
    x0, y0 = np.floor(np.where(ok, xp, 0)), np.floor(np.where(ok, yp, 0))
    fx, fy = np.where(ok, xp, 0) - x0, np.where(ok, yp, 0) - y0
    out = np.zeros((H, W), dtype=bool)
    for t in range(4):
        tx, ty = x0.astype(np.int64) + (t & 1), y0.astype(np.int64) + (t >> 1)
        w = (fx if t & 1 else 1 - fx) * (fy if t >> 1 else 1 - fy)
        inside = (tx >= 0) & (tx < W) & (ty >= 0) & (ty < H)
        out |= ok & inside & (w > 1e-6) & mask[np.clip(ty, 0, H - 1), np.clip(tx, 0, W - 1)]
    return out


# ---- one sequence of temporal calls, each compared with the mirrors --------------------------------------------------------------------------

class Seq:
    """a sequence of prt_denoise_records_temporal calls on context `rc`.  step() feeds one frame of records, reads the record history back and
    compares it and the picture with the mirrors; it returns (the mirror's dict, the history [H, W, 8], the picture).  rc None: no device --
    the mirror's own history (as float32) stands in, nothing is compared, and the caller's assertions about the mirror still run.
    other: a second context run in step with passes = 1, for feedback = "atrous" (test_temporal's _orbit_check)"""

    def __init__(self, W, H, rc=None, other=None, feedback="integrated", passes=5, label="", **tparams):
        self.W, self.H, self.rc, self.other, self.feedback, self.passes, self.label = W, H, rc, other, feedback, passes, label
        self.t = dict(T_DEFAULTS, **tparams)
        self.prev = None
        self.k = 0
        self.worst = {}

    def reset(self, **tparams):
        self.t = dict(T_DEFAULTS, **tparams)
        self.prev = None
        for r in (self.rc, self.other):
            if r is not None:
                r.reset_records_history()

    def _note(self, what, err, bound, mask):
        if mask.any():
            with np.errstate(all="ignore"):
                self.worst[what] = max(self.worst.get(what, 0.0), float(np.max((err / bound)[mask])))

    def _cmp(self, what, got, ref, scale, mask, rel=1e-4):
        got, ref = np.asarray(got, dtype=np.float64), np.asarray(ref, dtype=np.float64)
        if got.ndim == 3:
            scale = scale[..., None]
            mask = np.broadcast_to(mask[..., None], got.shape)
        self._note(what, np.abs(got - ref), rel * np.maximum(scale, 1e-6) * np.ones_like(got), mask)
        bad = mask & ~_close(got, ref, scale, rel)
        assert not bad.any(), (self.label, self.k, what, np.argwhere(bad)[:4].tolist())

    def step(self, rec, cam):
        with np.errstate(invalid="ignore"):                                # (NaN and Inf colours are part of the frames)
            return self._step(rec, cam)

    def _step(self, rec, cam):
        W, H, t = self.W, self.H, self.t
        fb, g, v_frame = rec[..., 0:4], rec[..., 4:12], rec[..., 12].astype(np.float64)
        hist_prev, g_prev, cam_prev = self.prev if self.prev is not None else (None, g, cam)
        ref = temporal_ref(fb, g, g_prev, hist_prev, cam, cam_prev, v_frame, **t)
        fin = np.isfinite(fb[..., :3]).all(-1)
        out = None
        if self.rc is None:
            h = np.concatenate([ref["ci"], ref["n"][..., None], ref["m1"][..., None], ref["m2"][..., None], ref["v"][..., None],
                                np.zeros((H, W, 1))], -1).astype(np.float32)
            h[..., :3] = np.where(fin[..., None], h[..., :3], fb[..., :3])
        else:
            records = _to_device(rec)
            kw = dict(t, feedback=self.feedback)
            out = self.rc.denoise_records_temporal(records, W, H, cam, passes=self.passes, **kw)
            h = self.rc.read_records_history(W, H)
            m = ref["margin_other"]
            mf = m & fin
            assert (_bits(h[..., 7]) == 0).all()
            self._cmp("n", h[..., 3], ref["n"], ref["n"], m)
            self._cmp("m1", h[..., 4], ref["m1"], ref["m1scale"], mf)
            self._cmp("m2", h[..., 5], ref["m2"], ref["m2scale"], mf)
            # v: the mirror's choice, except where its n is within 1e-3 of 4 -- there the device's f32 n may fall on either side of the
            # switch, and v must be one of the two candidates
            moment = np.maximum(ref["m2"] - ref["m1"] ** 2, 0.0)
            sharp = m & ~ref["near4"] & (fin | (ref["n"] < 4))
            self._cmp("v", h[..., 6], ref["v"], np.where(ref["n"] >= 4, ref["m2scale"], v_frame.max()), sharp)
            either = _close(h[..., 6], moment, ref["m2scale"]) | _close(h[..., 6], v_frame, v_frame.max())
            assert either[m & ref["near4"] & fin].all(), (self.label, self.k, "v at n = 4")
            # a pixel whose colour is not finite keeps its words and restarts
            assert (_bits(h[..., :3][~fin]) == _bits(fb[..., :3][~fin])).all() and (h[..., 3][~fin] == 1.0).all(), (self.label, self.k)
            assert np.isfinite(h[fin]).all() and np.isfinite(out[fin]).all(), (self.label, self.k)
            assert (_bits(out[..., 3]) == _bits(fb[..., 3])).all(), (self.label, self.k)
            if self.feedback == "integrated":
                self._cmp("c", h[..., :3], ref["ci"], ref["cscale"], mf)
                # the filter: prt_denoise's passes over the device's own {c_i, v}
                fref = denoise_ref(np.concatenate([h[..., :3], fb[..., 3:4]], -1), g, h[..., 6].astype(np.float64), passes=self.passes)
                bound = 1e-4 * np.abs(fref[fin]).max()
                self._note("picture", np.abs(out - fref).max(-1), np.full((H, W), bound), fin)
                assert np.abs(out - fref)[fin].max() <= bound, (self.label, self.k, "picture")
            else:
                o1 = self.other.denoise_records_temporal(records, W, H, cam, passes=1, **kw)
                h1 = self.other.read_records_history(W, H)
                assert (_bits(h1) == _bits(h)).all(), (self.label, self.k)             # the history does not depend on the passes after pass 0
                assert (_bits(h[..., :3]) == _bits(o1[..., :3])).all(), (self.label, self.k)       # feedback = pass 0's output
                # pass 0 of the mirror's {c_i, v}, on the pixels whose 5x5 window is all clear of thresholds
                ci = np.where(fin[..., None], ref["ci"], fb[..., :3].astype(np.float64))
                p0 = denoise_ref(np.concatenate([ci, fb[..., 3:4]], -1), g, h[..., 6].astype(np.float64), passes=1)
                win = fin.copy()
                pad = np.pad(m, 2, constant_values=True)
                for dy in range(5):
                    for dx in range(5):
                        win &= pad[dy:dy + H, dx:dx + W]
                assert win.mean() >= 0.5, (self.label, self.k, win.mean())
                bound = 1e-4 * np.abs(p0[..., :3][fin]).max()
                self._note("pass 0", np.abs(o1[..., :3] - p0[..., :3]).max(-1), np.full((H, W), bound), win)
                assert (np.abs(o1[..., :3] - p0[..., :3]).max(-1) <= bound)[win].all(), (self.label, self.k, "pass 0")
        self.prev = (h, g, cam)
        self.k += 1
        return ref, h, out

    def report(self):
        if self.rc is not None:
            print("%s: largest error / bound: %s" % (self.label, "  ".join("%s %.3g" % kv for kv in sorted(self.worst.items()))))


def _cam(prt, W, H, **orbit):
    return prt.orbit_camera(W, H, **orbit) if orbit else prt.default_camera(W, H)


# ---- the scenarios (each runs on a Seq with or without a device) ------------------------------------------------------------------------------

def scenario_still(prt, world, seq):
    """a still camera, 7 calls, default parameters: n = 1 .. 7 crosses the n >= 4 switch of the variance"""
    W, H = seq.W, seq.H
    cam = _cam(prt, W, H)
    for k in range(7):
        rec, _ = world.records(cam, W, H, k)
        ref, h, _ = seq.step(rec, cam)
        m = ref["margin_other"]
        assert m.mean() >= 0.95, (k, m.mean())
        assert (np.abs(ref["n"] - (k + 1)) < 1e-6)[m].all(), k
        assert (np.abs(h[..., 3] - (k + 1)) < 1e-3)[m].all(), k
        if k == 3:
            assert (m & ref["near4"]).sum() >= 0.9 * W * H               # the switch, on (nearly) every pixel, not masked
        if k >= 4:                                                        # ... and past it: the moment variance, not the frame's
            assert (m & ~ref["near4"] & (ref["n"] >= 4)).sum() >= 0.9 * W * H
            assert (np.abs(ref["v"] - rec[..., 12]) > 1e-3 * rec[..., 12])[m].mean() > 0.9
    assert (h[..., 3] >= 5).mean() >= 0.5
    assert ((1.0 / ref["n"] < 0.2) & m).mean() >= 0.5                     # ac = alpha_color = 0.2 > 1 / n is in force (the mirror's c_i has it)


def scenario_cap(cap):
    def run(prt, world, seq):
        """alpha = 0: a running mean until n reaches history_cap"""
        W, H = seq.W, seq.H
        cam = _cam(prt, W, H)
        seq.reset(alpha_color=0.0, alpha_moments=0.0, history_cap=cap)
        for k in range(6):
            rec, _ = world.records(cam, W, H, 20 + k)
            ref, h, _ = seq.step(rec, cam)
            m = ref["margin_other"]
            assert m.mean() >= 0.95, (k, m.mean())
            want = min(k + 1, cap)
            assert (np.abs(ref["n"] - want) < 1e-6)[m].all() and (np.abs(h[..., 3] - want) < 1e-3)[m].all(), (cap, k)
            if k >= cap:
                assert (m & (ref["n"] >= cap - 1e-6) & ref["hist"]).sum() >= 0.9 * W * H              # the cap is reached: fminf(.., cap) decides
            if cap == 1:
                # ac = 1: c_i = c_h + (c - c_h), which is c exactly -- c_h is the same pixel's colour with other noise, within a factor
                # of 2 of c, so the difference is exact (Sterbenz)
                assert (_bits(h[..., :3]) == _bits(rec[..., 0:3])).all(), k
            if cap <= 3:
                assert (_bits(h[..., 6]) == _bits(rec[..., 12]))[m].all(), (cap, k)                     # never leaves the frame's variance
            if cap == 4 and k >= 4:
                # n = min(n_h + 1, 4) = 4 exactly: the moment variance (n >= 4, not n > 4)
                exact = m & (h[..., 3] == 4.0)
                assert exact.sum() >= 20, exact.sum()
                moment = np.maximum(ref["m2"] - ref["m1"] ** 2, 0.0)
                assert _close(h[..., 6], moment, ref["m2scale"])[exact].all(), k
                assert (np.abs(moment - rec[..., 12]) > 1e-3 * rec[..., 12])[exact].mean() > 0.9
    return run


def scenario_alpha_one(prt, world, seq):
    """alpha_color = 1: c_i = c; alpha_moments = 1: m1 = L, m2 = L^2, v = 0 once n >= 4"""
    W, H = seq.W, seq.H
    cam = _cam(prt, W, H)
    for which in ("alpha_color", "alpha_moments"):
        seq.reset(**{which: 1.0})
        for k in range(5):
            rec, _ = world.records(cam, W, H, 40 + k)
            ref, h, _ = seq.step(rec, cam)
            m = ref["margin_other"]
            assert m.mean() >= 0.95 and (ref["hist"] & m).mean() >= (0.9 if k else 0.0)
            L = lum(rec[..., 0:3].astype(np.float64))
            if which == "alpha_color":
                assert (_bits(h[..., :3]) == _bits(rec[..., 0:3])).all(), k            # (exact: see scenario_cap)
                if k:
                    assert (np.abs(ref["m1"] - L) > 1e-3 * L)[m].mean() > 0.5                   # ... while the moments still blend
            else:
                # m1 = m1_h + (L - m1_h) and m2 likewise: L and L^2 to a few roundings of f32 (2^-23 each), so m2 - m1^2 is below 1e-6 L^2
                assert (np.abs(h[..., 4] - L) <= 1e-6 * L).all() and (np.abs(h[..., 5] - L * L) <= 1e-6 * L * L).all(), k
                if k >= 3:
                    assert (h[..., 3] >= 3.999)[m].all() and (h[..., 6] <= 1e-6 * L * L)[m & ~ref["near4"]].all(), k
                if k:
                    assert (np.abs(ref["ci"] - rec[..., 0:3]).max(-1) > 1e-3)[m].mean() > 0.5   # ... while the colour still blends


def scenario_moving(prt, world, seq):
    """a camera that moves by pixels per call: reprojection outside the frame, half outside it (renormalised by the taps inside), and onto
    the card from pixels it has just uncovered.  The populations are counted over the calls of the orbit"""
    W, H = seq.W, seq.H
    count = dict(outside=0, xband=0, yband=0, uncovered=0, kept=0)
    prev = None
    for k, mv in enumerate(MOVES):
        cam = _cam(prt, W, H, **mv)
        rec, sid = world.records(cam, W, H, 60 + k)
        ref, h, _ = seq.step(rec, cam)
        m = ref["margin_other"]
        assert m.mean() >= 0.95, (k, m.mean())
        if prev is not None:
            xp, yp, ef, cov = _geometry(rec, cam, prev[0])
            inr = (ef > 0) & (xp > -1) & (xp < W) & (yp > -1) & (yp < H)
            fresh = m & ~ref["hist"]
            if seq.rc is not None:
                assert (h[..., 3][fresh] == 1.0).all() and (_bits(h[..., :3][fresh]) == _bits(rec[..., 0:3][fresh])).all(), k
            count["outside"] += int((m & (ef > 0) & ~inr).sum())
            count["xband"] += int((m & inr & ref["hist"] & ((xp < 0) | (xp > W - 1))).sum())
            count["yband"] += int((m & inr & ref["hist"] & ((yp < 0) | (yp > H - 1))).sum())
            inside = inr & (xp >= 0) & (xp <= W - 1) & (yp >= 0) & (yp <= H - 1)
            count["uncovered"] += int((fresh & inside & (sid == 1) & _taps_hit(prev[1] == 2, xp, yp, inside)).sum())
            count["kept"] += int((m & ref["hist"]).sum())
        prev = (cam, sid)
    print("moving camera: margin-clear pixels per branch:", count)
    assert min(count["outside"], count["xband"], count["yband"], count["uncovered"]) >= 20, count
    assert count["kept"] >= 0.5 * W * H * (len(MOVES) - 1), count


def scenario_turned(prt, world, seq):
    """the previous camera looks the other way: dot(e, f) <= 0 for points and for directions, and every such pixel restarts"""
    W, H = seq.W, seq.H
    cam_a, cam_b = _cam(prt, W, H, d_yaw=3.0), _cam(prt, W, H)
    Ba, Bb = camera_basis(cam_a), camera_basis(cam_b)
    assert (Ba[1] - Ba[0]) @ (Bb[1] - Bb[0]) < 0                           # turned by more than 90 degrees
    seq.step(world.records(cam_a, W, H, 80)[0], cam_a)
    rec, _ = world.records(cam_b, W, H, 81)
    ref, h, _ = seq.step(rec, cam_b)
    m = ref["margin_other"]
    assert m.mean() >= 0.95, m.mean()
    xp, yp, ef, cov = _geometry(rec, cam_b, cam_a)
    behind = m & (ef <= 0)
    print("turned camera: behind the previous camera: %d covered, %d uncovered pixels" % ((behind & cov).sum(), (behind & ~cov).sum()))
    assert (behind & cov).sum() >= 20 and (behind & ~cov).sum() >= 20
    assert not ref["hist"][behind].any()
    assert (h[..., 3][behind] == 1.0).all() and (_bits(h[..., :3][behind]) == _bits(rec[..., 0:3][behind])).all()


DEPTH_ZONES = ((5, 11, 1.02), (11, 17, 1.10), (17, 23, 1.30))             # columns [a, b): the first frame's depth times s
NORMAL_ZONES = ((4, 10, 0.97), (10, 16, 0.85), (16, 22, 0.6))             # rows [a, b): the first frame's normals turned by acos(c)
STRIP = (25, 32)                                                          # columns [a, b): depth times 1.3 on the odd ones only
SUBPIXEL = dict(d_yaw=0.006, d_pitch=0.004)


def _zoned(rec):
    rec = rec.copy()
    for a, b, s in DEPTH_ZONES:
        rec[:, a:b, 11] *= np.float32(s)
    rec[:, STRIP[0] + 1:STRIP[1]:2, 11] *= np.float32(1.3)
    for a, b, c in NORMAL_ZONES:
        n = rec[a:b, :, 8:11].astype(np.float64)
        t = np.cross(n, [0.0, 1.0, 0.0])
        with np.errstate(all="ignore"):
            t = np.where(np.linalg.norm(t, axis=-1, keepdims=True) > 0, _unit(t), 0.0)
        rec[a:b, :, 8:11] = c * n + np.sqrt(1 - c * c) * t
    return rec


def scenario_tolerances(prt, world, seq):
    """tau_z and cos_n are read from the parameters: the zones of a distorted first frame that keep their history at (0.05, 0.9) and at
    (0.2, 0.7), and a strip where some of the four taps survive"""
    W, H = seq.W, seq.H
    cam_a, cam_b = _cam(prt, W, H), _cam(prt, W, H, **SUBPIXEL)
    rec_a = _zoned(world.records(cam_a, W, H, 90)[0])
    rec_b, _ = world.records(cam_b, W, H, 91)
    xp, yp, ef, cov = _geometry(rec_b, cam_b, cam_a)
    xs = np.arange(W)[None, :]
    assert (np.abs(xp - xs)[cov] < 1.0).all() and (np.abs(xp - xs)[cov] > 0.05).mean() > 0.7       # a sub-pixel step
    kept, clear = {}, {}
    for name, tol in (("default", dict()), ("loose", dict(tau_z=0.2, cos_n=0.7))):
        seq.reset(**tol)
        seq.step(rec_a, cam_a)
        ref, h, _ = seq.step(rec_b, cam_b)
        m = ref["margin_other"]
        assert m.mean() >= 0.95, (name, m.mean())
        if seq.rc is not None:
            assert ((h[..., 3] > 1.0) == ref["hist"])[m].all(), name                            # the zones that keep their history: the mirror's
        kept[name], clear[name] = ref["hist"], m
        in_strip = (xs >= STRIP[0] + 1) & (xs < STRIP[1] - 1) & cov
        some = m & in_strip & ref["hist"] & (ref["sw"] < 0.99) & (ref["sw"] > 0.011)
        print("tolerances (%s): %d strip pixels keep some of their taps" % (name, some.sum()))
        assert some.sum() >= 4, (name, some.sum())
    both = clear["default"] & clear["loose"] & cov
    n_both, n_loose, n_none = (both & kept["default"]).sum(), (both & kept["loose"] & ~kept["default"]).sum(), (both & ~kept["loose"]).sum()
    print("tolerances: kept by both %d, by (0.2, 0.7) only %d, by neither %d" % (n_both, n_loose, n_none))
    assert min(n_both, n_loose, n_none) >= 20
    assert not (both & kept["default"] & ~kept["loose"]).any()


BAD = [((6, 8), (np.nan, None, None)), ((9, 20), (np.nan, np.nan, np.nan)), ((14, 30), (None, None, np.nan)), ((20, 12), (None, np.nan, None)),
       ((5, 27), (np.inf, None, None)), ((12, 14), (np.inf, np.inf, np.inf)), ((17, 24), (None, np.inf, None)), ((23, 18), (None, None, np.inf))]


def scenario_non_finite(prt, world, seq):
    """NaN and +Inf colours: the pixel restarts and keeps its words; in the next frame its neighbours drop that tap and renormalise"""
    W, H = seq.W, seq.H
    cam_a, cam_b = _cam(prt, W, H), _cam(prt, W, H, **SUBPIXEL)
    for k in range(3):
        seq.step(world.records(cam_a, W, H, 100 + k)[0], cam_a)
    rec, _ = world.records(cam_a, W, H, 104)
    bad = np.zeros((H, W), dtype=bool)
    for (y, x), vals in BAD:
        bad[y, x] = True
        for ch, val in enumerate(vals):
            if val is not None:
                rec[y, x, ch] = val
    ref, h, _ = seq.step(rec, cam_a)
    assert (~np.isfinite(rec[..., 0:3]).all(-1) == bad).all() and not ref["hist"][bad].any()
    assert (h[..., 3][bad] == 1.0).all() and (_bits(h[..., :3][bad]) == _bits(rec[..., 0:3][bad])).all()
    rec, _ = world.records(cam_b, W, H, 103)
    ref, h, _ = seq.step(rec, cam_b)
    m = ref["margin_other"]
    assert m.mean() >= 0.95, m.mean()
    xp, yp, ef, cov = _geometry(rec, cam_b, cam_a)
    inr = (ef > 0) & (xp > -1) & (xp < W) & (yp > -1) & (yp < H)
    dropped = m & ref["hist"] & _taps_hit(bad, xp, yp, inr)
    print("non-finite colours (%s): %d pixels drop a tap and renormalise" % (seq.feedback, dropped.sum()))
    assert dropped.sum() >= 20, dropped.sum()
    assert (ref["sw"][dropped] < 1 - 1e-6).all()
    assert np.isfinite(h[..., :7]).all()


def scenario_2x2(prt, world, seq):
    """the smallest frame with a projection (W - 1 = H - 1 = 1)"""
    cam = prt.default_camera(2, 2, fovx=25.0)                              # (narrow: the four corner rays hit the back rectangle)
    for k in range(2):
        rec, sid = world.records(cam, 2, 2, 110 + k)
        assert (sid == 1).all()
        ref, h, _ = seq.step(rec, cam)
        assert ref["margin_other"].sum() >= 4 and (ref["hist"].sum() == (4 if k else 0))
        assert (np.abs(h[..., 3] - (k + 1)) < 1e-3).all()


SCENARIOS = {"still": scenario_still, "cap1": scenario_cap(1), "cap2": scenario_cap(2), "cap3": scenario_cap(3), "cap4": scenario_cap(4),
             "alpha_one": scenario_alpha_one, "moving": scenario_moving, "turned": scenario_turned, "tolerances": scenario_tolerances,
             "non_finite": scenario_non_finite, "2x2": scenario_2x2}


def _size(name):
    return (2, 2) if name == "2x2" else (W0, H0)


@pytest.mark.parametrize("name", list(SCENARIOS))
def test_scenario_holds_its_branches_on_the_mirror_alone(name):
    prt = _pkg()
    W, H = _size(name)
    SCENARIOS[name](prt, World(prt), Seq(W, H, label=name))


def test_world_is_the_same_from_every_camera():
    """a covered pixel's world point, projected into another camera, lands where that camera's frame shows the same surface at the same depth"""
    prt = _pkg()
    world = World(prt)
    cam_a, cam_b = _cam(prt, W0, H0), _cam(prt, W0, H0, **MOVES[2])
    rec_a, sid_a = world.records(cam_a, W0, H0, 0, noise=0.0)
    rec_b, sid_b = world.records(cam_b, W0, H0, 0, noise=0.0)
    assert set(np.unique(sid_a)) == {0, 1, 2} and (sid_a == 0).sum() >= 100 and (sid_a == 2).sum() >= 50
    xp, yp, ef, cov = _geometry(rec_b, cam_b, cam_a)
    Ba, Bb = camera_basis(cam_a), camera_basis(cam_b)
    X = Bb[0] + centre_dirs(Bb, W0, H0) * rec_b[..., 11].astype(np.float64)[..., None]
    inside = cov & (ef > 0) & (xp >= 0) & (xp <= W0 - 1) & (yp >= 0) & (yp <= H0 - 1)
    x0, y0 = np.floor(np.where(inside, xp, 0)).astype(np.int64), np.floor(np.where(inside, yp, 0)).astype(np.int64)
    x1, y1 = np.minimum(x0 + 1, W0 - 1), np.minimum(y0 + 1, H0 - 1)
    fx, fy = np.where(inside, xp, 0) - x0, np.where(inside, yp, 0) - y0
    same = inside & (sid_a[y0, x0] == sid_b) & (sid_a[y0, x1] == sid_b) & (sid_a[y1, x0] == sid_b) & (sid_a[y1, x1] == sid_b)
    za = rec_a[..., 11].astype(np.float64)
    z = (za[y0, x0] * (1 - fx) + za[y0, x1] * fx) * (1 - fy) + (za[y1, x0] * (1 - fx) + za[y1, x1] * fx) * fy
    assert (same & (sid_b == 1)).sum() >= 200 and (same & (sid_b == 2)).sum() >= 20
    assert (np.abs(z - np.linalg.norm(X - Ba[0], axis=-1)) < 2e-3 * z)[same].all()       # (a plane's depth along the rays is not quite bilinear)
    # colours are the world's: a still camera sees the same picture but for the noise
    again, _ = world.records(cam_a, W0, H0, 1, noise=0.0)
    assert (_bits(again[..., 0:3]) == _bits(rec_a[..., 0:3])).all() and (_bits(again[..., 4:12]) == _bits(rec_a[..., 4:12])).all()


# ---- on the GPU ------------------------------------------------------------------------------------------------------------------------------

def _ctx(prt):
    return prt.Renderer(prt.HostScene("cornell_coat.json").config(), device=0)              # no scene, no camera, no frame


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(SCENARIOS))
def test_scenario_equals_the_formulas(prt, name):
    W, H = _size(name)
    rc = _ctx(prt)
    seq = Seq(W, H, rc=rc, label=name)
    SCENARIOS[name](prt, World(prt), seq)
    seq.report()
    rc.close()


@pytest.mark.gpu
def test_non_finite_colours_with_atrous_feedback(prt):
    rc, other = _ctx(prt), _ctx(prt)
    seq = Seq(W0, H0, rc=rc, other=other, feedback="atrous", label="non_finite, atrous")
    scenario_non_finite(prt, World(prt), seq)
    seq.report()
    rc.close()
    other.close()


@pytest.mark.gpu
@pytest.mark.parametrize("W,H", [(1, 1), (1, 9), (9, 1)])
def test_frames_of_one_row_or_column_have_no_history(prt, W, H):
    """sx = x / (W - 1) or sy is 0 / 0: the projection is NaN, dot(e, f) > 0 is false, every call is prt_denoise_records'"""
    rc, plain = _ctx(prt), _ctx(prt)
    cam = prt.default_camera(W, H)
    for k in range(2):
        rec = _plain_records(W, H, 120 + k)
        records = _to_device(rec)
        kw = dict(passes=5, sigma_l=2.0, sigma_z=2.0)
        got = rc.denoise_records_temporal(records, W, H, cam, feedback="integrated", **kw)
        want = plain.denoise_records(records, W, H, **kw)
        assert (_bits(got) == _bits(want)).all(), k
        assert np.isfinite(got).all()
        h = rc.read_records_history(W, H)
        assert (h[..., 3] == 1.0).all() and (_bits(h[..., :3]) == _bits(rec[..., 0:3])).all(), k
        assert (_bits(h[..., 6]) == _bits(rec[..., 12])).all() and np.isfinite(h).all(), k
        v = rec[..., 12].astype(np.float64)
        ref = denoise_ref(rec[..., 0:4], rec[..., 4:12], v, sigma_l=2.0, sigma_z=2.0)
        assert np.abs(got - ref).max() <= 1e-4 * np.abs(ref).max(), k
    rc.close()
    plain.close()


SIGMAS = [dict(passes=8), dict(sigma_l=0.5), dict(sigma_n=4.0), dict(sigma_z=8.0), dict(sigma_a=0.5), dict(passes=8, sigma_l=0.5, sigma_z=8.0)]


def _kw_id(kw):
    return "-".join("%s=%g" % kv for kv in kw.items())


@pytest.fixture(scope="module")
def synthetic():
    """test_denoise_records' synthetic records with the normals of each plane jittered by a few degrees (with one normal per plane the
    depth edge hides sigma_n), and the mirror's pictures of them: computed once, never changed"""
    W, H = 40, 33
    rec, nan_at = _synthetic(W, H)
    n = rec[..., 8:11].astype(np.float64)
    has = np.linalg.norm(n, axis=-1, keepdims=True) > 0                  # (the uncovered band and the zero normal stay as they are)
    jit = n + np.random.default_rng(11).uniform(-0.08, 0.08, n.shape)
    rec[..., 8:11] = np.where(has, jit / np.linalg.norm(jit, axis=-1, keepdims=True), 0.0)
    fin = np.ones((H, W), dtype=bool)
    fin[nan_at] = False
    variances = {"stats": rec[..., 12].astype(np.float64), "spatial": spatial_variance(rec[..., 0:3].astype(np.float64))}
    refs = {(_kw_id(kw), s): denoise_ref(rec[..., 0:4], rec[..., 4:12], v, **kw) for kw in [dict()] + SIGMAS for s, v in variances.items()}
    for a in [rec] + list(refs.values()):
        a.setflags(write=False)
    return rec, fin, variances, refs


@pytest.mark.parametrize("kw", SIGMAS, ids=_kw_id)
def test_atrous_parameters_move_the_mirror(synthetic, kw):
    """a case checks its parameter only if the parameter changes the picture: by more than the comparison's bound at 20 pixels or more"""
    rec, fin, variances, refs = synthetic
    for source in variances:
        ref, default = refs[(_kw_id(kw), source)], refs[("", source)]
        moved = fin & (np.abs(ref - default).max(-1) > 2e-4 * np.abs(ref[fin]).max())
        assert moved.sum() >= 20, (kw, source, moved.sum())


@pytest.mark.gpu
@pytest.mark.parametrize("kw", SIGMAS, ids=_kw_id)
def test_atrous_parameters_and_long_passes(prt, synthetic, kw):
    """every sigma away from its default, one at a time, and passes 6 .. 8, whose steps (32 .. 128) reach the frame's far rows or beyond it"""
    rec, fin, variances, refs = synthetic
    H, W = rec.shape[:2]
    rc = _ctx(prt)
    records = _to_device(np.array(rec))
    for source in variances:
        got = rc.denoise_records(records, W, H, var_source=source, **kw)
        assert np.isfinite(got[fin]).all() and (_bits(got[~fin]) == _bits(rec[..., 0:4][~fin])).all(), source
        ref = refs[(_kw_id(kw), source)]
        err, bound = np.abs(got[fin] - ref[fin]).max(), 1e-4 * np.abs(ref[fin]).max()
        print("a-trous %s, %s: max error %.3e (bound %.3e)" % (kw, source, err, bound))
        assert err <= bound, (kw, source, err)
    rc.close()


@pytest.mark.gpu
@pytest.mark.parametrize("W,H", [(1, 1), (1, 7), (3, 2)])
def test_atrous_on_tiny_frames(prt, W, H):
    rc = _ctx(prt)
    rec = _plain_records(W, H, 130)
    records = _to_device(rec)
    for source, v in (("stats", rec[..., 12].astype(np.float64)), ("spatial", spatial_variance(rec[..., 0:3].astype(np.float64)))):
        for kw in (dict(), dict(passes=8), dict(passes=8, sigma_l=0.5, sigma_n=4.0, sigma_z=8.0, sigma_a=0.5)):
            got = rc.denoise_records(records, W, H, var_source=source, **kw)
            ref = denoise_ref(rec[..., 0:4], rec[..., 4:12], v, **kw)
            err, bound = np.abs(got - ref).max(), 1e-4 * np.abs(ref).max()
            print("a-trous %dx%d %s, %s: max error %.3e (bound %.3e)" % (W, H, kw, source, err, bound))
            assert np.isfinite(got).all() and err <= bound, (source, kw, err)
    rc.close()


@pytest.mark.gpu
def test_read_records_history_refusals(prt):
    W, H = 12, 7
    rc = _ctx(prt)
    cam = prt.default_camera(W, H)
    records = _to_device(_plain_records(W, H, 140))

    def code(fn, *a, **k):
        with pytest.raises(prt.PrtError) as e:
            fn(*a, **k)
        return e.value.code

    assert code(rc.read_records_history, W, H) == prt.PRT_ERR_NOT_READY                              # empty
    rc.denoise_records(records, W, H)                                                                # (the plain filter keeps no history)
    assert code(rc.read_records_history, W, H) == prt.PRT_ERR_NOT_READY
    rc.denoise_records_temporal(records, W, H, cam)
    h = rc.read_records_history(W, H)
    assert h.shape == (H, W, 8) and (h[..., 3] == 1.0).all()
    assert (_bits(rc.read_records_history(W, H)) == _bits(h)).all()                                  # reading changes nothing
    for w, hh in ((W, H - 1), (W + 1, H), (H, W), (0, H), (W, -1)):
        assert code(rc.read_records_history, w, hh) == prt.PRT_ERR_INVALID_ARGUMENT, (w, hh)
    assert rc.lib.prt_read_records_history(rc.ctx, W, H, None) == prt.PRT_ERR_INVALID_ARGUMENT
    assert (_bits(rc.read_records_history(W, H)) == _bits(h)).all()                                  # (refusals leave it alone)
    rc.denoise_records_temporal(records, W, H, cam)
    assert (np.abs(rc.read_records_history(W, H)[..., 3] - 2.0) < 1e-3).mean() > 0.5
    rc.reset_records_history()
    assert code(rc.read_records_history, W, H) == prt.PRT_ERR_NOT_READY
    rc.denoise_records_temporal(records, W, H, cam)
    rc.denoise_records_temporal(records, W, H - 2, cam)                                              # another size: the history is that frame's now
    assert code(rc.read_records_history, W, H) == prt.PRT_ERR_INVALID_ARGUMENT
    small = rc.read_records_history(W, H - 2)
    assert small.shape == (H - 2, W, 8) and (small[..., 3] == 1.0).all()
    assert code(rc.read_history) == prt.PRT_ERR_INVALID_ARGUMENT                                      # the context's own history is another matter
    rc.close()
