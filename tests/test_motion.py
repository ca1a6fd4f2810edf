"""Motion of deforming meshes in the temporal reprojection (prt_set_motion, prt_read_motion, prt_export_motion,
prt_denoise_records_temporal_motion; include/prt.h).  What is checked: the bodies of csrc/hip/pt_motion.h, compiled for the host, against a
float32 numpy mirror byte for byte; a float64 mirror of the temporal step with the motion plane (temporal_ref plus D: temporal_ref_motion of tests/mirrors.py), which
without a plane and with a plane of zeros is temporal_ref; a synthetic world with a card that moves by pixels per frame, where the plane
must cut the error of the integrated colour at least in half (on the mirror alone, and on the device); the motion plane of rendered scenes
against a float64 caster; the snapshot rule; the plumbing (guides unchanged, splits of the frame, export, the records call, motion off,
refusals, the read-only property, parallel.denoise_on_rank0)."""
import ctypes as C
import importlib
import os

import numpy as np
import pytest

from conftest import PKG_NAME
from cases import _cmp, H0, _plain_records, Rendered, RH, RW, T_DEFAULTS, _unit, W0, World
from mirrors import camera_basis, centre_dirs, _close, D_BOUND, denoise_ref, _mirror_history, project, temporal_ref, temporal_ref_motion
from support import assert_api, bits as _bits, pkg as _pkg, rodrigues as _rodrigues, to_device as _to_device


NEW_API = ("prt_set_motion", "prt_read_motion", "prt_export_motion", "prt_denoise_records_temporal_motion")
f32 = np.float32


# ---- no GPU: the API -----------------------------------------------------------------------------------------------------------------------------

def test_api_is_declared_exported_and_bound():
    header = assert_api(NEW_API)
    assert "PRT_ABI_VERSION 3" in header and "GHOSTS" not in header
    R = _pkg().Renderer
    for name in ("set_motion", "read_motion", "export_motion"):
        assert callable(getattr(R, name)), name
    import inspect
    assert "motion" in inspect.signature(R.denoise_records_temporal).parameters
    par = importlib.import_module(PKG_NAME + ".parallel")
    assert "motion" in inspect.signature(par.denoise_on_rank0).parameters


# ---- no GPU: the bodies of pt_motion.h against a float32 mirror ------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def emu():
    import motion_api
    motion_api.lib()
    return motion_api


def mirror_point(rec, u, v):
    """prt.h: q(rec) = (p0 - e1 u) + e2 v per component, float32, one rounding per operation"""
    rec, u, v = np.asarray(rec, dtype=f32), np.asarray(u, dtype=f32)[:, None], np.asarray(v, dtype=f32)[:, None]
    return (rec[:, 0:3] - rec[:, 3:6] * u) + rec[:, 6:9] * v


def mirror_displacement(prev, cur, u, v):
    return mirror_point(prev, u, v) - mirror_point(cur, u, v)


def mirror_pixel(d, hit, contributing):
    """prt.h: D = (sum of d_s in sample order) / (float)hits, m = (float)contributing * (1 / samples); zeros without hits"""
    K = len(hit)
    s, n, hits = np.zeros(3, dtype=f32), 0, 0
    for k in range(K):
        if not hit[k]:
            continue
        hits += 1
        if contributing[k]:
            s = s + np.asarray(d[k], dtype=f32)
            n += 1
    if hits == 0:
        return np.zeros(4, dtype=f32)
    return np.concatenate([s / f32(hits), [f32(n) * (f32(1.0) / f32(K))]]).astype(f32)


def _cases(seed=5, n=4096):
    """(prev records, cur records, u, v): random ones, then the edges the contract names"""
    rng = np.random.default_rng(seed)
    prev = rng.uniform(-3, 3, (n, 12)).astype(f32)
    cur = (prev + rng.normal(0, 0.2, (n, 12))).astype(f32)
    u = rng.uniform(0, 1, n).astype(f32)
    v = (rng.uniform(0, 1, n) * (1 - u)).astype(f32)
    u[0:64], v[64:128] = 0.0, 0.0                                  # u = 0, v = 0
    v[128:192] = f32(1.0) - u[128:192]                             # u + v = 1
    cur[192:320] = prev[192:320]                                   # identical records
    prev[320:352, 0:3] = 0.0; cur[320:352, 0:3] = -0.0             # signed zeros: p0, and edges times u = 0
    u[320:336] = 0.0; v[336:352] = -0.0
    prev[352:368, 3:9] = -0.0; cur[352:368, 3:9] = 0.0
    tiny = np.array([1e-45, -1e-45, 1.1754942e-38, -1.1754942e-38, 1.1754944e-38, 5e-42], dtype=f32)   # denormals and the smallest normal
    prev[368:432] = rng.choice(tiny, (64, 12)); cur[368:432] = rng.choice(tiny, (64, 12))
    prev[432:464, 0:3] = rng.choice(tiny, (32, 3))                 # a denormal p0 under ordinary edges
    return prev, cur, u, v


def test_displacement_body_equals_the_mirror(emu):
    prev, cur, u, v = _cases()
    n = len(u)
    got = emu.displacement(prev, cur, np.arange(n), np.stack([u, v], -1))
    want = mirror_displacement(prev, cur, u, v)
    assert got.tobytes() == want.astype(f32).tobytes()
    same = slice(192, 320)
    assert (_bits(got[same]) == 0).all(), "identical records: +0 in every component"
    assert (got[:192] != 0).any(-1).mean() > 0.99 and np.isfinite(got).all()
    # the slot indexes both tables: a permutation of the cases through one table of records
    perm = np.random.default_rng(6).permutation(n)
    got_p = emu.displacement(prev, cur, perm, np.stack([u[perm], v[perm]], -1))
    assert got_p.tobytes() == want[perm].astype(f32).tobytes()
    # u weighs vertex 1 and v vertex 2: at (1, 0) and (0, 1) the point is p1 = p0 - e1 and p2 = p0 + e2 of each record
    one, zero = np.ones(n, dtype=f32), np.zeros(n, dtype=f32)
    p1 = emu.displacement(prev, cur, np.arange(n), np.stack([one, zero], -1))
    p2 = emu.displacement(prev, cur, np.arange(n), np.stack([zero, one], -1))
    assert p1.tobytes() == ((prev[:, 0:3] - prev[:, 3:6]) - (cur[:, 0:3] - cur[:, 3:6])).tobytes()
    assert p2.tobytes() == ((prev[:, 0:3] + prev[:, 6:9]) - (cur[:, 0:3] + cur[:, 6:9])).tobytes()


@pytest.mark.parametrize("K", [1, 4, 64])
def test_pixel_reduction_equals_the_mirror(emu, K):
    rng = np.random.default_rng(100 + K)
    for trial in range(200):
        d = rng.normal(0, 1, (K, 3)).astype(f32)
        mode = trial % 5
        hit = rng.uniform(size=K) < (0.0, 1.0, 0.7, 0.7, 0.3)[mode]
        con = hit & (rng.uniform(size=K) < (1.0, 1.0, 0.0, 0.6, 0.5)[mode])
        if trial % 7 == 0:
            d[rng.uniform(size=K) < 0.5] = -0.0
        got, want = emu.pixel(d, hit, con), mirror_pixel(d, hit, con)
        assert got.tobytes() == want.tobytes(), (K, trial)
        if not hit.any():
            assert (_bits(got) == 0).all()
        if hit.any() and not con.any():
            assert (got == 0).all()
        if hit.all() and con.all():
            assert got[3] == f32(K) * (f32(1.0) / f32(K))


# ---- no GPU: prt.h prt_denoise_temporal with a motion plane, in float64 ------------------------------------------------------------------------------

def test_mirror_without_motion_is_temporal_ref():
    """D = None and D = 0 return arrays equal to temporal_ref's, on the synthetic world of tests/cases.py with a moving camera"""
    prt = _pkg()
    world = World(prt)
    cams = [prt.default_camera(W0, H0), prt.orbit_camera(W0, H0, d_yaw=0.04, d_pitch=0.012), prt.orbit_camera(W0, H0, d_yaw=0.10, d_pitch=0.03, d_radius=0.06)]
    prev = None
    for k, cam in enumerate(cams):
        rec, _ = world.records(cam, W0, H0, k)
        fb, g, v_frame = rec[..., 0:4], rec[..., 4:12], rec[..., 12].astype(np.float64)
        hist_prev, g_prev, cam_prev = prev if prev is not None else (None, g, cam)
        want = temporal_ref(fb, g, g_prev, hist_prev, cam, cam_prev, v_frame, **T_DEFAULTS)
        zeros = np.zeros((H0, W0, 4), dtype=f32)
        still = np.zeros((H0, W0, 4), dtype=f32)
        still[..., 3] = 1.0                                               # m > 0 with D = 0 moves nothing either
        for plane in (None, zeros, still):
            got = temporal_ref_motion(fb, g, g_prev, hist_prev, cam, cam_prev, v_frame, motion=plane, **T_DEFAULTS)
            assert set(got) == set(want)
            for key in want:
                assert np.array_equal(got[key], want[key], equal_nan=True), (k, key)
        if k:
            assert want["hist"].mean() > 0.5
        prev = (_mirror_history(want, fb), g, cam)


# ---- the moving card ---------------------------------------------------------------------------------------------------------------------------------

CARD_STEP = (2.0, 0.5)          # pixels per frame along the image's x and y (at the card's distance, W0 x H0 frame)
CARD_TURN = 0.02                # radians per frame about an axis near the card's normal
CARD_WAVE = 7.0                 # pixels per period of the card's pattern
CARD_NOISE = 0.05
CARD_FRAMES = 8
MIN_VALID_SHARE = 0.6           # of the card-interior pixels of the last frame: valid history and margin (the mirror: see the test's docstring)


class MovingWorld(World):
    """World whose card translates by CARD_STEP pixels and turns by CARD_TURN per frame.  The card's colour and albedo are functions of its
    LOCAL coordinates (a, b): the pattern moves with it.  frame(k) also gives the motion plane of the rigid transform between poses k - 1 and
    k -- D = (where the pixel's card point was) - (where it is), m = 1 on the card, zeros elsewhere and in frame 0 -- and the noise-free colour"""

    def __init__(self, prt):
        super().__init__(prt)
        P, M, Hz, Vt = camera_basis(prt.default_camera(W0, H0))
        self.cam = prt.default_camera(W0, H0)
        h, v = _unit(Hz), _unit(Vt)
        Cc, n, u, w, hu, hv = self.surfaces[1]
        self.px = 3.5 * np.linalg.norm(Hz) / ((W0 - 1) / 2.0)            # world units per pixel at the card's distance
        self.card = (Cc - 0.25 * h + 0.1 * v - 7.0 * self.px * h, n, u, w, hu, hv)
        self.h, self.v = h, v
        self.axis = _unit(n + 0.3 * u)

    def pose(self, k):
        Cc, n, u, w, hu, hv = self.card
        ang = k * CARD_TURN
        Ck = Cc + k * self.px * (CARD_STEP[0] * self.h - CARD_STEP[1] * self.v * np.sign(self.v @ np.array([0.0, 1.0, 0.0]) or 1.0))
        return Ck, _rodrigues(n, self.axis, ang), _rodrigues(u, self.axis, ang), _rodrigues(w, self.axis, ang), hu, hv

    def card_colour(self, a, b):
        k = 2 * np.pi / (CARD_WAVE * self.px)
        ph = np.stack([k * (a + 0.3 * b), k * (0.9 * b - 0.4 * a), k * (0.7 * a + 0.7 * b)], -1) + np.array([0.3, 1.7, 2.9])
        return 0.8 + 0.35 * np.sin(ph)

    def card_albedo(self, a, b):
        return 0.5 + 0.2 * np.stack([np.sin(1.5 * a + 0.4), np.cos(1.2 * b), np.sin(a - b)], -1)

    def frame(self, k, W=W0, H=H0, noise=CARD_NOISE):
        """(records [H, W, 16], surface id [H, W]: 0 none, 1 back, 2 card, motion plane [H, W, 4], noise-free colour [H, W, 3]) of frame k"""
        rng = np.random.default_rng(7000 + k)
        cam = self.cam
        P = camera_basis(cam)[0]
        d = centre_dirs(camera_basis(cam), W, H)
        z = np.full((H, W), np.inf)
        nrm, sid = np.zeros((H, W, 3)), np.zeros((H, W), dtype=np.int64)
        for s, (Cc, n, u, w, hu, hv) in enumerate([self.surfaces[0], self.pose(k)]):
            with np.errstate(divide="ignore", invalid="ignore"):
                t = ((Cc - P) @ n) / (d @ n)
            X = P + d * t[..., None]
            hit = (t > 1e-6) & (t < z) & (np.abs((X - Cc) @ u) <= hu) & (np.abs((X - Cc) @ w) <= hv)
            z = np.where(hit, t, z)
            nrm = np.where(hit[..., None], np.where(((d @ n) < 0)[..., None], n, -n), nrm)
            sid = np.where(hit, s + 1, sid)
        cov = sid > 0
        X = np.where(cov[..., None], P + d * np.where(cov, z, 0.0)[..., None], 6.0 * d)
        Ck, n, u, w, _, _ = self.pose(k)
        a, b = (X - Ck) @ u, (X - Ck) @ w
        on_card = (sid == 2)[..., None]
        clean = np.where(on_card, self.card_colour(a, b), self.colour(X))
        rec = np.zeros((H, W, 16), dtype=f32)
        rec[..., 0:3] = clean + rng.uniform(-noise, noise, (H, W, 3))
        rec[..., 3] = rng.uniform(0.0, 1.0, (H, W))
        rec[..., 4:7] = np.where(on_card, self.card_albedo(a, b), self.albedo(X))
        rec[..., 7] = cov
        rec[..., 8:11] = nrm
        rec[..., 11] = np.where(cov, z, 0.0)
        rec[..., 12] = rng.uniform(0.005, 0.1, (H, W))
        rec[..., 13] = 1.0
        plane = np.zeros((H, W, 4), dtype=f32)
        if k > 0:
            Cp, _, up, wp, _, _ = self.pose(k - 1)
            Xp = Cp + a[..., None] * up + b[..., None] * wp
            plane[..., :3] = np.where(on_card, Xp - X, 0.0)
            plane[..., 3] = sid == 2
        return rec, sid, plane, clean


def _card_records(pose):
    """the card of a pose as two triangles in the library's record layout (p0, e1 = p0 - p1, e2 = p2 - p0, n unused): float32 [2, 12]"""
    Cc, n, u, w, hu, hv = pose
    corner = lambda a, b: Cc + a * hu * u + b * hv * w
    out = np.zeros((2, 12), dtype=f32)
    for s, (v0, v1, v2) in enumerate(((corner(-1, -1), corner(1, -1), corner(-1, 1)), (corner(1, 1), corner(-1, 1), corner(1, -1)))):
        out[s, 0:3], out[s, 3:6], out[s, 6:9] = v0, v0 - v1, v2 - v0
    return out


def _card_barycentrics(world, k, rec, sid):
    """(slot, u, v) of every card pixel of frame k in the two triangles of _card_records"""
    Ck, n, u, w, hu, hv = world.pose(k)
    B = camera_basis(world.cam)
    X = B[0] + centre_dirs(B, *sid.shape[::-1]) * rec[..., 11].astype(np.float64)[..., None]
    a, b = ((X - Ck) @ u)[sid == 2], ((X - Ck) @ w)[sid == 2]
    uu, vv = (a + hu) / (2 * hu), (b + hv) / (2 * hv)
    second = uu + vv > 1
    return second.astype(np.uint32), np.where(second, 1 - uu, uu), np.where(second, 1 - vv, vv)


def _interior(sid_now, sid_prev, plane, rec, cam):
    """card pixels of this frame, all four neighbours on the card, whose point's previous position has its 2x2 taps on the previous card"""
    H, W = sid_now.shape
    card = sid_now == 2
    pad = np.pad(card, 1)
    inner = card & pad[:-2, 1:-1] & pad[2:, 1:-1] & pad[1:-1, :-2] & pad[1:-1, 2:]
    B = camera_basis(cam)
    X = B[0] + centre_dirs(B, W, H) * rec[..., 11].astype(np.float64)[..., None] + plane[..., :3]
    xp, yp, ef = project(B, X - B[0], W, H)
    x0, y0 = np.floor(np.where(inner, xp, 0)).astype(np.int64), np.floor(np.where(inner, yp, 0)).astype(np.int64)
    ok = inner & (x0 >= 0) & (y0 >= 0) & (x0 + 1 < W) & (y0 + 1 < H)
    x0, y0 = np.clip(x0, 0, W - 2), np.clip(y0, 0, H - 2)
    pc = sid_prev == 2
    return ok & pc[y0, x0] & pc[y0, x0 + 1] & pc[y0 + 1, x0] & pc[y0 + 1, x0 + 1]


def _call(rc, rec_t, W, H, cam, motion, **kw):
    """prt_denoise_records_temporal_motion through ctypes (device_motion may be None: a null plane through the NEW entry point)"""
    prt = _pkg()
    capi = prt._capi
    p = capi.DenoiseParams(int(kw.get("passes", 5)), 0, 3.0, 128.0, 1.0, 0.1)
    t = capi.TemporalParams(T_DEFAULTS["alpha_color"], T_DEFAULTS["alpha_moments"], T_DEFAULTS["tau_z"], T_DEFAULTS["cos_n"],
                            T_DEFAULTS["history_cap"], capi.PRT_TEMPORAL_FEEDBACK_INTEGRATED)
    out = np.zeros((H, W, 4), dtype=f32)
    rc._chk(rc.lib.prt_denoise_records_temporal_motion(rc.ctx, C.byref(p), C.byref(t), C.byref(cam), W, H, C.c_void_p(rec_t.data_ptr()),
                                                       None if motion is None else C.c_void_p(motion.data_ptr()), None,
                                                       out.ctypes.data_as(C.c_void_p), None), "prt_denoise_records_temporal_motion")
    return out


def run_card(world, mode, rc=None, label=""):
    """the moving-card sequence with the plane (mode "plane"), without (mode "none") or with a plane of zeros ("zeros") through the mirror
    (rc None: its own history, as float32, stands in for the device's) or through context rc, whose history and picture are compared with the
    mirror after every call.  Returns the per-frame list of (mirror dict, history, picture, sid, plane, clean, rec)"""
    W, H, cam = W0, H0, world.cam
    prev, out, worst = None, [], {}
    for k in range(CARD_FRAMES):
        rec, sid, plane, clean = world.frame(k)
        mot = {"plane": plane, "none": None, "zeros": np.zeros_like(plane)}[mode]
        fb, g, v_frame = rec[..., 0:4], rec[..., 4:12], rec[..., 12].astype(np.float64)
        hist_prev, g_prev = prev if prev is not None else (None, g)
        ref = temporal_ref_motion(fb, g, g_prev, hist_prev, cam, cam, v_frame, motion=mot, **T_DEFAULTS)
        pic = None
        if rc is None:
            h = _mirror_history(ref, fb)
        else:
            pic = _call(rc, _to_device(rec), W, H, cam, None if mot is None else _to_device(mot))
            h = rc.read_records_history(W, H)
            m = ref["margin_other"]
            _cmp(label, k, "n", h[..., 3], ref["n"], ref["n"], m, worst)
            _cmp(label, k, "m1", h[..., 4], ref["m1"], ref["m1scale"], m, worst)
            _cmp(label, k, "m2", h[..., 5], ref["m2"], ref["m2scale"], m, worst)
            _cmp(label, k, "c", h[..., :3], ref["ci"], ref["cscale"], m, worst)
            _cmp(label, k, "v", h[..., 6], ref["v"], np.where(ref["n"] >= 4, ref["m2scale"], v_frame.max()), m & ~ref["near4"], worst)
            moment = np.maximum(ref["m2"] - ref["m1"] ** 2, 0.0)
            either = _close(h[..., 6], moment, ref["m2scale"]) | _close(h[..., 6], v_frame, v_frame.max())
            assert either[m & ref["near4"]].all(), (label, k, "v at n = 4")
            assert ((h[..., 3] > 1.0) == ref["hist"])[m].all(), (label, k, "which pixels keep their history")
            fref = denoise_ref(np.concatenate([h[..., :3], fb[..., 3:4]], -1), g, h[..., 6].astype(np.float64), passes=5)
            bound = 1e-4 * np.abs(fref).max()
            worst["picture"] = max(worst.get("picture", 0.0), float(np.abs(pic - fref).max() / bound))
            assert np.abs(pic - fref).max() <= bound, (label, k, "picture")
        out.append((ref, h, pic, sid, plane, clean, rec))
        prev = (h, g)
    if rc is not None:
        print("%s: largest error / bound: %s" % (label, "  ".join("%s %.3g" % kv for kv in sorted(worst.items()))))
    return out


def card_figures(with_plane, without):
    """the three figures of the last frame: (share of the card-interior pixels with valid history and margin, RMS error of the integrated
    colour against the noise-free colour on those pixels with the plane, the same without, share of the frame's pixels left out by margin)"""
    ref, h, _, sid, plane, clean, rec = with_plane[-1]
    ref0, h0 = without[-1][0], without[-1][1]
    interior = _interior(sid, with_plane[-2][3], plane, rec, _pkg().default_camera(W0, H0))
    valid = interior & ref["hist"] & ref["margin_other"] & ref0["margin_other"]
    rms = [float(np.sqrt(((hh[..., :3].astype(np.float64) - clean) ** 2)[valid].mean())) for hh in (h, h0)]
    left_out = max(float((~r[0]["margin_other"]).mean()) for seq in (with_plane, without) for r in seq)
    return valid.sum() / max(interior.sum(), 1), rms[0], rms[1], left_out, int(interior.sum())


@pytest.fixture(scope="module")
def card_mirror():
    world = MovingWorld(_pkg())
    return world, run_card(world, "plane"), run_card(world, "none")


def test_moving_card_on_the_mirror(card_mirror, emu):
    """The card moves by (2, 0.5) pixels and turns by 0.02 rad per frame; its pattern has 7 pixels per period; colour noise +-0.05; 8 frames,
    default temporal parameters, the mirror standing in for the device.  Without the plane the reprojection looks at the same screen position
    of the previous frame, where the card showed another part of its pattern: the depth and normal tests pass and the history ghosts.
    The mirror's figures (recorded from this test's output): 86 card-interior pixels, 100 % of them with valid history and margin (required:
    60 %); RMS error of the integrated colour 0.041 with the plane (the colour noise averaged down, and the pattern softened by eight bilinear
    resamplings), 0.209 without: ratio 0.196 (required here: at most 0.25; of the device: at most 0.5); 0.0 % of the pixels left out by
    margin (cap 10 %)."""
    world, with_plane, without = card_mirror
    share, rms_with, rms_without, left_out, n_int = card_figures(with_plane, without)
    print("moving card (mirror): %d interior pixels, valid share %.3f, rms with %.4f without %.4f ratio %.3f, left out by margin %.3f"
          % (n_int, share, rms_with, rms_without, rms_with / rms_without, left_out))
    for k in range(1, CARD_FRAMES):                                   # a few pixels per frame
        _, _, _, sid, plane, _, _ = with_plane[k]
        step = np.linalg.norm(plane[..., :3][sid == 2], axis=-1) / world.px
        assert 1.5 <= step.min() and step.max() <= 4.0, (k, step.min(), step.max())
        assert (plane[..., 3] == (sid == 2)).all() and (plane[..., :3][sid != 2] == 0).all()
        # the rigid transform's plane is what the library's body makes of the card as two triangles, before and after the move
        slot, u, v = _card_barycentrics(world, k, with_plane[k][6], sid)
        d = emu.displacement(_card_records(world.pose(k - 1)), _card_records(world.pose(k)), slot, np.stack([u, v], -1))
        assert np.abs(d - plane[..., :3][sid == 2]).max() <= 2e-5, k
    assert n_int >= 40, n_int
    assert share >= MIN_VALID_SHARE, share
    assert rms_with <= 0.25 * rms_without, (rms_with, rms_without)
    assert left_out <= 0.10, left_out
    # the plane is what keeps the history: without it the same pixels still pass the depth and normal tests (they ghost, they do not restart)
    ref0 = without[-1][0]
    interior = _interior(with_plane[-1][3], with_plane[-2][3], with_plane[-1][4], with_plane[-1][6], world.cam)
    assert ref0["hist"][interior].mean() > 0.8


# ---- the 20-float tile of parallel.denoise_on_rank0(motion=True) over gloo ---------------------------------------------------------------------------

TILE_W, TILE_H = 7, 41
POISON = 0xDEADBEEF


def _tile_frame():
    words = np.random.default_rng(TILE_H).integers(0, 2 ** 32, (TILE_H, TILE_W, 20), dtype=np.uint32)
    words[words == POISON] = 0
    for k, s in enumerate((0x80000000, 0x7FC12345, 0xFFC00ABC, 0x00000001, 0x807FFFFF)):      # -0.0, NaNs with a payload, denormals
        words[:, k % TILE_W, (3 * k) % 16] = s
        words[:, (k + 2) % TILE_W, 16 + k % 4] = s
    return words


def _tile_worker(rank, world, port, out_path):
    import torch
    import torch.distributed as dist
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    par = importlib.import_module(PKG_NAME + ".parallel")
    rows = par.rows_of_rank(TILE_H, world, rank)
    padded = np.full((par.max_rows_per_rank(TILE_H, world), TILE_W, 20), POISON, dtype=np.uint32)
    padded[:len(rows)] = _tile_frame()[rows]
    t = torch.from_numpy(padded.view(np.float32))
    tile = par.pack_motion_tile(t[..., :16].contiguous(), t[..., 16:].contiguous())
    assert tile.shape == (padded.shape[0], TILE_W, 20) and tile.is_contiguous()
    full = par.gather_rows_on_rank0(tile, TILE_H, TILE_W, world, dist)
    dist.barrier()
    if rank == 0:
        rec, mot = par.split_motion_tile(full)
        assert rec.is_contiguous() and mot.is_contiguous() and rec.shape == (TILE_H, TILE_W, 16) and mot.shape == (TILE_H, TILE_W, 4)
        np.save(out_path, np.concatenate([rec.numpy().view(np.uint32), mot.numpy().view(np.uint32)], -1))
    dist.destroy_process_group()


def test_motion_tile_travels_unchanged(tmp_path):
    import torch.multiprocessing as mp
    out = str(tmp_path / "tile.npy")
    mp.spawn(_tile_worker, args=(2, 33500 + (os.getpid() % 2000), out), nprocs=2, join=True)
    got = np.load(out)
    assert not (got == POISON).any() and np.array_equal(got, _tile_frame())


# ---- on the GPU: synthetic records ---------------------------------------------------------------------------------------------------------------------

def _rec_ctx(prt):
    return prt.Renderer(prt.HostScene("cornell_coat.json").config(), device=0)              # no scene, no camera, no frame


@pytest.mark.gpu
def test_moving_card_on_the_device(prt, card_mirror):
    """the sequence through prt_denoise_records_temporal_motion: every call equals the mirror (fed with the device's own history); a null plane
    and a plane of zeros equal prt_denoise_records_temporal bit for bit; the plane halves the error on the device's output too"""
    world = card_mirror[0]
    ctx = [_rec_ctx(prt) for _ in range(4)]
    with_plane = run_card(world, "plane", rc=ctx[0], label="card, plane")
    without = run_card(world, "none", rc=ctx[1], label="card, null plane")
    zeros = run_card(world, "zeros", rc=ctx[2], label="card, zeros")
    for k in range(CARD_FRAMES):
        rec = with_plane[k][6]
        old = ctx[3].denoise_records_temporal(_to_device(rec), W0, H0, world.cam, feedback="integrated")
        h_old = ctx[3].read_records_history(W0, H0)
        for other in (without, zeros):
            assert (_bits(other[k][2]) == _bits(old)).all() and (_bits(other[k][1]) == _bits(h_old)).all(), k
    share, rms_with, rms_without, left_out, n_int = card_figures(with_plane, without)
    print("moving card (device): %d interior pixels, valid share %.3f, rms with %.4f without %.4f ratio %.3f, left out by margin %.3f"
          % (n_int, share, rms_with, rms_without, rms_with / rms_without, left_out))
    assert share >= MIN_VALID_SHARE and left_out <= 0.10
    assert rms_with <= 0.5 * rms_without, (rms_with, rms_without)
    for r in ctx:
        r.close()


@pytest.mark.gpu
@pytest.mark.parametrize("W,H", [(37, 1), (1, 1)])
def test_one_row_and_one_pixel_with_a_plane(prt, W, H):
    """Frames of one row and of one pixel.  The moving-card world cannot be shown at these sizes: create_cam_ray's sy = (H-1-y) / (H-1) is
    0 / 0 for H = 1 (and sx for W = 1), so the card's camera has no rays, and temporal_ref_motion has no margin anywhere (its dot(e, f) is
    NaN: prt.h's "no history when dot(e, f) <= 0" is not decided by a number).  What the sizes can show is what the kernel does with a
    plane when there is no projection: records with O(1) colours and depths and a plane with m = 1 and displacements of 0.3 on every
    pixel must give the bits of the call without a plane -- no history, n = 1 -- and stay finite; the frame is narrower than the 16 x 16
    workgroup in one or both directions."""
    a, b = _rec_ctx(prt), _rec_ctx(prt)
    cam = prt.default_camera(W, H)
    for k in range(2):
        rec = _plain_records(W, H, 300 + k)
        plane = np.random.default_rng(k).normal(0, 0.3, (H, W, 4)).astype(f32)
        plane[..., 3] = 1.0
        got = _call(a, _to_device(rec), W, H, cam, _to_device(plane))
        want = b.denoise_records_temporal(_to_device(rec), W, H, cam, feedback="integrated")
        assert (_bits(got) == _bits(want)).all() and np.isfinite(got).all(), k
        h = a.read_records_history(W, H)
        assert (_bits(h) == _bits(b.read_records_history(W, H))).all() and (h[..., 3] == 1.0).all(), k
    a.close()
    b.close()


# ---- on the GPU: the motion plane of rendered scenes ---------------------------------------------------------------------------------------------------

MIN_BEHIND_MIRROR = 20          # pixels of cornell_mixed (the camera of test_only_direct_mesh_hits_move) that see the mesh in the mirror sphere


def _zero_plane(plane):
    return (_bits(plane) == 0).all()


@pytest.mark.gpu
def test_motion_plane_matches_the_caster(prt):
    sc = Rendered(prt, "cornell_coat.json")
    r = sc.context(prt)
    r.update_vertices(sc.vB, sc.nB)
    r.render_guides(1)
    plane = r.read_motion()
    r.close()
    worst = sc.check(plane, "coat, one update")
    moving = (plane[..., 3] > 0) & (np.linalg.norm(plane[..., :3], axis=-1) > 0)
    print("motion plane, cornell_coat %dx%d: largest |D - caster| over the matching pixels %.3e (bound %.3e, cap %.3e); %.1f %% of the pixels move"
          % (RW, RH, worst, D_BOUND, 1e-3 * sc.diag, 100 * moving.mean()))
    assert D_BOUND <= 1e-3 * sc.diag
    assert moving.mean() >= 0.05
    assert worst <= D_BOUND, worst


@pytest.mark.gpu
def test_only_direct_mesh_hits_move(prt):
    """cornell_mixed, one update: m = 0 and D = 0 on every pixel whose caster hit is a sphere, a quad, a miss or lies behind a delta chain"""
    sc = Rendered(prt, "cornell_mixed.json", d_radius=-0.4)            # (closer: the mirror sphere shows more of the teapot)
    r = sc.context(prt)
    r.update_vertices(sc.vB, sc.nB)
    r.render_guides(1)
    plane = r.read_motion()
    g = r.read_guides()
    r.close()
    worst = sc.check(plane, "mixed, one update")                      # (within 1e-3 of the diagonal on all but 0.5 % of the pixels)
    print("motion plane, cornell_mixed %dx%d: largest |D - caster| over the matching pixels %.3e" % (RW, RH, worst))
    other = ~sc.mesh
    agree = other & ((g[..., 3] > 0) == sc.hit)                        # (silhouette pixels where device and caster see different things aside)
    assert (~sc.hit).sum() + (sc.hit & (sc.mid >= 0)).sum() >= 100 and agree.sum() >= 0.99 * other.sum()
    bad = other & (_bits(plane) != 0).any(-1)
    assert bad.mean() <= 0.005, bad.sum()
    assert (_bits(plane[~sc.hit & (g[..., 3] == 0)]) == 0).all()       # misses
    # the mesh behind a delta chain: pixels on the mirror sphere whose reflection shows the teapot.  The guides' first non-delta hit there
    # IS a mesh triangle; it carries no motion because a delta event came before it
    behind = sc.behind_mirror
    moved = behind & (_bits(plane) != 0).any(-1)
    print("cornell_mixed: %d pixels see the mesh in the mirror sphere, %d of them carry motion" % (behind.sum(), moved.sum()))
    assert behind.sum() >= MIN_BEHIND_MIRROR, behind.sum()
    assert moved.sum() <= 0.1 * behind.sum(), (moved.sum(), behind.sum())          # (the sphere's silhouette aside)


@pytest.mark.gpu
def test_snapshot_rule(prt):
    sc = Rendered(prt, "cornell_coat.json")
    # two updates A then B between guide renders: the displacement from the geometry before A to B
    r = sc.context(prt)
    r.update_vertices(sc.vA, sc.nA)
    r.update_vertices(sc.vB, sc.nB)
    r.render_guides(1)
    first = r.read_motion()
    assert sc.check(first, "A then B") <= D_BOUND
    # a second render_guides without an update: all zeros, and denoise_temporal gives the bits of a motion-off context run in step
    off = sc.context(prt, motion=False)
    off.update_vertices(sc.vA, sc.nA)
    off.update_vertices(sc.vB, sc.nB)
    seeds = prt.seed_pairs(2 * max(sc.cfg.max_bounces, 8) + 64)
    for k in range(2):
        outs = []
        for q in (r, off):
            q.reset()
            q.render_spp(2, seeds)
            q.render_guides(1)
            outs.append(q.denoise_temporal())
        assert _zero_plane(r.read_motion()), k
        assert (_bits(outs[0]) == _bits(outs[1])).all() and (_bits(r.read_history()) == _bits(off.read_history())).all(), k
    off.close()
    # a refused update (a NaN vertex) leaves the pending snapshot and the next plane as if it had not been called
    r.update_vertices(sc.v0, sc.n0)
    r.render_guides(1)                                                  # (geometry: the uploaded one again; snapshot consumed)
    r.update_vertices(sc.vB, sc.nB)
    bad = np.array(sc.vA)
    bad[len(bad) // 2, 1] = np.nan
    with pytest.raises(prt.PrtError) as e:
        r.update_vertices(bad, sc.nA)
    assert e.value.code == prt.PRT_ERR_INVALID_ARGUMENT
    r.render_guides(1)
    again = r.read_motion()
    assert sc.check(again, "B, then a refused update") <= D_BOUND
    assert (_bits(again) == _bits(first)).all()
    # a refused update with no snapshot pending takes none
    with pytest.raises(prt.PrtError):
        r.update_vertices(bad, sc.nA)
    r.render_guides(1)
    assert _zero_plane(r.read_motion())
    # upload_scene clears a pending snapshot
    r.update_vertices(sc.vA, sc.nA)
    r.upload_scene(sc.scene)
    r.render_guides(1)
    assert _zero_plane(r.read_motion())
    # ... and so does turning motion off and on again
    r.update_vertices(sc.vB, sc.nB)
    r.set_motion(False)
    r.set_motion(True)
    r.render_guides(1)
    assert _zero_plane(r.read_motion())
    r.close()


# ---- on the GPU: plumbing ------------------------------------------------------------------------------------------------------------------------------

def _torch_zeros(shape, fill=7.0):
    import torch
    t = torch.full(shape, fill, dtype=torch.float32, device="cuda:0")
    torch.cuda.synchronize()
    return t


@pytest.mark.gpu
def test_guides_and_splits(prt):
    """the eight guide floats are the same bits with motion on and off; the plane of a whole-frame context equals the union of a tile split and
    of a 2-part row-block split at 16 rows, and export_motion equals read_motion"""
    par = importlib.import_module(PKG_NAME + ".parallel")
    sc = Rendered(prt, "cornell_mixed.json")
    planes, guides = {}, {}
    for key, motion, part in (("on", True, None), ("off", False, None), ("t0", True, ("tile", 0, 20)), ("t1", True, ("tile", 20, RH - 20)),
                              ("b0", True, ("blocks", 0)), ("b1", True, ("blocks", 1))):
        r = sc.context(prt, motion=motion, part=part)
        r.update_vertices(sc.vB, sc.nB)
        r.render_guides(4)
        guides[key] = r.read_guides()
        if motion:
            planes[key] = r.read_motion()
            t = _torch_zeros((r.rows + 1, RW, 4))
            r.export_motion(t)
            r.synchronize()
            got = t.cpu().numpy()
            assert (_bits(got[:r.rows]) == _bits(planes[key])).all() and (got[r.rows:] == 7.0).all(), key
        r.close()
    assert (_bits(guides["on"]) == _bits(guides["off"])).all()
    whole = planes["on"]
    assert ((whole[..., 3] > 0) & (whole[..., 3] < 1)).any(), "K = 4: pixels partly on the mesh"
    assert (_bits(np.concatenate([planes["t0"], planes["t1"]], 0)) == _bits(whole)).all()
    union = np.zeros_like(whole)
    for p in (0, 1):
        union[par.rows_of_rank(RH, 2, p)] = planes["b%d" % p]
    assert (_bits(union) == _bits(whole)).all()


def _split_union(prt, sc, **kw):
    """the plane of a tile split of the frame, put together"""
    parts = []
    for row0, rows in ((0, 20), (20, RH - 20)):
        r = sc.context(prt, part=("tile", row0, rows), **kw)
        r.update_vertices(sc.vB, sc.nB)
        r.render_guides(4)
        parts.append(r.read_motion())
        r.close()
    return np.concatenate(parts, 0)


@pytest.mark.gpu
def test_sdf_instance(prt):
    """guide_motion_kernel<SDF> (cornell_sdf: the teapot among raymarched primitives): the guides are the plain SDF instance's bits; where a
    pixel carries motion the caster -- which knows no SDF primitives -- sees the mesh too and agrees on D; where the caster sees the mesh
    and the pixel carries none, an SDF primitive is in front (the guides' depth is shorter); the plane of a tile split is the whole frame's"""
    sc = Rendered(prt, "cornell_sdf.json")
    assert sc.cfg.geom_flags & 4, "PRT_GEOM_SDF: the SDF instances are the ones that run"
    on, off = sc.context(prt), sc.context(prt, motion=False)
    out = {}
    for K in (1, 4):
        for key, r in (("on", on), ("off", off)):
            r.update_vertices(sc.v0, sc.n0)
            r.render_guides(1)                                          # (the uploaded geometry; a pending snapshot consumed)
            r.update_vertices(sc.vB, sc.nB)
            r.render_guides(K)
            out[key, K] = r.read_guides()
        assert (_bits(out["on", K]) == _bits(out["off", K])).all(), K
        out["plane", K] = on.read_motion()
    on.close()
    off.close()
    plane, g = out["plane", 1], out["on", 1]
    m, D = plane[..., 3], plane[..., :3].astype(np.float64)
    assert ((m == 0) | (m == 1)).all() and (_bits(plane[m == 0]) == 0).all()
    dev = np.abs(D - sc.D).max(-1)
    moving = m > 0
    good = moving & sc.mesh & (dev <= 1e-3 * sc.diag)
    hidden = sc.mesh & ~moving
    in_front = hidden & (g[..., 3] > 0) & (g[..., 7] < sc.t * (1 - 1e-4))
    print("cornell_sdf: %d pixels carry motion (largest |D - caster| %.3e), %d mesh pixels of the caster are hidden by SDF primitives"
          % (moving.sum(), dev[good].max(), hidden.sum()))
    assert moving.sum() >= 100
    assert (moving & ~good).mean() <= 0.005 and (hidden & ~in_front).mean() <= 0.005
    assert dev[good].max() <= D_BOUND
    whole = out["plane", 4]
    assert ((whole[..., 3] > 0) & (whole[..., 3] < 1)).any()
    assert (_bits(_split_union(prt, sc)) == _bits(whole)).all()


@pytest.mark.gpu
def test_pixel_filter_instance(prt):
    """filtered_guides_motion_kernel: under a box filter of radius 0.5 the guide samples are the unfiltered ones (prt.h), so guides AND plane
    are the plain motion instance's bit for bit; under a tent filter the guides are the filtered plain instance's bits, the plane of a
    tile split is the whole frame's, and K = 1 (every filter's centre ray) gives the unfiltered K = 1 plane"""
    sc = Rendered(prt, "cornell_coat.json")
    got = {}
    for key, kw in (("plain", dict()), ("box", dict(pixel_filter=("box", 0.5))), ("tent", dict(pixel_filter=("tent", None))),
                    ("tent off", dict(pixel_filter=("tent", None), motion=False))):
        r = sc.context(prt, **kw)
        for K in (1, 4):
            r.update_vertices(sc.v0, sc.n0)
            r.render_guides(1)
            r.update_vertices(sc.vB, sc.nB)
            r.render_guides(K)
            got[key, K] = (r.read_guides(), r.read_motion() if kw.get("motion", True) else None)
        if key != "plain":
            r.reset()
            r.render_frames(prt.seed_pairs(2))
            assert "filter=" in r.kernel_variant(), r.kernel_variant()  # (the context does run the filter builds)
        r.close()
    for K in (1, 4):
        assert (_bits(got["box", K][0]) == _bits(got["plain", K][0])).all() and (_bits(got["box", K][1]) == _bits(got["plain", K][1])).all(), K
        assert (_bits(got["tent", K][0]) == _bits(got["tent off", K][0])).all(), K
    assert (_bits(got["tent", 1][1]) == _bits(got["plain", 1][1])).all()
    assert sc.check(got["tent", 1][1], "tent, K = 1") <= D_BOUND
    tent, plain = got["tent", 4][1], got["plain", 4][1]
    assert (_bits(tent) != _bits(plain)).any(), "a tent filter of radius 1 moves the guide samples"
    assert (np.abs(tent[..., :3] - plain[..., :3]).max(-1)[(tent[..., 3] == 1) & (plain[..., 3] == 1)] <= 0.05 * sc.diag).all()
    assert (_bits(_split_union(prt, sc, pixel_filter=("tent", None))) == _bits(tent)).all()


def _display_frame(prt, sc, r, k, seeds, update):
    if update is not None:
        r.update_vertices(*update)
    r.reset()
    r.render_spp(2, seeds)
    r.render_guides(2)


@pytest.mark.gpu
def test_context_plane_equals_the_records_call_and_motion_off_is_the_parent(prt):
    """3 displayed frames (no update, A, B).  prt_denoise_temporal with motion on equals prt_denoise_records_temporal_motion fed with the
    exported records and motion, and parallel.denoise_on_rank0(motion=True) on one rank, bit for bit; a context whose motion was turned on and
    off again gives the bits of one that never had it"""
    import torch
    par = importlib.import_module(PKG_NAME + ".parallel")
    sc = Rendered(prt, "cornell_coat.json")
    on, never, toggled = sc.context(prt), sc.context(prt, motion=False), sc.context(prt)
    toggled.set_motion(False)
    rec_ctx = _rec_ctx(prt)
    seeds = prt.seed_pairs(2 * max(sc.cfg.max_bounces, 8) + 64)
    differs = False
    for k, update in enumerate((None, (sc.vA, sc.nA), (sc.vB, sc.nB))):
        for r in (on, never, toggled):
            _display_frame(prt, sc, r, k, seeds, update)
        rec, mot = _torch_zeros((RH, RW, 16)), _torch_zeros((RH, RW, 4))
        on.export_denoise_inputs(rec)
        on.export_motion(mot)
        via_rank0 = par.denoise_on_rank0(on, RH, RW, 1, None, cam=sc.cam, temporal=True, motion=True)
        torch.cuda.synchronize()
        want = on.denoise_temporal()
        got = rec_ctx.denoise_records_temporal(rec, RW, RH, sc.cam, motion=mot)
        assert (_bits(got) == _bits(want)).all(), k
        assert (_bits(via_rank0.cpu().numpy()) == _bits(want)).all(), k
        assert (_bits(rec_ctx.read_records_history(RW, RH)) == _bits(on.read_history())).all(), k
        a, b = never.denoise_temporal(), toggled.denoise_temporal()
        assert (_bits(a) == _bits(b)).all() and (_bits(never.read_history()) == _bits(toggled.read_history())).all(), k
        assert (_bits(never.read_guides()) == _bits(toggled.read_guides())).all() and (_bits(never.read_framebuffer()) == _bits(toggled.read_framebuffer())).all(), k
        differs |= bool((_bits(a) != _bits(want)).any())
    assert differs, "the plane changes the picture of a deforming mesh"
    for r in (on, never, toggled, rec_ctx):
        r.close()


@pytest.mark.gpu
def test_refusals_and_read_only(prt):
    sc = Rendered(prt, "cornell_coat.json")

    def code(fn, *a, **k):
        with pytest.raises(prt.PrtError) as e:
            fn(*a, **k)
        return e.value.code

    r = sc.context(prt, motion=False)
    t = _torch_zeros((RH, RW, 4))
    r.render_guides(1)
    assert code(r.read_motion) == prt.PRT_ERR_NOT_READY and code(r.export_motion, t) == prt.PRT_ERR_NOT_READY          # motion off
    r.set_motion(True)
    assert code(r.read_guides) == prt.PRT_ERR_NOT_READY, "prt_set_motion makes the guides stale"
    assert code(r.read_motion) == prt.PRT_ERR_NOT_READY and code(r.export_motion, t) == prt.PRT_ERR_NOT_READY          # no valid guides
    assert r.lib.prt_read_motion(r.ctx, None) == prt.PRT_ERR_INVALID_ARGUMENT
    assert r.lib.prt_export_motion(r.ctx, None) == prt.PRT_ERR_INVALID_ARGUMENT
    assert r.lib.prt_set_motion(None, 1) == prt.PRT_ERR_INVALID_ARGUMENT
    r.update_vertices(sc.vB, sc.nB)
    r.reset()
    r.render_adaptive(prt.seed_pairs(4 * max(sc.cfg.max_bounces, 8) + 64), 2, 4, 0.0)
    r.render_guides(2)
    assert r.lib.prt_export_motion(r.ctx, C.c_void_p(t.data_ptr() + 4)) == prt.PRT_ERR_INVALID_ARGUMENT                # misaligned
    r.set_camera(sc.cam)
    assert code(r.read_motion) == prt.PRT_ERR_NOT_READY                                                                # stale with the guides
    r.render_guides(2)
    before = (r.read_framebuffer(), r.read_state(), r.read_adaptive_stats(), r.read_guides(), r.read_motion())
    rec = _torch_zeros((RH, RW, 16))
    r.export_denoise_inputs(rec)
    r.export_motion(t)
    r.read_motion()
    r.denoise_records_temporal(rec, RW, RH, sc.cam, motion=t)
    assert r.lib.prt_denoise_records_temporal_motion(r.ctx, None, None, C.byref(sc.cam), RW, RH, C.c_void_p(rec.data_ptr()),
                                                     C.c_void_p(t.data_ptr() + 4), None, None, None) == prt.PRT_ERR_INVALID_ARGUMENT
    assert r.lib.prt_denoise_records_temporal_motion(r.ctx, None, None, None, RW, RH, C.c_void_p(rec.data_ptr()), C.c_void_p(t.data_ptr()),
                                                     None, None, None) == prt.PRT_ERR_INVALID_ARGUMENT
    assert r.lib.prt_denoise_records_temporal_motion(r.ctx, None, None, C.byref(sc.cam), RW, RH, None, C.c_void_p(t.data_ptr()),
                                                     None, None, None) == prt.PRT_ERR_INVALID_ARGUMENT
    after = (r.read_framebuffer(), r.read_state(), r.read_adaptive_stats(), r.read_guides(), r.read_motion())
    for a, b in zip(before, after):
        assert a.tobytes() == b.tobytes()
    r.close()
    # a debug view: unsupported; a scene without triangles: accepted, zeros
    view_cfg = sc.scene.config()
    view_cfg.view_option = 1
    v = prt.Renderer(view_cfg, device=0)
    assert code(v.set_motion, True) == prt.PRT_ERR_UNSUPPORTED
    v.set_motion(False)
    v.close()
    # a scene without triangles (the spheres and quads of cornell_diffuse, its mesh taken out of the desc): accepted, zeros
    host = prt.HostScene("cornell_diffuse.json")
    desc = prt.SceneDesc.from_buffer_copy(bytes(host.desc))
    desc.triangle_count, desc.bvh_node_count = 0, 0
    desc.vertices = desc.normals = desc.primitive_indices = desc.bvh_nodes = None
    e = prt.Renderer(host.config(), device=0)
    e.upload_scene(desc)
    e.set_camera(sc.cam)
    e.resize(RW, RH)
    e.set_motion(True)
    assert code(e.update_vertices, sc.vB, sc.nB) == prt.PRT_ERR_NOT_READY
    seeds = prt.seed_pairs(2 * max(sc.cfg.max_bounces, 8) + 64)
    for k in range(2):
        e.reset()
        e.render_spp(2, seeds)
        e.render_guides(2)
        assert _zero_plane(e.read_motion()), k
        assert (e.read_guides()[..., 3] > 0).mean() > 0.5
        assert np.isfinite(e.denoise_temporal()).all()
    assert (np.abs(e.read_history()[..., 3] - 2.0) < 1e-3).mean() > 0.5
    e.close()
