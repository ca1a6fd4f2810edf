"""The denoiser's two routes over one frame, word for word: the context's own frame (prt_denoise, prt_denoise_temporal) against the same frame
as records (prt_export_denoise_inputs, then prt_denoise_records / prt_denoise_records_temporal on a context without a scene).  A 24x17 frame
is ragged against the filter's 16x16 workgroups in both directions; passes 1 and 2 end on either of the two ping-pong planes; the variance
comes from the stats plane and from the 5x5 moments; the temporal calls run twice on a moving camera, so the second reads a history, with
feedback "atrous" and once with the temporal response on.  The histories and the response planes of both routes are compared as well."""
import pytest

from cases import denoise_setup as _setup, _export
from support import bits as _bits

W, H = 24, 17                           # 2 x 2 workgroups of 16 x 16: the last column of them has 8 live columns, the last row 1 live row
SPP, GUIDE_K, CALLS = 2, 1, 2


@pytest.fixture(scope="module")
def routes(prt):
    """(the frame route's context, the records route's: no scene, camera or frame, render(k): frame k of an orbit in the first one -- the
    camera and the records of its frame)"""
    scene, cfg, cam0, rw = _setup(prt, "cornell_diffuse.json", W, H, pinhole=False)
    rc = prt.Renderer(cfg, device=0)
    n = SPP * 64 + 64

    def render(k):
        cam = prt.orbit_camera(W, H, d_yaw=0.02 * k) if k else prt.default_camera(W, H)
        rw.set_camera(cam)
        rw.reset()
        rw.render_adaptive(prt.seed_pairs(n, first_frame=1 + k * n), SPP, SPP, 0.0)      # "SPP spp", and the stats plane with it
        rw.render_guides(GUIDE_K)
        return cam, _export(rw)
    yield rw, rc, render
    rw.close()
    rc.close()


@pytest.mark.gpu
@pytest.mark.parametrize("source", ["stats", "spatial"])
def test_spatial_routes_agree(routes, source):
    rw, rc, render = routes
    cam, records = render(0)
    fb = rw.read_framebuffer()
    out = {}
    for passes in (1, 2):
        want = rw.denoise(passes=passes, var_source=source)
        got = rc.denoise_records(records, W, H, passes=passes, var_source=source)
        assert (_bits(got) == _bits(want)).all(), passes
        assert (_bits(want[..., 0:3]) != _bits(fb[..., 0:3])).any() and (_bits(want[..., 3]) == _bits(fb[..., 3])).all(), passes
        out[passes] = want
    assert (_bits(out[1]) != _bits(out[2])).any()


@pytest.mark.gpu
@pytest.mark.parametrize("source,passes,response", [("stats", 1, False), ("stats", 2, False), ("spatial", 1, False), ("spatial", 2, False),
                                                    ("stats", 2, True)])
def test_temporal_routes_agree(routes, source, passes, response):
    rw, rc, render = routes
    for r in (rw, rc):
        if response:
            r.set_temporal_response(4, 1, 2.0)
        else:
            r.set_temporal_response(None)
    rw.reset_history()
    rc.reset_records_history()
    kw = dict(passes=passes, var_source=source, feedback="atrous")
    try:
        for k in range(CALLS):
            cam, records = render(k)
            want = rw.denoise_temporal(**kw)
            got = rc.denoise_records_temporal(records, W, H, cam, **kw)
            assert (_bits(got) == _bits(want)).all(), k
            hist = rw.read_history()
            assert (_bits(rc.read_records_history(W, H)) == _bits(hist)).all(), k
            assert (hist[..., 3] > 1.0).any() == (k > 0), k                 # n of {c, n}: only the second call found a history to continue
            if response:
                resp = rw.read_response()
                assert (_bits(rc.read_records_response(W, H)) == _bits(resp)).all(), k
                assert (resp[..., 3] >= 1.0).any() == (k > 0), k            # the flag: history kept (1) or clamped (2)
    finally:
        for r in (rw, rc):
            r.set_temporal_response(None)
