"""The pixel-filter builds of the render kernel (PT_MATS_FILTER, pt_inst_filter_*.hip; prt_set_pixel_filter) held to the CPU oracle, bit for bit.

The filter path draws nothing from the RNG: a filtered render is the reference's algorithm with another image-plane point per path.  The oracle
(oracle/pt_oracle.c) takes those points as a table of per-path offsets {dx, dy} from OUTSIDE -- it knows neither the warps nor the hash -- and
applies the "Camera ray" sentence of include/prt.h.  The tables fed to it here:
  * box and tent: the numpy mirror of tests/mirrors.py (bit-exact with the host function for these kinds);
  * Gaussian and Blackman-Harris: on the host emulator the mirror's own table(kind, r), handed to both sides; on the GPU
    prt.pixel_filter_offsets (the product's table is internal; the host function is held to the mirror within 2 ulp and to the device bit for
    bit by test_pixel_filter.py).
No tolerance anywhere: equality of bits, path state (oracle.state_fields_equal) and image (oracle.images_equal).

Without a GPU: tests/emu (pt_device.h compiled for the host) against the oracle -- every filter set, kinds and radii, frames / "N spp" / resumed
runs, ragged frames, row tiles and row blocks (global pixel coordinates), schedules.  With one (-m gpu): the same through the C ABI -- the seven
rows of mirrors.SETS in frames, "N spp" and adaptive mode, the 5- and 6-wave builds under both pixel mappings, the ordered build, the
live-pixel-list launches, compiled set == generic dispatch, splits, checkpoints, walk_min_lanes -- and the filtered guides' coverage at K = 16
against a float64 caster.

Left out, and why: nothing of the issue's list.  The ordered ("expensive first") build only runs through trees of more than 64 k node pairs, so
its case renders a strip of the 871 k-triangle stand-in (as test_adaptive.py does for the big tree), not a Cornell box."""
import os

import numpy as np
import pytest

from conftest import GOLDEN
from cases import filter_setup as _setup, _quad_scene
from mirrors import camera_basis, DEFAULT_R, KINDS, offsets_ref, sample_u, SETS, table, warp
from support import assert_same_render as _same, variant_case


TABLE_KINDS = ("gaussian", "blackman-harris")


# ---- the offsets handed to the oracle ------------------------------------------------------------------------------------------------------------

def mirror_offsets(kind, r, W, H, K, T=None):
    """float32 (H, W, K, 2): offsets_ref of tests/mirrors.py for every pixel of a W x H frame, paths 0 .. K-1 (the same functions, whole
    arrays at a time).  T: the 257-entry table of the table kinds (default: the mirror's own)"""
    gy = np.arange(H, dtype=np.uint32)[:, None, None]
    gx = np.arange(W, dtype=np.uint32)[None, :, None]
    k = np.arange(K, dtype=np.uint32)[None, None, :]
    u, v = sample_u(gx, gy, k)
    if T is None and kind in TABLE_KINDS:
        T = table(kind, r)
    return np.ascontiguousarray(np.stack([warp(kind, r, u, T), warp(kind, r, v, T)], -1), dtype=np.float32)


def host_offsets(prt, kind, r, W, H, K, rows=None):
    """float32 (H, W, K, 2) from prt_pixel_filter_offsets (rows: only these global rows are filled)"""
    out = np.zeros((H, W, K, 2), dtype=np.float32)
    for gy in (range(H) if rows is None else rows):
        for gx in range(W):
            out[gy, gx] = prt.pixel_filter_offsets(kind, r, gx, gy, 0, K)
    return out


def gpu_offsets(prt, kind, r, W, H, K, rows=None):
    if kind in TABLE_KINDS:
        return host_offsets(prt, kind, r, W, H, K, rows)
    return mirror_offsets(kind, r, W, H, K)


def test_the_whole_frame_mirror_is_offsets_ref():
    """mirror_offsets is offsets_ref pixel by pixel (bits), so what holds for one holds for the other"""
    for kind in KINDS:
        tab = mirror_offsets(kind, DEFAULT_R[kind], 7, 5, 9)
        for gx, gy in ((0, 0), (6, 4), (3, 2)):
            assert (tab[gy, gx].view(np.uint32) == offsets_ref(kind, DEFAULT_R[kind], gx, gy, 0, 9).view(np.uint32)).all(), (kind, gx, gy)


# ---- the emulator against the oracle (no GPU) ----------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def emu():
    import emu_api
    emu_api.lib()
    return emu_api


# the sets launch_render has filter builds of: (variant, PT_EMU_GENERIC, what)
EMU_SETS = [("cornell_diffuse", False, "LIGHT|DIFF"), ("cornell_media", False, "LIGHT|DIFF,medium"), ("cornell_coat", False, "COAT"),
            ("cornell_roughcond", False, "ROUGH_COND"), ("cornell_roughdiel", False, "ROUGH_DIEL"), ("cornell_mixed", False, "generic"),
            ("cornell_media_hg", True, "generic,medium"), ("cornell_diffuse", True, "generic, forced")]
# the four kinds at their default radius, an off-default radius, and the maximum (offsets reach four pixels outside the frame at its borders)
FILTERS = [("box", 0.5), ("tent", 1.0), ("gaussian", 1.5), ("blackman-harris", 2.0), ("gaussian", 0.3), ("tent", 4.0), ("blackman-harris", 4.0)]


def _scene(prt, variant, W, H, pinhole=False):
    scene, cfg, cam, env = variant_case(prt, variant, W, H)
    if pinhole:
        cam.apertureRadius = 0.0
    return scene, cfg, cam, env


def _emu_filter(kind, r):
    T = table(kind, r) if kind in TABLE_KINDS else None
    return (KINDS[kind], r, T), T


@pytest.mark.parametrize("kind,r", FILTERS)
@pytest.mark.parametrize("variant,generic,what", EMU_SETS)
def test_filter_builds_on_host_match_the_oracle(prt, oracle, emu, monkeypatch, variant, generic, what, kind, r):
    """every filter set x kinds and radii, default camera (aperture open: the lens draws follow the offset), frames mode"""
    if generic:
        monkeypatch.setenv("PT_EMU_GENERIC", "1")
    W, H, frames = 29, 19, 96
    scene, cfg, cam, env = _scene(prt, variant, W, H)
    seeds = prt.seed_pairs(frames)
    pf, T = _emu_filter(kind, r)
    off = mirror_offsets(kind, r, W, H, frames, T)
    if r == 4.0:
        assert np.abs(off).max() > 3.0                           # the offsets do leave the frame
    ostate, oimg = oracle.Restatement().render(cfg, scene.desc, cam, W, H, seeds, env=env, threads=8, offsets=off)
    state, img = emu.render(oracle.PATH_STATE_DTYPE, cfg, scene.desc, cam, W, H, seeds, env=env, sched_seed=31, pixel_filter=pf)
    assert int(state["samples"].max()) > 8
    _same(oracle, ostate, oimg, state, img, "%s (%s) %s %g" % (variant, what, kind, r))
    # not vacuous: the centre-ray oracle is another picture
    cstate, cimg = oracle.Restatement().render(cfg, scene.desc, cam, W, H, seeds, env=env, threads=8)
    assert not oracle.images_equal(cimg, img)


@pytest.mark.parametrize("variant,kind", [("cornell_coat", "tent"), ("cornell_edge", "blackman-harris")])
def test_pinhole_camera_on_host(prt, oracle, emu, variant, kind):
    W, H, frames = 29, 19, 96
    scene, cfg, cam, env = _scene(prt, variant, W, H, pinhole=True)
    assert cam.apertureRadius == 0.0
    seeds = prt.seed_pairs(frames)
    r = DEFAULT_R[kind]
    pf, T = _emu_filter(kind, r)
    off = mirror_offsets(kind, r, W, H, frames, T)
    ostate, oimg = oracle.Restatement().render(cfg, scene.desc, cam, W, H, seeds, env=env, threads=8, offsets=off)
    state, img = emu.render(oracle.PATH_STATE_DTYPE, cfg, scene.desc, cam, W, H, seeds, env=env, pixel_filter=pf)
    _same(oracle, ostate, oimg, state, img, "%s pinhole %s" % (variant, kind))


@pytest.mark.parametrize("sched", [(8, 0), (1, 0), (8, 12345)])
@pytest.mark.parametrize("variant,kind", [("cornell_coat", "gaussian"), ("cornell_media", "tent")])
def test_schedules_on_host(prt, oracle, emu, variant, kind, sched):
    W, H, frames = 29, 19, 96
    scene, cfg, cam, env = _scene(prt, variant, W, H)
    seeds = prt.seed_pairs(frames)
    r = DEFAULT_R[kind]
    pf, T = _emu_filter(kind, r)
    off = mirror_offsets(kind, r, W, H, frames, T)
    ostate, oimg = oracle.Restatement().render(cfg, scene.desc, cam, W, H, seeds, env=env, threads=8, offsets=off)
    state, img = emu.render(oracle.PATH_STATE_DTYPE, cfg, scene.desc, cam, W, H, seeds, env=env, walk_min_lanes=sched[0], sched_seed=sched[1],
                            pixel_filter=pf)
    _same(oracle, ostate, oimg, state, img, "%s %s schedule %s" % (variant, kind, sched))


@pytest.mark.parametrize("variant,kind", [("cornell_diffuse", "box"), ("cornell_roughdiel", "gaussian"), ("cornell_media", "tent")])
def test_spp_mode_and_resumed_runs_on_host(prt, oracle, emu, variant, kind):
    """"N spp" mode in launches of 32 frames (with and without lanes running ahead), and a run continued from a saved state: the path index
    continues from the state's `samples`, it does not restart with the launch"""
    W, H, spp = 29, 19, 12
    maxf = spp * 16 + 64
    scene, cfg, cam, env = _scene(prt, variant, W, H)
    seeds = prt.seed_pairs(maxf)
    r = DEFAULT_R[kind]
    pf, T = _emu_filter(kind, r)
    off = mirror_offsets(kind, r, W, H, spp, T)                   # exactly spp paths: one path more would be refused
    ostate, oimg = oracle.Restatement().render(cfg, scene.desc, cam, W, H, seeds, env=env, threads=8, spp_limit=spp, offsets=off)
    assert (ostate["samples"] == spp).all() and (ostate["reset"] != 0).all()
    state = img = None
    for f in range(0, maxf, 32):
        state, img = emu.render(oracle.PATH_STATE_DTYPE, cfg, scene.desc, cam, W, H, seeds[2 * f:2 * (f + 32)], first_frame=1 + f,
                                state=state, img=img, env=env, spp_limit=spp, sched_seed=99 + f, pixel_filter=pf)
    _same(oracle, ostate, oimg, state, img, "%s %s: N spp in launches of 32" % (variant, kind))
    state = img = None
    ahead = np.zeros(W * H, dtype=np.uint32)
    ran_ahead = 0
    for f in range(0, maxf, 32):
        state, img = emu.render(oracle.PATH_STATE_DTYPE, cfg, scene.desc, cam, W, H, seeds[2 * f:], first_frame=1 + f,
                                state=state, img=img, env=env, spp_limit=spp, sched_seed=7 + f, walk_min_lanes=6, window=32, ahead=ahead,
                                pixel_filter=pf)
        ran_ahead += int((ahead > 0).sum())
    assert ran_ahead > 0 and not ahead.any()
    _same(oracle, ostate, oimg, state, img, "%s %s: N spp, lanes running ahead" % (variant, kind))
    # frames mode, resumed: 40 frames, the state saved, 56 more with first_frame advanced -- both sides resumed, and against one run of 96
    frames, cut = 96, 40
    off = mirror_offsets(kind, r, W, H, frames, T)
    wstate, wimg = oracle.Restatement().render(cfg, scene.desc, cam, W, H, seeds[:2 * frames], env=env, threads=8, offsets=off)
    s1, _ = emu.render(oracle.PATH_STATE_DTYPE, cfg, scene.desc, cam, W, H, seeds[:2 * cut], env=env, pixel_filter=pf)
    assert int(s1["samples"].min()) >= 2                          # every pixel is past its first path: a restarted index would show
    saved = s1.copy()
    s2, i2 = emu.render(oracle.PATH_STATE_DTYPE, cfg, scene.desc, cam, W, H, seeds[2 * cut:2 * frames], first_frame=1 + cut, state=saved.copy(),
                        env=env, sched_seed=5, pixel_filter=pf)
    _same(oracle, wstate, wimg, s2, i2, "%s %s: emulator resumed vs one oracle run" % (variant, kind))
    o2, oi2 = oracle.Restatement().render(cfg, scene.desc, cam, W, H, seeds[2 * cut:2 * frames], first_frame=1 + cut,
                                          state=saved.view(oracle.PATH_STATE_DTYPE).copy(), env=env, threads=8, offsets=off)
    _same(oracle, wstate, wimg, o2, oi2, "%s %s: oracle resumed vs one oracle run" % (variant, kind))


@pytest.mark.parametrize("variant,kind,r", [("cornell_mixed", "tent", 1.0), ("cornell_media_hg", "gaussian", 1.5), ("cornell_coat", "box", 4.0)])
def test_ragged_frame_row_tile_and_row_blocks_on_host(prt, oracle, emu, variant, kind, r):
    """width and height not multiples of 8; a tile with row0 > 0 and an interleaved row-block part: the hash takes GLOBAL gx, gy.  Each part
    against the oracle's render of the same part AND against the rows of the oracle's whole frame"""
    W, H, frames = 37, 23, 64
    scene, cfg, cam, env = _scene(prt, variant, W, H)
    seeds = prt.seed_pairs(frames)
    pf, T = _emu_filter(kind, r)
    off = mirror_offsets(kind, r, W, H, frames, T)
    O = oracle.Restatement()
    ostate, oimg = O.render(cfg, scene.desc, cam, W, H, seeds, env=env, threads=8, offsets=off)
    state, img = emu.render(oracle.PATH_STATE_DTYPE, cfg, scene.desc, cam, W, H, seeds, env=env, sched_seed=7, pixel_filter=pf)
    _same(oracle, ostate, oimg, state, img, variant + " ragged")
    row0, rows = 5, 11
    tstate, timg = emu.render(oracle.PATH_STATE_DTYPE, cfg, scene.desc, cam, W, H, seeds, env=env, sched_seed=8, row0=row0, rows=rows, pixel_filter=pf)
    pstate, pimg = O.render(cfg, scene.desc, cam, W, H, seeds, env=env, threads=8, row0=row0, rows=rows, offsets=off)
    _same(oracle, pstate, pimg, tstate, timg, variant + " tile at row 5")
    _same(oracle, ostate.reshape(H, W)[row0:row0 + rows].reshape(-1), oimg[row0:row0 + rows], tstate, timg, variant + " tile vs the frame's rows")
    blocks = (4, 3, 1)
    rows_b = [y for y in range(H) if (y // blocks[0]) % blocks[1] == blocks[2]]
    bstate, bimg = emu.render(oracle.PATH_STATE_DTYPE, cfg, scene.desc, cam, W, H, seeds, env=env, sched_seed=9, blocks=blocks, pixel_filter=pf)
    qstate, qimg = O.render(cfg, scene.desc, cam, W, H, seeds, env=env, threads=8, blocks=blocks, offsets=off)
    _same(oracle, qstate, qimg, bstate, bimg, variant + " row blocks")
    _same(oracle, ostate.reshape(H, W)[rows_b].reshape(-1), oimg[rows_b], bstate, bimg, variant + " row blocks vs the frame's rows")


@pytest.mark.parametrize("variant", ["cornell_coat", "cornell_media_hg"])
def test_oracle_zero_table_is_the_centre_ray_and_a_short_table_is_refused(prt, oracle, variant):
    """the oracle alone: a table of zeros gives the golden's bits (as NULL does); a path beyond the table is an error, not a clamp"""
    g = np.load(os.path.join(GOLDEN, variant + ".npz"))
    W, H, frames = int(g["width"]), int(g["height"]), int(g["frames"])
    scene, cfg, cam, env = _scene(prt, variant, W, H)
    seeds = prt.seed_pairs(frames)
    gstate = np.ascontiguousarray(g["state"]).view(oracle.PATH_STATE_DTYPE).reshape(-1)
    O = oracle.Restatement()
    nstate, nimg = O.render(cfg, scene.desc, cam, W, H, seeds, env=env, threads=8)
    _same(oracle, gstate, g["image"], nstate, nimg, variant + " no table")
    K = int(gstate["samples"].max())
    zstate, zimg = O.render(cfg, scene.desc, cam, W, H, seeds, env=env, threads=8, offsets=np.zeros((H, W, K, 2), np.float32))
    _same(oracle, gstate, g["image"], zstate, zimg, variant + " table of zeros")
    with pytest.raises(RuntimeError, match="-6"):
        O.render(cfg, scene.desc, cam, W, H, seeds, env=env, threads=8, offsets=np.zeros((H, W, K - 1, 2), np.float32))
    with pytest.raises(ValueError):
        O.render(cfg, scene.desc, cam, W, H, seeds, env=env, threads=8, offsets=np.zeros((H, W + 1, K, 2), np.float32))


def test_emulator_refuses_what_the_product_refuses_under_a_filter(prt, oracle, emu):
    W, H = 16, 8
    seeds = prt.seed_pairs(4)
    cam = prt.default_camera(W, H)
    mixed = prt.HostScene("cornell_mixed.json")
    edits = [lambda c: setattr(c, "view_option", 1), lambda c: setattr(c, "pick_random_light", 1), lambda c: setattr(c, "env_importance_sampling", 1)]
    cases = []
    for edit in edits:
        cfg = mixed.config()
        edit(cfg)
        cases.append((mixed, cfg))
    sdf = prt.HostScene("cornell_sdf.json")
    cases.append((sdf, sdf.config()))
    for scene, cfg in cases:
        emu.render(oracle.PATH_STATE_DTYPE, cfg, scene.desc, cam, W, H, seeds, env=prt.make_sky(64, 32))           # fine without a filter
        with pytest.raises(RuntimeError) as e:
            emu.render(oracle.PATH_STATE_DTYPE, cfg, scene.desc, cam, W, H, seeds, env=prt.make_sky(64, 32), pixel_filter=(KINDS["tent"], 1.0, None))
        assert e.value.code == prt.PRT_ERR_UNSUPPORTED
    cfg = mixed.config()
    for pf in ((KINDS["gaussian"], 1.5, None), (7, 1.0, None), (KINDS["box"], 4.5, None), (KINDS["box"], float("nan"), None)):
        with pytest.raises(RuntimeError) as e:
            emu.render(oracle.PATH_STATE_DTYPE, cfg, mixed.desc, cam, W, H, seeds, pixel_filter=pf)
        assert e.value.code == prt.PRT_ERR_INVALID_ARGUMENT


# ---- the GPU against the oracle ------------------------------------------------------------------------------------------------------------------

SET_KINDS = [("tent", 1.0), ("gaussian", 1.5), ("blackman-harris", 2.0), ("box", 0.5), ("gaussian", 0.3), ("tent", 4.0), ("blackman-harris", 2.0)]
GPU_ROWS = [row + kr for row, kr in zip(SETS, SET_KINDS)]


def _gpu_setup(prt, scene_json, W, H, env, generic=False, pinhole=False):
    scene, cfg, cam, r = _setup(prt, scene_json, W, H, env=env, pinhole=pinhole)
    if generic:
        r.set_option("generic", 1)
    return scene, cfg, cam, r, (prt.make_sky(64, 32) if env else None)


def _forced_generic(scene_json, tag):
    return tag == "generic" and scene_json == "cornell_diffuse.json"


def _gpu_same(oracle, ostate, oimg, r, what, mask=None):
    state = r.read_state().view(oracle.PATH_STATE_DTYPE)
    img = r.read_framebuffer()
    if mask is not None:
        ostate, state = ostate[mask], state[mask]
        oimg, img = oimg.reshape(-1, 4)[mask], img.reshape(-1, 4)[mask]
    bad = oracle.state_fields_equal(ostate, state)
    assert not bad, "%s: path state differs from the oracle in %s" % (what, bad)
    assert oracle.images_equal(oimg, img), "%s: framebuffer differs from the oracle" % what


def _variant_names(v, kind, tag):
    assert "filter=%s" % kind in v and tag in v, v


@pytest.mark.gpu
@pytest.mark.parametrize("scene_json,env,tag,kind,rad", GPU_ROWS)
def test_gpu_filter_sets_match_the_oracle_in_frames_and_spp_mode(prt, oracle, scene_json, env, tag, kind, rad):
    W, H, frames, spp = 40, 24, 40, 16
    scene, cfg, cam, r, sky = _gpu_setup(prt, scene_json, W, H, env, _forced_generic(scene_json, tag))
    r.set_pixel_filter(kind, rad)
    seeds = prt.seed_pairs(spp * 16 + 64)
    off = gpu_offsets(prt, kind, rad, W, H, frames)
    O = oracle.Restatement()
    ostate, oimg = O.render(cfg, scene.desc, cam, W, H, seeds[:2 * frames], env=sky, threads=16, offsets=off)
    r.reset()
    r.render_frames(seeds[:2 * frames])
    _variant_names(r.kernel_variant(), kind, tag)
    _gpu_same(oracle, ostate, oimg, r, "%s %s %g, frames" % (tag, kind, rad))
    ostate, oimg = O.render(cfg, scene.desc, cam, W, H, seeds, env=sky, threads=16, spp_limit=spp, offsets=off[:, :, :spp])
    assert (ostate["samples"] == spp).all()
    r.reset()
    r.render_spp(spp, seeds)
    _variant_names(r.kernel_variant(), kind, tag)
    _gpu_same(oracle, ostate, oimg, r, "%s %s %g, %d spp" % (tag, kind, rad, spp))
    r.close()


def _adaptive_against_the_oracle(prt, oracle, r, cfg, scene, cam, sky, W, H, kind, rad, what, lo=4, hi=32, rel=0.2):
    """every distinct path count kk of an adaptive render against the oracle at spp_limit = kk, on the pixels that stopped there"""
    seeds = prt.seed_pairs(hi * 16 + 64)
    r.reset()
    r.render_adaptive(seeds, lo, hi, rel)
    v = r.kernel_variant()
    assert "adaptive" in v and "filter=%s" % kind in v, v
    k = r.read_state()["samples"]
    ks = np.unique(k)
    assert len(ks) >= 3, "%s: vacuous, the pixels stopped at %s" % (what, ks)
    off = gpu_offsets(prt, kind, rad, W, H, hi)
    O = oracle.Restatement()
    for kk in ks:
        ostate, oimg = O.render(cfg, scene.desc, cam, W, H, seeds, env=sky, threads=16, spp_limit=int(kk), offsets=off)
        _gpu_same(oracle, ostate, oimg, r, "%s: pixels of %d paths" % (what, kk), mask=k == kk)
    return ks


@pytest.mark.gpu
@pytest.mark.parametrize("scene_json,env,tag,kind,rad", GPU_ROWS)
def test_gpu_filter_sets_match_the_oracle_in_adaptive_mode(prt, oracle, scene_json, env, tag, kind, rad):
    W, H = 40, 24
    scene, cfg, cam, r, sky = _gpu_setup(prt, scene_json, W, H, env, _forced_generic(scene_json, tag))
    r.set_pixel_filter(kind, rad)
    _adaptive_against_the_oracle(prt, oracle, r, cfg, scene, cam, sky, W, H, kind, rad, "%s %s %g adaptive" % (tag, kind, rad))
    assert tag in r.kernel_variant()
    r.close()


@pytest.mark.gpu
@pytest.mark.parametrize("scene_json,env,tag,kind,rad", GPU_ROWS)
def test_gpu_wave_count_builds_and_pixel_mappings_match_the_oracle(prt, oracle, scene_json, env, tag, kind, rad):
    """the 5- and 6-wave builds of every filter instance under both pixel-to-wave mappings, forced and read back; ragged frame"""
    W, H, spp = 37, 23, 8
    scene, cfg, cam, r, sky = _gpu_setup(prt, scene_json, W, H, env, _forced_generic(scene_json, tag))
    r.set_pixel_filter(kind, rad)
    seeds = prt.seed_pairs(spp * 16 + 64)
    off = gpu_offsets(prt, kind, rad, W, H, spp)
    ostate, oimg = oracle.Restatement().render(cfg, scene.desc, cam, W, H, seeds, env=sky, threads=16, spp_limit=spp, offsets=off)
    for waves in (5, 6):
        for scatter in (0, 1):
            r.set_option("waves", waves)
            r.set_option("scatter", scatter)
            r.reset()
            r.render_spp(spp, seeds)
            v = r.kernel_variant()
            _variant_names(v, kind, tag)
            assert "waves=%d" % waves in v and ("pixels=scattered" if scatter else "pixels=tiles") in v, v
            _gpu_same(oracle, ostate, oimg, r, "%s %s waves=%d scatter=%d" % (tag, kind, waves, scatter))
    r.close()


@pytest.mark.gpu
@pytest.mark.parametrize("scene_json,env,tag,kind,rad", [row for row in GPU_ROWS if not _forced_generic(row[0], row[2]) and row[0] != "cornell_mixed.json"])
def test_gpu_compiled_filter_set_equals_the_filtered_generic_dispatch(prt, scene_json, env, tag, kind, rad):
    W, H, spp = 40, 24, 16
    scene, cfg, cam, r, sky = _gpu_setup(prt, scene_json, W, H, env)
    r.set_pixel_filter(kind, rad)
    seeds = prt.seed_pairs(spp * 16 + 64)
    out = []
    for generic in (0, 1):
        r.set_option("generic", generic)
        r.reset()
        r.render_spp(spp, seeds)
        v = r.kernel_variant()
        assert "filter=%s" % kind in v and ("generic" in v) == bool(generic), v
        out.append((np.ascontiguousarray(r.read_state()).view(np.uint8), np.ascontiguousarray(r.read_framebuffer()).view(np.uint32)))
    assert (out[0][0] == out[1][0]).all() and (out[0][1] == out[1][1]).all(), (tag, kind)
    r.close()


@pytest.mark.gpu
@pytest.mark.parametrize("scene_json,env,waves", [("cornell_coat.json", False, 5), ("cornell_roughdiel.json", True, 6)])
def test_gpu_live_pixel_list_launches_match_the_oracle(prt, oracle, scene_json, env, waves):
    """prt_render_adaptive's list launches of a filter instance (options "compact", "compact_below", "frames_per_launch").  An adaptive render has
    ONE build per set, at the wave count its tile launches take (launch_variant: the option "waves" does not apply): the coat set's is the
    5-wave build, the rough dielectric's the 6-wave one -- read back"""
    W, H = 64, 40
    kind, rad = "tent", 1.0
    scene, cfg, cam, r, sky = _gpu_setup(prt, scene_json, W, H, env)
    r.set_pixel_filter(kind, rad)
    r.set_option("compact", 1)
    r.set_option("compact_below", 100)
    r.set_option("frames_per_launch", 8)
    _adaptive_against_the_oracle(prt, oracle, r, cfg, scene, cam, sky, W, H, kind, rad, "live lists, %s" % scene_json)
    rep = r.adaptive_report()
    assert rep.list_launches >= 1 and 0 < rep.list_live_lanes <= rep.list_lanes, (rep.list_launches, rep.list_live_lanes, rep.list_lanes)
    assert "waves=%d" % waves in r.kernel_variant(), r.kernel_variant()
    r.close()


@pytest.mark.gpu
def test_gpu_ordered_build_matches_the_oracle(prt, oracle, monkeypatch):
    """the ORDER build (FrameArgs::tile_order, "expensive first") of a filter instance: it only runs through a tree of more than 64 k node pairs,
    so a strip of the 871 k-triangle stand-in's 1080p frame, 3 spp in launches of 8 frames, whole tiles forced; read back, and against the oracle"""
    W, H, row0, rows, spp = 1920, 1080, 500, 16, 3
    kind, rad = "tent", 1.0
    prt.ensure_dragon_standin()
    scene = prt.HostScene("cornell_dragon.json")
    cfg = scene.config()
    cam = prt.default_camera(W, H)
    seeds = prt.seed_pairs(spp * 16 + 64)
    r = prt.Renderer(cfg, device=0)
    r.upload_scene(scene)
    r.set_camera(cam)
    r.set_tile(W, H, row0, rows)
    r.set_pixel_filter(kind, rad)
    r.set_option("tile_order", 1)
    r.set_option("scatter", 0)
    r.set_option("frames_per_launch", 8)
    r.render_spp(spp, seeds)
    v = r.kernel_variant()
    assert "expensive first" in v and "filter=tent" in v, v
    gy = np.arange(row0, row0 + rows, dtype=np.uint32)[:, None, None]
    u, w = sample_u(np.arange(W, dtype=np.uint32)[None, :, None], gy, np.arange(spp, dtype=np.uint32)[None, None, :])
    off = np.zeros((H, W, spp, 2), dtype=np.float32)              # only the strip's rows are read
    off[row0:row0 + rows] = np.stack([warp(kind, rad, u), warp(kind, rad, w)], -1)
    ostate, oimg = oracle.Restatement().render(cfg, scene.desc, cam, W, H, seeds, threads=16, spp_limit=spp, row0=row0, rows=rows, offsets=off)
    _gpu_same(oracle, ostate, oimg, r, "ordered build, big tree")
    r.close()


@pytest.mark.gpu
def test_gpu_splits_and_resume_match_the_oracle(prt, oracle):
    """a ragged frame, a tile with row0 > 0, a row-block part and a checkpointed run (prt_read_state / prt_write_state), each against the
    oracle's render of the same thing rather than against another GPU run"""
    W, H, spp = 61, 43, 12
    kind, rad = "gaussian", 1.5
    scene, cfg, cam, r, sky = _gpu_setup(prt, "cornell_mixed.json", W, H, True)
    r.set_pixel_filter(kind, rad)
    seeds = prt.seed_pairs(spp * 16 + 64)
    frames, cut = 120, 50
    off = host_offsets(prt, kind, rad, W, H, frames)
    O = oracle.Restatement()
    ostate, oimg = O.render(cfg, scene.desc, cam, W, H, seeds, env=sky, threads=16, spp_limit=spp, offsets=off)
    r.render_spp(spp, seeds)
    _gpu_same(oracle, ostate, oimg, r, "ragged frame")
    row0, rows = 13, 17
    r.set_tile(W, H, row0, rows)
    r.render_spp(spp, seeds)
    assert "filter=gaussian" in r.kernel_variant()
    pstate, pimg = O.render(cfg, scene.desc, cam, W, H, seeds, env=sky, threads=16, spp_limit=spp, row0=row0, rows=rows, offsets=off)
    _gpu_same(oracle, pstate, pimg, r, "tile at row 13")
    blocks = (8, 3, 1)
    r.set_row_blocks(W, H, *blocks)
    r.render_spp(spp, seeds)
    assert "filter=gaussian" in r.kernel_variant()
    qstate, qimg = O.render(cfg, scene.desc, cam, W, H, seeds, env=sky, threads=16, spp_limit=spp, blocks=blocks, offsets=off)
    _gpu_same(oracle, qstate, qimg, r, "row blocks (8, 3, 1)")
    # checkpoint / resume, frames mode: the path index continues from the state's `samples`
    r.resize(W, H)
    wstate, wimg = O.render(cfg, scene.desc, cam, W, H, seeds[:2 * frames], env=sky, threads=16, offsets=off)
    r.render_frames(seeds[:2 * cut])
    saved = r.read_state()
    assert int(saved["samples"].min()) >= 2
    r.reset()
    r.write_state(saved)
    r.render_frames(seeds[2 * cut:2 * frames], first_frame=1 + cut)
    _gpu_same(oracle, wstate, wimg, r, "resumed at frame %d" % (1 + cut))
    r.close()


@pytest.mark.gpu
@pytest.mark.parametrize("lanes", [1, 64])
def test_gpu_walk_min_lanes_under_a_filter(prt, oracle, lanes):
    W, H, spp = 40, 24, 16
    kind, rad = "blackman-harris", 2.0
    scene, cfg, cam, r, sky = _gpu_setup(prt, "cornell_roughdiel.json", W, H, True)
    r.set_pixel_filter(kind, rad)
    r.set_walk_min_lanes(lanes)
    seeds = prt.seed_pairs(spp * 16 + 64)
    off = host_offsets(prt, kind, rad, W, H, spp)
    ostate, oimg = oracle.Restatement().render(cfg, scene.desc, cam, W, H, seeds, env=sky, threads=16, spp_limit=spp, offsets=off)
    r.render_spp(spp, seeds)
    _variant_names(r.kernel_variant(), kind, "ROUGH_DIEL")
    _gpu_same(oracle, ostate, oimg, r, "walk_min_lanes %d" % lanes)
    r.close()


# ---- filtered guides at K > 1 against a float64 caster -------------------------------------------------------------------------------------------

GUIDE_K = 16


def guide_points(kind, r, K):
    """the K guide sample offsets (dx, dy) of prt.h (prt_render_guides; prt_set_pixel_filter "Guides under a filter"): the R2 point of sample s in
    f32, (0.5, 0.5) for s = 0, warped by the mirror's warp"""
    f = np.float32
    s = np.arange(K, dtype=np.uint32).astype(f)
    fx = f(0.5) + s * f(0.7548776662)
    fy = f(0.5) + s * f(0.5698402910)
    fx, fy = fx - np.floor(fx), fy - np.floor(fy)
    fx[0] = fy[0] = f(0.5)
    T = table(kind, r) if kind in TABLE_KINDS else None
    return warp(kind, r, fx, T), warp(kind, r, fy, T)


def cast_quad(cam, W, H, c, e0, e1, dx, dy, dtype):
    """the K sample rays of every pixel through the pinhole camera model of test_pixel_filter._coverage against the quad (hit_quad's region), all
    arithmetic in `dtype`.  Returns hits (H, W, K) and the hit distance along the normalised ray"""
    t_ = lambda a: np.asarray(a, dtype=dtype)
    Pc, M, Hz, Vt = (t_(a) for a in camera_basis(cam))
    c, e0, e1 = t_(c), t_(e0), t_(e1)
    n = np.cross(e0, e1).astype(dtype)
    anchor = c - (e0 + e1) / dtype(2)
    one, two = dtype(1), dtype(2)
    xs = t_(np.arange(W))[None, :, None] + t_(dx)[None, None, :]
    ys = t_(H - 1 - np.arange(H))[:, None, None] - t_(dy)[None, None, :]
    sx, sy = xs / dtype(W - 1), ys / dtype(H - 1)
    on = M + Hz * (two * sx - one)[..., None] + Vt * (two * sy - one)[..., None]
    d = (on - Pc).astype(dtype)
    t = ((c - Pc) @ n) / (d @ n)
    X = Pc + d * t[..., None] - anchor
    b0, b1 = (X @ e0) / (e0 @ e0), (X @ e1) / (e1 @ e1)
    hit = (b0 >= 0) & (b0 <= 1) & (b1 >= 0) & (b1 <= 1) & (t > 0)
    return hit, (t * np.linalg.norm(d, axis=-1)).astype(np.float64)


def _guide_case(prt, kind):
    W, H = 96, 64
    js, cam, c, e0, e1 = _quad_scene(prt, W, H)
    dx, dy = guide_points(kind, DEFAULT_R[kind], GUIDE_K)
    hit64, dist = cast_quad(cam, W, H, c, e0, e1, dx, dy, np.float64)
    hit32, _ = cast_quad(cam, W, H, c, e0, e1, dx, dy, np.float32)
    return js, cam, (e0, e1), hit64, hit32, dist


# pixels whose K = 16 coverage differs between the caster run in float32 and in float64 (the CPU count the cap of the GPU test is made of;
# ~300 edge pixels x 16 samples x 1e-5: a handful at most)
CASTER_F32_VS_F64 = {"box": 0, "tent": 0, "gaussian": 0, "blackman-harris": 0}


@pytest.mark.parametrize("kind", list(KINDS))
def test_the_caster_in_float32_and_float64(prt, kind):
    """the condition the GPU test's cap rests on, measured where no GPU is involved: the float64 caster and its float32 twin disagree on a
    handful of pixels at most (recorded in CASTER_F32_VS_F64)"""
    _, _, _, hit64, hit32, _ = _guide_case(prt, kind)
    differ = int((hit64.sum(-1) != hit32.sum(-1)).sum())
    assert differ == CASTER_F32_VS_F64[kind], (kind, differ)
    assert differ <= 8
    cov = hit64.mean(-1)
    assert ((cov > 0) & (cov < 1)).sum() > 50 and (cov == 1).sum() > 100 and (cov == 0).sum() > 100


@pytest.mark.gpu
@pytest.mark.parametrize("kind", list(KINDS))
def test_gpu_filtered_guides_coverage_matches_a_float64_caster(prt, kind):
    """coverage (hits / K, guides channel 3) is a multiple of 1 / K: equal to the float64 count of the same K sample points except where a sample
    ray passes within f32 rounding of an edge.  Cap on such pixels: max(4, 4 x the float32-vs-float64 count of the numpy caster), each off by
    exactly 1 / K.  CPU counts: box 0, tent 0, gaussian 0, blackman-harris 0 (CASTER_F32_VS_F64) -> the cap is 4 pixels for every kind.
    Depth and normal of fully covered pixels: test_guides_match_a_float64_caster's tolerances"""
    W, H, K = 96, 64, GUIDE_K
    js, cam, (e0, e1), hit64, hit32, dist = _guide_case(prt, kind)
    cpu_differ = int((hit64.sum(-1) != hit32.sum(-1)).sum())
    cap = max(4, 4 * cpu_differ)
    scene = prt.HostScene(js, text=True)
    r = prt.Renderer(scene.config(), device=0)
    r.upload_scene(scene); r.set_camera(cam); r.resize(W, H)
    r.set_pixel_filter(kind)
    r.render_guides(K)
    g = r.read_guides()
    r.close()
    cov = g[..., 3].astype(np.float64) * K
    ref = hit64.sum(-1).astype(np.float64)
    diff = cov - ref
    off = diff != 0
    print("%s: %d pixels differ from the float64 caster (cap %d, the caster's own f32 / f64 count %d)" % (kind, int(off.sum()), cap, cpu_differ))
    assert (np.abs(diff[off]) == 1.0).all(), (kind, np.argwhere(off)[:5].tolist(), diff[off][:5])
    assert int(off.sum()) <= cap, (kind, int(off.sum()), cap, np.argwhere(off)[:8].tolist())
    assert ((ref > 0) & (ref < K)).sum() > 50
    full = (ref == K) & ~off
    assert full.sum() > 100
    n = np.cross(e0, e1); n = -n / np.linalg.norm(n)            # the side facing the camera (the hit has dot(n, dir) > 0: negated)
    assert (np.abs(g[..., 4:7][full] - n).max(-1) <= 1e-3).all(), kind
    depth = dist.mean(-1)[full]
    assert (np.abs(g[..., 7][full] - depth) <= 1e-4 * depth).all(), (kind, float(np.abs(g[..., 7][full] / depth - 1).max()))
    empty = (ref == 0) & ~off
    assert (g[..., 3][empty] == 0).all() and (g[..., 7][empty] == 0).all()
