"""The Lambert-only builds of the lane machine (compiled set LIGHT|DIFF; csrc/hip/pt_device.h lane_front_shared_disk, lambert_only):

  * lane_front sends the lanes that restart a path behind a thin lens and the lanes that sample Lambert through ONE disk sample block
    (disk_sample) instead of one each in create_cam_ray and cosine_hemisphere;
  * lane_back takes the vertex's colour from Lane::weight instead of loading the material a second time.

Same operations on the same operands: every render below equals the CPU restatement of the reference (oracle_api.Restatement) bit for bit,
path state and framebuffer -- the emulator (the device header compiled for the host, random walk-phase lengths) without a GPU, the device
through prt_render_frames and prt_render_spp with one.  A lane that drew one number too many or too few in the shared block would leave its
generator out of step for every later segment.  The sets outside the new path (a medium; the run-time
dispatch; the light pick) are rendered too, and so are scenes whose probes end on the sampled sphere light and on a light that is not the
sampled one.  The listing of the headline instance holds one quadrant conversion of sincos_pair in its frame loop where the parent had two.

A third piece was built and measured and is not in the tree: the cap of the sampled sphere light formed once for the MIS term of a probe
that ended on that sphere and for the light sample (profiles/r25_disk_sample_ab.txt: alone it lost 1.1 ... 1.6 %, beside
the other two it changed nothing).  What it rested on is a property of the two functions as they stand, and the per-function entry (fn 5)
shows it on the known-answer inputs of the sphere light: where sphere_sample_direct goes on (C > 0) its pdf is sphere_direct_pdf's value
bit for bit, and where C <= 0 it returns before it draws."""
import os
import re
import subprocess

import numpy as np
import pytest

from conftest import GOLDEN, ROOT
from cases import frame_loop, HEADLINE, HIP, HIPCC, kernel_lines
from support import assert_same_render as _same, bits, variant_case


W, H = 24, 20                                   # ragged edge tiles in both directions
SPP = 3                                         # of the prt_render_spp runs

# case -> (scene variant, camera, pick_random_light (None: the variant's own), frames, the build it runs (None: not asserted))
LIGHT_DIFF = "render_kernel<LIGHT|DIFF>"
CASES = {
    "lens": ("cornell_diffuse", "lens", None, 64, LIGHT_DIFF),
    "pinhole": ("cornell_diffuse", "pinhole", None, 64, LIGHT_DIFF),           # restarting lanes draw nothing in the shared block
    "medium": ("cornell_media", "lens", None, 64, "render_kernel<LIGHT|DIFF,medium>"),
    "mixed": ("cornell_mixed", "lens", None, 64, "render_kernel<generic>"),
    "sphere_light": ("cornell_diffuse", "lens", None, 96, LIGHT_DIFF),        # every light hit is the sampled sphere
    "two_lights": ("cornell_twolights", "lens", None, 96, "render_kernel<generic,pick_random_light>"),
    # the same scene without the pick: the compiled set, the sphere sampled, and probes that end on the quad light (direct_pdf_mesh as before)
    "two_lights_first": ("cornell_twolights", "lens", 0, 96, LIGHT_DIFF),
}


def _case(prt, name):
    variant, camera, pick, frames, build = CASES[name]
    scene, cfg, _, env = variant_case(prt, variant, W, H)
    if pick is not None:
        cfg.pick_random_light = pick
    if camera == "pinhole":
        cam = prt.orbit_camera(W, H, d_aperture=-1.0)
        assert cam.apertureRadius == 0.0
    else:
        cam = prt.default_camera(W, H)
        assert cam.apertureRadius > 0.00001
    return scene, cfg, cam, env, prt.seed_pairs(frames), build


@pytest.fixture(scope="module")
def restatement(prt, oracle):
    """the oracle's render of a case, computed once: name, spp_limit -> (state, image)"""
    done = {}

    def get(name, spp_limit=0):
        if (name, spp_limit) not in done:
            scene, cfg, cam, env, seeds, _ = _case(prt, name)
            state, img = oracle.Restatement().render(cfg, scene.desc, cam, W, H, seeds, env=env, spp_limit=spp_limit, threads=8)
            state.setflags(write=False)
            img.setflags(write=False)
            done[(name, spp_limit)] = (state, img)
        return done[(name, spp_limit)]
    return get


@pytest.fixture(scope="module")
def emu():
    import emu_api
    emu_api.lib()
    return emu_api


@pytest.mark.parametrize("name", list(CASES))
def test_emulator_matches_restatement(prt, oracle, emu, restatement, name):
    scene, cfg, cam, env, seeds, build = _case(prt, name)
    ostate, oimg = restatement(name)
    for sched in ((8, 0), (8, 4242), (3, 17)):
        state, img = emu.render(oracle.PATH_STATE_DTYPE, cfg, scene.desc, cam, W, H, seeds, env=env, walk_min_lanes=sched[0], sched_seed=sched[1])
        _same(oracle, ostate, oimg, state, img, "%s schedule %s" % (name, sched))
        assert emu.last_variant() == build
    if name == "lens":                          # lanes restart paths in the wave in which others shade: both groups met in the shared block
        assert int(ostate["samples"].min()) >= 2 and int(ostate["diff"].max()) >= 1


def _sphere_light_tables():
    g = np.load(os.path.join(GOLDEN, "kat_functions.npz"))
    names = sorted({k.split("/")[0] for k in g.files})
    return [(n, g[n + "/params"], g[n + "/cases"], g[n + "/expect"]) for n in names if int(g[n + "/fn"]) == 5]


def _same_floats(a, b):
    """equal as words, a NaN equal to a NaN (the fixture's NaN and a device's differ in sign, as tests/test_kat.py allows)"""
    return bool(((bits(a) == bits(b)) | (np.isnan(a) & np.isnan(b))).all())


def check_sphere_cap(run):
    """fn 5: [0] sphere_sample_direct's return, [5] its pdf, [6] sphere_direct_pdf of the same sphere and point, [30..31] the generator"""
    tables = _sphere_light_tables()
    assert tables
    failed = 0
    for name, params, cases, expect in tables:
        out = run(5, params, cases)
        assert _same_floats(out[:, 6], expect[:, 6]) and _same_floats(out[:, 5], expect[:, 5]), name     # (the reference's answers)
        ok = out[:, 0] != 0.0
        assert _same_floats(out[ok, 5], out[ok, 6]), "%s: the sample's pdf is not sphere_direct_pdf's" % name
        assert (bits(out[~ok, 30:32]) == bits(cases[~ok, 30:32])).all(), "%s: a failed sample drew" % name
        failed += int((~ok).sum())
    assert failed > 0, "no C <= 0 case among the known-answer inputs"


def test_sphere_sample_pdf_is_the_direct_pdf_on_host(emu):
    check_sphere_cap(emu.selftest_fn)


needs_hipcc = pytest.mark.skipif(not os.path.exists(HIPCC), reason="no hipcc")


@needs_hipcc
def test_frame_loop_converts_one_quadrant(tmp_path):
    """sincos_pair's quadrant (v_cvt_i32_f32 of prt_sincos_kernel) once in the frame loop of render_kernel<LIGHT|DIFF, no medium, 6 waves>:
    the parent's listing has two, create_cam_ray's and cosine_hemisphere's"""
    out = tmp_path / "pt_kernels.s"
    cmd = [HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=off", "-fno-fast-math", "-fno-slp-vectorize", "-DPT_UNITY", "-S",
           "--cuda-device-only", "-DPT_DEV_ONE_VARIANT", "-I" + os.path.join(ROOT, "include"), "-I" + HIP, "-o", str(out), os.path.join(HIP, "pt_kernels.hip")]
    subprocess.run(cmd, check=True, capture_output=True, timeout=1800)
    loop = [l.split(";")[0] for l in frame_loop(kernel_lines(out.read_text(), HEADLINE))]
    assert len(loop) > 2000, len(loop)                                     # (the parser found the frame loop)
    # the quadrant is the integer of k = rint(x * 2 / pi), and the reduction's first step multiplies the same k by -pi / 2 (0xbfc90fdb) a
    # few instructions away; the loop's other float-to-int conversions (env_lookup's texel indices) have no such neighbour
    first_steps = [l for l in loop if "0xbfc90fdb" in l]
    quadrants = []
    for i, l in enumerate(loop):
        m = re.match(r"\s+v_cvt_i32_f32\w*\s+v\d+,\s*(v\d+)\s*$", l)
        if m and any("0xbfc90fdb" in x and re.search(r"\b%s\b" % m.group(1), x) for x in loop[max(0, i - 12):i + 13]):
            quadrants.append(l.strip())
    assert len(quadrants) == 1 and len(first_steps) == 1, (quadrants, first_steps)


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(CASES))
def test_device_matches_restatement(prt, oracle, restatement, name):
    scene, cfg, cam, env, seeds, build = _case(prt, name)
    r = prt.Renderer(cfg, device=0)
    try:
        r.upload_scene(scene)
        if env is not None:
            r.upload_envmap(env)
        r.set_camera(cam)
        r.resize(W, H)
        r.render_frames(seeds)
        assert build in r.kernel_variant()
        ostate, oimg = restatement(name)
        _same(oracle, ostate, oimg, r.read_state(), r.read_framebuffer(), name + " prt_render_frames")
        r.reset()
        used = r.render_spp(SPP, seeds)         # every pixel frozen after SPP paths: the restatement's "N spp" rule over the same frames
        assert 0 < used <= len(seeds) // 2
        ostate, oimg = restatement(name, SPP)
        assert (ostate["samples"] == SPP).all()
        _same(oracle, ostate, oimg, r.read_state(), r.read_framebuffer(), name + " prt_render_spp")
    finally:
        r.close()


@pytest.mark.gpu
def test_sphere_sample_pdf_is_the_direct_pdf_on_device(prt):
    scene = prt.HostScene("cornell_diffuse.json")
    r = prt.Renderer(scene.config(), device=0)
    try:
        check_sphere_cap(r.selftest_fn)
    finally:
        r.close()
