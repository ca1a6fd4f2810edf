"""Ray queries (prt_cast_rays, prt_occluded, prt_cast_pixels and the device variants; include/prt.h "Ray queries").  The contract checked here:
the bodies of csrc/hip/pt_cast.h, run on the host by tests/emu/cast_emu.cpp, agree with an independent float64 caster (the Caster of
tests/mirrors.py, extended below to arbitrary rays and to primitive and triangle ids); occlusion and closest hit agree exactly where the
code says they must; no bit of a record depends on the wave a ray runs in, on the schedule of the walk or on the rays around it; invalid
rays are misses; the kernels have no scratch.  On the GPU: the C ABI equals the emulator bit for bit, prt_cast_pixels equals the guides'
depth, a cast sees every update, it writes nothing of the context, and every refusal leaves the output alone."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from conftest import ROOT
from cases import cast_ray_sets as _rays, _chain_desc, desc_with, meshes_of, move_quad, move_sphere, random_rays, scene_of
from mirrors import Caster, EPS, _nrm

PKG = os.path.join(ROOT, "photorealistic-rendering-using-opencl_amd")
HIP = os.path.join(PKG, "csrc", "hip")
HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
f32 = np.float32
W, H = 64, 48
MISS, TRIANGLE = -2, -1
SCENES = ["cornell_diffuse", "cornell_edge", "cornell_sdf", "cornell_quadlight"]
NO_SDF = ["cornell_diffuse", "cornell_edge", "cornell_quadlight"]


@pytest.fixture(scope="module")
def emu():
    import cast_api
    cast_api.lib()
    return cast_api


def _words(a):
    return np.ascontiguousarray(a).view(np.uint32).reshape(len(a), -1)


# ---- scenes and ray sets (computed once, shared, never written to) -------------------------------------------------------------------------

_emu = {}                                # (the scenes and the ray sets are cases.cast_scenes and cases.cast_ray_sets: here _rays)


def pixel_grid():
    ys, xs = np.mgrid[0:H, 0:W]
    return np.stack([xs.ravel(), ys.ravel()], 1).astype(np.int32)


def camera_rays(prt, emu):
    """the pixel-centre pinhole rays of a 64 x 48 frame of the default camera, aperture closed"""
    if "camera" not in _rays:
        cam = prt.default_camera(W, H)
        cam.apertureRadius = 0.0
        r = emu.pixel_rays(cam, W, H, pixel_grid())
        r.setflags(write=False)
        _rays["camera"] = r
    return _rays["camera"]


def ray_set(prt, emu, name, which):
    return camera_rays(prt, emu) if which == "camera" else random_rays(prt, emu, name)


def emu_records(prt, emu, name, which):
    """(hits, occluded) of the emulator on a scene's ray set"""
    key = (name, which)
    if key not in _emu:
        sc, cfg = scene_of(prt, name)
        rays = ray_set(prt, emu, name, which)
        h, o = emu.cast(cfg, sc.desc, rays), emu.occluded(cfg, sc.desc, rays)
        h.setflags(write=False)
        o.setflags(write=False)
        _emu[key] = (h, o)
    return _emu[key]


# ---- the float64 caster, extended: arbitrary rays with a limit, primitive ids, triangle ids by brute force over all triangles ------------------

class RayCaster(Caster):
    def cast(self, o, d, tmax):
        """closest hit of each ray in (EPS, min(tmax, 20)): t (inf = miss), normal as finish_closest leaves it, id (-2 miss, -1 triangle, i = meshes[i]),
        tri (the caller's triangle)"""
        R = o.shape[0]
        best = np.minimum(np.asarray(tmax, dtype=np.float64), 20.0) * np.ones(R)
        nrm = np.zeros((R, 3))
        mid = np.full(R, MISS)
        tri = np.zeros(R, dtype=np.int64)
        for a in range(0, R if self.T else 0, 64):                  # every triangle against every ray, 64 rays at a time
            oo, dd = o[a:a + 64, None, :], d[a:a + 64, None, :]
            with np.errstate(divide="ignore", invalid="ignore"):
                pv = np.cross(dd, self.e2[None])
                inv_det = 1.0 / (self.e1[None] * pv).sum(-1)
                tv = oo - self.p0[None]
                u = (tv * pv).sum(-1) * inv_det
                qv = np.cross(tv, self.e1[None])
                v = (dd * qv).sum(-1) * inv_det
                t = (self.e2[None] * qv).sum(-1) * inv_det
                ok = (u >= 0) & (v >= 0) & (u + v <= 1) & (t > EPS) & (t < best[a:a + 64, None])
            t = np.where(ok, t, np.inf)
            k = t.argmin(1)
            rows = np.arange(len(k))
            hit = ok[rows, k]
            nn = self.nv[k]
            uk, vk = u[rows, k][:, None], v[rows, k][:, None]
            sl = slice(a, a + len(k))
            best[sl] = np.where(hit, t[rows, k], best[sl])
            mid[sl] = np.where(hit, TRIANGLE, mid[sl])
            tri[sl] = np.where(hit, k, 0)
            with np.errstate(invalid="ignore"):
                nrm[sl] = np.where(hit[:, None], _nrm(nn[:, 0] * (1 - uk - vk) + nn[:, 1] * uk + nn[:, 2] * vk), nrm[sl])
        for c, rad, i in self.spheres:
            p = o - c
            B = (p * d).sum(1)
            det = B * B - ((p * p).sum(1) - rad * rad)
            ok = det >= 0
            sq = np.sqrt(np.where(ok, det, 0))
            t1, t2 = -B - sq, -B + sq
            t = np.where((t1 > EPS) & (t1 < best), t1, np.where((t2 > EPS) & (t2 < best), t2, np.inf))
            hit = ok & np.isfinite(t)
            best = np.where(hit, t, best)
            nrm = np.where(hit[:, None], _nrm(o + d * np.where(hit, t, 0)[:, None] - c), nrm)
            mid = np.where(hit, i, mid)
        for base, e0, e1, qn, i in self.quads:
            anchor = base - (e0 + e1) * 0.5
            nd = d @ qn
            with np.errstate(divide="ignore", invalid="ignore"):
                t = ((anchor - o) @ qn) / nd
                q = o + d * t[:, None]
                x0, x1 = ((q - anchor) @ e0) / (e0 @ e0), ((q - anchor) @ e1) / (e1 @ e1)
                hit = (nd > 1e-5) & (t > EPS) & (t < best) & (x0 >= 0) & (x0 <= 1) & (x1 >= 0) & (x1 <= 1)
            best = np.where(hit, t, best)
            nrm = np.where(hit[:, None], qn, nrm)
            mid = np.where(hit, i, mid)
        found = mid > MISS
        best = np.where(found, best, np.inf)
        tri = np.where(mid == TRIANGLE, tri, 0)
        for r in np.nonzero(found)[0]:                            # finish_closest: the normal of a non-transmissive hit faces the ray
            if mid[r] == TRIANGLE and self.ntrans:                # (prt.h: with a dielectric kind in the scene a triangle's normal is never turned --
                continue                                          # the reference looks its material up at meshes[-1], a record of zeros)
            _, t_bits, _ = self.mat(mid[r])
            if (t_bits & 0xffff & ~self.ntrans) and (nrm[r] @ d[r]) > 0:
                nrm[r] = -nrm[r]
        return best, nrm, mid, tri


def disagreements(hits, ref):
    """per ray: the record differs from the float64 caster's by more than test_guides_match_a_float64_caster allows"""
    t, n, mid, tri = ref
    miss = hits["id"] == MISS
    ref_miss = ~np.isfinite(t)
    both = ~miss & ~ref_miss
    with np.errstate(invalid="ignore"):
        t_ok = both & (np.abs(hits["t"] - t) <= 1e-4 * np.maximum(np.abs(t), 1e-30))
        n_bad = both & (np.abs(hits["normal"] - n).max(-1) > 1e-3)
    id_bad = t_ok & (hits["id"] != mid)
    tri_bad = t_ok & (hits["id"] == TRIANGLE) & (mid == TRIANGLE) & (hits["tri"] != tri)
    return (miss != ref_miss) | (both & ~t_ok) | n_bad | id_bad | tri_bad


# ---- no GPU: 1. an independent caster ---------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", ["cornell_diffuse", "cornell_mixed"])
@pytest.mark.parametrize("which", ["camera", "random"])
def test_emulator_matches_a_float64_caster(prt, emu, name, which):
    sc, cfg = scene_of(prt, name)
    rays = ray_set(prt, emu, name, which)
    hits = emu_records(prt, emu, name, which)[0]
    ref = RayCaster(sc, cfg).cast(rays[:, 0:3].astype(np.float64), rays[:, 4:7].astype(np.float64), rays[:, 3])
    bad = disagreements(hits, ref)
    print("%s, %s rays: %d of %d differ (%.3f %%); hits %.1f %%, triangles %.1f %%" %
          (name, which, bad.sum(), len(bad), 100 * bad.mean(), 100 * (hits["id"] != MISS).mean(), 100 * (hits["id"] == TRIANGLE).mean()))
    assert bad.mean() <= 0.005, "%s, %s rays: %.2f %% of the rays differ (first %s)" % (name, which, 100 * bad.mean(), np.nonzero(bad)[0][:5].tolist())
    assert (hits["id"] != MISS).mean() > 0.5 and (hits["id"] == TRIANGLE).any()
    # what a record is made of: a miss is the miss record, a triangle carries barycentrics and an index, everything else zeros there
    w = _words(hits)
    miss = hits["id"] == MISS
    assert not w[miss][:, [0, 1, 2, 3, 4, 5, 6, 8, 9, 10, 11]].any()
    notri = hits["id"] != TRIANGLE
    assert not w[notri][:, 1:4].any()
    assert (hits["tri"] < sc.desc.triangle_count).all() and (hits["flags"] <= 1).all()
    o, d = rays[:, 0:3].astype(np.float64), rays[:, 4:7].astype(np.float64)
    hit = ~miss
    assert np.allclose(hits["pos"][hit], (o + d * hits["t"][:, None].astype(np.float64))[hit], atol=1e-5)


# ---- no GPU: 2. exact properties on the emulator ----------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", NO_SDF)
def test_occlusion_is_the_closest_hit_on_scenes_without_sdf(prt, emu, name):
    sc, cfg = scene_of(prt, name)
    for which in ("camera", "random"):
        for tmax in (20.0, 0.5, 1.0, 2.0):
            rays = ray_set(prt, emu, name, which).copy()
            rays[:, 3] = tmax
            h, o = emu.cast(cfg, sc.desc, rays), emu.occluded(cfg, sc.desc, rays)
            assert np.array_equal(o == 1, h["id"] != MISS), (name, which, tmax, np.nonzero((o == 1) != (h["id"] != MISS))[0][:5].tolist())
            assert set(np.unique(o).tolist()) <= {0, 1}
            assert (h["t"][h["id"] != MISS] < min(tmax, 20.0)).all()


@pytest.mark.parametrize("name", SCENES)
def test_records_do_not_depend_on_the_wave_or_the_schedule(prt, emu, name):
    sc, cfg = scene_of(prt, name)
    rays = random_rays(prt, emu, name)
    h, o = emu_records(prt, emu, name, "random")
    perm = np.random.default_rng(7).permutation(len(rays))
    assert np.array_equal(_words(emu.cast(cfg, sc.desc, rays[perm])), _words(h)[perm])
    assert np.array_equal(emu.occluded(cfg, sc.desc, rays[perm]), o[perm])
    for sched in (0, 2, 3):                                        # the plain loop, two random schedules
        assert np.array_equal(_words(emu.cast(cfg, sc.desc, rays, sched=sched)), _words(h)), sched
        assert np.array_equal(emu.occluded(cfg, sc.desc, rays, sched=sched), o), sched
    for n in (1, 63, 64, 65, 130):                                 # (cast_api checks the guard words behind every output)
        assert np.array_equal(_words(emu.cast(cfg, sc.desc, rays[:n])), _words(h)[:n]), n
        assert np.array_equal(emu.occluded(cfg, sc.desc, rays[:n]), o[:n]), n


INVALID = {"nan origin": (1, np.nan), "inf direction": (5, np.inf), "-inf direction": (6, -np.inf), "tmax 0": (3, 0.0), "tmax -0": (3, -0.0),
           "tmax negative": (3, -1.0), "tmax nan": (3, np.nan), "zero direction": None}
MISS_WORDS = np.array([0, 0, 0, 0, 0, 0, 0, 0xFFFFFFFE, 0, 0, 0, 0], dtype=np.uint32)


def with_invalid_rays(rays):
    """`rays` with one invalid ray of each kind planted between valid ones: (rays, the planted indices)"""
    rays = rays.copy()
    at = {}
    for k, (kind, what) in enumerate(INVALID.items()):
        i = 3 + 17 * k                                             # spread over three waves of 64
        if what is None:
            rays[i, 4:7] = (0.0, -0.0, 0.0)
        else:
            rays[i, what[0]] = what[1]
        at[kind] = i
    return rays, at


@pytest.mark.parametrize("name", ["cornell_diffuse", "cornell_sdf"])
def test_invalid_rays_are_misses_and_disturb_nothing(prt, emu, name):
    sc, cfg = scene_of(prt, name)
    good = random_rays(prt, emu, name)[:130]
    h0, o0 = emu_records(prt, emu, name, "random")
    rays, at = with_invalid_rays(good)
    for sched in (0, 1):
        h, o = emu.cast(cfg, sc.desc, rays, sched=sched), emu.occluded(cfg, sc.desc, rays, sched=sched)
        planted = np.zeros(len(rays), dtype=bool)
        for kind, i in at.items():
            assert np.array_equal(_words(h)[i], MISS_WORDS), kind
            assert o[i] == 0, kind
            planted[i] = True
        assert np.array_equal(_words(h)[~planted], _words(h0)[:130][~planted])
        assert np.array_equal(o[~planted], o0[:130][~planted])
    far = good.copy()
    far[:, 3] = 1e30                                               # limit = min(tmax, 20)
    assert np.array_equal(_words(emu.cast(cfg, sc.desc, far)), _words(h0)[:130])
    assert np.array_equal(emu.occluded(cfg, sc.desc, far), o0[:130])
    far[:, 3] = np.inf
    assert np.array_equal(_words(emu.cast(cfg, sc.desc, far)), _words(h0)[:130])


# ---- no GPU: 3. scratch ------------------------------------------------------------------------------------------------------------------------

def test_cast_kernels_have_no_scratch():
    cmd = [HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=off", "-fno-fast-math", "-fno-slp-vectorize", "-c",
           "--cuda-device-only", "-I" + os.path.join(ROOT, "include"), "-I" + HIP, "-Rpass-analysis=kernel-resource-usage", "-o", os.devnull,
           os.path.join(HIP, "pt_cast.hip")]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stderr[-4000:]
    kernels, cur = {}, None
    for line in r.stderr.splitlines():
        m = re.search(r"Function Name: (\S+)", line)
        if m:
            cur = m.group(1)
        m = re.search(r"ScratchSize \[bytes/lane\]: (\d+)", line)
        if m and cur:
            kernels[cur] = int(m.group(1))
    names = " ".join(kernels)
    assert names.count("cast_kernel") == 4, kernels                  # SDF off / on x closest / any
    assert "cast_pixel_rays_kernel" in names, kernels
    assert all(v == 0 for v in kernels.values()), kernels


# ---- on the GPU ----------------------------------------------------------------------------------------------------------------------------------

def _renderer(prt, name, camera=True, size=True, pinhole=True):
    sc, cfg = scene_of(prt, name)
    r = prt.Renderer(cfg, device=0)
    r.upload_scene(sc)
    if camera:
        cam = prt.default_camera(W, H)
        if pinhole:
            cam.apertureRadius = 0.0
        r.set_camera(cam)
    if size:
        r.resize(W, H)
    return r


def _device_cast(r, rays):
    import torch
    d_rays = torch.from_numpy(np.array(rays, dtype=f32)).cuda()
    hits = r.cast_rays(d_rays)
    occ = r.occluded(d_rays)
    torch.cuda.synchronize()
    return hits.cpu().numpy().view(np.uint32), occ.cpu().numpy().view(np.uint32)


def _check_against_emulator(prt, emu, name, door):
    r = _renderer(prt, name, camera=False, size=False)             # a cast needs neither camera nor frame size
    for which in ("camera", "random"):
        rays = ray_set(prt, emu, name, which)
        eh, eo = emu_records(prt, emu, name, which)
        if door == "host":
            h, o = _words(r.cast_rays(rays)), r.occluded(rays)
        else:
            h, o = _device_cast(r, rays)
        bad = np.nonzero((h != _words(eh)).any(1))[0]
        assert bad.size == 0, "%s, %s rays, %s door: %d records differ from the emulator (first %s)" % (name, which, door, bad.size, bad[:5].tolist())
        assert np.array_equal(o, eo), (name, which, door)
    r.close()


@pytest.mark.gpu
@pytest.mark.parametrize("door", ["host", "device"])
@pytest.mark.parametrize("name", ["cornell_edge", "cornell_diffuse", "cornell_sdf", "cornell_quadlight"])
def test_device_equals_the_emulator(prt, emu, name, door):
    _check_against_emulator(prt, emu, name, door)


@pytest.mark.gpu
def test_many_rays_with_a_ragged_tail(prt, emu):
    name, n = "cornell_diffuse", 65537
    sc, cfg = scene_of(prt, name)
    rays = random_rays(prt, emu, name, n=n, seed=21)
    eh, eo = emu.cast(cfg, sc.desc, rays), emu.occluded(cfg, sc.desc, rays)
    r = _renderer(prt, name, camera=False, size=False)
    assert np.array_equal(_words(r.cast_rays(rays)), _words(eh))
    assert np.array_equal(r.occluded(rays), eo)
    r.close()


@pytest.mark.gpu
def test_cast_pixels_equals_the_guides_depth(prt, emu):
    name = "cornell_diffuse"
    sc, cfg = scene_of(prt, name)
    r = _renderer(prt, name)
    r.render_guides(1)
    g = r.read_guides()
    xy = pixel_grid()
    hits = r.cast_pixels(xy)
    cov = g[..., 3].ravel() == 1.0
    assert cov.mean() > 0.5
    assert np.array_equal(hits["t"].view(np.uint32)[cov], g[..., 7].ravel().view(np.uint32)[cov])
    assert (hits["id"][~cov] == MISS).all()
    assert np.array_equal(_words(hits), _words(emu_records(prt, emu, name, "camera")[0]))
    # pixels outside the frame are misses; the ones inside are unaffected
    some = np.array([[-1, 3], [5, 7], [W, 0], [9, H], [63, 47], [0, -5]], dtype=np.int32)
    got = r.cast_pixels(some)
    assert np.array_equal(_words(got)[[0, 2, 3, 5]], np.tile(MISS_WORDS, (4, 1)))
    assert np.array_equal(_words(got)[[1, 4]], _words(hits)[[7 * W + 5, 47 * W + 63]])
    r.close()
    # the default lens camera: still the centre ray through the middle of the lens
    lens = prt.default_camera(W, H)
    assert lens.apertureRadius > 1e-5
    r = _renderer(prt, name, pinhole=False)
    want = emu.cast(cfg, sc.desc, emu.pixel_rays(lens, W, H, xy))
    assert np.array_equal(_words(r.cast_pixels(xy)), _words(want))
    r.close()


def _displaced(v):
    """the vertices moved by a smooth displacement of 5 % of the mesh's extent"""
    v = np.array(v, dtype=f32).reshape(-1, 4)
    ext = (v[:, :3].max(0) - v[:, :3].min(0)).astype(np.float64)
    p = v[:, :3].astype(np.float64)
    amp = 0.05 * ext.max()
    d = amp * np.stack([np.sin(4 * p[:, 1] + 1), np.sin(5 * p[:, 2] + 2), np.sin(3 * p[:, 0])], 1)
    v[:, :3] = (p + d).astype(f32)
    return v


@pytest.mark.gpu
def test_casts_see_vertex_updates_and_rebuilds(prt, emu):
    name = "cornell_diffuse"
    sc, cfg = scene_of(prt, name)
    a = prt.scene_arrays(sc.desc)
    v = _displaced(a["vertices"])
    rays = np.concatenate([camera_rays(prt, emu), random_rays(prt, emu, name)])
    before = np.concatenate([_words(emu_records(prt, emu, name, w)[0]) for w in ("camera", "random")])
    r = _renderer(prt, name, camera=False, size=False)
    assert np.array_equal(_words(r.cast_rays(rays)), before)
    # the refit: the emulator on a fresh pack of the new vertices in the refitted nodes
    r.update_vertices(v)
    nodes = a["nodes"].copy()
    nodes["bounds"] = r.read_bvh_bounds()
    d = desc_with(prt, sc.desc, vertices=v, bvh_nodes=nodes)
    want = emu.cast(cfg, d, rays)
    got = r.cast_rays(rays)
    assert np.array_equal(_words(got), _words(want))
    assert np.array_equal(r.occluded(rays), emu.occluded(cfg, d, rays))
    assert (_words(got) != before).any(1).mean() > 0.02            # the scene did move
    # the rebuild: ... of the tree prt_read_bvh returns
    r.rebuild_bvh(v)
    nodes2, prims2 = r.read_bvh()
    d2 = desc_with(prt, sc.desc, vertices=v, bvh_nodes=nodes2, bvh_node_count=len(nodes2), primitive_indices=prims2)
    got2 = r.cast_rays(rays)
    assert np.array_equal(_words(got2), _words(emu.cast(cfg, d2, rays)))
    assert np.array_equal(r.occluded(rays), emu.occluded(cfg, d2, rays))
    r.close()
    # tri still names the caller's triangle: the brute-force caster over the caller's arrays
    tri_rays = np.nonzero(got2["id"] == TRIANGLE)[0]
    assert tri_rays.size > 200
    ref = RayCaster(_DescScene(d), cfg).cast(rays[tri_rays, 0:3].astype(np.float64), rays[tri_rays, 4:7].astype(np.float64), rays[tri_rays, 3])
    bad = disagreements(got2[tri_rays], ref)
    assert bad.mean() <= 0.005, (bad.sum(), tri_rays[bad][:5].tolist())
    # ... and the hit point is where its barycentrics put it in the caller's triangle
    h = got2[tri_rays]
    p = v.reshape(-1, 3, 4)[h["tri"], :, :3].astype(np.float64)
    q = p[:, 0] * (1 - h["u"] - h["v"])[:, None] + p[:, 1] * h["u"][:, None] + p[:, 2] * h["v"][:, None]
    assert np.abs(q - h["pos"]).max() < 1e-4


class _DescScene:
    """what Caster reads of a scene: its desc"""
    def __init__(self, desc):
        self.desc = desc


@pytest.mark.gpu
def test_casts_see_primitive_updates(prt, emu):
    name = "cornell_diffuse"
    sc, cfg = scene_of(prt, name)
    n_sph = int(sc.desc.object_count[0])
    m = meshes_of(sc.desc)
    move_sphere(m, 0, dpos=(0.15, -0.2, 0.1), dr=0.05)             # move a sphere
    move_quad(m, n_sph + 1, ang=0.2)                               # turn a quad
    d = desc_with(prt, sc.desc, meshes=m)
    rays = np.concatenate([camera_rays(prt, emu), random_rays(prt, emu, name)])
    before = np.concatenate([_words(emu_records(prt, emu, name, w)[0]) for w in ("camera", "random")])
    r = _renderer(prt, name, camera=False, size=False)
    r.update_primitives(m)
    got = r.cast_rays(rays)
    assert np.array_equal(_words(got), _words(emu.cast(cfg, d, rays)))
    assert np.array_equal(r.occluded(rays), emu.occluded(cfg, d, rays))
    assert (_words(got) != before).any(1).mean() > 0.02
    r.close()


@pytest.mark.gpu
def test_casts_work_on_a_tree_the_refit_refuses(prt, emu):
    """a caller's chain of 300 nested pairs: prt_update_vertices refuses it (one launch per level, at most 256), a cast needs slot_vtx alone"""
    name = "cornell_diffuse"
    sc, cfg = scene_of(prt, name)
    desc, keep = _chain_desc(prt, sc, 300)
    rays = random_rays(prt, emu, name)
    r = prt.Renderer(cfg, device=0)
    r.upload_scene(desc)
    with pytest.raises(prt.PrtError) as ei:
        r.update_vertices(prt.scene_arrays(desc)["vertices"].copy())
    assert ei.value.code == prt.PRT_ERR_UNSUPPORTED
    got = r.cast_rays(rays)
    assert np.array_equal(_words(got), _words(emu.cast(cfg, desc, rays)))
    assert np.array_equal(r.occluded(rays), emu.occluded(cfg, desc, rays))
    pi = prt.scene_arrays(desc)["primitive_indices"]
    tri = got["tri"][got["id"] == TRIANGLE]
    assert tri.size and np.isin(tri, pi[:301]).all()               # the chain's leaves hold the first 301 entries of primitive_indices
    r.close()


def _session(prt, name, cast):
    """4 frames, guides, one temporal denoise, (the casts,) 4 more frames: everything a cast must not touch"""
    sc, cfg = scene_of(prt, name)
    r = _renderer(prt, name)
    seeds = prt.seed_pairs(8)
    r.render_frames(seeds[:8], first_frame=1)
    r.render_guides(2)
    r.denoise_temporal()
    if cast is not None:
        cast(r)
    guides = r.read_guides()                                       # (refused if the guides had gone stale)
    r.render_frames(seeds[8:], first_frame=5)
    out = (r.read_state(), r.read_framebuffer(), guides, r.read_history(), r.kernel_variant())
    r.close()
    return out


@pytest.mark.gpu
def test_a_cast_writes_nothing_of_the_context(prt, emu):
    name = "cornell_diffuse"
    rays = random_rays(prt, emu, name)

    def cast(r):
        h = r.cast_rays(rays)
        assert np.array_equal(_words(h), _words(emu_records(prt, emu, name, "random")[0]))
        r.occluded(rays)
        r.cast_pixels(pixel_grid())
        _device_cast(r, rays)
    a, b = _session(prt, name, cast), _session(prt, name, None)
    for x, y, what in zip(a[:4], b[:4], ("state", "framebuffer", "guides", "history")):
        assert np.array_equal(np.ascontiguousarray(x).view(np.uint8), np.ascontiguousarray(y).view(np.uint8)), what
    assert a[4] == b[4] and a[4]


@pytest.mark.gpu
def test_refusals_leave_the_output_untouched(prt, emu):
    import torch
    name = "cornell_diffuse"
    sc, cfg = scene_of(prt, name)
    lib = prt.load_library()
    rays = np.ascontiguousarray(random_rays(prt, emu, name)[:64])
    n = len(rays)
    hits = np.full((n, 12), 0xA5A5A5A5, dtype=np.uint32)
    occ = np.full(n, 0xA5A5A5A5, dtype=np.uint32)
    xy = pixel_grid()[:n].copy()
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    OK, INVALID_ARGUMENT, NOT_READY = 0, prt.PRT_ERR_INVALID_ARGUMENT, prt.PRT_ERR_NOT_READY

    def untouched():
        return (hits == 0xA5A5A5A5).all() and (occ == 0xA5A5A5A5).all()

    r = prt.Renderer(cfg, device=0)                                # no scene
    assert lib.prt_cast_rays(r.ctx, p(rays), n, p(hits)) == NOT_READY
    assert lib.prt_occluded(r.ctx, p(rays), n, p(occ)) == NOT_READY
    assert lib.prt_cast_pixels(r.ctx, p(xy), n, p(hits)) == NOT_READY
    r.upload_scene(sc)                                             # a scene, no camera, no frame size: casts work, pixels do not
    assert lib.prt_cast_pixels(r.ctx, p(xy), n, p(hits)) == NOT_READY and untouched()
    with pytest.raises(prt.PrtError) as ei:
        r.cast_pixels(xy)
    assert ei.value.code == NOT_READY
    r.set_camera(prt.default_camera(W, H))
    assert lib.prt_cast_pixels(r.ctx, p(xy), n, p(hits)) == NOT_READY and untouched()       # no frame size
    assert lib.prt_cast_rays(r.ctx, None, n, p(hits)) == INVALID_ARGUMENT
    assert lib.prt_cast_rays(r.ctx, p(rays), n, None) == INVALID_ARGUMENT
    assert lib.prt_occluded(r.ctx, None, n, p(occ)) == INVALID_ARGUMENT
    assert lib.prt_occluded(r.ctx, p(rays), n, None) == INVALID_ARGUMENT
    assert lib.prt_cast_rays(r.ctx, p(rays), (1 << 26) + 1, p(hits)) == INVALID_ARGUMENT
    assert lib.prt_occluded(r.ctx, p(rays), (1 << 26) + 1, p(occ)) == INVALID_ARGUMENT
    assert untouched()
    assert lib.prt_cast_rays(r.ctx, p(rays), 0, p(hits)) == OK and lib.prt_occluded(r.ctx, p(rays), 0, p(occ)) == OK
    assert lib.prt_cast_rays(r.ctx, None, 0, None) == OK and untouched()
    d_rays = torch.from_numpy(np.concatenate([rays.ravel(), np.zeros(8, dtype=f32)])).cuda()
    d_hits = torch.full((n * 12 + 8,), 7.0, dtype=torch.float32, device="cuda")
    base_r, base_h = d_rays.data_ptr(), d_hits.data_ptr()
    assert base_r % 16 == 0 and base_h % 16 == 0
    for fn in (lib.prt_cast_rays_device, lib.prt_occluded_device):
        assert fn(r.ctx, C.c_void_p(base_r + 4), n, C.c_void_p(base_h)) == INVALID_ARGUMENT
        assert fn(r.ctx, C.c_void_p(base_r), n, C.c_void_p(base_h + 8)) == INVALID_ARGUMENT
        assert fn(r.ctx, None, n, C.c_void_p(base_h)) == INVALID_ARGUMENT
        assert fn(r.ctx, C.c_void_p(base_r), (1 << 26) + 1, C.c_void_p(base_h)) == INVALID_ARGUMENT
        assert fn(r.ctx, C.c_void_p(base_r), 0, C.c_void_p(base_h)) == OK
    assert (d_hits == 7.0).all().item()
    r.resize(W, H)
    assert lib.prt_cast_pixels(r.ctx, None, n, p(hits)) == INVALID_ARGUMENT and lib.prt_cast_pixels(r.ctx, p(xy), n, None) == INVALID_ARGUMENT
    assert lib.prt_cast_pixels(r.ctx, p(xy), (1 << 26) + 1, p(hits)) == INVALID_ARGUMENT and untouched()
    assert lib.prt_cast_pixels(r.ctx, p(xy), n, p(hits)) == OK and not untouched()
    r.close()


@pytest.mark.gpu
def test_casts_are_refused_after_a_half_failed_render(prt, emu):
    """a render call that failed half-way (faked as in test_gpu_parity.py: option "test_drop_report") leaves the state undefined: the queries
    are refused like every call that goes through ready(), until prt_reset"""
    name = "cornell_diffuse"
    sc, cfg = scene_of(prt, name)
    rays = np.ascontiguousarray(random_rays(prt, emu, name)[:64])
    Wb, Hb, spp = 640, 640, 2
    r = prt.Renderer(cfg, device=0)
    r.upload_scene(sc)
    r.set_camera(prt.default_camera(Wb, Hb))
    r.resize(Wb, Hb)
    r.set_option("test_drop_report", 1)
    with pytest.raises(prt.PrtError):
        r.render_spp(spp, prt.seed_pairs(spp * 16 + 64))
    r.set_option("test_drop_report", 0)
    for call in (lambda: r.cast_rays(rays), lambda: r.occluded(rays), lambda: r.cast_pixels(pixel_grid())):
        with pytest.raises(prt.PrtError) as ei:
            call()
        assert ei.value.code == prt.PRT_ERR_NOT_READY and "half-way" in str(ei.value)
    r.reset()
    assert np.array_equal(_words(r.cast_rays(rays)), _words(emu_records(prt, emu, name, "random")[0])[:64])
    r.close()


@pytest.mark.gpu
def test_cli_pick(prt):
    name = "cornell_diffuse"
    exe = os.path.join(PKG, "prt_render")
    out = subprocess.run([exe, "-scene", os.path.join(ROOT, "scenes", name + ".json"), "-models", os.path.join(ROOT, "scenes", "models") + os.sep,
                          "-pick", "32,24", "-width", str(W), "-height", str(H)], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr[-2000:]
    lines = out.stdout.strip().splitlines()
    assert len(lines) == 1, out.stdout
    m = re.match(r"pick 32,24: id=(-?\d+) tri=(\d+) t=(\S+) pos=(\S+),(\S+),(\S+) normal=(\S+),(\S+),(\S+) ", lines[0])
    assert m, lines[0]
    r = _renderer(prt, name, pinhole=False)                        # the CLI's camera: the default one, lens and all
    h = r.cast_pixels(np.array([[32, 24]], dtype=np.int32))[0]
    r.close()
    assert int(m.group(1)) == h["id"] and int(m.group(2)) == h["tri"]
    got = np.array([float(x) for x in m.groups()[2:]], dtype=f32)
    want = np.concatenate([[h["t"]], h["pos"], h["normal"]]).astype(f32)
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), (lines[0], h)
    assert h["id"] != MISS
