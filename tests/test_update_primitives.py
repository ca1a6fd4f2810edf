"""prt_update_primitives: spheres, quads and SDF primitives moved in place, and their motion in the motion plane (include/prt.h;
csrc/hip/pt_prims.h / .hip, the primitive-motion instances of the guide kernels in pt_denoise.hip).

CPU tests run the bodies of pt_prims.h on the host (tests/emu/prims_emu.cpp) against a float32 numpy mirror, byte for byte.  GPU tests: a render
after an update equals the CPU oracle on the moved scene and a fresh context that uploads it; refusals and the lifetime; the motion plane
against the float64 Caster of tests/mirrors.py, extended by the primitives' previous pose; the per-kind and the snapshot rule; the plumbing; and a
sphere that approaches the camera, whose temporal history follows it only with the plane."""
import ctypes as C
import importlib
import json
import os
import re

import numpy as np
import pytest

from conftest import PKG_NAME, ROOT
from cases import Case, _cmp, deform, desc_with, meshes_of, move_quad, move_sdf, move_sphere, TILT
from mirrors import (camera_basis, centre_dirs, D_BOUND as TRI_D_BOUND, MAT_COND, MAT_DIEL, MAT_ROUGH_COND, MAT_ROUGH_DIEL, _mirror_history,
                     MotionCaster, _point, project, temporal_ref_motion)
from support import assert_api, assert_same_render, bits as _bits, bytes_flat as _bytes, pkg as _pkg, to_device, variant_case


PKG = os.path.join(ROOT, PKG_NAME)
NEW_API = ("prt_update_primitives", "prt_update_primitives_device")
f32 = np.float32
W, H, FRAMES = 64, 48, 8
NAN, INF = f32(np.nan), f32(np.inf)


# ---- no GPU: the API ---------------------------------------------------------------------------------------------------------------------------------

def test_api_is_declared_exported_and_bound():
    header = assert_api(NEW_API)
    assert "What still does not follow: spheres" not in header and "stays prt_upload_scene's job" not in header
    assert callable(getattr(_pkg().Renderer, "update_primitives"))


# ---- no GPU: the bodies of pt_prims.h against a float32 mirror ------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def emu():
    import prims_api
    prims_api.lib()
    return prims_api


def _dot(a, b):
    return (a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1]) + a[..., 2] * b[..., 2]


def mirror_half_ulp(c):
    with np.errstate(invalid="ignore"):
        return np.where((c >= f32(2.0 ** -40)) & (c <= f32(2.0 ** 40)), c * f32(2.0 ** -24), NAN).astype(f32)


def mirror_pack(meshes, n_sph, n_sdf):
    """prt.h prt_update_primitives in float32 numpy: the three tables as float32 rows (the SDF record's word 3 holds t as an integer)"""
    pos, j = meshes["pos"].astype(f32), meshes["joker"].astype(f32)
    sph = np.concatenate([pos[:n_sph, :3], j[:n_sph, 0:1]], 1)
    k = slice(n_sph, n_sph + n_sdf)
    sdf = np.zeros((n_sdf, 8), dtype=f32)
    sdf[:, :3] = pos[k, :3]
    sdf.view(np.uint32)[:, 3] = meshes["t"][k]
    sdf[:, 4:8] = j[k, 0:4]
    q = j[n_sph + n_sdf:]
    base, e0, e1, nrm, area = q[:, 0:3], q[:, 3:6], q[:, 6:9], q[:, 9:12], q[:, 12]
    with np.errstate(all="ignore"):
        anchor = base - (e0 + e1) * f32(0.5)
        e0e0, e1e1 = _dot(e0, e0), _dot(e1, e1)
    quad = np.concatenate([base, area[:, None], e0, e0e0[:, None], e1, e1e1[:, None], nrm, mirror_half_ulp(e0e0)[:, None], anchor,
                           mirror_half_ulp(e1e1)[:, None]], 1).astype(f32)
    return sph, sdf, quad


READ_FIELDS = {"sphere": [("pos", 0), ("pos", 1), ("pos", 2), ("joker", 0)],
               "sdf": [("pos", 0), ("pos", 1), ("pos", 2), ("joker", 0), ("joker", 1), ("joker", 2), ("joker", 3)],
               "quad": [("joker", k) for k in range(13)]}
SDF_TYPES = (4 | 16, 4 | 32, 4 | 64, 4 | 128)


def random_meshes(emu, n_sph, n_sdf, n_quad, seed):
    """records of the three kinds with finite geometry and NaN bit patterns in every byte that is not read"""
    rng = np.random.default_rng(seed)
    n = n_sph + n_sdf + n_quad
    m = np.frombuffer(np.full(n * emu.MESH_BYTES, 0xFF, dtype=np.uint8).tobytes(), dtype=emu.MESH_DTYPE).copy()
    m["pos"][:, :3] = rng.uniform(-3, 3, (n, 3))
    m["joker"][:, :13] = rng.uniform(-2, 2, (n, 13))
    m["t"][:n_sph] = 1
    m["t"][n_sph:n_sph + n_sdf] = np.array(SDF_TYPES, dtype=np.uint8)[rng.integers(0, 4, n_sdf)]
    m["t"][n_sph + n_sdf:] = 8
    return m


def test_pack_body_equals_the_mirror(emu):
    n_sph, n_sdf, n_quad = 3001, 2003, 4007
    m = random_meshes(emu, n_sph, n_sdf, n_quad, 3)
    q0 = n_sph + n_sdf
    m["joker"][0, 0] = 0.0                                      # a zero radius
    m["pos"][1, :3] = (-0.0, 0.0, -0.0)
    m["joker"][q0, 3:6] = 0.0                                   # a zero edge: u0 is NaN
    m["joker"][q0 + 1, 3:6] = (1e-7, 0.0, -0.0)                 # e0e0 below 2^-40
    m["joker"][q0 + 2, 6:9] = (3e6, 0.0, 0.0)                   # e1e1 above 2^40
    m["joker"][q0 + 3, 0:3] = (-0.0, -0.0, 0.0)
    m["joker"][q0 + 4, 3:6] = (2.0 ** -20, 0.0, 0.0)            # e0e0 = 2^-40 exactly: inside
    m["joker"][q0 + 5, 6:9] = (2.0 ** 20, 0.0, 0.0)             # e1e1 = 2^40 exactly: inside
    sph, sdf, quad, bad = emu.pack(m, n_sph, n_sdf, m["t"])
    assert not bad.any()
    wsph, wsdf, wquad = mirror_pack(m, n_sph, n_sdf)
    assert np.array_equal(_bytes(sph), _bytes(wsph))
    assert np.array_equal(_bytes(sdf), _bytes(wsdf))
    assert np.array_equal(_bytes(quad), _bytes(wquad))
    assert np.isnan(quad[0, 15]) and np.isnan(quad[1, 15]) and np.isnan(quad[2, 19])
    assert not np.isnan(quad[4, 15]) and not np.isnan(quad[5, 19])
    # a scene with one kind only, and with none
    for counts in ((5, 0, 0), (0, 5, 0), (0, 0, 5), (0, 0, 0)):
        mm = random_meshes(emu, *counts, seed=4)
        got = emu.pack(mm, counts[0], counts[1], mm["t"])
        want = mirror_pack(mm, counts[0], counts[1])
        for g, w_ in zip(got[:3], want):
            assert np.array_equal(_bytes(g), _bytes(w_)), counts


def test_refusal_flag(emu):
    n_sph, n_sdf, n_quad = 7, 6, 9
    m = random_meshes(emu, n_sph, n_sdf, n_quad, 5)
    first = {"sphere": 0, "sdf": n_sph, "quad": n_sph + n_sdf}
    for kind, fields in READ_FIELDS.items():
        i = first[kind] + 3
        for v in (NAN, INF, -INF):
            for name, k in fields:
                mm = m.copy()
                mm[name][i, k] = v
                bad = emu.pack(mm, n_sph, n_sdf, m["t"])[3]
                assert bad[i] and bad.sum() == 1, (kind, name, k, v)
        mm = m.copy()
        mm["t"][i] ^= 64
        bad = emu.pack(mm, n_sph, n_sdf, m["t"])[3]
        assert bad[i] and bad.sum() == 1, kind
        # what is not read: mat, the paddings, pos[3], the joker entries behind the kind's own, a quad's pos
        mm = m.copy()
        mm["mat"][i] = 0xFF
        mm["_pad0"][i] = 0xFF
        mm["_pad1"][i] = 0xFF
        mm["pos"][i, 3] = NAN
        read_j = sum(1 for name, _ in fields if name == "joker")
        mm["joker"][i, read_j:] = NAN
        assert read_j <= 13
        mm["joker"][i, 13:] = INF
        if kind == "quad":
            mm["pos"][i] = NAN
        assert not emu.pack(mm, n_sph, n_sdf, m["t"])[3].any(), kind


def mirror_sphere(prev, cur, p):
    with np.errstate(all="ignore"):
        w = p - cur[:, :3]
        ln = np.sqrt(_dot(w, w))
        return ((prev[:, :3] - cur[:, :3]) + (w / ln[:, None]) * (prev[:, 3] - cur[:, 3])[:, None]).astype(f32)


def mirror_quad_point(rec, a, b):
    return (rec[:, 16:19] + rec[:, 4:7] * a[:, None]) + rec[:, 8:11] * b[:, None]


def mirror_quad(prev, cur, p):
    with np.errstate(all="ignore"):
        w = p - cur[:, 16:19]
        a, b = _dot(w, cur[:, 4:7]) / cur[:, 7], _dot(w, cur[:, 8:11]) / cur[:, 11]
        return (mirror_quad_point(prev, a, b) - mirror_quad_point(cur, a, b)).astype(f32)


def mirror_sdf(prev, cur):
    return (prev[:, :3] - cur[:, :3]).astype(f32)


def _hit_cases(emu, seed=7, n=4096):
    """n records of each kind in two poses with a real hit point on the current one: a point of the sphere, (a, b) in [0, 1] of the quad"""
    rng = np.random.default_rng(seed)
    cur_m, prev_m = random_meshes(emu, n, n, n, seed), random_meshes(emu, n, n, n, seed + 1)
    cur_m["joker"][:n, 0] = np.abs(cur_m["joker"][:n, 0]) + f32(0.05)
    prev_m["t"] = cur_m["t"]
    still = np.arange(0, n, 8)                                  # every eighth record of each kind does not move
    for k in range(3):
        prev_m[k * n + still] = cur_m[k * n + still]
    cur, prev = mirror_pack(cur_m, n, n), mirror_pack(prev_m, n, n)
    d = rng.normal(size=(n, 3))
    d = (d / np.linalg.norm(d, axis=1, keepdims=True)).astype(f32)
    p_sph = (cur[0][:, :3] + d * cur[0][:, 3:4]).astype(f32)
    a, b = rng.uniform(0, 1, n).astype(f32), rng.uniform(0, 1, n).astype(f32)
    a[:4], b[:4] = (0, 1, 0, 1), (0, 0, 1, 1)
    p_quad = mirror_quad_point(cur[2], a, b).astype(f32)
    return cur, prev, p_sph, p_quad, still


def test_displacement_bodies_equal_the_mirror(emu):
    cur, prev, p_sph, p_quad, still = _hit_cases(emu)
    n = len(p_sph)
    idx = np.arange(n, dtype=np.uint32)
    perm = np.random.default_rng(1).permutation(n).astype(np.uint32)          # (the bodies index the tables: not in table order)
    got = emu.sphere_displacement(prev[0], cur[0], perm, p_sph[perm])
    assert np.array_equal(_bits(got), _bits(mirror_sphere(prev[0], cur[0], p_sph)[perm]))
    assert (_bits(emu.sphere_displacement(prev[0], cur[0], idx, p_sph)[still]) == 0).all(), "an unchanged sphere: +0"
    got = emu.quad_displacement(prev[2], cur[2], perm, p_quad[perm])
    assert np.array_equal(_bits(got), _bits(mirror_quad(prev[2], cur[2], p_quad)[perm]))
    assert (_bits(emu.quad_displacement(prev[2], cur[2], idx, p_quad)[still]) == 0).all(), "an unchanged quad: +0"
    got = emu.sdf_displacement(prev[1], cur[1], perm)
    assert np.array_equal(_bits(got), _bits(mirror_sdf(prev[1], cur[1])[perm]))
    assert (_bits(emu.sdf_displacement(prev[1], cur[1], idx)[still]) == 0).all(), "an unchanged SDF primitive: +0"
    assert (np.abs(got).max(1) > 0).mean() > 0.8


def mirror_pixel(d, hit, contributing):
    s, n, hits = np.zeros(3, dtype=f32), 0, 0
    for k in range(len(hit)):
        if not hit[k]:
            continue
        hits += 1
        if contributing[k]:
            s = (s + d[k]).astype(f32)
            n += 1
    if hits == 0:
        return np.zeros(4, dtype=f32)
    return np.concatenate([s / f32(hits), [f32(n) * (f32(1.0) / f32(len(hit)))]]).astype(f32)


@pytest.mark.parametrize("K", [1, 4, 64])
def test_pixel_reduction_equals_the_mirror(emu, K):
    """samples of mixed kinds (misses, triangles, spheres, SDF primitives, quads; some behind a delta event) under the four combinations of
    pending snapshots: the per-kind rule and the reduction of pt_motion.h"""
    cur, prev, p_sph, p_quad, _ = _hit_cases(emu, seed=11, n=64)
    n = 64
    rng = np.random.default_rng(K)
    for trial in range(24):
        kind = rng.integers(-2, 3, K)                          # -2 miss, -1 triangle, 0 sphere, 1 SDF, 2 quad
        rec = rng.integers(0, n, K)
        first = rng.uniform(size=K) < 0.8
        mid = np.where(kind < 0, kind, kind * n + rec).astype(np.int32)
        p = np.where((kind == 2)[:, None], p_quad[rec], p_sph[rec]).astype(f32)
        tri_d = rng.uniform(-1, 1, (K, 3)).astype(f32)
        d = np.zeros((K, 3), dtype=f32)
        for k in range(K):
            r = rec[k:k + 1]
            if kind[k] == -1:
                d[k] = tri_d[k]
            elif kind[k] == 0:
                d[k] = mirror_sphere(prev[0][r], cur[0][r], p[k:k + 1])[0]
            elif kind[k] == 1:
                d[k] = mirror_sdf(prev[1][r], cur[1][r])[0]
            elif kind[k] == 2:
                d[k] = mirror_quad(prev[2][r], cur[2][r], p[k:k + 1])[0]
        for tri_snap in (0, 1):
            for prim_snap in (0, 1):
                con = first & (((kind == -1) & bool(tri_snap)) | ((kind >= 0) & bool(prim_snap)))
                want = mirror_pixel(d, kind > -2, con)
                got = emu.pixel((prev[0], cur[0]), (prev[1], cur[1]), (prev[2], cur[2]), mid, first, p, tri_d, tri_snap, prim_snap)
                assert np.array_equal(_bits(got), _bits(want)), (K, trial, tri_snap, prim_snap)
                if not tri_snap and not prim_snap:
                    assert (_bits(got) == 0).all()


def test_sanitizer_program(emu, tmp_path):
    """the stand-alone program of prims_emu.cpp (its own main: random records, the edge cases, every refusal, the displacements and the
    reduction) under -fsanitize=address,undefined on the CPU"""
    import subprocess
    exe = emu.build_main(str(tmp_path / "prims_emu_main"))
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0 and "0 mismatches" in r.stdout, r.stdout[-2000:]


def test_pack_kernel_has_no_scratch():
    """prims_pack_kernel for gfx950: no scratch, no LDS (the primitive-motion instances of the guide kernels are held to no scratch by
    test_denoise.py::test_denoise_kernels_have_no_scratch, which compiles all of pt_denoise.hip)"""
    import subprocess
    hip = os.path.join(PKG, "csrc", "hip")
    cmd = [os.environ.get("HIPCC", "/opt/rocm/bin/hipcc"), "--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=off", "-fno-fast-math",
           "-fno-slp-vectorize", "-c", "--cuda-device-only", "-I" + os.path.join(ROOT, "include"), "-I" + hip, "-Rpass-analysis=kernel-resource-usage",
           "-o", os.devnull, os.path.join(hip, "pt_prims.hip")]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-4000:]
    assert "prims_pack_kernel" in r.stderr
    assert re.findall(r"ScratchSize \[bytes/lane\]: (\d+)", r.stderr) == ["0"] and re.findall(r"LDS Size \[bytes/block\]: (\d+)", r.stderr) == ["0"]


# ---- moved scenes ----------------------------------------------------------------------------------------------------------------------------------------

def moves_mixed(m, which="B"):
    """cornell_mixed: 4 spheres (0 the light, 1 a mirror, 2 glass, 3 rough glass), quads 4 .. 9 (4 the floor, 7 the back wall)"""
    s = 1.0 if which == "B" else -0.6
    move_sphere(m, 3, (0.10 * s, 0.05 * s, -0.12 * s), 0.05 * s)
    move_quad(m, 7, (0.05 * s, -0.04 * s, 0.10 * s), TILT, 0.06 * s)
    move_quad(m, 4, (0.0, 0.03 * s, 0.0))
    move_sphere(m, 0, (0.20 * s, -0.10 * s, 0.10 * s))         # the light


def moves_quadlight(m, which="B"):
    """cornell_quadlight: sphere 0, quad 1 the light (its area is sampled), quads 2 .. 7 the box"""
    s = 1.0 if which == "B" else -0.6
    move_sphere(m, 0, (-0.15 * s, 0.05 * s, 0.10 * s), -0.05 * s)
    move_quad(m, 1, (0.30 * s, -0.05 * s, 0.20 * s), TILT, 0.1 * s, scale=1.0 + 0.25 * s)
    move_quad(m, 5, (0.0, 0.0, 0.05 * s), TILT, 0.03 * s)


def moves_sdf(m, which="B"):
    """cornell_sdf: sphere 0 the light, SDF primitives 1 .. 4 (sphere, box, round box, plane), quads 5 .. 10"""
    s = 1.0 if which == "B" else -0.6
    move_sdf(m, 1, (0.10 * s, 0.05 * s, -0.08 * s))
    move_sdf(m, 2, (-0.12 * s, 0.02 * s, 0.05 * s))
    move_sdf(m, 3, (0.0, 0.04 * s, 0.10 * s))
    move_sphere(m, 0, (-0.20 * s, -0.10 * s, 0.05 * s))


def _prims_only_text():
    with open(os.path.join(ROOT, "scenes", "cornell_mixed.json")) as f:
        s = json.load(f)
    del s["scene"]["obj"]
    return json.dumps(s)


def _front_sphere_text(radius=0.4, pos=(0.0, 1.0, 1.2)):
    """cornell_diffuse with a diffuse sphere (mesh 1) in front of the teapot"""
    with open(os.path.join(ROOT, "scenes", "cornell_diffuse.json")) as f:
        s = json.load(f)
    s["scene"]["spheres"].append({"pos": list(pos), "radius": radius, "material": {"color": [0.3, 0.5, 0.9], "type": 1}})
    return json.dumps(s)


class Moved:
    """a scene, its primitive records as uploaded (m0) and in two moved poses A and B, with the descs that hold them; shared and never written to"""
    _cache = {}
    SCENES = {"cornell_mixed": moves_mixed, "cornell_quadlight": moves_quadlight, "cornell_sdf": moves_sdf, "prims_only": moves_mixed}

    def __new__(cls, prt, name):
        if name not in cls._cache:
            self = super().__new__(cls)
            self.prt, self.name = prt, name
            if name == "prims_only":
                self.scene = prt.HostScene(_prims_only_text(), text=True)
                self.cfg, self.cam, self.env = self.scene.config(), prt.default_camera(W, H), prt.make_sky(64, 32)
            else:
                self.scene, self.cfg, self.cam, self.env = variant_case(prt, name, W, H)
            self.desc = self.scene.desc
            self.m0 = meshes_of(self.desc)
            self.mA, self.mB = self.m0.copy(), self.m0.copy()
            cls.SCENES[name](self.mA, "A")
            cls.SCENES[name](self.mB, "B")
            for a in (self.m0, self.mA, self.mB):
                a.setflags(write=False)
            self.descA, self.descB = desc_with(prt, self.desc, self.mA), desc_with(prt, self.desc, self.mB)
            self._oracle = {}
            cls._cache[name] = self
        return cls._cache[name]

    def context(self, desc=None):
        r = self.prt.Renderer(self.cfg, device=0)
        r.upload_scene(desc if desc is not None else self.desc)
        if self.env is not None:
            r.upload_envmap(self.env)
        r.set_camera(self.cam)
        r.resize(W, H)
        return r

    def render(self, r):
        r.reset()
        r.render_frames(self.prt.seed_pairs(FRAMES))
        return r.read_state(), r.read_framebuffer()

    def oracle_render(self, oracle, key, desc):
        if key not in self._oracle:
            st, img = oracle.Restatement().render(self.cfg, desc, self.cam, W, H, self.prt.seed_pairs(FRAMES), env=self.env, threads=8)
            st.setflags(write=False)
            img.setflags(write=False)
            self._oracle[key] = (st, img)
        return self._oracle[key]


def _assert_same(oracle, want, got, what):
    assert_same_render(oracle, want[0], want[1], got[0], got[1], what)


def _to_device(meshes):
    return to_device(np.ascontiguousarray(meshes).view(np.uint8).copy())


def _update(r, meshes, door):
    if door == "host":
        r.update_primitives(meshes)
    else:
        r.update_primitives(_to_device(meshes))


# ---- on the GPU: update equals upload equals oracle ------------------------------------------------------------------------------------------------------

@pytest.mark.gpu
@pytest.mark.parametrize("name", ["cornell_mixed", "cornell_quadlight", "cornell_sdf", "prims_only"])
def test_update_equals_upload_equals_oracle(prt, oracle, name):
    sc = Moved(prt, name)
    assert (name == "prims_only") == (sc.desc.triangle_count == 0)
    want = sc.oracle_render(oracle, "B", sc.descB)
    still = sc.oracle_render(oracle, "0", sc.desc)
    assert not oracle.images_equal(want[1], still[1]), "the move changes the picture"
    fresh = sc.context(sc.descB)
    _assert_same(oracle, want, sc.render(fresh), name + ": a fresh context on the moved scene")
    fresh.close()
    for door in ("host", "device"):
        r = sc.context()
        _update(r, sc.mB, door)
        _assert_same(oracle, want, sc.render(r), "%s: after update_primitives (%s)" % (name, door))
        r.close()


@pytest.mark.gpu
def test_a_then_b_equals_b_and_back(prt, oracle):
    sc = Moved(prt, "cornell_mixed")
    r = sc.context()
    r.update_primitives(sc.mA)
    _assert_same(oracle, sc.oracle_render(oracle, "A", sc.descA), sc.render(r), "A")
    r.update_primitives(sc.mB)
    _assert_same(oracle, sc.oracle_render(oracle, "B", sc.descB), sc.render(r), "A then B")
    r.update_primitives(sc.m0)
    _assert_same(oracle, sc.oracle_render(oracle, "0", sc.desc), sc.render(r), "back to the uploaded meshes")
    # a ctypes array of Mesh, as a HostScene.desc holds it
    arr = (prt._capi.Mesh * len(sc.mB)).from_buffer_copy(sc.mB.tobytes())
    r.update_primitives(arr)
    _assert_same(oracle, sc.oracle_render(oracle, "B", sc.descB), sc.render(r), "a ctypes array")
    r.close()


def _code(fn, *a, **k):
    try:
        fn(*a, **k)
    except _pkg().PrtError as e:
        return e.code
    return 0


@pytest.mark.gpu
def test_refusals_leave_the_scene_and_the_snapshot(prt, oracle):
    import torch
    sc = Moved(prt, "cornell_sdf")                             # (all three kinds)
    n = len(sc.m0)
    r = prt.Renderer(sc.cfg, device=0)
    assert r.lib.prt_update_primitives(r.ctx, sc.mB.ctypes.data_as(C.c_void_p), n) == prt.PRT_ERR_NOT_READY
    assert r.lib.prt_update_primitives_device(r.ctx, C.c_void_p(_to_device(sc.mB).data_ptr()), n) == prt.PRT_ERR_NOT_READY
    r.close()
    bad_cases = {}
    for label, i, name, k, v in (("sphere pos", 0, "pos", 1, NAN), ("sphere radius", 0, "joker", 0, INF), ("sdf pos", 2, "pos", 0, -INF),
                                 ("sdf param", 3, "joker", 3, NAN), ("quad edge", 7, "joker", 4, NAN), ("quad area", 6, "joker", 12, INF)):
        m = sc.mB.copy()
        m[name][i, k] = v
        bad_cases[label] = m
    m = sc.mB.copy()
    m["t"][2] = 4 | 64                                          # the SDF box becomes a round box
    bad_cases["sdf sub-type"] = m
    m = sc.mB.copy()
    m["t"][0] = 8
    bad_cases["kind"] = m
    unread = sc.mB.copy()
    unread["mat"][:] = 0xFF
    unread["_pad0"][:] = 0xFF
    unread["_pad1"][:] = 0xFF
    unread["pos"][:, 3] = NAN
    unread["joker"][:, 13:] = NAN
    unread["joker"][0, 1:] = NAN
    unread["joker"][1:5, 4:] = NAN
    unread["pos"][5:] = NAN                                     # (a quad's pos)
    r = sc.context()
    r.set_motion(True)
    r.update_primitives(sc.mA)
    r.render_guides(1)
    before = sc.render(r)
    r.update_primitives(sc.mB)                                  # a snapshot (of A) is pending from here on
    after = sc.render(r)
    _assert_same(oracle, sc.oracle_render(oracle, "B", sc.descB), after, "B")
    dev_ok = _to_device(sc.mB)
    refusals = [("null host", lambda: r.lib.prt_update_primitives(r.ctx, None, n)), ("null device", lambda: r.lib.prt_update_primitives_device(r.ctx, None, n)),
                ("count + 1", lambda: r.lib.prt_update_primitives(r.ctx, sc.mA.ctypes.data_as(C.c_void_p), n + 1)),
                ("count 0", lambda: r.lib.prt_update_primitives_device(r.ctx, C.c_void_p(dev_ok.data_ptr()), 0)),
                ("misaligned", lambda: r.lib.prt_update_primitives_device(r.ctx, C.c_void_p(dev_ok.data_ptr() + 4), n))]
    for label, m in bad_cases.items():
        refusals.append((label + " (host)", lambda m=m: _code(r.update_primitives, m)))
        refusals.append((label + " (device)", lambda m=m: _code(r.update_primitives, _to_device(m))))
    for label, call in refusals:
        assert call() == prt.PRT_ERR_INVALID_ARGUMENT, label
    _assert_same(oracle, after, sc.render(r), "after %d refused updates" % len(refusals))
    r.render_guides(1)
    plane = r.read_motion()
    # ... and an unrefused run: the plane measures from A to B
    q = sc.context()
    q.set_motion(True)
    q.update_primitives(sc.mA)
    q.render_guides(1)
    q.update_primitives(sc.mB)
    q.render_guides(1)
    want_plane = q.read_motion()
    q.close()
    assert (_bits(plane) == _bits(want_plane)).all() and (_bits(plane[..., :3]) != 0).any()
    # a refused update with no snapshot pending takes none
    assert _code(r.update_primitives, bad_cases["quad edge"]) == prt.PRT_ERR_INVALID_ARGUMENT
    r.render_guides(1)
    assert (_bits(r.read_motion()) == 0).all()
    # non-finite values in fields that are not read are not a refusal
    for door in ("host", "device"):
        r.update_primitives(sc.mA)
        _update(r, unread, door)
        _assert_same(oracle, after, sc.render(r), "unread fields (%s)" % door)
    r.close()
    assert not oracle.images_equal(before[1], after[1])


@pytest.mark.gpu
def test_count_zero_on_a_scene_without_primitives(prt):
    """the teapot of cornell_mixed alone, lit by the sky: count == 0 succeeds and does nothing"""
    sc = Moved(prt, "cornell_mixed")
    cfg = type(sc.cfg).from_buffer_copy(bytes(sc.cfg))
    cfg.light_count = 0
    d = desc_with(prt, sc.desc)
    for k in range(8):
        d.object_count[k] = 0
    d.meshes = None
    r = prt.Renderer(cfg, device=0)
    r.upload_scene(d)
    r.upload_envmap(sc.env)
    r.set_camera(sc.cam)
    r.resize(W, H)
    before = sc.render(r)
    assert r.lib.prt_update_primitives(r.ctx, None, 0) == 0
    assert r.lib.prt_update_primitives_device(r.ctx, None, 0) == 0
    assert r.lib.prt_update_primitives(r.ctx, sc.m0.ctypes.data_as(C.c_void_p), len(sc.m0)) == prt.PRT_ERR_INVALID_ARGUMENT
    after = sc.render(r)
    r.close()
    assert np.array_equal(_bytes(before[0]), _bytes(after[0])) and np.array_equal(_bytes(before[1]), _bytes(after[1]))


@pytest.mark.gpu
def test_lifetime(prt, oracle):
    sc = Moved(prt, "cornell_mixed")
    r = sc.context()
    r.render_frames(prt.seed_pairs(FRAMES))
    variant = r.kernel_variant()
    r.render_guides(2)
    r.denoise_temporal(passes=1)
    hist, fb, state = r.read_history(), r.read_framebuffer(), r.read_state()
    r.read_guides()
    r.update_primitives(sc.mB)
    assert _code(r.read_guides) == prt.PRT_ERR_NOT_READY
    assert np.array_equal(_bytes(r.read_history()), _bytes(hist)), "the history is kept"
    assert np.array_equal(_bytes(r.read_framebuffer()), _bytes(fb)), "the framebuffer is unchanged until the next render"
    assert np.array_equal(_bytes(r.read_state()), _bytes(state)), "the path state is kept"
    _assert_same(oracle, sc.oracle_render(oracle, "B", sc.descB), sc.render(r), "render after the lifetime checks")
    assert r.kernel_variant() == variant
    # the tables survive each other: a refit, then a primitive update, then a rebuild, each against the oracle
    case = Case(prt, "cornell_mixed", seed=11, scene=sc.scene)
    r.update_vertices(case.v, case.n)
    d = desc_with(prt, case.new_desc, sc.mB)
    d._keep += [case.v, case.n, case.nodes]
    _assert_same(oracle, sc.oracle_render(oracle, "B + refit", d), sc.render(r), "update_primitives then update_vertices")
    r.update_primitives(sc.mA)
    d = desc_with(prt, case.new_desc, sc.mA)
    _assert_same(oracle, sc.oracle_render(oracle, "A + refit", d), sc.render(r), "update_vertices then update_primitives")
    r.rebuild_bvh(case.v, case.n, 4)
    nodes, prims = r.read_bvh()
    d = desc_with(prt, case.new_desc, sc.mA, bvh_nodes=nodes, primitive_indices=prims, bvh_node_count=len(nodes))
    _assert_same(oracle, sc.oracle_render(oracle, "A + rebuild", d), sc.render(r), "rebuild_bvh after update_primitives")
    r.update_primitives(sc.mB)
    d = desc_with(prt, case.new_desc, sc.mB, bvh_nodes=nodes, primitive_indices=prims, bvh_node_count=len(nodes))
    _assert_same(oracle, sc.oracle_render(oracle, "B + rebuild", d), sc.render(r), "update_primitives after rebuild_bvh")
    r.close()


# ---- on the GPU: the motion plane --------------------------------------------------------------------------------------------------------------------

# the largest |D - caster's D| over the matching pixels measured on an MI355X (cornell_mixed and the front-sphere scene at 64x48; DESIGN.md s4
# "Moving primitives"), and the bound: 4 x that -- never looser than 1e-3 of the smallest moved primitive's size (a sphere's radius, a quad's
# shorter edge), under which a wrong record or swapped edges cannot fit
PRIM_D_MEASURED = 5.7e-6        # (cornell_mixed; the front-sphere scene: 2.2e-6)
PRIM_D_BOUND = 4 * PRIM_D_MEASURED


class _SceneLike:
    def __init__(self, desc):
        self.desc = desc


def _delta(tb):
    return bool(((tb & MAT_COND) and not (tb & MAT_ROUGH_COND)) or ((tb & MAT_DIEL) and not (tb & MAT_ROUGH_DIEL)))


class PrimCaster(MotionCaster):
    """mirrors.MotionCaster on the CURRENT scene (moved primitives, given vertices), extended by the primitives' previous pose: plane()
    is prt.h's {D, m} of the pinhole centre rays in float64.  sphere: c_prev + (p - c) r_prev / r - p; quad: through (a, b)"""

    def __init__(self, prt, sc_desc, cfg, m_cur, m_prev, v_cur, v_prev):
        cur_desc = desc_with(prt, sc_desc, np.ascontiguousarray(m_cur))
        super().__init__(_SceneLike(cur_desc), cfg, v_cur if v_cur is not None else np.zeros((0, 4)))
        self.m_cur, self.m_prev = m_cur, m_prev
        self.v_prev = None if v_prev is None else np.asarray(v_prev, dtype=np.float64).reshape(-1, 3, 4)[..., :3]
        self.cnt = list(sc_desc.object_count)

    def plane(self, cam, Wf, Hf, tri_snap, prim_snap):
        mesh, tri, u, v, mid, hit, t, behind = self.first_hits(cam, Wf, Hf)
        B = camera_basis(cam)
        d = centre_dirs(B, Wf, Hf)
        p = B[0] + d * t[..., None]
        D = np.zeros((Hf, Wf, 3))
        m = np.zeros((Hf, Wf))
        if tri_snap:
            D = np.where(mesh[..., None], _point(self.v_prev, tri, u, v) - _point(self.vtx, tri, u, v), D)
            m = np.where(mesh, 1.0, m)
        kind = np.full((Hf, Wf), -1)
        if prim_snap:
            n_sph, n_sdf = self.cnt[0], self.cnt[1]
            for i in range(self.cnt[7]):
                px = hit & (mid == i)
                if not px.any() or _delta(self.mats[i][1]):
                    continue
                m = np.where(px, 1.0, m)
                kind = np.where(px, i, kind)
                cur, prev = self.m_cur[i], self.m_prev[i]
                if cur.tobytes() == prev.tobytes():
                    continue                                    # (an unchanged record: exactly 0, not this expression's rounding)
                if i < n_sph:
                    c, cp = cur["pos"][:3].astype(np.float64), prev["pos"][:3].astype(np.float64)
                    r, rp = float(cur["joker"][0]), float(prev["joker"][0])
                    Di = cp + (p - c) * (rp / r) - p
                elif i < n_sph + n_sdf:
                    Di = np.broadcast_to(prev["pos"][:3].astype(np.float64) - cur["pos"][:3].astype(np.float64), p.shape)
                else:
                    jc, jp = cur["joker"].astype(np.float64), prev["joker"].astype(np.float64)
                    an_c, an_p = jc[0:3] - (jc[3:6] + jc[6:9]) * 0.5, jp[0:3] - (jp[3:6] + jp[6:9]) * 0.5
                    w_ = p - an_c
                    a, b = (w_ @ jc[3:6]) / (jc[3:6] @ jc[3:6]), (w_ @ jc[6:9]) / (jc[6:9] @ jc[6:9])
                    Di = (an_p + jp[3:6] * a[..., None] + jp[6:9] * b[..., None]) - (an_c + jc[3:6] * a[..., None] + jc[6:9] * b[..., None])
                D = np.where(px[..., None], Di, D)
        return dict(D=D, m=m, mesh=mesh, mid=mid, hit=hit, kind=kind)


def _size(m, moved):
    """the smallest size among the moved primitives `moved` of the records m: a sphere's radius, a quad's shorter edge"""
    out = []
    for i in moved:
        j = m["joker"][i].astype(np.float64)
        out.append(abs(j[0]) if m["t"][i] == 1 else min(np.linalg.norm(j[3:6]), np.linalg.norm(j[6:9])))
    return min(out)


def _check_plane(plane, want, size, what):
    """the device's K = 1 plane against the caster's: at most 0.5 % of the pixels may differ in m or by more than 1e-3 of the primitive's size;
    returns the largest deviation of D over the matching pixels and the share of pixels that move"""
    m, D = plane[..., 3], plane[..., :3].astype(np.float64)
    assert ((m == 0) | (m == 1)).all(), what
    dev = np.abs(D - want["D"]).max(-1)
    match = ((m > 0) == (want["m"] > 0)) & (dev <= 1e-3 * size)
    assert (~match).mean() <= 0.005, "%s: %.2f %% of the pixels differ from the caster" % (what, 100 * (~match).mean())
    assert (D[m == 0] == 0).all(), what
    moving = (m > 0) & (_bits(plane[..., :3]) != 0).any(-1)
    return float(dev[match].max()), float(moving.mean())


class MotionScene:
    """a scene with a pinhole camera, its records as uploaded and moved, the teapot's vertices as uploaded and deformed (seed 11), and the
    caster's planes; computed once, shared, never written to"""
    _cache = {}

    def __new__(cls, prt, name):
        if name not in cls._cache:
            self = super().__new__(cls)
            self.prt, self.name = prt, name
            if name == "front_sphere":
                self.scene = prt.HostScene(_front_sphere_text(), text=True)
            else:
                self.scene = prt.HostScene(name + ".json")
            self.cfg = self.scene.config()
            self.cam = prt.default_camera(W, H)
            self.cam.apertureRadius = 0.0
            self.env = prt.make_sky(64, 32)
            self.m0 = meshes_of(self.scene.desc)
            self.mB = self.m0.copy()
            if name == "front_sphere":
                move_sphere(self.mB, 1, (0.15, -0.08, 0.20), 0.06)
                move_quad(self.mB, 5, (0.0, 0.0, 0.06), TILT, 0.04)          # the back wall
                self.moved = (1, 5)
            elif name == "cornell_mixed":
                moves_mixed(self.mB)
                move_sphere(self.mB, 1, (0.1, 0.0, 0.05))                    # the mirror moves too: it carries no motion
                self.moved = (3, 7, 4, 0)
            else:
                moves_sdf(self.mB)
                self.moved = (0,)
            a = prt.scene_arrays(self.scene.desc)
            self.v0, self.n0 = a["vertices"].copy(), a["normals"].copy()
            self.vB, self.nB = deform(self.v0, self.n0, 11)
            for arr in (self.m0, self.mB, self.v0, self.n0, self.vB, self.nB):
                arr.setflags(write=False)
            self.size = _size(self.m0, self.moved)
            self._planes = {}
            cls._cache[name] = self
        return cls._cache[name]

    def caster_plane(self, tri, prim):
        """the caster's plane after the updates named: tri (the vertices went from v0 to vB), prim (the records from m0 to mB)"""
        key = (tri, prim)
        if key not in self._planes:
            c = PrimCaster(self.prt, self.scene.desc, self.cfg, self.mB if prim else self.m0, self.m0, self.vB if tri else self.v0, self.v0)
            self._planes[key] = c.plane(self.cam, W, H, tri, prim)
        return self._planes[key]

    def context(self, motion=True, part=None, pixel_filter=None, size=(W, H)):
        r = self.prt.Renderer(self.cfg, device=0)
        r.upload_scene(self.scene)
        if pixel_filter is not None:
            r.set_pixel_filter(*pixel_filter)
        r.upload_envmap(self.env)
        cam = self.cam
        if size != (W, H):
            cam = self.prt.default_camera(*size)
            cam.apertureRadius = 0.0
        r.set_camera(cam)
        if part is None:
            r.resize(*size)
        elif part[0] == "tile":
            r.set_tile(size[0], size[1], part[1], part[2])
        else:
            r.set_row_blocks(size[0], size[1], part[1], 2, part[2])
        if motion:
            r.set_motion(True)
        return r


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["cornell_mixed", "front_sphere"])
def test_plane_matches_the_caster(prt, name):
    ms = MotionScene(prt, name)
    r = ms.context()
    r.update_primitives(ms.mB)
    r.render_guides(1)
    plane = r.read_motion()
    r.close()
    worst, moving = _check_plane(plane, ms.caster_plane(False, True), ms.size, name)
    print("primitive motion plane, %s %dx%d: largest |D - caster| over the matching pixels %.3e (bound %.3e, cap %.3e); %.1f %% of the pixels move"
          % (name, W, H, worst, PRIM_D_BOUND, 1e-3 * ms.size, 100 * moving))
    assert PRIM_D_BOUND <= 1e-3 * ms.size
    assert moving >= 0.05
    assert worst <= PRIM_D_BOUND, worst


@pytest.mark.gpu
def test_per_kind_rule(prt):
    ms = MotionScene(prt, "cornell_mixed")
    only_prims, both, only_tris = ms.caster_plane(False, True), ms.caster_plane(True, True), ms.caster_plane(True, False)
    r = ms.context()
    # primitives only: triangle pixels have zero bits
    r.update_primitives(ms.mB)
    r.render_guides(1)
    plane = r.read_motion()
    g = r.read_guides()
    _check_plane(plane, only_prims, ms.size, "primitives only")
    tri_px = only_prims["mesh"]
    assert tri_px.sum() >= 100
    assert (tri_px & (_bits(plane) != 0).any(-1)).mean() <= 0.005
    # a moved mirror sphere: its pixels carry no motion (the silhouette aside)
    mirror = only_prims["hit"] & (only_prims["mid"] == 1)
    moved = mirror & (_bits(plane) != 0).any(-1)
    print("cornell_mixed: %d pixels on the moved mirror sphere, %d of them carry motion" % (mirror.sum(), moved.sum()))
    assert mirror.sum() >= 20 and moved.sum() <= 0.1 * mirror.sum()
    assert (_bits(plane[~only_prims["hit"] & (g[..., 3] == 0)]) == 0).all()       # misses
    # back, the snapshot consumed; then both kinds of update: both kinds carry motion
    r.update_primitives(ms.m0)
    r.render_guides(1)
    r.update_vertices(ms.vB, ms.nB)
    r.update_primitives(ms.mB)
    r.render_guides(1)
    plane = r.read_motion()
    m, D = plane[..., 3], plane[..., :3].astype(np.float64)
    dev = np.abs(D - both["D"]).max(-1)
    match = ((m > 0) == (both["m"] > 0)) & (dev <= 1e-3 * ms.size)
    assert (~match).mean() <= 0.005
    assert dev[match & both["mesh"]].max() <= TRI_D_BOUND and dev[match & ~both["mesh"]].max() <= PRIM_D_BOUND
    assert (match & both["mesh"] & (D != 0).any(-1)).sum() >= 50 and (match & (both["kind"] >= 0) & (D != 0).any(-1)).sum() >= 100
    # back; then the vertices alone: primitive pixels read as zeros (the parent's plane)
    r.update_primitives(ms.m0)
    r.update_vertices(ms.v0, ms.n0)
    r.render_guides(1)
    r.update_vertices(ms.vB, ms.nB)
    r.render_guides(1)
    plane = r.read_motion()
    r.close()
    prim_px = only_tris["hit"] & (only_tris["mid"] >= 0)
    assert (prim_px & (_bits(plane) != 0).any(-1)).mean() <= 0.005
    assert ((plane[..., 3] > 0) == only_tris["mesh"]).mean() >= 0.995


def _zero(plane):
    return (_bits(plane) == 0).all()


@pytest.mark.gpu
def test_snapshot_rule(prt):
    ms = MotionScene(prt, "cornell_mixed")
    mA = ms.m0.copy()
    moves_mixed(mA, "A")
    r = ms.context()
    r.update_primitives(ms.mB)
    r.render_guides(1)
    first = r.read_motion()
    assert not _zero(first)
    r.render_guides(1)
    assert _zero(r.read_motion()), "a second render_guides without an update"
    # A then B measures from before A
    r.update_primitives(ms.m0)
    r.render_guides(1)
    r.update_primitives(mA)
    r.update_primitives(ms.mB)
    r.render_guides(1)
    assert (_bits(r.read_motion()) == _bits(first)).all(), "A then B: the displacement from the geometry before A to B"
    # a refused update leaves the pending snapshot alone
    r.update_primitives(ms.m0)
    r.render_guides(1)
    r.update_primitives(ms.mB)
    bad = mA.copy()
    bad["joker"][3, 0] = NAN
    assert _code(r.update_primitives, bad) == prt.PRT_ERR_INVALID_ARGUMENT
    r.render_guides(1)
    assert (_bits(r.read_motion()) == _bits(first)).all()
    # upload_scene drops it, and so does turning motion off and on again
    r.update_primitives(ms.m0)
    r.upload_scene(ms.scene)
    r.render_guides(1)
    assert _zero(r.read_motion())
    r.update_primitives(ms.mB)
    r.set_motion(False)
    r.set_motion(True)
    r.render_guides(1)
    assert _zero(r.read_motion())
    # the two snapshots are independent: a triangle snapshot consumed alone, then a primitive one alone
    r.update_primitives(ms.m0)
    r.render_guides(1)
    r.update_vertices(ms.vB, ms.nB)
    r.render_guides(1)
    r.update_primitives(ms.mB)
    r.render_guides(1)
    tri_px = ms.caster_plane(True, True)["mesh"]
    assert (tri_px & (_bits(r.read_motion()) != 0).any(-1)).mean() <= 0.005
    r.close()


def _union(ms, K, size, update, **kw):
    par = importlib.import_module(PKG_NAME + ".parallel")
    Wf, Hf = size
    out = {}
    split = Hf // 2 - 1 if Hf > 8 else 2
    B = 16 if Hf > 16 else 1
    for key, part in (("whole", None), ("t0", ("tile", 0, split)), ("t1", ("tile", split, Hf - split)), ("b0", ("blocks", B, 0)), ("b1", ("blocks", B, 1))):
        r = ms.context(part=part, size=size, **kw)
        update(r)
        r.render_guides(K)
        out[key] = r.read_motion()
        r.close()
    tiles = np.concatenate([out["t0"], out["t1"]], 0)
    blocks = np.zeros_like(out["whole"])
    rows = np.arange(Hf)
    for p in (0, 1):
        blocks[rows[(rows // B) % 2 == p]] = out["b%d" % p]
    return out["whole"], tiles, blocks


@pytest.mark.gpu
@pytest.mark.parametrize("K,size", [(1, (W, H)), (4, (W, H)), (1, (9, 5)), (4, (9, 5))])
def test_splits(prt, K, size):
    """tile and row-block parts in union equal the whole frame bit for bit, with both kinds of snapshot pending"""
    ms = MotionScene(prt, "cornell_mixed")

    def update(r):
        r.update_vertices(ms.vB, ms.nB)
        r.update_primitives(ms.mB)
    whole, tiles, blocks = _union(ms, K, size, update)
    assert not _zero(whole)
    if K == 4 and size == (W, H):
        assert ((whole[..., 3] > 0) & (whole[..., 3] < 1)).any(), "K = 4: pixels partly on a contributing surface"
    assert (_bits(tiles) == _bits(whole)).all()
    assert (_bits(blocks) == _bits(whole)).all()


@pytest.mark.gpu
def test_pixel_filter_instance_and_guides(prt):
    """the pixel-filter instance at box 0.5 equals the plain instance (guides and plane), with and without the triangle term; the eight guide
    floats are the same bits in every instance"""
    ms = MotionScene(prt, "cornell_mixed")
    got = {}
    for key, kw, tri in (("plain", {}, False), ("box", dict(pixel_filter=("box", 0.5)), False), ("plain+tri", {}, True),
                         ("box+tri", dict(pixel_filter=("box", 0.5)), True), ("off", dict(motion=False), True)):
        r = ms.context(**kw)
        if tri:
            r.update_vertices(ms.vB, ms.nB)
        r.update_primitives(ms.mB)
        r.render_guides(4)
        got[key] = (r.read_guides(), r.read_motion() if kw.get("motion", True) else None)
        r.close()
    for a, b in (("plain", "box"), ("plain+tri", "box+tri")):
        assert (_bits(got[a][0]) == _bits(got[b][0])).all() and (_bits(got[a][1]) == _bits(got[b][1])).all(), (a, b)
    assert (_bits(got["plain+tri"][0]) == _bits(got["off"][0])).all(), "the guides with motion on and off"
    assert (_bits(got["plain"][1]) != _bits(got["plain+tri"][1])).any()


@pytest.mark.gpu
def test_sdf_instance(prt):
    """cornell_sdf, translations only: every moving pixel's D has exactly the bits of pos_prev - pos_cur of a translated SDF primitive or sphere"""
    ms = MotionScene(prt, "cornell_sdf")
    assert ms.cfg.geom_flags & 4
    r, off = ms.context(), ms.context(motion=False)
    for q in (r, off):
        q.update_primitives(ms.mB)
        q.render_guides(1)
    plane = r.read_motion()
    assert (_bits(r.read_guides()) == _bits(off.read_guides())).all()
    r.close()
    off.close()
    allowed = set()
    for i in range(len(ms.m0)):
        d = ms.m0["pos"][i, :3] - ms.mB["pos"][i, :3]
        if (d != 0).any():
            allowed.add(tuple(int(x) for x in _bits(d)))
    assert len(allowed) == 4
    moving = (plane[..., 3] > 0) & (_bits(plane[..., :3]) != 0).any(-1)
    seen = {tuple(int(x) for x in _bits(px[:3])) for px in plane[moving]}
    print("cornell_sdf: %d moving pixels, %d distinct displacements" % (moving.sum(), len(seen)))
    assert moving.mean() >= 0.05
    assert seen <= allowed, seen - allowed
    assert len(seen) >= 3, "the SDF sphere, box and round box are all in view"
    assert ((plane[..., 3] == 0) | (plane[..., 3] == 1)).all()


@pytest.mark.gpu
def test_motion_off_changes_nothing_but_the_geometry(prt):
    """a motion-off context: the update takes no snapshot and there is no plane; denoise_temporal of a motion-on context whose plane is zeros runs
    in step with it, bit for bit"""
    ms = MotionScene(prt, "cornell_mixed")
    on, off = ms.context(), ms.context(motion=False)
    seeds = prt.seed_pairs(2 * max(ms.cfg.max_bounces, 8) + 64)
    for q in (on, off):
        q.update_primitives(ms.mB)
    on.render_guides(1)                                         # (the snapshot consumed)
    assert _code(off.read_motion) == prt.PRT_ERR_NOT_READY
    for k in range(2):
        outs = []
        for q in (on, off):
            q.reset()
            q.render_spp(2, seeds)
            q.render_guides(1)
            outs.append(q.denoise_temporal())
        assert _zero(on.read_motion()), k
        assert (_bits(outs[0]) == _bits(outs[1])).all() and (_bits(on.read_history()) == _bits(off.read_history())).all(), k
        assert (_bits(on.read_framebuffer()) == _bits(off.read_framebuffer())).all(), k
    on.close()
    off.close()


# ---- the history follows the primitive: a diffuse sphere approaches a still pinhole camera ---------------------------------------------------------------

APPROACH_F = 4                  # displayed frames
APPROACH_STEP = 0.45            # the sphere's step towards the camera per frame: beyond tau_z * depth + the depth gradient on its interior
T_PARAMS = dict(alpha_color=0.2, alpha_moments=0.2, tau_z=0.05, cos_n=0.9, history_cap=32)


def _erode2(mask):
    out = mask.copy()
    Hm, Wm = mask.shape
    pad = np.pad(mask, 2, constant_values=False)
    for dy in range(5):
        for dx in range(5):
            out &= pad[dy:dy + Hm, dx:dx + Wm]
    return out


class Approach:
    """the box of cornell_mixed without the teapot (no triangles: the caster is quick), its four spheres, and a diffuse sphere (mesh 4) that
    comes towards the camera by APPROACH_STEP per displayed frame.  The float64 mirror: temporal_ref_motion on the caster's guides and planes"""
    _cache = {}

    def __new__(cls, prt):
        if "a" not in cls._cache:
            self = super().__new__(cls)
            self.prt = prt
            s = json.loads(_prims_only_text())
            s["scene"]["spheres"].append({"pos": [0.3, 1.3, 0.2], "radius": 0.45, "material": {"color": [0.3, 0.5, 0.9], "type": 1}})
            self.scene = prt.HostScene(json.dumps(s), text=True)
            self.cfg = self.scene.config()
            self.cam = prt.default_camera(W, H)
            self.cam.apertureRadius = 0.0
            self.env = prt.make_sky(64, 32)
            m0 = meshes_of(self.scene.desc)
            eye = np.array(self.cam.position[:3], dtype=np.float64)
            to_eye = eye - m0["pos"][4, :3]
            to_eye /= np.linalg.norm(to_eye)
            self.poses = []
            for k in range(APPROACH_F):
                m = m0.copy()
                move_sphere(m, 4, to_eye * (APPROACH_STEP * k))
                m.setflags(write=False)
                self.poses.append(m)
            self.g, self.plane, self.on_sphere = [], [], []
            for k in range(APPROACH_F):
                c = PrimCaster(prt, self.scene.desc, self.cfg, self.poses[k], self.poses[max(k - 1, 0)], None, None)
                self.g.append(c.guides(self.cam, W, H).astype(f32))
                w = c.plane(self.cam, W, H, False, k > 0)
                self.plane.append(np.concatenate([w["D"], w["m"][..., None]], -1).astype(f32))
                self.on_sphere.append(w["hit"] & (w["mid"] == 4))
            self.interior = _erode2(self.on_sphere[-1])
            self.mirror = {True: self._run(True), False: self._run(False)}
            cls._cache["a"] = self
        return cls._cache["a"]

    def _run(self, with_plane):
        """the mirror over the caster's own inputs (the colour: the caster's albedo): the per-frame list of temporal_ref_motion's dicts"""
        prev, out = None, []
        for k in range(APPROACH_F):
            g = self.g[k]
            fb = np.concatenate([g[..., :3], np.ones((H, W, 1), dtype=f32)], -1)
            hist_prev, g_prev = prev if prev is not None else (None, g)
            ref = temporal_ref_motion(fb, g, g_prev, hist_prev, self.cam, self.cam, np.zeros((H, W)), motion=self.plane[k] if with_plane else None,
                                      **T_PARAMS)
            out.append(ref)
            prev = (_mirror_history(ref, fb), g)
        return out

    def shares(self, n_with, n_without):
        i = self.interior
        return float((n_with[i] >= APPROACH_F - 1).mean()), float((n_without[i] == 1).mean())


def test_history_follows_the_sphere_on_the_mirror():
    """The mirror's figures (recorded from this test's output): step 0.45 per frame, the sphere's distance 3.64 -> 2.29 over F = 4 frames, 169
    interior pixels of 333 on the sphere; n >= F - 1 on 100 % of them with the plane, n == 1 on 100 % without.  Required of the mirror itself: n >= F - 1 on at least
    90 % of the sphere's interior (its pixels of the last frame eroded by two) with the plane, n == 1 on at least 90 % without"""
    ap = Approach(_pkg())
    with_share, without_share = ap.shares(ap.mirror[True][-1]["n"], ap.mirror[False][-1]["n"])
    sphere = ap.poses[-1][4]
    z = np.linalg.norm(np.array(ap.cam.position[:3]) - sphere["pos"][:3])
    print("approaching sphere (mirror): %d interior pixels of %d on the sphere, distance %.2f -> %.2f, n >= F - 1 on %.3f with the plane, n == 1 on %.3f without"
          % (ap.interior.sum(), ap.on_sphere[-1].sum(), z + APPROACH_STEP * (APPROACH_F - 1), z, with_share, without_share))
    assert ap.interior.sum() >= 40
    assert with_share >= 0.9 and without_share >= 0.9, (with_share, without_share)
    for k in range(1, APPROACH_F):
        moving = (ap.plane[k][..., 3] > 0) & (ap.plane[k][..., :3] != 0).any(-1)
        assert (moving == ap.on_sphere[k]).all(), k


def _footprint_scale(g, plane, hist_prev, cam):
    """per pixel the largest |colour| of the previous history in the 4x4 window around the pixel's reprojected position (prt.h: X + D through
    the camera).  The device forms the bilinear weights in f32 from a position that is off by about 1e-6 pixels, so a tap whose exact weight
    is 0 comes in with a weight of that size: next to the light (5.0) a black pixel gets 5e-6, far above 1e-4 of its own colour.  The
    mirror's own scale counts only taps with a weight above 1e-6; this one counts every value the footprint can touch"""
    B = camera_basis(cam)
    X = B[0] + centre_dirs(B, W, H) * g[..., 7].astype(np.float64)[..., None]
    moved = (g[..., 3] > 0) & (plane[..., 3] > 0) & (plane[..., :3] != 0).any(-1)
    X = np.where(moved[..., None], X + plane[..., :3], X)
    xp, yp, _ = project(B, X - B[0], W, H)
    x0 = np.clip(np.floor(np.nan_to_num(xp)).astype(np.int64), 0, W - 1)
    y0 = np.clip(np.floor(np.nan_to_num(yp)).astype(np.int64), 0, H - 1)
    mag = np.abs(hist_prev[..., :3]).max(-1)
    out = np.zeros((H, W))
    for dy in range(-1, 3):
        for dx in range(-1, 3):
            out = np.maximum(out, mag[np.clip(y0 + dy, 0, H - 1), np.clip(x0 + dx, 0, W - 1)])
    return out


@pytest.mark.gpu
def test_history_follows_the_sphere_on_the_device(prt):
    """F = 4 displayed frames (update, reset, render, guides at K = 1, denoise_temporal with the integrated feedback) in a context with motion on
    and in one with motion off.  Held to the mirror's two conditions on the mirror's interior mask; to the mirror's n (the caster's guides
    and planes) wherever the device's coverage agrees with the caster's and the mirror is not within its margin of a threshold; and, with the
    plane, to a mirror fed with the device's own inputs and history: n and the integrated colour within 1e-4, as the card test of test_motion
    (relative to the largest colour in the pixel's reprojection footprint: _footprint_scale says why).
    Figures (MI355X, 64x48, step 0.45): see DESIGN.md s4 "Moving primitives"."""
    ap = Approach(prt)
    seeds = prt.seed_pairs(2 * max(ap.cfg.max_bounces, 8) + 64)
    hist = {}
    for motion in (True, False):
        r = prt.Renderer(ap.cfg, device=0)
        r.upload_scene(ap.scene)
        r.upload_envmap(ap.env)
        r.set_camera(ap.cam)
        r.resize(W, H)
        r.set_motion(motion)
        prev, worst = None, {}
        for k in range(APPROACH_F):
            if k:
                r.update_primitives(ap.poses[k])
            r.reset()
            r.render_spp(2, seeds)
            r.render_guides(1)
            r.denoise_temporal(feedback="integrated")
            h, g, fb = r.read_history(), r.read_guides(), r.read_framebuffer()
            caster_ref = ap.mirror[motion][k]
            agree = ((g[..., 3] > 0) == (ap.g[k][..., 3] > 0)) & caster_ref["margin_other"]
            if k:
                agree &= (g_last[..., 3] > 0) == (ap.g[k - 1][..., 3] > 0)
            same_n = np.abs(h[..., 3] - caster_ref["n"]) <= 1e-4 * caster_ref["n"]
            print("approaching sphere (device, motion %s), frame %d: n differs from the caster's mirror on %d of %d pixels" % (motion, k, (agree & ~same_n).sum(), agree.sum()))
            assert (agree & ~same_n & ap.interior).sum() == 0, (motion, k)
            assert (agree & ~same_n).mean() <= 0.005, (motion, k, "the silhouette allowance of the caster tests")
            if motion:
                plane = r.read_motion()
                hist_prev, g_prev = prev if prev is not None else (None, g)
                ref = temporal_ref_motion(fb, g, g_prev, hist_prev, ap.cam, ap.cam, np.zeros((H, W)), motion=plane, **T_PARAMS)
                mm = ref["margin_other"]
                _cmp("approach", k, "n", h[..., 3], ref["n"], ref["n"], mm, worst)
                scale = ref["cscale"] if prev is None else np.maximum(ref["cscale"], _footprint_scale(g, plane, prev[0], ap.cam))
                _cmp("approach", k, "c", h[..., :3], ref["ci"], scale, mm, worst)
                assert mm.mean() >= 0.9
            prev, g_last = (h, g), g
        hist[motion] = h
        r.close()
        if motion:
            print("approaching sphere (device): largest error / bound against the in-step mirror: %s" % "  ".join("%s %.3g" % kv for kv in sorted(worst.items())))
    with_share, without_share = ap.shares(hist[True][..., 3], hist[False][..., 3])
    print("approaching sphere (device): n >= F - 1 on %.3f of the interior with the plane, n == 1 on %.3f without" % (with_share, without_share))
    assert with_share >= 0.9 and without_share >= 0.9, (with_share, without_share)
