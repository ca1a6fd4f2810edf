"""tests/emu/prims_api.py -- TEST INFRASTRUCTURE: builds and binds tests/emu/libprims_emu.so, the bodies of prt_update_primitives and of the
primitives' motion (csrc/hip/pt_prims.h) compiled for the host (prims_emu.cpp), as motion_api.py does for the triangles' motion."""
import ctypes as C

import numpy as np

import _emu
from _emu import aligned, ptr

MESH_BYTES = 256
# numpy view of prt_mesh (include/prt_types.h)
MESH_DTYPE = np.dtype([("mat", "u1", 64), ("pos", "<f4", 4), ("_pad0", "u1", 48), ("joker", "<f4", 16), ("t", "u1"), ("_pad1", "u1", 63)])
SPHERE_FLOATS, SDF_FLOATS, QUAD_FLOATS = 4, 8, 20          # DevSphere, DevSdf, DevQuad (csrc/hip/pt_layout.h)
assert MESH_DTYPE.itemsize == MESH_BYTES

NAME, SRCS, OPT, INCS = "prims_emu", [_emu.src("prims_emu.cpp")], "-O2", (_emu.INCLUDE, _emu.HIP)
LIB = _emu.lib_path(NAME)
_DISP = (None, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p])
PROTOTYPES = {
    "prims_emu_pack": (C.c_uint32, [C.c_void_p, C.c_uint32, C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "prims_emu_sphere": _DISP,
    "prims_emu_quad": _DISP,
    "prims_emu_sdf": (None, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p]),
    "prims_emu_pixel": (None, [C.c_void_p] * 6 + [C.c_uint32, C.c_uint32] + [C.c_void_p] * 4 + [C.c_int, C.c_int, C.c_uint32, C.c_void_p]),
}


def build():
    return _emu.build_lib(NAME, SRCS, OPT, incs=INCS)


def lib():
    return _emu.shared_lib(NAME, SRCS, OPT, prototypes=PROTOTYPES, incs=INCS)


def build_main(out, sanitize=True):
    """the stand-alone program of prims_emu.cpp (its own main) at `out`, under -fsanitize=address,undefined unless told otherwise"""
    san = ["-Xarch_host", "-fsanitize=address,undefined", "-Xarch_host", "-fno-sanitize-recover=all", "-g"] if sanitize else []
    return _emu.program(out, SRCS, OPT, ("PRIMS_EMU_MAIN",), san, incs=INCS)


def _al(a, floats):
    a = np.asarray(a, dtype=np.float32).reshape(-1, floats)
    out = aligned((max(len(a), 1), floats), np.float32)
    out[:len(a)] = a.view(np.float32)
    return out


def pack(meshes, n_spheres, n_sdfs, types):
    """prims_pack of every record: meshes a MESH_DTYPE array -> (spheres float32 [n, 4], sdfs float32 [n, 8] (bits: word 3 is the type), quads
    float32 [n, 20], bad bool [count])"""
    count = len(meshes)
    m = aligned((max(count, 1),), MESH_DTYPE)
    m[:count] = meshes
    n_quads = count - n_spheres - n_sdfs
    sph, sdf, quad = aligned((max(n_spheres, 1), 4), np.float32), aligned((max(n_sdfs, 1), 8), np.float32), aligned((max(n_quads, 1), 20), np.float32)
    types = np.ascontiguousarray(types, dtype=np.uint8)
    bad = np.zeros(max(count, 1), dtype=np.uint8)
    lib().prims_emu_pack(ptr(m), count, n_spheres, n_sdfs, ptr(types), ptr(sph), ptr(sdf), ptr(quad), ptr(bad))
    return sph[:n_spheres].copy(), sdf[:n_sdfs].copy(), quad[:n_quads].copy(), bad[:count].astype(bool)


def _disp(fn, floats, prev, cur, idx, p):
    a, b = _al(prev, floats), _al(cur, floats)
    idx = np.ascontiguousarray(idx, dtype=np.uint32)
    out = np.zeros((len(idx), 3), dtype=np.float32)
    if p is None:
        fn(ptr(a), ptr(b), ptr(idx), len(idx), ptr(out))
    else:
        p = np.ascontiguousarray(p, dtype=np.float32)
        fn(ptr(a), ptr(b), ptr(idx), ptr(p), len(idx), ptr(out))
    return out


def sphere_displacement(prev, cur, idx, p):
    return _disp(lib().prims_emu_sphere, SPHERE_FLOATS, prev, cur, idx, p)


def quad_displacement(prev, cur, idx, p):
    return _disp(lib().prims_emu_quad, QUAD_FLOATS, prev, cur, idx, p)


def sdf_displacement(prev, cur, idx):
    return _disp(lib().prims_emu_sdf, SDF_FLOATS, prev, cur, idx, None)


def pixel(sph, sdf, quad, mid, first, p, tri_d, tri_snap, prim_snap):
    """one pixel's {D, m}: sph / sdf / quad = (prev, cur) table pairs; mid int32 [K] (-2 miss, -1 triangle), first bool [K], p / tri_d float32 [K, 3]"""
    t = [_al(x, f) for pair, f in ((sph, SPHERE_FLOATS), (sdf, SDF_FLOATS), (quad, QUAD_FLOATS)) for x in pair]
    mid = np.ascontiguousarray(mid, dtype=np.int32)
    first = np.ascontiguousarray(first, dtype=np.uint8)
    p = np.ascontiguousarray(p, dtype=np.float32)
    tri_d = np.ascontiguousarray(tri_d, dtype=np.float32)
    out = np.zeros(4, dtype=np.float32)
    lib().prims_emu_pixel(*[ptr(x) for x in t], len(sph[0]), len(sdf[0]), ptr(mid), ptr(first), ptr(p), ptr(tri_d), int(tri_snap), int(prim_snap), len(mid),
                          ptr(out))
    return out
