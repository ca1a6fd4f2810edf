"""tests/emu/motion_api.py -- TEST INFRASTRUCTURE: builds and binds tests/emu/libmotion_emu.so, the bodies of the motion plane
(csrc/hip/pt_motion.h) compiled for the host (motion_emu.cpp), as refit_api.py does for the refit."""
import ctypes as C

import numpy as np

import _emu
from _emu import aligned_copy, ptr

NAME, SRCS, OPT, INCS = "motion_emu", [_emu.src("motion_emu.cpp")], "-O2", (_emu.INCLUDE, _emu.HIP)
LIB = _emu.lib_path(NAME)
PROTOTYPES = {
    "motion_emu_displacement": (None, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p]),
    "motion_emu_pixel": (None, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p]),
}


def build():
    return _emu.build_lib(NAME, SRCS, OPT, incs=INCS)


def lib():
    return _emu.shared_lib(NAME, SRCS, OPT, prototypes=PROTOTYPES, incs=INCS)


def _aligned_records(rec):
    """float32 [n, 12] -> a 16-byte aligned copy (TriGeom is alignas(16))"""
    return aligned_copy(np.asarray(rec, dtype=np.float32).reshape(-1, 12), np.float32)


def displacement(prev, cur, slots, uv):
    """motion_displacement of every case: prev / cur float32 [n_slots, 12] (TriGeom: p0, e1, e2, n), slots uint32 [n], uv float32 [n, 2] ->
    float32 [n, 3]"""
    p, c = _aligned_records(prev), _aligned_records(cur)
    slots = np.ascontiguousarray(slots, dtype=np.uint32)
    uv = np.ascontiguousarray(uv, dtype=np.float32)
    assert slots.size == 0 or int(slots.max()) < len(p) == len(c)
    out = np.zeros((len(slots), 3), dtype=np.float32)
    lib().motion_emu_displacement(ptr(p), ptr(c), ptr(slots), ptr(uv), len(slots), ptr(out))
    return out


def pixel(d, hit, contributing):
    """the per-pixel reduction over K samples: d float32 [K, 3], hit / contributing bool [K] -> float32 [4] = {D, m}"""
    d = np.ascontiguousarray(d, dtype=np.float32)
    hit = np.ascontiguousarray(hit, dtype=np.uint8)
    con = np.ascontiguousarray(contributing, dtype=np.uint8)
    out = np.zeros(4, dtype=np.float32)
    lib().motion_emu_pixel(ptr(d), ptr(hit), ptr(con), len(hit), ptr(out))
    return out
