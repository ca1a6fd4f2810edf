"""tests/emu/normals_api.py -- TEST INFRASTRUCTURE: builds and binds tests/emu/libnormals_emu.so, the bodies of the smooth-normal kernels
(csrc/hip/pt_normals.h) and the host group-table builder compiled for the host with the library's flags and run serially (normals_emu.cpp)."""
import ctypes as C

import numpy as np

import _emu
from _emu import aligned, aligned_copy, ptr

UNIT, AREA = 0, 1

NAME, SRCS, OPT = "normals_emu", [_emu.src("normals_emu.cpp")], ("-O3", "-fno-slp-vectorize")
LIB = _emu.lib_path(NAME)
PROTOTYPES = {
    "normals_emu_weld": (C.c_int, [C.c_void_p, C.c_uint32, C.c_void_p, C.POINTER(C.c_uint32)]),
    "normals_emu_table": (C.c_int, [C.c_void_p, C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p]),
    "normals_emu_generate": (C.c_int, [C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint32, C.c_uint32, C.c_float, C.c_void_p, C.c_void_p]),
}


def build():
    return _emu.build_lib(NAME, SRCS, OPT)


def lib():
    return _emu.shared_lib(NAME, SRCS, OPT, prototypes=PROTOTYPES)


def table(groups, n_groups):
    """the group table of prt_set_smooth_normals: (group_first uint32 [n_groups + 1], member_face uint32 [3T]); None for an id >= n_groups"""
    g = np.ascontiguousarray(groups, dtype=np.uint32)
    T = g.size // 3
    first, member = np.zeros(n_groups + 1, dtype=np.uint32), np.zeros(3 * T, dtype=np.uint32)
    if lib().normals_emu_table(ptr(g), T, n_groups, ptr(first), ptr(member)):
        return None
    return first, member


def generate(vertices, groups, n_groups, weighting, crease_cos):
    """the bodies, serially: (normals float32 [3T, 4], face records {f, l} float32 [T, 4]); None for an id >= n_groups"""
    v = aligned_copy(np.asarray(vertices, dtype=np.float32).reshape(-1), np.float32)          # (the bodies load and store float4s)
    g = np.ascontiguousarray(groups, dtype=np.uint32)
    T = v.size // 12
    assert g.size == 3 * T
    out, face = aligned((3 * T, 4), np.float32), np.zeros((T, 4), dtype=np.float32)
    if lib().normals_emu_generate(ptr(v), T, ptr(g), n_groups, weighting, C.c_float(crease_cos), ptr(out), ptr(face)):
        return None
    return out.copy(), face
