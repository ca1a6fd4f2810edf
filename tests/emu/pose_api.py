"""tests/emu/pose_api.py -- TEST INFRASTRUCTURE: builds and binds tests/emu/libpose_emu.so, the body of the pose kernel (csrc/hip/pt_pose.h)
and the checks of prt_set_skin compiled for the host with the library's flags and run serially (pose_emu.cpp)."""
import ctypes as C

import numpy as np

import _emu
from _emu import aligned_copy as _aligned, ptr

NAME, SRCS, OPT = "pose_emu", [_emu.src("pose_emu.cpp")], ("-O3", "-fno-slp-vectorize")
LIB = _emu.lib_path(NAME)
PROTOTYPES = {
    "pose_emu_check": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32]),
    "pose_emu_pose": (None, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p]),
    "pose_emu_max_bones": (C.c_uint32, []),
}


def build():
    return _emu.build_lib(NAME, SRCS, OPT)


def lib():
    return _emu.shared_lib(NAME, SRCS, OPT, prototypes=PROTOTYPES)


def check(rest_v, rest_n, bone_index, bone_weight, n_bones):
    """the refusals of prt_set_skin: True = accepted"""
    v = np.ascontiguousarray(rest_v, dtype=np.float32)
    n = None if rest_n is None else np.ascontiguousarray(rest_n, dtype=np.float32)
    b, w = np.ascontiguousarray(bone_index, dtype=np.uint16), np.ascontiguousarray(bone_weight, dtype=np.float32)
    return lib().pose_emu_check(ptr(v), ptr(n), ptr(b), ptr(w), int(n_bones), v.size // 12) == 0


def pose(rest_v, rest_n, bone_index, bone_weight, matrices):
    """the body, serially: (vertices, normals) float32 [corners, 4]; normals None without rest normals.  The matrix table is copied into a
    buffer of exactly its size"""
    v = _aligned(rest_v, np.float32)
    corners = v.size // 4
    n = None if rest_n is None else _aligned(rest_n, np.float32)
    b, w, m = _aligned(bone_index, np.uint16), _aligned(bone_weight, np.float32), _aligned(matrices, np.float32)
    assert b.size == 4 * corners and w.size == 4 * corners and m.size % 12 == 0 and (n is None or n.size == 4 * corners)
    out_v = _aligned(np.full(4 * corners, np.nan), np.float32)
    out_n = None if n is None else _aligned(np.full(4 * corners, np.nan), np.float32)
    lib().pose_emu_pose(ptr(v), ptr(n), ptr(b), ptr(w), ptr(m), corners, ptr(out_v), ptr(out_n))
    return out_v.reshape(-1, 4).copy(), None if out_n is None else out_n.reshape(-1, 4).copy()
