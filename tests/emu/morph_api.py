"""tests/emu/morph_api.py -- TEST INFRASTRUCTURE: builds and binds tests/emu/libmorph_emu.so, the bodies of the morph kernels
(csrc/hip/pt_morph.h) and the checks and the table builder of prt_set_morph_targets compiled for the host with the library's flags and run
serially (morph_emu.cpp)."""
import ctypes as C

import numpy as np

import _emu
from _emu import aligned_copy as _aligned, ptr

NAME, SRCS, OPT = "morph_emu", [_emu.src("morph_emu.cpp")], ("-O3", "-fno-slp-vectorize")
LIB = _emu.lib_path(NAME)
PROTOTYPES = {
    "morph_emu_check": (C.c_int, [C.c_void_p, C.c_uint32]),
    "morph_emu_table": (C.c_uint32, [C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p]),
    "morph_emu_morph": (None, [C.c_void_p] * 6 + [C.c_uint32, C.c_void_p, C.c_void_p]),
    "morph_emu_pose_morphed": (None, [C.c_void_p] * 9 + [C.c_uint32, C.c_void_p, C.c_void_p]),
    "morph_emu_max_targets": (C.c_uint32, []),
}


class Target(C.Structure):                                  # prt_morph_target (include/prt.h)
    _fields_ = [("corner", C.c_void_p), ("d_position", C.c_void_p), ("d_normal", C.c_void_p), ("n_entries", C.c_uint32), ("_pad", C.c_uint32)]


class Set(C.Structure):                                     # prt_morph_set
    _fields_ = [("base_vertices", C.c_void_p), ("base_normals", C.c_void_p), ("targets", C.c_void_p), ("n_targets", C.c_uint32), ("_pad", C.c_uint32)]


def build():
    return _emu.build_lib(NAME, SRCS, OPT)


def lib():
    return _emu.shared_lib(NAME, SRCS, OPT, prototypes=PROTOTYPES)


def make_set(base_v, base_n, targets, n_targets=None, n_entries=None):
    """(prt_morph_set, what it points to): targets a list of (corner, d_position, d_normal or None); arrays are passed as they are (None = a
    null pointer).  n_targets / n_entries (a list) override the counts, for the refusals"""
    v = None if base_v is None else np.ascontiguousarray(base_v, dtype=np.float32)
    n = None if base_n is None else np.ascontiguousarray(base_n, dtype=np.float32)
    keep = [v, n]
    rec = None
    if targets is not None:
        rec = (Target * max(len(targets), 1))()
        for t, (corner, dp, dn) in enumerate(targets):
            corner = None if corner is None else np.ascontiguousarray(corner, dtype=np.uint32)
            dp = None if dp is None else np.ascontiguousarray(dp, dtype=np.float32)
            dn = None if dn is None else np.ascontiguousarray(dn, dtype=np.float32)
            keep += [corner, dp, dn]
            count = (0 if corner is None else corner.size) if n_entries is None else n_entries[t]
            rec[t] = Target(ptr(corner), ptr(dp), ptr(dn), int(count), 0)
        keep.append(rec)
    count = (0 if targets is None else len(targets)) if n_targets is None else n_targets
    return Set(ptr(v), ptr(n), None if rec is None else C.cast(rec, C.c_void_p), int(count), 0), keep


def check(base_v, base_n, targets, n_tris, **counts):
    """the refusals of prt_set_morph_targets: 0 = accepted, else the code it returns"""
    s, keep = make_set(base_v, base_n, targets, **counts)
    return lib().morph_emu_check(_emu.ref(s), int(n_tris))


def table(base_v, base_n, targets, n_tris):
    """the per-corner table of an accepted set: (offset uint32 [3T + 1], entry_p float32 [E, 4], entry_n float32 [E, 4] or None), each in a
    buffer of exactly its size"""
    s, keep = make_set(base_v, base_n, targets)
    total = int(lib().morph_emu_table(_emu.ref(s), int(n_tris), None, None, None))
    offset = np.zeros(3 * int(n_tris) + 1, dtype=np.uint32)
    entry_p = _emu.aligned((total, 4), np.float32)
    entry_n = None if base_n is None else _emu.aligned((total, 4), np.float32)
    lib().morph_emu_table(_emu.ref(s), int(n_tris), ptr(offset), ptr(entry_p), ptr(entry_n))
    return offset, entry_p, entry_n


def _run(base_v, base_n, targets, weights, skin=None):
    v = _aligned(base_v, np.float32)
    corners = v.size // 4
    n = None if base_n is None else _aligned(base_n, np.float32)
    offset, entry_p, entry_n = table(base_v, base_n, targets, corners // 3)
    w = np.array(weights, dtype=np.float32).reshape(-1).copy()             # exactly len(targets) floats
    assert w.size == len(targets) and corners % 3 == 0
    out_v = _aligned(np.full(4 * corners, np.nan), np.float32)
    out_n = None if n is None else _aligned(np.full(4 * corners, np.nan), np.float32)
    if skin is None:
        lib().morph_emu_morph(ptr(v), ptr(n), ptr(offset), ptr(entry_p), ptr(entry_n), ptr(w), corners, ptr(out_v), ptr(out_n))
    else:
        b, bw, m = _aligned(skin[0], np.uint16), _aligned(skin[1], np.float32), _aligned(skin[2], np.float32)
        assert b.size == 4 * corners and bw.size == 4 * corners and m.size % 12 == 0
        lib().morph_emu_pose_morphed(ptr(v), ptr(n), ptr(offset), ptr(entry_p), ptr(entry_n), ptr(w), ptr(b), ptr(bw), ptr(m), corners, ptr(out_v),
                                     ptr(out_n))
    return out_v.reshape(-1, 4).copy(), None if out_n is None else out_n.reshape(-1, 4).copy()


def morph(base_v, base_n, targets, weights):
    """the body of prt_morph, serially, over the table the builder makes: (vertices, normals) float32 [corners, 4]; normals None without base
    normals"""
    return _run(base_v, base_n, targets, weights)


def pose_morphed(base_v, base_n, targets, weights, bone_index, bone_weight, matrices):
    """the fused body, serially"""
    return _run(base_v, base_n, targets, weights, (bone_index, bone_weight, matrices))
