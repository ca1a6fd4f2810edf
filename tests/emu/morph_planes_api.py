"""tests/emu/morph_planes_api.py -- TEST INFRASTRUCTURE: builds and binds tests/emu/libmorph_planes_emu.so, the bodies of the plane-layout
morph kernels (csrc/hip/pt_morph.h), the builder of the plane table and the report's arithmetic compiled for the host with the library's
flags and run serially in the kernel's launch shape (morph_planes_emu.cpp).  Sets are described as in morph_api (make_set)."""
import ctypes as C

import numpy as np

import _emu
from _emu import aligned_copy as _aligned, ptr
from morph_api import make_set

NAME, SRCS, OPT = "morph_planes_emu", [_emu.src("morph_planes_emu.cpp")], ("-O3", "-fno-slp-vectorize")
LIB = _emu.lib_path(NAME)
PROTOTYPES = {
    "morph_planes_emu_table": (None, [C.c_void_p, C.c_uint32] + [C.c_void_p] * 5),
    "morph_planes_emu_table_bytes": (C.c_uint64, [C.c_uint32, C.c_uint32, C.c_uint64, C.c_uint64, C.c_int]),
    "morph_planes_emu_morph": (None, [C.c_void_p] * 7 + [C.c_uint32, C.c_void_p, C.c_void_p]),
    "morph_planes_emu_pose_morphed": (None, [C.c_void_p] * 10 + [C.c_uint32, C.c_void_p, C.c_void_p]),
}
CORNERS, PLANES = 0, 1                                      # PRT_MORPH_LAYOUT_* (include/prt.h)


def build():
    return _emu.build_lib(NAME, SRCS, OPT)


def lib():
    return _emu.shared_lib(NAME, SRCS, OPT, prototypes=PROTOTYPES)


def table(base_v, base_n, targets, n_tris):
    """the plane table of an accepted set: (block_first uint32 [B + 1], head uint32 [P, 4] = {target, 0, mask_lo, mask_hi}, plane_p float32
    [P, 3, 64], plane_n float32 [P, 3, 64] or None, entries), each array in a buffer of exactly its size"""
    s, keep = make_set(base_v, base_n, targets)
    counts = np.zeros(2, dtype=np.uint64)
    lib().morph_planes_emu_table(_emu.ref(s), int(n_tris), ptr(counts), None, None, None, None)
    planes = int(counts[0])
    block_first = np.zeros((3 * int(n_tris) + 63) // 64 + 1, dtype=np.uint32)
    head = _emu.aligned((planes, 4), np.uint32)
    plane_p = _emu.aligned((planes, 3, 64), np.float32)
    plane_n = None if base_n is None else _emu.aligned((planes, 3, 64), np.float32)
    lib().morph_planes_emu_table(_emu.ref(s), int(n_tris), ptr(counts), ptr(block_first), ptr(head), ptr(plane_p), ptr(plane_n))
    return block_first, head, plane_p, plane_n, int(counts[1])


def table_bytes(layout, n_tris, entries, planes, with_normals):
    """prt_get_morph_report's table_bytes by the library's own function"""
    return int(lib().morph_planes_emu_table_bytes(int(layout), int(n_tris), int(entries), int(planes), 1 if with_normals else 0))


def report(base_v, base_n, targets, n_tris, layout):
    """what prt_get_morph_report returns for the set under `layout`, from the builder and the library's arithmetic"""
    block_first, head, _, _, entries = table(base_v, base_n, targets, n_tris)
    planes = len(head) if layout == PLANES else 0
    return {"layout": layout, "n_targets": len(targets), "entries": entries, "planes": planes,
            "table_bytes": table_bytes(layout, n_tris, entries, planes, base_n is not None)}


def _run(base_v, base_n, targets, weights, skin=None):
    v = _aligned(base_v, np.float32)
    corners = v.size // 4
    n = None if base_n is None else _aligned(base_n, np.float32)
    block_first, head, plane_p, plane_n, _ = table(base_v, base_n, targets, corners // 3)
    w = np.array(weights, dtype=np.float32).reshape(-1).copy()             # exactly len(targets) floats
    assert w.size == len(targets) and corners % 3 == 0
    out_v = _aligned(np.full(4 * corners, np.nan), np.float32)
    out_n = None if n is None else _aligned(np.full(4 * corners, np.nan), np.float32)
    if skin is None:
        lib().morph_planes_emu_morph(ptr(v), ptr(n), ptr(block_first), ptr(head), ptr(plane_p), ptr(plane_n), ptr(w), corners, ptr(out_v), ptr(out_n))
    else:
        b, bw, m = _aligned(skin[0], np.uint16), _aligned(skin[1], np.float32), _aligned(skin[2], np.float32)
        assert b.size == 4 * corners and bw.size == 4 * corners and m.size % 12 == 0
        lib().morph_planes_emu_pose_morphed(ptr(v), ptr(n), ptr(block_first), ptr(head), ptr(plane_p), ptr(plane_n), ptr(w), ptr(b), ptr(bw), ptr(m),
                                            corners, ptr(out_v), ptr(out_n))
    return out_v.reshape(-1, 4).copy(), None if out_n is None else out_n.reshape(-1, 4).copy()


def morph(base_v, base_n, targets, weights):
    """the body of prt_morph under PRT_MORPH_LAYOUT_PLANES, serially, over the table the builder makes: (vertices, normals) float32
    [corners, 4]; normals None without base normals"""
    return _run(base_v, base_n, targets, weights)


def pose_morphed(base_v, base_n, targets, weights, bone_index, bone_weight, matrices):
    """the fused body, serially"""
    return _run(base_v, base_n, targets, weights, (bone_index, bone_weight, matrices))
