"""tests/emu/cost_api.py -- TEST INFRASTRUCTURE: builds and binds tests/emu/libcost_emu.so, the bodies of the tree-cost kernels
(csrc/hip/pt_cost.h) compiled for the host and run serially over a pair table (cost_emu.cpp)."""
import ctypes as C

import numpy as np

import _emu
from _emu import PAIR_DTYPE, ptr          # noqa: F401  (PAIR_DTYPE: for the tests)

NAME, SRCS, OPT = "cost_emu", [_emu.src("cost_emu.cpp"), _emu.PACK], "-O2"
LIB = _emu.lib_path(NAME)
PROTOTYPES = {
    "cost_emu_pack": (C.c_int, [C.c_void_p, C.c_void_p, C.POINTER(C.c_void_p), C.c_char_p, C.c_int]),
    "cost_emu_free": (None, [C.c_void_p]),
    "cost_emu_sizes": (None, [C.c_void_p, C.c_void_p]),
    "cost_emu_get": (None, [C.c_void_p, C.c_void_p, C.c_void_p]),
    "cost_emu_update": (C.c_int, [C.c_void_p, C.c_uint32, C.c_void_p]),
    "cost_emu_cost": (None, [C.c_void_p, C.c_void_p]),
    "cost_emu_table": (None, [C.c_void_p, C.c_uint32, C.c_void_p, C.c_int, C.c_uint32, C.c_void_p]),
}


def build():
    return _emu.build_lib(NAME, SRCS, OPT)


def lib():
    return _emu.shared_lib(NAME, SRCS, OPT, prototypes=PROTOTYPES)


class Packed(_emu.PackedScene):
    """pack_scene's output of (cfg, desc): the pair table and the root's box, the refit's bodies over them, and the cost bodies"""
    PREFIX, lib = "cost_emu", staticmethod(lib)
    SIZES = ("n_pairs", "n_slots", "n_levels", "n_nodes", "root_is_leaf", "root_leaf_count")
    KEYS = ("pairs", "root")

    def update(self, vertices):
        """the refit's bodies over the boxes, serially; True = refused (a non-finite vertex)"""
        v = np.ascontiguousarray(vertices, dtype=np.float32)
        assert v.size >= 12 * self.n_tris
        return bool(lib().cost_emu_update(self.handle, self.n_tris, ptr(v)))

    def cost(self):
        """(cost, S) of the table as it is now: uploaded, or refitted by update()"""
        out = np.zeros(2, dtype=np.float64)
        lib().cost_emu_cost(self.handle, ptr(out))
        return float(out[0]), float(out[1])


def table_cost(pairs, root=None, leaf_count=None):
    """(cost, S) of a caller's table: pairs [n] of PAIR_DTYPE under an inner root -- or, with leaf_count, of a leaf root of that many triangles
    with the box root (6 floats)"""
    out = np.zeros(2, dtype=np.float64)
    if leaf_count is not None:
        r = np.ascontiguousarray(root, dtype=np.float32)
        assert r.size == 6
        lib().cost_emu_table(None, 0, ptr(r), 1, int(leaf_count), ptr(out))
    else:
        p = _emu.aligned_copy(np.asarray(pairs, dtype=PAIR_DTYPE).reshape(-1), PAIR_DTYPE)
        assert len(p) >= 1
        lib().cost_emu_table(ptr(p), len(p), None, 0, 0, ptr(out))
    return float(out[0]), float(out[1])
