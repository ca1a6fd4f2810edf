"""tests/emu/refit_api.py -- TEST INFRASTRUCTURE: builds and binds tests/emu/librefit_emu.so, the bodies of the refit kernels
(csrc/hip/pt_refit.h) compiled for the host and run serially over pack_scene's output (refit_emu.cpp)."""
import ctypes as C

import numpy as np

import _emu
from _emu import PAIR_DTYPE, ptr          # noqa: F401  (PAIR_DTYPE: for the tests)

NAME, SRCS, OPT = "refit_emu", [_emu.src("refit_emu.cpp"), _emu.PACK], "-O2"
LIB = _emu.lib_path(NAME)
PROTOTYPES = {
    "refit_emu_pack": (C.c_int, [C.c_void_p, C.c_void_p, C.POINTER(C.c_void_p), C.c_char_p, C.c_int]),
    "refit_emu_free": (None, [C.c_void_p]),
    "refit_emu_sizes": (None, [C.c_void_p, C.c_void_p]),
    "refit_emu_get": (None, [C.c_void_p] + [C.c_void_p] * 8),
    "refit_emu_update": (C.c_int, [C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p]),
}


def build():
    return _emu.build_lib(NAME, SRCS, OPT)


def lib():
    return _emu.shared_lib(NAME, SRCS, OPT, prototypes=PROTOTYPES)


class Packed(_emu.PackedScene):
    """pack_scene's output of (cfg, desc): the records and the refit tables, and the refit bodies run over them"""
    PREFIX, lib = "refit_emu", staticmethod(lib)
    SIZES = ("n_pairs", "n_slots", "n_levels", "n_nodes", "root_is_leaf", "stack_levels")
    KEYS = ("pairs", "tri_geom", "tri_nrm", "root", "slot_vtx", "level_pairs", "level_first", "node_box")

    def update(self, vertices, normals=None):
        """the refit bodies, serially; True = refused (a non-finite vertex)"""
        v = np.ascontiguousarray(vertices, dtype=np.float32)
        n = None if normals is None else np.ascontiguousarray(normals, dtype=np.float32)
        assert v.size >= 12 * self.n_tris and (n is None or n.size >= 12 * self.n_tris)
        return bool(lib().refit_emu_update(self.handle, self.n_tris, ptr(v), ptr(n)))
