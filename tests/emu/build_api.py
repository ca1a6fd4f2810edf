"""tests/emu/build_api.py -- TEST INFRASTRUCTURE: builds and binds tests/emu/libbuild_emu.so, the bodies of the build kernels
(csrc/hip/pt_build.h) and of the refit kernels compiled for the host and run serially over pack_scene's output (build_emu.cpp)."""
import ctypes as C

import numpy as np

import _emu
from _emu import PAIR_DTYPE, ptr          # noqa: F401  (PAIR_DTYPE: for the tests)

NAME, SRCS, OPT = "build_emu", [_emu.src("build_emu.cpp"), _emu.PACK], "-O2"
LIB = _emu.lib_path(NAME)
PROTOTYPES = {
    "build_emu_pack": (C.c_int, [C.c_void_p, C.c_void_p, C.POINTER(C.c_void_p), C.c_char_p, C.c_int]),
    "build_emu_free": (None, [C.c_void_p]),
    "build_emu_sizes": (None, [C.c_void_p, C.c_void_p]),
    "build_emu_get": (None, [C.c_void_p] + [C.c_void_p] * 9),
    "build_emu_set_motion": (None, [C.c_void_p, C.c_int]),
    "build_emu_consume_snapshot": (None, [C.c_void_p]),
    "build_emu_update": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p]),
    "build_emu_rebuild": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32]),
    "build_emu_read_bvh": (C.c_uint32, [C.c_void_p, C.c_void_p, C.c_void_p]),
}

NODE_DTYPE = np.dtype([("bounds", "<f4", 6), ("first", "<u4"), ("count", "<u4"), ("leaf", "u1"), ("_p", "u1", 3)])      # prt_bvh_node
REFUSED = {1: "a non-finite vertex", 2: "normals None and a triangle without a normal record", 3: "max_leaf above 64"}


def build():
    return _emu.build_lib(NAME, SRCS, OPT)


def lib():
    return _emu.shared_lib(NAME, SRCS, OPT, prototypes=PROTOTYPES)


class Packed(_emu.PackedScene):
    """pack_scene's output of (cfg, desc), and prt_update_vertices / prt_rebuild_bvh run over it serially by the kernels' bodies"""
    PREFIX, lib = "build_emu", staticmethod(lib)
    SIZES = ("n_pairs", "n_slots", "n_levels", "n_nodes", "root_is_leaf", "stack_levels", "root_leaf_first", "root_leaf_count", "snap_valid", "n_prev")
    KEYS = ("pairs", "tri_geom", "tri_nrm", "root", "slot_vtx", "level_pairs", "level_first", "node_box", "prev")

    def _tables(self):
        return dict(super()._tables(), prev=np.zeros((self.n_prev, 48), dtype=np.uint8))

    def get(self):
        """PackedScene.get's copies, with prev uint8 [n_prev, 48] (bytes) and the scalars"""
        out = super().get()
        out["scalars"] = np.array([self.n_pairs, self.n_slots, self.n_levels, self.root_is_leaf, self.stack_levels, self.root_leaf_first,
                                   self.root_leaf_count], dtype=np.uint32)
        return out

    def _arrays(self, vertices, normals):
        v = np.ascontiguousarray(vertices, dtype=np.float32)
        n = None if normals is None else np.ascontiguousarray(normals, dtype=np.float32)
        assert v.size >= 12 * self.n_tris and (n is None or n.size >= 12 * self.n_tris)
        return v, n

    def set_motion(self, on):
        lib().build_emu_set_motion(self.handle, 1 if on else 0)
        self._sizes()

    def consume_snapshot(self):
        lib().build_emu_consume_snapshot(self.handle)
        self._sizes()

    def update(self, vertices, normals=None):
        v, n = self._arrays(vertices, normals)
        rc = int(lib().build_emu_update(self.handle, ptr(v), ptr(n)))
        self._sizes()
        return rc

    def rebuild(self, vertices, normals=None, max_leaf=0):
        """the build bodies, serially; 0, or a key of REFUSED (nothing was written)"""
        v, n = self._arrays(vertices, normals)
        rc = int(lib().build_emu_rebuild(self.handle, ptr(v), ptr(n), int(max_leaf)))
        assert rc < 100, "the build bodies left inconsistent tables (%d)" % rc
        self._sizes()
        return rc

    def read_bvh(self):
        """(nodes, primitive_indices) of a rebuilt tree, as prt_read_bvh makes them"""
        nodes = np.zeros(int(lib().build_emu_read_bvh(self.handle, None, None)), dtype=NODE_DTYPE)
        prims = np.zeros(self.n_slots, dtype=np.uint64)
        lib().build_emu_read_bvh(self.handle, ptr(nodes), ptr(prims))
        return nodes, prims
