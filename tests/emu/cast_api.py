"""tests/emu/cast_api.py -- TEST INFRASTRUCTURE: builds and binds tests/emu/libcast_emu.so, the per-ray bodies of the ray queries
(csrc/hip/pt_cast.h) compiled for the host over a scene packed by pt_pack.cpp (cast_emu.cpp), as emu_api.py does for the lane machine."""
import ctypes as C

import numpy as np

import _emu
from _emu import aligned, ptr, ref

RAY_FLOATS, HIT_WORDS = 8, 12
# numpy view of prt_hit (include/prt.h)
HIT_DTYPE = np.dtype([("t", "<f4"), ("u", "<f4"), ("v", "<f4"), ("tri", "<u4"), ("normal", "<f4", 3), ("id", "<i4"), ("pos", "<f4", 3), ("flags", "<u4")])
assert HIT_DTYPE.itemsize == 48
GUARD = 0xA5A5A5A5

NAME, SRCS, OPT, DEFINES = "cast_emu", [_emu.src("cast_emu.cpp"), _emu.PACK], "-O2", ("PT_EMU",)
LIB = _emu.lib_path(NAME)
PROTOTYPES = {
    "cast_emu": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_uint32, C.c_void_p, C.c_uint32, C.c_void_p, C.c_char_p, C.c_int]),
    "cast_emu_pixel_rays": (None, [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_uint32, C.c_void_p]),
    "cast_emu_root_box": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p]),
}


def build():
    return _emu.build_lib(NAME, SRCS, OPT, DEFINES)


def lib():
    return _emu.shared_lib(NAME, SRCS, OPT, DEFINES, PROTOTYPES)


def _rays(rays):
    rays = np.asarray(rays, dtype=np.float32).reshape(-1, RAY_FLOATS)
    r = aligned((max(len(rays), 1), RAY_FLOATS), np.float32)
    r[:len(rays)] = rays
    return r, len(rays)


def _run(cfg, desc, any_hit, sched, rays, words):
    r, n = _rays(rays)
    out = aligned((n * words + 16,), np.uint32)            # 16 guard words behind the n records
    out[:] = GUARD
    err = C.create_string_buffer(256)
    rc = lib().cast_emu(ref(cfg), ref(desc), int(any_hit), int(sched), ptr(r), n, ptr(out), err, 256)
    if rc:
        raise RuntimeError("cast_emu failed (%d): %s" % (rc, err.value.decode()))
    assert (out[n * words:] == GUARD).all(), "cast_emu wrote behind its %d records" % n
    return out[:n * words].copy()


def cast(cfg, desc, rays, sched=1):
    """prt_cast_rays on the host: rays float32 [n, 8] -> HIT_DTYPE [n].  sched: 0 the plain loop, 1 the kernel's schedule, >= 2 a random one"""
    return _run(cfg, desc, 0, sched, rays, HIT_WORDS).view(HIT_DTYPE)


def occluded(cfg, desc, rays, sched=1):
    """prt_occluded on the host: uint32 [n]"""
    return _run(cfg, desc, 1, sched, rays, 1)


def pixel_rays(cam, width, full_height, xy):
    """the rays prt_cast_pixels generates for the (x, y) pairs xy: float32 [n, 8]"""
    xy = np.ascontiguousarray(xy, dtype=np.int32).reshape(-1, 2)
    r = aligned((max(len(xy), 1), RAY_FLOATS), np.float32)
    lib().cast_emu_pixel_rays(ref(cam), int(width), int(full_height), ptr(xy), len(xy), ptr(r))
    return r[:len(xy)].copy()


def root_box(cfg, desc):
    """float32 [6] = min_x max_x min_y max_y min_z max_z of the packed tree's root (zeros for a scene without triangles)"""
    box = np.zeros(6, dtype=np.float32)
    rc = lib().cast_emu_root_box(ref(cfg), ref(desc), ptr(box))
    if rc:
        raise RuntimeError("pack_scene failed (%d)" % rc)
    return box
