"""tests/emu/emu_api.py -- TEST INFRASTRUCTURE: builds and binds tests/emu/libpt_emu.so, the product's device header
(csrc/hip/pt_device.h) compiled for the host and driven by a wave emulator (pt_emu.cpp)."""
import ctypes as C

import numpy as np

import _emu
from _emu import ptr, ref

NAME, SRCS, OPT, DEFINES = "pt_emu", [_emu.src("pt_emu.cpp"), _emu.PACK], "-O2", ("PT_EMU",)
LIB = _emu.lib_path(NAME)
PROTOTYPES = {
    "emu_render": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int,
                             C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int,
                             C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p,
                             C.c_uint32, C.c_uint32, C.c_uint32, C.c_char_p, C.c_int, C.c_uint32, C.c_void_p,
                             C.c_uint32, C.c_float, C.c_void_p]),
    "emu_select_variant": (C.c_int, [C.c_uint32, C.c_int, C.c_uint32, C.c_int, C.c_int, C.c_int, C.c_uint32, C.c_uint32, C.c_int, C.c_int,
                                     C.POINTER(C.c_uint32), C.POINTER(C.c_int), C.POINTER(C.c_char_p)]),
    "emu_last_variant": (C.c_char_p, []),
    "emu_variant_row": (C.c_int, [C.c_int, C.POINTER(C.c_uint32), C.POINTER(C.c_int), C.POINTER(C.c_char_p), C.POINTER(C.c_char_p)]),
    "emu_selftest_fn": (None, [C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int]),
    "emu_selftest_env": (None, [C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_int]),
}


def build():
    return _emu.build_lib(NAME, SRCS, OPT, DEFINES)


def lib():
    return _emu.shared_lib(NAME, SRCS, OPT, DEFINES, PROTOTYPES)


def select_variant(active_mats, has_medium, n_sdfs, view, pick_random_light, env_is, dist_mask, filter_kind, generic, any_dist):
    """the row of the variant table (csrc/hip/pt_variant.h) launch_render takes: (MATS, MEDIUM, name), or None if select_variant names no row"""
    mats, medium, name = C.c_uint32(), C.c_int(), C.c_char_p()
    i = lib().emu_select_variant(active_mats, has_medium, n_sdfs, view, pick_random_light, env_is, dist_mask, filter_kind, generic, any_dist,
                                 C.byref(mats), C.byref(medium), C.byref(name))
    return None if i < 0 else (mats.value, bool(medium.value), name.value.decode())


def last_variant():
    """the name of the row the last render() ran (what prt_kernel_variant reports of a launch, without its wave count and mapping)"""
    return lib().emu_last_variant().decode()


def variant_table():
    """every row of the variant table: [(MATS, MEDIUM, name, instance file)]"""
    mats, medium, name, file = C.c_uint32(), C.c_int(), C.c_char_p(), C.c_char_p()
    rows = []
    for i in range(lib().emu_variant_row(-1, C.byref(mats), C.byref(medium), C.byref(name), C.byref(file))):
        lib().emu_variant_row(i, C.byref(mats), C.byref(medium), C.byref(name), C.byref(file))
        rows.append((mats.value, bool(medium.value), name.value.decode(), file.value.decode()))
    return rows


def selftest_fn(fn, params, cases):
    params = np.ascontiguousarray(params, dtype=np.float32)
    cases = np.ascontiguousarray(cases, dtype=np.float32)
    out = np.zeros_like(cases)
    lib().emu_selftest_fn(int(fn), ptr(params), ptr(cases), ptr(out), cases.shape[0])
    return out


def selftest_env(fn, env, cases):
    """prt_selftest_fn fn 13 / 14 on the host: env float32 [h, w, 3], cases [n, 32] -> [n, 32] (csrc/hip/pt_selftest.h selftest_env)"""
    env = np.ascontiguousarray(env, dtype=np.float32)
    cases = np.ascontiguousarray(cases, dtype=np.float32)
    assert env.ndim == 3 and env.shape[2] == 3 and cases.ndim == 2 and cases.shape[1] == 32
    out = np.zeros_like(cases)
    lib().emu_selftest_env(int(fn), ptr(env), env.shape[1], env.shape[0], ptr(cases), ptr(out), cases.shape[0])
    return out


def render(state_dtype, cfg, desc, camera, W, H, seed_pairs, first_frame=1, state=None, env=None, spp_limit=0,
           walk_min_lanes=8, sched_seed=0, row0=0, rows=None, blocks=None, img=None, window=None, ahead=None, pixel_filter=None):
    """same call shape as oracle_api.Restatement.render.  pixel_filter = (kind 1 .. 4, radius, table): prt_set_pixel_filter's state, run
    through the PT_MATS_FILTER builds; table = the 257 float32 entries T[0 .. 256] of the Gaussian and Blackman-Harris kinds, None otherwise.  `window` / `ahead`: the launch covers the first `window` frames of
    seed_pairs only, but (FrameArgs::run_ahead, "N spp" launches) a lane may go on into the rest while its wave waits for
    others; `ahead` (uint32 per pixel, in / out) is how far each pixel is into the NEXT launch."""
    if blocks is not None:
        rows = sum(1 for r in range(H) if (r // blocks[0]) % blocks[1] == blocks[2])
    rows = H if rows is None else rows
    seed_frames = len(seed_pairs) // 2
    n_frames = seed_frames if window is None else min(window, seed_frames)
    if state is None:
        state = np.zeros(W * rows, dtype=state_dtype)
    if img is None:
        img = np.zeros((rows, W, 4), dtype=np.float32)      # a launch only writes the pixels it advanced (like the framebuffer)
    seeds = np.ascontiguousarray(seed_pairs, dtype=np.int32)
    envp, ew, eh = None, 0, 0
    if env is not None:
        env = np.ascontiguousarray(env, dtype=np.float32)
        envp, eh, ew = ptr(env), env.shape[0], env.shape[1]
    b = blocks if blocks is not None else (1, 1, 0)
    fkind, frad, ftab = 0, 0.0, None
    if pixel_filter is not None:
        fkind, frad, ftab = pixel_filter
        if ftab is not None:
            ftab = np.ascontiguousarray(ftab, dtype=np.float32)
            assert ftab.shape == (257,)
    err = C.create_string_buffer(256)
    rc = lib().emu_render(ref(cfg), ref(desc), ref(camera), envp, ew, eh, W, H, row0, rows, b[0], b[1], b[2], first_frame, n_frames,
                          ptr(seeds), ptr(state), ptr(img), spp_limit, walk_min_lanes, sched_seed, err, 256, seed_frames,
                          ptr(ahead), int(fkind), float(frad), ptr(ftab))
    if rc:
        e = RuntimeError("emu_render failed (%d): %s" % (rc, err.value.decode()))
        e.code = rc
        raise e
    return state, img
