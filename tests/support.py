"""tests/support.py -- TEST INFRASTRUCTURE: the small helpers the test files share (a plain module: no fixtures, no hooks)."""
import ctypes as C
import importlib
import os
import sys

import numpy as np

from conftest import PKG_NAME, ROOT, VARIANTS, variant_camera, variant_config

sys.path.insert(0, os.path.join(ROOT, "tests", "emu"))      # the host emulators' bindings (emu_api, refit_api, ...): once, for every test file


def pkg():
    """the product package, for tests that need no built library (its Python side only)"""
    return importlib.import_module(PKG_NAME)


def variant_case(prt, variant, W, H, scene=None):
    """(scene, cfg, cam, env) of a variant of conftest.VARIANTS at W x H: its scene file (or the HostScene given), its config with the
    variant's phase function, the reference's default camera and the 64 x 32 sky where the variant uses one (else None)"""
    scene_json, phase, use_env = VARIANTS[variant]
    scene = scene or prt.HostScene(scene_json)
    cfg = variant_config(scene, variant)
    cfg.phase_function = phase
    return scene, cfg, variant_camera(prt, variant, W, H), (prt.make_sky(64, 32) if use_env else None)


def assert_api(names, prt=None):
    """each name is declared in include/prt.h as `int name(prt_ctx*`, bound in _capi.PRT_API and exported by the built libprt.so: by the file
    itself and by the library as the package loads it, every prototype bound (built here if it is missing and no `prt` fixture, which
    builds it, was given).  Returns the header's text for what else a test looks for in it"""
    with open(os.path.join(ROOT, "include", "prt.h")) as f:
        header = f.read()
    capi = importlib.import_module(PKG_NAME + "._capi")
    bound = {n for n, _, _ in capi.PRT_API}
    lib = os.path.join(ROOT, PKG_NAME, "libprt.so")
    if prt is None and not os.path.exists(lib):
        import __graft_entry__ as ge
        ge.build()
    libs = [capi.load_library(), C.CDLL(lib)]           # (in this order: load_library brings torch's HIP runtime in first)
    for name in names:
        assert ("int %s(prt_ctx*" % name) in header, "%s is not declared in include/prt.h" % name
        assert name in bound, "%s is not in _capi.PRT_API" % name
        assert all(hasattr(l, name) for l in libs), "%s is not exported by libprt.so" % name
    return header


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def bytes_flat(a):
    return np.ascontiguousarray(a).view(np.uint8).reshape(-1)


def bytes_rows(state):
    """one row of bytes per element of a record array"""
    return np.ascontiguousarray(state).view(np.uint8).reshape(state.size, -1)


def assert_same_render(oracle, want_state, want_img, state, img, what):
    """path state equal to the oracle's field for field, and the framebuffer equal to its image"""
    bad = oracle.state_fields_equal(want_state.view(oracle.PATH_STATE_DTYPE), state.view(oracle.PATH_STATE_DTYPE))
    assert not bad, "%s: path state differs in %s" % (what, bad)
    assert oracle.images_equal(want_img, img), "%s: framebuffer differs" % what


def relmse(x, ref):
    return float(np.mean((x[..., :3] - ref[..., :3]) ** 2 / (ref[..., :3] ** 2 + 1e-2)))


def rodrigues(x, axis, ang):
    """x turned by ang about axis (normalised here: a unit axis whose float64 norm is exactly 1 is left as it is, bit for bit)"""
    axis = np.asarray(axis, dtype=np.float64)
    axis = axis / np.linalg.norm(axis)
    return x * np.cos(ang) + np.cross(axis, x) * np.sin(ang) + axis * (axis @ x) * (1 - np.cos(ang))


def to_device(a):
    """a numpy array as a tensor on cuda:0, finished (the library's streams do not wait for torch's)"""
    import torch
    t = torch.from_numpy(np.ascontiguousarray(a)).to("cuda:0")
    torch.cuda.synchronize()
    return t
