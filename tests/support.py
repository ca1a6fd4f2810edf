"""tests/support.py -- TEST INFRASTRUCTURE: the small helpers the test files share (a plain module: no fixtures, no hooks)."""
import importlib

import numpy as np

PKG_NAME = "photorealistic-rendering-using-opencl_amd"


def pkg():
    """the product package, for tests that need no built library (its Python side only)"""
    return importlib.import_module(PKG_NAME)


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
