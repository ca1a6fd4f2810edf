"""Which door of the C ABI a Renderer method takes for which argument, and what arrives there -- without a device: a Renderer made with
Renderer.__new__ over a stub library that records (symbol, arguments) and returns 0.  numpy arrays and None take the host door, integer
addresses the device door (tensors need a device: the ..._through_both_doors GPU tests); mode, max_leaf and count arrive as given; a short
array is refused before any call; the node count is re-read after whatever may have built a new tree.
"""
import ctypes as C

import numpy as np
import pytest

T, MESHES, BONES, TARGETS = 2, 3, 4, 3
NODES_UPLOADED, NODES_READ = 3, 7
ADDR, ADDR2 = 0x7F0000001000, 0x7F0000002000
f32 = np.float32


class StubLib:
    """every attribute is a function that records its call; prt_read_bvh writes a node count through its byref argument"""

    def __init__(self):
        self.calls = []

    def __getattr__(self, name):
        def fn(*args):
            self.calls.append((name, args))
            if name == "prt_read_bvh" and args[2] is not None:
                args[2]._obj.value = NODES_READ
            return 0
        return fn


def _addr(p):
    """the address a recorded pointer argument carries (None for NULL)"""
    if p is None or isinstance(p, int):
        return p
    return C.cast(p, C.c_void_p).value


@pytest.fixture()
def r(prt):
    r = prt.Renderer.__new__(prt.Renderer)
    r.lib, r.ctx = StubLib(), C.c_void_p(1)
    r.width = r.height = r.rows = 0
    r.triangle_count, r.mesh_count, r.bvh_node_count = T, MESHES, NODES_UPLOADED      # (as upload_scene leaves them)
    r._skin, r._morph, r._policy = (BONES, True), (TARGETS, True), False
    yield r
    r.ctx = C.c_void_p()                                    # (nothing for close() to destroy)


def _deformer_calls(prt, r):
    """(method, symbol, arrays of the full size, what follows the arrays on the host call with rebuild / max_leaf as given)"""
    v, n = np.ones((3 * T, 4), dtype=f32), np.ones((3 * T, 4), dtype=f32)
    M, w = np.ones((BONES, 12), dtype=f32), np.ones(TARGETS, dtype=f32)
    return [(r.update_vertices, "prt_update_vertices", (v, n), False), (r.rebuild_bvh, "prt_rebuild_bvh", (v, n), False),
            (r.pose, "prt_pose", (M,), True), (r.morph, "prt_morph", (w,), True), (r.pose_morphed, "prt_pose_morphed", (M, w), True)]


def _tail(symbol, rebuild, mode, max_leaf):
    if "update_vertices" in symbol:
        return (), {}
    if "rebuild_bvh" in symbol:
        return (max_leaf,), {"max_leaf": max_leaf}
    return (mode, max_leaf), {"rebuild": rebuild, "max_leaf": max_leaf}


def _first(r):
    """the first recorded call without the context, pointers as addresses"""
    name, args = r.lib.calls[0]
    assert args[0] is r.ctx
    return name, tuple(_addr(a) for a in args[1:])


@pytest.mark.parametrize("rebuild,mode", [(False, 0), (True, 1), (2, 2)])
def test_numpy_and_none_take_the_host_door(prt, r, rebuild, mode):
    for which in range(5):
        for null in (False, True):
            r.lib.calls.clear()
            call, symbol, arrays, _ = _deformer_calls(prt, r)[which]
            tail, kw = _tail(symbol, rebuild, mode, 5)
            call(*([None] * len(arrays) if null else arrays), **kw)
            want = tuple(None if null else a.ctypes.data for a in arrays)
            assert _first(r) == (symbol, want + tail), symbol


@pytest.mark.parametrize("rebuild,mode", [(False, 0), (True, 1), (2, 2)])
def test_an_address_takes_the_device_door(prt, r, rebuild, mode):
    for which in range(5):
        r.lib.calls.clear()
        call, symbol, arrays, _ = _deformer_calls(prt, r)[which]
        tail, kw = _tail(symbol, rebuild, mode, 64)
        addrs = (ADDR, ADDR2)[:len(arrays)]
        call(*addrs, **kw)
        assert _first(r) == (symbol + "_device", addrs + tail), symbol
    # normals None beside a vertex address: NULL through the device door
    for call, symbol, tail in ((r.update_vertices, "prt_update_vertices_device", ()), (r.rebuild_bvh, "prt_rebuild_bvh_device", (0,))):
        r.lib.calls.clear()
        call(ADDR)
        assert _first(r) == (symbol, (ADDR, None) + tail)


def test_defaults_are_refit_and_the_librarys_leaf_size(prt, r):
    for which in (2, 3, 4):
        r.lib.calls.clear()
        call, symbol, arrays, _ = _deformer_calls(prt, r)[which]
        call(*arrays)
        assert _first(r)[1][-2:] == (prt._capi.POSE_REFIT, 0)
    r.lib.calls.clear()
    r.rebuild_bvh(np.ones((3 * T, 4), dtype=f32))
    assert _first(r)[1][-2:] == (None, 0)


def test_an_array_one_element_short_is_refused_before_any_call(prt, r):
    for which in range(5):
        call, symbol, arrays, _ = _deformer_calls(prt, r)[which]
        for short in range(len(arrays)):
            args = [a.reshape(-1)[:-1].copy() if i == short else a for i, a in enumerate(arrays)]
            with pytest.raises(ValueError):
                call(*args)
            assert r.lib.calls == [], "%s with argument %d short" % (symbol, short)
    assert r.bvh_node_count == NODES_UPLOADED


def test_pose_morphed_refuses_mixed_arguments(prt, r):
    M, w = np.ones((BONES, 12), dtype=f32), np.ones(TARGETS, dtype=f32)
    for args in ((M, ADDR), (ADDR, w), (None, ADDR), (ADDR, None)):
        with pytest.raises(ValueError):
            r.pose_morphed(*args)
    assert r.lib.calls == []


def _node_count_read(r):
    reads = [args for name, args in r.lib.calls if name == "prt_read_bvh"]
    assert len(reads) <= 1 and all(a[1] is None and a[3] is None for a in reads)
    assert r.lib.calls[-1][0] == "prt_read_bvh" if reads else True, "the count is read after the call that may have built the tree"
    return bool(reads)


@pytest.mark.parametrize("device", [False, True])
def test_node_count_is_read_again_after_what_may_build_a_tree(prt, r, device):
    def args_of(arrays):
        return (ADDR, ADDR2)[:len(arrays)] if device else arrays

    for which in range(5):
        call, symbol, arrays, has_mode = _deformer_calls(prt, r)[which]
        always = symbol == "prt_rebuild_bvh"
        # a plain refit
        r.lib.calls.clear()
        r.bvh_node_count, r._policy = NODES_UPLOADED, False
        call(*args_of(arrays))
        assert _node_count_read(r) == always and r.bvh_node_count == (NODES_READ if always else NODES_UPLOADED), symbol
        # a refit under a rebuild policy
        r.lib.calls.clear()
        r.bvh_node_count, r._policy = NODES_UPLOADED, True
        call(*args_of(arrays))
        assert _node_count_read(r) and r.bvh_node_count == NODES_READ, symbol
        # a rebuild
        if has_mode:
            r.lib.calls.clear()
            r.bvh_node_count, r._policy = NODES_UPLOADED, False
            call(*args_of(arrays), rebuild=True)
            assert _node_count_read(r) and r.bvh_node_count == NODES_READ, symbol
            # an unknown mode goes to the library as it is; it is no rebuild
            r.lib.calls.clear()
            r.bvh_node_count = NODES_UPLOADED
            call(*args_of(arrays), rebuild=2)
            assert not _node_count_read(r) and r.bvh_node_count == NODES_UPLOADED, symbol


def test_turning_the_skin_and_the_set_off(prt, r):
    r.set_skin(None)
    assert r.lib.calls == [("prt_set_skin", (r.ctx, None))] and r._skin is None
    r.lib.calls.clear()
    r.set_morph_targets(None)
    assert r.lib.calls == [("prt_set_morph_targets", (r.ctx, None))] and r._morph is None
    # without them the frame's arrays have no minimum size: the library refuses the call
    r.lib.calls.clear()
    r.pose(np.zeros(0, dtype=f32))
    r.morph(np.zeros(0, dtype=f32))
    assert [name for name, _ in r.lib.calls] == ["prt_pose", "prt_morph"]


def test_update_primitives_forms(prt, r):
    Mesh = prt._capi.Mesh
    records = (Mesh * MESHES)()
    as_numpy = np.zeros(MESHES * C.sizeof(Mesh), dtype=np.uint8)
    host = [(as_numpy, as_numpy.ctypes.data), (records, C.addressof(records)), (None, None),
            (C.cast(records, C.POINTER(Mesh)), C.addressof(records)), (C.c_void_p(ADDR), ADDR)]
    for arg, want in host:
        r.lib.calls.clear()
        r.update_primitives(arg)
        assert _first(r) == ("prt_update_primitives", (want, MESHES)), type(arg)
    r.lib.calls.clear()
    r.update_primitives(records, count=2)
    assert _first(r) == ("prt_update_primitives", (C.addressof(records), 2))
    for arg in (ADDR, None):
        r.lib.calls.clear()
        r.update_primitives(arg, device=True)
        assert _first(r) == ("prt_update_primitives_device", (arg, MESHES))
    r.lib.calls.clear()
    with pytest.raises(ValueError):
        r.update_primitives(as_numpy[:-1])
    assert r.lib.calls == []


def test_ray_queries_take_the_host_door_for_numpy(prt, r):
    rays = np.zeros((5, prt._capi.RAY_FLOATS), dtype=f32)
    hits = r.cast_rays(rays)
    name, args = r.lib.calls[0]
    assert name == "prt_cast_rays" and _addr(args[1]) == rays.ctypes.data and args[2] == 5 and _addr(args[3]) == hits.ctypes.data
    assert hits.dtype == np.dtype(prt._capi.HIT_DTYPE) and hits.shape == (5,)
    r.lib.calls.clear()
    flags = r.occluded(rays)
    name, args = r.lib.calls[0]
    assert name == "prt_occluded" and _addr(args[1]) == rays.ctypes.data and args[2] == 5 and _addr(args[3]) == flags.ctypes.data
    assert flags.dtype == np.uint32 and flags.shape == (5,)
    # a list is converted and takes the host door too; a wrong shape is refused before any call
    r.lib.calls.clear()
    assert r.occluded([[0.0] * 8] * 2).shape == (2,) and r.lib.calls[0][0] == "prt_occluded" and r.lib.calls[0][1][2] == 2
    r.lib.calls.clear()
    for bad in (np.zeros((5, 7), dtype=f32), None, ADDR):
        with pytest.raises(ValueError):
            r.cast_rays(bad)
    assert r.lib.calls == []
