"""photorealistic-rendering-using-opencl_amd -- MI355X-native drop-in for the radiance loop of
Mourtz/Photorealistic-Rendering-using-OpenCL (kernels/main.cl render_kernel).

The product is `libprt.so` (hand-written HIP for gfx950 behind the C ABI of include/prt.h, plus the
C++ host model that keeps the reference's host_scene / Camera / BVH API).  This Python module is
plumbing only: it mirrors the host sequence of the reference's src/main.cpp
(load scene -> build BVH -> upload -> set camera -> render frames -> read the image) on top of the
C ABI so tests, bench.py and torch.distributed launches can drive it.  Nothing here computes
pixels and nothing falls back to a CPU path: without libprt.so or without a HIP device the calls
raise.
"""
import ctypes as C
import os

import numpy as np

from . import _capi
from ._capi import NORMALS_WEIGHTINGS, LOADER_CREASE_COS, PIXEL_FILTERS,PIXEL_FILTER_DEFAULT_RADIUS, DENOISE_DEFAULTS, DenoiseParams, TEMPORAL_DEFAULTS, TemporalParams, RESPONSE_DEFAULTS, TemporalResponse, Adaptive, AdaptiveReport, Camera, Config, SceneDesc, Stats, load_library, PATH_STATE_DTYPE

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
SCENES_DIR = os.path.join(REPO, "scenes")
MODELS_DIR = os.path.join(SCENES_DIR, "models")

__all__ = ["NORMALS_WEIGHTINGS", "LOADER_CREASE_COS", "weld_corners", "PIXEL_FILTERS","PIXEL_FILTER_DEFAULT_RADIUS", "pixel_filter_offsets", "env_cdf", "adaptive_converged", "adaptive_luminance", "Adaptive", "AdaptiveReport", "DenoiseParams", "DENOISE_DEFAULTS", "TemporalParams", "TEMPORAL_DEFAULTS", "TemporalResponse", "RESPONSE_DEFAULTS", "ensure_dragon_standin", "HostScene", "Renderer", "default_camera", "orbit_camera", "seed_pairs", "scene_arrays", "bvh_cost", "make_sky", "load_hdr", "write_hdr", "PrtError",
           "Camera", "Config", "SceneDesc", "Stats", "PATH_STATE_DTYPE", "SCENES_DIR", "MODELS_DIR", "build", "model_meshes", "build_id", "source_build_id", "check_build_id", "StaleLibrary"]


class PrtError(RuntimeError):
    """a prt_* call returned a negative prt_status (include/prt.h); `code` is that status"""
    def __init__(self, msg, code=None):
        super().__init__(msg)
        self.code = code


# prt_status, include/prt.h
PRT_OK, PRT_ERR_INVALID_ARGUMENT, PRT_ERR_NO_DEVICE, PRT_ERR_HIP, PRT_ERR_NOT_READY, PRT_ERR_UNSUPPORTED = 0, -1, -2, -3, -4, -5


def _build_module():
    import importlib.util
    spec = importlib.util.spec_from_file_location("_prt_build", os.path.join(HERE, "build.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def build(verbose=False):
    """compile libprt.so in-tree (hipcc --offload-arch=gfx950)"""
    return _build_module().build(verbose=verbose)


def build_id():
    """prt_build_id() of the loaded library: the hash of the sources, headers and flags it was built from"""
    return load_library().prt_build_id().decode()


def source_build_id():
    """the id a library built from the working tree as it is NOW would carry (build.py source_build_id)"""
    return _build_module().source_build_id()


class StaleLibrary(RuntimeError):
    pass


def check_build_id():
    """raises StaleLibrary unless the loaded libprt.so was built from the working tree as it is now.  A development variant named through
    PRT_LIB (tools/build_variant.sh: "variant-<name>-<hash of its sources>") is somebody's deliberate choice and passes as what it says."""
    have, want = build_id(), source_build_id()
    if have != want and not (os.environ.get("PRT_LIB") and have.startswith("variant-")):
        raise StaleLibrary("libprt.so was built from other sources than the working tree holds (library %s, tree %s): "
                           "rebuild with `python __graft_entry__.py build`" % (have, want))
    return have


def model_meshes(path, max_meshes=64):
    """[(triangles, welded vertices, de-indexing gives the soup back)] per mesh of a model file (csrc/host/model_loader.h)"""
    lib = load_library()
    counts = (C.c_uint32 * (3 * max_meshes))()
    err = C.create_string_buffer(512)
    n = lib.prth_model_meshes(path.encode(), counts, max_meshes, err, 512)
    if n < 0:
        raise PrtError("model load failed: %s" % err.value.decode(), n)
    return [(counts[3 * m], counts[3 * m + 1], bool(counts[3 * m + 2])) for m in range(min(n, max_meshes))]


def ensure_dragon_standin():
    """scenes/cornell_dragon.json needs scenes/models/dragon_standin.prtmesh (62 MB, ~871 k triangles):
    generated on demand by scenes/make_dragon_standin.py, never committed"""
    path = os.path.join(MODELS_DIR, "dragon_standin.prtmesh")
    if not os.path.exists(path):
        import importlib.util
        spec = importlib.util.spec_from_file_location("_make_dragon", os.path.join(SCENES_DIR, "make_dragon_standin.py"))
        mod = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(mod)
        mod.write(path)
    return path


class HostScene:
    """host_scene + ModelLoader + BVH of the reference's main() (src/main.cpp:375-415), through
    csrc/host/host_capi.h.  Holds the host buffers the C ABI consumes."""

    def __init__(self, scene_json, models_dir=None, text=False):
        self.lib = load_library()
        err = C.create_string_buffer(512)
        md = (models_dir or MODELS_DIR).encode()
        if text:
            self.handle = self.lib.prth_scene_load_text(scene_json.encode(), md, err, 512)
        else:
            path = scene_json if os.path.exists(scene_json) else os.path.join(SCENES_DIR, scene_json)
            self.handle = self.lib.prth_scene_load(path.encode(), md, err, 512)
        if not self.handle:
            raise PrtError("scene load failed: %s" % err.value.decode())
        self.desc = SceneDesc()
        self.lib.prth_scene_get_desc(self.handle, C.byref(self.desc))

    def config(self, alpha_testing=False):
        cfg = Config()
        self.lib.prth_scene_get_config(self.handle, 1 if alpha_testing else 0, C.byref(cfg))
        return cfg

    @property
    def bvh_depth(self):
        return self.lib.prth_scene_bvh_depth(self.handle)

    def close(self):
        if getattr(self, "handle", None):
            self.lib.prth_scene_free(self.handle)
            self.handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def default_camera(width, height, fovx=45.0):
    """initCamera() + buildRenderCamera() of the reference (src/main.cpp:312-319)"""
    cam = Camera()
    rc = load_library().prth_default_camera(width, height, C.c_float(fovx), C.byref(cam))
    if rc:
        raise PrtError("prth_default_camera: %d" % rc)
    return cam


def orbit_camera(width, height, fovx=45.0, d_yaw=0.0, d_pitch=0.0, d_radius=0.0, d_aperture=0.0, d_focal=0.0):
    cam = Camera()
    rc = load_library().prth_orbit_camera(width, height, C.c_float(fovx), C.c_float(d_yaw), C.c_float(d_pitch),
                                          C.c_float(d_radius), C.c_float(d_aperture), C.c_float(d_focal), C.byref(cam))
    if rc:
        raise PrtError("prth_orbit_camera: %d" % rc)
    return cam


def adaptive_luminance(acc):
    """the luminance prt_render_adaptive keeps per pixel (prt.h): 0.2126 r + 0.7152 g + 0.0722 b in float32, left to right, of acc [..., >= 3]"""
    acc = np.asarray(acc, dtype=np.float32)
    return (np.float32(0.2126) * acc[..., 0] + np.float32(0.7152) * acc[..., 1]) + np.float32(0.0722) * acc[..., 2]


def adaptive_converged(l, s2, n, rel_err, abs_floor):
    """the convergence test of prt_render_adaptive (prt.h), elementwise in numpy float32 with the device's operations in the device's order:
    m = l / n; v = max((s2 - l m) / (n (n - 1)), 0); t = rel_err max(m, abs_floor); converged = v < t^2.  l, s2: the plane of read_adaptive_stats();
    n: paths (samples >= 2).  Returns (converged, standard error of the mean = sqrt(v), mean luminance m) -- the last two for error maps."""
    f = np.float32
    l = np.asarray(l, dtype=f)
    s2 = np.asarray(s2, dtype=f)
    n = np.asarray(n, dtype=np.uint32)
    nf = n.astype(f)
    with np.errstate(divide="ignore", invalid="ignore"):
        m = l / nf
        v = np.fmax((s2 - l * m) / (nf * (n - np.uint32(1)).astype(f)), f(0))
        t = f(rel_err) * np.fmax(m, f(abs_floor))
        return v < t * t, np.sqrt(v), m


def _filter_kind(kind):
    if isinstance(kind, str):
        if kind not in PIXEL_FILTERS:
            raise ValueError("unknown pixel filter %r (one of %s)" % (kind, ", ".join(PIXEL_FILTERS)))
        return PIXEL_FILTERS[kind]
    return int(kind)


def pixel_filter_offsets(kind, radius, gx, gy, k0, n):
    """prt_pixel_filter_offsets: the filter offsets {dx, dy} of paths k0 .. k0+n-1 of global pixel (gx, gy) as float32 [n, 2] (prt.h; kind by name
    or PRT_FILTER_* number, radius None = the kind's default).  Needs no GPU"""
    out = np.zeros((int(n), 2), dtype=np.float32)
    r = -1.0 if radius is None else float(radius)
    rc = load_library().prt_pixel_filter_offsets(_filter_kind(kind), C.c_float(r), int(gx) & 0xFFFFFFFF, int(gy) & 0xFFFFFFFF,
                                                 int(k0) & 0xFFFFFFFF, int(n), out.ctypes.data_as(C.c_void_p))
    if rc:
        raise PrtError("prt_pixel_filter_offsets failed (%d): %s" % (rc, load_library().prt_last_global_error().decode()), rc)
    return out


def env_cdf(rgb):
    """prt_env_cdf: the tables prt_upload_envmap builds of a map float32 [h, w, 3] under env_importance_sampling (prt.h): (rows float32 [h + 1],
    cols float32 [h, w + 1]).  Needs no GPU"""
    rgb = np.ascontiguousarray(rgb, dtype=np.float32)
    assert rgb.ndim == 3 and rgb.shape[2] == 3
    h, w = rgb.shape[:2]
    rows, cols = np.zeros(h + 1, dtype=np.float32), np.zeros((h, w + 1), dtype=np.float32)
    rc = load_library().prt_env_cdf(rgb.ctypes.data_as(C.c_void_p), w, h, rows.ctypes.data_as(C.c_void_p), cols.ctypes.data_as(C.c_void_p))
    if rc:
        raise PrtError("prt_env_cdf failed (%d): %s" % (rc, load_library().prt_last_global_error().decode()), rc)
    return rows, cols


def weld_corners(vertices):
    """prt_weld_corners: (groups uint32 [3T], n_groups) of vertices float32 [3T, 4] -- corners at bit-identical positions (-0 = +0) share a
    group, groups numbered by first appearance (prt.h): the smoothing topology of the loader, for Renderer.set_smooth_normals.  Needs no GPU"""
    v = np.ascontiguousarray(vertices, dtype=np.float32)
    if v.size == 0 or v.size % 12:
        raise ValueError("weld_corners: needs float32 [3T, 4] with T > 0")
    T = v.size // 12
    groups, n = np.zeros(3 * T, dtype=np.uint32), C.c_uint32(0)
    rc = load_library().prt_weld_corners(v.ctypes.data_as(C.c_void_p), T, groups.ctypes.data_as(C.c_void_p), C.byref(n))
    if rc:
        raise PrtError("prt_weld_corners failed (%d): %s" % (rc, load_library().prt_last_global_error().decode()), rc)
    return groups, int(n.value)


def scene_arrays(desc):
    """numpy views (no copies: `desc`'s owner must stay alive) of a SceneDesc's triangle buffers: vertices and normals float32 [3T, 4],
    primitive_indices uint64 [T], nodes [bvh_node_count] of _capi.BVH_NODE_DTYPE"""
    T, N = int(desc.triangle_count), int(desc.bvh_node_count)

    def view(addr, nbytes, dtype):
        if not addr or not nbytes:
            return np.zeros(0, dtype=dtype)
        return np.frombuffer((C.c_char * nbytes).from_address(addr), dtype=dtype)
    return {"vertices": view(desc.vertices, 48 * T, np.float32).reshape(-1, 4), "normals": view(desc.normals, 48 * T, np.float32).reshape(-1, 4),
            "primitive_indices": view(desc.primitive_indices, 8 * T, np.uint64), "nodes": view(desc.bvh_nodes, 36 * N, np.dtype(_capi.BVH_NODE_DTYPE))}


def bvh_cost(nodes, bounds=None):
    """SAH cost of a tree in the reference's node layout (a [N] array of _capi.BVH_NODE_DTYPE), with `bounds` ([N, 6]: min_x max_x min_y max_y
    min_z max_z, e.g. Renderer.read_bvh_bounds() after a refit) in place of the nodes' own: (sum over inner nodes of area + sum over leaves
    of area x primitive_count) / area of the root, over the nodes the root reaches.  float64, pure numpy, summed in node order: the same
    inputs give the same number anywhere.  For deciding when a refitted tree has degraded enough to rebuild it; needs no device"""
    nodes = np.asarray(nodes)
    if nodes.dtype.names is None:
        nodes = nodes.view(np.dtype(_capi.BVH_NODE_DTYPE)).reshape(-1)
    b = np.asarray(nodes["bounds"] if bounds is None else bounds, dtype=np.float64).reshape(len(nodes), 6)
    leaf = nodes["leaf"] != 0
    reached = np.zeros(len(nodes), dtype=bool)
    front = np.array([0], dtype=np.int64)
    while front.size:                                   # level by level: the nodes the root reaches
        reached[front] = True
        inner = front[~leaf[front]]
        first = nodes["first"][inner].astype(np.int64)
        front = np.concatenate([first, first + 1])
        front = front[~reached[front]]
    d = np.maximum(b[:, 1::2] - b[:, 0::2], 0.0)
    area = 2.0 * (d[:, 0] * d[:, 1] + d[:, 1] * d[:, 2] + d[:, 2] * d[:, 0])
    weight = np.where(leaf, nodes["count"].astype(np.float64), 1.0)
    terms = np.where(reached, area * weight, 0.0)
    return float(np.cumsum(terms)[-1] / area[0])        # (cumsum: strictly in node order)


def seed_pairs(n_frames, first_frame=1):
    """(random0, random1) per frame: the un-seeded glibc rand() stream of the reference host,
    two values consumed by initCLKernel first (src/main.cpp:226-227,301-302)."""
    out = np.zeros(2 * n_frames, dtype=np.int32)
    rc = load_library().prth_seed_pairs(first_frame, n_frames, out.ctypes.data_as(C.c_void_p))
    if rc:
        raise PrtError("prth_seed_pairs: %d" % rc)
    return out


def make_sky(width=1024, height=512):
    """deterministic procedural RGB32F environment map (stand-in for the -hdr file no one ships)"""
    out = np.zeros((height, width, 3), dtype=np.float32)
    rc = load_library().prth_make_sky(width, height, out.ctypes.data_as(C.c_void_p))
    if rc:
        raise PrtError("prth_make_sky: %d" % rc)
    return out


def load_hdr(path):
    """loadHDR of the reference (include/Texture/texture.h:31-39): a Radiance .hdr file -> float32 [h, w, 3]"""
    lib = load_library()
    w, h = C.c_int(0), C.c_int(0)
    data = C.POINTER(C.c_float)()
    err = C.create_string_buffer(256)
    handle = lib.prth_hdr_load(os.fsencode(path), C.byref(w), C.byref(h), C.byref(data), err, 256)
    if not handle:
        raise PrtError("load_hdr: %s" % err.value.decode())
    try:
        return np.ctypeslib.as_array(data, shape=(h.value, w.value, 3)).copy()
    finally:
        lib.prth_hdr_free(handle)


def write_hdr(path, pixels, bottom_up=True):
    """saveImage() with `-encoder 1` of the reference (include/GL/cl_gl_interop.h:151-156): float32 [h, w, 3 or 4] -> a Radiance .hdr file"""
    pixels = np.ascontiguousarray(pixels, dtype=np.float32)
    assert pixels.ndim == 3 and pixels.shape[2] >= 3
    err = C.create_string_buffer(256)
    if load_library().prth_hdr_write(os.fsencode(path), pixels.ctypes.data_as(C.c_void_p), pixels.shape[1], pixels.shape[0], pixels.shape[2],
                                     1 if bottom_up else 0, err, 256):
        raise PrtError("write_hdr: %s" % err.value.decode())


class Renderer:
    """One prt context (one HIP device).  Method names follow the C ABI one to one."""

    def __init__(self, config, device=0):
        self.lib = load_library()
        self.ctx = C.c_void_p()
        rc = self.lib.prt_create(device, C.byref(config), C.byref(self.ctx))
        if rc:
            raise PrtError("prt_create failed (%d): %s" % (rc, self.lib.prt_last_global_error().decode()))
        self.width = self.height = self.rows = 0
        # what upload_scene and the set_* calls keep of the scene: the sizes the arrays of later calls are checked against
        self.triangle_count = self.mesh_count = self.bvh_node_count = 0
        self._skin = self._morph = None                    # (n_bones, has normals), (n_targets, has normals)
        self._policy = False

    def _chk(self, rc, what):
        if rc:
            raise PrtError("%s failed (%d): %s" % (what, rc, self.lib.prt_last_error(self.ctx).decode()), rc)

    def _arg(self, a, count, what, wait=True):
        """(pointer or None, is_device) of one float32 array argument of at least `count` elements: None and a numpy array are the host
        door's, a tensor on this context's device (wait: work queued on torch's current stream is waited for) and an integer address the
        device door's"""
        if a is None:
            return None, False
        if isinstance(a, np.ndarray):
            h = np.ascontiguousarray(a, dtype=np.float32)
            if h.size < count:
                raise ValueError("%s: needs float32 arrays of at least %d elements" % (what, count))
            return h.ctypes.data_as(C.c_void_p), False     # (the pointer keeps a converted copy alive)
        if wait and hasattr(a, "data_ptr"):
            import torch
            torch.cuda.current_stream(a.device).synchronize()
        return self._device_ptr(a, count, what), True

    def _through(self, name, arrays, *tail):
        """prt_X(ctx, arrays..., tail...) through its host door `name` or its device door `name`_device: the first of `arrays`, (array, least
        size) pairs, decides, and the others go with it (None is NULL through either).  A first array that is a tensor is the one whose
        stream is waited for: the call's tensors are on one device"""
        what, ptrs, device = name[4:], [], None
        for a, count in arrays:
            p, d = self._arg(a, count, what, device is None)
            if device is None:
                device = d
            elif p is not None and d != device:
                raise ValueError("%s: the arrays must all be host arrays or all be on the device" % what)
            ptrs.append(p)
        if device:
            name += "_device"
        self._chk(getattr(self.lib, name)(self.ctx, *ptrs, *tail), name)

    @staticmethod
    def _mode(rebuild):
        """PRT_POSE_* of a `rebuild` argument: False, True, or the number itself"""
        return _capi.POSE_REBUILD if rebuild is True else _capi.POSE_REFIT if rebuild is False else int(rebuild)

    def _refresh_node_count(self, mode=None):
        """the node count of a tree that may be a new one: after a rebuild (mode None: rebuild_bvh itself), and after a refit under a rebuild
        policy"""
        if mode is None or mode == _capi.POSE_REBUILD or self._policy:
            count = C.c_uint32(0)
            self._chk(self.lib.prt_read_bvh(self.ctx, None, C.byref(count), None), "prt_read_bvh")
            self.bvh_node_count = int(count.value)

    def _read(self, name, shape, dtype, *head):
        """a read-back prt_X(ctx, head..., out) into a new array"""
        out = np.zeros(shape, dtype=dtype)
        self._chk(getattr(self.lib, name)(self.ctx, *head, out.ctypes.data_as(C.c_void_p)), name)
        return out

    def _read_deformed(self, name, with_normals):
        """prt_read_posed / prt_read_morphed: (vertices, normals or None) float32 [3T, 4]"""
        v = np.zeros((3 * self.triangle_count, 4), dtype=np.float32)
        n = np.zeros_like(v) if with_normals else None
        self._chk(getattr(self.lib, name)(self.ctx, v.ctypes.data_as(C.c_void_p), None if n is None else n.ctypes.data_as(C.c_void_p)), name)
        return v, n

    def upload_scene(self, scene):
        desc = scene.desc if isinstance(scene, HostScene) else scene
        self._chk(self.lib.prt_upload_scene(self.ctx, C.byref(desc)), "prt_upload_scene")
        self.triangle_count = int(desc.triangle_count)
        self.mesh_count = int(desc.object_count[7])
        self.bvh_node_count = int(desc.bvh_node_count) if desc.triangle_count else 0
        self._skin = None                                  # (the library turns the skin off: T may have changed)
        self._morph = None                                 # (... and the morph targets)
        self._policy = False                               # (... and the rebuild policy)

    def update_vertices(self, vertices, normals=None):
        """prt_update_vertices / prt_update_vertices_device: new vertices (and normals; None keeps the uploaded ones) for the uploaded scene,
        the tree refitted on the device (prt.h).  Both float32 [3T, 4] in the layout of SceneDesc.  numpy arrays take the host entry point;
        torch tensors on this context's device (work queued on torch's current stream is waited for) or device addresses the device one"""
        floats = 12 * self.triangle_count
        self._through("prt_update_vertices", [(vertices, floats), (normals, floats)])
        self._refresh_node_count(_capi.POSE_REFIT)

    def update_primitives(self, meshes, device=False, count=None):
        """prt_update_primitives / prt_update_primitives_device: the prt_mesh records (256 bytes each, all object_count[7] of them, in the
        uploaded order) of the moved spheres, SDF primitives and quads into the uploaded scene (prt.h).  Host door: the Mesh array of a
        HostScene.desc (a ctypes array or pointer), or a numpy array / view of count x 256 bytes.  device=True, a torch tensor or an integer
        address: the device door (count x 256 bytes, 16-byte aligned; work queued on torch's current stream is waited for)"""
        count = self.mesh_count if count is None else int(count)     # (count: the uploaded scene's, unless given)
        nbytes = count * C.sizeof(_capi.Mesh)
        if hasattr(meshes, "data_ptr"):
            import torch
            if not meshes.is_contiguous() or meshes.numel() * meshes.element_size() < nbytes:
                raise ValueError("update_primitives: needs a contiguous tensor of at least %d bytes" % nbytes)
            torch.cuda.current_stream(meshes.device).synchronize()
            self._chk(self.lib.prt_update_primitives_device(self.ctx, C.c_void_p(meshes.data_ptr()), count), "prt_update_primitives_device")
            return
        if device:
            self._chk(self.lib.prt_update_primitives_device(self.ctx, C.c_void_p(int(meshes)) if meshes is not None else None, count),
                      "prt_update_primitives_device")
            return
        if isinstance(meshes, np.ndarray):
            m = np.ascontiguousarray(meshes)
            if m.nbytes < nbytes:
                raise ValueError("update_primitives: needs %d bytes of prt_mesh records" % nbytes)
            ptr = m.ctypes.data_as(C.c_void_p)
        elif meshes is None or isinstance(meshes, (int, C.c_void_p)):
            ptr = meshes
        else:
            ptr = C.cast(meshes, C.c_void_p)               # a ctypes array of Mesh, or a pointer to one
        self._chk(self.lib.prt_update_primitives(self.ctx, ptr, count), "prt_update_primitives")

    def read_bvh_bounds(self):
        """prt_read_bvh_bounds: float32 [bvh_node_count, 6] = min_x max_x min_y max_y min_z max_z per node of the uploaded tree, in its numbering"""
        return self._read("prt_read_bvh_bounds", (self.bvh_node_count, 6), np.float32)

    def rebuild_bvh(self, vertices, normals=None, max_leaf=0):
        """prt_rebuild_bvh / prt_rebuild_bvh_device: new vertices (and normals; None carries the current ones over) and a new Morton-order tree
        over all T triangles, built on the device (prt.h).  Arguments as update_vertices; max_leaf 1 .. 64, 0 = the library's default"""
        floats = 12 * self.triangle_count
        self._through("prt_rebuild_bvh", [(vertices, floats), (normals, floats)], int(max_leaf))
        self._refresh_node_count()

    def set_smooth_normals(self, groups, n_groups=None, weighting="unit", crease_cos=LOADER_CREASE_COS):
        """prt_set_smooth_normals: the smoothing topology of the uploaded mesh -- groups uint32 [3T], one id per corner (weld_corners gives the
        loader's); n_groups None = the largest id + 1; weighting "unit" (the loader's rule) or "area".  From then on update_vertices and
        rebuild_bvh with normals None generate the normals from the new vertices on the device (prt.h).  groups None turns it off"""
        if groups is None:
            self._chk(self.lib.prt_set_smooth_normals(self.ctx, None, 0, 0, C.c_float(0.0)), "prt_set_smooth_normals")
            return
        g = np.ascontiguousarray(groups, dtype=np.uint32).reshape(-1)
        if g.size < 3 * self.triangle_count:
            raise ValueError("set_smooth_normals: needs %d group ids" % (3 * self.triangle_count))
        if isinstance(weighting, str):
            if weighting not in NORMALS_WEIGHTINGS:
                raise ValueError("unknown weighting %r (one of %s)" % (weighting, ", ".join(NORMALS_WEIGHTINGS)))
            weighting = NORMALS_WEIGHTINGS[weighting]
        if n_groups is None:
            n_groups = int(g.max()) + 1 if g.size else 0
        self._chk(self.lib.prt_set_smooth_normals(self.ctx, g.ctypes.data_as(C.c_void_p), int(n_groups), int(weighting), C.c_float(crease_cos)),
                  "prt_set_smooth_normals")

    def read_normals(self):
        """prt_read_normals: float32 [3T, 4], the current normal records in corner order (lane 3 = 0; zeros for a triangle no leaf holds)"""
        return self._read("prt_read_normals", (3 * self.triangle_count, 4), np.float32)

    def set_skin(self, rest_vertices, rest_normals=None, bone_index=None, bone_weight=None, n_bones=0):
        """prt_set_skin: the rest pose (float32 [3T, 4]; rest_normals None = no normals are posed) and the influences of every corner
        (bone_index uint16 [3T, 4], bone_weight float32 [3T, 4]) of the uploaded mesh, n_bones 1 .. 65536.  From then on pose() moves the
        mesh from n_bones 3x4 matrices (prt.h).  rest_vertices None turns it off"""
        if rest_vertices is None:
            self._chk(self.lib.prt_set_skin(self.ctx, None), "prt_set_skin")
            self._skin = None
            return
        corners = 3 * self.triangle_count
        v = np.ascontiguousarray(rest_vertices, dtype=np.float32)
        n = None if rest_normals is None else np.ascontiguousarray(rest_normals, dtype=np.float32)
        b = None if bone_index is None else np.ascontiguousarray(bone_index, dtype=np.uint16)
        w = None if bone_weight is None else np.ascontiguousarray(bone_weight, dtype=np.float32)
        if any(a is not None and a.size < 4 * corners for a in (v, n, b, w)):
            raise ValueError("set_skin: needs arrays of at least %d elements" % (4 * corners))
        ptr = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)
        skin = _capi.Skin(ptr(v), ptr(n), ptr(b), ptr(w), int(n_bones), 0)
        self._chk(self.lib.prt_set_skin(self.ctx, C.byref(skin)), "prt_set_skin")
        self._skin = (int(n_bones), n is not None)

    def pose(self, matrices, rebuild=False, max_leaf=0):
        """prt_pose / prt_pose_device: the mesh posed on the device from n_bones 3x4 row-major matrices (float32 [n_bones, 12] or [n_bones, 3, 4]),
        then refitted (rebuild False) or rebuilt (rebuild True, max_leaf as rebuild_bvh).  A numpy array takes the host door; a torch tensor
        on this context's device (work queued on torch's current stream is waited for) or a device address the device door"""
        mode = self._mode(rebuild)
        self._through("prt_pose", [(matrices, 12 * self._skin[0] if self._skin else 0)], mode, int(max_leaf))
        self._refresh_node_count(mode)

    def read_posed(self):
        """prt_read_posed: (vertices, normals) float32 [3T, 4] of the last pose, accepted or refused; normals None for a skin without rest normals"""
        return self._read_deformed("prt_read_posed", bool(self._skin and self._skin[1]))

    def set_morph_targets(self, base_vertices, base_normals=None, targets=None, layout="corners"):
        """prt_set_morph_targets: the base mesh (float32 [3T, 4]; base_normals None = no normals are morphed) and the targets, a list of
        (corner uint32 [n], d_position float32 [n, 4], d_normal float32 [n, 4] or None) with strictly ascending corners.  From then on
        morph() moves the mesh from one weight per target, and pose_morphed() morphs in front of the skin (prt.h).  base_vertices None turns
        it off.  layout "corners" (prt_set_morph_targets' per-corner table) or "planes" (prt_set_morph_targets_layout: one plane per target
        and block of 64 corners, a morph costs the planes of the targets with a non-zero weight); morph_report() tells which suits a set"""
        if isinstance(layout, str):
            if layout not in _capi.MORPH_LAYOUTS:
                raise ValueError("unknown layout %r (one of %s)" % (layout, ", ".join(_capi.MORPH_LAYOUTS)))
            layout = _capi.MORPH_LAYOUTS[layout]
        if base_vertices is None:
            self._chk(self.lib.prt_set_morph_targets(self.ctx, None), "prt_set_morph_targets")
            self._morph = None
            return
        corners = 3 * self.triangle_count
        v = np.ascontiguousarray(base_vertices, dtype=np.float32)
        n = None if base_normals is None else np.ascontiguousarray(base_normals, dtype=np.float32)
        if any(a is not None and a.size < 4 * corners for a in (v, n)):
            raise ValueError("set_morph_targets: needs base arrays of at least %d elements" % (4 * corners))
        ptr = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)
        keep = []
        for t, target in enumerate(targets or ()):
            corner, dp, dn = target
            corner = None if corner is None else np.ascontiguousarray(corner, dtype=np.uint32).reshape(-1)
            dp = None if dp is None else np.ascontiguousarray(dp, dtype=np.float32)
            dn = None if dn is None else np.ascontiguousarray(dn, dtype=np.float32)
            entries = 0 if corner is None else corner.size
            if any(a is not None and a.size < 4 * entries for a in (dp, dn)):
                raise ValueError("set_morph_targets: target %d needs delta arrays of at least %d elements" % (t, 4 * entries))
            keep.append((corner, dp, dn, entries))
        records = (_capi.MorphTarget * max(len(keep), 1))()
        for t, (corner, dp, dn, entries) in enumerate(keep):
            records[t] = _capi.MorphTarget(ptr(corner), ptr(dp), ptr(dn), entries, 0)
        desc = _capi.MorphSet(ptr(v), ptr(n), records if targets is not None else None, len(keep), 0)
        if layout == _capi.MORPH_LAYOUT_CORNERS:
            self._chk(self.lib.prt_set_morph_targets(self.ctx, C.byref(desc)), "prt_set_morph_targets")
        else:
            self._chk(self.lib.prt_set_morph_targets_layout(self.ctx, C.byref(desc), int(layout)), "prt_set_morph_targets_layout")
        self._morph = (len(keep), n is not None)

    def morph_report(self):
        """prt_get_morph_report of the set in force: dict of layout ("corners" / "planes"), n_targets, entries, planes, table_bytes (the device
        bytes of the delta tables alone) and fill = entries / (64 planes) (None under "corners"): planes suit a set whose fill is high"""
        rep = _capi.MorphReport()
        self._chk(self.lib.prt_get_morph_report(self.ctx, C.byref(rep)), "prt_get_morph_report")
        names = {v: k for k, v in _capi.MORPH_LAYOUTS.items()}
        return {"layout": names.get(int(rep.layout), int(rep.layout)), "n_targets": int(rep.n_targets), "entries": int(rep.entries),
                "planes": int(rep.planes), "table_bytes": int(rep.table_bytes),
                "fill": rep.entries / (64.0 * rep.planes) if rep.planes else None}

    def morph(self, weights, rebuild=False, max_leaf=0):
        """prt_morph / prt_morph_device: the mesh morphed on the device from one float32 weight per target, then refitted (rebuild False) or
        rebuilt (rebuild True, max_leaf as rebuild_bvh).  A numpy array takes the host door; a torch tensor on this context's device (work
        queued on torch's current stream is waited for) or a device address the device door"""
        mode = self._mode(rebuild)
        self._through("prt_morph", [(weights, self._morph[0] if self._morph else 0)], mode, int(max_leaf))
        self._refresh_node_count(mode)

    def pose_morphed(self, matrices, weights, rebuild=False, max_leaf=0):
        """prt_pose_morphed / prt_pose_morphed_device: the mesh morphed and then posed by the skin, in one kernel; matrices as pose(), weights
        as morph().  Two numpy arrays (or None) take the host door, two tensors or device addresses the device door; read_posed() returns
        the result"""
        if (isinstance(matrices, np.ndarray) or matrices is None) != (isinstance(weights, np.ndarray) or weights is None):
            raise ValueError("pose_morphed: matrices and weights must both be host arrays or both be on the device")
        mode = self._mode(rebuild)
        self._through("prt_pose_morphed", [(matrices, 12 * self._skin[0] if self._skin else 0), (weights, self._morph[0] if self._morph else 0)],
                      mode, int(max_leaf))
        self._refresh_node_count(mode)

    def read_morphed(self):
        """prt_read_morphed: (vertices, normals) float32 [3T, 4] of the last morph(), accepted or refused; normals None for a set without
        base normals"""
        return self._read_deformed("prt_read_morphed", bool(self._morph and self._morph[1]))

    def read_bvh(self):
        """prt_read_bvh: (nodes [node_count] of _capi.BVH_NODE_DTYPE, primitive_indices uint64 [T]): the current tree in the reference's layout,
        node 0 the root -- the uploaded tree with its current boxes, or the rebuilt one"""
        count = C.c_uint32(0)
        self._chk(self.lib.prt_read_bvh(self.ctx, None, C.byref(count), None), "prt_read_bvh")
        nodes = np.zeros(int(count.value), dtype=np.dtype(_capi.BVH_NODE_DTYPE))
        prims = np.zeros(self.triangle_count, dtype=np.uint64)
        if nodes.size:
            self._chk(self.lib.prt_read_bvh(self.ctx, nodes.ctypes.data_as(C.c_void_p), C.byref(count), prims.ctypes.data_as(C.c_void_p)), "prt_read_bvh")
        return nodes, prims

    def bvh_cost(self):
        """prt_bvh_cost: the SAH cost of the current tree -- uploaded, refitted or rebuilt -- summed on the device in the fixed order of prt.h
        (float; the module's bvh_cost(read_bvh()[0]) up to the order of the sum).  Reads the scene only"""
        cost = C.c_double(0.0)
        self._chk(self.lib.prt_bvh_cost(self.ctx, C.byref(cost)), "prt_bvh_cost")
        return float(cost.value)

    def set_rebuild_policy(self, limit, max_leaf=0):
        """prt_set_rebuild_policy: from now on update_vertices, and pose / morph / pose_morphed with rebuild False, cost the refitted tree and
        rebuild it (max_leaf as rebuild_bvh) once the cost passes limit x the cost of the last built tree (prt.h).  limit None turns it off"""
        if limit is None:
            self._chk(self.lib.prt_set_rebuild_policy(self.ctx, None), "prt_set_rebuild_policy")
            self._policy = False
            return
        policy = _capi.RebuildPolicy(float(limit), int(max_leaf))
        self._chk(self.lib.prt_set_rebuild_policy(self.ctx, C.byref(policy)), "prt_set_rebuild_policy")
        self._policy = True

    def rebuild_report(self):
        """prt_get_rebuild_report: what the last refit-path call under the policy did, as a dict: cost (after its refit), baseline (in force
        now), rebuilt (bool), rebuilds (by the policy, since it was set)"""
        rep = _capi.RebuildReport()
        self._chk(self.lib.prt_get_rebuild_report(self.ctx, C.byref(rep)), "prt_get_rebuild_report")
        return {"cost": float(rep.cost), "baseline": float(rep.baseline), "rebuilt": bool(rep.rebuilt), "rebuilds": int(rep.rebuilds)}

    def _query(self, name, rays, out, words):
        """prt_cast_rays / prt_occluded and their device variants: rays a float32 [n, 8] numpy array (host door) or a tensor on this context's
        device (device door: work queued on torch's current stream is waited for; `out` a float32 tensor of n x words elements, or None for a
        new one)"""
        if hasattr(rays, "data_ptr"):
            import torch
            if rays.dim() != 2 or rays.shape[1] != _capi.RAY_FLOATS:
                raise ValueError("%s: needs a [n, 8] float32 tensor (prt_ray: origin, tmax, dir, pad)" % name)
            n = int(rays.shape[0])
            if out is None:
                out = torch.zeros((n, words) if words > 1 else (n,), dtype=torch.float32, device=rays.device)
            torch.cuda.current_stream(rays.device).synchronize()
            self._chk(getattr(self.lib, name + "_device")(self.ctx, self._device_ptr(rays, n * _capi.RAY_FLOATS, name), n,
                                                          self._device_ptr(out, n * words, name)), name + "_device")
            return out
        r = np.ascontiguousarray(rays, dtype=np.float32)
        if r.ndim != 2 or r.shape[1] != _capi.RAY_FLOATS:
            raise ValueError("%s: needs a float32 array [n, 8] (prt_ray: origin, tmax, dir, pad)" % name)
        host = np.zeros(len(r) * words, dtype=np.uint32)
        self._chk(getattr(self.lib, name)(self.ctx, r.ctypes.data_as(C.c_void_p), len(r), host.ctypes.data_as(C.c_void_p)), name)
        return host

    def cast_rays(self, rays, out=None):
        """prt_cast_rays / prt_cast_rays_device: the closest hit of every ray against the scene as it is now (prt.h "Ray queries").  rays
        float32 [n, 8] = {origin.xyz, tmax, dir.xyz, pad}.  A numpy array returns a structured array of _capi.HIT_DTYPE (t, u, v, tri, normal,
        id, pos, flags); a tensor on this device writes the records (12 words each) into `out` (float32 [n, 12], or a new tensor) and returns it"""
        res = self._query("prt_cast_rays", rays, out, _capi.HIT_FLOATS)
        return res.view(np.dtype(_capi.HIT_DTYPE)) if isinstance(res, np.ndarray) else res

    def occluded(self, rays, out=None):
        """prt_occluded / prt_occluded_device: 1 per ray with something in (eps, tmax), else 0.  numpy in: uint32 [n] out; a tensor in: the
        flags as the words of a float32 [n] tensor (view it as int32)"""
        return self._query("prt_occluded", rays, out, 1)

    def cast_pixels(self, xy):
        """prt_cast_pixels: the hit of the centre ray of every pixel (x, y) of xy (int32 [n, 2], full-frame coordinates, framebuffer order):
        a structured array of _capi.HIT_DTYPE.  Needs a camera and a frame size"""
        p = np.ascontiguousarray(xy, dtype=np.int32).reshape(-1, 2)
        host = np.zeros(len(p), dtype=np.dtype(_capi.HIT_DTYPE))
        self._chk(self.lib.prt_cast_pixels(self.ctx, p.ctypes.data_as(C.c_void_p), len(p), host.ctypes.data_as(C.c_void_p)), "prt_cast_pixels")
        return host

    def set_camera(self, cam):
        self._chk(self.lib.prt_set_camera(self.ctx, C.byref(cam)), "prt_set_camera")

    def upload_envmap(self, rgb):
        rgb = np.ascontiguousarray(rgb, dtype=np.float32)
        self._chk(self.lib.prt_upload_envmap(self.ctx, rgb.ctypes.data_as(C.c_void_p), rgb.shape[1], rgb.shape[0]),
                  "prt_upload_envmap")

    def resize(self, width, height):
        self._chk(self.lib.prt_resize(self.ctx, width, height), "prt_resize")
        self.width, self.height, self.rows = width, height, height

    def set_tile(self, width, full_height, row0, rows):
        self._chk(self.lib.prt_set_tile(self.ctx, width, full_height, row0, rows), "prt_set_tile")
        self.width, self.height, self.rows = width, full_height, rows

    def set_row_blocks(self, width, full_height, block_rows, n_parts, part):
        self._chk(self.lib.prt_set_row_blocks(self.ctx, width, full_height, block_rows, n_parts, part), "prt_set_row_blocks")
        rows = sum(1 for r in range(full_height) if (r // block_rows) % n_parts == part)
        self.width, self.height, self.rows = width, full_height, rows

    def reset(self):
        self._chk(self.lib.prt_reset(self.ctx), "prt_reset")

    def render_frames(self, seeds, first_frame=1):
        seeds = np.ascontiguousarray(seeds, dtype=np.int32)
        self._chk(self.lib.prt_render_frames(self.ctx, first_frame, len(seeds) // 2, seeds.ctypes.data_as(C.c_void_p)),
                  "prt_render_frames")

    def render_spp(self, spp, seeds):
        seeds = np.ascontiguousarray(seeds, dtype=np.int32)
        used = C.c_uint32(0)
        self._chk(self.lib.prt_render_spp(self.ctx, spp, len(seeds) // 2, seeds.ctypes.data_as(C.c_void_p), C.byref(used)),
                  "prt_render_spp")
        return used.value

    def render_adaptive(self, seeds, min_spp, max_spp, rel_err, abs_floor=0.0):
        """prt_render_adaptive: every pixel renders paths until its mean luminance is judged converged (at least min_spp, at most max_spp
        paths; prt.h).  Returns the frames used."""
        seeds = np.ascontiguousarray(seeds, dtype=np.int32)
        a = Adaptive(int(min_spp), int(max_spp), float(rel_err), float(abs_floor))
        used = C.c_uint32(0)
        self._chk(self.lib.prt_render_adaptive(self.ctx, C.byref(a), len(seeds) // 2, seeds.ctypes.data_as(C.c_void_p), C.byref(used)),
                  "prt_render_adaptive")
        return used.value

    def read_adaptive_stats(self):
        """the adaptive plane: float32 [rows * width, 2] = {l, s2} per pixel, framebuffer order"""
        return self._read("prt_read_adaptive_stats", (self.rows * self.width, 2), np.float32)

    def adaptive_report(self):
        rep = AdaptiveReport()
        self._chk(self.lib.prt_get_adaptive_report(self.ctx, C.byref(rep)), "prt_get_adaptive_report")
        return rep

    def render_guides(self, samples=4):
        """prt_render_guides: `samples` guide samples per pixel (1 .. 64; prt.h has the sample positions and the delta chain)"""
        self._chk(self.lib.prt_render_guides(self.ctx, int(samples)), "prt_render_guides")

    def read_guides(self):
        """the guide plane: float32 [rows, width, 8] = {albedo.rgb, coverage, normal.xyz, depth} per pixel, framebuffer order"""
        return self._read("prt_read_guides", (self.rows, self.width, 8), np.float32)

    def set_motion(self, enable=True):
        """prt_set_motion: the guide renders also write the motion plane of the deforming mesh (update_vertices) and denoise_temporal
        reprojects through it (prt.h).  Off by default; makes the guides stale, keeps the histories"""
        self._chk(self.lib.prt_set_motion(self.ctx, 1 if enable else 0), "prt_set_motion")

    def read_motion(self):
        """the motion plane of the last render_guides: float32 [rows, width, 4] = {D.xyz, m} per pixel, framebuffer order (prt.h)"""
        return self._read("prt_read_motion", (self.rows, self.width, 4), np.float32)

    def export_motion(self, ptr_or_tensor):
        """prt_export_motion: the motion plane of this context's frame part into device memory: a [rows, width, 4] float32 tensor on this
        device (more rows are left alone) or a device address"""
        p = self._device_ptr(ptr_or_tensor, self.rows * self.width * _capi.MOTION_FLOATS, "export_motion")
        self._chk(self.lib.prt_export_motion(self.ctx, p), "prt_export_motion")

    _VAR_SOURCES = {"auto": _capi.PRT_DENOISE_VAR_AUTO, "stats": _capi.PRT_DENOISE_VAR_STATS, "spatial": _capi.PRT_DENOISE_VAR_SPATIAL}

    def denoise(self, passes=DENOISE_DEFAULTS["passes"], var_source="auto", sigma_l=DENOISE_DEFAULTS["sigma_l"],
                sigma_n=DENOISE_DEFAULTS["sigma_n"], sigma_z=DENOISE_DEFAULTS["sigma_z"], sigma_a=DENOISE_DEFAULTS["sigma_a"], tonemap=False):
        """prt_denoise: the a-trous filter of prt.h over the framebuffer, guided by the guides.  var_source: "auto" | "stats" | "spatial".
        Returns float32 [rows, width, 4] (prt_read_framebuffer's layout), or with tonemap=True uint8 [rows, width, 4] (prt_tonemap_rgba8's)"""
        p = DenoiseParams(int(passes), self._VAR_SOURCES[var_source], float(sigma_l), float(sigma_n), float(sigma_z), float(sigma_a))
        if tonemap:
            out = np.zeros((self.rows, self.width, 4), dtype=np.uint8)
            self._chk(self.lib.prt_denoise(self.ctx, C.byref(p), None, out.ctypes.data_as(C.c_void_p)), "prt_denoise")
        else:
            out = np.zeros((self.rows, self.width, 4), dtype=np.float32)
            self._chk(self.lib.prt_denoise(self.ctx, C.byref(p), out.ctypes.data_as(C.c_void_p), None), "prt_denoise")
        return out

    _FEEDBACK = {"integrated": _capi.PRT_TEMPORAL_FEEDBACK_INTEGRATED, "atrous": _capi.PRT_TEMPORAL_FEEDBACK_ATROUS}

    def denoise_temporal(self, passes=DENOISE_DEFAULTS["passes"], var_source="auto", sigma_l=DENOISE_DEFAULTS["sigma_l"],
                         sigma_n=DENOISE_DEFAULTS["sigma_n"], sigma_z=DENOISE_DEFAULTS["sigma_z"], sigma_a=DENOISE_DEFAULTS["sigma_a"],
                         alpha_color=TEMPORAL_DEFAULTS["alpha_color"], alpha_moments=TEMPORAL_DEFAULTS["alpha_moments"],
                         tau_z=TEMPORAL_DEFAULTS["tau_z"], cos_n=TEMPORAL_DEFAULTS["cos_n"], history_cap=TEMPORAL_DEFAULTS["history_cap"],
                         feedback=TEMPORAL_DEFAULTS["feedback"], tonemap=False):
        """prt_denoise_temporal: the history reprojected into this camera and blended with the framebuffer, then denoise()'s filter (prt.h).
        Takes denoise()'s keywords plus the temporal ones; feedback: "atrous" (pass 0's output becomes the history) | "integrated".
        With set_temporal_response() on, the blended colour is clamped to the fast history's neighbourhood in front of the filter.
        Returns what denoise() returns"""
        p = DenoiseParams(int(passes), self._VAR_SOURCES[var_source], float(sigma_l), float(sigma_n), float(sigma_z), float(sigma_a))
        t = TemporalParams(float(alpha_color), float(alpha_moments), float(tau_z), float(cos_n), int(history_cap), self._FEEDBACK[feedback])
        out = np.zeros((self.rows, self.width, 4), dtype=np.uint8 if tonemap else np.float32)
        ptr = out.ctypes.data_as(C.c_void_p)
        self._chk(self.lib.prt_denoise_temporal(self.ctx, C.byref(p), C.byref(t), None if tonemap else ptr, ptr if tonemap else None),
                  "prt_denoise_temporal")
        return out

    def read_history(self):
        """the temporal history: float32 [rows, width, 8] = {c.rgb, n, m1, m2, v, 0} per pixel, framebuffer order"""
        return self._read("prt_read_history", (self.rows, self.width, 8), np.float32)

    def reset_history(self):
        self._chk(self.lib.prt_reset_history(self.ctx), "prt_reset_history")

    def set_temporal_response(self, fast_cap=_capi.RESPONSE_DEFAULTS["fast_cap"], radius=_capi.RESPONSE_DEFAULTS["radius"],
                              k=_capi.RESPONSE_DEFAULTS["k"]):
        """prt_set_temporal_response: a fast history of fast_cap frames beside both histories of this context, and the clamp of the blended
        colour to mean +- k sigma of its (2 radius + 1)^2 neighbourhood (prt.h).  set_temporal_response(None) turns it off.  A change of
        the setting empties both histories"""
        if fast_cap is None:
            self._chk(self.lib.prt_set_temporal_response(self.ctx, None), "prt_set_temporal_response")
            return
        r = TemporalResponse(int(fast_cap), int(radius), float(k), 0)
        self._chk(self.lib.prt_set_temporal_response(self.ctx, C.byref(r)), "prt_set_temporal_response")

    def read_response(self):
        """the temporal response of the frame history: float32 [rows, width, 4] = {f.rgb, flag} per pixel, framebuffer order; flag 0 no
        history, 1 history kept, 2 clamped"""
        return self._read("prt_read_response", (self.rows, self.width, 4), np.float32)

    @staticmethod
    def _device_ptr(t, floats, what):
        """the device address of `t`: an integer, or a tensor (anything with data_ptr(): it must be contiguous float32 of at least `floats`
        elements -- the library writes or reads that many without seeing the tensor)"""
        if not hasattr(t, "data_ptr"):
            return C.c_void_p(int(t))
        if not t.is_contiguous() or t.element_size() != 4 or not t.is_floating_point() or t.numel() < floats:
            raise ValueError("%s: needs a contiguous float32 tensor of at least %d elements" % (what, floats))
        return C.c_void_p(t.data_ptr())

    def export_denoise_inputs(self, ptr_or_tensor):
        """prt_export_denoise_inputs: the denoiser's inputs of this context's frame part as records (16 floats per pixel, prt.h) into device
        memory: a [rows, width, 16] float32 tensor on this device (more rows are left alone) or a device address"""
        p = self._device_ptr(ptr_or_tensor, self.rows * self.width * _capi.DENOISE_RECORD_FLOATS, "export_denoise_inputs")
        self._chk(self.lib.prt_export_denoise_inputs(self.ctx, p), "prt_export_denoise_inputs")

    def _records_call(self, name, head, records, width, height, tonemap, out, extra=()):
        width, height = int(width), int(height)
        rec = (self._device_ptr(records, width * height * _capi.DENOISE_RECORD_FLOATS, name),) + tuple(extra)
        fn = getattr(self.lib, name)
        if out is not None:
            self._chk(fn(self.ctx, *head, width, height, *rec, self._device_ptr(out, width * height * 4, name), None, None), name)
            return out
        host = np.zeros((max(height, 0), max(width, 0), 4), dtype=np.uint8 if tonemap else np.float32)   # a size below 1 is the library's to refuse
        ptr = host.ctypes.data_as(C.c_void_p)
        self._chk(fn(self.ctx, *head, width, height, *rec, None, None if tonemap else ptr, ptr if tonemap else None), name)
        return host

    def denoise_records(self, records, width, height, passes=DENOISE_DEFAULTS["passes"], var_source="auto", sigma_l=DENOISE_DEFAULTS["sigma_l"],
                        sigma_n=DENOISE_DEFAULTS["sigma_n"], sigma_z=DENOISE_DEFAULTS["sigma_z"], sigma_a=DENOISE_DEFAULTS["sigma_a"],
                        tonemap=False, out=None):
        """prt_denoise_records: denoise()'s filter over a width x height frame given as records in device memory (a [height, width, 16] float32
        tensor on this device, or a device address): the gathered export_denoise_inputs() of every part of the frame.  The context needs no
        scene or frame of its own.  Returns what denoise() returns; with `out` (a [height, width, 4] float32 tensor on this device, or a device
        address) the picture stays on the device: it is written there and `out` is returned"""
        p = DenoiseParams(int(passes), self._VAR_SOURCES[var_source], float(sigma_l), float(sigma_n), float(sigma_z), float(sigma_a))
        return self._records_call("prt_denoise_records", (C.byref(p),), records, width, height, tonemap, out)

    def denoise_records_temporal(self, records, width, height, cam, passes=DENOISE_DEFAULTS["passes"], var_source="auto",
                                 sigma_l=DENOISE_DEFAULTS["sigma_l"], sigma_n=DENOISE_DEFAULTS["sigma_n"], sigma_z=DENOISE_DEFAULTS["sigma_z"],
                                 sigma_a=DENOISE_DEFAULTS["sigma_a"], alpha_color=TEMPORAL_DEFAULTS["alpha_color"],
                                 alpha_moments=TEMPORAL_DEFAULTS["alpha_moments"], tau_z=TEMPORAL_DEFAULTS["tau_z"], cos_n=TEMPORAL_DEFAULTS["cos_n"],
                                 history_cap=TEMPORAL_DEFAULTS["history_cap"], feedback=TEMPORAL_DEFAULTS["feedback"], tonemap=False, out=None,
                                 motion=None):
        """prt_denoise_records_temporal: denoise_records() with denoise_temporal()'s step in front.  `cam`: the camera the records were rendered
        with.  The record history is this context's second one (reset_records_history(); a call with another size empties it too).
        set_temporal_response() applies to it as to denoise_temporal()'s.
        motion: None, or the frame's motion plane (a [height, width, 4] float32 tensor on this device or a device address: the gathered
        export_motion() of every part) -- prt_denoise_records_temporal_motion"""
        p = DenoiseParams(int(passes), self._VAR_SOURCES[var_source], float(sigma_l), float(sigma_n), float(sigma_z), float(sigma_a))
        t = TemporalParams(float(alpha_color), float(alpha_moments), float(tau_z), float(cos_n), int(history_cap), self._FEEDBACK[feedback])
        head = (C.byref(p), C.byref(t), C.byref(cam) if cam is not None else None)
        if motion is None:
            return self._records_call("prt_denoise_records_temporal", head, records, width, height, tonemap, out)
        mp = self._device_ptr(motion, int(width) * int(height) * _capi.MOTION_FLOATS, "prt_denoise_records_temporal_motion")
        return self._records_call("prt_denoise_records_temporal_motion", head, records, width, height, tonemap, out, extra=(mp,))

    def reset_records_history(self):
        self._chk(self.lib.prt_reset_records_history(self.ctx), "prt_reset_records_history")

    def read_records_history(self, width, height):
        """the record history of denoise_records_temporal()'s width x height frame: float32 [height, width, 8] = {c.rgb, n, m1, m2, v, 0} per
        pixel, framebuffer order (read_history()'s twin)"""
        width, height = int(width), int(height)                # (a size below 1 is the library's to refuse)
        return self._read("prt_read_records_history", (max(height, 0), max(width, 0), 8), np.float32, width, height)

    def read_records_response(self, width, height):
        """read_response()'s twin for the record history: float32 [height, width, 4] = {f.rgb, flag} per pixel"""
        width, height = int(width), int(height)
        return self._read("prt_read_records_response", (max(height, 0), max(width, 0), 4), np.float32, width, height)

    def set_pixel_filter(self, kind="tent", radius=None):
        """prt_set_pixel_filter: antialiasing by filter importance sampling (prt.h).  kind: a name of PIXEL_FILTERS ("none", "box", "tent",
        "gaussian", "blackman-harris") or its number; radius None = the kind's default.  Resets the frame and makes the guides stale"""
        r = -1.0 if radius is None else float(radius)
        self._chk(self.lib.prt_set_pixel_filter(self.ctx, _filter_kind(kind), C.c_float(r)), "prt_set_pixel_filter")

    def set_walk_min_lanes(self, lanes):
        self._chk(self.lib.prt_set_walk_min_lanes(self.ctx, int(lanes)), "prt_set_walk_min_lanes")

    def set_option(self, name, value):
        self._chk(self.lib.prt_set_option(self.ctx, name.encode(), int(value)), "prt_set_option")

    def kernel_variant(self):
        return self.lib.prt_kernel_variant(self.ctx).decode()

    def synchronize(self):
        self._chk(self.lib.prt_synchronize(self.ctx), "prt_synchronize")

    def read_framebuffer(self):
        return self._read("prt_read_framebuffer", (self.rows, self.width, 4), np.float32)

    def tonemap_rgba8(self):
        """the reference's display transform (shaders/tonemapper.glsl) of the framebuffer, rows bottom-up"""
        return self._read("prt_tonemap_rgba8", (self.rows, self.width, 4), np.uint8)

    def copy_framebuffer_to_device(self, device_ptr):
        self._chk(self.lib.prt_copy_framebuffer_to_device(self.ctx, C.c_void_p(device_ptr)), "prt_copy_framebuffer_to_device")

    def read_state(self):
        return self._read("prt_read_state", self.rows * self.width, np.dtype(PATH_STATE_DTYPE))

    def write_state(self, state):
        state = np.ascontiguousarray(state)
        assert state.dtype.itemsize == 112 and state.size == self.rows * self.width
        self._chk(self.lib.prt_write_state(self.ctx, state.ctypes.data_as(C.c_void_p)), "prt_write_state")

    def set_stream(self, hip_stream_ptr):
        self._chk(self.lib.prt_set_stream(self.ctx, C.c_void_p(hip_stream_ptr)), "prt_set_stream")

    def stats(self):
        st = Stats()
        self._chk(self.lib.prt_get_stats(self.ctx, C.byref(st)), "prt_get_stats")
        return st

    def counts(self, spp=0):
        st = Stats()
        self._chk(self.lib.prt_query_counts(self.ctx, spp, C.byref(st)), "prt_query_counts")
        return st

    def selftest_math(self, fn, a, b):
        a = np.ascontiguousarray(a, dtype=np.float32)
        b = np.ascontiguousarray(b, dtype=np.float32)
        out = np.zeros_like(a)
        self._chk(self.lib.prt_selftest_math(self.ctx, fn, a.ctypes.data_as(C.c_void_p), b.ctypes.data_as(C.c_void_p),
                                             out.ctypes.data_as(C.c_void_p), a.size), "prt_selftest_math")
        return out

    def selftest_fn(self, fn, params, cases):
        """prt_selftest_fn: params = 80 floats, cases = [n, 32] float32 -> [n, 32] float32 (fn 13 / 14 work on the uploaded map; params unused)"""
        params = np.ascontiguousarray(params, dtype=np.float32)
        cases = np.ascontiguousarray(cases, dtype=np.float32)
        assert params.size == 80 and cases.ndim == 2 and cases.shape[1] == 32
        out = np.zeros_like(cases)
        self._chk(self.lib.prt_selftest_fn(self.ctx, int(fn), params.ctypes.data_as(C.c_void_p), cases.ctypes.data_as(C.c_void_p),
                                           out.ctypes.data_as(C.c_void_p), cases.shape[0]), "prt_selftest_fn")
        return out

    def close(self):
        if getattr(self, "ctx", None) and self.ctx.value:
            self.lib.prt_destroy(self.ctx)
            self.ctx = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
