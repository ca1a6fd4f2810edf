"""The render kernels read the node pairs, the triangle records, the vertex normals and the materials at {table base, 32-bit byte offset}
(csrc/hip/pt_layout.h pair_offset / rec48_offset / table_limit_error; pt_device.h table_at / const_table_at; include/prt.h PRT_MAX_*).

CPU: tests/offsets32_check.cpp, a stand-alone host program over the shared headers, checks the offset expressions against the 64-bit
address they replace (first record, last record at the limit, slot * 48 at 2^32 / 48 - 1, with a base whose low word is nearly full) and the
size rule -- a pure function of the counts, so no table is allocated: the last accepted count of slots, pairs and materials is accepted, the
next one is refused, and the refusal names the limit.

GPU: what can go wrong is an offset at the far end of a table, not the frame size.  A 40-triangle mesh under a caller's tree of three
pairs with loose boxes (every ray visits every pair, the last one included) whose LAST slot is a triangle that fills the view; a triangle
hit shades with the OBJ material, which is the last record of the material table.  Frames 8 x 8 and 9 x 7, 4 spp, state and framebuffer bit
for bit against the CPU oracle, through the compiled material set and the generic one, and again after prt_rebuild_bvh_device."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from conftest import ROOT
from mirrors import NODE_T
from support import assert_same_render

HIP = os.path.join(ROOT, "photorealistic-rendering-using-opencl_amd", "csrc", "hip")
HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
f32 = np.float32

MAX_SLOTS = (2 ** 32 - 1) // 48          # 89 478 485 records of 48 bytes stay below 4 GiB
MAX_PAIRS = (2 ** 32 - 1) // 64          # 2^26 - 1 records of 64 bytes
MAX_MATS = (2 ** 32 - 1) // 48


# ---- CPU: the stand-alone program ------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def check_output(tmp_path_factory):
    exe = tmp_path_factory.mktemp("offsets32") / "offsets32_check"
    cmd = [HIPCC, "-std=c++17", "-O2", "-ffp-contract=off", "-fno-fast-math", "-DPT_EMU", "-x", "hip", "--cuda-host-only", "-Wno-unused-command-line-argument",
           "-I" + os.path.join(ROOT, "include"), "-I" + HIP, "-o", str(exe), os.path.join(ROOT, "tests", "offsets32_check.cpp")]
    subprocess.run(cmd, check=True, capture_output=True, timeout=600)
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=60)
    return r.returncode, r.stdout.split("\n")


needs_hipcc = pytest.mark.skipif(not os.path.exists(HIPCC), reason="no hipcc")


@needs_hipcc
def test_offsets_equal_the_64_bit_addresses_they_replace(check_output):
    rc, lines = check_output
    bad = [l for l in lines if l.startswith("FAIL")]
    assert rc == 0 and not bad and "all ok" in lines, bad
    ok = [l for l in lines if l.startswith("ok ")]
    for want in ("pairs[0] table_at", "pairs[%d] table_at" % (MAX_PAIRS - 1), "tri_geom[0] table_at", "tri_geom[%d] const_table_at" % (2 ** 32 // 48 - 1),
                 "tri_nrm[%d] table_at" % (MAX_SLOTS - 1), "mats[0] const_table_at", "mats[%d] const_table_at" % (MAX_MATS - 1), "slot * 48 at 2^32 / 48 - 1"):
        assert any(want in l for l in ok), want


@needs_hipcc
def test_size_rule_accepts_the_last_count_and_refuses_the_next(check_output):
    rc, lines = check_output
    limits = {}
    for l in lines:
        m = re.match(r"limit (\w+) (\d+) (.*)", l)
        if m:
            limits[m.group(1)] = (int(m.group(2)), m.group(3))
    assert {k: v[0] for k, v in limits.items()} == {"slots": MAX_SLOTS, "pairs": MAX_PAIRS, "materials": MAX_MATS}
    for table, last in (("slots", MAX_SLOTS), ("pairs", MAX_PAIRS), ("materials", MAX_MATS)):
        assert any(l == "ok %s: %d accepted" % (table, last) for l in lines), table
        assert any(l == "ok %s: %d refused" % (table, last + 1) for l in lines), table
        assert str(last) in limits[table][1], "the refusal does not name the limit: " + limits[table][1]
    assert "PRT_MAX_TRIANGLE_SLOTS" in limits["slots"][1] and "PRT_MAX_NODE_PAIRS" in limits["pairs"][1] and "PRT_MAX_MATERIALS" in limits["materials"][1]


def test_prt_h_states_the_limits():
    text = open(os.path.join(ROOT, "include", "prt.h")).read()
    for name, value in (("PRT_MAX_TRIANGLE_SLOTS", MAX_SLOTS), ("PRT_MAX_NODE_PAIRS", MAX_PAIRS), ("PRT_MAX_MATERIALS", MAX_MATS)):
        assert re.search(r"#define %s %du\b" % (name, value), text), name


# ---- GPU: the far end of every table -----------------------------------------------------------------------------------------------------------

T = 40
SPP = 4


class FarEnd:
    """cornell_diffuse's primitives with a mesh of its first T - 1 triangles plus one that fills the view, under a three-pair tree whose last
    leaf ends with that triangle (= the last slot): root -> {leaf 0..9, inner -> {leaf 10..19, inner -> {leaf 20..29, leaf 30..39}}}"""

    def __init__(self, prt):
        self.prt = prt
        self.scene = prt.HostScene("cornell_diffuse.json")
        self.cfg = self.scene.config()
        a = prt.scene_arrays(self.scene.desc)
        self.v = np.ascontiguousarray(a["vertices"][:3 * T], dtype=f32).copy()
        self.n = np.ascontiguousarray(a["normals"][:3 * T], dtype=f32).copy()
        cam = prt.default_camera(8, 8)
        pos, view, up = (np.array(list(x)[:3], dtype=np.float64) for x in (cam.position, cam.view, cam.up))
        right = np.cross(view, up)
        right /= np.linalg.norm(right)
        upv = np.cross(right, view)
        centre = pos + view * 1.5
        self.v[3 * (T - 1):, :3] = np.array([centre - 4 * right - 3 * upv, centre + 4 * right - 3 * upv, centre + 5 * upv], dtype=f32)
        self.n[3 * (T - 1):, :3] = (-view).astype(f32)
        self.pi = np.arange(T, dtype=np.uint64)
        nodes = np.zeros(7, dtype=NODE_T)
        nodes["bounds"] = np.array([-8, 8, -8, 8, -8, 8], dtype=f32)           # loose: every ray visits every pair
        nodes[0]["first"] = 1
        nodes[1]["first"], nodes[1]["count"], nodes[1]["leaf"] = 0, 10, 1
        nodes[2]["first"] = 3
        nodes[3]["first"], nodes[3]["count"], nodes[3]["leaf"] = 10, 10, 1
        nodes[4]["first"] = 5
        nodes[5]["first"], nodes[5]["count"], nodes[5]["leaf"] = 20, 10, 1
        nodes[6]["first"], nodes[6]["count"], nodes[6]["leaf"] = 30, 10, 1
        self.nodes = nodes
        self.desc = self.make_desc(self.nodes, self.pi)

    def make_desc(self, nodes, pi):
        d = self.prt.SceneDesc.from_buffer_copy(bytes(self.scene.desc))
        d.vertices = self.v.ctypes.data_as(C.c_void_p)
        d.normals = self.n.ctypes.data_as(C.c_void_p)
        d.primitive_indices = pi.ctypes.data_as(C.c_void_p)
        d.triangle_count = T
        d.bvh_nodes = nodes.ctypes.data_as(C.c_void_p)
        d.bvh_node_count = len(nodes)
        return d


@pytest.fixture(scope="module")
def far_end(prt):
    return FarEnd(prt)


_oracle_cache = {}


def _oracle(oracle, case, desc, key, W, H):
    """the oracle's render (computed once per key, shared, never written to)"""
    if key not in _oracle_cache:
        st, img = oracle.Restatement().render(case.cfg, desc, case.prt.default_camera(W, H), W, H, case.prt.seed_pairs(SPP), threads=4)
        st.setflags(write=False)
        img.setflags(write=False)
        _oracle_cache[key] = (st, img)
    return _oracle_cache[key]


def _same(oracle, want, state, img, what):
    assert_same_render(oracle, want[0], want[1], state, img, what)


def _render(r, prt):
    r.reset()
    r.render_frames(prt.seed_pairs(SPP))
    return r.read_state(), r.read_framebuffer()


def test_the_packed_far_end_is_where_the_test_says(prt, far_end):
    """pack_scene of the case (host only): three pairs, 40 slots, the view-filling triangle in the last slot, and the OBJ material last"""
    import refit_api
    p = refit_api.Packed(far_end.cfg, far_end.desc)
    got = p.get()
    assert (p.n_pairs, p.n_slots) == (3, T)
    assert got["slot_vtx"][-1] == 3 * (T - 1), "the last slot is not the view-filling triangle"
    assert got["pairs"]["meta"][2].tolist() == [20, 10, 30, 10], "the last pair does not hold the last two leaves"
    assert np.array_equal(got["tri_geom"][-1].view(f32)[:3], far_end.v[3 * (T - 1), :3])
    p.close()


@pytest.mark.gpu
@pytest.mark.parametrize("generic", [0, 1], ids=["compiled", "generic"])
@pytest.mark.parametrize("W,H", [(8, 8), (9, 7)])
def test_last_slot_last_pair_last_material_match_the_oracle(prt, oracle, far_end, W, H, generic):
    want = _oracle(oracle, far_end, far_end.desc, ("tree", W, H), W, H)
    # the view-filling triangle is what the primary rays hit: without it the picture is another one
    r = prt.Renderer(far_end.cfg, device=0)
    r.set_option("generic", generic)
    r.upload_scene(far_end.desc)
    r.set_camera(prt.default_camera(W, H))
    r.resize(W, H)
    state, img = _render(r, prt)
    assert ("generic" in r.kernel_variant()) == bool(generic), r.kernel_variant()
    _same(oracle, want, state, img, "three-pair tree %dx%d generic=%d" % (W, H, generic))
    # the same scene under the tree the device builds
    import torch
    r.rebuild_bvh(torch.from_numpy(far_end.v).cuda(), torch.from_numpy(far_end.n).cuda(), 2)
    nodes, prims = r.read_bvh()
    nodes, prims = np.ascontiguousarray(nodes), np.ascontiguousarray(prims, dtype=np.uint64)
    state, img = _render(r, prt)
    r.close()
    want2 = _oracle(oracle, far_end, far_end.make_desc(nodes, prims), ("rebuilt", W, H), W, H)
    _same(oracle, want2, state, img, "rebuilt tree %dx%d generic=%d" % (W, H, generic))


def test_the_view_filling_triangle_is_hit(prt, oracle, far_end):
    """the oracle's picture changes when the last slot's triangle is moved out of view: the far end of the tables is on the rays' way"""
    want = _oracle(oracle, far_end, far_end.desc, ("tree", 8, 8), 8, 8)
    v = far_end.v.copy()
    v[3 * (T - 1):, 1] += 30.0
    d = far_end.make_desc(far_end.nodes, far_end.pi)
    d.vertices = v.ctypes.data_as(C.c_void_p)
    st, img = oracle.Restatement().render(far_end.cfg, d, prt.default_camera(8, 8), 8, 8, prt.seed_pairs(SPP), threads=4)
    assert not oracle.images_equal(want[1], img)
