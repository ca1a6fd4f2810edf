"""Code-generation guard (no GPU) for the addressing of the per-lane tables, modelled on test_codegen.py.  It compiles the one-variant listing
of the headline kernel (tools/isa.sh: pt_kernels.hip with -DPT_UNITY -DPT_DEV_ONE_VARIANT, render_kernel<LIGHT|DIFF, no medium, 6 waves>)
and reads its frame loop -- the longest backward-branch span of the kernel:

  * every per-lane load of the frame loop (node pairs, triangle records, vertex normals, materials, a primitive by the lane's own mesh
    index, environment texels) takes {scalar base pair, one 32-bit vector offset}: `global_load_* v[..], vOff, s[b:b+1]`, never the
    64-bit `v[a:a+1], off` form;
  * the 64-bit address arithmetic that form needed (v_mad_u64_u32, v_mad_i64_i32, v_lshl_add_u64) is gone from the frame loop.

What the parent commit's listing gave for the same counts (the same parser, the same flags): 31 global loads in the frame loop, all 31 in the
`off` form; 18 v_mad_u64_u32 + 2 v_mad_i64_i32 + 3 v_lshl_add_u64.  (The issue's own count is of the whole kernel, path start and end
included: 37 loads, 22 + 3 multiply-adds.)  This tree: 31 loads, all with a scalar base; no 64-bit multiply-add or shift-add.

The root step is not guarded here.  The parent's frame loop holds 34 `v_mov_b32 v, s` that a v_cndmask reads, 24 of them in the two root
steps of walk_begin (12 each: one per plane of the root pair).  The arm that took the planes as the fma's scalar operand and selected
afterwards brought the 34 down to 10 -- and was dropped: alone it measured +0.3 % with 0.04 % between its slowest and the parent's fastest
run, and together with the 32-bit offsets it was slower than the offsets alone in every round (DESIGN.md s4,
profiles/r16_addressing_ab.txt).  This tree holds the parent's 34."""
import os
import re
import subprocess

import pytest

from conftest import ROOT
from cases import frame_loop, HIP, HIPCC, kernel_lines


def addressing_counts(text):
    loop = frame_loop(kernel_lines(text))
    loads = [l for l in loop if re.match(r"\s+global_load", l)]
    return {
        "loads": len(loads),
        "loads_scalar_base": sum(1 for l in loads if re.match(r"\s+global_load_\w+\s+v(\d+|\[\d+:\d+\]),\s*v\d+,\s*s\[\d+:\d+\]", l)),
        "loads_vgpr_pair": sum(1 for l in loads if re.search(r"v\[\d+:\d+\],\s*off\b", l)),
        "mad64": sum(1 for l in loop if re.match(r"\s+v_mad_(u64_u32|i64_i32)\b", l)),
        "lshl_add64": sum(1 for l in loop if re.match(r"\s+v_lshl_add_u64\b", l)),
    }


@pytest.fixture(scope="module")
def listing(tmp_path_factory):
    out = tmp_path_factory.mktemp("isa") / "pt_kernels.s"
    cmd = [HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=off", "-fno-fast-math", "-fno-slp-vectorize", "-DPT_UNITY", "-S",
           "--cuda-device-only", "-DPT_DEV_ONE_VARIANT", "-I" + os.path.join(ROOT, "include"), "-I" + HIP, "-o", str(out), os.path.join(HIP, "pt_kernels.hip")]
    subprocess.run(cmd, check=True, capture_output=True, timeout=1800)
    return addressing_counts(out.read_text())


needs_hipcc = pytest.mark.skipif(not os.path.exists(HIPCC), reason="no hipcc")


@needs_hipcc
def test_frame_loop_loads_take_a_scalar_base(listing):
    assert listing["loads"] >= 20, listing                      # (the parser found the frame loop and its loads)
    assert listing["loads_vgpr_pair"] == 0 and listing["loads_scalar_base"] == listing["loads"], listing


@needs_hipcc
def test_frame_loop_has_no_64_bit_address_arithmetic(listing):
    assert listing["mad64"] == 0 and listing["lshl_add64"] == 0, listing
