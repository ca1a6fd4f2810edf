"""Code-generation guard (no GPU): the exact fast paths of csrc/hip/pt_device.h -- hw_recip, hw_sqrt, out_of_unit_range -- choose their
IEEE expression by a WAVE vote.  A lane-wise choice compiles to a two-sided exec-masked region (saveexec / xor / exec branch / the IEEE
expansion / andn2 saveexec / fast path / or exec) at every one of their sites in the frame loop; the vote to one scalar conditional
branch to an IEEE block that lies out of the way, with nothing masked.  Bit-exact either way, so no parity test sees the difference:
this compiles tests/probes/coldpath_probe.hip (load, helper, store) to a listing and looks at the shape.  The pair helper of sine and
cosine has no branch at all and one evaluation of the kernel."""
import os
import re
import shutil
import subprocess

import pytest

from conftest import ROOT

HIP = os.path.join(ROOT, "photorealistic-rendering-using-opencl_amd", "csrc", "hip")
HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"


@pytest.fixture(scope="module")
def kernels(tmp_path_factory):
    """kernel name -> its instructions (mnemonic and operands), from the listing of the probe built with the product's flags"""
    out = tmp_path_factory.mktemp("coldpaths") / "coldpath_probe.s"
    cmd = [HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=off", "-fno-fast-math", "-fno-slp-vectorize", "-S",
           "--cuda-device-only", "-I" + os.path.join(ROOT, "include"), "-I" + HIP, "-o", str(out), os.path.join(ROOT, "tests", "probes", "coldpath_probe.hip")]
    subprocess.run(cmd, check=True, capture_output=True, timeout=600)
    found, cur = {}, None
    for line in out.read_text().split("\n"):
        m = re.match(r"^(probe_\w+):", line)
        if m:
            cur = m.group(1)
            found[cur] = []
        elif line.startswith(".Lfunc_end"):
            cur = None
        elif cur and re.match(r"\.LBB\w+:", line):
            found[cur].append(line.split(":")[0] + ":")                  # a block label
        elif cur and re.match(r"\s+[a-z]\w*", line):
            found[cur].append(line.split(";")[0].strip())
    return found


def _count(insts, pattern):
    return sum(1 for i in insts if re.match(pattern, i))


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="no hipcc")
@pytest.mark.parametrize("kernel, ieee", [("probe_recip", r"v_div_fixup_f32"), ("probe_sqrt", r"v_sqrt_f32"), ("probe_unit_range", r"v_div_fixup_f32")])
def test_slow_path_is_one_scalar_branch_with_nothing_masked(kernels, kernel, ieee):
    insts = kernels[kernel]
    assert _count(insts, r"s_\w+_saveexec") == 0, [i for i in insts if "saveexec" in i]
    assert _count(insts, r"s_cbranch_exec") == 0, [i for i in insts if i.startswith("s_cbranch")]
    assert _count(insts, r"s_cbranch_(vcc|scc)") == 1, [i for i in insts if i.startswith("s_cbranch")]
    # the branch leads to the IEEE expression, of which there is one copy, in a block that lies behind the branch (out of the fast path's way)
    assert _count(insts, ieee) == 1, insts
    branch = next(k for k, i in enumerate(insts) if re.match(r"s_cbranch_(vcc|scc)", i))
    target = insts.index(insts[branch].split()[-1] + ":")
    slow = next(k for k, i in enumerate(insts) if re.match(ieee, i))
    later_labels = [k for k, i in enumerate(insts) if i.endswith(":") and k > target]
    assert branch < target < slow and all(slow < k for k in later_labels), (branch, target, slow, insts)


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="no hipcc")
def test_sine_and_cosine_of_one_argument_share_one_evaluation(kernels):
    """prt_sincos_kernel once: one reduction (three fma steps after one multiply by 2 / pi), the two polynomials, and selects -- no branch.
    Two calls (prt_sin, prt_cos) are twice the fma count and a guard branch each"""
    insts = kernels["probe_sincos"]
    assert _count(insts, r"s_cbranch") == 0 and _count(insts, r"s_\w+_saveexec") == 0, [i for i in insts if i.startswith("s_")]
    fmas = _count(insts, r"v_fma\w*_f32")                 # v_fma / v_fmac / v_fmaak / v_fmamk
    assert 12 <= fmas <= 16, (fmas, insts)                # 3 reduction + 5 + 1 sine + 5 + 2 cosine = 16 in the source; two evaluations: 32
    assert _count(insts, r"v_cvt_i32_f32") == 1, insts   # one quadrant
