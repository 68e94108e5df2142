"""Static checks on the gfx950 ISA of the fused row_flow_v2 kernel (``rowflow_v2.hip``; hipcc cross-compiles without a GPU), after
tests/test_isa_hdr.py: nothing spills or touches scratch, the 1x9 layers are fp16 MFMA, and LDS and registers stay inside the
budget the file states for two workgroups of 256 threads per CU (160 KiB of LDS and 512 registers per SIMD lane on this part:
81920 B and 256 registers per workgroup)."""
import os
import re
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from nunif_amd import build  # noqa: E402

LDS_BUDGET, VGPR_BUDGET = 81920, 256
LDS_STATED = 78720                       # the figure in the header comment of rowflow_v2.hip and in DESIGN.md


@pytest.fixture(scope="module")
def kernels(tmp_path_factory):
    """{mangled kernel name: (body, metadata dict)} of rowflow_v2.hip"""
    try:
        build.hipcc()
    except RuntimeError:
        pytest.skip("hipcc not available")
    out = os.path.join(str(tmp_path_factory.mktemp("isa")), "rowflow_v2.s")
    flags = [x for x in build.FLAGS if x != "-fPIC"] + build.EXTRA_FLAGS.get("rowflow_v2.hip", [])
    subprocess.run([build.hipcc()] + flags + ["-S", "--cuda-device-only", "-I", os.path.join(ROOT, "include"), "-o", out,
                                              os.path.join(build.CSRC, "rowflow_v2.hip")], check=True, capture_output=True)
    text = open(out).read()
    meta = {}
    for block in re.split(r"\n\s+- \.agpr_count:", text)[1:]:
        name = re.search(r"\.name:\s+(\S+)", block).group(1)
        meta[name] = {k: int(v) for k, v in re.findall(r"\.(\w+):\s+(\d+)\n", block.split("\n  - ")[0])}
    found = {}
    for m in re.finditer(r"^(_Z\w+):.*?\n(.*?)s_endpgm", text, re.S | re.M):
        if m.group(1) in meta:
            found[m.group(1)] = (m.group(2), meta[m.group(1)])
    return found


def test_both_instances_are_there(kernels):
    assert len(kernels) == 2 and all("rf2_kernel" in k for k in kernels), sorted(kernels)      # delta, debug taps


def test_no_scratch_no_spills(kernels):
    for name, (body, md) in kernels.items():
        assert md["private_segment_fixed_size"] == 0 and md["vgpr_spill_count"] == 0, (name, md)
        assert "scratch_" not in body, name


def test_fp16_mfma_carries_the_row_convs(kernels):
    for name, (body, md) in kernels.items():
        n = len(re.findall(r"^\s*v_mfma_f32_16x16x32[_.]f16", body, re.M))
        assert n == 5 + 10 + 18, (name, n)           # one per weight fragment: L1 1 x 5, L2 2 x 5, L3 2 x 9 (n-tiles x k-steps)


def test_lds_and_registers_fit_two_workgroups_per_cu(kernels):
    for name, (body, md) in kernels.items():
        assert md["group_segment_fixed_size"] == LDS_STATED <= LDS_BUDGET, (name, md["group_segment_fixed_size"])
        assert md["vgpr_count"] <= VGPR_BUDGET, (name, md)          # the unified count: arch + acc registers
