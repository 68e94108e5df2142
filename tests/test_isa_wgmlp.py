"""Static checks on the gfx950 ISA of wgmlp.hip (hipcc cross-compiles without a GPU), after tests/test_isa_row_flow_v2.py: the fused
window-gMLP kernel neither spills nor touches scratch, its four matrix products are fp16 MFMA, and its LDS and registers are the
figures csrc/wgmlp_host.h and DESIGN.md state: 52224 B at C = 128 (two workgroups of 256 threads per CU: 160 KiB of LDS and 512
registers per SIMD lane, so at most 256 registers) and 103424 B at C = 256 (one workgroup per CU)."""
import os
import re
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from nunif_amd import build  # noqa: E402

LDS_STATED = {128: 52224, 256: 103424}
# arch + acc registers per lane, (C, debug taps): the figures of DESIGN.md 7.12.  256 is the budget for two workgroups per CU.
VGPR_STATED = {(128, False): 252, (256, False): 328, (128, True): 305, (256, True): 391}


@pytest.fixture(scope="module")
def kernels(tmp_path_factory):
    """{mangled kernel name: (body, metadata dict)} of wgmlp.hip"""
    try:
        build.hipcc()
    except RuntimeError:
        pytest.skip("hipcc not available")
    out = os.path.join(str(tmp_path_factory.mktemp("isa")), "wgmlp.s")
    flags = [x for x in build.FLAGS if x != "-fPIC"] + build.EXTRA_FLAGS.get("wgmlp.hip", [])
    subprocess.run([build.hipcc()] + flags + ["-S", "--cuda-device-only", "-I", os.path.join(ROOT, "include"), "-o", out,
                                              os.path.join(build.CSRC, "wgmlp.hip")], check=True, capture_output=True)
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


def _gmlp(kernels):
    out = {}
    for name, v in kernels.items():
        m = re.search(r"wgmlp_block_kernelILi(\d+)ELb(\d)E", name)
        if m:
            out[(int(m.group(1)), bool(int(m.group(2))))] = v
    return out


def test_all_instances_are_there(kernels):
    assert sorted(_gmlp(kernels)) == [(128, False), (128, True), (256, False), (256, True)]      # C x debug taps
    assert sum("wg_stem_conv_kernel" in k for k in kernels) == 2                                   # 8 and 16 output channels


def test_no_scratch_no_spills(kernels):
    for name, (body, md) in kernels.items():
        assert md["private_segment_fixed_size"] == 0 and md["vgpr_spill_count"] == 0, (name, md)
        assert "scratch_" not in body, name


def test_fp16_mfma_carries_the_four_products(kernels):
    for (C, taps), (body, md) in _gmlp(kernels).items():
        n = len(re.findall(r"^\s*v_mfma_f32_16x16x32[_.]f16", body, re.M))
        # per loop body: proj_in and proj_out 2 tiles x 4 token tiles x C / 32 k-steps each, the mixing 4 token tiles x 2 k-steps
        assert n == 2 * (2 * 4 * C // 32) + 4 * 2, (C, taps, n)


def test_lds_and_registers_are_the_stated_figures(kernels):
    for (C, taps), (body, md) in _gmlp(kernels).items():
        assert md["group_segment_fixed_size"] == LDS_STATED[C], (C, taps, md["group_segment_fixed_size"])
        assert md["vgpr_count"] == VGPR_STATED[(C, taps)], (C, taps, md)       # the unified count: arch + acc registers
    assert VGPR_STATED[(128, False)] <= 256
