"""Static checks on the gfx950 ISA of nunif_amd/csrc/stlizer_pass3.hip (hipcc cross-compiles without a GPU), after
tests/test_isa_find_transform.py: no kernel uses scratch or spills, and each stays inside a register budget."""
import os
import re
import subprocess

import pytest

from nunif_amd import build

FNAME = "stlizer_pass3.hip"
# 256-thread workgroups, one wave per SIMD: 64 VGPRs or fewer keep all 8 waves of a SIMD resident.  The launches are latency
# bound, so residency is what lets the many small workgroups of a long video overlap.
VGPR_BUDGET = 64
KERNELS = ("pass3_begin_kernel", "pass3_recursion_kernel", "pass3_move_kernel", "pass3_output_kernel", "pass3_scene_weight_kernel",
           "pass3_prefix_kernel", "pass3_conv_kernel")


@pytest.fixture(scope="module")
def kernels(tmp_path_factory):
    try:
        build.hipcc()
    except RuntimeError:
        pytest.skip("hipcc not available")
    out = os.path.join(str(tmp_path_factory.mktemp("isa_pass3")), FNAME + ".s")
    flags = [x for x in build.FLAGS if x != "-fPIC"] + build.EXTRA_FLAGS.get(FNAME, [])
    subprocess.run([build.hipcc()] + flags + ["-S", "--cuda-device-only", "-o", out, os.path.join(build.CSRC, FNAME)],
                   check=True, capture_output=True)
    text = open(out).read()
    meta = {}
    for blk in text.split("- .agpr_count:")[1:]:
        name = re.search(r"\.name:\s+(\S+)", blk).group(1)
        meta[name] = tuple(int(re.search(rf"\.{key}:\s+(\d+)", blk).group(1))
                           for key in ("private_segment_fixed_size", "vgpr_spill_count", "sgpr_spill_count", "vgpr_count"))
    return meta


def test_built_without_fp_contraction():
    assert "-ffp-contract=off" in build.EXTRA_FLAGS.get(FNAME, [])


def test_every_kernel_is_there_without_scratch_or_spills_and_inside_its_register_budget(kernels):
    for k in KERNELS:
        assert any(k in name for name in kernels), k
    for name, (scratch, vspill, sspill, vgpr) in kernels.items():
        print(f"{name}: {vgpr} VGPRs")
        assert scratch == 0 and vspill == 0 and sspill == 0, (name, scratch, vspill, sspill)
        assert vgpr <= VGPR_BUDGET, (name, vgpr)
