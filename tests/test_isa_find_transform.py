"""Static checks on the gfx950 ISA of nunif_amd/csrc/find_transform.hip (hipcc cross-compiles without a GPU), after
tests/test_isa_da3.py: the kernel uses no scratch and does not spill, and its register count stays inside what its launch shape
needs."""
import os
import re
import subprocess

import pytest

from nunif_amd import build

FNAME = "find_transform.hip"
# the build shows 35 VGPRs; a 256-thread workgroup is one wave per SIMD, and 64 or fewer keep all 8 waves of a SIMD resident, so
# eight pairs share a CU
VGPR_BUDGET = {"find_transform_step_kernel": 64}


@pytest.fixture(scope="module")
def kernels(tmp_path_factory):
    try:
        build.hipcc()
    except RuntimeError:
        pytest.skip("hipcc not available")
    out = os.path.join(str(tmp_path_factory.mktemp("isa_find_transform")), FNAME + ".s")
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


def test_the_kernel_is_there_without_scratch_or_spills_and_inside_its_register_budget(kernels):
    assert any("find_transform_step_kernel" in k for k in kernels)
    for name, (scratch, vspill, sspill, vgpr) in kernels.items():
        print(f"{name}: {vgpr} VGPRs")
        assert scratch == 0 and vspill == 0 and sspill == 0, (name, scratch, vspill, sspill)
        budget = next(v for k, v in VGPR_BUDGET.items() if k in name)
        assert vgpr <= budget, (name, vgpr, budget)
