"""Static check on the gfx950 code objects of nunif_amd/csrc/jpeg.hip (hipcc cross-compiles without a GPU), metadata only: every
kernel of the file is there, none has a private segment or spills, and the LDS of each stays inside the budget DESIGN.md states:
16 KB for the entropy kernel (ten one-wave workgroups per CU) and 17 KB for the DCT kernels."""
import os
import re
import subprocess

import pytest

from nunif_amd import build

FNAME = "jpeg.hip"
LDS_BUDGET = {"jpeg_entropy_kernel": 16 * 1024, "jpeg_dct_kernelILi420E": 17 * 1024, "jpeg_dct_kernelILi444E": 17 * 1024,
              "jpeg_scan_kernel": 64, "jpeg_gather_kernel": 0}


@pytest.fixture(scope="module")
def meta(tmp_path_factory):
    out = os.path.join(str(tmp_path_factory.mktemp("isa_jpeg")), FNAME + ".s")
    flags = [x for x in build.FLAGS if x != "-fPIC"] + build.EXTRA_FLAGS.get(FNAME, [])
    subprocess.run([build.hipcc()] + flags + ["-S", "--cuda-device-only", "-o", out, os.path.join(build.CSRC, FNAME)],
                   check=True, capture_output=True)
    text = open(out).read()
    found = {}
    for blk in text.split("- .agpr_count:")[1:]:
        name = re.search(r"\.name:\s+(\S+)", blk).group(1)
        found[name] = {key: int(re.search(r"\." + key + r":\s+(\d+)", blk).group(1))
                       for key in ("private_segment_fixed_size", "vgpr_spill_count", "sgpr_spill_count",
                                   "group_segment_fixed_size", "max_flat_workgroup_size")}
    return found


def test_every_kernel_is_there_without_scratch_and_inside_its_lds_budget(meta):
    assert len(meta) == len(LDS_BUDGET)
    for stem, budget in LDS_BUDGET.items():
        name = next((k for k in meta if stem in k), None)
        assert name, stem
        m = meta[name]
        assert m["private_segment_fixed_size"] == 0 and m["vgpr_spill_count"] == 0 and m["sgpr_spill_count"] == 0, (name, m)
        assert m["group_segment_fixed_size"] <= budget, (name, m)


def test_the_entropy_kernel_is_one_wave(meta):
    name = next(k for k in meta if "jpeg_entropy_kernel" in k)
    assert meta[name]["max_flat_workgroup_size"] == 64
