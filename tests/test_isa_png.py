"""Static check on the gfx950 code objects of nunif_amd/csrc/png.hip (hipcc cross-compiles without a GPU), metadata only: every
kernel of the file is there, none has a private segment or spills, the LDS of each stays inside the budget DESIGN.md states
(16 KB for the emit kernel: its bit buffer of one pass, the CRC table and the code tables; 8 KB for the one-wave code builder;
4 KB for the histogram kernel), and the VGPR counts allow the launch shapes: at most 128 for the 256-thread kernels that keep a
stripe each (four workgroups per CU), at most 64 for the others."""
import os
import re
import subprocess

import pytest

from nunif_amd import build

FNAME = "png.hip"
# kernel: (LDS bytes, VGPRs, workgroup size)
BUDGET = {"png_filter_kernelILi0E": (0, 64, 256), "png_filter_kernelILi1E": (0, 64, 256), "png_filter_kernelILi2E": (0, 64, 256),
          "png_hist_kernel": (4 * 1024, 64, 256), "png_codes_kernel": (8 * 1024, 64, 64), "png_scan_kernel": (256, 64, 256),
          "png_emit_kernel": (16 * 1024, 128, 256)}


@pytest.fixture(scope="module")
def meta(tmp_path_factory):
    out = os.path.join(str(tmp_path_factory.mktemp("isa_png")), FNAME + ".s")
    flags = [x for x in build.FLAGS if x != "-fPIC"] + build.EXTRA_FLAGS.get(FNAME, [])
    subprocess.run([build.hipcc()] + flags + ["-S", "--cuda-device-only", "-o", out, os.path.join(build.CSRC, FNAME)],
                   check=True, capture_output=True)
    text = open(out).read()
    found = {}
    for blk in text.split("- .agpr_count:")[1:]:
        name = re.search(r"\.name:\s+(\S+)", blk).group(1)
        found[name] = {key: int(re.search(r"\." + key + r":\s+(\d+)", blk).group(1))
                       for key in ("private_segment_fixed_size", "vgpr_spill_count", "sgpr_spill_count",
                                   "group_segment_fixed_size", "max_flat_workgroup_size", "vgpr_count")}
    return found


def test_every_kernel_is_there_without_scratch_and_inside_its_budget(meta):
    assert len(meta) == len(BUDGET)
    for stem, (lds, vgprs, threads) in BUDGET.items():
        name = next((k for k in meta if stem in k), None)
        assert name, stem
        m = meta[name]
        assert m["private_segment_fixed_size"] == 0 and m["vgpr_spill_count"] == 0 and m["sgpr_spill_count"] == 0, (name, m)
        assert m["group_segment_fixed_size"] <= lds, (name, m)
        assert m["vgpr_count"] <= vgprs, (name, m)
        assert m["max_flat_workgroup_size"] == threads, (name, m)
