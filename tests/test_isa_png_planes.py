"""Static check on the gfx950 code object of nunif_amd/csrc/png_planes.hip, the plane forms of the PNG encoder (4 RGBA 8, 5 grey 8,
6 grey + alpha 8), metadata only: the three instantiations of the filter kernel are there and nothing else, they have no private
segment and spill nothing, use no LDS and stay within the 64 VGPRs tests/test_isa_png.py holds the instantiations of png.hip to.
The kernels behind the filtered bytes are png.hip's, and that test keeps their budgets."""
import os
import re
import subprocess

import pytest

from nunif_amd import build

FNAME = "png_planes.hip"
# kernel: (LDS bytes, VGPRs, workgroup size)
NEW = {"png_filter_kernelILi4E": (0, 64, 256), "png_filter_kernelILi5E": (0, 64, 256), "png_filter_kernelILi6E": (0, 64, 256)}


@pytest.fixture(scope="module")
def meta(tmp_path_factory):
    out = os.path.join(str(tmp_path_factory.mktemp("isa_png_planes")), FNAME + ".s")
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


def test_the_plane_filter_kernels_have_no_scratch_and_stay_inside_the_budget(meta):
    assert len(meta) == len(NEW)
    for stem, (lds, vgprs, threads) in NEW.items():
        name = next((k for k in meta if stem in k), None)
        assert name, stem
        m = meta[name]
        print(name, m)
        assert m["private_segment_fixed_size"] == 0 and m["vgpr_spill_count"] == 0 and m["sgpr_spill_count"] == 0, (name, m)
        assert m["group_segment_fixed_size"] <= lds, (name, m)
        assert m["vgpr_count"] <= vgprs, (name, m)
        assert m["max_flat_workgroup_size"] == threads, (name, m)
