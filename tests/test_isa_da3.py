"""Static checks on the gfx950 ISA of nunif_amd/csrc/da3_disparity.hip (hipcc cross-compiles without a GPU), after
tests/test_isa_autocrop.py: no kernel uses scratch or spills, the per-pixel kernels move 16 bytes per lane, and the register counts
stay inside what their launch shapes need."""
import os
import re
import subprocess

import pytest

from nunif_amd import build

FNAME = "da3_disparity.hip"
LOAD16, STORE16 = "global_load_dwordx4", "global_store_dwordx4"
# VGPRs the build shows (hist 22, step 30, count 10 / 16, disparity 21 / 15, apply 30 / 26, mlp 62) with headroom; 64 or fewer keep
# all 8 waves of a SIMD resident, which the 1024-thread selection kernels (4 waves per SIMD and block) do not even need
VGPR_BUDGET = {"da3_hist_kernel": 32, "da3_step_kernel": 40, "da3_count_kernel": 24, "da3_disparity_kernel": 32,
               "da3mono_apply_kernel": 40, "da3mono_mlp_kernel": 64, "da3_debug_stats_kernel": 16}


@pytest.fixture(scope="module")
def kernels(tmp_path_factory):
    try:
        build.hipcc()
    except RuntimeError:
        pytest.skip("hipcc not available")
    out = os.path.join(str(tmp_path_factory.mktemp("isa_da3")), FNAME + ".s")
    flags = [x for x in build.FLAGS if x != "-fPIC"] + build.EXTRA_FLAGS.get(FNAME, [])
    subprocess.run([build.hipcc()] + flags + ["-S", "--cuda-device-only", "-o", out, os.path.join(build.CSRC, FNAME)],
                   check=True, capture_output=True)
    text = open(out).read()
    meta = {}
    for blk in text.split("- .agpr_count:")[1:]:
        name = re.search(r"\.name:\s+(\S+)", blk).group(1)
        meta[name] = tuple(int(re.search(rf"\.{key}:\s+(\d+)", blk).group(1))
                           for key in ("private_segment_fixed_size", "vgpr_spill_count", "sgpr_spill_count", "vgpr_count"))
    body = {}
    for name in meta:
        body[name] = re.search(r"^" + re.escape(name) + r":[^\n]*\n(.*?)\n\s*s_endpgm", text, flags=re.S | re.M).group(1)
    return meta, body


def test_built_without_fp_contraction():
    assert "-ffp-contract=off" in build.EXTRA_FLAGS.get(FNAME, [])


def test_every_kernel_is_there_without_scratch_or_spills_and_inside_its_register_budget(kernels):
    meta, _ = kernels
    for stem in ("da3_hist_kernelILb0ELb0E", "da3_hist_kernelILb0ELb1E", "da3_hist_kernelILb1ELb0E", "da3_hist_kernelILb1ELb1E",
                 "da3_step_kernelILi0E", "da3_step_kernelILi1E", "da3_count_kernelILb0E", "da3_count_kernelILb1E",
                 "da3_disparity_kernelILb0E", "da3_disparity_kernelILb1E", "da3mono_apply_kernelILb0E", "da3mono_apply_kernelILb1E",
                 "da3mono_mlp_kernel"):
        assert any(stem in k for k in meta), stem
    for name, (scratch, vspill, sspill, vgpr) in meta.items():
        print(f"{name}: {vgpr} VGPRs")
        assert scratch == 0 and vspill == 0 and sspill == 0, (name, scratch, vspill, sspill)
        budget = next(v for k, v in VGPR_BUDGET.items() if k in name)
        assert vgpr <= budget, (name, vgpr, budget)


def test_pixel_kernels_move_16_bytes_per_lane(kernels):
    _, body = kernels

    def ops(stem, prefix):
        return re.findall(rf"^\s*({prefix}\w*)", next(v for k, v in body.items() if stem in k), re.M)

    assert ops("da3_disparity_kernelILb1E", "global_load_").count(LOAD16) == 2           # depth and sky
    assert STORE16 in ops("da3_disparity_kernelILb1E", "global_store_")
    assert ops("da3mono_apply_kernelILb1E", "global_load_").count(LOAD16) == 1
    assert ops("da3mono_apply_kernelILb1E", "global_store_") == [STORE16]
    assert LOAD16 in ops("da3_count_kernelILb1E", "global_load_")
    assert LOAD16 in ops("da3_hist_kernelILb0ELb1E", "global_load_")
    assert ops("da3_hist_kernelILb1ELb1E", "global_load_").count(LOAD16) == 2
