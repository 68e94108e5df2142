"""Static check on the gfx950 ISA of nunif_amd/csrc/sod_v1.hip (hipcc cross-compiles without a GPU): every kernel of the file
builds without scratch memory (no private segment, no vector register spilled to it).  And the per-frame forward warp of
iw3_warp.hip (``forward_warp_per_frame_kernel``, the same rows as ``forward_warp_kernel`` with the convergence read on the device)
keeps the scalar kernel's occupancy limits: 1024 threads x 2 workgroups per CU need <= 64 VGPRs and <= 80 SGPRs."""
import os
import re
import subprocess

import pytest

from nunif_amd import build

FNAME = "sod_v1.hip"


@pytest.fixture(scope="module")
def kernels(tmp_path_factory):
    out = os.path.join(str(tmp_path_factory.mktemp("isa_sod")), FNAME + ".s")
    flags = [x for x in build.FLAGS if x != "-fPIC"] + build.EXTRA_FLAGS.get(FNAME, [])
    subprocess.run([build.hipcc()] + flags + ["-S", "--cuda-device-only", "-o", out, os.path.join(build.CSRC, FNAME)],
                   check=True, capture_output=True)
    text = open(out).read()
    meta = {}
    for blk in text.split("- .agpr_count:")[1:]:
        name = re.search(r"\.name:\s+(\S+)", blk).group(1)
        meta[name] = (int(re.search(r"\.private_segment_fixed_size:\s+(\d+)", blk).group(1)),
                      int(re.search(r"\.vgpr_spill_count:\s+(\d+)", blk).group(1)),
                      int(re.search(r"\.sgpr_spill_count:\s+(\d+)", blk).group(1)))
    return meta


def test_every_kernel_is_there_and_none_uses_scratch(kernels):
    for stem in ("sod_entry_kernel", "sod_conv_kernelILi0E", "sod_conv_kernelILi1E", "sod_conv_kernelILi2E", "sod_head_kernel",
                 "sod_depth_position_kernel", "sod_ema_kernel"):
        assert any(stem in k for k in kernels), stem
    for name, (scratch, vspill, sspill) in kernels.items():
        assert scratch == 0 and vspill == 0, (name, scratch, vspill, sspill)


def test_per_frame_forward_warp_keeps_two_rows_per_cu(tmp_path):
    fname = "iw3_warp.hip"
    out = str(tmp_path / (fname + ".s"))
    flags = [x for x in build.FLAGS if x != "-fPIC"] + build.EXTRA_FLAGS.get(fname, [])
    subprocess.run([build.hipcc()] + flags + ["-S", "--cuda-device-only", "-o", out, os.path.join(build.CSRC, fname)],
                   check=True, capture_output=True)
    hits = []
    for blk in open(out).read().split("- .agpr_count:")[1:]:
        name = re.search(r"\.name:\s+(\S+)", blk).group(1)
        if "forward_warp_per_frame_kernel" in name:
            hits.append((name, int(re.search(r"\.sgpr_count:\s+(\d+)", blk).group(1)), int(re.search(r"\.vgpr_count:\s+(\d+)", blk).group(1)),
                         int(re.search(r"\.private_segment_fixed_size:\s+(\d+)", blk).group(1))))
    assert len(hits) == 2                       # rows up to 2 048 pixels, and up to 4 096
    for name, sg, vg, scratch in hits:
        assert vg <= 64 and sg <= 80 and scratch == 0, (name, sg, vg, scratch)
