"""Static check on the gfx950 ISA of nunif_amd/csrc/autocrop.hip (hipcc cross-compiles without a GPU): every kernel of the file
builds without scratch memory, and the full-frame passes move 16 bytes per lane: ``crop_pad`` loads and stores them, the row pass
and both column passes load them."""
import os
import re
import subprocess

import pytest

from nunif_amd import build

FNAME = "autocrop.hip"
LOAD16, STORE16 = "global_load_dwordx4", "global_store_dwordx4"


@pytest.fixture(scope="module")
def kernels(tmp_path_factory):
    out = os.path.join(str(tmp_path_factory.mktemp("isa_autocrop")), FNAME + ".s")
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
    body = {}
    for name in meta:
        m = re.search(r"^" + re.escape(name) + r":[^\n]*\n(.*?)\n\s*s_endpgm", text, flags=re.S | re.M)
        body[name] = m.group(1)
    return meta, body


def test_every_kernel_is_there_and_none_uses_scratch(kernels):
    meta, _ = kernels
    for stem in ("autocrop_rows_kernelILb0E", "autocrop_rows_kernelILb1E", "autocrop_cols_partial_kernelILi4E",
                 "autocrop_cols_partial_kernelILi1E", "autocrop_cols_final_kernel", "autocrop_cols_flat_kernelILi4E",
                 "autocrop_cols_flat_kernelILi1E", "autocrop_crop_pad_kernelILb1E", "autocrop_crop_pad_kernelILb0E"):
        assert any(stem in k for k in meta), stem
    for name, (scratch, vspill, sspill) in meta.items():
        assert scratch == 0 and vspill == 0 and sspill == 0, (name, scratch, vspill, sspill)


def test_full_frame_accesses_are_16_bytes_wide(kernels):
    _, body = kernels

    def one(stem):
        return next(v for k, v in body.items() if stem in k)

    crop = one("autocrop_crop_pad_kernelILb1E")
    assert LOAD16 in crop and STORE16 in crop
    for stem in ("autocrop_rows_kernelILb0E", "autocrop_rows_kernelILb1E", "autocrop_cols_partial_kernelILi4E",
                 "autocrop_cols_flat_kernelILi4E"):
        assert LOAD16 in one(stem), stem
