"""Static check on the gfx950 ISA of nunif_amd/csrc/cliqa.hip (hipcc cross-compiles without a GPU): every kernel is there, none uses
scratch memory, the matrix instructions are the f16 MFMA family only, and every workgroup's LDS stays within 64 KB."""
import os
import re
import subprocess

import pytest

from nunif_amd import build

FNAME = "cliqa.hip"
KERNELS = ("cliqa_entry_kernel", "cliqa_conv_pool_kernelILi64E", "cliqa_conv_pool_kernelILi128E", "cliqa_head_kernel",
           "cliqa_head_final_kernel", "cliqa_patch_score_kernel", "cliqa_patch_gather_kernel")


@pytest.fixture(scope="module")
def isa(tmp_path_factory):
    out = os.path.join(str(tmp_path_factory.mktemp("isa_cliqa")), FNAME + ".s")
    flags = [x for x in build.FLAGS if x != "-fPIC"] + build.EXTRA_FLAGS.get(FNAME, [])
    subprocess.run([build.hipcc()] + flags + ["-S", "--cuda-device-only", "-o", out, os.path.join(build.CSRC, FNAME)],
                   check=True, capture_output=True)
    text = open(out).read()
    meta = {}
    for blk in text.split("- .agpr_count:")[1:]:
        name = re.search(r"\.name:\s+(\S+)", blk).group(1)
        meta[name] = {k: int(re.search(r"\.%s:\s+(\d+)" % k, blk).group(1))
                      for k in ("private_segment_fixed_size", "vgpr_spill_count", "sgpr_spill_count", "group_segment_fixed_size")}
    return text, meta


def test_every_kernel_is_there_without_scratch_and_within_64k_of_lds(isa):
    _, meta = isa
    for stem in KERNELS:
        assert any(stem in k for k in meta), stem
    for name, m in meta.items():
        assert m["private_segment_fixed_size"] == 0 and m["vgpr_spill_count"] == 0, (name, m)
        assert m["group_segment_fixed_size"] <= 64 * 1024, (name, m)


def test_matrix_instructions_are_f16_mfma_only(isa):
    text, _ = isa
    ops = set(re.findall(r"^\s+(v_(?:mfma|smfmac|wmma|swmmac)\w+)", text, flags=re.M))
    assert ops, "no matrix instruction in cliqa.hip"
    assert all(re.fullmatch(r"v_mfma_f32_(16x16x32|32x32x16)_f16", op) for op in ops), ops
