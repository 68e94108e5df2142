"""Static check on the gfx950 ISA of nunif_amd/csrc/zoedepth_head.hip (hipcc cross-compiles without a GPU): every kernel of the
file builds without scratch memory and without LDS (the stages are pixel-parallel: weights come through scalar loads, the 1x1 convs
run on swin_kernels.hip's MFMA ``gemm_kernel``, so this file holds no MFMA of its own), inside the register budget of at least two
256-thread workgroups per SIMD row (128 VGPRs); the final stage reads the embedding and the bin centres 16 bytes per lane."""
import os
import re
import subprocess

import pytest

from nunif_amd import build

FNAME = "zoedepth_head.hip"
KERNELS = ("zoe_seed_kernel", "zoe_addup_kernel", "zoe_attractor_kernel", "zoe_final_kernel", "zoe_prep_kernel")


@pytest.fixture(scope="module")
def kernels(tmp_path_factory):
    out = os.path.join(str(tmp_path_factory.mktemp("isa_zoedepth")), FNAME + ".s")
    flags = [x for x in build.FLAGS if x != "-fPIC"] + build.EXTRA_FLAGS.get(FNAME, [])
    subprocess.run([build.hipcc()] + flags + ["-S", "--cuda-device-only", "-o", out, os.path.join(build.CSRC, FNAME)],
                   check=True, capture_output=True)
    text = open(out).read()
    meta = {}
    for blk in text.split("- .agpr_count:")[1:]:
        name = re.search(r"\.name:\s+(\S+)", blk).group(1)
        meta[name] = {k: int(re.search(r"\." + k + r":\s+(\d+)", blk).group(1))
                      for k in ("private_segment_fixed_size", "vgpr_spill_count", "sgpr_spill_count", "group_segment_fixed_size", "vgpr_count")}
    body = {}
    for name in meta:
        m = re.search(r"^" + re.escape(name) + r":[^\n]*\n(.*?)\n\s*s_endpgm", text, flags=re.S | re.M)
        body[name] = m.group(1)
    return meta, body


def test_kernels_no_scratch_no_lds_register_budget(kernels):
    meta, _ = kernels
    for stem in KERNELS:
        assert any(stem in k for k in meta), stem
    for name, m in meta.items():
        assert m["private_segment_fixed_size"] == 0 and m["vgpr_spill_count"] == 0 and m["sgpr_spill_count"] == 0, (name, m)
        assert m["group_segment_fixed_size"] == 0, (name, m)
        assert m["vgpr_count"] <= 128, (name, m)


def test_no_mfma_here_and_wide_loads_in_the_final_stage(kernels):
    _, body = kernels
    for name, text in body.items():
        assert "v_mfma" not in text, name
    final = next(v for k, v in body.items() if "zoe_final_kernel" in k)
    assert "global_load_dwordx4" in final
    assert "global_atomic" not in "".join(body.values())
