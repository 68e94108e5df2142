"""Static checks on the gfx950 ISA of nunif_amd/csrc/superpoint.hip (hipcc cross-compiles without a GPU): no kernel uses scratch
or spills, the convolutions run on the exact fp32-input MFMA and nothing in the file uses a reduced-precision one, and the warp and
the descriptor sampler move 16 bytes per access along their contiguous axis."""
import os
import re
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from nunif_amd import build  # noqa: E402

FNAME = "superpoint.hip"


@pytest.fixture(scope="module")
def isa(tmp_path_factory):
    try:
        build.hipcc()
    except RuntimeError:
        pytest.skip("hipcc not available")
    out = os.path.join(str(tmp_path_factory.mktemp("isa_superpoint")), FNAME + ".s")
    flags = [x for x in build.FLAGS if x != "-fPIC"] + build.EXTRA_FLAGS.get(FNAME, [])
    subprocess.run([build.hipcc()] + flags + ["-S", "--cuda-device-only", "-I", os.path.join(ROOT, "include"), "-o", out,
                                              os.path.join(build.CSRC, FNAME)], check=True, capture_output=True)
    text = open(out).read()
    meta = {m.group(1): (int(m.group(2)), int(m.group(3))) for m in re.finditer(
        r"\.name:\s+(\S+)\n(?:.*\n)*?\s+\.vgpr_count:\s+(\d+)\n\s+\.vgpr_spill_count:\s+(\d+)", text)}
    bodies = {m.group(1): m.group(2) for m in re.finditer(r"^(_Z\w+):.*?\n(.*?)s_endpgm", text, re.S | re.M)}
    return {k: (bodies[k],) + meta[k] for k in bodies if k in meta}


def test_every_kernel_is_there(isa):
    names = " ".join(isa)
    for needle in ("sp_gemm", "sp_conv_first", "sp_nms_step", "sp_row_count", "sp_row_scan", "sp_compact", "sp_sample", "sp_match",
                   "sp_affine_warp"):
        assert needle in names, needle
    assert sum("sp_gemm" in k for k in isa) == 6          # 3x3 conv at 64 / 128 columns, each with and without the pool; two heads


def test_no_scratch_and_no_spills(isa):
    for name, (body, vgprs, spills) in isa.items():
        assert spills == 0 and "scratch_" not in body, (name, spills)
        assert vgprs <= 256, (name, vgprs)


def test_conv_kernels_run_on_the_fp32_input_mfma_only(isa):
    for name, (body, _, _) in isa.items():
        mfma = set(re.findall(r"\bv_mfma_\w+", body))
        if "sp_gemm" in name:
            assert mfma == {"v_mfma_f32_32x32x2_f32"}, (name, mfma)
        else:
            assert not mfma, (name, mfma)
        assert "v_cvt_f16_f32" not in body and "v_cvt_pk_bf16_f32" not in body, name


def test_warp_and_sampler_use_wide_accesses(isa):
    (vec,) = [b for k, (b, _, _) in isa.items() if "sp_affine_warpILb1" in k]
    assert "global_store_dwordx4" in vec
    (sampler,) = [b for k, (b, _, _) in isa.items() if "sp_sample" in k]
    assert "global_load_dwordx4" in sampler and "global_store_dwordx4" in sampler
    assert not re.search(r"global_load_dword\s", sampler.split("global_load_dwordx4", 1)[1]), "taps are 16-byte loads"
