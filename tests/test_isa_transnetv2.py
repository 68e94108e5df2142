"""Static checks on the gfx950 ISA of nunif_amd/csrc/transnetv2.hip (hipcc cross-compiles without a GPU): the GEMM kernels keep
their accumulators in registers (no scratch, no spills), the matrix path is the exact fp32-input MFMA, and nothing in the file uses
an fp16 / bf16 MFMA (the reference runs this net in fp32 and thresholds the result)."""
import os
import re
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from nunif_amd import build  # noqa: E402

FNAME = "transnetv2.hip"


@pytest.fixture(scope="module")
def isa(tmp_path_factory):
    try:
        build.hipcc()
    except RuntimeError:
        pytest.skip("hipcc not available")
    out = os.path.join(str(tmp_path_factory.mktemp("isa_transnetv2")), FNAME + ".s")
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
    for needle in ("tn_gemm", "tn_spatial_mean", "tn_project", "tn_histogram", "tn_band_fc", "tn_heads"):
        assert needle in names, needle
    assert sum("tn_gemm" in k for k in isa) == 8          # spatial x3, temporal x2, temporal+pool x2, fc1


def test_gemm_kernels_have_no_scratch_and_no_spills(isa):
    for name, (body, vgprs, spills) in isa.items():
        assert spills == 0 and "scratch_" not in body, (name, spills)
        assert vgprs <= 256, (name, vgprs)


def test_matrix_path_is_fp32_input_mfma_only(isa):
    for name, (body, _, _) in isa.items():
        mfma = set(re.findall(r"\bv_mfma_\w+", body))
        if "tn_gemm" in name:
            assert mfma == {"v_mfma_f32_32x32x2_f32"}, (name, mfma)
        else:
            assert not mfma, (name, mfma)
        assert not re.search(r"v_mfma_\w*(f16|bf16|fp8|bf8)", body), name
        assert "v_cvt_f16_f32" not in body and "v_cvt_pk_bf16_f32" not in body, name


def test_histogram_counts_in_lds(isa):
    (body,) = [b for k, (b, _, _) in isa.items() if "tn_histogram" in k]
    assert re.search(r"ds_add_(rtn_)?u32", body) and "global_atomic" not in body
