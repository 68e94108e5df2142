"""Static checks on the gfx950 ISA of nunif_amd/csrc/outpaint.hip (hipcc cross-compiles without a GPU): no kernel uses scratch or
spills, every GEMM runs on the exact fp32-input MFMA and nothing in the file uses a reduced-precision one, and the window and tile
kernels stay inside 64 KiB of LDS so that two workgroups share a CU."""
import os
import re
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from nunif_amd import build  # noqa: E402

FNAME = "outpaint.hip"
GEMM_KERNELS = ("op_mha", "op_pool", "op_pw")


@pytest.fixture(scope="module")
def isa(tmp_path_factory):
    try:
        build.hipcc()
    except RuntimeError:
        pytest.skip("hipcc not available")
    out = os.path.join(str(tmp_path_factory.mktemp("isa_outpaint")), FNAME + ".s")
    flags = [x for x in build.FLAGS if x != "-fPIC"] + build.EXTRA_FLAGS.get(FNAME, [])
    subprocess.run([build.hipcc()] + flags + ["-S", "--cuda-device-only", "-I", os.path.join(ROOT, "include"), "-o", out,
                                              os.path.join(build.CSRC, FNAME)], check=True, capture_output=True)
    text = open(out).read()
    meta = {}
    for m in re.finditer(r"- \.agpr_count:.*?\.name:\s+(\S+)\n.*?\.wavefront_size", text, re.S):
        block = m.group(0)
        field = lambda k: int(re.search(r"\." + k + r":\s+(\d+)", block).group(1))      # noqa: E731
        meta[m.group(1)] = (field("vgpr_count"), field("vgpr_spill_count"), field("private_segment_fixed_size"),
                            field("group_segment_fixed_size"))
    bodies = {m.group(1): m.group(2) for m in re.finditer(r"^(_Z\w+):.*?\n(.*?)s_endpgm", text, re.S | re.M)}
    return {k: (bodies[k],) + meta[k] for k in bodies if k in meta}


def test_every_kernel_is_there(isa):
    names = " ".join(isa)
    for needle in ("op_entry", "op_down", "op_mha", "op_pool", "op_pw", "op_proj3", "op_exit", "op_buffer"):
        assert needle in names, needle
    assert sum("op_mha" in k for k in isa) == 2 and sum("op_pool" in k for k in isa) == 2        # C = 64 and C = 32
    assert sum("op_down" in k for k in isa) == 3 and sum("op_pw" in k for k in isa) == 2


def test_no_scratch_no_spills_and_lds_for_two_workgroups(isa):
    for name, (body, vgprs, spills, private, lds) in isa.items():
        assert spills == 0 and private == 0 and "scratch_" not in body, (name, spills, private)
        assert vgprs <= 256, (name, vgprs)
        assert lds <= 65536, (name, lds)


def test_gemms_run_on_the_fp32_input_mfma_only(isa):
    for name, (body, *_rest) in isa.items():
        mfma = set(re.findall(r"\bv_mfma_\w+", body))
        if any(k in name for k in GEMM_KERNELS):
            assert mfma == {"v_mfma_f32_32x32x2_f32"}, (name, mfma)
        else:
            assert not mfma, (name, mfma)
        assert "v_cvt_f16_f32" not in body and "v_cvt_pk_bf16_f32" not in body, name
