"""Static checks on the gfx950 ISA of the fused HDR planar entry (``hdr_planes.hip``; hipcc cross-compiles without a GPU), after
tests/test_isa_hdr.py: six kernels, {PQ, HLG} x {u16, chw, debug}; nothing spills or touches scratch or LDS; the fast path keeps its
16-byte luma loads and 16-byte stores; no flat accesses; and at most 128 VGPRs — the 256-thread block is one wave per SIMD, and 128
registers keep four blocks resident on a CU, the target tests/test_isa_pixfmt.py states for the kernel this one shares its shape with.

Measured VGPR counts (ROCm 7.2 hipcc): PQ 70 / 70 / 70, HLG 68 / 69 / 67 for u16 / chw / debug — seven waves per SIMD."""
import os
import re
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from nunif_amd import build  # noqa: E402

VGPR_TARGET = 128


@pytest.fixture(scope="module")
def kernels(tmp_path_factory):
    """{mangled kernel name: (body, vgprs, spills, scratch bytes, LDS bytes)} of hdr_planes.hip"""
    try:
        build.hipcc()
    except RuntimeError:
        pytest.skip("hipcc not available")
    out = os.path.join(str(tmp_path_factory.mktemp("isa")), "hdr_planes.s")
    flags = [x for x in build.FLAGS if x != "-fPIC"] + build.EXTRA_FLAGS.get("hdr_planes.hip", [])
    subprocess.run([build.hipcc()] + flags + ["-S", "--cuda-device-only", "-I", os.path.join(ROOT, "include"), "-o", out,
                                              os.path.join(build.CSRC, "hdr_planes.hip")], check=True, capture_output=True)
    text = open(out).read()
    meta = {m.group(2): (int(m.group(4)), int(m.group(5)), int(m.group(3)), int(m.group(1))) for m in re.finditer(
        r"\.group_segment_fixed_size:\s+(\d+)\n(?:.*\n)*?\s+\.name:\s+(\S+)\n(?:.*\n)*?\s+\.private_segment_fixed_size:\s+(\d+)\n"
        r"(?:.*\n)*?\s+\.vgpr_count:\s+(\d+)\n\s+\.vgpr_spill_count:\s+(\d+)", text)}
    found = {}
    for m in re.finditer(r"^(_Z\w+):.*?\n(.*?)\.Lfunc_end", text, re.S | re.M):
        if m.group(1) in meta:
            found[m.group(1)] = (m.group(2),) + meta[m.group(1)]
    return found


def _ops(body, prefix):
    return re.findall(rf"^\s*({prefix}\w*)", body, re.M)


def test_hdr_planes_is_built_without_fp_contraction_and_without_slp():
    flags = build.EXTRA_FLAGS.get("hdr_planes.hip", [])
    assert "-ffp-contract=off" in flags and "-fno-slp-vectorize" in flags      # bit-equal to pixfmt.hip + hdr.hip, built the same way


def test_six_kernels_without_scratch_spills_or_lds(kernels):
    assert len(kernels) == 6, sorted(kernels)                                  # {PQ, HLG} x {u16, chw, debug}
    for trc in (16, 18):
        for form in (0, 1, 2):
            assert sum(f"yuv_hdr_to_tensor_kernelILi{trc}ELi{form}E" in n for n in kernels) == 1, (trc, form)
    for name, (body, vg, sp, scratch, lds) in kernels.items():
        print(name, "VGPRs", vg)
        assert sp == 0 and scratch == 0 and lds == 0 and "scratch_" not in body, (name, sp, scratch, lds)
        assert vg <= VGPR_TARGET, (name, vg)
        assert not _ops(body, "flat_") and not _ops(body, "ds_") and not _ops(body, "buffer_"), name


@pytest.mark.parametrize("trc", [16, 18])
@pytest.mark.parametrize("form,stores", [(0, 3), (1, 6), (2, 6)])
def test_fast_path_keeps_its_16_byte_accesses(kernels, trc, form, stores):
    (name, (body, *_)), = [kv for kv in kernels.items() if f"yuv_hdr_to_tensor_kernelILi{trc}ELi{form}E" in kv[0]]
    loads, st = _ops(body, "global_load_"), _ops(body, "global_store_")
    assert loads.count("global_load_dwordx4") >= 2, (name, loads)              # the two luma rows: 8 samples of 16 bits each
    assert loads.count("global_load_dwordx2") >= 6, (name, loads)              # 3 rows x 2 planes of the chroma neighbourhood
    assert st.count("global_store_dwordx4") >= 2 * stores, (name, st)          # two rows, each in the form's 16-byte pieces
