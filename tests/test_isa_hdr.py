"""Static checks on the gfx950 ISA of the HDR -> SDR kernels (``hdr.hip``; hipcc cross-compiles without a GPU), after
tests/test_isa_grain.py: the lane-owns-eight-pixels instances read rgb48 in three 16-byte loads and store nothing narrower than 16
bytes, nothing spills, and the register count leaves the 256-thread launch shape its full occupancy."""
import os
import re
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from nunif_amd import build  # noqa: E402


@pytest.fixture(scope="module")
def kernels(tmp_path_factory):
    """{mangled kernel name: (body, vgprs, spills)} of hdr.hip"""
    try:
        build.hipcc()
    except RuntimeError:
        pytest.skip("hipcc not available")
    out = os.path.join(str(tmp_path_factory.mktemp("isa")), "hdr.s")
    flags = [x for x in build.FLAGS if x != "-fPIC"] + build.EXTRA_FLAGS.get("hdr.hip", [])
    subprocess.run([build.hipcc()] + flags + ["-S", "--cuda-device-only", "-I", os.path.join(ROOT, "include"), "-o", out,
                                              os.path.join(build.CSRC, "hdr.hip")], check=True, capture_output=True)
    text = open(out).read()
    meta = {m.group(1): (int(m.group(2)), int(m.group(3))) for m in re.finditer(
        r"\.name:\s+(\S+)\n(?:.*\n)*?\s+\.vgpr_count:\s+(\d+)\n\s+\.vgpr_spill_count:\s+(\d+)", text)}
    found = {}
    for m in re.finditer(r"^(_Z\w+):.*?\n(.*?)s_endpgm", text, re.S | re.M):
        if m.group(1) in meta:
            found[m.group(1)] = (m.group(2),) + meta[m.group(1)]
    return found


def _ops(body, prefix):
    return re.findall(rf"^\s*({prefix}\w*)", body, re.M)


def test_hdr_is_built_without_fp_contraction():
    assert "-ffp-contract=off" in build.EXTRA_FLAGS.get("hdr.hip", [])           # the reference's roundings, operation by operation


def test_no_kernel_of_hdr_hip_spills_or_uses_scratch(kernels):
    assert len(kernels) == 12, sorted(kernels)                                   # {PQ, HLG} x {u16, chw, debug} x {8 pixels, 1 pixel}
    for name, (body, vg, sp) in kernels.items():
        # 256 threads = 4 waves per block, one per SIMD; 64 registers or fewer keep all 8 waves of a SIMD resident
        assert sp == 0 and "scratch_" not in body and vg <= 64, (name, vg, sp)


@pytest.mark.parametrize("trc", [16, 18])
@pytest.mark.parametrize("form,stores", [(0, 3), (1, 6), (2, 6)])
def test_vector_path_keeps_its_16_byte_accesses(kernels, trc, form, stores):
    (name, (body, vg, sp)), = [kv for kv in kernels.items() if f"hdr2sdr_vec_kernelILi{trc}ELi{form}E" in kv[0]]
    loads, st = _ops(body, "global_load_"), _ops(body, "global_store_")
    assert loads == ["global_load_dwordx4"] * 3, (name, loads)                   # 8 pixels of rgb48 = 48 bytes
    assert st == ["global_store_dwordx4"] * stores, (name, st)
    assert not _ops(body, "flat_") and not _ops(body, "buffer_") and not _ops(body, "ds_"), name
