"""Static checks on the gfx950 ISA of the pixel-format kernels (``pixfmt.hip``; hipcc cross-compiles without a GPU), after
tests/test_isa_hdr.py: nothing spills or touches scratch, the tensor side moves in 16-byte accesses, the luma planes in accesses of
8 bytes (uint8) or 16 bytes (uint16), and the register count keeps the 256-thread launch shape at its occupancy target.

Only the luma accesses are checked for their width.  A lane's share of a chroma plane at 4:2:0 is 4 samples: 4 bytes at 8 bit (one
4-byte access and one neighbouring sample), 8 bytes at 10 bit — the "8 bytes on the plane side" holds for luma at every format and
for chroma at 10 bit and at 4:4:4, not for 8-bit 4:2:0 chroma, which is what the 8-luma lane shape gives.

Measured VGPR counts (ROCm 7.2 hipcc): planes -> tensor 66 / 47 / 67 for yuv420p / yuv444p / yuv420p10le (71 / 52 / 71 with the rgb
side frame), tensor -> planes 78 / 50 / 80.  The target is 4 waves per SIMD (128 registers or fewer): both kernels stream, a lane
has 8 to 14 independent wide accesses in flight, and four blocks per CU already cover the memory latency; the counts above leave
6 or 7 waves."""
import os
import re
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from nunif_amd import build  # noqa: E402

VGPR_TARGET = 128
MEASURED_MAX = 80


@pytest.fixture(scope="module")
def kernels(tmp_path_factory):
    """{mangled kernel name: (body, vgprs, spills)} of pixfmt.hip"""
    try:
        build.hipcc()
    except RuntimeError:
        pytest.skip("hipcc not available")
    out = os.path.join(str(tmp_path_factory.mktemp("isa")), "pixfmt.s")
    flags = [x for x in build.FLAGS if x != "-fPIC"] + build.EXTRA_FLAGS.get("pixfmt.hip", [])
    subprocess.run([build.hipcc()] + flags + ["-S", "--cuda-device-only", "-I", os.path.join(ROOT, "include"), "-o", out,
                                              os.path.join(build.CSRC, "pixfmt.hip")], check=True, capture_output=True)
    text = open(out).read()
    meta = {m.group(1): (int(m.group(2)), int(m.group(3))) for m in re.finditer(
        r"\.name:\s+(\S+)\n(?:.*\n)*?\s+\.vgpr_count:\s+(\d+)\n\s+\.vgpr_spill_count:\s+(\d+)", text)}
    found = {}
    for m in re.finditer(r"^(_Z\w+):.*?\n(.*?)\.Lfunc_end", text, re.S | re.M):
        if m.group(1) in meta:
            found[m.group(1)] = (m.group(2),) + meta[m.group(1)]
    return found


def _ops(body, prefix):
    return re.findall(rf"^\s*({prefix}\w*)", body, re.M)


def test_pixfmt_is_built_without_fp_contraction_and_without_slp():
    flags = build.EXTRA_FLAGS.get("pixfmt.hip", [])
    assert "-ffp-contract=off" in flags and "-fno-slp-vectorize" in flags


def test_no_kernel_spills_or_uses_scratch(kernels):
    assert len(kernels) == 12, sorted(kernels)            # 3 formats x {chw, chw + frame, debug} in, 3 formats out
    for name, (body, vg, sp) in kernels.items():
        print(name, vg)
        assert sp == 0 and "scratch_" not in body and vg <= VGPR_TARGET, (name, vg, sp)
        assert vg <= MEASURED_MAX + 8, (name, vg)         # a compiler that needs a third more registers is worth a look
        assert not _ops(body, "flat_") and not _ops(body, "ds_"), name


@pytest.mark.parametrize("fmt,luma", [(0, "dwordx2"), (1, "dwordx2"), (2, "dwordx4")])
def test_entry_access_widths(kernels, fmt, luma):
    for name, (body, vg, sp) in kernels.items():
        if f"yuv_to_tensor_kernelILi{fmt}E" not in name:
            continue
        loads, stores = _ops(body, "global_load_"), _ops(body, "global_store_")
        assert loads.count(f"global_load_{luma}") >= 2, (name, loads)          # the two luma rows (and chroma at 4:4:4 / 10 bit)
        assert stores.count("global_store_dwordx4") >= 12, (name, stores)       # 2 rows x 3 channels x 2 pieces of the tensor
        if name.endswith("Lb1EEEvPKhS2_S2_lllPfPhiiiNS_8PixConstE"):
            # with the side frame: 24 bytes a row at 8 bit (hipcc joins them into 16 + 8), 48 bytes a row at 16 bit
            assert stores.count("global_store_dwordx4") >= (14 if fmt != 2 else 18), (name, stores)
            assert fmt == 2 or stores.count("global_store_dwordx2") >= 2, (name, stores)


@pytest.mark.parametrize("fmt,luma", [(0, "dwordx2"), (1, "dwordx2"), (2, "dwordx4")])
def test_exit_access_widths(kernels, fmt, luma):
    (name, (body, vg, sp)), = [kv for kv in kernels.items() if f"tensor_to_yuv_kernelILi{fmt}E" in kv[0]]
    loads, stores = _ops(body, "global_load_"), _ops(body, "global_store_")
    assert loads.count("global_load_dwordx4") >= 12, (name, loads)              # 2 rows x 3 channels x 2 pieces of the tensor
    assert stores.count(f"global_store_{luma}") >= 2, (name, stores)            # the two luma rows
