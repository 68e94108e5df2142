"""Static checks on the gfx950 ISA of the fused film-grain video step (``grain.hip``; hipcc cross-compiles without a GPU), after
tests/test_isa_invariants.py: it is a streaming kernel judged by bytes, so the lane-owns-four-pixels instances must keep their
wide accesses — 16-byte planar loads of the frame and the noise buffer, 16-byte stores of the noise buffer, and an HWC frame
store of at least 8 bytes per lane — and nothing may spill."""
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
    """{mangled kernel name: (body, vgprs, spills)} of grain.hip"""
    try:
        build.hipcc()
    except RuntimeError:
        pytest.skip("hipcc not available")
    out = os.path.join(str(tmp_path_factory.mktemp("isa")), "grain.s")
    flags = [x for x in build.FLAGS if x != "-fPIC"] + build.EXTRA_FLAGS.get("grain.hip", [])
    subprocess.run([build.hipcc()] + flags + ["-S", "--cuda-device-only", "-I", os.path.join(ROOT, "include"), "-o", out,
                                              os.path.join(build.CSRC, "grain.hip")], check=True, capture_output=True)
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


def test_grain_is_built_without_fp_contraction():
    assert "-ffp-contract=off" in build.EXTRA_FLAGS.get("grain.hip", [])        # fused == separate launches, byte for byte


def test_no_kernel_of_grain_hip_spills_or_uses_scratch(kernels):
    assert len(kernels) >= 9, sorted(kernels)
    for name, (body, vg, sp) in kernels.items():
        assert sp == 0 and "scratch_" not in body and vg <= 128, (name, vg, sp)


@pytest.mark.parametrize("pixel,frame_stores", [("Ih", {"global_store_dwordx3": 1}),
                                                ("It", {"global_store_dwordx4": 1, "global_store_dwordx2": 1})])
def test_fused_step_keeps_its_wide_accesses(kernels, pixel, frame_stores):
    (name, (body, vg, sp)), = [kv for kv in kernels.items() if "grain_video_step_kernel" + pixel + "Lb1E" in kv[0]]
    loads, stores = _ops(body, "global_load_"), _ops(body, "global_store_")
    # 3 channels x (frame, noise buffer): six 16-byte loads and nothing narrower
    assert loads.count("global_load_dwordx4") == 6 and len(loads) == 6, (name, loads)
    # the noise buffer: three 16-byte stores; the HWC frame: 12 B in one store (8 bit) or 16 B + 8 B (16 bit) — all >= 8 B per lane
    expect = {"global_store_dwordx4": 3}
    for op, n in frame_stores.items():
        expect[op] = expect.get(op, 0) + n
    assert {op: stores.count(op) for op in set(stores)} == expect, (name, stores)
    assert not _ops(body, "flat_") and not _ops(body, "buffer_"), name
