"""Static checks on the gfx950 ISA of the LISTED instance of the C = 192 tail (proj_mlp_ws_kernel<G32, true>), in the
manner of test_isa_invariants.py: the group descriptors must arrive by scalar loads only, so that the loop keeps no compiler-visible
vector load and the three hand-counted vmcnt waits stay the only ones in it.  hipcc cross-compiles without a GPU."""
import os
import re
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from nunif_amd import build  # noqa: E402

FNAME = "swin_block_tail_ws.hip"


@pytest.fixture(scope="module")
def instances(tmp_path_factory):
    """{(G32, LIST): (body, vgprs, spills)} of proj_mlp_ws_kernel"""
    try:
        hipcc = build.hipcc()
    except RuntimeError:
        pytest.skip("hipcc not available")
    out = str(tmp_path_factory.mktemp("isa_ws") / (FNAME + ".s"))
    flags = [x for x in build.FLAGS if x != "-fPIC"] + build.EXTRA_FLAGS.get(FNAME, [])
    subprocess.run([hipcc] + flags + ["-S", "--cuda-device-only", "-I", os.path.join(ROOT, "include"), "-o", out,
                                      os.path.join(build.CSRC, FNAME)], check=True, capture_output=True)
    text = open(out).read()
    meta = {m.group(1): (int(m.group(2)), int(m.group(3))) for m in re.finditer(
        r"\.name:\s+(\S+)\n(?:.*\n)*?\s+\.vgpr_count:\s+(\d+)\n\s+\.vgpr_spill_count:\s+(\d+)", text)}
    found = {}
    for m in re.finditer(r"^(_Z\w+):.*?\n(.*?)s_endpgm", text, re.S | re.M):
        k = re.search(r"proj_mlp_ws_kernelILb([01])ELb([01])E", m.group(1))
        if k and m.group(1) in meta:
            found[(int(k.group(1)), int(k.group(2)))] = (m.group(2),) + meta[m.group(1)]
    assert sorted(found) == [(0, 0), (0, 1), (1, 0), (1, 1)], sorted(found)
    return found


def _loop(body):
    lines = body.splitlines()
    head = max(i for i, ln in enumerate(lines) if "Loop Header" in ln or "Inner Loop" in ln)      # the trip loop is the last loop
    return lines[head:]


@pytest.mark.parametrize("g32", [0, 1])
def test_listed_instance_keeps_the_pipeline_of_the_whole_tile_one(instances, g32):
    body, vg, sp = instances[(g32, 1)]
    whole, wvg, wsp = instances[(g32, 0)]
    assert sp == 0 and "scratch_" not in body
    assert "flat_load" not in body
    assert vg <= 256, vg
    assert body.count("global_load_lds_dwordx4") == whole.count("global_load_lds_dwordx4") > 0
    waits = [re.sub(r"\s+", " ", ln.strip()) for ln in _loop(body) if "s_waitcnt" in ln and "vmcnt(" in ln]
    assert sorted(waits) == ["s_waitcnt vmcnt(0)", "s_waitcnt vmcnt(2)", "s_waitcnt vmcnt(4)"], waits
    # the descriptors: scalar loads of 32 bytes, and no vector load from global memory other than the LDS-DMA in the loop
    loop = _loop(body)
    assert any("s_load_dwordx8" in ln for ln in loop)
    assert not any(re.search(r"\b(global|buffer)_load_(?!lds_)", ln) for ln in loop), [ln for ln in loop if "global_load_d" in ln][:3]


@pytest.mark.parametrize("g32", [0, 1])
def test_whole_tile_instance_has_no_descriptor_loads(instances, g32):
    body, vg, sp = instances[(g32, 0)]
    assert sp == 0 and "scratch_" not in body and "flat_load" not in body
    assert "s_load_dwordx8" not in "\n".join(_loop(body))
    waits = [re.sub(r"\s+", " ", ln.strip()) for ln in _loop(body) if "s_waitcnt" in ln and "vmcnt(" in ln]
    assert sorted(waits) == ["s_waitcnt vmcnt(0)", "s_waitcnt vmcnt(2)", "s_waitcnt vmcnt(4)"], waits
