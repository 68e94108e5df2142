"""The host half of the WABlock (nunif_amd/csrc/wa_block_host.h: the WindowScoreBias table and the packed arrays of one block, shared
by row_flow_v3, MLBW, DepthAA and, for the table, swin_unet_v2) checked on the CPU under the host sanitizers:
tests/cpp/wa_block_host_check.cpp builds them from a seeded state dict of its own, checks the padding rule of the stride-16 table, the
sizes and the refused shapes, and prints every table as 32-bit patterns and a 64-bit hash of every packed array.  Those must be the
values of tests/golden/wa_block_host.json, which was recorded once from the loops as they stood in rowflow.hip (make_block),
depth_aa.hip (make_daa_block) and swin_unet_v2.hip (make_wac) BEFORE they moved into the header — held verbatim in a throw-away program
with the same seeded inputs — and not from the header under test.  The program is a child process of its own; nothing is loaded into
this interpreter."""
import json
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from nunif_amd import build  # noqa: E402

CASES = {"w3c64": 16, "w4c64": 16, "w4c128": 16, "w8c32": 64, "t6": 36, "t8": 64}      # case -> table stride
ARRAYS = ["wfrag", "bqkv", "bproj", "w1", "b1", "w3", "b3"]


@pytest.fixture(scope="module")
def check_output(tmp_path_factory):
    try:
        hipcc = build.hipcc()
    except RuntimeError:
        pytest.skip("hipcc not available")
    exe = str(tmp_path_factory.mktemp("wa_block") / "wa_block_host_check")
    src = os.path.join(ROOT, "tests", "cpp", "wa_block_host_check.cpp")
    cmd = [hipcc, "-O1", "-g", "-std=c++17", f"--offload-arch={build.ARCH}", "-x", "hip", "-Wall", "-Wno-unused-function",
           "-Xarch_host", "-fsanitize=address,undefined", "-Xarch_host", "-fno-sanitize-recover=undefined", src, "-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, f"compile failed:\n{r.stdout}\n{r.stderr}"
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    return r


def test_wa_block_host_header(check_output):
    r = check_output
    print("\n".join(l for l in r.stdout.splitlines() if not l.startswith(("table ", "hash "))))
    assert r.returncode == 0, f"wa_block_host_check failed ({r.returncode}):\n{r.stdout[-4000:]}\n{r.stderr[-4000:]}"
    assert "wa_block_host: ok" in r.stdout


def test_the_bytes_are_the_ones_built_before_the_block_moved(check_output):
    with open(os.path.join(ROOT, "tests", "golden", "wa_block_host.json")) as f:
        want = json.load(f)
    tables, hashes = {}, {}
    for line in check_output.stdout.splitlines():
        w = line.split()
        if w[:1] == ["table"]:
            tables[w[1]] = {"stride": int(w[2]), "words": w[3]}
        elif w[:1] == ["hash"]:
            hashes.setdefault(w[1], {})[w[2]] = w[3]
    assert sorted(want["tables"]) == sorted(CASES) and sorted(tables) == sorted(CASES)
    for case, stride in CASES.items():
        assert want["tables"][case]["stride"] == stride and len(want["tables"][case]["words"]) == 8 * stride * stride, case
        assert tables[case] == want["tables"][case], case
    blocks = [c for c in CASES if c.startswith("w")]
    assert sorted(want["hashes"]) == sorted(blocks) and sorted(hashes) == sorted(blocks)
    for case in blocks:
        assert sorted(want["hashes"][case]) == sorted(ARRAYS), case
        assert hashes[case] == want["hashes"][case], case
