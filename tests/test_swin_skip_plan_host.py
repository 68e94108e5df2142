"""The plan builder of a swin_unet frame render (nunif_amd/csrc/swin_skip_plan_host.h: extents, window lists, group tables, producer
lists and their layout in one upload) checked on the CPU under the host sanitizers: tests/cpp/swin_skip_plan_host_check.cpp compares
every piece with a brute force or a direct call of its own builder, and prints a record of the plans of two frames, which must be the
words the library uploaded before the builder moved into the header (tests/golden/swin_skip_plan_words.json, recorded from that build).
The program is a child process of its own; nothing is loaded into this interpreter."""
import json
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from nunif_amd import build  # noqa: E402


@pytest.fixture(scope="module")
def check_output(tmp_path_factory):
    try:
        hipcc = build.hipcc()
    except RuntimeError:
        pytest.skip("hipcc not available")
    exe = str(tmp_path_factory.mktemp("skip_plan") / "swin_skip_plan_host_check")
    src = os.path.join(ROOT, "tests", "cpp", "swin_skip_plan_host_check.cpp")
    cmd = [hipcc, "-O1", "-g", "-std=c++17", f"--offload-arch={build.ARCH}", "-x", "hip", "-Wall", "-Wno-unused-function",
           "-Xarch_host", "-fsanitize=address,undefined", "-Xarch_host", "-fno-sanitize-recover=undefined", src, "-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, f"compile failed:\n{r.stdout}\n{r.stderr}"
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    return r


def test_swin_skip_plan_host_header(check_output):
    r = check_output
    print("\n".join(l for l in r.stdout.splitlines() if not l.startswith("plan ")))
    assert r.returncode == 0, f"swin_skip_plan_host_check failed ({r.returncode}):\n{r.stdout[-4000:]}\n{r.stderr[-4000:]}"
    assert "swin_skip_plan_host: ok" in r.stdout


def test_the_words_are_the_ones_uploaded_before_the_builder_moved(check_output):
    key = lambda p: tuple(p[k] for k in ("tile", "h", "w", "scale", "tile_begin", "B", "level"))  # noqa: E731
    with open(os.path.join(ROOT, "tests", "golden", "swin_skip_plan_words.json")) as f:
        want = {key(p): p for p in json.load(f)["plans"]}
    got = {key(p): p for p in (json.loads(l[5:]) for l in check_output.stdout.splitlines() if l.startswith("plan "))}
    assert len(want) == 12 and sorted(got) == sorted(want)
    for k in sorted(want):
        assert got[k] == want[k], k
