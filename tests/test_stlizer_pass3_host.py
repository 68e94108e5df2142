"""The host-only workspace layout of stlizer pass 3 (nunif_amd/csrc/stlizer_pass3_host.h) checked on the CPU:
tests/cpp/stlizer_pass3_host_check.cpp walks the regions at N = 1, 257 and 1 048 576 (aligned, disjoint, as large as the kernels
reach, ending at workspace_bytes), built with the host address and undefined-behaviour sanitizers.  The program is a child process
of its own; nothing is loaded into this interpreter."""
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from nunif_amd import build  # noqa: E402


def test_stlizer_pass3_host_layout(tmp_path):
    try:
        hipcc = build.hipcc()
    except RuntimeError:
        pytest.skip("hipcc not available")
    exe = str(tmp_path / "stlizer_pass3_host_check")
    src = os.path.join(ROOT, "tests", "cpp", "stlizer_pass3_host_check.cpp")
    cmd = [hipcc, "-O1", "-g", "-std=c++17", f"--offload-arch={build.ARCH}", "-x", "hip", "-Wall", "-Wno-unused-function",
           "-Xarch_host", "-fsanitize=address,undefined", "-Xarch_host", "-fno-sanitize-recover=undefined", src, "-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, f"compile failed:\n{r.stdout}\n{r.stderr}"
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    print(r.stdout)
    assert r.returncode == 0, f"stlizer_pass3_host_check failed ({r.returncode}):\n{r.stdout}\n{r.stderr}"
    assert "stlizer_pass3_host: ok" in r.stdout


def test_python_layout_constants_match_the_header():
    from nunif_amd.stlizer import pass3 as P
    text = open(os.path.join(ROOT, "nunif_amd", "csrc", "stlizer_pass3_host.h")).read()
    assert f"kRecDoubles = {P.REC_DOUBLES};" in text and f"kMaxTaps = {P.MAX_TAPS};" in text
    assert f"kMaxIteration = {P.MAX_ITERATION};" in text and "kMaxN = 1 << 20;" in text and P.MAX_FRAMES == 1 << 20
    fields = text[text.index("enum Rec {"):text.index("R_END")]
    order = [w.strip().lower()[2:] for w in __import__("re").findall(r"R_[A-Z_]+", fields)]
    assert order == list(P.REC) and order[-1] == "al"
