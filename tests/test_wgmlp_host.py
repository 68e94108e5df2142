"""The host half of the wgmlp engine (nunif_amd/csrc/wgmlp_host.h: accepted shapes, window counts, launch size, LDS map, workspace
layout, packed-weight index) checked on the CPU under the host address and undefined-behaviour sanitizers by the stand-alone program
tests/cpp/wgmlp_host_check.cpp, like the other ``*_host_check.cpp``.  The program is a child process of its own; nothing is loaded
into this interpreter."""
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from nunif_amd import build  # noqa: E402


def test_wgmlp_host_header(tmp_path):
    try:
        hipcc = build.hipcc()
    except RuntimeError:
        pytest.skip("hipcc not available")
    exe = str(tmp_path / "wgmlp_host_check")
    src = os.path.join(ROOT, "tests", "cpp", "wgmlp_host_check.cpp")
    cmd = [hipcc, "-O1", "-g", "-std=c++17", f"--offload-arch={build.ARCH}", "-x", "hip", "-Wall", "-Wno-unused-function",
           "-Xarch_host", "-fsanitize=address,undefined", "-Xarch_host", "-fno-sanitize-recover=undefined", src, "-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, f"compile failed:\n{r.stdout}\n{r.stderr}"
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, f"wgmlp_host_check failed ({r.returncode}):\n{r.stdout[-4000:]}\n{r.stderr[-4000:]}"
    assert "wgmlp_host: ok" in r.stdout
