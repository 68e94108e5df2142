"""The host-side weight layout (nunif_amd/csrc/host_weights.h) checked on the CPU: tests/cpp/host_weights_check.cpp states the
MFMA fragment layout by its inverse and is built with the host sanitizers, so every index expression of the header runs under
their bounds checking.  The program is a child process of its own; nothing is loaded into this interpreter."""
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from nunif_amd import build  # noqa: E402


def test_host_weights_layout(tmp_path):
    try:
        hipcc = build.hipcc()
    except RuntimeError:
        pytest.skip("hipcc not available")
    exe = str(tmp_path / "host_weights_check")
    src = os.path.join(ROOT, "tests", "cpp", "host_weights_check.cpp")
    cmd = [hipcc, "-O1", "-g", "-std=c++17", f"--offload-arch={build.ARCH}", "-x", "hip", "-Wall", "-Wno-unused-function",
           "-Xarch_host", "-fsanitize=address,undefined", "-Xarch_host", "-fno-sanitize-recover=undefined", src, "-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, f"compile failed:\n{r.stdout}\n{r.stderr}"
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    print(r.stdout)
    assert r.returncode == 0, f"host_weights_check failed ({r.returncode}):\n{r.stdout}\n{r.stderr}"
    assert "host_weights: ok" in r.stdout
