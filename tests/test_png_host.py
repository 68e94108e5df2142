"""The host-only part of the PNG encoder (nunif_amd/csrc/png_host.h) checked on the CPU: tests/cpp/png_host_check.cpp runs the
header writer, the CRC table and the powers of x that combine piecewise CRCs against known vectors, and the bound and workspace
arithmetic at H, W in {1, 2, 17, 8192} and stripe_rows in {1, 16, H}, built with the host sanitizers so that every index
expression of the header runs under their bounds checking.  The program is a child process of its own; nothing is loaded into
this interpreter."""
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from nunif_amd import build  # noqa: E402


def test_png_host_header(tmp_path):
    try:
        hipcc = build.hipcc()
    except RuntimeError:
        pytest.skip("hipcc not available")
    exe = str(tmp_path / "png_host_check")
    src = os.path.join(ROOT, "tests", "cpp", "png_host_check.cpp")
    cmd = [hipcc, "-O1", "-g", "-std=c++17", f"--offload-arch={build.ARCH}", "-x", "hip", "-Wall", "-Wno-unused-function",
           "-Xarch_host", "-fsanitize=address,undefined", "-Xarch_host", "-fno-sanitize-recover=undefined", src, "-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, f"compile failed:\n{r.stdout}\n{r.stderr}"
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    print(r.stdout)
    assert r.returncode == 0, f"png_host_check failed ({r.returncode}):\n{r.stdout}\n{r.stderr}"
    assert "png_host: ok" in r.stdout
