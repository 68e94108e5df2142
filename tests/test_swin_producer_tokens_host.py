"""The producer-table builder of a swin_unet frame render (nunif_amd/csrc/swin_producer_tokens_host.h) checked on the CPU under the host
sanitizers: tests/cpp/swin_producer_tokens_host_check.cpp builds every producer's table for sides 48 .. 240 into exactly sized heap
buffers.  The program is a child process of its own; nothing is loaded into this interpreter."""
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from nunif_amd import build  # noqa: E402


def test_swin_producer_tokens_host_header(tmp_path):
    try:
        hipcc = build.hipcc()
    except RuntimeError:
        pytest.skip("hipcc not available")
    exe = str(tmp_path / "swin_producer_tokens_host_check")
    src = os.path.join(ROOT, "tests", "cpp", "swin_producer_tokens_host_check.cpp")
    cmd = [hipcc, "-O1", "-g", "-std=c++17", f"--offload-arch={build.ARCH}", "-x", "hip", "-Wall", "-Wno-unused-function",
           "-Xarch_host", "-fsanitize=address,undefined", "-Xarch_host", "-fno-sanitize-recover=undefined", src, "-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, f"compile failed:\n{r.stdout}\n{r.stderr}"
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    print(r.stdout)
    assert r.returncode == 0, f"swin_producer_tokens_host_check failed ({r.returncode}):\n{r.stdout}\n{r.stderr}"
    assert "swin_producer_tokens_host: ok" in r.stdout
