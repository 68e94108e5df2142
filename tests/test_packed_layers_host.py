"""The packed Linear / conv layers of the fp16 engines (nunif_amd/csrc/packed_layers.h) checked on the CPU:
tests/cpp/packed_layers_check.cpp states each packing by its inverse, compares every argument builder field by field with a
value-initialised struct and checks the per-slice structs of the sliced conv launcher.  It is built with the host sanitizers, so
every index expression of the header runs under their bounds checking.  The program is a child process of its own; nothing is
loaded into this interpreter and nothing is launched."""
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from nunif_amd import build  # noqa: E402


def test_packed_layers_host(tmp_path):
    try:
        hipcc = build.hipcc()
    except RuntimeError:
        pytest.skip("hipcc not available")
    exe = str(tmp_path / "packed_layers_check")
    src = os.path.join(ROOT, "tests", "cpp", "packed_layers_check.cpp")
    cmd = [hipcc, "-O1", "-g", "-std=c++17", f"--offload-arch={build.ARCH}", "-x", "hip", "-Wall", "-Wno-unused-function",
           "-Xarch_host", "-fsanitize=address,undefined", "-Xarch_host", "-fno-sanitize-recover=undefined", src, "-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, f"compile failed:\n{r.stdout}\n{r.stderr}"
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    print(r.stdout)
    assert r.returncode == 0, f"packed_layers_check failed ({r.returncode}):\n{r.stdout}\n{r.stderr}"
    assert "packed_layers: ok" in r.stdout
