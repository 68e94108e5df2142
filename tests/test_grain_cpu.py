"""Film grain, the parts that need no GPU: the new C-ABI entries are declared, exported and bound; the Python layer keeps the
reference's signatures (``nunif/utils/rgb_noise.py:5,21``, ``waifu2x/ui_utils.py:104``) and refuses CPU tensors; and the
arithmetic of tests/grain_ref.py — the float64 restatement, torch's nearest index rule, the moment statistics and their
standard errors — is proven on ``torch.randn`` and on the reference's recorded results (tests/golden/rgb_noise.npz, written by
tests/golden/make_golden_grain.py) before tests/test_gpu_grain.py applies it to the engine."""
import inspect
import os
import re

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import grain_ref as G
from conftest import GOLDEN, ROOT

NEW_SYMBOLS = ["nunif_hip_rgb_noise", "nunif_hip_apply_rgb_noise", "nunif_hip_grain_blend", "nunif_hip_grain_video_step",
               "nunif_hip_frame_to_tensor_rot"]
APPLY_CASES = {"s01": (0.1, 2.2, True), "s02": (0.2, 2.2, True), "s10": (1.0, 2.2, True),
               "s01_flat": (0.1, 2.2, False), "s02_flat": (0.2, 2.2, False), "s10_flat": (1.0, 2.2, False),
               "s02_g18": (0.2, 1.8, True)}


@pytest.fixture(scope="module")
def golden():
    return dict(np.load(os.path.join(GOLDEN, "rgb_noise.npz")))


def test_new_abi_entries_are_declared_exported_and_bound(hiplib):
    from nunif_amd import _hip
    header = open(os.path.join(ROOT, "include", "nunif_hip.h")).read()
    header = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    for s in NEW_SYMBOLS:
        assert re.search(rf"\b{s}\s*\(", header), f"{s} is not declared in nunif_hip.h"
        assert s in _hip.SIGNATURES, f"{s} has no ctypes signature"
        assert hasattr(hiplib, s), f"{s} is not exported by the library"


def test_python_signatures_are_the_references():
    from nunif_amd.nunif.utils import rgb_noise as R
    from nunif_amd.waifu2x import ui_utils as U
    assert str(inspect.signature(R.rgb_noise_like)) == "(base, level=2)"
    assert str(inspect.signature(R.apply_rgb_noise)) == \
        "(rgb, noise, strength=0.2, gamma=2.2, light_decay=True, light_decay_strength=0.8)"
    assert str(inspect.signature(U.process_video)) == "(ctx, input_filename, output_path, args)"


def test_cpu_tensors_raise():
    from nunif_amd.nunif.utils import rgb_noise as R
    from nunif_amd.waifu2x.video import Waifu2xVideoStream
    x = torch.rand(3, 8, 8)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        R.rgb_noise_like(x)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        R.apply_rgb_noise(x, x)
    with pytest.raises(RuntimeError, match="no CPU"):
        R.generate((3, 8, 8), "cpu")
    with pytest.raises(RuntimeError, match="no CPU"):
        Waifu2xVideoStream(None, None, device="cpu")


def test_process_video_needs_an_installed_reference():
    import nunif_amd.install as inst
    from nunif_amd.waifu2x import ui_utils as U
    if inst.is_installed():
        inst.uninstall()
    with pytest.raises(RuntimeError, match="install"):
        U.process_video(None, "in.mp4", "out.mp4", None)


@pytest.mark.parametrize("out_size,in_size", [(101, 50), (67, 33), (1024, 512), (7, 3), (3841, 1920), (2161, 1080)])
def test_nearest_index_rule_is_torchs(out_size, in_size):
    grid = torch.arange(in_size, dtype=torch.float32).view(1, 1, 1, in_size)
    up = F.interpolate(grid, size=(1, out_size), mode="nearest").view(-1).numpy().astype(np.int64)
    assert np.array_equal(up, G.nearest_index(out_size, in_size))


@pytest.mark.parametrize("level", [1, 2])
def test_moment_checks_hold_on_torch_randn(level):
    """The statistics and standard errors of grain_ref.moments on a generator known to be right."""
    g = torch.Generator().manual_seed(1234 + level)
    noise, n1, n2 = G.rgb_noise_like_torch((3, 1024, 1024), level, g, parts=True)
    print(f"level {level}:")
    assert not G.check_moments(G.moments(noise, level))
    other = G.rgb_noise_like_torch((3, 1024, 1024), level, g)
    assert not G.check_moments({"channels_0_1": G.cross_moment(noise[0], noise[1], level),
                                "two_draws": G.cross_moment(noise, other, level)})
    if level == 2:
        assert not G.check_moments({"kurtosis_grid": G.moments(n2, 1)["excess_kurtosis"]})


def test_moment_checks_reject_a_wrong_field():
    """A field with the wrong cell structure or a repeated channel must fail: the checks have teeth."""
    g = torch.Generator().manual_seed(7)
    n1 = torch.randn(3, 256, 256, generator=g)
    assert G.check_moments(G.moments(n1 * math_sqrt_half(), 2))                    # right variance, no 2x2 cells
    assert G.check_moments({"same": G.cross_moment(n1[0], n1[0] * 0.1 + n1[1], 1)})


def math_sqrt_half():
    return 0.5 ** 0.5


def test_fixture_holds_what_the_tests_need(golden):
    x = golden["x3"]
    assert x.shape == (3, 48, 80) and x.dtype == np.float32
    assert (x == 0).any() and (x == 1).any() and ((x > 0) & (x < 0.02)).sum() > 1000
    assert golden["x4"].shape == (2, 3, 24, 40) and golden["video_noise"].shape == (3, 3, 24, 40)
    assert os.path.getsize(os.path.join(GOLDEN, "rgb_noise.npz")) < 1 << 20


def test_float64_restatement_agrees_with_the_recorded_reference(golden):
    """The reference's fp32 results against apply64: the linear-domain error is fp32 rounding (the issue quotes 1.3e-7 on a larger
    input of the same kind), and the recorded one-step shares are reproduced."""
    for name, (s, gm, ld) in APPLY_CASES.items():
        ref64 = G.apply64(golden["x3"], golden["noise3"], s, gm, ld)
        y = golden[f"apply_{name}"]
        lin = np.abs(y.astype(np.float64) ** gm - ref64 ** gm).max()
        s8, s16 = G.step_shares(G.quantise(y, 8), G.quantise(ref64, 8)), G.step_shares(G.quantise(y, 16), G.quantise(ref64, 16))
        print(f"{name}: reference fp32 vs float64: linear {lin:.3g}  output {np.abs(y - ref64).max():.3g}  8 bit {s8}  16 bit {s16}")
        assert lin < 5e-7
        assert np.allclose(golden[f"shares_{name}"], [*s8, *s16])
        assert s8[1] <= 1 and s8[0] <= 1e-3 and s16[1] <= 1
    y4 = G.apply64(golden["x4"], golden["noise4"], 0.2)
    assert np.abs(golden["apply4_s02"] ** 2.2 - y4 ** 2.2).max() < 5e-7


@pytest.mark.parametrize("name,speed", [("v08", 0.8), ("v03", 0.3)])
def test_blend_restatement_agrees_with_the_recorded_reference(golden, name, speed):
    buf32, buf64 = None, None
    for i in range(3):
        buf32 = G.blend32(buf32, golden["video_noise"][i], speed)
        buf64 = G.blend64(buf64, golden["video_noise"][i], speed)
        assert np.array_equal(buf32, golden[f"video_buf_{name}"][i]), i       # the fp32 recurrence, bit for bit
        assert np.abs(buf64 - golden[f"video_buf_{name}"][i]).max() < 1e-6
        y = G.apply64(golden["video_x"][i], buf64, 0.2)
        assert np.abs(golden[f"video_out_{name}"][i].astype(np.float64) ** 2.2 - y ** 2.2).max() < 1e-6
