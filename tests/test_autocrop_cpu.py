"""--autocrop without a GPU: the float64 restatement (tests/autocrop_f64.py) reproduces the masks and slices that the reference
classes recorded in tests/golden/autocrop.npz, its fp32 run reproduces the recorded statistics, every statistic of every shared
input keeps 0.01 from its threshold, and the engine module's host arithmetic and signatures equal the live reference's."""
import inspect
import os
import random

import numpy as np
import pytest
import torch

import autocrop_cases as C
import autocrop_f64 as R
from conftest import GOLDEN
from oracle import refstub


@pytest.fixture(scope="module")
def golden():
    return dict(np.load(os.path.join(GOLDEN, "autocrop.npz")))


@pytest.fixture(scope="module")
def f64_stats():
    return {kind: {name: R.stats(x, kind) for name, x in C.all_inputs(kind).items()} for kind in C.KINDS}


def test_every_statistic_keeps_its_margin(f64_stats):
    for kind in C.KINDS:
        for name, st in f64_stats[kind].items():
            assert R.margin(st, kind) >= C.MARGIN, (kind, name, R.margin(st, kind))


def test_restatement_reproduces_the_recorded_masks_and_slices(golden, f64_stats):
    for kind in C.KINDS:
        for name in list(C.CASES) + ["batch"]:
            m = R.masks(f64_stats[kind][name], kind)
            for key in ("tb", "lr"):
                want = golden[f"{name}/{kind}/mask_{key}"].astype(bool)
                assert np.array_equal(m[key].numpy().reshape(want.shape), want), (kind, name, key)
    for mode in C.MODES:
        kind = mode.split("_")[0]
        for mod in C.MODS:
            for name in C.CASES:
                m = R.masks(f64_stats[kind][name], kind)
                sh, sw = R.slices(m["tb"][0], m["lr"][0], mode, mod)
                assert C.enc_slice(sh) + C.enc_slice(sw) == golden[f"{name}/{mode}/{mod}/slices"].tolist(), (name, mode, mod)


def test_sequence_counts_and_crop(golden, f64_stats):
    """19 of 20 frames carry the bars: in fp32, 19 / 20 >= 0.95 holds and the bars of the single frame come back."""
    for kind in C.KINDS:
        m = R.masks(f64_stats[kind]["seq"], kind)
        assert np.array_equal(m["tb"].sum(0).numpy(), golden[f"seq/{kind}/count_tb"])
        assert np.array_equal(m["lr"].sum(0).numpy(), golden[f"seq/{kind}/count_lr"])
        assert golden[f"seq/{kind}/count_tb"].max() == C.SEQ_FRAMES - 1
        for mod in C.MODS:
            assert golden[f"seq/{kind}/{mod}/slices"].tolist() == golden[f"s37x67/{kind}/{mod}/slices"].tolist()


def test_fp32_restatement_reproduces_the_recorded_statistics(golden):
    for kind in C.KINDS:
        for name, x in C.all_inputs(kind).items():
            for k, v in R.stats(x, kind, torch.float32).items():
                assert np.array_equal(v.numpy(), golden[f"{name}/{kind}/{k}"]), (kind, name, k)


def test_special_frames_give_no_crop(golden):
    for name in ("all_bar", "no_bar", "s1x1"):
        for mode in C.MODES:
            assert golden[f"{name}/{mode}/2/slices"].tolist() == [-1, -1, -1, -1]
            assert golden[f"{name}/{mode}/2/crop"].tolist() == [-1, -1, -1, -1]


def test_analyze_video_without_pyav_says_so():
    import importlib.util
    if importlib.util.find_spec("av") is not None:
        pytest.skip("PyAV is installed here")
    from nunif_amd.nunif.utils.autocrop import autocrop_analyze_video
    with pytest.raises(RuntimeError, match="PyAV"):
        autocrop_analyze_video("nothing.mp4")


def test_input_checks_need_no_device():
    from nunif_amd.nunif.utils.autocrop import AutoCropDetector
    with pytest.raises(ValueError):
        AutoCropDetector("black").update(_Fake((1, 8, 8)))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        AutoCropDetector.detect(torch.zeros(3, 8, 8))


class _Fake:
    """Shape-only stand-in for a device tensor: the channel check comes before any device work."""
    def __init__(self, shape):
        self.shape, self.ndim = shape, len(shape)
        self.device = torch.device("cuda:0")

    def unsqueeze(self, d):
        return _Fake((1,) + tuple(self.shape))


needs_reference = pytest.mark.skipif(not refstub.reference_available(), reason="the reference checkout is not mounted here")


@needs_reference
def test_host_helpers_equal_the_live_reference():
    refstub.install()
    import nunif.utils.autocrop as ref
    import nunif_amd.nunif.utils.autocrop as ours
    rng = random.Random(5)
    for _ in range(300):
        H, W = rng.randint(1, 64), rng.randint(1, 64)

        def rand_slice(n):
            a = rng.choice([None] + list(range(0, n + 1)))
            b = rng.choice([None] + list(range(0, n + 1)))
            return slice(a, b)

        sh, sw, mod = rand_slice(H), rand_slice(W), rng.choice([1, 2, 4, 8])
        assert ours.AutoCropDetector.apply_mod(sh, mod) == ref.AutoCropDetector.apply_mod(sh, mod)
        assert ours.AutoCrop.calc_pad(sh, sw, H, W) == ref.AutoCrop.calc_pad(sh, sw, H, W)
        assert ours.AutoCrop.calc_crop(sh, sw, H, W) == ref.AutoCrop.calc_crop(sh, sw, H, W)
        g = torch.Generator().manual_seed(rng.randint(0, 1 << 30))
        kind = rng.choice(["rand", "bars", "all", "none"])
        mask = {"rand": torch.rand(H, generator=g) < 0.5, "all": torch.ones(H, dtype=torch.bool),
                "none": torch.zeros(H, dtype=torch.bool)}.get(kind)
        if mask is None:
            mask = torch.zeros(H, dtype=torch.bool)
            mask[:rng.randint(0, H)] = True
            mask[H - rng.randint(0, H):] = True
        assert ours.AutoCropDetector.mask_to_slice_tb(mask.view(1, H, 1)) == ref.AutoCropDetector.mask_to_slice_tb(mask.view(1, H, 1))
        assert ours.AutoCropDetector.mask_to_slice_lr(mask.view(1, 1, H)) == ref.AutoCropDetector.mask_to_slice_lr(mask.view(1, 1, H))
        assert R.mask_to_slice(mask) == ref.AutoCropDetector.mask_to_slice_tb(mask.view(1, H, 1))


@needs_reference
def test_signatures_equal_the_live_reference():
    refstub.install()
    import nunif.utils.autocrop as ref
    import nunif_amd.nunif.utils.autocrop as ours
    assert inspect.signature(ours.autocrop_analyze_video) == inspect.signature(ref.autocrop_analyze_video)
    for cls, names in (("AutoCropDetector", ("__init__", "reset", "update", "get_crop", "detect", "apply_mod", "mask_to_slice_tb",
                                             "mask_to_slice_lr", "detect_tb", "detect_lr")),
                       ("AutoCrop", ("__init__", "get_slice", "get_pad", "get_crop", "calc_pad", "calc_crop", "from_image",
                                     "from_video_file", "crop", "uncrop")),
                       ("AutoCropDummy", ("__init__", "crop", "uncrop"))):
        for name in names:
            assert inspect.signature(getattr(getattr(ours, cls), name)) == inspect.signature(getattr(getattr(ref, cls), name)), \
                (cls, name)


def test_abi_symbols_are_declared_exported_and_bound(hiplib):
    from nunif_amd import _hip
    header = open(os.path.join(os.path.dirname(GOLDEN), "..", "include", "nunif_hip.h")).read()
    for s in ("nunif_hip_autocrop_stats", "nunif_hip_autocrop_debug_stats", "nunif_hip_autocrop_crop_pad"):
        assert s + "(" in header and s in _hip.SIGNATURES and hasattr(hiplib, s)
