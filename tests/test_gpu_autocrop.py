"""--autocrop on the HIP engine (nunif_amd/csrc/autocrop.hip, nunif_amd/nunif/utils/autocrop.py) against the float64 restatement
(tests/autocrop_f64.py) and what the reference classes recorded in tests/golden/autocrop.npz.

Statistics: every vector of the debug entry against float64 with the recorded fp32 run as the yardstick,
``e_hip <= 2.2 * e_ref + 2^-23`` for the largest error of a vector (the worst ratios: profiles/autocrop.txt).  Every statistic of
every input keeps 0.01 from its threshold (tests/test_autocrop_cpu.py), so masks, slices, pads and crops are compared with
equality.  ``crop`` / ``uncrop`` are copies and ``process_image_autocrop`` of a padded frame is ``process_image`` of the frame:
``torch.equal``."""
import os
from types import SimpleNamespace

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import autocrop_cases as C
import autocrop_f64 as R
from conftest import GOLDEN, synth_image

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


@pytest.fixture(scope="module")
def golden():
    return dict(np.load(os.path.join(GOLDEN, "autocrop.npz")))


@pytest.fixture(scope="module")
def inputs():
    return {kind: C.all_inputs(kind) for kind in C.KINDS}


@pytest.fixture(scope="module")
def A(hiplib):
    import nunif_amd.nunif.utils.autocrop as mod
    return mod


def enc(slices):
    return C.enc_slice(slices[0]) + C.enc_slice(slices[1])


@pytest.mark.parametrize("kind", C.KINDS)
def test_statistics_against_float64(A, golden, inputs, kind):
    worst = {k: 0.0 for k in C.STAT_KEYS}
    for name, x in inputs[kind].items():
        got = {k: v.cpu() for k, v in A.debug_stats(x.to(DEV), black_only=kind == "black").items()}
        ratios = C.error_ratios(got, R.stats(x, kind), {k: golden[f"{name}/{kind}/{k}"] for k in C.STAT_KEYS})
        for k, (ratio, e_hip, e_ref) in ratios.items():
            print(f"{kind} {name} {k}: e_hip {e_hip:.3e} e_ref {e_ref:.3e} ratio {ratio:.3f}")
            worst[k] = max(worst[k], ratio)
        # the counters of the same call are the sums of the decisions the statistics imply
        m = R.masks({k: got[k].double() for k in C.STAT_KEYS}, kind)
        assert torch.equal(got["count_tb"].long(), m["tb"].sum(0)) and torch.equal(got["count_lr"].long(), m["lr"].sum(0)), name
    print(kind, "worst ratios", worst)
    assert max(worst.values()) <= 1.0, worst


@pytest.mark.parametrize("kind", C.KINDS)
def test_masks_equal_the_reference(A, golden, inputs, kind):
    black = kind == "black"
    for name in C.CASES:
        x = inputs[kind][name][0].to(DEV)
        tb, lr = A.AutoCropDetector.detect_tb(x, black_only=black), A.AutoCropDetector.detect_lr(x, black_only=black)
        H, W = x.shape[-2:]
        assert tb.shape == (1, H, 1) and lr.shape == (1, 1, W) and tb.dtype == torch.bool and lr.dtype == torch.bool
        assert np.array_equal(tb.flatten().cpu().numpy(), golden[f"{name}/{kind}/mask_tb"].astype(bool)), name
        assert np.array_equal(lr.flatten().cpu().numpy(), golden[f"{name}/{kind}/mask_lr"].astype(bool)), name
    xb = inputs[kind]["batch"].to(DEV)
    tb, lr = A.AutoCropDetector.detect_tb(xb, black_only=black), A.AutoCropDetector.detect_lr(xb, black_only=black)
    assert tb.shape == (3, 1, 48, 1) and lr.shape == (3, 1, 1, 84)
    assert np.array_equal(tb.flatten(1).cpu().numpy(), golden[f"batch/{kind}/mask_tb"].astype(bool))
    assert np.array_equal(lr.flatten(1).cpu().numpy(), golden[f"batch/{kind}/mask_lr"].astype(bool))


@pytest.mark.parametrize("mode", C.MODES)
def test_slices_pads_and_crops_equal_the_reference(A, golden, inputs, mode):
    kind = mode.split("_")[0]
    for name in C.CASES:
        x = inputs[kind][name][0].to(DEV)
        for mod in C.MODS:
            key = f"{name}/{mode}/{mod}"
            assert enc(A.AutoCropDetector.detect(x, mode=mode, mod=mod)) == golden[key + "/slices"].tolist(), key
            det = A.AutoCropDetector(mode=mode, mod=mod)
            det.update(x)
            assert enc(det.get_crop()) == golden[key + "/slices"].tolist(), key
            ac = A.AutoCrop.from_image(x.unsqueeze(0) if mod == 2 else x, mode=mode.upper(), mod=mod)
            assert enc(ac.get_slice()) == golden[key + "/slices"].tolist(), key
            assert list(ac.get_pad()) == golden[key + "/pad"].tolist(), key
            assert list(ac.get_crop() or (-1, -1, -1, -1)) == golden[key + "/crop"].tolist(), key


@pytest.mark.parametrize("kind", C.KINDS)
def test_update_batch_frames_reset_and_the_sequence(A, golden, inputs, kind):
    xb = inputs[kind]["batch"].to(DEV)
    whole, single = A.AutoCropDetector(mode=kind, mod=1), A.AutoCropDetector(mode=kind, mod=1)
    whole.update(xb)
    for f in xb:
        single.update(f)
    assert whole.frame_count == single.frame_count == 3
    assert whole.border_count_tb.shape == (1, 48, 1) and whole.border_count_lr.shape == (1, 1, 84)
    assert whole.border_count_tb.dtype == torch.int32
    assert torch.equal(whole.border_count_tb, single.border_count_tb) and torch.equal(whole.border_count_lr, single.border_count_lr)
    assert np.array_equal(whole.border_count_tb.flatten().cpu().numpy(), golden[f"batch/{kind}/mask_tb"].sum(0))
    assert np.array_equal(whole.border_count_lr.flatten().cpu().numpy(), golden[f"batch/{kind}/mask_lr"].sum(0))
    whole.reset()
    assert whole.border_count_tb is None and whole.border_count_lr is None and whole.frame_count == 0
    assert whole.get_crop() == (slice(None), slice(None))
    # a *_tb mode keeps no column counter
    tb_only = A.AutoCropDetector(mode=kind + "_tb")
    tb_only.update(xb)
    assert tb_only.border_count_lr is None and torch.equal(tb_only.border_count_tb, single.border_count_tb)

    seq = inputs[kind]["seq"].to(DEV)
    for mode in (kind, kind + "_tb", kind + "_lr"):
        for mod in C.MODS:
            det = A.AutoCropDetector(mode=mode, mod=mod)
            det.update(seq[:7])
            det.update(seq[7:9].half())                       # another float dtype is converted
            for f in seq[9:]:
                det.update(f)
            assert det.frame_count == C.SEQ_FRAMES
            assert enc(det.get_crop()) == golden[f"seq/{mode}/{mod}/slices"].tolist(), (mode, mod)
            if mode == kind:
                assert np.array_equal(det.border_count_tb.flatten().cpu().numpy(), golden[f"seq/{kind}/count_tb"])
                assert np.array_equal(det.border_count_lr.flatten().cpu().numpy(), golden[f"seq/{kind}/count_lr"])
                # one frame in twenty differs: a stricter threshold drops the bars
                assert det.get_crop(frame_variation_threshold=0.96) == (slice(None), slice(None))


def test_non_contiguous_input_and_refusals(A, inputs):
    x = inputs["black"]["s37x67"][0].to(DEV)
    want = A.AutoCropDetector.detect(x, mode="black", mod=1)
    hwc = x.permute(1, 2, 0).contiguous()
    assert A.AutoCropDetector.detect(hwc.permute(2, 0, 1), mode="black", mod=1) == want
    with pytest.raises(ValueError):
        A.AutoCropDetector("black").update(x[:1])
    with pytest.raises(ValueError):
        A.AutoCropDetector("black").update(torch.zeros(2, 4, 8, 8, device=DEV))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        A.AutoCropDetector("black").update(x.cpu())
    from nunif_amd._hip import NunifHipError
    with pytest.raises(NunifHipError, match="exceeds the built tiling"):
        A.AutoCropDetector("black").update(torch.zeros(3, 2, A.MAX_W + 4, device=DEV))
    with pytest.raises(NunifHipError, match="exceeds the built tiling"):
        A.AutoCropDetector("flat").update(torch.zeros(3, A.MAX_H + 1, 2, device=DEV))


@pytest.mark.parametrize("kind", C.KINDS)
def test_the_largest_supported_frames_run(A, kind):
    """H = 4608 and W = 8192 are the limits the flat tiling sets (155 776 and 135 168 bytes of LDS per workgroup): one narrow
    frame at each, statistics and decisions against the float64 restatement under the same bound (yardstick: its fp32 run)."""
    for H, W, bars in ((A.MAX_H, 8, (9, 0, 4, 0)), (4, A.MAX_W, (1, 0, 0, 12))):
        x = C.make_frame(kind, H, W, *bars, seed=60).unsqueeze(0)
        f64 = R.stats(x, kind)
        assert R.margin(f64, kind) >= C.MARGIN
        got = {k: v.cpu() for k, v in A.debug_stats(x.to(DEV), black_only=kind == "black").items()}
        ratios = C.error_ratios(got, f64, R.stats(x, kind, torch.float32))
        print(kind, H, W, {k: round(v[0], 3) for k, v in ratios.items()})
        assert max(v[0] for v in ratios.values()) <= 1.0, (H, W, ratios)
        m = R.masks(f64, kind)
        assert torch.equal(got["count_tb"].bool(), m["tb"][0]) and torch.equal(got["count_lr"].bool(), m["lr"][0]), (H, W)
        assert int(m["tb"].sum()) >= bars[0] and int(m["lr"].sum()) >= bars[2] + bars[3]


@pytest.mark.parametrize("kind", C.KINDS)
def test_results_are_bit_identical_from_call_to_call_and_across_streams(A, inputs, kind):
    black = kind == "black"
    for name in ("s130x259", "s1100x40", "s10x1032", "batch"):
        x = inputs[kind][name].to(DEV)
        first = A.debug_stats(x, black_only=black)
        again = A.debug_stats(x, black_only=black)
        torch.cuda.synchronize()
        streams = [torch.cuda.Stream(device=DEV) for _ in range(2)]
        outs = []
        for s in streams:
            with torch.cuda.stream(s):
                outs.append(A.debug_stats(x, black_only=black))
        torch.cuda.synchronize()
        for other in [again] + outs:
            for k, v in first.items():
                assert torch.equal(v.view(torch.int32), other[k].view(torch.int32)), (name, k)


CROPS = [  # H, W, slice_h, slice_w
    (37, 67, slice(5, 34), slice(7, None)),               # odd offsets, scalar stores
    (40, 64, slice(None, 31), slice(4, 60)),              # 16-byte loads and stores; touches the top
    (40, 64, slice(3, None), slice(None, None)),          # touches bottom, left and right
    (40, 64, slice(2, 38), slice(3, 63)),                 # aligned stores, unaligned loads
    (16, 24, slice(None), slice(1, 21)),
    (9, 6, slice(8, None), slice(None, 1)),               # one pixel
    (12, 1032, slice(1, 11), slice(8, 1028)),             # more than one workgroup
]


@pytest.mark.parametrize("channels,batch", [(3, None), (1, None), (3, 2), (1, 3)])
def test_crop_and_uncrop_are_copies(A, channels, batch):
    g = torch.Generator().manual_seed(17)
    for H, W, sh, sw in CROPS:
        shape = (channels, H, W) if batch is None else (batch, channels, H, W)
        x = torch.rand(shape, generator=g).to(DEV)
        pad = A.AutoCrop.calc_pad(sh, sw, H, W)
        for pad_value in (0, 0.5):
            ac = A.AutoCrop(sh, sw, pad, pad_value, A.AutoCrop.calc_crop(sh, sw, H, W), True)
            cropped = ac.crop(x)
            assert cropped.is_contiguous() and torch.equal(cropped, x[..., sh, sw]), (H, W, sh, sw)
            back = ac.uncrop(cropped)
            assert back.shape == x.shape and back.is_contiguous()
            assert torch.equal(back, F.pad(cropped, pad, mode="constant", value=pad_value)), (H, W, sh, sw, pad_value)
        off = A.AutoCrop(sh, sw, pad, 0, None, False)
        assert off.uncrop(cropped) is cropped
        whole = A.AutoCrop(slice(None), slice(None), (0, 0, 0, 0), 0, None, True)          # no bars: nothing is moved
        assert whole.crop(x) is x and whole.uncrop(x) is x
        strided = x.transpose(-1, -2)
        assert whole.crop(strided).is_contiguous() and torch.equal(whole.crop(strided), strided)
    half = torch.rand((3, 20, 24), generator=g).to(DEV).half()
    ac = A.AutoCrop(slice(2, 18), slice(4, None), (4, 0, 2, 2), 0.5, (4, 2, 20, 16), True)
    assert ac.crop(half).dtype == torch.float16 and torch.equal(ac.crop(half), half[:, 2:18, 4:])
    assert torch.equal(ac.uncrop(ac.crop(half)), F.pad(half[:, 2:18, 4:], (4, 0, 2, 2), value=0.5))
    dummy = A.AutoCropDummy()
    assert dummy.crop(half) is half and dummy.uncrop(half) is half


def test_process_image_autocrop_on_a_padded_frame(hiplib):
    """The 120 x 200 image of test_gpu_iw3_pipeline.py::test_process_image_entry inside black bars (top 10, bottom 14, left 6)."""
    from nunif_amd.iw3.base_depth_model import CallableDepthModel
    from nunif_amd.iw3.utils import (apply_divergence, apply_rgbd, postprocess_image, process_image, process_image_autocrop)
    net = lambda t: t.mean(1) + 0.3 * t[:, 0]                              # noqa: E731
    model = CallableDepthModel(net, lower_bound=56).load(gpu=0)
    x = synth_image(97, 3, 120, 200).to(DEV)
    pad = (6, 0, 10, 14)
    framed = F.pad(x, pad, mode="constant", value=0.0)
    for extra in ({}, {"rgbd": True}):
        plain = SimpleNamespace(mapper="mul_1", convergence=0.5, divergence=3.0, method="forward_fill", synthetic_view="both",
                                edge_dilation=2, tta=False, **extra)
        args = SimpleNamespace(**{**vars(plain), "autocrop": "black"})
        out = process_image_autocrop(framed, args, model, autocrop_uncrop=False)
        assert out.shape == (3, 120, 400) and torch.equal(out, process_image(x, plain, model)), extra
        depth = model.minmax_normalize_chw(model.infer(x, edge_dilation=2))
        left, right = apply_rgbd(x, depth, mapper="mul_1") if extra else apply_divergence(depth, x, plain, None)
        want = postprocess_image(F.pad(left, pad, value=0.0), F.pad(right, pad, value=0.0), plain)
        out = process_image_autocrop(framed, args, model, autocrop_uncrop=True)
        assert out.shape == (3, 144, 412) and torch.equal(out, want), extra
        # without the flag nothing is cropped
        assert torch.equal(process_image_autocrop(x, plain, model), process_image(x, plain, model))
        with pytest.raises(NotImplementedError, match="process_image_autocrop"):
            process_image(framed, args, model)


class _QueueSideModel:
    """Stands in for a video inpaint side model: answers None once (its queue is filling), then 4-D eyes."""

    def __init__(self):
        self.calls = 0

    def infer(self, im, depth, **kwargs):
        self.calls += 1
        if self.calls % 2 == 1:
            return None, None
        return im * 0.75, (im.flip(-1) * 0.5).contiguous()


def test_process_image_autocrop_with_a_side_model_that_answers_in_batches(hiplib):
    """The 4-D branch (iw3/utils.py:535-540): the side model's [1,3,H,W] eyes are unbatched, then padded back."""
    from nunif_amd.iw3.base_depth_model import CallableDepthModel
    from nunif_amd.iw3.utils import postprocess_image, process_image, process_image_autocrop
    net = lambda t: t.mean(1) + 0.3 * t[:, 0]                              # noqa: E731
    model = CallableDepthModel(net, lower_bound=56).load(gpu=0)
    x = synth_image(97, 3, 120, 200).to(DEV)
    pad = (6, 0, 10, 14)
    framed = F.pad(x, pad, mode="constant", value=0.0)
    plain = SimpleNamespace(mapper="mul_1", convergence=0.5, divergence=3.0, method="forward_inpaint", synthetic_view="both",
                            edge_dilation=2, tta=False)
    args = SimpleNamespace(**{**vars(plain), "autocrop": "black"})
    side = _QueueSideModel()
    out = process_image_autocrop(framed, args, model, side_model=side, autocrop_uncrop=False)
    assert side.calls == 2 and out.shape == (3, 120, 400)
    assert torch.equal(out, process_image(x, plain, model, side_model=_QueueSideModel()))
    left, right = x * 0.75, (x.flip(-1) * 0.5).contiguous()
    assert torch.equal(out, postprocess_image(left, right, plain))
    out = process_image_autocrop(framed, args, model, side_model=_QueueSideModel(), autocrop_uncrop=True)
    assert out.shape == (3, 144, 412)
    assert torch.equal(out, postprocess_image(F.pad(left, pad, value=0.0), F.pad(right, pad, value=0.0), plain))
