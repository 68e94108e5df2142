"""ZoeD_Any_* on the GPU: the metric-bins head alone against float64 (yardstick: the restatement under the fp16-autocast emulation,
limits of test_gpu_depth_errloc.py through errloc, cells of one bottleneck pixel's footprint; the five bin-centre taps under
A_TAP / B_TAP), determinism, NaN handling, ``forward_features``, the pre-processing kernel, ``ZoeDepthModel.infer`` end to end and
the scheduler.  The seeded small encoder (ViT-S under a DPT neck of width 256), inputs of at most 112 x 224.

Measured worst ratios: profiles/zoedepth_errloc.txt."""
import os

import numpy as np
import pytest
import torch

import errloc as E
import zoedepth_ref as R
from conftest import GOLDEN

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
HEAD_SEED = 4100
SHAPES = [(1, 1, 1), (2, 2, 3), (3, 3, 5), (1, 4, 8)]             # (B, bottleneck h, w): outputs 28 x 14 .. 112 x 210, B = 3


@pytest.fixture(scope="module")
def head_sd():
    from nunif_amd.synthetic import zoedepth_head_state_dict
    return zoedepth_head_state_dict(HEAD_SEED, prefix="")


@pytest.fixture(scope="module")
def head(hiplib, head_sd):
    from nunif_amd.iw3.zoedepth_model import HipZoeDepthHead
    return HipZoeDepthHead(head_sd, DEV)


_refs = {}


def refs(head_sd, case):
    """(inputs, [y64] + taps64, [yemu] + taps_emu) of a case: computed once, shared, never written to."""
    if case not in _refs:
        B, bh, bw = case
        E.set_threads()
        inp = R.random_inputs(HEAD_SEED + 100 + 10 * bh + bw, B, bh, bw)
        t64, te = [], []
        with torch.inference_mode():
            y64 = R.head_f64(head_sd, *inp, taps=t64)
            ye = R.head_emulated(head_sd, *inp, taps=te)
        _refs[case] = (inp, [y64] + t64, [ye] + te)
    return _refs[case]


def run_head(head, inp):
    oc, bt, blocks, rel = inp
    f, keep = head.features_from_maps(oc, bt, blocks)
    y = head.forward(f, rel.to(DEV))
    torch.cuda.synchronize()
    return y.unsqueeze(1), keep


def stats(y, y64, ye, bh, bw, tap):
    A, B = (E.A_TAP, E.B_TAP) if tap else (E.A_SIDE, E.B_SIDE)
    cell = (max(1, y64.shape[2] // bh), max(1, y64.shape[3] // bw))
    tau = E.TAP_TAU_REL * float(y64.double().pow(2).mean().sqrt())
    return E.localised_stats(y.cpu(), y64, ye, [(cell, (0, 0))], B, tau), A, B, tau


@pytest.mark.parametrize("case", SHAPES, ids=lambda c: f"B{c[0]}_{c[1]}x{c[2]}")
def test_head_against_float64(head, head_sd, case, capsys):
    inp, y64s, yes = refs(head_sd, case)
    y, _ = run_head(head, inp)
    outs = [y] + head.debug_taps()
    lines, checks = [], []
    for j, (o, y64, ye) in enumerate(zip(outs, y64s, yes)):
        assert o.shape == y64.shape, (j, o.shape, y64.shape)
        st, A, B, tau = stats(o, y64, ye, case[1], case[2], j > 0)
        lines.append(f"zoedepth head {case} {'out' if j == 0 else f'tap{j - 1}'}: global {st['global']:.3f} (limit {A}) worst {st['worst']:.3f} "
                     f"(limit {B}) err {st['_gmax']:.3e} noise {st['_nmax']:.3e}")
        checks.append((st, A, B, tau, lines[-1]))
    with capsys.disabled():
        print("\n" + "\n".join(lines))
    out_dir = os.environ.get("NUNIF_ZOEDEPTH_ERRLOC_OUT")
    if out_dir:
        with open(os.path.join(out_dir, "zoedepth_errloc.txt"), "a") as f:
            f.write("\n".join(lines) + "\n")
    for st, A, B, tau, line in checks:
        E.assert_localised(st, A, B, tau, label=line)


def test_head_is_deterministic_and_batch_independent(head, head_sd):
    inp, _, _ = refs(head_sd, (3, 3, 5))
    y, _ = run_head(head, inp)
    y2, _ = run_head(head, inp)
    assert torch.equal(y, y2)
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        y3, _ = run_head(head, inp)
    assert torch.equal(y, y3)
    oc, bt, blocks, rel = inp
    for b in range(3):
        yb, _ = run_head(head, (oc[b:b + 1], bt[b:b + 1], [t[b:b + 1] for t in blocks], rel[b:b + 1]))
        assert torch.equal(yb[0], y[b]), b


def test_head_nan_to_num(head, head_sd):
    inp, _, _ = refs(head_sd, (2, 2, 3))
    oc, bt, blocks, rel = inp
    rel = rel.clone()
    rel[0, 3, 5], rel[0, 10, 7], rel[1, 20, 2] = float("nan"), float("inf"), float("-inf")
    y, _ = run_head(head, (oc, bt, blocks, rel))
    with torch.inference_mode():
        want = torch.nan_to_num(R.head_forward(head_sd, oc, bt, blocks, rel))
    assert bool(torch.isfinite(y).all())
    planted = [(0, 0, 3, 5), (0, 0, 10, 7), (1, 0, 20, 2)]
    for idx in planted:
        assert float(y.cpu()[idx]) == float(want[idx]), (idx, float(y.cpu()[idx]), float(want[idx]))
    clean, _ = run_head(head, inp)
    mask = torch.ones_like(y, dtype=torch.bool)
    for idx in planted:
        mask[idx] = False
    assert torch.equal(y[mask], clean[mask])                   # a pixel's NaN stays in that pixel


@pytest.fixture(scope="module")
def net_sd():
    from nunif_amd.synthetic import zoedepth_any_state_dict
    return zoedepth_any_state_dict(4300, grid=16)


@pytest.fixture(scope="module")
def net(hiplib, net_sd):
    from nunif_amd.iw3.zoedepth_model import HipZoeDepthAny
    return HipZoeDepthAny(net_sd, DEV)


def test_forward_features_leaves_the_same_depth(net):
    from nunif_amd.iw3.depth_anything_v2 import HipDepthAnythingV2
    x = (torch.rand(2, 3, 56, 98, generator=torch.Generator().manual_seed(5)) * 2 - 1).to(DEV)
    plain = net.core(x)
    rel, feats = net.forward_features(x)
    assert torch.equal(plain, rel)
    assert torch.equal(net.core(x), plain)
    assert (feats.bh, feats.bw, feats.channels) == (2, 4, 256) and list(feats.rh) == [4, 8, 16, 32] and list(feats.rw) == [7, 14, 28, 56]


def prep_cases(fix):
    return [(i, str(n), *(int(v) for v in fix["prep_shapes"][i])) for i, n in enumerate(fix["prep_names"])]


def test_preprocess_kernel_against_the_reference_fixture(hiplib):
    import importlib.util
    from nunif_amd.iw3.zoedepth_model import batch_preprocess
    fix = np.load(os.path.join(GOLDEN, "zoedepth.npz"))
    spec = importlib.util.spec_from_file_location("make_golden_zoedepth", os.path.join(GOLDEN, "make_golden_zoedepth.py"))
    gen = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(gen)
    for i, name, B, H, W in prep_cases(fix):
        y, pad_h, pad_w = batch_preprocess(gen.frame(4200 + i, B, H, W).to(DEV))
        y = y.cpu()
        tol = 2e-6
        assert [pad_h, pad_w] == [int(v) for v in fix[f"prep_{i}_pads"]] and list(y.shape) == [int(v) for v in fix[f"prep_{i}_shape"]], name
        if f"prep_{i}_y" in fix:
            assert float((y - torch.from_numpy(fix[f"prep_{i}_y"])).abs().max()) <= tol, name
        else:
            assert float((y[:, :, :pad_h + 8, :pad_w + 8] - torch.from_numpy(fix[f"prep_{i}_tl"])).abs().max()) <= tol, name
            assert float((y[:, :, -pad_h - 8:, -pad_w - 8:] - torch.from_numpy(fix[f"prep_{i}_br"])).abs().max()) <= tol, name
            assert abs(float(y.double().sum()) - float(fix[f"prep_{i}_sum"])) <= tol * y.numel(), name
            assert float((y[:, :, 3::64] - torch.from_numpy(fix[f"prep_{i}_rows"])).abs().max()) <= tol, name
            assert float((y[:, :, :, 3::64] - torch.from_numpy(fix[f"prep_{i}_cols"])).abs().max()) <= tol, name


def chain(sd, x, tta, emulate, edge_dilation=0):
    """``batch_infer`` :88-148 on the CPU: float64, or the fp16-autocast emulation of the network (enable_amp covers ``_forward``
    only: crop, ``dilate_edge(-out)`` and the flip merge run in fp32 behind it, in float64 in the float64 chain)."""
    from oracle import dilation as ODil
    from oracle.fp16_emulation import fp16_autocast_emulation, half_weights
    xp, pad_h, pad_w = R.batch_preprocess(x.double())
    if tta:
        xp = torch.cat([xp, torch.flip(xp, dims=[3])], dim=0)
    if emulate:
        with fp16_autocast_emulation():
            out = R.model_forward(half_weights(sd), xp.float())
    else:
        out = R.model_forward({k: v.double() for k, v in sd.items()}, xp)
    out = -torch.nan_to_num(out)[:, :, pad_h:out.shape[2] - pad_h, pad_w:out.shape[3] - pad_w]
    if edge_dilation:
        gauss = ODil.GAUSS
        ODil.GAUSS = gauss.to(out.dtype)
        try:
            out = ODil.dilate_edge(out, edge_dilation)
        finally:
            ODil.GAUSS = gauss
    out = out.double()
    if tta:
        a, b = out.chunk(2, dim=0)
        out = (a + torch.flip(b, dims=[3])) * 0.5
    return out


@pytest.fixture(scope="module")
def model(net_sd, hiplib):
    from nunif_amd.iw3.depth_model_factory import create_depth_model
    m = create_depth_model("ZoeD_Any_N")
    return m.load(gpu=0, state_dict=net_sd)


@pytest.mark.parametrize("shape", [(3, 90, 160), (2, 3, 160, 90)], ids=["chw_90x160", "bchw_160x90"])
@pytest.mark.parametrize("edge_dilation", [0, 2])
@pytest.mark.parametrize("tta", [False, True])
def test_infer_end_to_end(model, net_sd, shape, tta, edge_dilation, capsys):
    """``ZoeDepthModel.infer`` against the float64 chain (pre-processing, network, crop, ``dilate_edge(-out)``, flip merge) under
    the limits of the head test, for tta on / off and edge_dilation 0 / 2."""
    E.set_threads()
    x = torch.rand(*shape, generator=torch.Generator().manual_seed(9))
    y = model.infer(x.to(DEV), tta=tta, edge_dilation=edge_dilation)
    xb = x if x.dim() == 4 else x.unsqueeze(0)
    assert y.shape[:-2] == ((xb.shape[0], 1) if x.dim() == 4 else (1,)) and model.is_metric()
    yb = (y if x.dim() == 4 else y.unsqueeze(0)).cpu()
    with torch.inference_mode():
        y64, ye = chain(net_sd, xb, tta, False, edge_dilation), chain(net_sd, xb, tta, True, edge_dilation)
    assert yb.shape == y64.shape
    bh, bw = (y64.shape[2] + 27) // 28, (y64.shape[3] + 27) // 28
    st, A, B, tau = stats(yb, y64, ye, bh, bw, False)
    line = (f"zoedepth infer {shape} tta={tta} edge_dilation={edge_dilation}: global {st['global']:.3f} worst {st['worst']:.3f} "
            f"err {st['_gmax']:.3e} noise {st['_nmax']:.3e}")
    with capsys.disabled():
        print("\n" + line)
    out_dir = os.environ.get("NUNIF_ZOEDEPTH_ERRLOC_OUT")
    if out_dir:
        with open(os.path.join(out_dir, "zoedepth_errloc.txt"), "a") as f:
            f.write(line + "\n")
    E.assert_localised(st, A, B, tau, label=line)


def _args(batch_size, **kw):
    import argparse
    base = dict(batch_size=batch_size, tta=False, low_vram=False, disable_amp=True, edge_dilation=2, depth_aa=False,
                rgbd=False, half_rgbd=False, method="grid_sample", mapper="none", divergence=2.0, convergence=0.5,
                synthetic_view="both", pix_fmt="yuv420p", state={"device": torch.device(DEV)})
    base.update(kw)
    return argparse.Namespace(**base)


def test_scheduler_runs_with_the_model(model):
    """``process_image`` and ``bind_batch_frame_callback`` take the model like any other depth model."""
    from nunif_amd.iw3 import utils as U
    from nunif_amd.iw3.frame_pipeline import bind_batch_frame_callback
    g = torch.Generator().manual_seed(11)
    sbs = U.process_image(torch.rand(3, 90, 160, generator=g).to(DEV), _args(1), model)
    assert sbs.shape == (3, 90, 320) and bool(torch.isfinite(sbs).all())
    model.reset()
    cb, pre = bind_batch_frame_callback(model, None, set(), _args(2))
    frames = cb(pre(torch.rand(2, 3, 90, 160, generator=g).to(DEV), [0, 1], False)) or []
    frames += cb(pre(None, [], True)) or []
    assert len(frames) == 2
    model.reset()
