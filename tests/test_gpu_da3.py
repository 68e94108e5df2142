"""Any_V3_Mono on the device: the multi-rank selection against ``torch.sort``, the disparity stage and the model forward against
float64 with the fp32 restatement's own error as yardstick (tests/da3_ref.py), and ``DepthAnythingV3MonoModel.infer`` around a
seeded stand-in backbone."""
import math
import os

import numpy as np
import pytest
import torch

import da3_ref as R
from conftest import GOLDEN

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SEED = 20
ALL_SHAPES = R.SHAPES + (R.LARGE,)


@pytest.fixture(scope="module")
def fix():
    return np.load(os.path.join(GOLDEN, "da3_disparity.npz"))


@pytest.fixture(scope="module")
def sd(fix):
    return {k[3:]: torch.from_numpy(fix[k]) for k in fix.files if k.startswith("sd_")}


@pytest.fixture(scope="module")
def net(sd):
    import nunif_amd.iw3.models  # noqa: F401
    from nunif_amd.nunif.models import create_model
    m = create_model("iw3.da3mono_disparity")
    m.load_state_dict(sd)
    return m.eval().to(DEV)


def feats(x, **kw):
    from nunif_amd.iw3.models import DA3MonoDisparity
    return DA3MonoDisparity.extract_features(x, **kw)


def check_rule(got, ref32, ref64, what):
    ok, e_hip, bound = R.within_rule(got.cpu(), ref32, ref64)
    print(f"{what}: e_hip {e_hip:.3e} bound {bound:.3e}")
    assert ok, (what, e_hip, bound)


# ---- features ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", ALL_SHAPES, ids=lambda s: "x".join(map(str, s)))
@pytest.mark.parametrize("kind", R.KINDS)
def test_features_equal_indexing_the_sort(shape, kind):
    B, H, W = shape
    x = R.depth_map(kind, B, H, W, SEED)
    got = feats(x.to(DEV))
    assert got.shape == (B, 64) and torch.equal(got.cpu(), R.extract_features(x)), (shape, kind)
    if B == 1:
        assert torch.equal(feats(x[0].to(DEV)), got[0])                         # the 3-D form


def test_features_of_a_batch_are_those_of_its_images_on_any_stream():
    xs = [R.depth_map(k, 1, 56, 98, SEED + i) for i, k in enumerate(R.KINDS)]
    x = torch.cat(xs).to(DEV)
    whole = feats(x)
    for b in range(len(xs)):
        assert torch.equal(feats(x[b:b + 1]), whole[b:b + 1]), b
    assert torch.equal(feats(x), whole)
    side = torch.cuda.Stream(device=DEV)
    side.wait_stream(torch.cuda.current_stream(DEV))
    with torch.cuda.stream(side):
        other = feats(x)
    side.synchronize()
    assert torch.equal(other, whole)


@pytest.mark.parametrize("shape", [(1, 1, 3), (3, 37, 53), (2, 518, 920)])
def test_features_workspace_bound_is_honoured(hiplib, shape):
    B, H, W = shape
    need = hiplib.nunif_hip_da3mono_features_workspace_bytes(B, H, W)
    guard = 4096
    buf = torch.full((need + guard,), 0xA5, dtype=torch.uint8, device=DEV)
    x = R.depth_map("noise", B, H, W, SEED)
    got = feats(x.to(DEV), workspace=buf[:need])
    assert torch.equal(got.cpu(), R.extract_features(x))
    assert bool((buf[need:] == 0xA5).all())
    from nunif_amd import _hip
    with pytest.raises(_hip.NunifHipError):
        feats(x.to(DEV), workspace=buf[:need - 16])


# ---- disparity stage ---------------------------------------------------------------------------------------------------------------------
def stage(depth, sky, raw, **kw):
    from nunif_amd.iw3.depth_anything_v3_model import disparity_stage
    return disparity_stage(depth.to(DEV), sky.to(DEV), raw_output=raw, **kw)


@pytest.mark.parametrize("shape", ALL_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_stage_not_raw(shape):
    B, H, W = shape
    depth, sky = R.depth_map("noise", B, H, W, SEED), R.sky_map(B, H, W, SEED)          # a seventh of the sky map is ON the threshold
    got = stage(depth, sky, False)
    assert got.shape == (B, 1, H, W)
    check_rule(got, R.forward_stage(depth, sky, False), R.forward_stage(depth, sky, False, dtype=torch.float64), f"stage {shape}")
    assert torch.equal(stage(depth, sky, False), got)


def test_stage_all_sky_rule_is_exact(fix):
    """0, 9, 10 (one of them exactly on the threshold) and 11 non-sky pixels: zeros exactly below 10."""
    depth, sky = torch.from_numpy(fix["count_depth"]), torch.from_numpy(fix["count_sky"])
    got = stage(depth, sky, False).cpu()
    assert [bool((g == 0).all()) for g in got] == [True, True, False, False]
    check_rule(got, torch.from_numpy(fix["count_out"]), R.forward_stage(depth, sky, False, dtype=torch.float64), "count cases")
    on = torch.full_like(sky, R.SKY_THRESH)                                  # every pixel on the threshold: none is sky, w = 0
    got = stage(depth, on, False).cpu()
    assert torch.equal(got, R.forward_stage(depth, on, False))


def _raw_checks(depth, sky, what):
    from nunif_amd.iw3.depth_anything_v3_model import disparity_debug_stats
    B = depth.shape[0]
    got, ws = stage(depth, sky, True, return_workspace=True)
    stats, counts = disparity_debug_stats(ws, B)
    stats, counts = stats.cpu(), counts.cpu()
    for b in range(B):
        v = torch.sort(depth[b][~(sky[b] > R.SKY_THRESH)])[0]
        m = v.numel()
        assert int(counts[b]) == m, (what, b)
        p = 0.99 * (m - 1)
        lo, hi = v[math.floor(p)], v[math.ceil(p)]
        assert stats[b, 0] == lo and stats[b, 1] == hi, (what, b, stats[b], lo, hi)          # bit-equal to the sort's
        q64 = float(lo) + (float(hi) - float(lo)) * (p - math.floor(p))
        ulp = float(torch.nextafter(torch.tensor(abs(q64), dtype=torch.float32), torch.tensor(math.inf)) - abs(np.float32(q64)))
        assert abs(float(stats[b, 2]) - q64) <= ulp, (what, b, float(stats[b, 2]), q64)
    check_rule(got, R.forward_stage(depth, sky, True), R.forward_stage(depth, sky, True, dtype=torch.float64), what)
    assert torch.equal(stage(depth, sky, True), got)
    return got


@pytest.mark.parametrize("shape", ALL_SHAPES, ids=lambda s: "x".join(map(str, s)))
@pytest.mark.parametrize("kind", ["noise", "ramp_ties", "low_bits"])
def test_stage_raw(shape, kind):
    B, H, W = shape
    _raw_checks(R.depth_map(kind, B, H, W, SEED), R.sky_map(B, H, W, SEED), f"raw {shape} {kind}")


def test_stage_raw_small_counts_and_all_sky(fix):
    depth, sky = torch.from_numpy(fix["rawcount_depth"]), torch.from_numpy(fix["rawcount_sky"])
    assert [int((s <= R.SKY_THRESH).sum()) for s in sky] == [1, 2, 100, 101]
    _raw_checks(depth, sky, "raw counts 1, 2, 100, 101")
    sky = torch.cat([sky[:2], torch.full_like(sky[:1], 0.9), sky[3:]])      # image 2 all sky: the reference raises, the engine zeros
    got = stage(depth, sky, True).cpu()
    want = R.forward_stage(depth, sky, True, all_sky_zeros=True)
    assert bool((got[2] == 0).all())
    check_rule(got, want, R.forward_stage(depth, sky, True, dtype=torch.float64, all_sky_zeros=True), "raw with an all-sky image")


# ---- model forward -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", ALL_SHAPES, ids=lambda s: "x".join(map(str, s)))
@pytest.mark.parametrize("kind", ["noise", "ramp_ties"])
def test_model_forward(fix, sd, net, shape, kind):
    B, H, W = shape
    x = R.depth_map(kind, B, H, W, SEED)
    got = net(x.to(DEV))
    key = f"fwd_{R.SHAPES.index(shape)}_{kind}" if shape in R.SHAPES else None
    ref32 = torch.from_numpy(fix[key]) if key else R.model_forward(sd, x)
    ref64 = R.model_forward(sd, x, dtype=torch.float64)
    check_rule(got, ref32, ref64, f"forward {shape} {kind}")
    if B == 1:
        assert torch.equal(net(x[0].to(DEV)), got[0])                       # the 3-D form == the batched form on one image
    if kind == "ramp_ties":
        # exactly the tied maximum moves: without sky_shift every pixel is 1 / (depth + shift)
        shift = R.mlp(sd, R.extract_features(x), torch.float64)[:, 0].reshape(-1, 1, 1, 1)
        plain = 1.0 / (x.double() + shift)
        moved = (got.cpu().double() - plain).abs() > 1e-3 * plain
        assert torch.equal(moved, x == x.amax(dim=(1, 2, 3), keepdim=True))
        if H * W >= 64:                                                      # (of 3 pixels two are the maximum)
            assert 0.2 < float(moved.float().mean()) < 0.3


# ---- DepthAnythingV3MonoModel ----------------------------------------------------------------------------------------------------------------
class StandIn:
    """A seeded stand-in for the hub net: (B, 1, 3, H, W) -> depth and sky [B, 1, H, W] from fixed mixes of the input channels."""

    def __init__(self):
        g = torch.Generator().manual_seed(9)
        self.wd, self.ws = torch.rand(3, generator=g).to(DEV), torch.rand(3, generator=g).to(DEV)
        self.calls = []

    def __call__(self, x):
        assert x.ndim == 5 and x.shape[1] == 1 and x.shape[2] == 3
        x = x[:, 0].float()
        depth = ((x * self.wd.view(1, 3, 1, 1)).sum(1, keepdim=True).abs() + 0.3)
        sky = torch.sigmoid((x * self.ws.view(1, 3, 1, 1)).sum(1, keepdim=True) * 2.0)
        self.calls.append((depth, sky))
        return {"depth": depth, "sky": sky}


def _depth_aa():
    import nunif_amd.iw3.models  # noqa: F401
    from nunif_amd.nunif.models import create_model
    torch.manual_seed(4)
    aa = create_model("iw3.depth_aa")
    sd = aa.state_dict()
    sd["proj_out.weight"] = torch.randn_like(sd["proj_out.weight"]) * 0.05
    aa.load_state_dict(sd)
    return aa.eval().to(DEV)


@pytest.mark.parametrize("name,mode", [("Any_V3_Mono", "max"), ("Any_V3_Mono_01", "minmax")])
@pytest.mark.parametrize("tta,aa,dilation,raw", [(False, False, 0, False), (True, True, 2, False), (True, False, 2, True),
                                                 (False, True, 0, True)])
def test_infer_is_the_chain_on_the_engine_s_own_intermediates(name, mode, tta, aa, dilation, raw):
    from nunif_amd.iw3.depth_anything_model import batch_preprocess
    from nunif_amd.iw3.depth_model_factory import create_depth_model
    from nunif_amd.iw3.dilation import dilate_edge
    from conftest import synth_image
    net = StandIn()
    m = create_depth_model(name)
    m.load(gpu=0, resolution=56, raw_output=raw, backbone=net, depth_aa=_depth_aa())
    assert m.scaler.mode == mode
    im = torch.stack([synth_image(31, 3, 70, 100), synth_image(32, 3, 70, 100)]).to(DEV)
    got = m.infer(im, tta=tta, depth_aa=aa, edge_dilation=dilation, enable_amp=False)
    x = batch_preprocess(im, 56)
    assert got.shape == (2, 1) + tuple(x.shape[2:]) and got.is_cuda and len(net.calls) == 1
    depth, sky = (v.cpu() for v in net.calls[0])
    assert depth.shape[0] == (4 if tta else 2)
    # the stage on the recorded backbone output, by the rule; then the engine's own DepthAA / dilate_edge on the engine's stage
    from nunif_amd.iw3.depth_anything_v3_model import disparity_stage
    out = disparity_stage(depth.to(DEV), sky.to(DEV), raw_output=raw)
    check_rule(out, R.forward_stage(depth, sky, raw), R.forward_stage(depth, sky, raw, dtype=torch.float64), f"infer stage raw={raw}")
    if aa:
        out = m.depth_aa.infer(out)
    if dilation:
        out = dilate_edge(out, dilation) if not raw else -dilate_edge(-out, dilation)
    if tta:
        out = (out[:2] + torch.flip(out[2:], dims=[3])) * 0.5
    assert torch.equal(got, out)
    single = m.infer(im[0], tta=tta, depth_aa=aa, edge_dilation=dilation, enable_amp=False)
    assert single.shape == got.shape[1:]
    # normalisation through the model's scaler
    norm = m.minmax_normalize_chw(got[0])
    assert float(norm.max()) == 1.0 and (mode == "max" or float(norm.min()) == 0.0)
    m.reset()


def test_infer_with_the_trained_disparity_model_and_process_image(net, sd):
    from nunif_amd.iw3.depth_model_factory import create_depth_model
    from conftest import synth_image
    back = StandIn()
    m = create_depth_model("Any_V3_Mono")
    m.load(gpu=0, resolution=56, backbone=back, disparity_model=net)
    im = synth_image(33, 3, 70, 100).to(DEV)
    got = m.infer(im, enable_amp=False)
    depth = back.calls[0][0].cpu()
    check_rule(got.unsqueeze(0), R.model_forward(sd, depth), R.model_forward(sd, depth, dtype=torch.float64), "infer with disparity_model")
    # process_image end to end: depth -> the scaler (max mode) -> forward_fill -> side by side
    import argparse
    from nunif_amd.iw3 import utils as U
    args = argparse.Namespace(batch_size=1, tta=False, low_vram=False, disable_amp=True, edge_dilation=2, depth_aa=False, rgbd=False,
                              half_rgbd=False, method="forward_fill", mapper="none", divergence=2.0, convergence=0.5,
                              synthetic_view="both", pix_fmt="yuv420p", state={"device": torch.device(DEV)})
    m.reset()
    sbs = U.process_image(im, args, m)
    assert sbs.shape == (3, 70, 200) and bool(torch.isfinite(sbs).all())
    assert not torch.equal(sbs[:, :, :100], sbs[:, :, 100:])
