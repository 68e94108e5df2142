"""SOD v1 / the convergence estimator on the HIP engine (nunif_amd/csrc/sod_v1.hip) against the float64 restatement
(tests/sod_f64.py), with the reference class's own recorded fp32 result (tests/golden/sod_v1.npz) as the yardstick: the kernels
take fp32 operands, as transnetv2.hip does, so the limit is that file's 2.2 for the output and 3.5 for the seven taps,
``e_hip <= limit * e_ref + 1e-6`` for the max error per image.  And the per-frame convergence tensor through the warps:
frame b of a batch call equals the scalar call with that frame's value, byte for byte.

Measured on one MI355X: saliency worst ratio e_hip / e_ref 1.275 (flat, B = 3), taps worst 1.180 (hx1); estimator end to end
3.2e-8 against a half-precision reference deviation of 5.1e-4."""
import os
import types

import numpy as np
import pytest
import torch

import sod_f64 as R
from conftest import GOLDEN

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
LIMIT, TAP_LIMIT = 2.2, 3.5
TAPS = ("hx1", "hx2", "hx3", "hx4", "hx5", "hx6", "hx1d")


@pytest.fixture(scope="module")
def golden():
    return dict(np.load(os.path.join(GOLDEN, "sod_v1.npz")))


@pytest.fixture(scope="module")
def sd():
    from nunif_amd.synthetic import sod_v1_state_dict
    return sod_v1_state_dict(R.WEIGHT_SEED)


@pytest.fixture(scope="module")
def model(sd):
    from nunif_amd.iw3.models.sod_v1 import SODV1
    m = SODV1()
    m.load_state_dict(sd)
    return m.to(DEV).eval()


@pytest.fixture(scope="module")
def truth(sd):
    """float64 saliency, resized depth and taps of the three cases, computed once."""
    out = {}
    for name, *_ in R.CASES:
        taps = {}
        rgb, depth = R.case_inputs(name)
        sal, d = R.infer(sd, rgb, depth, taps=taps)
        out[name] = (sal, d, taps)
    return out


def batch_inputs():
    pairs = [R.case_inputs(name) for name, *_ in R.CASES]
    return torch.cat([p[0] for p in pairs]).to(DEV), torch.cat([p[1] for p in pairs]).to(DEV)


@pytest.mark.parametrize("B", [1, 3])
def test_net_against_float64(model, golden, truth, B):
    names = [c[0] for c in R.CASES][:B]
    rgb, depth = batch_inputs()
    sal, d, taps = model.debug_taps(rgb[:B], depth[:B])
    for i, name in enumerate(names):
        s64, d64, t64 = truth[name]
        e_ref = float(R.max_err_per_image(torch.from_numpy(golden[name + "/sal32"]), s64)[0])
        e_hip = float(R.max_err_per_image(sal[i:i + 1].cpu(), s64)[0])
        print(f"\n[sod_v1] B={B} {name}: e_ref {e_ref:.4g} e_hip {e_hip:.4g} ratio {e_hip / max(e_ref, 1e-30):.3f}")
        assert e_hip <= LIMIT * e_ref + 1e-6
        assert float((d[i:i + 1].cpu().double() - d64).abs().max()) <= 2e-6
        for k, tname in enumerate(TAPS):
            t_ref = float(golden[name + "/tap_err32"][k])
            t_hip = float(R.max_err_per_image(taps[tname][i:i + 1].cpu(), t64[tname])[0])
            print(f"[sod_v1]   {tname}: e_ref {t_ref:.4g} e_hip {t_hip:.4g} ratio {t_hip / max(t_ref, 1e-30):.3f}")
            assert t_hip <= TAP_LIMIT * t_ref + 1e-6, tname


def test_batch_equals_single_images_and_streams_agree(model):
    rgb, depth = batch_inputs()
    sal, d = model.infer(rgb, depth)
    for i in range(3):
        s1, d1 = model.infer(rgb[i:i + 1], depth[i:i + 1])
        assert torch.equal(s1[0], sal[i]) and torch.equal(d1[0], d[i])
    outs = []
    for _ in range(2):
        st = torch.cuda.Stream(device=DEV)
        st.wait_stream(torch.cuda.current_stream(DEV))
        with torch.cuda.stream(st):
            outs.append(model.infer(rgb, depth)[0])
        st.synchronize()
    assert torch.equal(outs[0], outs[1]) and torch.equal(outs[0], sal)


@pytest.mark.parametrize("rgb_size,depth_size", [((97, 131), (37, 53)), ((270, 480), (74, 130))])
def test_entry_kernel_against_interpolate_float64(rgb_size, depth_size):
    import ctypes
    from nunif_amd import _hip
    rgb1, depth1 = R.scene(7, rgb_size, depth_size)
    rgb2, depth2 = R.scene(8, rgb_size, depth_size)
    rgb, depth = torch.cat([rgb1, rgb2]).to(DEV), torch.cat([depth1, depth2]).to(DEV)
    x6 = torch.empty((2, 6, 192, 192), device=DEV)
    d = torch.empty((2, 1, 192, 192), device=DEV)
    p = lambda t: ctypes.c_void_p(t.data_ptr())     # noqa: E731
    _hip.check(_hip.lib().nunif_hip_sod_v1_entry(p(rgb), *rgb_size, p(depth), *depth_size, 2, p(x6), p(d),
                                                 _hip.current_stream_ptr(torch.device(DEV))))
    want6, wantd = R.entry(rgb.cpu().double(), depth.cpu().double())
    assert float((x6.cpu().double() - want6).abs().max()) <= 2e-6
    assert float((d.cpu().double() - wantd).abs().max()) <= 2e-6


def _mask_of(n, total=192 * 192, seed=0):
    idx = torch.randperm(total, generator=torch.Generator().manual_seed(seed))[:n]
    s = torch.zeros(total)
    s[idx] = 0.9
    return s.reshape(1, 1, 192, 192)


def test_quantile_kernel_against_float64(golden):
    from nunif_amd.iw3.convergence_estimator import ConvergenceEstimator
    cases = []
    for name, *_ in R.CASES:
        cases.append((torch.from_numpy(golden[name + "/sal32"]), torch.from_numpy(golden[name + "/depth32"]), 0.5))
    cases.append((torch.from_numpy(golden["empty/sal32"]), torch.from_numpy(golden["scene_a/depth32"]), 0.5))
    d_a = torch.from_numpy(golden["scene_a/depth32"])
    for n in (1, 2, 36863, 36864):
        cases.append((_mask_of(n, seed=n), d_a, 0.5))
    cases.append((_mask_of(50), torch.full((1, 1, 192, 192), 0.6), 0.5))             # all equal
    cases.append((_mask_of(36864), d_a, 0.95))                                       # clamped at 1
    cases.append((_mask_of(36864), d_a, 0.0))
    for k, (s, d, pos) in enumerate(cases):
        want = float(R.depth_position(s.double(), d.double(), pos)[0])
        got = ConvergenceEstimator.depth_position_from_ratio(s.to(DEV), d.to(DEV), pos)
        assert got.shape == (1, 1, 1, 1) and got.dtype == torch.float32 and got.is_cuda
        assert abs(float(got) - want) <= 2e-6, (k, float(got), want)
        if int((s > 0.5).sum()) == 0:
            assert float(got) == 0.5
    s = torch.cat([c[0] for c in cases[:4]])
    d = torch.cat([c[1] for c in cases[:4]])
    got = ConvergenceEstimator.depth_position_from_ratio(s.to(DEV), d.to(DEV), 0.5).flatten().cpu()
    want = R.depth_position(s.double(), d.double(), 0.5)
    assert float((got.double() - want).abs().max()) <= 2e-6 and float(got[3]) == 0.5


def test_estimator_end_to_end_with_ema_and_resets(sd, golden):
    from nunif_amd.iw3.convergence_estimator import ConvergenceEstimator
    rgbs, depths = R.ema_inputs()
    resets = [i in R.EMA_RESETS for i in range(R.EMA_FRAMES)]
    est = ConvergenceEstimator(R.CONVERGENCE, device_id=0, enable_ema=True, decay=R.EMA_DECAY, state_dict=sd)
    got = []
    for i0, i1 in ((0, 3), (3, 6), (6, 8)):
        z = est(rgbs[i0:i1].to(DEV), depths[i0:i1].to(DEV), reset_pts=resets[i0:i1])
        assert z.shape == (i1 - i0, 1, 1, 1) and z.is_cuda
        got.append(z.flatten().cpu())
    got = torch.cat(got).double()
    sal, d = R.infer(sd, rgbs, depths)
    z64 = R.depth_position(sal, d, R.CONVERGENCE)
    want, state = [], None
    for i0, i1 in ((0, 3), (3, 6), (6, 8)):
        o, state = R.ema(z64[i0:i1], R.EMA_DECAY, resets[i0:i1], state)
        want.append(o)
    want = torch.cat(want)
    e_ref = float((torch.from_numpy(golden["ema/out16"]).double() - want).abs().max())
    e_hip = float((got - want).abs().max())
    print(f"\n[sod_v1] estimator: e_ref(half) {e_ref:.4g} e_hip {e_hip:.4g}")
    assert e_hip <= 2.5 * e_ref + 2e-6
    # the empty mask: exactly 0.5, EMA off
    from nunif_amd.synthetic import sod_v1_state_dict
    est = ConvergenceEstimator(R.CONVERGENCE, device_id=0, state_dict=sod_v1_state_dict(R.WEIGHT_SEED, out_bias=R.EMPTY_OUT_BIAS))
    assert float(est(rgbs[:1].to(DEV), depths[:1].to(DEV))) == 0.5


# ---- the per-frame value through the warps -----------------------------------------------------------------------------------
class _Stub:
    def __init__(self, values):
        self.values = torch.tensor(values, dtype=torch.float32, device=DEV).reshape(-1, 1, 1, 1)

    def __call__(self, im, depth, reset_pts=None):
        return self.values[:depth.shape[0]]


def _args(method, convergence=0.5, model=None):
    return types.SimpleNamespace(method=method, divergence=2.0, convergence=convergence, mapper="none", synthetic_view="both",
                                 state={"convergence_model": model}, warp_steps=None, preserve_screen_border=False,
                                 disable_amp=False, stereo_width=None)


def _frames():
    g = torch.Generator().manual_seed(5)
    im = torch.rand(3, 3, 64, 96, generator=g).to(DEV)
    depth = torch.rand(3, 1, 64, 96, generator=g).to(DEV)
    return im, depth


@pytest.fixture(scope="module")
def row_flow():
    from nunif_amd.iw3.models.row_flow_v3 import RowFlowV3
    from nunif_amd import synthetic
    m = RowFlowV3().eval()
    m.load_state_dict(synthetic.row_flow_v3_state_dict(3))
    m = m.to(DEV)
    m.delta_output = True
    return m


@pytest.mark.parametrize("method", ["forward_fill", "grid_sample", "row_flow_v3"])
def test_per_frame_convergence_equals_scalar_calls(method, row_flow):
    from nunif_amd.iw3.utils import apply_divergence
    side = row_flow if method == "row_flow_v3" else None
    im, depth = _frames()
    values = [0.2, 0.5, 0.8]
    left, right = apply_divergence(depth, im, _args(method, model=_Stub(values)), side)
    for b, v in enumerate(values):
        v32 = float(torch.tensor(v, dtype=torch.float32))
        le, ri = apply_divergence(depth[b:b + 1], im[b:b + 1], _args(method, convergence=v32), side)
        assert torch.equal(le[0], left[b]) and torch.equal(ri[0], right[b]), (method, b)
    other, _ = apply_divergence(depth[0:1], im[0:1], _args(method, convergence=float(torch.tensor(values[2], dtype=torch.float32))), side)
    assert not torch.equal(other[0], left[0])                           # frame 0 is warped with ITS value, not frame 2's
    le_t, ri_t = apply_divergence(depth, im, _args(method, model=_Stub([0.5, 0.5, 0.5])), side)
    le_s, ri_s = apply_divergence(depth, im, _args(method, convergence=0.5), side)
    assert torch.equal(le_t, le_s) and torch.equal(ri_t, ri_s)


def test_process_image_with_the_real_estimator(sd):
    from nunif_amd.iw3.convergence_estimator import ConvergenceEstimator
    from nunif_amd.iw3 import utils as U

    class Depth:
        def get_ema_buffer_size(self):
            return 1

        def infer(self, x, **kw):
            return x.mean(dim=0, keepdim=True)

        def minmax_normalize_chw(self, d):
            return (d - d.min()) / (d.max() - d.min())

    est = ConvergenceEstimator(0.5, device_id=0, state_dict=sd)
    args = _args("forward_fill", model=est)
    x = R.scene(4, (64, 96), (64, 96))[0][0].to(DEV)
    out = U.process_image(x, args, Depth())
    assert out.shape == (3, 64, 192) and bool(torch.isfinite(out).all())


# ---- every stereo method, with the estimator built from a checkpoint in the model directory -------------------------------------
ALL_METHODS = ["NULL", "forward", "forward_fill", "backward", "grid_sample", "row_flow_v3", "row_flow", "row_flow_v3_sym",
               "row_flow_sym", "mlbw_l2", "mlbw_l4", "mlbw_l2s", "mlbw_l4s", "forward_inpaint", "mlbw_l2_inpaint"]


@pytest.fixture(scope="module")
def model_dir(tmp_path_factory, sd):
    """A model directory with seeded checkpoints under the reference's file names (stereo_model_factory / convergence_estimator)."""
    from nunif_amd.iw3 import models  # noqa: F401
    from nunif_amd.iw3 import stereo_model_factory as F
    from nunif_amd.iw3.convergence_estimator import SOD_FILE
    from nunif_amd.nunif.models import create_model, save_model
    from nunif_amd import synthetic as S
    d = str(tmp_path_factory.mktemp("hub"))
    ck = os.path.join(d, "checkpoints")
    os.makedirs(ck)

    def save(name, state, filename):
        m = create_model(name)
        m.load_state_dict(state, strict=True)
        save_model(m, os.path.join(ck, filename))

    save("iw3.sod_v1", sd, SOD_FILE)
    save("sbs.row_flow_v3", S.row_flow_v3_state_dict(301), F.ROW_FLOW_V3)
    save("sbs.row_flow_v3", S.row_flow_v3_state_dict(302), F.ROW_FLOW_V3_SYM)
    save("sbs.mlbw_l2", S.mlbw_state_dict(411, 2, False), F.MLBW[("l2", 1)])
    save("sbs.mlbw_l4", S.mlbw_state_dict(413, 4, False), F.MLBW[("l4", 1)])
    save("sbs.mlbw_l2s", S.mlbw_state_dict(412, 2, True), F.MLBW[("l2s", 1)])
    save("sbs.mlbw_l4s", S.mlbw_state_dict(414, 4, True), F.MLBW[("l4s", 1)])
    save("sbs.mask_mlbw_l2", S.mlbw_state_dict(431, 2, False, hole_mask=True), F.MASK_MLBW_L2_D1)
    save("inpaint.light_inpaint_v1", S.light_inpaint_state_dict(701), F.INPAINT_MODELS["light_inpaint_v1"]["image"])
    save("inpaint.light_video_inpaint_v1", S.light_video_inpaint_state_dict(801), F.INPAINT_MODELS["light_inpaint_v1"]["video"])
    return d


@pytest.fixture(scope="module")
def estimator(model_dir):
    from nunif_amd.iw3.convergence_estimator import ConvergenceEstimator
    return ConvergenceEstimator(0.5, device_id=0, model_dir=model_dir)        # the checkpoint is found by its file name


def _scene_batch():
    pairs = [R.scene(20 + i, (64, 96), (64, 96)) for i in range(2)]
    return torch.cat([p[0] for p in pairs]).to(DEV), torch.cat([p[1] for p in pairs]).to(DEV)


@pytest.mark.parametrize("method", ALL_METHODS)
def test_every_method_runs_with_the_estimator_and_a_mapper(method, model_dir, estimator):
    """What ``iw3.cli --convergence-mode sod_v1`` does per batch, for every method name the engine accepts, with mapper pow2:
    the right shape, finite, and frame b equal to the scalar call with that frame's mapped convergence, byte for byte."""
    from nunif_amd.iw3 import stereo_model_factory as F
    from nunif_amd.iw3.mapper import get_mapper
    from nunif_amd.iw3.utils import apply_divergence
    side = F.create_stereo_model(method, 2.0, 0, model_dir=model_dir)
    im, depth = _scene_batch()
    args = _args(method, model=estimator)
    args.mapper = "pow2"
    left, right = apply_divergence(depth, im, args, side)
    assert left.shape == im.shape and right.shape == im.shape
    assert bool(torch.isfinite(left).all()) and bool(torch.isfinite(right).all())
    conv = get_mapper("pow2")(estimator(im, depth))
    assert conv.shape == (2, 1, 1, 1) and conv.is_cuda
    raw = estimator(im, depth).flatten().cpu()
    assert torch.allclose(conv.flatten().cpu(), raw * raw, atol=1e-6) and 0.0 < float(raw.min()) and float(raw.max()) < 1.0
    for b in range(2):
        scalar = _args(method, convergence=float(conv[b]))
        scalar.mapper = "pow2"
        le, ri = apply_divergence(depth[b:b + 1], im[b:b + 1], scalar, side)
        assert torch.equal(le[0], left[b]) and torch.equal(ri[0], right[b]), (method, b)


@pytest.mark.parametrize("method", ["mlbw_l2_inpaint", "forward_inpaint"])
def test_inpaint_infer_accepts_a_one_element_tensor(method, model_dir):
    """Image mode, one frame: ``side_model.infer`` with a one-element convergence tensor equals the scalar call."""
    from nunif_amd.iw3 import stereo_model_factory as F
    side = F.create_stereo_model(method, 2.0, 0, model_dir=model_dir)
    side.set_mode("image")
    im, depth = _scene_batch()
    im, depth = im[:1], depth[:1]
    t = torch.tensor([0.3], dtype=torch.float32, device=DEV)
    kw = dict(divergence=2.0, preserve_screen_border=False, synthetic_view="both", inner_dilation=0, outer_dilation=0,
              max_width=None, enable_amp=True)
    le_t, ri_t = side.infer(im, depth, convergence=t, **kw)
    le_s, ri_s = side.infer(im, depth, convergence=float(t[0]), **kw)
    assert le_t.shape == im.shape and torch.equal(le_t, le_s) and torch.equal(ri_t, ri_s)
    le_o, _ = side.infer(im, depth, convergence=0.7, **kw)
    assert not torch.equal(le_o, le_t)
