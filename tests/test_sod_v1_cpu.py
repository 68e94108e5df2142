"""SOD v1 / convergence estimator without a GPU: the float64 restatement (tests/sod_f64.py) against the reference class's recorded
fp32 result (tests/golden/sod_v1.npz, written by tests/golden/make_golden_sod.py), the state-dict layout and ``.pth`` round trip
against the live reference, the BatchNorm fold, the quantile rule against ``torch.quantile`` in float64, the EMA sequence, and the
conditions on the inputs that make the GPU comparison (tests/test_gpu_sod_v1.py) meaningful."""
import os

import numpy as np
import pytest
import torch

import sod_f64 as R
from conftest import GOLDEN
from oracle import refstub


@pytest.fixture(scope="module")
def golden():
    return dict(np.load(os.path.join(GOLDEN, "sod_v1.npz")))


@pytest.fixture(scope="module")
def sd():
    from nunif_amd.synthetic import sod_v1_state_dict
    return sod_v1_state_dict(R.WEIGHT_SEED)


@pytest.fixture(scope="module")
def truth(sd):
    out = {}
    for name, *_ in R.CASES:
        rgb, depth = R.case_inputs(name)
        out[name] = R.infer(sd, rgb, depth)
    return out


def test_restatement_equals_the_recorded_fp32_reference(golden, truth):
    for name, (sal, depth) in truth.items():
        e = float(R.max_err_per_image(torch.from_numpy(golden[name + "/sal32"]), sal).max())
        print(f"\n[sod_v1] {name}: e_ref(fp32) {e:.3g}")
        assert e < 2e-4                                  # fp32 through ~40 convolutions in series on logits of +-15
        assert float((torch.from_numpy(golden[name + "/depth32"]).double() - depth).abs().max()) < 1e-6
        assert float(torch.from_numpy(golden[name + "/tap_err32"]).max()) < 1e-2


def test_conditions_on_the_inputs(golden, truth):
    populated = 0
    for name, (sal64, _) in truth.items():
        ref = torch.from_numpy(golden[name + "/sal32"]).double()
        e_ref = float(R.max_err_per_image(ref, sal64).max())
        near = float(((ref - 0.5).abs() <= 8 * e_ref).double().mean())
        frac = float((ref > 0.5).double().mean())
        print(f"\n[sod_v1] {name}: mask {frac:.3f}, within 8 e_ref of 0.5: {near:.5f}")
        assert near <= 0.02
        populated += 0.0 < frac < 1.0
    assert populated >= 2
    assert int((golden["empty/sal32"] > 0.5).sum()) == 0
    d = golden["flat/depth32"]
    assert float(d.max() - d.min()) < 1e-6 and abs(float(golden["flat/z32"][0]) - 0.4) < 1e-6


def test_key_layout_and_bn_fold(sd):
    from nunif_amd.iw3.models.sod_v1 import SODV1, fold_bn, pack_weights, rebnconvs, state_dict_shapes
    m = SODV1()
    assert m.i2i_in_size == 192 and m.name == "iw3.sod_v1" and m.name_alias == ("iw3.dsod_v1",)
    assert [(k, tuple(v.shape)) for k, v in m.state_dict().items()] == [(k, tuple(s)) for k, s in state_dict_shapes().items()]
    assert len(rebnconvs()) == 112
    m.load_state_dict(sd)
    p = "u2netp.stage1d.rebnconv3d."
    w, b = fold_bn(sd, p)
    x = torch.randn(2, 32, 9, 11, dtype=torch.float64, generator=torch.Generator().manual_seed(0))
    want = R.rebnconv(R._cast(sd, torch.float64), p[:-1], x, 1)
    got = torch.relu(torch.nn.functional.conv2d(x, w.double(), b.double(), padding=1))
    assert float((got - want).abs().max()) < 1e-5
    packed = pack_weights(sd)
    assert tuple(packed["stage1d.rebnconv3d.w"].shape) == (2, 32, 9, 8)
    assert torch.equal(packed["stage1d.rebnconv3d.w"][1, 5, 7, 3], w[11, 5, 2, 1])
    assert tuple(packed["side.w"].shape) == (6, 64, 9) and tuple(packed["stage1.rebnconvin.w"].shape) == (8, 6, 9, 8)


@pytest.mark.skipif(not refstub.reference_available(), reason="the reference checkout is not mounted here")
def test_state_dict_and_pth_round_trip_against_the_live_class(sd, tmp_path):
    refstub.install()
    from iw3.models.sod_v1 import SODV1 as Ref
    from nunif_amd.iw3.models.sod_v1 import SODV1
    ref = Ref()
    ours = SODV1()
    assert [(k, tuple(v.shape)) for k, v in ref.state_dict().items()] == [(k, tuple(v.shape)) for k, v in ours.state_dict().items()]
    ref.load_state_dict(sd)
    path = str(tmp_path / "iw3_sod_v1_20260125.pth")
    torch.save({"nunif_model": 1, "name": ref.name, "kwargs": ref.get_kwargs(), "state_dict": ref.state_dict()}, path)
    from nunif_amd.nunif.models import load_model
    m, _ = load_model(path, weights_only=True)
    assert isinstance(m, SODV1)
    assert all(torch.equal(v, sd[k]) for k, v in m.state_dict().items())


QUANTILE_CASES = {"empty": [], "one": [0.3], "two": [0.2, 0.7], "equal": [0.6] * 50,
                  "clamped": list(np.linspace(0.0, 1.0, 400) ** 0.25)}


def test_quantile_rule_against_torch_quantile_float64():
    for name, vals in QUANTILE_CASES.items():
        d = torch.zeros(1, 1, 32, 32, dtype=torch.float64)
        s = torch.zeros(1, 1, 32, 32, dtype=torch.float64)
        d.view(-1)[:len(vals)] = torch.tensor(vals, dtype=torch.float64)
        s.view(-1)[:len(vals)] = 1.0
        pos = 0.95 if name == "clamped" else 0.5
        z = float(R.depth_position(s, d, pos)[0])
        if not vals:
            want = 0.5
        else:
            v = torch.tensor(vals, dtype=torch.float64)
            q1, q9 = float(torch.quantile(v, 0.1)), float(torch.quantile(v, 0.9))
            want = q1 if q9 - q1 < 1e-6 else min(max((q1 + q9) / 2 + (pos - 0.5) * 3 * (q9 - q1), 0.0), 1.0)
        assert abs(z - want) < 1e-12, name
    assert float(R.depth_position(s, d, 0.95)[0]) == 1.0


def test_ema_sequence_equals_the_recorded_one(golden):
    z = torch.from_numpy(golden["ema/z32"])
    resets = [i in R.EMA_RESETS for i in range(R.EMA_FRAMES)]
    out, state = [], None
    for i0, i1 in ((0, 3), (3, 6), (6, 8)):
        o, state = R.ema(z[i0:i1], R.EMA_DECAY, resets[i0:i1], state)
        out.append(o)
    assert torch.equal(torch.cat(out), torch.from_numpy(golden["ema/out32"]))
    assert float(golden["ema/out32"][3]) == float(golden["ema/z32"][3])       # the reset of frame 2 shows at frame 3


def test_abi_declares_and_binds_the_new_entries():
    from nunif_amd import _hip
    for name in ("nunif_hip_sod_v1_create", "nunif_hip_sod_v1_forward", "nunif_hip_sod_v1_destroy", "nunif_hip_sod_v1_entry",
                 "nunif_hip_sod_v1_debug_taps", "nunif_hip_sod_v1_depth_position", "nunif_hip_sod_v1_ema"):
        assert name in _hip.SIGNATURES and hasattr(_hip.lib(), name)


def test_missing_checkpoint_names_the_file(tmp_path):
    from nunif_amd.iw3.convergence_estimator import ConvergenceEstimator
    with pytest.raises(FileNotFoundError, match="iw3_sod_v1_20260125.pth"):
        ConvergenceEstimator(0.5, device_id=-1, model_dir=str(tmp_path))
