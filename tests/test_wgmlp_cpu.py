"""``waifu2x.wgmlp_4x`` without a GPU: the torch restatement (tests/wgmlp_ref.py) against the fixture recorded from the reference's
own class (tests/golden/wgmlp.npz, make_golden_wgmlp.py) and against the live class where the reference tree is present; the product
model's contract (registry name, geometry, key layout, refusals); and the proof that the seeded weights and inputs SEE the mistakes a
kernel is likely to make: each mutation of the restatement moves the output by at least 10 x the bound the GPU tests hold the engine
to (2.5 x the fp16 emulation's own error).

Measured (seed 21, tile 64, batch 2; max |mutation - exact| at the net's output over the bound 2.5 x max |emulation - exact| = 3.85e-3):
mix_transposed 51.6, pad_zero 19.3, ln2_on_u 72.9, shift_order 58.1, down_strided 68.4, up_repeat 73.8, dilation_swapped 14.4,
patch_crop 28.1.  tanh GELU is 0.02 there and cannot be more with any weights: around z = +-2 the tanh form differs from the erf form
by 4.7e-4 at most, the size of one fp16 rounding of the activation.  It is held where the two forms CAN be told apart, in the tail:
the ``gelu`` tap of the window-gMLP alone with ``wgmlp_ref.gelu_tail_weights`` (pre-activations in [-3.9, -3.5]; its docstring has the
reasoning), against the tap bound of the GPU tests, 3.5 x the emulation's error: measured 44.9 x the emulation's error at C = 128 and
42.6 x at C = 256, i.e. 12.8 and 12.2 x the bound.  tests/test_gpu_wgmlp.py runs the kernel on the same weights and input.
This is a DEVIATION from the issue, which asks for every mutation at 10 x the bound "on the test inputs": for this one mutation the
weights of one block are shifted for the purpose and the bound is the tap's, not the output's.
"""
import os

import numpy as np
import pytest
import torch

import wgmlp_ref as R
from conftest import GOLDEN

SEED, INPUT_SEED = 21, 5
NAME = "waifu2x.wgmlp_4x"
A_OUT, A_TAP = 2.5, 3.5               # tests/errloc.py: the global bounds of the GPU tests, outputs and taps
GELU_TAIL_CASES = ((0, 128), (3, 256))      # (block, channels) of the kernel-alone GELU-tail case, as in tests/test_gpu_wgmlp.py
GELU_TAIL_SHAPE, GELU_TAIL_SEED = (1, 16, 24), 7


@pytest.fixture(scope="module")
def case():
    from nunif_amd import synthetic
    g = {k: torch.from_numpy(v) for k, v in np.load(os.path.join(GOLDEN, "wgmlp.npz")).items()}
    sd = synthetic.wgmlp_state_dict(SEED)
    x = g["x"]
    assert torch.equal(x, R.test_input(INPUT_SEED, 2, 64))
    with torch.inference_mode():
        torch.set_num_threads(max(1, min(16, os.cpu_count() or 8)))
        y64 = R.forward64(sd, x, raw=True)
        noise = float((R.emulated(sd, x, raw=True).double() - y64).abs().max())
    return sd, x, g, y64, noise


def _model():
    from nunif_amd.nunif.models import create_model
    import nunif_amd.waifu2x.utils  # noqa: F401
    return create_model(NAME)


def test_create_model_knows_the_name():
    m = _model()
    assert type(m).__name__ == "WGMLP4x" and m.name == NAME
    assert (m.i2i_scale, m.i2i_offset, m.i2i_blend_size, m.i2i_in_channels) == (4, 36, 16, 3)
    assert m.find_valid_tile_size(256) == 256 and m.find_valid_tile_size(128) == 112 and m.find_valid_tile_size(64) == 64
    with pytest.raises(ValueError):
        m.find_valid_tile_size(32)
    # a fresh model is the nearest-neighbour upscaler (scale_bias 0, the mixing near zero with bias 1) and has no CPU path
    sd = m.state_dict()
    assert float(sd["unet.to_image.scale_bias"]) == 0.0
    ws = sd["unet.wgmlp2.blocks.0.gmlp.gmlp.proj_spatial.weight"]
    assert ws.shape == (64, 64, 1) and float(ws.abs().max()) <= 1e-3 / 256 and torch.equal(sd["unet.wgmlp2.blocks.0.gmlp.gmlp.proj_spatial.bias"], torch.ones(64))
    with pytest.raises(RuntimeError):
        m.eval()(torch.zeros(1, 3, 64, 64))


def test_refused_geometries_and_forms():
    from nunif_amd.nunif.models import create_model
    import nunif_amd.waifu2x.utils  # noqa: F401
    for kw in (dict(base_dim=96), dict(lv1_mlp_ratio=1), dict(lv2_mlp_ratio=4), dict(in_channels=1), dict(out_channels=1)):
        with pytest.raises(ValueError, match="base_dim 128"):
            create_model(NAME, **kw)
    m = _model()
    with pytest.raises(NotImplementedError, match="training-time"):
        m.set_tile_mode()
    with pytest.raises(NotImplementedError, match="IRMixIn"):
        m.eval()(torch.zeros(1, 19, 64, 64))
    assert m.has_callback() is False


def test_seeded_weights_load_and_are_not_the_initialisation():
    from nunif_amd import synthetic
    m = _model()
    for regime in ("benign", "hot"):
        sd = synthetic.wgmlp_state_dict(3, regime)
        assert {k: tuple(v.shape) for k, v in sd.items()} == {k: tuple(v.shape) for k, v in m.state_dict().items()}
        m.load_state_dict(sd, strict=True)
        assert 0.5 <= float(sd["unet.to_image.scale_bias"]) <= 1.0
        for p in R.block_prefixes():
            ws, bs = sd[p + "gmlp.gmlp.proj_spatial.weight"], sd[p + "gmlp.gmlp.proj_spatial.bias"]
            assert 0.08 < float(ws.std()) < 0.4 and 0.5 < float(bs.mean()) < 1.5 and float(bs.std()) > 0.1
            assert float((sd[p + "norm1.weight"] - 1).abs().max()) > 0.05 and float((sd[p + "norm2.weight"] - 1).abs().max()) > 0.05
        assert all(float(v.abs().max()) > 0 for k, v in sd.items() if k.endswith(".bias"))
    assert torch.equal(synthetic.wgmlp_state_dict(3)["unet.patch.weight"], synthetic.wgmlp_state_dict(3)["unet.patch.weight"])
    bad = dict(sd)
    bad.pop("unet.patch.bias")
    with pytest.raises(RuntimeError):
        m.load_state_dict(bad, strict=True)


def test_restatement_fp32_matches_the_fixture(case):
    sd, x, g, _, _ = case
    taps = {}
    with torch.inference_mode():
        raw = R.forward(sd, x, taps=taps, raw=True)
        y = R.forward(sd, x)
    assert raw.shape == (2, 3, 184, 184)
    assert float((raw[0] - g["raw0"]).abs().max()) < 2e-5 and float((raw[1, :, :96, :96] - g["raw1"]).abs().max()) < 2e-5
    assert torch.equal(y, raw.clamp(0, 1))
    assert float((taps["ir"][:, :, 8:40, 8:40] - g["ir"]).abs().max()) < 2e-5
    for i, p in enumerate(("unet.wgmlp1.blocks.1.", "unet.wgmlp2.blocks.2.", "unet.wgmlp3.blocks.2.")):
        ref = g[f"tap{i}"]
        assert float((taps[p][:, 4:20, 4:20, :32] - ref).abs().max()) < 2e-5 * max(1.0, float(ref.abs().max())), p
    # a meaningful fixture: a picture, not clamped away, and the net's residual is visible in it
    sat = float(((raw <= 0) | (raw >= 1)).float().mean())
    nn4 = torch.nn.functional.interpolate(x, scale_factor=4, mode="nearest")[:, :, 36:-36, 36:-36]
    assert sat < 0.1 and float(raw.std()) > 0.05 and float((raw - nn4).pow(2).mean().sqrt()) > 0.05


def test_shift_order_is_reversed():
    assert R.shift_config(2) == (True, False) and R.shift_config(4) == (True, False, True, False) and R.shift_config(3) == (False, True, False)
    from nunif_amd.waifu2x.models.wgmlp import block_names
    assert [s for _, _, s, _ in block_names()] == list(R.shift_config(2) + R.shift_config(4) + R.shift_config(3))
    assert [p for p, _, _, _ in block_names()] == R.block_prefixes()


@pytest.mark.parametrize("mutation", R.MUTATIONS)
def test_mutations_are_visible(case, mutation):
    sd, x, _, y64, noise = case
    if mutation == "gelu_tanh":
        for blk, C in GELU_TAIL_CASES:
            p = R.block_prefixes()[blk]
            t = R.gelu_tail_weights(sd, p)
            xm = R.gmlp_input(GELU_TAIL_SEED, *GELU_TAIL_SHAPE, C)
            t64, te, tm = {}, {}, {}
            with torch.inference_mode():
                R.gmlp64(t, p, xm, True, t64)
                R.gmlp_emulated(t, p, xm, True, te)
                R.window_gmlp(R.cast(t, torch.float64), p, xm.double(), True, tm, mut={mutation})
            d = float((tm["gelu"] - t64["gelu"]).abs().max())
            bound = A_TAP * float((te["gelu"].double() - t64["gelu"]).abs().max())
            print(f"\n{mutation} C={C}: max |mutated - exact| at the gelu tap {d:.3e}, GPU tap bound {bound:.3e}, ratio {d / bound:.1f}")
            assert d >= 10.0 * bound, (mutation, C, d, bound)
        return
    with torch.inference_mode():
        d = float((R.forward64(sd, x, raw=True, mut={mutation}) - y64).abs().max())
    bound = A_OUT * noise
    print(f"\n{mutation}: max |mutated - exact| {d:.3e}, GPU bound {bound:.3e} (2.5 x {noise:.3e}), ratio {d / bound:.1f}")
    assert d >= 10.0 * bound, (mutation, d, bound)


def _reference_class():
    from oracle import refstub
    if not refstub.reference_available():
        pytest.skip("needs the reference tree")
    refstub.install()
    from waifu2x.models.wgmlp import WGMLP4x
    return WGMLP4x


def test_restatement_float64_matches_the_live_class(case):
    sd, x, _, y64, _ = case
    ref = _reference_class()().eval().double()
    ref.load_state_dict(R.cast(sd, torch.float64), strict=True)
    with torch.inference_mode():
        y = ref(x.double())
    assert float((y - y64.clamp(0, 1)).abs().max()) < 1e-10


def test_layout_geometry_and_checkpoints_match_the_live_class(tmp_path):
    ref = _reference_class()().eval()
    m = _model()
    rsd, sd = ref.state_dict(), m.state_dict()
    assert list(rsd.keys()) == list(sd.keys())
    for k in rsd:
        assert rsd[k].shape == sd[k].shape and rsd[k].dtype == sd[k].dtype, k
    assert torch.equal(rsd["unet.to_image.resampling.weight"], sd["unet.to_image.resampling.weight"])
    assert (ref.i2i_scale, ref.i2i_offset, ref.i2i_blend_size, ref.i2i_in_channels) == (m.i2i_scale, m.i2i_offset, m.i2i_blend_size, m.i2i_in_channels)
    assert ref.name == m.name
    for size in range(8, 1025):
        try:
            want = ref.find_valid_tile_size(size)
        except ValueError:
            with pytest.raises(ValueError):
                m.find_valid_tile_size(size)
            continue
        assert m.find_valid_tile_size(size) == want, size
    # a .pth round-trips between the trees both ways
    a, b = str(tmp_path / "ref.pth"), str(tmp_path / "hip.pth")
    torch.save(rsd, a)
    m.load_state_dict(torch.load(a), strict=True)
    assert all(torch.equal(m.state_dict()[k], rsd[k]) for k in rsd)
    from nunif_amd import synthetic
    m.load_state_dict(synthetic.wgmlp_state_dict(8), strict=True)
    torch.save(m.state_dict(), b)
    ref.load_state_dict(torch.load(b), strict=True)
    assert all(torch.equal(ref.state_dict()[k], m.state_dict()[k]) for k in rsd)
