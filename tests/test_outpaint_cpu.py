"""CPU side of the outpaint engine: the restatement tests/outpaint_f64.py in fp32 against the fixture recorded from the reference
class (tests/golden/outpaint.npz) and in float64 against the live class, the state-dict layout, ``pack_weights``' bias table, the
conditions on the test inputs that tests/test_gpu_outpaint.py relies on, and six deliberate mistakes that the GPU test's check must
each catch when they are made in the restatement."""
import math
import os
import sys

import numpy as np
import pytest
import torch

import outpaint_f64 as R
from conftest import GOLDEN
from oracle import refstub

RATIO = 2.2
needs_reference = pytest.mark.skipif(not refstub.reference_available(), reason="the reference checkout is not mounted here")


@pytest.fixture(scope="module")
def fixture():
    return dict(np.load(os.path.join(GOLDEN, "outpaint.npz")))


@pytest.fixture(scope="module")
def sd():
    from nunif_amd.synthetic import light_outpaint_state_dict
    return light_outpaint_state_dict(R.WEIGHT_SEED)


_cache = {}


def restated(sd, name, dtype, mut=()):
    key = (name, dtype, tuple(mut))
    if key not in _cache:
        x, mask = R.case_input(name)
        with torch.inference_mode():
            _cache[key] = R.infer(sd, x, mask, R.CASES[name][3], "raw", dtype, mut)
    return _cache[key]


def ulp32(v):
    return 2.0 ** (math.floor(math.log2(max(float(v), 1e-30))) - 23)


@pytest.mark.parametrize("name", R.FIXTURE_CASES)
def test_restatement_fp32_reproduces_the_reference_class(sd, fixture, name):
    out, taps = restated(sd, name, torch.float32)
    ref = fixture[f"out/{name}/raw"]
    assert out.shape == ref.shape
    assert np.abs(out.numpy() - ref).max() < 1e-5 * max(1.0, np.abs(ref).max())
    if name in R.FIXTURE_TAP_CASES:
        for t in R.TAPS:
            ref = fixture[f"tap/{name}/{t}"]
            assert np.abs(taps[t].numpy() - ref).max() < 1e-5 * max(1.0, np.abs(ref).max()), t


@pytest.mark.parametrize("name", R.FIXTURE_CASES)
def test_reference_fp32_error_is_small(sd, fixture, name):
    """The conditioning guard: with the seeded weights the reference's own fp32 result is within 1e-4 of float64 (a net that
    amplified rounding would make every ratio of the GPU test meaningless), and the output is a signal, not zeros."""
    out64, taps64 = restated(sd, name, torch.float64)
    ref = torch.from_numpy(fixture[f"out/{name}/raw"]).double()
    assert (ref - out64).abs().max().item() < 1e-4
    assert 0.5 < out64.pow(2).mean().sqrt().item() < 5.0
    if name in R.FIXTURE_TAP_CASES:
        for t in R.TAPS:
            assert (torch.from_numpy(fixture[f"tap/{name}/{t}"]).double() - taps64[t]).abs().max().item() < 1e-4, t


@pytest.mark.parametrize("name", ("d", "g"))
def test_restatement_fp32_error_is_small_where_it_is_the_yardstick(sd, name):
    out64, _ = restated(sd, name, torch.float64)
    out32, _ = restated(sd, name, torch.float32)
    assert 1e-7 < (out32.double() - out64).abs().max().item() < 1e-4


@needs_reference
@pytest.mark.parametrize("name", ("a", "b", "c", "d", "e", "f"))
def test_restatement_float64_equals_the_live_class(sd, name):
    sys.path.insert(0, os.path.join(GOLDEN))
    import make_golden_outpaint as G
    x, mask = R.case_input(name)
    z, taps = G.run_reference(G.reference_model(torch.float64), x.double(), mask, R.CASES[name][3])
    out64, taps64 = restated(sd, name, torch.float64)
    assert (z - out64).abs().max().item() < 1e-12
    for t in R.TAPS:
        assert (taps[t] - taps64[t]).abs().max().item() < 1e-12, t


@needs_reference
def test_composite_and_forward_tails_equal_the_live_class(sd):
    sys.path.insert(0, os.path.join(GOLDEN))
    import make_golden_outpaint as G
    model = G.reference_model(torch.float64)
    for name in ("a", "c", "e"):
        x, mask = R.case_input(name)
        with torch.inference_mode():
            comp = model.infer(x.double().clone(), mask, max_size=R.CASES[name][3], composite=True)
            fwd = model(x.double().clone(), mask)
            assert (comp - R.infer(sd, x, mask, R.CASES[name][3], "composite", torch.float64)[0]).abs().max().item() < 1e-12
            assert (fwd - R.infer(sd, x, mask, R.CASES[name][3], "forward", torch.float64)[0]).abs().max().item() < 1e-12


@needs_reference
def test_key_layout_and_bias_table_equal_the_live_class(sd):
    refstub.install()
    from stlizer.models.light_outpaint_v1 import LightOutpaintV1 as Ref
    from nunif_amd.stlizer.models.light_outpaint_v1 import LightOutpaintV1, pack_weights, state_dict_shapes
    ref = Ref()
    rsd = ref.state_dict()
    assert list(rsd) == list(state_dict_shapes()) == list(LightOutpaintV1().state_dict())
    assert all(tuple(rsd[k].shape) == tuple(s) for k, s in state_dict_shapes().items())
    assert all(torch.equal(rsd[k], LightOutpaintV1().state_dict()[k]) for k in rsd if k.endswith((".index", ".delta")))
    ref.load_state_dict(sd)
    packed = pack_weights(sd)
    for blk, e in ((ref.net.enc_block[0], "enc"), (ref.net.mid_block[0], "mid0"), (ref.net.mid_block[2], "mid1"), (ref.net.dec_block[0], "dec")):
        with torch.inference_mode():
            want = blk.bias()
        assert want.shape == (64, 64) and (packed[e + ".mha.table"] - want).abs().max().item() < 1e-6
        assert (want - want.t()).abs().max().item() > 1e-3, "the table is not symmetric: a transpose shows"
    assert (ref.name, ref.i2i_scale, ref.i2i_offset, ref.i2i_in_channels) == (
        LightOutpaintV1.name, LightOutpaintV1().i2i_scale, LightOutpaintV1().i2i_offset, LightOutpaintV1().i2i_in_channels)


def test_state_dict_roundtrip_and_refusals(sd):
    from nunif_amd.stlizer.models.light_outpaint_v1 import LightOutpaintV1, pack_weights
    m = LightOutpaintV1()
    m.load_state_dict(sd)
    back = m.state_dict()
    assert list(back) == list(sd) and all(torch.equal(back[k], sd[k]) for k in sd)
    assert back["net.enc_block.0.bias.index"].dtype == torch.int64
    with pytest.raises(RuntimeError):
        m.load_state_dict({k: v for k, v in sd.items() if k != "net.proj_mid.bias"})
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        m.infer(torch.zeros(1, 3, 64, 64), torch.zeros(1, 1, 64, 64, dtype=torch.bool))
    p = pack_weights(sd)
    assert p["enc.mha.qkv.w"].shape == (64, 192) and p["mid0.pool.pw1.w"].shape == (32, 64) and p["dec.pool.dw.w"].shape == (9, 128)
    # head 1's q columns of the packed matrix are rows 32..63 of the reference's weight; chunk 1 of the pool's first conv starts
    # with channels 32..63 and goes on with their gates 96..127
    assert torch.equal(p["enc.mha.qkv.w"][:, 96:128], sd["net.enc_block.0.mha.mha.qkv_proj.weight"][32:64].t())
    assert torch.equal(p["enc.pool.pw1.w"][:, 64:96], sd["net.enc_block.1.mlp.0.weight"][32:64, :, 0, 0].t())
    assert torch.equal(p["enc.pool.pw1.w"][:, 96:128], sd["net.enc_block.1.mlp.0.weight"][96:128, :, 0, 0].t())


@pytest.mark.parametrize("name", ("e", "f", "g"))
def test_no_resized_mask_value_is_near_the_threshold(name):
    _, mask = R.case_input(name)
    pooled = R.resized_pooled_mask(mask, R.CASES[name][3])
    assert pooled is not None and int(((pooled - 0.5).abs() < 1e-4).sum()) == 0
    assert 0.02 < (pooled > 0.5).float().mean().item() < 0.6


def test_case_geometry():
    assert R.net_size(150, 84, 96) == (96, 54) and R.net_size(90, 170, 128) == (68, 128) and R.net_size(700, 396, 640) == (640, 362)
    assert R.net_size(64, 64, 640) == (64, 64)
    x, mask = R.case_input("a")
    assert float(x[mask.expand_as(x)].min()) > 0.0, "case a keeps the picture under the mask"
    assert bool(R.case_input("b")[1].all()) and not bool(R.case_input("c")[1][0].equal(R.case_input("c")[1][1]))


# which case shows which mistake: the smallest one that has the mechanism
MUTATION_CASE = {"bias_transposed": "a", "pool_div25": "a", "dw_zero_pad": "a", "mask_unpadded": "a", "merged_resize": "e",
                 "skip_last_window_row": "c"}


@pytest.mark.parametrize("mut", R.MUTATIONS)
def test_the_check_catches_each_mistake(sd, fixture, mut):
    """The GPU test's bound, ``e <= 2.2 * e_ref + A`` on the raw output, applied to the fp32 restatement with one mistake built in:
    it must fail (and pass without the mistake)."""
    name = MUTATION_CASE[mut]
    out64, _ = restated(sd, name, torch.float64)
    ref = torch.from_numpy(fixture[f"out/{name}/raw"]).double()
    e_ref = (ref - out64).abs().max().item()
    A = 2 * ulp32(out64.abs().max().item())
    good = (restated(sd, name, torch.float32)[0].double() - out64).abs().max().item()
    bad = (restated(sd, name, torch.float32, (mut,))[0].double() - out64).abs().max().item()
    assert good <= RATIO * e_ref + A
    assert bad > 100 * (RATIO * e_ref + A), (mut, bad, e_ref)


def test_buffer_restatement_and_blend_weight():
    from nunif_amd.stlizer.outpaint import blend_weight
    assert blend_weight(0.6, 29.97) == R.blend_weight(0.6, 29.97) == 0.5           # (1 - 0.6) clamps up to 0.5
    assert abs(blend_weight(0.25, 29.97) - 0.25) < 1e-12 and blend_weight(0.25, 60.0) == 0.5
    frames, coarse = R.buffer_case(3, clean_frame=1)
    out, buf = R.buffer_step(frames, coarse, None, [False, False, True], 0.25, torch.float64)
    assert not torch.isnan(out).any() and torch.equal(out[1], frames[1].double().clamp(0, 1))
    # frame 2 resets: the buffer is coarse_2 * d + coarse_2 * (1 - d)
    d = float(torch.tensor(0.25, dtype=torch.float32))
    assert torch.allclose(buf, coarse[2].double() * d + coarse[2].double() * float(torch.tensor(0.75, dtype=torch.float32)))
    nan1 = torch.isnan(frames[0, 1]) & ~torch.isnan(frames[0, 0])
    assert nan1.any(), "the per-element mask differs between channels somewhere"
