"""CPU side of the SuperPoint engine: the restatement tests/superpoint_f64.py in fp32 against the fixture recorded from the
reference class (tests/golden/superpoint.npz), the state-dict layout, ``pack_weights``, and the conditions on the test inputs that
tests/test_gpu_superpoint.py relies on (how many pixels / rows are too close to a decision to be pinned)."""
import os

import numpy as np
import pytest
import torch

import superpoint_f64 as R
from conftest import GOLDEN
from oracle import refstub


@pytest.fixture(scope="module")
def fixture():
    return dict(np.load(os.path.join(GOLDEN, "superpoint.npz")))


@pytest.fixture(scope="module")
def sd():
    from nunif_amd.synthetic import superpoint_state_dict
    return superpoint_state_dict(R.WEIGHT_SEED)


_cache = {}


def dense(sd, name, dtype):
    if (name, dtype) not in _cache:
        with torch.inference_mode():
            _cache[(name, dtype)] = R.dense(sd, R.case_image(name), dtype)
    return _cache[(name, dtype)]


def test_restatement_fp32_reproduces_the_reference_keypoints_at_120x160(sd, fixture):
    """The fixture holds no dense map of this shape (size): the restatement is tied to the reference class through what the class
    returned, the keypoints and their scores of all three images.  The coordinates are equal; a score is the fp32 score-map value
    at a keypoint, which differs between two fp32 evaluations by their rounding (bound: the dense bound of the other shapes)."""
    name = "s120x160"
    kps, _ = R.keypoints(dense(sd, name, torch.float32)["scores"])
    assert len(kps) == 3
    for b, (xy, s) in enumerate(kps):
        assert np.array_equal(xy.numpy(), fixture[f"sp/{name}/{b}/keypoints"])
        assert np.abs(s.numpy() - fixture[f"sp/{name}/{b}/keypoint_scores"]).max() < 2e-5


@pytest.mark.parametrize("name", [n for n in R.CASES if n != "s120x160"])
def test_restatement_fp32_reproduces_the_reference_class(sd, fixture, name):
    out = dense(sd, name, torch.float32)
    assert np.abs(out["scores"].numpy() - fixture[f"sp/{name}/scores"]).max() < 2e-5
    if name in R.DENSE_DESCRIPTOR_CASES:
        assert np.abs(out["descriptors"].numpy() - fixture[f"sp/{name}/descriptors"]).max() < 2e-6
    for tap in R.TAP_CASES.get(name, ()):
        ref = fixture[f"sp/{name}/{tap}"]
        assert np.abs(out[tap].numpy() - ref).max() < 1e-5 * max(1.0, np.abs(ref).max())
    kps, _ = R.keypoints(torch.from_numpy(fixture[f"sp/{name}/scores"]))
    for b, (xy, s) in enumerate(kps):
        assert np.array_equal(xy.numpy(), fixture[f"sp/{name}/{b}/keypoints"])
        assert np.array_equal(s.numpy(), fixture[f"sp/{name}/{b}/keypoint_scores"])
        if name in R.DENSE_DESCRIPTOR_CASES:
            d = R.sample(xy, torch.from_numpy(fixture[f"sp/{name}/descriptors"][b]))
            assert np.abs(d.numpy() - fixture[f"sp/{name}/{b}/descriptors"]).max() < 1e-6


def test_keypoint_counts_are_in_a_usable_regime(fixture):
    for name, (B, *_rest) in R.CASES.items():
        for b in range(B):
            n = len(fixture[f"sp/{name}/{b}/keypoints"])
            assert 20 <= n <= 400, (name, b, n)
            assert fixture[f"sp/{name}/{b}/keypoint_scores"].max() > 0.9


@pytest.mark.parametrize("name", list(R.CASES))
def test_unsure_band_is_small_for_the_reference(sd, fixture, name):
    """The input condition of the end-to-end GPU test: for the reference fp32 alone, the band of pixels within 8 e_ref of a
    decision holds at most 1 % of the pixels and at most 2 % of the float64 keypoints, and outside it the reference's keypoints
    are the float64 keypoints.  s120x160 has no recorded dense map: its e_ref comes from the fp32 restatement (tied to the class
    by the test above), its reference keypoints from the fixture like the others'."""
    s64 = dense(sd, name, torch.float64)["scores"]
    key = f"sp/{name}/scores"
    ref = (torch.from_numpy(fixture[key]) if key in fixture else dense(sd, name, torch.float32)["scores"]).double()
    e_ref = (ref - s64).abs().max().item()
    band = R.unsure_band(s64, e_ref)
    assert band.double().mean().item() <= 0.01, (name, band.double().mean().item())
    kps64, _ = R.keypoints(s64)
    total = in_band = 0
    for b, (xy, _) in enumerate(kps64):
        x, y = xy[:, 0].long(), xy[:, 1].long()
        total += len(xy)
        in_band += int(band[b][y, x].sum())
        ref_xy = {tuple(v) for v in fixture[f"sp/{name}/{b}/keypoints"].astype(int).tolist()}
        f64_xy = {tuple(v) for v in xy.long().tolist()}
        for px, py in ref_xy ^ f64_xy:
            assert band[b, py, px], (name, b, px, py)
    assert in_band <= 0.02 * total, (name, in_band, total)


@pytest.mark.parametrize("name", list(R.MATCH_CASES))
def test_match_rows_with_a_clear_winner_are_at_least_98_percent(fixture, name):
    d1, d2 = R.match_inputs(name)
    idx64, sim64, gap = R.match(d1, d2, torch.float64)
    ref_sim = torch.from_numpy(fixture[f"match/{name}/sim"]).double()
    e_ref = (ref_sim - sim64).abs().max().item()
    sure = gap > 8 * e_ref
    assert sure.double().mean().item() >= 0.98, name
    assert torch.equal(torch.from_numpy(fixture[f"match/{name}/index"])[sure], idx64[sure])
    if d1.shape[0] > 1:
        assert (sim64 > 0.5).any() and (sim64 < 0.5).any(), "both sides of stlizer's cosine threshold are populated"


def test_restatement_warp_fp32_reproduces_apply_transform(fixture):
    x = R.warp_image("w21x33")
    for pname in R.WARP_PARAMS:
        p = R.warp_params("w21x33", pname)
        for padding in ("zeros", "border"):
            got = R.warp(x, *p, padding, torch.float32)
            assert np.abs(got.numpy() - fixture[f"warp/w21x33/{pname}/{padding}"]).max() < 2e-5, (pname, padding)


def test_pool_floors_at_44x61(sd):
    out = dense(sd, "s44x61", torch.float32)
    assert out["backbone.0"].shape[-2:] == (22, 30) and out["backbone.1"].shape[-2:] == (11, 15)
    assert out["backbone.2"].shape[-2:] == (5, 7) and out["scores"].shape == (1, 40, 56)


def test_state_dict_layout_and_roundtrip(sd):
    from nunif_amd.nunif.utils.superpoint import SuperPoint, state_dict_shapes
    m = SuperPoint(detection_threshold=0.01)
    assert list(m.state_dict()) == list(state_dict_shapes()) and m.conf.detection_threshold == 0.01 and m.stride == 8
    m.load_state_dict(sd)
    back = m.state_dict()
    assert all(torch.equal(back[k], sd[k]) for k in sd)
    with pytest.raises(RuntimeError):
        m.load_state_dict({k: v for k, v in sd.items() if k != "detector.1.bn.weight"})
    with pytest.raises(NotImplementedError):
        SuperPoint(channels=[32, 64, 128, 128, 256])
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        m(torch.zeros(1, 1, 16, 16))


@pytest.mark.skipif(not refstub.reference_available(), reason="the reference checkout is not mounted here")
def test_key_layout_equals_the_live_class():
    refstub.install()
    import nunif.utils.superpoint as KU
    from nunif_amd.nunif.utils.superpoint import SuperPoint, state_dict_shapes
    ref = KU.SuperPoint().state_dict()
    assert list(ref) == list(state_dict_shapes())
    assert all(tuple(ref[k].shape) == tuple(s) for k, s in state_dict_shapes().items())
    assert SuperPoint.default_conf == KU.SuperPoint.default_conf


def test_pack_weights_affine_and_head_fold(sd):
    from nunif_amd.nunif.utils.superpoint import pack_weights
    p = pack_weights(sd)
    g = torch.Generator().manual_seed(5)
    # a 3x3 block: conv -> relu -> affine equals conv -> relu -> BN
    x = torch.randn(1, 64, 6, 7, generator=g).double()
    want = R.unit(sd, "backbone.1.0", x, True, torch.float64)
    w = p["backbone.1.0.w"].double().view(3, 3, 64, 64).permute(3, 2, 0, 1)
    y = torch.relu(torch.nn.functional.conv2d(x, w, p["backbone.1.0.bias"].double(), padding=1))
    got = y * p["backbone.1.0.scale"].double().view(1, -1, 1, 1) + p["backbone.1.0.shift"].double().view(1, -1, 1, 1)
    assert (got - want).abs().max() < 1e-5
    # the two 3x3 head convs side by side, the two 1x1 convs with their BN folded and zero padded columns
    assert p["heads.w"].shape == (1152, 512) and p["detector.w"].shape == (256, 96) and p["descriptor.w"].shape == (256, 256)
    assert torch.equal(p["detector.w"][:, 65:], torch.zeros(256, 31)) and torch.equal(p["detector.bias"][65:], torch.zeros(31))
    h = torch.randn(1, 256, 3, 4, generator=g).double()
    for name, n in (("detector", 65), ("descriptor", 256)):
        want = R.unit(sd, name + ".1", h, False, torch.float64)
        got = torch.einsum("bchw,cn->bnhw", h, p[name + ".w"].double()[:, :n]) + p[name + ".bias"].double()[:n].view(1, -1, 1, 1)
        assert (got - want).abs().max() < 1e-5, name
