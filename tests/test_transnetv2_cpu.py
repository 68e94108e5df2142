"""TransNetV2 without a GPU: the float restatement against the reference class's recorded fp32 result, the state-dict layout
against the live reference, the detector windowing against the reference's ``detect_boundary`` (tests/golden/transnetv2.npz,
written by tests/golden/make_golden_transnetv2.py), and the conditions that make the GPU comparison meaningful."""
import os
import re

import numpy as np
import pytest
import torch

import transnetv2_ref as R
from conftest import GOLDEN, ROOT
from oracle import refstub


@pytest.fixture(scope="module")
def fixture():
    return dict(np.load(os.path.join(GOLDEN, "transnetv2.npz")))


@pytest.fixture(scope="module")
def sd():
    from nunif_amd.synthetic import transnetv2_state_dict
    return transnetv2_state_dict(R.WEIGHT_SEED)


@pytest.fixture(scope="module")
def f64(sd):
    with torch.inference_mode():
        return {name: R.forward(sd, R.case_frames(name), torch.float64) for name in R.FIXTURE_CASES}


def _fix(fixture, name):
    return torch.from_numpy(fixture[f"a/{name}/one_hot"]).double(), torch.from_numpy(fixture[f"a/{name}/many_hot"]).double()


def _err(a, b):
    return max((a[0] - b[0]).abs().max().item(), (a[1] - b[1]).abs().max().item())


def test_restatement_fp32_matches_the_reference_class(sd, fixture, f64):
    """Two fp32 evaluations of the same formulas (same torch ops): they differ from each other by no more than each differs from
    float64, and by a few 1e-7 of the logit scale."""
    for name in R.FIXTURE_CASES:
        with torch.inference_mode():
            one, many = R.forward(sd, R.case_frames(name), torch.float32)
        ref = _fix(fixture, name)
        assert one.shape == ref[0].shape
        scale = max(1.0, ref[0].abs().max().item(), ref[1].abs().max().item())
        d = _err((one.double(), many.double()), ref)
        assert d <= 2 * _err(ref, f64[name]) + 1e-6 * scale, (name, d)


def test_fixture_meets_the_conditions_of_the_decision_test(fixture, f64):
    """For every case: frames whose float64 logit lies within m = 8 * e_ref of zero are at most 2 %; the reference's own fp32
    decision equals the float64 one on all others; and (a one-frame window has one side only) both sides of the threshold hold a
    frame with |logit| > 100 m.  Without these the GPU decision test could pass while comparing nothing."""
    for name, (T, B, _, _, _) in R.FIXTURE_CASES.items():
        ref, (one64, _) = _fix(fixture, name), f64[name]
        m = 8 * _err(ref, f64[name])
        near = one64.abs() < m
        assert near.double().mean().item() <= 0.02, (name, int(near.sum()))
        assert torch.equal((ref[0] > 0)[~near], (one64 > 0)[~near]), name
        if T * B > 1:
            assert (one64 > 100 * m).any() and (one64 < -100 * m).any(), (name, one64.min().item(), one64.max().item(), m)
        else:
            assert one64.abs().min() > 100 * m


def test_detector_clips_have_no_frame_near_the_threshold(sd, fixture):
    """The detector sets are compared outright on the 237- and 101-frame clips: every probability the reference thresholded there is
    far from 0.5 against the fp32-vs-float64 error of its window."""
    for n in (237, 101):
        clip, windows, probs = R.detect_clip(n), fixture[f"b/{n}/windows"], fixture[f"b/{n}/probs"]
        for w in range(windows.shape[0]):
            with torch.inference_mode():
                one64, _ = R.forward(sd, clip[torch.from_numpy(windows[w]).long()], torch.float64)
            p = torch.from_numpy(probs[w]).double().clamp(1e-12, 1 - 1e-7)
            e_ref = (torch.log(p / (1 - p)) - one64[0]).abs()[one64[0].abs() < 10].max().item()
            assert one64[0].abs().min().item() > 8 * e_ref, (n, w)


@pytest.mark.skipif(not refstub.reference_available(), reason="the reference checkout is not mounted here")
def test_state_dict_layout_equals_the_live_reference():
    refstub.install()
    from nunif.utils.transnetv2 import TransNetV2 as Ref
    from nunif_amd.nunif.utils.transnetv2 import TransNetV2, state_dict_shapes
    ref = Ref().state_dict()
    assert list(ref) == list(state_dict_shapes())
    assert {k: tuple(v.shape) for k, v in ref.items()} == {k: tuple(s) for k, s in state_dict_shapes().items()}
    ours = TransNetV2()
    assert {k: (tuple(v.shape), v.dtype) for k, v in ours.state_dict().items()} == {k: (tuple(v.shape), v.dtype) for k, v in ref.items()}
    ours.load_state_dict(ref)
    assert all(torch.equal(v, ref[k]) for k, v in ours.state_dict().items())


def test_constructor_options():
    from nunif_amd.nunif.utils.transnetv2 import TransNetV2
    for opt in ("use_convex_comb_reg", "use_resnet_features", "use_resnet_like_top", "frame_similarity_on_last_layer"):
        with pytest.raises(NotImplementedError):
            TransNetV2(**{opt: True})
    with pytest.raises(NotImplementedError, match="geometry"):
        TransNetV2(F=32)
    with pytest.raises(NotImplementedError, match="geometry"):
        TransNetV2(use_mean_pooling=True)
    m = TransNetV2()
    assert not m.training
    with pytest.raises(RuntimeError, match="size mismatch"):
        sd = m.state_dict()
        sd["fc1.bias"] = torch.zeros(3)
        m.load_state_dict(sd)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        m(torch.zeros(4, 3, 27, 48))


def test_load_without_a_file_names_the_path(tmp_path):
    from nunif_amd.nunif.utils.transnetv2 import TransNetV2, WEIGHTS_FILE
    with pytest.raises(FileNotFoundError) as e:
        TransNetV2().load(model_dir=str(tmp_path))
    assert os.path.join(str(tmp_path), "checkpoints", WEIGHTS_FILE) in str(e.value)


def test_load_reads_the_checkpoint_file(tmp_path, sd):
    from nunif_amd.nunif.utils.transnetv2 import TransNetV2, WEIGHTS_FILE
    os.makedirs(tmp_path / "checkpoints")
    torch.save(sd, str(tmp_path / "checkpoints" / WEIGHTS_FILE))
    m = TransNetV2().load(model_dir=str(tmp_path))
    assert torch.equal(m.state_dict()["fc1.weight"], sd["fc1.weight"])


def test_packed_weights_fold_batchnorm(sd):
    """The packed layout evaluated with plain matrix products equals the restatement's first DDCNN layer (float64)."""
    from nunif_amd.nunif.utils.transnetv2 import pack_weights
    packed = {k: v.double() for k, v in pack_weights(sd).items()}
    x = R.make_clip(20, 3, "cuts").double()                                             # [T,3,27,48]
    want = R.ddcnn({k: v.double() for k, v in sd.items() if v.is_floating_point()}, "SDDCNN.0.DDCNN.0.",
                   x.permute(1, 0, 2, 3).unsqueeze(0), True)[0]                         # [64,T,27,48]
    cols = torch.nn.functional.unfold(x, 3, padding=1).view(20, 3, 9, 27 * 48)          # [T,c,tap,pix]
    a = cols.permute(0, 3, 2, 1).reshape(20, 27 * 48, 27)                               # k = tap*3 + c
    s = a @ packed["b0.l0.ws"][:27]                                                     # [T,pix,128]
    out = []
    for i, d in enumerate((1, 2, 4, 8)):
        br = torch.nn.functional.pad(s[:, :, i * 32:(i + 1) * 32], (0, 0, 0, 0, d, d))
        g = torch.cat([br[j * d:j * d + 20] for j in range(3)], dim=2)                  # [T,pix,96]
        out.append((g @ packed["b0.l0.wt"][i])[:, :, :16])
    y = torch.relu(torch.cat(out, dim=2) + packed["b0.l0.bias"].double())
    got = y.permute(2, 0, 1).reshape(64, 20, 27, 48)
    assert (got - want).abs().max().item() < 1e-5 * max(1.0, want.abs().max().item())    # fp32 rounding of the folded weights


def test_histogram_is_degenerate_on_unit_range_and_real_on_bytes():
    x = R.case_frames("t100_cuts")
    h = R.color_histograms(x.unsqueeze(0) if x.ndim == 4 else x)
    assert torch.equal(h[..., 0], torch.ones_like(h[..., 0])) and h[..., 1:].abs().max() == 0
    band = R._band(h)
    t = 10
    assert torch.equal(band[0, t, 40:], torch.ones(61, dtype=band.dtype)) and band[0, t, :40].abs().max() == 0
    h8 = R.color_histograms(R.case_frames("t100_u8"))
    assert (h8 > 0).sum(dim=-1).min() > 1                     # several occupied bins per frame
    assert R._band(h8)[0, 50].min() < 0.9                     # and a similarity that really varies across a cut


class _Replay:
    """A detector model that records the frame indices of every window and replays the probabilities of fixture (b)."""

    def __init__(self, clip, probs):
        self.index = {clip[i].numpy().tobytes(): i for i in range(clip.shape[0])}
        self.probs, self.windows = probs, []

    def predict(self, x):
        self.windows.append([self.index[x[i].numpy().tobytes()] for i in range(x.shape[0])])
        return torch.from_numpy(self.probs[len(self.windows) - 1]).view(1, -1)


@pytest.mark.parametrize("n", R.DETECT_LENGTHS)
def test_boundary_detector_windowing_equals_the_reference(fixture, n):
    from nunif_amd.nunif.utils.shot_boundary_detection import BoundaryDetector
    clip = R.detect_clip(n)
    model = _Replay(clip, fixture[f"b/{n}/probs"])
    det = BoundaryDetector(model)
    for i in range(0, n, 25):
        j = min(i + 25, n)
        det.push(clip[i:j], [1000 + 40 * k for k in range(i, j)])
    got = det.finish()
    assert np.array_equal(np.asarray(model.windows, dtype=np.int32), fixture[f"b/{n}/windows"])
    assert sorted(got) == fixture[f"b/{n}/set"].tolist()


def test_boundary_detector_edges():
    from nunif_amd.nunif.utils.shot_boundary_detection import BoundaryDetector, detect_boundary
    det = BoundaryDetector(lambda x: (torch.zeros(1, x.shape[0], 1), {}))
    assert det.finish() == set()
    with pytest.raises(ValueError):
        det.push(torch.zeros(26, 3, 27, 48), list(range(26)))
    with pytest.raises(AssertionError):
        BoundaryDetector(None, window_size=100, padding_size=50)
    det = BoundaryDetector(lambda x: (torch.full((1, x.shape[0], 1), 3.0), {}))       # the reference's callable contract
    det.push(torch.zeros(3, 3, 27, 48), [5, 6, 7])
    assert det.finish() == {5, 6, 7}
    if not refstub.reference_available():
        with pytest.raises(RuntimeError, match="nunif.utils.video"):
            detect_boundary("x.mp4")


def test_abi_names_are_declared_and_bound():
    from nunif_amd import _hip
    header = open(os.path.join(ROOT, "include", "nunif_hip.h")).read()
    for name in ("nunif_hip_transnetv2_create", "nunif_hip_transnetv2_forward", "nunif_hip_transnetv2_destroy"):
        assert re.search(r"\b" + name + r"\s*\(", header) and name in _hip.SIGNATURES
