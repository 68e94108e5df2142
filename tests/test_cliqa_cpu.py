"""cliqa without a GPU: the float64 restatement (tests/cliqa_f64.py) against the reference classes' recorded results
(tests/golden/cliqa.npz), the BatchNorm fold of ``pack_weights``, the state-dict key layout and ``predict_*`` signatures against the
live reference where it is mounted, the selection inputs' score gaps, and four mutations of the restatement that the GPU tests'
output bound must tell from the right net."""
import ast
import inspect
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import cliqa_f64 as C
from oracle import refstub
from nunif_amd.cliqa.models import _net
from nunif_amd.synthetic import cliqa_state_dict

needs_reference = pytest.mark.skipif(not refstub.reference_available(), reason="the reference checkout is not mounted here")
GOLD = C.golden()
out_bound = C.out_bound


def tag(kind, shape):
    return f"{kind}.{shape[0]}x{shape[1]}x{shape[2]}"


def close(a, b, rel):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return np.abs(a - b).max() <= rel * max(np.abs(b).max(), 1e-300)


@pytest.mark.parametrize("kind", C.KINDS)
@pytest.mark.parametrize("shape", C.SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_float64_restatement_equals_the_reference_classes(kind, shape):
    sd, x, y64, _, t64, _ = C.references(kind, shape)
    t = tag(kind, shape)
    assert close(C.digest(x), GOLD[t + ".x"], 0.0)
    if kind == "scale_factor":
        assert close(y64[0].numpy(), GOLD[t + ".raw"], 1e-12)
        assert close(torch.clamp(y64[0], 1.0, 2.0).numpy(), GOLD[t + ".out0"], 1e-12)
    else:
        for i, y in enumerate(y64):
            assert close(y.numpy(), GOLD[f"{t}.out{i}"], 1e-12), (t, i)
    for n in C.TAPS:
        assert close(C.digest(t64[n]), GOLD[f"{t}.{n}"], 1e-12), (t, n)
    if shape in C.WHOLE_TAP_SHAPES:                                  # element by element, to the fixture's float32 storage
        whole = np.load(C.GOLDEN_TAPS % kind)
        for n in C.TAPS:
            ref = whole[f"{t}.{n}"]
            assert ref.dtype == np.float32 and ref.shape == tuple(t64[n].shape)
            assert np.array_equal(t64[n].float().numpy(), ref), (t, n)


@pytest.mark.parametrize("kind", C.KINDS)
def test_fp32_restatement_is_within_its_own_rounding(kind):
    shape = (2, 21, 30)
    sd, x, y64, _, _, _ = C.references(kind, shape)
    with torch.inference_mode():
        y32 = C.forward(sd, x, kind, clamp=False)
    for a, b in zip(y32, y64):
        # seven convs of up to 1152 products in series, fp32: a relative 1e-4 of the output is loose by an order of magnitude
        assert float((a.double() - b).abs().max()) <= 1e-4 * float(b.abs().max())


@pytest.mark.parametrize("kind", C.KINDS)
def test_pack_weights_fold_equals_conv_then_batchnorm(kind):
    sd = {k: (v.double() if v.is_floating_point() else v) for k, v in cliqa_state_dict(C.SEED[kind], kind).items()}
    g = torch.Generator().manual_seed(3)
    layers = list(_net.TRUNK) + [(None, h + ".0", h + ".1", 128, 256) for h in C.HEADS[kind]]
    for _, conv, bn, cin, _ in layers:
        w, b = _net.fold_bn(sd, conv, bn)
        x = torch.randn((2, w.shape[1], 7, 9), generator=g, dtype=torch.float64)
        want = C._conv_bn(sd, conv, bn, x, "constant")
        got = F.conv2d(x, w, b, padding=1)
        assert float((got - want).abs().max()) <= 1e-12 * float(want.abs().max()), conv
    kind2, packed = _net.pack_weights(cliqa_state_dict(C.SEED[kind], kind))
    assert kind2 == kind and all(v.dtype == torch.float32 and v.is_contiguous() for v in packed.values())
    w, b = _net.fold_bn(sd, "features.3", "features.4")
    assert torch.equal(packed["conv2.w"], w.float()) and torch.equal(packed["conv2.b"], b.float())


def test_synthetic_batchnorm_is_not_the_identity():
    for kind in C.KINDS:
        sd = cliqa_state_dict(C.SEED[kind], kind)
        for k, v in sd.items():
            if k.endswith(("running_mean", "running_var")) or (k.endswith((".weight", ".bias")) and v.dim() == 1 and v.numel() > 1):
                assert float(v.float().std()) > 0.01, k
        assert list(sd) == list(_net.state_dict_shapes(kind))


@pytest.mark.parametrize("kind", C.KINDS)
def test_model_surface(kind):
    import nunif_amd.cliqa.models as M
    from nunif_amd.nunif.models import create_model
    cls = {"jpeg_quality": M.JPEGQuality, "grain_noise_level": M.GrainNoiseLevel, "scale_factor": M.ScaleFactor}[kind]
    m = create_model("cliqa." + kind)
    assert type(m) is cls and not m.training
    assert {k: tuple(v.shape) for k, v in m.state_dict().items()} == dict(_net.state_dict_shapes(kind))
    sd = cliqa_state_dict(C.SEED[kind], kind)
    m.load_state_dict(sd)
    back = m.state_dict()
    assert list(back) == list(sd) and all(torch.equal(back[k], sd[k]) for k in sd)
    assert back["features.1.num_batches_tracked"].dtype == torch.long
    x = C.net_input(kind, (1, 8, 8))
    assert torch.equal(cls.preprocess(x), C.preprocess(kind, x))
    with pytest.raises(RuntimeError, match="inference-only"):
        m.train()(x)
    with pytest.raises(RuntimeError, match="ROCm device"):
        m.eval()(x)                                              # no CPU fallback
    assert _net.detect_kind(sd.keys()) == kind


@needs_reference
@pytest.mark.parametrize("kind", C.KINDS)
def test_key_layout_equals_the_live_reference_and_a_pth_round_trips(kind, tmp_path):
    refstub.install()
    import cliqa.models as RM
    import nunif_amd.cliqa.models as M
    name = {"jpeg_quality": "JPEGQuality", "grain_noise_level": "GrainNoiseLevel", "scale_factor": "ScaleFactor"}[kind]
    ref, ours = getattr(RM, name)(), getattr(M, name)()
    assert ref.name == ours.name
    rsd = ref.state_dict()
    assert [(k, tuple(v.shape), v.dtype) for k, v in rsd.items()] == [(k, tuple(v.shape), v.dtype) for k, v in ours.state_dict().items()]
    sd = cliqa_state_dict(C.SEED[kind], kind)
    ref.load_state_dict(sd)
    torch.save(ref.state_dict(), tmp_path / "ref.pth")
    ours.load_state_dict(torch.load(tmp_path / "ref.pth", weights_only=True))
    torch.save(ours.state_dict(), tmp_path / "ours.pth")
    ref2 = getattr(RM, name)()
    ref2.load_state_dict(torch.load(tmp_path / "ours.pth", weights_only=True))
    assert all(torch.equal(ref2.state_dict()[k], sd[k]) for k in sd)
    assert inspect.signature(getattr(RM, name).preprocess) == inspect.signature(getattr(M, name).preprocess)


@needs_reference
def test_predict_signatures_equal_the_reference_source():
    """``cliqa.utils`` imports torchvision: its signatures are read from the source, not by importing it."""
    import nunif_amd.cliqa.utils as U

    def sigs(path):
        tree = ast.parse(open(path).read())
        return {f.name: ast.unparse(f.args) for f in tree.body if isinstance(f, ast.FunctionDef)}
    ref = sigs(os.path.join(refstub.REFERENCE_ROOT, "cliqa", "utils.py"))
    ours = sigs(U.__file__)
    for fn in ("predict_jpeg_quality", "predict_grain_noise_psnr", "predict_resize_quality", "std_score", "safe_pad"):
        assert ref[fn] == ours[fn], fn
    assert ours["extract_patches"].startswith(ref["extract_patches"])      # plus the trailing `device=None`
    assert U.PATCH_SIZE == 128


# the first conv's padding is checked on the 8 x 8 case, where every pixel lies on the border or next to it
MUTATIONS = (("zero_pad_first", (1, 8, 8)), ("replicate_later", (3, 16, 24)), ("ceil_pool", (2, 21, 30)), ("max_subsampling", (3, 16, 24)))


@pytest.mark.parametrize("mutate,shape", MUTATIONS, ids=[m for m, _ in MUTATIONS])
def test_the_output_bound_tells_a_mutated_net(mutate, shape):
    kind = "jpeg_quality"
    sd, x, y64, yemu, _, _ = C.references(kind, shape)
    with torch.inference_mode():
        ymut = C.forward64(sd, x, kind, mutate=mutate, clamp=False)
    ratios = [float((m - a).abs().max()) / out_bound(a, e) for m, a, e in zip(ymut, y64, yemu)]
    print(mutate, ratios)
    assert max(ratios) >= 10.0, (mutate, ratios)


@pytest.mark.parametrize("case", C.SELECT, ids=lambda c: "%dx%d_%d" % c)
def test_selection_inputs_have_a_score_gap(case):
    t = "select.%dx%d.%d" % case
    scores, _ = C.std_scores64(C.select_image(case))
    assert close(scores.numpy(), GOLD[t + ".scores"], 1e-12)
    order = torch.argsort(scores, descending=True)
    k = min(case[2], scores.numel())
    assert order[:k].tolist() == GOLD[t + ".indices"].tolist()
    s = scores[order]
    for i in range(min(k, s.numel() - 1)):                         # every neighbour down to the (K+1)-th
        assert float((s[i] - s[i + 1]) / s[i]) >= 1e-3, (case, i)
    rows, cols = case[0] // C.PATCH, case[1] // C.PATCH
    assert scores.numel() == rows * cols


def test_host_side_refusals():
    import nunif_amd.cliqa.utils as U
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        U.select_patches(torch.rand(3, 128, 128), 8)
    with pytest.raises(NotImplementedError):
        U.extract_patches(torch.rand(3, 128, 128), 8, score_fn=lambda p: p)
    a = U.safe_pad(np.arange(5 * 7 * 3, dtype=np.uint8).reshape(5, 7, 3), 8)
    assert a.shape == (8, 8, 3) and (a[5] == a[3]).all() and (a[:, 7] == a[:, 5]).all()
    p = torch.rand(4, 3, 16, 16)
    assert torch.equal(U.std_score(p), torch.std(p, dim=[2, 3]).mean(dim=1))
