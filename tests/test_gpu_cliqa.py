"""cliqa on the HIP engine against float64 (tests/cliqa_f64.py, pinned to the reference classes by tests/golden/cliqa.npz).

Outputs, per case and head: ``max_b |y_hip - y64| <= 2.1 max_b |y_emu - y64| + floor``; y_emu is the reference's own fp16-autocast
arithmetic emulated on the CPU, the floor one fp16 ulp at ``max |y64|`` (the reference's result is stored in fp16).  Taps (the maps
behind the three pools, the head maps in front of the global pools): ``errloc`` per 8 x 8 cell of map positions, aligned and shifted
by 4 (1 x 1 where the map is smaller), limits 3.5 global / 5.5 per region, tau = TAP_TAU_REL x rms.  The measured ratios are printed
before they are asserted (figures: profiles/cliqa.txt)."""
import numpy as np
import pytest
import torch

import cliqa_f64 as C
import errloc as E

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GOLD = C.golden()
fp16_ulp, out_bound = C.fp16_ulp, C.out_bound
K_SCORE = 2.2
_models = {}


def model_for(kind, sd=None):
    import nunif_amd.cliqa.models as M
    cls = {"jpeg_quality": M.JPEGQuality, "grain_noise_level": M.GrainNoiseLevel, "scale_factor": M.ScaleFactor}[kind]
    if sd is not None:
        m = cls()
        m.load_state_dict(sd)
        return m.to(DEV)
    if kind not in _models:
        from nunif_amd.synthetic import cliqa_state_dict
        m = cls()
        m.load_state_dict(cliqa_state_dict(C.SEED[kind], kind))
        _models[kind] = m.to(DEV)
    return _models[kind]


def as_tuple(y):
    return tuple(y) if isinstance(y, (tuple, list)) else (y,)


def ref_outputs(kind, shape):
    _, _, y64, yemu, _, _ = C.references(kind, shape)
    if kind == "scale_factor":
        return tuple(torch.clamp(v, 1.0, 2.0) for v in y64), tuple(torch.clamp(v, 1.0, 2.0) for v in yemu)
    return y64, yemu


@pytest.mark.parametrize("kind", C.KINDS)
@pytest.mark.parametrize("shape", C.SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_outputs_and_taps_against_float64(kind, shape):
    _, x, _, _, t64, temu = C.references(kind, shape)
    y64, yemu = ref_outputs(kind, shape)
    m = model_for(kind)
    m.group = 8 if shape[0] > 8 else 0                             # B = 9: two groups
    try:
        outs, taps = m.debug_taps(x.to(DEV))
        plain = as_tuple(m(x.to(DEV)))
    finally:
        m.group = 0
    assert all(torch.equal(a, b) for a, b in zip(outs, plain)), "taps changed the outputs"
    for i, (y, a, e) in enumerate(zip(outs, y64, yemu)):
        assert y.shape == (shape[0], 1) and y.dtype == torch.float32
        err, bound = float((y.cpu().double() - a).abs().max()), out_bound(a, e)
        print(f"cliqa.{kind} {shape} head {i}: err {err:.3e} emu {float((e.double() - a).abs().max()):.3e} bound {bound:.3e} "
              f"ratio to bound {err / bound:.2f}")
        assert err <= bound, (kind, shape, i, err, bound)
    for n in C.TAPS:
        a = t64[n]
        cell = 8 if min(a.shape[2:]) >= 8 else 1
        tau = E.TAP_TAU_REL * float(a.double().pow(2).mean().sqrt())
        st = E.localised_stats(taps[n].cpu(), a, temu[n], [(cell, 0)], B=E.B_TAP, tau=tau)
        print(f"cliqa.{kind} {shape} tap {n}: {E.summary(st)}")
        E.assert_localised(st, E.A_TAP, E.B_TAP, tau, label=f"cliqa.{kind} {shape} {n}")


@pytest.mark.parametrize("kind", C.KINDS)
def test_batch_equals_single_patches_calls_and_streams(kind):
    x = C.net_input(kind, (3, 16, 24)).to(DEV)
    m = model_for(kind)
    whole = as_tuple(m(x))
    for b in range(3):
        one = as_tuple(m(x[b:b + 1]))
        assert all(torch.equal(o[0], w[b]) for o, w in zip(one, whole)), b
    assert all(torch.equal(a, b) for a, b in zip(as_tuple(m(x)), whole))
    s1, s2 = torch.cuda.Stream(DEV), torch.cuda.Stream(DEV)
    torch.cuda.synchronize()
    with torch.cuda.stream(s1):
        y1 = as_tuple(m(x))
    with torch.cuda.stream(s2):
        y2 = as_tuple(m(x))
    torch.cuda.synchronize()
    assert all(torch.equal(a, w) and torch.equal(b, w) for a, b, w in zip(y1, y2, whole))
    m.group = 2
    try:
        grouped = as_tuple(m(x))
    finally:
        m.group = 0
    assert all(torch.equal(a, w) for a, w in zip(grouped, whole))


@pytest.mark.parametrize("kind", C.KINDS)
def test_workspace_reuse_across_shapes(kind):
    m = model_for(kind)
    x = C.net_input(kind, (2, 128, 128)).to(DEV)
    first = as_tuple(m(x))
    m(C.net_input(kind, (2, 21, 30)).to(DEV))
    assert all(torch.equal(a, b) for a, b in zip(as_tuple(m(x)), first))


def test_scale_factor_eval_clamp_and_refusals():
    from nunif_amd.synthetic import cliqa_state_dict
    x = C.net_input("scale_factor", (3, 16, 24)).to(DEV)
    for shift, want in ((3.0, 2.0), (-3.0, 1.0)):
        sd = cliqa_state_dict(C.SEED["scale_factor"], "scale_factor")
        sd["scale_factor_output.4.bias"] = sd["scale_factor_output.4.bias"] + shift
        assert torch.equal(model_for("scale_factor", sd)(x), torch.full((3, 1), want, device=DEV))
    m = model_for("scale_factor")
    with pytest.raises(ValueError):
        m(torch.rand(1, 3, 7, 32, device=DEV))
    with pytest.raises(RuntimeError, match="inference-only"):
        m.train()(x)
    m.eval()
    # a workspace one byte short is refused before anything is launched
    import ctypes
    from nunif_amd import _hip
    eng, lib = m.engine(), _hip.lib()
    need = lib.nunif_hip_cliqa_workspace_bytes(eng.handle, 3, 16, 24, 0)
    assert need > 0 and lib.nunif_hip_cliqa_workspace_bytes(eng.handle, 3, 7, 24, 0) == 0
    ws = torch.empty((need,), dtype=torch.uint8, device=DEV)
    out = torch.empty((3, 1), device=DEV)
    with pytest.raises(_hip.NunifHipError, match="workspace"):
        eng.call(lib.nunif_hip_cliqa_forward, eng.handle, ctypes.c_void_p(x.data_ptr()), 3, 16, 24, 0, ctypes.c_void_p(ws.data_ptr()),
                 need - 1, ctypes.c_void_p(out.data_ptr()), ctypes.c_void_p(None))


@pytest.mark.parametrize("case", C.SELECT, ids=lambda c: "%dx%d_%d" % c)
def test_patch_selection(case):
    import nunif_amd.cliqa.utils as U
    t = "select.%dx%d.%d" % case
    img = C.select_image(case)
    s64, all_patches = C.std_scores64(img)
    assert np.array_equal(s64.numpy(), GOLD[t + ".scores"])
    patches, indices, scores = U.select_patches(img.to(DEV), case[2])
    e_ref = float((U.std_score(all_patches).double() - s64).abs().max())          # the fp32 torch expression
    e_hip = float((scores.cpu().double() - s64).abs().max())
    print(f"cliqa select {case}: score err {e_hip:.3e}, fp32 expression {e_ref:.3e}")
    assert e_hip <= K_SCORE * e_ref
    assert indices.cpu().tolist() == GOLD[t + ".indices"].tolist()
    assert torch.equal(patches.cpu(), all_patches[indices.cpu()])
    assert np.abs(C.digest(patches.cpu()) - GOLD[t + ".patches"]).max() <= 1e-12
    assert torch.equal(U.extract_patches(img.to(DEV), case[2]), patches)


def test_patch_selection_refuses_a_small_image():
    import nunif_amd.cliqa.utils as U
    with pytest.raises(ValueError, match="smaller than a patch"):
        U.extract_patches(torch.rand(3, 127, 300, device=DEV), 8)
    from PIL import Image
    small = Image.fromarray((np.random.RandomState(0).rand(100, 140, 3) * 255).astype(np.uint8))
    assert U.extract_patches(small, 8, device=DEV).shape == (1, 3, 128, 128)     # safe_pad on the host


def shifted(kind, key, value):
    from nunif_amd.synthetic import cliqa_state_dict
    sd = cliqa_state_dict(C.SEED[kind], kind)
    sd[key] = torch.tensor([value])
    return model_for(kind, sd)


def test_predict_functions():
    import nunif_amd.cliqa.utils as U
    shape = (2, 128, 128)
    # jpeg quality
    x = C.net_input("jpeg_quality", shape)
    y64, yemu = ref_outputs("jpeg_quality", shape)
    m = model_for("jpeg_quality")
    quality, prob = U.predict_jpeg_quality(m, x.to(DEV))
    want = GOLD["jpeg_quality.predict"]
    print("predict_jpeg_quality", quality, prob, want)
    assert isinstance(quality, float) and abs(quality - want[0]) <= out_bound(y64[0], yemu[0])
    assert abs(prob - want[1]) <= out_bound(y64[1], yemu[1])
    assert U.predict_jpeg_quality(shifted("jpeg_quality", "quality_output.4.bias", 500.0), x.to(DEV))[0] == 100.0
    assert U.predict_jpeg_quality(shifted("jpeg_quality", "quality_output.4.bias", -500.0), x.to(DEV))[0] == 0.0
    stack = torch.stack([x, C.net_input("jpeg_quality", (2, 128, 128)).flip(0), x.flip(3)]).to(DEV)       # [3, 2, 3, 128, 128]
    q, p = U.predict_jpeg_quality_batch(m, stack)
    assert q.shape == (3,) and p.shape == (3,)
    for i in range(3):
        qi, pi = U.predict_jpeg_quality(m, stack[i])
        assert qi == q[i].item() and pi == p[i].item()
    # grain noise
    x = C.net_input("grain_noise_level", shape)
    y64, yemu = ref_outputs("grain_noise_level", shape)
    m = model_for("grain_noise_level")
    psnr = U.predict_grain_noise_psnr(m, x.to(DEV))
    print("predict_grain_noise_psnr", psnr, GOLD["grain_noise_level.predict"])
    assert abs(psnr - GOLD["grain_noise_level.predict"][0]) <= out_bound(y64[0], yemu[0])
    assert U.predict_grain_noise_psnr(shifted("grain_noise_level", "noise_level_output.4.bias", 500.0), x.to(DEV)) == 0.0
    assert U.predict_grain_noise_psnr(shifted("grain_noise_level", "noise_level_output.4.bias", -500.0), x.to(DEV)) == 50.0
    stack = torch.stack([x, x.flip(2)]).to(DEV)
    b = U.predict_grain_noise_psnr_batch(m, stack)
    assert [U.predict_grain_noise_psnr(m, stack[i]) for i in range(2)] == b.tolist()
    # resize quality
    x = C.net_input("scale_factor", shape)
    y64, yemu = ref_outputs("scale_factor", shape)
    m = model_for("scale_factor")
    rq = U.predict_resize_quality(m, x.to(DEV))
    print("predict_resize_quality", rq, GOLD["scale_factor.predict"])
    assert isinstance(rq, int) and abs(rq - GOLD["scale_factor.predict"][0]) <= int(np.ceil(100 * out_bound(y64[0], yemu[0])))
    assert U.predict_resize_quality(shifted("scale_factor", "scale_factor_output.4.bias", 9.0), x.to(DEV)) == 0
    assert U.predict_resize_quality(shifted("scale_factor", "scale_factor_output.4.bias", -9.0), x.to(DEV)) == 100
    sf, q = U.predict_resize_quality_batch(m, torch.stack([x, x.flip(3)]).to(DEV))
    assert [U.predict_resize_quality(m, v.to(DEV)) for v in (x, x.flip(3))] == q.tolist()
    assert fp16_ulp(1.5) == 2.0 ** -10
