"""CPU: ``tests/errloc.py`` on the light inpaint nets (``inpaint.light_inpaint_v1``, ``inpaint.light_video_inpaint_v1*``), the
fp16-autocast emulation standing in for the engine.

The counterpart of ``test_gpu_inpaint_errloc.py`` for ``csrc/light_inpaint.hip``.  (a) The inputs of ``tests/inpaint_cases.py`` are fit:
the reference alone shows that the masks let the net through in every cell and that no token decision sits on its threshold.  (b) The
clean emulation passes every case with ratio <= 1, outputs and taps.  (c) Eleven mutations of the forward, each one a way a kernel of
the engine could be wrong, are applied to a restatement of the oracle path (``_net`` below, bit-equal to the oracle without a mutation)
and run under the emulation: the check the GPU test makes, outputs (A_OUT / B_OUT / TAU_OUT) or taps (A_TAP / B_TAP, tau = 2e-3 rms),
fails for every one.  Recorded when this was written (seeded weights; global / worst-region ratio, limit 2.5 / 3.75 for the output
and 3.5 / 5.5 for a tap; "first tap" = the first map in engine order that fails):

    mutation (case)                                              output            first failing tap, its ratios
    proj_spatial transposed in enc2.1 (image 1x100x180)          76.4 / 84.2       enc2.1.gmlp   181 / 189
    proj_spatial transposed in dec1 (image 1x100x180)            8.3 / 9.7         dec1.gmlp     8.4 / 9.7
    dec1 mixing bias rotated by one token (image 1x100x180)      3.5 / 4.3         dec1.gmlp     7.2 / 8.6
    enc1 shifted block replicate- instead of zero-padded         225 / 260         enc1.gmlp     756 / 915
    enc1 padded tokens left out of the mixing                    150 / 197         enc1.gmlp     709 / 804
    last window of dec1 skipped (image 1x63x65)                  2.4 / 4.1         dec1.gmlp     8.0 / 8.8
    GLU halves swapped in enc2.2 (image 1x100x180)               211 / 225         enc2.2        340 / 379
    enc1 shortcut counted once (image 1x100x180)                 173 / 184         enc1.gmlp     627 / 734
    temporal matrix transposed in enc2.1 (small 12x40x56)        29.4 / 84.2       enc2.1.gmlp   107 / 182
    token rule "all 16 pixels" (image 1x100x180 close)           327 / 498         patch 3689 / 4909; mtok differs
    mirror_x applied to the mask too (image 1x100x180 flip)      336 / 511         patch 2325 / 3039; hard, soft, mtok differ

The late defects are the narrow ones: the dec1 bias rotation reads 3.5 / 4.3 at the output (on a 1 x 100 x 180 comb input with
other strips the output check reads 2.24 / 2.95, a pass) and a skipped last window 2.4 / 4.1, the global bound passing; the
``dec1.gmlp`` tap holds both at twice its limits, and for every mutation the first failing tap is the mutated block's own: nothing
upstream fails.
"""
import pytest
import torch
import torch.nn.functional as F

import errloc as E
import inpaint_cases as S
from oracle import light_inpaint as OL
from oracle.fp16_emulation import fp16_autocast_emulation, half_weights


# ---- (a) the inputs ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", S.CASES, ids=S.case_id)
def test_inputs_are_fit(case):
    net, shape, flip, regime, pre, masks = case
    ref = S.references(case)
    x, y64, t64 = ref["x"], ref["y64"], ref["taps64"]
    hard, soft = t64["hard"], t64["soft"]
    assert y64.dtype == torch.float64 and y64.shape == x.shape and hard.dtype == soft.dtype == torch.float32
    assert 0.05 <= float(x.min()) and float(x.max()) <= 0.95 and (x.numel() == 3 or float(x.std()) > 0.1)    # not saturated, not flat
    if shape[0] == 12:                                                                            # the frames differ: the temporal mixing matters
        assert min(float((x[i] - x[i + 1]).abs().mean()) for i in range(11)) > 0.05
        assert all(not torch.equal(ref["mask"][i], ref["mask"][i + 1]) for i in range(11))
    frac = S.masked_fraction(hard)
    for i, kind in enumerate(S.mask_kinds(case)):
        if kind == "comb":
            assert 0.2 <= float(frac[i]) <= 0.6, (i, float(frac[i]))
            assert float(S.masked_fraction(hard, padded=True)[i]) <= 0.6
            # every (64, 64) cell, the partial ones included, shows the net at full weight somewhere
            assert float(F.max_pool2d(soft[i:i + 1], 64, 64, ceil_mode=True).min()) >= 0.5
        else:
            assert float(frac[i]) == (1.0 if kind == "all" else 0.0)
    # the hot weights drive 11.8 % of the picture into the clamp: that is the regime, not the input (its outputs are judged mostly
    # outside the clamp by the taps); a bound of its own so that a drift is noticed
    assert float(((y64 == 0) | (y64 == 1)).float().mean()) <= (0.15 if regime == "hot" else 0.01)
    # the token decision max(soft) > 0.99: a non-hole pixel's soft value stays below about 0.977, so it equals "any hole pixel in the
    # token", and no token is near the threshold
    h, w = soft.shape[2:]
    tmax = F.max_pool2d(F.pad(soft, (0, 64 - w % 64, 0, 64 - h % 64), mode="replicate"), 4)
    assert float((tmax - 0.99).abs().min()) >= 0.005
    assert torch.equal(tmax > 0.99, t64["mtok"]) and torch.equal(t64["mtok"], ref["tapse"]["mtok"])
    assert torch.equal(t64["mtok"], F.max_pool2d(F.pad(hard, (0, 64 - w % 64, 0, 64 - h % 64), mode="replicate"), 4) > 0)
    assert torch.equal(soft, ref["tapse"]["soft"]) and torch.equal(hard, ref["tapse"]["hard"])    # fp32 in every precision


def test_cases_take_the_paths_they_are_for():
    assert S.conv_patches((3, 100, 200)) == 24 and S.conv_patches((1, 270, 480)) == 40 and S.conv_patches((1, 270, 480), 2) == 10
    assert S.conv_patches((12, 40, 56)) == 24 and S.conv_patches((12, 72, 136)) == 96
    b, h, w = S.BIGGEST[1]
    t1 = b * (h + 64 - h % 64) * (w + 64 - w % 64) // 16
    assert t1 // 256 >= 128 and t1 // 4 >= 16384 and t1 >= 32768 and S.conv_patches(S.BIGGEST[1]) == 256
    assert h // 64 == w // 64 == 15 and min(h, w) == 960, "960 is the smallest side that pads to 1024"
    assert S.case_id(S.DMA_CASE) == "image-1x270x480" and S.case_id(S.BIGGEST) == "image-1x960x961"
    assert E.cells_for(S.IMAGE) == [((64, 64), (0, 0)), ((32, 128), (0, 0))] == E.cells_for(S.LARGE)
    assert E.cells_for(S.IMAGE, level=1) == [((16, 16), (0, 0)), ((8, 32), (0, 0))]
    assert E.cells_for(S.SMALL, level=2) == [((8, 8), (0, 0)), ((8, 32), (0, 0))]
    assert len({S.case_id(c) for c in S.CASES}) == len(S.CASES)


# ---- (b) the clean emulation ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", S.CASES, ids=S.case_id)
def test_clean_emulation_passes(case):
    net = case[0]
    ref = S.references(case)
    st = E.assert_localised(S.output_stats(ref["ye"], ref, net), E.A_OUT, E.B_OUT, E.TAU_OUT, label=S.case_id(case))
    assert st["worst"] <= 1.0 and st["global"] <= 1.0
    assert set(ref["taps64"]) == {n for n, _ in S.tap_names(net)} | {"hard", "soft", "mtok"}
    for name, level in S.tap_names(net):
        t64, te = ref["taps64"][name], ref["tapse"][name]
        assert t64.dtype == torch.float64 and t64.shape == te.shape and t64.shape[0] == case[1][0]
        st = E.assert_localised(S.tap_stats(te, t64, te, net, level), E.A_TAP, E.B_TAP, S.tau_for(t64), label=name)
        assert st["worst"] <= 1.0 and st["global"] <= 1.0


# ---- (c) a restatement of the oracle path with the mutations ------------------------------------------------------------------------
def _gmlp(sd, p, x, ws, shift, mut):
    """``oracle.light_inpaint.window_gmlp`` (``ws`` = 0: ``temporal_gmlp``) with hooks: proj_out(...) + the gMLP's own shortcut."""
    pad = ws // 2 if shift else 0
    xin = x
    if pad:
        x = F.pad(x, (pad,) * 4, mode="replicate" if "replicate_pad" in mut else "constant")
    shape = x.shape
    if ws:
        t = OL._windows(x, ws)
    else:
        T, C, H, W = x.shape
        t = x.permute(2, 3, 0, 1).reshape(H * W, T, C)
    a = F.gelu(F.linear(OL._ln(t, sd[p + "norm1.weight"]), sd[p + "gmlp.gmlp.proj_in.weight"], sd[p + "gmlp.gmlp.proj_in.bias"]))
    if pad and "absent" in mut:                                        # padded tokens contribute nothing: proj_in(0) taken as 0
        a = a * OL._windows(F.pad(torch.ones_like(xin[:, :1]), (pad,) * 4), ws)
    u, v = a.chunk(2, dim=-1)
    ws_w, ws_b = sd[p + "gmlp.gmlp.proj_spatial.weight"], sd[p + "gmlp.gmlp.proj_spatial.bias"]
    if "spatial_T" in mut:
        ws_w = ws_w.transpose(0, 1).contiguous()
    if "bias_rot" in mut:
        ws_b = torch.roll(ws_b, 1)
    v = F.conv1d(OL._ln(v, sd[p + "norm2.weight"]), ws_w, ws_b)
    po = F.linear(u * v, sd[p + "gmlp.gmlp.proj_out.weight"], sd[p + "gmlp.gmlp.proj_out.bias"])
    if "skip_last" in mut:
        po = torch.cat([po[:-1], torch.zeros_like(po[-1:])])
    t = po + t
    if ws:
        x = OL._unwindows(t, shape, ws)
        x = x[:, :, pad:x.shape[2] - pad, pad:x.shape[3] - pad] if pad else x
    else:
        x = t.reshape(H, W, T, C).permute(2, 3, 0, 1)
    return x


def _block(sd, p, x, ws, shift, muts, taps):
    mut = muts.get(p[:-1], ())
    g = _gmlp(sd, p, x, ws, shift, mut)
    x = (g if "one_shortcut" in mut else x + g)
    taps[p + "gmlp"] = x
    y = F.conv2d(x, sd[p + "glu_conv.w1.weight"], sd[p + "glu_conv.w1.bias"])
    if "glu_swap" in mut:
        y = torch.cat(y.chunk(2, dim=1)[::-1], dim=1)
    y = F.glu(y, dim=1)
    x = x + F.conv2d(F.pad(y, (1, 1, 1, 1), mode="replicate"), sd[p + "glu_conv.w2.weight"], sd[p + "glu_conv.w2.bias"])
    taps[p[:-1]] = x
    return x


def _net(sd, net, xp, soft, muts, taps):
    """``oracle.light_inpaint.forward`` / ``video_forward`` on the pre-processed frames; ``muts``: {block or "net": mutation names}."""
    video = net != S.IMAGE
    H, W = xp.shape[2:]
    pad1, pad2 = 64 - W % 64, 64 - H % 64
    x = F.pad((xp - 0.5) / 0.5, (0, pad1, 0, pad2), mode="replicate")
    mp = F.pad(soft, (0, pad1, 0, pad2), mode="replicate")
    mt = F.pixel_unshuffle(mp, 4)
    taps["mtok"] = mtok = (mt.amin(dim=1, keepdim=True) if "all16" in muts.get("net", ()) else mt.amax(dim=1, keepdim=True)) > 0.99
    if video:
        x = F.leaky_relu(F.conv2d(x, sd["patch.weight"], sd["patch.bias"], stride=4), 0.1)
    else:
        x = F.leaky_relu(F.conv2d(F.pixel_unshuffle(x, 4), sd["patch.0.weight"], sd["patch.0.bias"]), 0.2)
    taps["patch"] = x = torch.where(mtok, sd["mask_bias"], x)
    x1 = _block(sd, "enc1.", x, 16, not video, muts, taps)
    taps["down"] = x2 = F.conv2d(x1, sd["down.weight"], sd["down.bias"], stride=2)
    kinds = ("s1", "t", "s0", "t", "s1") if video else ("s0", "s1", "s0", "s1")
    for i, kind in enumerate(kinds):
        x2 = _block(sd, f"enc2.{i}.", x2, 0 if kind == "t" else 8, kind == "s1", muts, taps)
    taps["up"] = x = x1 + F.pixel_shuffle(F.conv2d(x2, sd["up.weight"], sd["up.bias"]), 2)
    x = _block(sd, "dec1.", x, 16, False, muts, taps)
    if video:
        taps["to_image"] = x = F.conv2d(x, sd["to_image.weight"], sd["to_image.bias"])
    else:
        taps["to_image"] = x = F.conv2d(F.pad(x, (1, 1, 1, 1), mode="replicate"), sd["to_image.1.weight"], sd["to_image.1.bias"])
    y = F.pixel_shuffle(x, 4)[:, :, :H, :W]
    return (xp * (1 - soft) + y * soft).clamp(0, 1)


def _run(case, muts, emulate=True, flip_mask=False):
    """(y, taps) of the restated forward of a case, under the emulation (as ``errloc.emulated`` runs the oracle) or in fp32."""
    net, shape, flip = case[:3]
    ref = S.references(case)
    sd, x = S.state_dict(net, case[3]), ref["x"]
    xm = torch.flip(x, (3,)) if flip else x
    taps = {}
    xp, soft = E.inpaint_preprocess(xm.float(), torch.flip(ref["mask"], (3,)) if flip_mask else ref["mask"], ref["pre"], taps)
    if not emulate:
        return _net(sd, net, xp, soft, muts, taps), taps
    with fp16_autocast_emulation():
        return _net(half_weights(sd), net, xp, soft, muts, taps), taps


@pytest.mark.parametrize("case", [S.MAIN_CASE, S.IMAGE_CASES[2], S.MAIN_VIDEO_CASE, S.VIDEO_CASES[3]], ids=S.case_id)
def test_the_restatement_is_the_oracle(case):
    """Without a mutation ``_net`` computes what the oracle computes, bit for bit, in fp32 and under the emulation, taps included."""
    net, ref = case[0], S.references(case)
    y, taps = _run(case, {})
    assert torch.equal(y, ref["ye"])
    for name, _ in S.tap_names(net):
        assert torch.equal(taps[name], ref["tapse"][name]), name
    y32, _ = _run(case, {}, emulate=False)
    fn = OL.infer if net == S.IMAGE else OL.video_infer
    assert torch.equal(y32, fn(S.state_dict(net), ref["x"], ref["mask"], **ref["pre"]))


FLIP_CASE, CLOSE_CASE = S.IMAGE_CASES[7], S.IMAGE_CASES[10]
# name -> (case, mutations, the tap that must hold it or None, flip the mask)
MUTATIONS = {
    "proj_spatial transposed in enc2.1": (S.MAIN_CASE, {"enc2.1": ("spatial_T",)}, "enc2.1.gmlp", False),
    "proj_spatial transposed in dec1": (S.MAIN_CASE, {"dec1": ("spatial_T",)}, "dec1.gmlp", False),
    "dec1 mixing bias rotated by one token": (S.MAIN_CASE, {"dec1": ("bias_rot",)}, "dec1.gmlp", False),
    "enc1 shifted block replicate-padded": (S.MAIN_CASE, {"enc1": ("replicate_pad",)}, "enc1.gmlp", False),
    "enc1 padded tokens left out of the mixing": (S.MAIN_CASE, {"enc1": ("absent",)}, "enc1.gmlp", False),
    "last window of dec1 skipped": (S.IMAGE_CASES[2], {"dec1": ("skip_last",)}, "dec1.gmlp", False),
    "GLU halves swapped in enc2.2": (S.MAIN_CASE, {"enc2.2": ("glu_swap",)}, "enc2.2", False),
    "enc1 shortcut counted once": (S.MAIN_CASE, {"enc1": ("one_shortcut",)}, "enc1.gmlp", False),
    "temporal matrix transposed in enc2.1": (S.MAIN_VIDEO_CASE, {"enc2.1": ("spatial_T",)}, "enc2.1.gmlp", False),
    # (the plain combs are token-aligned: "all" and "any" agree on them; the dilated strips of the closing case are 7 pixels wide)
    "token rule all 16 pixels": (CLOSE_CASE, {"net": ("all16",)}, None, False),
    "mirror_x applied to the mask too": (FLIP_CASE, {}, None, True),
}


def _fails(st, A, B, tau):
    try:
        E.assert_localised(st, A, B, tau)
    except AssertionError:
        return True
    return False


@pytest.mark.parametrize("name", list(MUTATIONS))
def test_mutation_is_caught(name, capsys):
    case, muts, tap, flip_mask = MUTATIONS[name]
    net, ref = case[0], S.references(case)
    assert (S.case_id(FLIP_CASE), S.case_id(CLOSE_CASE)) == ("image-1x100x180-flip", "image-1x100x180-close")
    y, taps = _run(case, muts, flip_mask=flip_mask)
    assert not torch.equal(y, ref["ye"])
    st = S.output_stats(y, ref, net)
    out_caught = _fails(st, E.A_OUT, E.B_OUT, E.TAU_OUT)
    exact = [n for n in ("hard", "soft", "mtok") if not torch.equal(taps[n], ref["taps64"][n])]
    first = None
    for n, level in S.tap_names(net):
        ts = S.tap_stats(taps[n], ref["taps64"][n], ref["tapse"][n], net, level)
        if _fails(ts, E.A_TAP, E.B_TAP, S.tau_for(ref["taps64"][n])):
            first = (n, ts["global"], ts["worst"])
            break
    with capsys.disabled():
        print(f"\n{name} ({S.case_id(case)}): output {st['global']:.1f} / {st['worst']:.1f} {'caught' if out_caught else 'PASS'}; "
              + (f"first failing tap {first[0]} {first[1]:.1f} / {first[2]:.1f}" if first else "no fp16 tap fails")
              + (f"; exact taps that differ: {exact}" if exact else ""))
    assert out_caught or first or exact, name
    if tap is not None:
        assert first is not None and first[0] == tap, (name, first)              # the taps name the block: nothing upstream fails
    else:
        assert exact, name
