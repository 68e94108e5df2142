"""CPU: the swin_unet_v2 tap checks of ``test_gpu_swin_v2_errloc.py`` on the oracle alone (no GPU).

(a) ``swin_v2_cases.forward`` is ``oracle.swin_unet_v2.model_forward`` bit for bit, taps included, and the clean emulation passes
every tap of every net case with ratio <= 1.  (b) Nine mutations of that forward, each one a way ``v2_wattn_kernel``, the GLU, the
shortcut kernels, the packing of ``up1`` or the image head could be wrong, evaluated in float64 on the 2x net (seed 42, tile 64,
batch 1): each exceeds the TAP bound of the block it sits in (B_TAP 5.5 per region, with the tap's cells and channel group) by 10 x
or more.  The first one — the padded tokens of ONE shifted block taken as q / k / v = 0 instead of the qkv bias — passes the
output-only check of ``test_gpu_swin_errloc.py`` on the synthetic weights (every bias N(0, 0.02)); that is asserted too, so the gap
the taps close stays documented.  On the loud-bias weights (``qkv_proj.bias`` N(0, 0.5)) a padded key differs from zero by as much as
a real one, and the output sees it as well.  (c) The stand-alone attention: the four window mutations against the stand-alone
bound, and the conditions on its inputs — padded keys carry weight, no row is one-hot.  (d) The cells of a v2 tap.

Recorded when this was written (float64 mutation against the emulation's own error; tap limits 3.5 / 5.5, output limits 2.5 / 3.75):

    mutation                                          tap                  tap global / region   output global / region
    padded q/k/v zeroed in wac3.blocks.1              wac3.blocks.1.att    22.1 / 103.7          0.60 / 0.88   PASSES
      the same, loud-bias weights                     wac3.blocks.1.att    751 / 1398            27.7 / 46.9
    padded keys masked in wac2.blocks.0               wac2.blocks.0.att    972 / 2567            25.9 / 38.2
    bias table transposed in ir.path2.3               ir.path2.3.att       142 / 132             5.73 / 7.45
    head 0 reads head 1's V in wac1.blocks.1          wac1.blocks.1.att    1536 / 2230           76.8 / 100
    pad of ws/2 - 1 in wac1.blocks.0                  wac1.blocks.0.att    462 / 1423            23.9 / 32.9
    GLU halves swapped in wac3.blocks.0               wac3.blocks.0        294 / 557             118 / 157
    down1 shortcut over the wrong channel stride      down1                739 / 1331            180 / 229
    up1 sub-pixel order q <-> c                       up1                  330 / 602             178 / 218
    residual-image crop off by one                    residual             1060 / 1729           575 / 727

The attention alone (8, shifted, 16 x 24, C = 96, B = 3; limit 1): pad_zero 907 / 1420 (whole map / worst (window, head)),
pad_masked 958 / 1425, transposed 460 / 1271, head_v 928 / 2189.
"""
import pytest
import torch

import errloc as E
import swin_v2_cases as S
from conftest import psnr
from oracle import swin_unet_v2 as OV

CASE = (2, 64, 1, "synthetic")
LOUD = (2, 64, 1, "loud-bias")
TEN = 10.0

# name -> (net case, muts, the tap it is held to)
MUTATIONS = {
    "padded q/k/v zeroed in wac3.blocks.1": (CASE, {"wac3.blocks.1": ("pad_zero",)}, "wac3.blocks.1.att"),
    "padded q/k/v zeroed in wac3.blocks.1, loud bias": (LOUD, {"wac3.blocks.1": ("pad_zero",)}, "wac3.blocks.1.att"),
    "padded keys masked in wac2.blocks.0": (CASE, {"wac2.blocks.0": ("pad_masked",)}, "wac2.blocks.0.att"),
    "bias table transposed in ir.path2.3": (CASE, {"ir.path2.3": ("transposed",)}, "ir.path2.3.att"),
    "head 0 reads head 1's V in wac1.blocks.1": (CASE, {"wac1.blocks.1": ("head_v",)}, "wac1.blocks.1.att"),
    "pad of ws/2 - 1 in wac1.blocks.0": (CASE, {"wac1.blocks.0": ("pad_short",)}, "wac1.blocks.0.att"),
    "GLU halves swapped in wac3.blocks.0": (CASE, {"wac3.blocks.0": ("glu_swapped",)}, "wac3.blocks.0"),
    "down1 shortcut over the wrong channel stride": (CASE, {"net": ("down1_stride",)}, "down1"),
    "up1 sub-pixel order q <-> c": (CASE, {"net": ("up1_order",)}, "up1"),
    "residual-image crop off by one": (CASE, {"net": ("crop_off",)}, "residual"),
}


def test_the_restatement_is_the_oracle():
    for case in (CASE, (1, 64, 1, "synthetic")):
        scale = case[0]
        sd, x = S.state_dict(scale), S.make_input(64, 1)
        ta, tb = {}, {}
        assert torch.equal(S.forward(sd, x, scale, ta), OV.model_forward(sd, x, scale, taps=tb))
        assert list(ta) == list(tb) and all(torch.equal(ta[k], tb[k]) for k in ta)
    x, y64, ye, t64, te = S.references(CASE)
    t = {}
    assert torch.equal(S.forward64(S.state_dict(2), x, 2, t), y64) and all(torch.equal(t[k], t64[k]) for k in t64)


def test_tap_names_are_the_engine_layout():
    """The oracle fills the maps of ``HipSwinUNetV2Engine.tap_layout`` in its order and with its shapes (no GPU: the layout is host
    arithmetic on the state dict)."""
    from nunif_amd.waifu2x.models.swin_unet_v2 import HipSwinUNetV2Engine
    for case in S.NET_CASES:
        scale, tile, batch, _ = case
        x, y64, ye, t64, te = S.references(case)
        eng = HipSwinUNetV2Engine.__new__(HipSwinUNetV2Engine)
        sd = S.state_dict(scale)
        eng.scale_factor, eng.dims, eng.blocks = scale, (sd["unet.patch.weight"].shape[0], sd["unet.down1.conv.weight"].shape[0]), (2, 4, 3)
        layout = eng.tap_layout(batch, tile)
        assert [n for n, _ in layout] == list(t64) == list(te), case
        assert all(tuple(t64[n].shape) == s for n, s in layout), case
        assert len(layout) == 2 * 11 + 5 and set(E.v2_blocks()) == {n for n, _ in layout if n + ".att" in t64}


@pytest.mark.parametrize("case", S.NET_CASES, ids=S.case_id)
def test_clean_emulation_passes(case):
    x, y64, ye, t64, te = S.references(case)
    name = S.NAMES[case[0]]
    st = E.check_localised(ye, y64, ye, E.cells_for(name), E.A_OUT, E.B_OUT, E.TAU_OUT, label=S.case_id(case))
    assert st["worst"] <= 1.0
    for tap in t64:
        st = S.tap_stats(name, tap, te[tap], t64[tap], te[tap])
        E.assert_localised(st, E.A_TAP, E.B_TAP, st["_tau"], f"{S.case_id(case)} {tap}")
        assert st["worst"] <= 1.0 and st["global"] <= 1.0, tap
        assert float(t64[tap].abs().max()) > 0.0


def test_loud_bias_keeps_a_sane_emulation():
    """The redrawn biases do not blow the yardstick up: the emulation's output is still >= 50 dB from float64."""
    x, y64, ye, t64, te = S.references(LOUD)
    assert psnr(ye, y64) >= 50.0, psnr(ye, y64)
    assert not torch.equal(y64, S.references(CASE)[1])


def _mutated(case, muts):
    x, y64, ye, t64, te = S.references(case)
    t = {}
    y = S.forward64(S.state_dict(case[0], case[3]), x, case[0], t, muts)
    return y, t, (y64, ye, t64, te)


@pytest.mark.parametrize("name", list(MUTATIONS))
def test_mutation_exceeds_its_tap_bound_tenfold(name, capsys):
    case, muts, tap = MUTATIONS[name]
    y, t, (y64, ye, t64, te) = _mutated(case, muts)
    st = S.tap_stats(S.NAMES[case[0]], tap, t[tap], t64[tap], te[tap])
    so = E.localised_stats(y, y64, ye, E.cells_for(S.NAMES[case[0]]), E.B_OUT, E.TAU_OUT)
    with capsys.disabled():
        print(f"\n{name} [{case[3]}]: tap {tap} global {st['global']:.1f} worst region {st['worst']:.1f} (limits {E.A_TAP} / {E.B_TAP}); "
              f"output global {so['global']:.2f} worst region {so['worst']:.2f} (limits {E.A_OUT} / {E.B_OUT})")
    assert st["worst"] >= TEN * E.B_TAP, (name, st["worst"])


def test_one_block_with_zero_padded_tokens_passes_the_output_check(capsys):
    """The gap: on the synthetic weights the output-only check does not see ONE shifted block that takes its padded tokens for
    zero (global and per region below the EMULATION's own error), while that block's ``att`` tap is over its limit tenfold."""
    y, t, (y64, ye, t64, te) = _mutated(CASE, {"wac3.blocks.1": ("pad_zero",)})
    so = E.check_localised(y, y64, ye, E.cells_for(S.NAMES[2]), E.A_OUT, E.B_OUT, E.TAU_OUT, label="pad_zero output")
    st = S.tap_stats(S.NAMES[2], "wac3.blocks.1.att", t["wac3.blocks.1.att"], t64["wac3.blocks.1.att"], te["wac3.blocks.1.att"])
    with capsys.disabled():
        print(f"\npadded q/k/v zeroed in wac3.blocks.1 [synthetic]: output global {so['global']:.2f} worst region {so['worst']:.2f} "
              f"-> PASSES; tap global {st['global']:.1f} worst region {st['worst']:.1f}")
    assert so["global"] < 1.0 and so["worst"] < 1.0
    assert st["worst"] >= TEN * E.B_TAP


# ---- the attention alone ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", S.WATTN_CASES, ids=S.case_id)
def test_wattn_inputs_meet_their_conditions(case):
    """Padded keys carry at least 0.2 of the softmax weight for at least half of the inside queries of every border window (and
    head), no row's top weight exceeds 0.99, and the fp32 evaluation is itself inside the bound with k = 1."""
    ws, shift, H, W, C, B = case
    qkv, btab, bqkv, ref64, ref32h, w64 = S.wattn_references(case)
    assert float(w64.amax(-1).max()) <= 0.99
    inside = S.inside_mask(case)                                   # [nwy, nwx, N]
    border = ~inside.all(-1)
    assert bool(border.any()) == bool(shift)
    if shift:
        mass = (w64 * (~inside)[None, :, :, None, None, :]).sum(-1)                      # [B, nwy, nwx, heads, N]
        ok = ((mass >= 0.2) & inside[None, :, :, None, :]).sum(-1)
        need = (inside.sum(-1) + 1) // 2 * border                  # a window wholly inside the map has no padded key
        assert bool((ok >= need[None, :, :, None]).all()), (ok - need[None, :, :, None]).min()
    st = S.wattn_stats(case, ref32h, ref64, ref32h)
    assert st["global"] <= 1.0 / S.K_FP32 and st["worst"] <= 1.0 / S.K_FP32


@pytest.mark.parametrize("mut", ["pad_zero", "pad_masked", "transposed", "head_v"])
def test_wattn_mutation_is_caught_alone(mut, capsys):
    case = S.WATTN_CASES[2]                                        # 8, shifted, 16 x 24, C = 96, B = 3
    qkv, btab, bqkv, ref64, ref32h, w64 = S.wattn_references(case)
    got = S.wattn_ref(case, qkv, btab, bqkv, torch.float32, mut=(mut,))[0].half()
    st = S.wattn_stats(case, got, ref64, ref32h)
    with capsys.disabled():
        print(f"\nwattn alone, {mut}: global {st['global']:.1f} worst (window, head) {st['worst']:.1f} (limit 1)")
    assert st["global"] >= TEN and st["worst"] >= TEN


def test_wattn_window_layout_round_trip():
    for case in S.WATTN_CASES:
        ws, shift, H, W, C, B = case
        att = torch.randn(B, H, W, C)
        w = S.wattn_to_windows(case, att)
        inside = S.inside_mask(case)
        assert w.shape[1:3] == inside.shape[:2] and w.shape[3] == C // 32
        assert float((w.abs() * (~inside)[None, :, :, None, :, None]).max()) == 0.0
        assert torch.isclose(w.double().sum(), att.double().sum())
    assert float(S.half_ulp_fp16(torch.tensor(1.5))) == 2.0 ** -11 and float(S.half_ulp_fp16(torch.tensor(0.3))) == 2.0 ** -13


# ---- the cells ----------------------------------------------------------------------------------------------------------------------
def test_cells():
    name = S.NAMES[2]
    b = E.v2_blocks()
    assert list(b) == ["ir.path2.2", "ir.path2.3", "wac1.blocks.0", "wac1.blocks.1", "wac2.blocks.0", "wac2.blocks.1", "wac2.blocks.2",
                       "wac2.blocks.3", "wac3.blocks.0", "wac3.blocks.1", "wac3.blocks.2"]
    assert b["wac1.blocks.0"] == (8, True) and b["wac1.blocks.1"] == (6, False) and b["wac3.blocks.1"] == (8, True)
    assert [k for k, v in b.items() if v[1]] == ["ir.path2.2", "wac1.blocks.0", "wac2.blocks.0", "wac2.blocks.2", "wac3.blocks.1"]
    assert E.v2_tap_cells(name, "wac1.blocks.0.att") == ([(8, 4)], 32) and E.v2_tap_cells(name, "wac1.blocks.0") == ([(8, 4)], 16)
    assert E.v2_tap_cells(name, "wac1.blocks.1.att") == ([(6, 0)], 32) and E.v2_tap_cells(name, "wac2.blocks.1") == ([(8, 0)], 16)
    assert E.v2_tap_cells(name, "ir") == ([(16, 0)], 16) and E.v2_tap_cells(name, "residual") == (E.cells_for(name), None)
    # a window of 6 shifted (three first layers: get_shift_config(3) shifts block 1): cells start at -3
    assert E.v2_tap_cells(name, "wac1.blocks.1.att", E.v2_blocks(n1=2) | {"wac1.blocks.1": (6, True)}) == ([(6, 3)], 32)
    # both partitions are looked at, whatever the block's own: a planted error is reported in the window that holds it
    e = torch.zeros(1, 32, 24, 24)
    e[0, 5, 9, 13] = 1.0
    st = E.localised_stats(e, e * 0, e * 0 + 1e-3, [(8, 4)], E.B_TAP, 0.0, group=32)
    assert sorted({d["offset"] for d in st["regions"]}) == [0, 4]
    hit = [d for d in st["regions"] if d["ratio"] > 1.0]
    assert {(d["offset"], d["row"], d["col"]) for d in hit} == {(0, 1, 1), (4, 1, 2)}
