"""CPU: ``tests/errloc.py`` on the iw3 depth path (``iw3.depth_anything``, ``iw3.depth_aa``), the fp16-autocast emulation standing in
for the engine.

The counterpart of ``test_errloc_sidenet.py`` for ``csrc/depth_anything.hip`` / ``depth_mlp.hip`` / ``conv3_lds.hip`` / ``depth_aa.hip`` /
``wa_block.hip``, pinned on FINAL OUTPUTS only (``tests/depth_cases.py``: the cases and what each one meets).

(a) Conditions on the inputs.  The bound divides by the emulation's own error per region, so it needs that error to be a usable
yardstick everywhere: for every depth-engine case and every partition ((14, 14) / (56, 56) / (8, 32), aligned and shifted by half
a cell) every region's noise is above 0, the largest region noise is at most 10x the smallest (measured: at most 7.3x, (8, 32) of
the taps 8-11 variant; 6.4x for (14, 14)), and no pixel of a ReLU head's output is exactly 0 — so the bound carries no exception
list.  DepthAA's output is the input depth plus a small edit and the emulation's error there is the fp16 rounding of that sum, one
ulp of the depth VALUE: the ``synth_depth`` maps are near 0 along their border and near 1 inside, so the quietest (16, 16) region
(a 1 x 8 pixel corner sliver) is up to 61x quieter than the loudest.  A seed does not mend that: over the seeds 0..19 of ``synth_depth``
the spread is 13.4x at best (median 51x) at 2 x 33 x 47, 11.2x (23x) at 31 x 95 and 20.6x (54x) at 3 x 64 x 80; only the two
one-window shapes stay below 10x (2.1x / 5.1x at worst).  For DepthAA the test therefore asserts
noise > 0 per region and that the quiet regions are governed by the relative floor of the side nets (tau = TAP_TAU_REL x rms is above
the WHOLE map's noise there), not by a division.
(b) The fp32 oracle passes with a worst ratio below 0.05; the emulation against itself gives exactly 1.
(c) Mutations, each a way a kernel could be wrong, applied by wrapping what the oracle module calls (``ODA.torch.softmax``,
``ODA.F.linear`` / ``interpolate`` / ``conv2d``, ``ODA.interpolate_pos_embed``; ``ODAA.F.pad``, ``ODAA.RF.window_mha`` /
``window_score_bias``: the oracle's own text stays untouched) and run under the fp16 emulation, so they carry realistic noise on top
of the defect.  Each must fail ``check_localised``; beside each the test prints whether today's whole-map bar
(``psnr >= 50 and rel < 1e-2``; DepthAA: ``rel < 2e-2`` on the edit and 50 dB) would have passed.  Recorded when this was written
(B = 3.6):

    mutation                                                         shape        worst region ratio   old bar
    1 last key not attended in block 5                               56 x 112     8.3                  fail (49.9 dB, rel 1.7e-2)
    2 one zero-score padded key attended, every block                56 x 112     30.6                 fail (42.4 dB)
    3 class token missing from the keys of block 5                   112 x 112    47.6                 fail (42.4 dB)
    4 last 16-query tile keeps block 4's attention output (block 5)  112 x 224    25.4                 fail (52.6 dB, rel 1.4e-2)
    5 position grid transposed                                       42 x 70      323                  fail (18.9 dB)
    6 refinenet3's resize with align_corners=False                   42 x 70      80.2                 fail (31.4 dB)
    7 resize_layers.3 sampled one pixel off                          42 x 70      368                  fail (17.9 dB)
    8 last partial patch of output_conv2.0 behind a replicate pad    56 x 112     243                  fail (39.7 dB)
    DepthAA bias table transposed                                    2 x 33 x 47  39.1                 fail (rel 1.5e-1)
    DepthAA shift pad replicate instead of zero                      2 x 33 x 47  22.0                 fail (rel 5.5e-2; 51.5 dB passes)
    DepthAA centred pad off by one                                   2 x 33 x 47  25.4                 fail (rel 5.1e-2; 52.0 dB passes)
    DepthAA last window row skipped                                  2 x 33 x 47  31.6                 fail (rel 9.5e-2)
    2b one zero-score padded key attended in block 5 ONLY            56 x 112     2.3 (global 1.9)     PASS (57.6 dB, rel 4.9e-3)

At these sizes a token is 1 / 32 to 1 / 128 of the map, so the whole-map bar sees most of the defects too, some by a hair (1: 49.9 dB
against 50; 4: rel 1.4e-2 against 1e-2): the same defect in a map four times the size would pass it, while a region ratio does not
dilute.  The figures move by some 10 % with the CPU that computes the emulation (the summation order in front of each fp16 rounding).

What pinning final outputs cannot see is listed in ``NOT_CAUGHT`` with the ratio reached, printed and not asserted: 2b, one padded key
of score 0 (weight 1 / 34 of an average row, its V the last key's) in ONE of the twelve blocks, stays inside the fp16 noise of the
final map (2.3 against B = 3.6); a token-level tap of the encoder would be needed to see it.
"""
import contextlib

import pytest
import torch
import torch.nn.functional as F

import depth_cases as D
import errloc as E
from oracle import depth_aa as ODAA
from oracle import depth_anything_v2 as ODA
from oracle import row_flow_v3 as ORF
from oracle.fp16_emulation import fp16_autocast_emulation, half_weights

A, B = E.A_SIDE, E.B_SIDE
NEG = float("-inf")


# ---- cells ------------------------------------------------------------------------------------------------------------------------
def test_cells():
    assert E.cells_for(D.NET) == [((14, 14), (0, 0)), ((56, 56), (0, 0)), ((8, 32), (0, 0))]
    assert E.depth_aa_pad(16, 16) == (8, 8) and E.depth_aa_pad(5, 9) == (5, 3) and E.depth_aa_pad(33, 47) == (7, 0)
    assert E.depth_aa_pad(31, 95) == (0, 0) and E.depth_aa_pad(64, 80) == (8, 8)
    assert E.cells_for(D.AA, shape=(16, 16)) == [((16, 16), (8, 8), (8, 8))]
    assert E.cells_for(D.AA, shape=(33, 47)) == [((16, 16), (9, 0), (8, 8))]
    assert E.cells_for(D.AA, shape=(5, 9)) == [((16, 16), (11, 13), (8, 8))]
    st = E.localised_stats(torch.ones(1, 1, 28, 28), torch.zeros(1, 1, 28, 28), torch.ones(1, 1, 28, 28), E.cells_for(D.NET), 1.0, 0.0)
    assert sorted({(d["cell"], d["offset"]) for d in st["regions"]}) == [((8, 32), (0, 0)), ((8, 32), (4, 16)), ((14, 14), (0, 0)),
                                                                          ((14, 14), (7, 7)), ((56, 56), (0, 0)), ((56, 56), (28, 28))]
    assert (E.A_SIDE, E.B_SIDE, E.TAP_TAU_REL) == (2.1, 3.6, 2e-3)
    for case in D.CASES:                                              # the token counts the cases are there for
        assert D.tokens(*case[1][1:]) == D.NP[case[1][1:]]


# ---- (a) conditions on the inputs -------------------------------------------------------------------------------------------------
def _region_noise(name, y64, ye):
    """[(cell, offset, region noise [B,1,ny,nx])] of every partition ``localised_stats`` looks at."""
    noise, out = ye.double() - y64, []
    for cell, base, *shift in D.cells(name, y64.shape):
        (ch, cw), (sy, sx) = cell, (shift[0] if shift else (cell[0] // 2, cell[1] // 2))
        for off in sorted({(base[0] % ch, base[1] % cw), ((base[0] + sy) % ch, (base[1] + sx) % cw)}):
            out.append((cell, off, E.region_max(noise, cell, off)))
    return out


@pytest.mark.parametrize("case", D.CASES, ids=D.case_id)
def test_depth_anything_input_conditions(case):
    x, y64, ye = D.references(case)
    b, h, w = case[1]
    assert y64.dtype == torch.float64 and y64.shape == ye.shape == (b, 1, h, w) and float(y64.std()) > 1e-3
    assert int((y64 == 0).sum()) == 0 and int((ye == 0).sum()) == 0, "an output pixel is exactly 0: change the case's seed"
    for cell, off, r in _region_noise(D.NET, y64, ye):
        assert float(r.min()) > 0.0, (cell, off)
        assert float(r.max()) <= 10.0 * float(r.min()), (cell, off, float(r.max()) / float(r.min()))
    st = E.check_localised(ye, y64, ye, D.cells(D.NET, y64.shape), A, B, 0.0, label=D.case_id(case))
    assert st["global"] == 1.0 and st["worst"] == 1.0                  # the emulation against itself: exactly 1


@pytest.mark.parametrize("case", D.AA_CASES, ids=D.aa_case_id)
def test_depth_aa_input_conditions(case):
    x, y64, ye = D.aa_references(case)
    assert y64.dtype == torch.float64 and y64.shape == ye.shape == x.shape
    assert float((y64 - x.double()).abs().mean()) > 2e-3 * float(x.max() - x.min())      # the net really edits the depth
    tau = D.tau_for(y64)
    for cell, off, r in _region_noise(D.AA, y64, ye):
        assert float(r.min()) > 0.0, (cell, off)
        assert float(r.max()) <= 1.5 * tau, (cell, off, float(r.max()), tau)        # quiet regions: the floor decides, not a division
    st = E.check_localised(ye, y64, ye, D.cells(D.AA, y64.shape), A, B, 0.0, label=D.aa_case_id(case))
    assert st["global"] == 1.0 and st["worst"] == 1.0


# ---- (b) fp32 ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", D.CASES, ids=D.case_id)
def test_depth_anything_fp32_is_far_inside_the_bound(case):
    """fp32 ``model_forward``: worst ratio below 0.05."""
    enc, shape, taps, max_depth = case
    x, y64, ye = D.references(case)
    y = ODA.model_forward(D.case_state_dict(case), x, taps=taps, max_depth=max_depth).unsqueeze(1)
    st = E.check_localised(y, y64, ye, D.cells(D.NET, y64.shape), A, B, D.tau_for(y64), label=D.case_id(case))
    assert st["worst"] < 0.05 and st["global"] < 0.05, E.summary(st)


@pytest.mark.parametrize("case", D.AA_CASES, ids=D.aa_case_id)
def test_depth_aa_fp32_is_far_inside_the_bound(case):
    shape, mode = case
    x, y64, ye = D.aa_references(case)
    y = ODAA.infer(D.aa_state_dict(), x) if mode == "infer" else ODAA.forward(D.aa_state_dict(), x, clamp=False)
    st = E.check_localised(y, y64, ye, D.cells(D.AA, y64.shape), A, B, D.tau_for(y64), label=D.aa_case_id(case))
    assert st["worst"] < 0.05 and st["global"] < 0.05, E.summary(st)


def test_depth_aa_constant_map_through_infer():
    """scale = max - min = 0: (x - min) / 0 is nan, ``nan_to_num`` makes it 0, and forward(0) * 0 + min is the constant itself."""
    x = torch.full((2, 1, 33, 47), 7.25)
    y = ODAA.infer(D.aa_state_dict(), x)
    assert torch.equal(y, x) and torch.equal(E.oracle64(D.aa_state_dict(), x, D.AA, infer=True), x.double())


# ---- (c) the mutations ------------------------------------------------------------------------------------------------------------
class _Shim:
    """A module as the oracle sees it, with some of its functions wrapped (the module itself stays as it is)."""

    def __init__(self, real, **wrapped):
        self._real = real
        self.__dict__.update(wrapped)

    def __getattr__(self, name):
        return getattr(self._real, name)


@contextlib.contextmanager
def _wrapped(module, **shims):
    """``module.torch`` / ``.F`` / ``.RF`` / a function of it replaced for the duration: {"torch": {"softmax": f}, ...}."""
    saved = {k: getattr(module, k) for k in shims}
    try:
        for k, v in shims.items():
            setattr(module, k, _Shim(saved[k], **v) if isinstance(v, dict) else v)
        yield
    finally:
        for k, v in saved.items():
            setattr(module, k, v)


def _in_call(n, real, edit):
    """``real`` but for its n-th call (0-based; None: every call), which goes through ``edit(real, *args, **kwargs)``."""
    count = [0]

    def f(*args, **kwargs):
        i, count[0] = count[0], count[0] + 1
        return edit(real, *args, **kwargs) if n is None or i == n else real(*args, **kwargs)
    return f


def _drop_key(k):
    def edit(real, s, dim=-1):
        s = s.clone()
        s[..., k] = NEG
        return real(s, dim=dim)
    return edit


def _padded_key(real, s, dim=-1):
    """One key past the sequence attended with score 0 (``da_attn_kernel`` clamps staged keys at Np - 1: its V is the last key's)."""
    p = real(torch.cat([s, torch.zeros_like(s[..., :1])], dim=-1), dim=dim)
    p, extra = p[..., :-1].clone(), p[..., -1]
    p[..., -1] += extra
    return p


def _stale_last_tile(block, embed):
    """F.linear: the input of block ``block``'s attn.proj (the attention output; the only [embed, embed] Linear) keeps the previous
    block's rows from the last 16-query tile on."""
    state = {"n": 0, "prev": None}

    def linear(x, w, b=None):
        if tuple(w.shape) == (embed, embed):
            i, state["n"] = state["n"], state["n"] + 1
            if i == block:
                q0 = (x.shape[1] - 1) // 16 * 16
                x = torch.cat([x[:, :q0], state["prev"][:, q0:]], dim=1)
            state["prev"] = x
        return F.linear(x, w, b)
    return linear


def _pos_transposed(pos_embed, gh, gw):
    pe = ODA_INTERPOLATE(pos_embed, gw, gh)
    patch = pe[:, 1:].reshape(1, gw, gh, -1).transpose(1, 2).reshape(1, gh * gw, -1)
    return torch.cat([pe[:, :1], patch], dim=1)


ODA_INTERPOLATE = ODA.interpolate_pos_embed


def _bilinear_call(n):
    """F.interpolate: the n-th BILINEAR call (the fusion blocks 4, 3, 2, 1, then the final resize) with align_corners=False."""
    count = [0]

    def interpolate(x, *args, **kwargs):
        if kwargs.get("mode") == "bilinear":
            i, count[0] = count[0], count[0] + 1
            if i == n:
                kwargs = dict(kwargs, align_corners=False)
        return F.interpolate(x, *args, **kwargs)
    return interpolate


def _stride2_one_off(x, w, b=None, stride=1, padding=0):
    """F.conv2d: resize_layers.3 (the only stride-2 conv) reads x[2 oy + ky] instead of x[2 oy + ky - 1]."""
    if stride == 2:
        return F.conv2d(F.pad(x, (0, 2, 0, 2)), w, b, stride=2, padding=0)
    return F.conv2d(x, w, b, stride=stride, padding=padding)


def _last_patch_replicate(weight):
    """F.conv2d: the rightmost, partial 32-column patch of the conv with ``weight`` is computed behind a replicate pad."""
    def conv2d(x, w, b=None, stride=1, padding=0):
        y = F.conv2d(x, w, b, stride=stride, padding=padding)
        if w is weight:
            c0 = x.shape[3] // 32 * 32
            assert 0 < c0 < x.shape[3], "no partial patch at this width"
            yr = F.conv2d(F.pad(x, (1, 1, 1, 1), mode="replicate"), w, b)
            y = torch.cat([y[..., :c0], yr[..., c0:]], dim=3)
        return y
    return conv2d


def _mutations(hw):
    """name -> (shape, shims of oracle.depth_anything_v2) for the state dict ``hw`` the forward runs with."""
    embed = hw["pretrained.patch_embed.proj.bias"].shape[0]
    sm = torch.softmax
    return {
        "1 last key not attended in block 5": ((1, 56, 112), {"torch": {"softmax": _in_call(5, sm, _drop_key(-1))}}),
        "2 one zero-score padded key attended in every block": ((1, 56, 112), {"torch": {"softmax": _in_call(None, sm, _padded_key)}}),
        "2b one zero-score padded key attended in block 5 only": ((1, 56, 112), {"torch": {"softmax": _in_call(5, sm, _padded_key)}}),
        "3 class token missing from the keys of block 5": ((2, 112, 112), {"torch": {"softmax": _in_call(5, sm, _drop_key(0))}}),
        "4 last 16-query tile keeps block 4's attention output in block 5": ((1, 112, 224), {"F": {"linear": _stale_last_tile(5, embed)}}),
        "5 position grid transposed": ((2, 42, 70), {"interpolate_pos_embed": _pos_transposed}),
        "6 refinenet3's resize with align_corners=False": ((2, 42, 70), {"F": {"interpolate": _bilinear_call(1)}}),
        "7 resize_layers.3 sampled one pixel off": ((2, 42, 70), {"F": {"conv2d": _stride2_one_off}}),
        "8 last partial patch of output_conv2.0 behind a replicate pad": (
            (1, 56, 112), {"F": {"conv2d": _last_patch_replicate(hw["depth_head.scratch.output_conv2.0.weight"])}}),
    }


MUTATIONS = ["1 last key", "2 one zero-score", "2b one zero-score", "3 class token", "4 last 16-query", "5 position", "6 refinenet3", "7 resize_layers.3", "8 last partial"]
# mutations that a check of the final output does not catch even at their smallest shape: name prefix -> the worst ratio reached
NOT_CAUGHT = {"2b one zero-score": 2.32}


def _run_mutation(prefix):
    hw = half_weights(D.state_dict("vits"))
    name, (shape, shims) = next((k, v) for k, v in _mutations(hw).items() if k.startswith(prefix))
    case = ("vits", shape, None, 0.0)
    x, y64, ye = D.references(case)
    with _wrapped(ODA, **shims), fp16_autocast_emulation():
        y = ODA.model_forward(hw, x.float()).unsqueeze(1)
    assert torch.equal(E.emulated(D.state_dict("vits"), x, D.NET), ye), "the wrapping outlived the mutation"
    assert not torch.equal(y, ye), f"{name}: the mutation changed nothing"
    st = D.stats(y, y64, ye, D.NET, B)
    try:
        E.assert_localised(st, A, B, D.tau_for(y64), label=name)
        caught = False
    except AssertionError:
        caught = True
    old_ok, p, rel = D.old_asserts(y, y64)
    return name, shape, caught, st, old_ok, p, rel


@pytest.mark.parametrize("prefix", MUTATIONS)
def test_depth_anything_mutation(prefix, capsys):
    name, shape, caught, st, old_ok, p, rel = _run_mutation(prefix)
    with capsys.disabled():
        print(f"\ndepth_anything {name} ({shape[1]} x {shape[2]}): global {st['global']:.2f} worst region ratio {st['worst']:.2f} "
              f"(A {A}, B {B}); {p:.1f} dB rel {rel:.1e} -> old bar {'PASS' if old_ok else 'fail'}")
    if prefix in NOT_CAUGHT:
        assert not caught, f"{name} is caught now (ratio {st['worst']:.2f}): move it to the asserted list"
    else:
        assert caught, (name, E.summary(st))


# DepthAA: shims of oracle.depth_aa
def _aa_bias_transposed(sd, p, window):
    return ORF.window_score_bias(sd, p, window).transpose(0, 1)


def _aa_pad(kind):
    def pad(x, pad, mode="constant", value=None):
        if kind == "shift replicate" and mode == "constant":
            return F.pad(x, pad, mode="replicate")
        if kind == "centred off by one" and mode == "replicate" and x.shape[1] == 1:        # the [B,1,h,w] input, not conv_mlp's pad
            pw1, pw2, ph1, ph2 = pad
            return F.pad(x, (pw1 + 1, pw2 - 1, ph1, ph2), mode="replicate")
        return F.pad(x, pad, mode=mode, value=value)
    return pad


def _aa_skip_last_window_row(sd, p, x, window, bias, num_heads=2):
    o = ORF.window_mha(sd, p, x, window, bias, num_heads=num_heads).clone()
    o[:, :, -window[0]:] = 0.0
    return o


AA_MUTATIONS = {
    "bias table transposed": {"RF": {"window_score_bias": _aa_bias_transposed}},
    "shift pad replicate instead of zero": {"F": {"pad": _aa_pad("shift replicate")}},
    "centred pad off by one": {"F": {"pad": _aa_pad("centred off by one")}},
    "last window row skipped": {"RF": {"window_mha": _aa_skip_last_window_row}},
}
AA_MUTATION_CASE = ((2, 33, 47), "forward")
AA_NOT_CAUGHT = {}


@pytest.mark.parametrize("name", list(AA_MUTATIONS))
def test_depth_aa_mutation(name, capsys):
    x, y64, ye = D.aa_references(AA_MUTATION_CASE)
    hw = half_weights(D.aa_state_dict())
    with _wrapped(ODAA, **AA_MUTATIONS[name]), fp16_autocast_emulation():
        y = ODAA.forward(hw, x.float(), clamp=False)
    assert torch.equal(E.emulated(D.aa_state_dict(), x, D.AA), ye), "the wrapping outlived the mutation"
    assert not torch.equal(y, ye), f"{name}: the mutation changed nothing"
    st = D.stats(y, y64, ye, D.AA, B)
    try:
        E.assert_localised(st, A, B, D.tau_for(y64), label=name)
        caught = False
    except AssertionError:
        caught = True
    edit, edit_ref = y.double() - x.double(), y64 - x.double()
    rel = float((edit - edit_ref).pow(2).mean().sqrt() / edit_ref.pow(2).mean().sqrt())
    p = E.psnr_db(y, y64)
    with capsys.disabled():
        print(f"\ndepth_aa {name} (2 x 33 x 47): global {st['global']:.2f} worst region ratio {st['worst']:.2f} (A {A}, B {B}); edit rel {rel:.1e} "
              f"{p:.1f} dB -> old bar {'PASS' if rel < 2e-2 and p >= 50.0 else 'fail'}")
    if name in AA_NOT_CAUGHT:
        assert not caught, f"{name} is caught now (ratio {st['worst']:.2f}): move it to the asserted list"
    else:
        assert caught, (name, E.summary(st))
