"""CPU: ``tests/errloc.py`` on the iw3 side nets (``sbs.row_flow_v3``, ``sbs.mlbw_*``), the fp16-autocast emulation standing in for
the engine.

The counterpart of ``test_errloc.py`` / ``test_errloc_cunet.py`` for ``csrc/rowflow.hip`` and the WABlock it runs (``csrc/wa_block.hip``), whose kernels go wrong per window (one
window per wave) and per edge.  (a) The clean emulation passes every case of ``test_gpu_sidenet_errloc.py`` with ratio <= 1.  (b)
Six mutations of the forward, each one a way ``wmha_kernel`` / ``rf_input_kernel`` / ``mlbw_in_kernel`` could be wrong, are applied
to a restatement of the oracle path (``_row_flow`` / ``_mlbw`` below, bit-equal to the oracle without a mutation) and run under the
emulation: ``check_localised`` with the side-net cells fails for every one.  Recorded when this was written (seeded weights, depth
58 x 104 unless noted, B = 3.6; "old" = the whole-image asserts of test_row_flow.py / test_mlbw.py on the same output: max / mean of
|delta error| below 2e-2 / 2e-3 (MLBW 5e-2 / 4e-3), warped image >= 50 dB):

    mutation                                                   worst region ratio   max / mean delta error   warp PSNR   old asserts
    3 x 3 score bias transposed ([key][query])                 83.8                 8.7e-2 / 8.0e-3          57.0 dB     fail (max, mean)
    7 padded keys of the 3 x 3 window unmasked                 275.3                3.2e-1 / 3.8e-2          46.3 dB     fail (all three)
    last 4 x 4 window skipped (11 x 95: the wave tail)         516.7                2.8e-1 / 1.3e-2          51.0 dB     fail (max, mean)
    last 3 x 3 window skipped (11 x 95)                        455.4                2.4e-1 / 6.6e-3          52.2 dB     fail (max, mean)
    right pad replicates the wrong edge under flip             88.3                 4.6e-2 / 1.2e-3          59.6 dB     fail (max only)
    MLBW shifted-block padded tokens absent  l2 / l2s / l4     174 / 103 / 199      2.9e-1 / 1.8e-2 (l2)     51.3 dB     fail (max, mean)
    MLBW centred pad off by one (pw1 + 1)    l2 / l2s / l4     125 / 110 / 138      2.4e-1 / 2.7e-2 (l2)     48.1 dB     fail (all three)
    one (4, 32) window of row_flow off by 1.2e-2 px            16.5                 1.4e-2 / 4.7e-4          59.9 dB     PASS

With these weights a whole window computed wrongly is a defect of tenths of a pixel, so the old max assert sees it too (the mean and
the PSNR asserts mostly do not); what the old asserts cannot see is the last row, six times the emulation's worst error in one window.
At the fixture's own shape (58 x 104, 60 x 24 tokens) the last window of the map lies wholly in the padding, seven tokens from the
nearest real one: skipping it changes NO output pixel, which is why the skipped-window mutations (and the GPU wave-tail case) run at
11 x 95.  (c) The ``tau`` floor decides in regions whose emulation error is below ``tau / B``.  (d) The rectangular-cell bookkeeping
reports a planted error with its row, column and band.
"""
import math

import pytest
import torch
import torch.nn.functional as F

import errloc as E
import sidenet_cases as S
from conftest import psnr, synth_image
from oracle import mlbw as OM
from oracle import row_flow_v3 as ORF
from oracle.fp16_emulation import fp16_autocast_emulation, half_weights

A, B = E.A_SIDE, E.B_SIDE
FIXTURE = (1, 58, 104)


# ---- a restatement of the oracle path with the mutations --------------------------------------------------------------------------
def _window_mha(sd, p, x, window, bias, num_heads, mut=(), valid=None):
    """``oracle.row_flow_v3.window_mha`` with hooks.  mut: "unmasked" (the tokens of a window padded to the 16 rows of the MFMA tile
    with zero-input tokens that take part as keys: k / v = the projection's bias, score bias 0), "skip_last" (the last window of the
    map gets no attention output), "absent" (keys whose ``valid`` entry is 0 are masked out instead of attending as bias-only
    tokens)."""
    b, c, h, w = x.shape
    sh, sw = window
    oh, ow = h // sh, w // sw
    n = sh * sw

    def to_bnc(z):
        cc = z.shape[1]
        return z.reshape(b, cc, oh, sh, ow, sw).permute(0, 2, 4, 3, 5, 1).reshape(b * oh * ow, n, cc)
    t = to_bnc(x)
    nk = n
    if "unmasked" in mut and n < 16:
        t = torch.cat([t, t.new_zeros(t.shape[0], 16 - n, c)], dim=1)
        bias = F.pad(bias, (0, 16 - n, 0, 16 - n))
        nk = 16
    qkv = F.linear(t, sd[p + "mha.qkv_proj.weight"], sd[p + "mha.qkv_proj.bias"])
    q, k, v = qkv.split(c, dim=-1)
    hd = c // num_heads

    def heads(z):
        return z.view(-1, nk, num_heads, hd).permute(0, 2, 1, 3)
    q, k, v = heads(q), heads(k), heads(v)
    s = (q @ k.transpose(-1, -2)) * (1.0 / math.sqrt(hd)) + bias
    if "absent" in mut and valid is not None:
        s = s.masked_fill(to_bnc(valid)[:, None, None, :, 0] == 0, float("-inf"))
    o = torch.softmax(s, dim=-1) @ v
    o = o.permute(0, 2, 1, 3).reshape(-1, nk, c)
    o = F.linear(o, sd[p + "mha.head_proj.weight"], sd[p + "mha.head_proj.bias"])[:, :n]
    if "skip_last" in mut:
        o = torch.cat([o[:-1], torch.zeros_like(o[-1:])])
    return o.reshape(b, oh, ow, sh, sw, c).permute(0, 5, 1, 3, 2, 4).reshape(b, c, h, w)


def _rf_block(sd, p, x, window, mut=()):
    bias = ORF.window_score_bias(sd, p + "bias.", window)
    if "transposed" in mut:
        bias = bias.transpose(0, 1)
    x = x + _window_mha(sd, p + "mha.", x, window, bias, 2, mut)
    z = F.gelu(F.conv2d(x, sd[p + "conv_mlp.0.weight"], sd[p + "conv_mlp.0.bias"]))
    z = F.conv2d(F.pad(z, (1, 1, 1, 1), mode="replicate"), sd[p + "conv_mlp.3.weight"], sd[p + "conv_mlp.3.bias"])
    return x + F.leaky_relu(z, 0.1)


def _row_flow(sd, x, mut44=(), mut33=(), wrong_edge=False):
    """``oracle.row_flow_v3.delta_forward``; ``wrong_edge``: the right pad replicates column 0 of the (mirrored) planes, the edge a
    kernel that clamps in the wrong frame would read."""
    h, w = x.shape[2:]
    pad1, pad2 = 96 - w % 96, 12 - h % 12
    if wrong_edge:
        x = F.pad(torch.cat([x, x[..., :1].expand(-1, -1, -1, pad1)], dim=3), (0, 0, 0, pad2), mode="replicate")
    else:
        x = F.pad(x, (0, pad1, 0, pad2), mode="replicate")
    x = ORF.pixel_unshuffle_w(x, 8)
    x = F.conv2d(x, sd["blocks.0.weight"], sd["blocks.0.bias"])
    x = _rf_block(sd, "blocks.1.", x, (4, 4), mut44)
    x = _rf_block(sd, "blocks.2.", x, (3, 3), mut33)
    x = ORF.pixel_shuffle_w(x, 8)[:, :, :h, :w]
    return F.conv2d(F.pad(x, (1, 1, 1, 1), mode="replicate"), sd["last_layer.1.weight"], sd["last_layer.1.bias"])


def _mlbw(sd, x, num_layers, mut=(), pad_shift=0):
    """``oracle.mlbw.delta_forward``; ``pad_shift``: the input is padded by pw1 + ``pad_shift`` columns on the left (what
    mlbw_in_kernel would read with ``xs - (pw1 + 1)``) while the crop of the output stays at pw1."""
    h, w = x.shape[2:]
    pad_w, pad_h = 32 - w % 32, 4 - h % 4
    pw1, ph1 = pad_w // 2, pad_h // 2
    pw2, ph2 = pad_w - pw1, pad_h - ph1
    x = F.pad(x, (pw1 + pad_shift, pw2 - pad_shift, ph1, ph2), mode="replicate")
    x1 = F.leaky_relu(F.conv2d(F.pad(x, (4, 4, 0, 0), mode="replicate"), sd["lv1_in.1.weight"], sd["lv1_in.1.bias"]), 0.2)
    x = ORF.pixel_unshuffle_w(x1, 8)
    n_blocks = sum(1 for k in sd if k.startswith("lv2.") and k.endswith("mha.mha.qkv_proj.weight"))
    for i, shift in enumerate(OM.block_shifts(n_blocks)):
        p = f"lv2.{i}."
        ph, pw = (2 if shift[0] else 0), (2 if shift[1] else 0)
        xs = F.pad(x, (pw, pw, ph, ph)) if ph or pw else x
        valid = F.pad(torch.ones_like(x[:, :1]), (pw, pw, ph, ph)) if ph or pw else None
        a = _window_mha(sd, p + "mha.", xs, (4, 4), ORF.window_score_bias(sd, p + "bias.", (4, 4)), num_layers, mut, valid)
        if ph or pw:
            a = a[:, :, ph:a.shape[2] - ph, pw:a.shape[3] - pw]
        x = x + a
        z = F.gelu(F.conv2d(x, sd[p + "conv_mlp.0.weight"], sd[p + "conv_mlp.0.bias"]))
        x = x + F.conv2d(F.pad(z, (1, 1, 1, 1), mode="replicate"), sd[p + "conv_mlp.3.weight"], sd[p + "conv_mlp.3.bias"])
    x = ORF.pixel_shuffle_w(x, 8)
    x = F.conv2d(F.pad(x + x1, (4, 4, 0, 0), mode="replicate"), sd["lv1_out.1.weight"], sd["lv1_out.1.bias"])
    x = x[:, :, ph1:x.shape[2] - ph2, pw1:x.shape[3] - pw2]
    delta, weight = x[:, :2 * num_layers].chunk(2, dim=1)
    return delta, F.softmax(weight.float(), dim=1)


def _emulate(fn, sd, *args, **kwargs):
    with fp16_autocast_emulation():
        return fn(half_weights(sd), *args, **kwargs)


def test_the_restatement_is_the_oracle():
    """Without a mutation ``_row_flow`` / ``_mlbw`` compute what the oracle computes, bit for bit, in fp32 and under the emulation."""
    for shape in (FIXTURE, (2, 11, 95)):
        x = S.planes(shape)
        sd = S.state_dict(E.ROW_FLOW)
        assert torch.equal(_row_flow(sd, x), ORF.delta_forward(sd, x))
        assert torch.equal(_emulate(_row_flow, sd, x), E.emulated(sd, x, E.ROW_FLOW))
        for net in ("sbs.mlbw_l2", "sbs.mlbw_l2s", "sbs.mlbw_l4"):
            sd, layers = S.state_dict(net), E.MLBW[net][0]
            for got, want in zip(_mlbw(sd, x, layers), OM.delta_forward(sd, x, layers)):
                assert torch.equal(got, want)
            for got, want in zip(_emulate(_mlbw, sd, x, layers), E.emulated(sd, x, net)):
                assert torch.equal(got, want)


# ---- (a) the clean emulation ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", S.CASES, ids=S.case_id)
def test_clean_emulation_passes(case):
    net, shape, flip, regime = case
    x, y64, ye = S.references(case)
    assert len(y64) == len(S.outputs(net))
    for name, r64, re in zip(S.outputs(net), y64, ye):
        assert r64.dtype == torch.float64 and r64.shape[0] == shape[0] and r64.shape[2:] == shape[1:]
        st = E.check_localised(re, r64, re, E.cells_for(net, shape=shape[1:]), A, B, S.tau_for(r64), label=f"{S.case_id(case)} {name}")
        assert st["worst"] <= 1.0 and st["global"] <= 1.0


def test_cells():
    assert E.cells_for(E.ROW_FLOW) == [((4, 32), (0, 0)), ((3, 24), (0, 0)), ((12, 96), (0, 0))]
    assert E.mlbw_pad(58, 104) == (1, 12) and E.mlbw_pad(4, 32) == (2, 16) and E.mlbw_pad(3, 31) == (0, 0) and E.mlbw_pad(21, 65) == (1, 15)
    assert E.cells_for("sbs.mlbw_l2", shape=(58, 104)) == [((4, 32), (3, 20), (2, 16))] == E.cells_for("sbs.mlbw_l4", shape=(58, 104))
    assert E.cells_for("sbs.mask_mlbw_l2", shape=(4, 32)) == [((4, 32), (2, 16), (2, 16))]
    assert E.cells_for("sbs.mlbw_l2s", shape=(21, 65)) == [((4, 32), (3, 17), (0, 16))]
    assert E.cells_for("waifu2x.swin_unet_2x") == [(12, 0), (24, 0), (48, 0)]            # the square forms are as they were
    # the stride loops really run in the two large cases, the wave tails in the small ones
    assert S.row_flow_windows(S.ROW_FLOW_BIG, 4) == 9504 > 4 * 2048 and S.mlbw_windows(S.MLBW_BIG) == 1056 > 4 * 256 and S.mlbw_windows(S.MLBW_BIG, True) == 1156
    assert S.row_flow_windows((1, 11, 95), 4) == 9 and S.row_flow_windows((1, 11, 95), 3) == 16


# ---- (b) the mutations ------------------------------------------------------------------------------------------------------------
def _old_asserts(net, d, d64, w=None, w64=None):
    """The whole-image asserts of test_row_flow.py / test_mlbw.py on the same outputs: (passes, max, mean, PSNR of the warp)."""
    err = (d.double() - d64).abs()
    lim = (2e-2, 2e-3) if net == E.ROW_FLOW else (5e-2, 4e-3)
    ok = err.max().item() < lim[0] and err.mean().item() < lim[1]
    b, layers, h, wd = d64.shape
    c = torch.stack([synth_image(90 + i, 3, h, wd) for i in range(b)]).double()
    grid, scale = ORF.make_grid(b, wd, h).double(), 1.0 / (wd // 2 - 1)

    def warp(dd, ww):
        z = torch.zeros_like(c)
        for i in range(layers):
            di = dd[:, i:i + 1].double()
            z = z + ORF.backward_warp(c, grid, torch.cat([di, torch.zeros_like(di)], 1), scale) * (1.0 if ww is None else ww[:, i:i + 1].double())
        return z.clamp(0, 1)
    p = psnr(warp(d, w), warp(d64, w64))
    if w is not None:
        ew = (w.double() - w64).abs()
        ok = ok and ew.max().item() < 3e-2 and ew.mean().item() < 2e-3
    return ok and p >= 50.0, err.max().item(), err.mean().item(), p


def _caught(outs, y64, ye, net, shape):
    """(any output fails check_localised, worst region ratio)"""
    worst, caught = 0.0, False
    for y, r64, re in zip(outs, y64, ye):
        st = S.stats(y, r64, re, net, shape, B)
        worst = max(worst, st["worst"])
        try:
            E.assert_localised(st, A, B, S.tau_for(r64), label=net)
        except AssertionError:
            caught = True
    return caught, worst


# (shape, flip, mutation).  The last window of the fixture's 60 x 24 token map lies in the padding, 7 tokens from the nearest real
# one: skipping it changes no output pixel, so the skipped window runs at 11 x 95 (12 x 12 tokens, 9 windows of 4 x 4: the last
# one is the wave tail, and holds the bottom-right corner of the depth map)
ROW_FLOW_MUTATIONS = {
    "3x3 score bias transposed": (FIXTURE, False, dict(mut33=("transposed",))),
    "7 padded keys of the 3x3 window unmasked": (FIXTURE, False, dict(mut33=("unmasked",))),
    "last 4x4 window skipped": ((1, 11, 95), False, dict(mut44=("skip_last",))),
    "last 3x3 window skipped": ((1, 11, 95), False, dict(mut33=("skip_last",))),
    "right pad replicates the wrong edge under flip": (FIXTURE, True, dict(wrong_edge=True)),
}
MLBW_MUTATIONS = {
    "shifted-block padded tokens absent": dict(mut=("absent",)),
    "centred pad off by one": dict(pad_shift=1),
}


@pytest.mark.parametrize("name", list(ROW_FLOW_MUTATIONS))
def test_row_flow_mutation_is_caught(name, capsys):
    shape, flip, kwargs = ROW_FLOW_MUTATIONS[name]
    case = (E.ROW_FLOW, shape, flip, "benign")
    x, y64, ye = S.references(case)
    xm = torch.flip(x, (3,)) if flip else x
    y = _emulate(_row_flow, S.state_dict(E.ROW_FLOW), xm, **kwargs)
    assert not torch.equal(y, ye[0])
    caught, worst = _caught((y,), y64, ye, E.ROW_FLOW, shape)
    old_ok, emax, emean, p = _old_asserts(E.ROW_FLOW, y, y64[0])
    with capsys.disabled():
        print(f"\nrow_flow_v3 {name}: worst region ratio {worst:.1f} (B {B}); delta error max {emax:.1e} mean {emean:.1e}, warp "
              f"{p:.1f} dB -> old asserts {'PASS' if old_ok else 'fail'}")
    assert caught, (name, worst)


@pytest.mark.parametrize("net", ["sbs.mlbw_l2", "sbs.mlbw_l2s", "sbs.mlbw_l4"])
@pytest.mark.parametrize("name", list(MLBW_MUTATIONS))
def test_mlbw_mutation_is_caught(name, net, capsys):
    case = (net, FIXTURE, False, "benign")
    x, y64, ye = S.references(case)
    d, w = _emulate(_mlbw, S.state_dict(net), x, E.MLBW[net][0], **MLBW_MUTATIONS[name])
    caught, worst = _caught((d, w), y64, ye, net, FIXTURE)
    old_ok, emax, emean, p = _old_asserts(net, d, y64[0], w, y64[1])
    with capsys.disabled():
        print(f"\n{net} {name}: worst region ratio {worst:.1f} (B {B}); delta error max {emax:.1e} mean {emean:.1e}, warp {p:.1f} dB "
              f"-> old asserts {'PASS' if old_ok else 'fail'}")
    assert caught, (name, net, worst)


def test_one_window_defect_the_old_asserts_cannot_see(capsys):
    """One (4, 32) window of the row_flow delta off by 1.2e-2 px (six times the emulation's worst error on this fixture): below all
    three whole-image asserts, caught by the localised check, which names the window."""
    case = (E.ROW_FLOW, FIXTURE, False, "benign")
    _, y64, ye = S.references(case)
    y = ye[0].clone()
    y[0, 0, 28:32, 64:96] += 1.2e-2                                  # window row 7, column 2 of the 4 x 4 partition
    old_ok, emax, emean, p = _old_asserts(E.ROW_FLOW, y, y64[0])
    assert old_ok and p >= 59.0, (emax, emean, p)
    with pytest.raises(AssertionError, match=r"interior region \(row 7, col 2\) of cell \(4, 32\) offset \(0, 0\)"):
        E.check_localised(y, y64[0], ye[0], [((4, 32), (0, 0), (0, 0))], 1e9, B, S.tau_for(y64[0]), label="one window")
    caught, worst = _caught((y,), y64, ye, E.ROW_FLOW, FIXTURE)
    with capsys.disabled():
        print(f"\nrow_flow_v3 one window + 1.2e-2: worst region ratio {worst:.1f}; max {emax:.1e} mean {emean:.1e}, warp {p:.1f} dB -> old asserts PASS")
    assert caught


# ---- (c) the tau floor ------------------------------------------------------------------------------------------------------------
def test_tau_floor_decides_in_quiet_regions():
    """Regions whose emulation error is below tau / B exist (the l2s layer weights: fp16 error of a softmax output near 2.5e-4 against
    tau = 2e-3 x rms = 1.4e-3); there the bound is tau-dominated: a defect of 0.9 tau on top of the emulation passes, one of
    B x noise + 1.1 tau fails, and without the floor the first would have failed by an arbitrary factor."""
    case = ("sbs.mlbw_l2s", FIXTURE, False, "benign")
    _, y64, ye = S.references(case)
    w64, we = y64[1], ye[1]
    tau = S.tau_for(w64)
    cells = E.cells_for(case[0], shape=FIXTURE[1:])
    cell, off = cells[0][0], cells[0][1]
    noise = E.region_max(we.double() - w64, cell, off)
    assert float(noise.min()) < tau / B
    ry, rx = divmod(int(noise[0, 0].argmin()), noise.shape[3])
    n = float(noise[0, 0, ry, rx])
    top, left = (cell[0] - off[0]) % cell[0], (cell[1] - off[1]) % cell[1]
    ys, xs = slice(max(0, ry * cell[0] - top), ry * cell[0] - top + cell[0]), slice(max(0, rx * cell[1] - left), rx * cell[1] - left + cell[1])

    def with_defect(d):
        y = w64.clone()                                                # exact but for the defect: err = d in that region
        y[0, :, ys, xs] += d
        return y
    E.check_localised(with_defect(0.9 * tau), w64, we, cells, 1e9, B, tau, label="below the floor")
    with pytest.raises(AssertionError, match=f"row {ry}, col {rx}"):
        E.check_localised(with_defect(B * n + 1.1 * tau), w64, we, cells, 1e9, B, tau, label="above the floor")
    st0 = E.localised_stats(with_defect(0.9 * tau), w64, we, cells, B, 0.0)
    assert st0["worst"] > B                                            # a zero floor lets division by a quiet region decide


# ---- (d) rectangular cells --------------------------------------------------------------------------------------------------------
def test_rectangular_cells_report_row_column_and_band():
    e = torch.zeros(2, 1, 25, 97)
    e[1, 0, 7, 50] = -3.0                                               # (3, 24) cell: row 2, column 2
    r = E.region_max(e, (3, 24), (0, 0))
    assert r.shape == (2, 1, 9, 5) and r[1, 0, 2, 2] == 3.0 and r.sum() == 3.0
    r = E.region_max(e, (3, 24), (1, 12))                              # rows [0,1) [1,4) [4,7) [7,10); columns [0,12) [12,36) [36,60)
    assert r.shape == (2, 1, 9, 5) and r[1, 0, 3, 2] == 3.0
    r = E.region_max(e, (4, 32), (3, 20))                              # MLBW at 58 x 104: rows [0,3) [3,7) [7,11); columns [0,20) [20,52)
    assert r.shape == (2, 1, 7, 4) and r[1, 0, 2, 1] == 3.0
    assert torch.equal(E.region_max(e, 6, 3), E.region_max(e, (6, 6), (3, 3)))          # an int is the square form
    base = torch.full((2, 1, 25, 97), 1e-3)
    y = base.clone()
    y[1, 0, 7, 50] += 1.0
    with pytest.raises(AssertionError) as ex:
        E.check_localised(y, base * 0, base, [((3, 24), (0, 0), (0, 0))], 1e9, 4.0, 0.0, label="t")
    msg = str(ex.value)
    assert "image 1" in msg and "interior region (row 2, col 2) of cell (3, 24) offset (0, 0) [pixel 6,48] channel 0" in msg, msg
    y = base.clone()
    y[0, 0, 24, 96] += 1.0                                              # the one real pixel of the second 96-column block, last row
    with pytest.raises(AssertionError) as ex:
        E.check_localised(y, base * 0, base, E.cells_for(E.ROW_FLOW), 1e9, 4.0, 0.0, label="t")
    msg = str(ex.value)
    assert "image 0" in msg and "bottom+right region (row 8, col 4) of cell (3, 24) offset (0, 0) [pixel 24,96]" in msg, msg
    st = E.localised_stats(y, base * 0, base, [((12, 96), (0, 0), (0, 0))], 4.0, 0.0)
    assert st["regions"][0]["row"] == 2 and st["regions"][0]["col"] == 1 and st["regions"][0]["band"] == "bottom+right"
    # the shift of an entry is the second partition: (0, 16) moves the columns only
    st = E.localised_stats(y, base * 0, base, [((4, 32), (3, 17), (0, 16))], 4.0, 0.0)
    assert sorted({d["offset"] for d in st["regions"]}) == [(3, 1), (3, 17)]
