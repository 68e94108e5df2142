"""The cases of the Video-Depth-Anything temporal-module checks (helper module, not a conftest): shared by ``test_errloc_vda.py`` (CPU:
the references alone, and the engine's arrangement restated in torch) and ``test_gpu_vda_errloc.py`` (the HIP engine through
``debug_temporal``), so that both run the same shapes.

A case is (encoder, module, row, form).  Weights: ``video_depth_anything_state_dict(5, grid=8, encoder=e)``; a module's width C comes
from the encoder (ViT-S 192 / 384 / 64 / 64, ViT-B 384 / 768 / 128 / 128, ViT-L 1024 / 1024 / 256 / 256).  The attention kernels:
``vda_tattn2_kernel<C>`` with NPX = 32 / 16 / 8 / 4 / 4 pixels per workgroup for C = 64 / 128 / 192 / 256 / 384, and the per-head
``vda_tattn_kernel`` (32 pixels per workgroup; the only form for C = 768 / 1024, ``form`` "1" = NUNIF_VDA_TATTN=1 for the others).
GroupNorm: RL = 256 / (C / 8) row lanes, NB = min(256, ceil(P / 4 RL)) blocks.

    row          H x W    P     frames                  what it meets
    1x1          1 x 1    1     3, single               the smallest real map; a workgroup with one live pixel; fewer rows than row lanes
    1x5          1 x 5    5     66, single              fill, slide, ``start`` once round the ring and past it; P < NPX for 32 / 16 / 8, NPX + 1 for 4
    1x5-batched  1 x 5    5     the same 66 as batches  fill and slide inside a batch (frames 30-32 are one batch); blockIdx.y; the f P 3 C offsets
    3x11         3 x 11   33    3 (B = 3)               one pixel beyond a block for every NPX and for the per-head form's 32
    3x11-offset  3 x 11   33    3 (B = 3)               every channel group's mean = 50 x its std: E[x^2] - mean^2 of vda_gn_finalize_kernel
    9x11         9 x 11   99    2, single               the shape of test_video_depth_anything_net.py
    45x46        45 x 46  2070  2, single; C = 1024     GroupNorm at the 256-block cap (RL = 2, R = 9 rows per block: 4-5 per lane)

Every row runs for modules 0, 1, 2 of every encoder (all seven widths); module 3 shares module 2's width and gets 3x11 only.

Inputs: ``maps`` — a smooth random field drifting by (1, 2) pixels per frame plus 5 % noise, as ``clip()`` of
test_video_depth_anything_net.py — scaled to the rms the DPT head feeds the module: ``INPUT_RMS``, measured in one oracle forward of a
70 x 98 ``clip(2, ...)`` frame per encoder.  The maps are fp16-valued (the engine rounds its input on entry), so the float64 oracle,
the emulation and the engine see the same numbers.
"""
import functools

import torch
import torch.nn.functional as F

import errloc as E
from oracle import video_depth_anything_net as VN

NET = E.VDA_TEMPORAL
SEED = 5
WIDTHS = {"vits": (192, 384, 64, 64), "vitb": (384, 768, 128, 128), "vitl": (1024, 1024, 256, 256)}
# rms of the module's input map in one oracle forward (seed 5, grid 8, clip(2, 1, 70, 98)): modules 0..3
INPUT_RMS = {"vits": (1.00, 0.81, 0.93, 1.73), "vitb": (1.01, 0.81, 0.90, 1.68), "vitl": (1.00, 0.84, 0.87, 1.62)}
BATCHES_66 = (3, 1, 4, 3, 3, 5, 3, 3, 2, 3, 3, 2, 3, 1, 4, 3, 3, 5, 3, 3, 2, 3, 1)
ROWS = {                                                 # row -> ((H, W), the frames per engine call, offset map)
    "1x1": ((1, 1), (1, 1, 1), False),
    "1x5": ((1, 5), (1,) * 66, False),
    "1x5-batched": ((1, 5), BATCHES_66, False),
    "3x11": ((3, 11), (3,), False),
    "3x11-offset": ((3, 11), (3,), True),
    "9x11": ((9, 11), (1, 1), False),
    "45x46": ((45, 46), (1, 1), False),
}
assert sum(BATCHES_66) == 66
OFFSET_RATIO = 50.0


def _cases():
    out = []
    for enc, widths in WIDTHS.items():
        for module in range(4):
            C = widths[module]
            rows = ["3x11"] if module == 3 else [r for r in ROWS if r != "45x46"]
            if (enc, module) == ("vitl", 0):
                rows.append("45x46")
            for form in (("0", "1") if C <= 384 else ("0",)):
                out += [(enc, module, r, form) for r in rows]
    return out


CASES = _cases()
VITS_CASES = [c for c in CASES if c[0] == "vits"]
WIDE_CASES = [c for c in CASES if c[0] != "vits"]


def case_id(case):
    enc, module, row, form = case
    return f"{enc}-m{module}-C{WIDTHS[enc][module]}-{row}" + ("-perhead" if form == "1" else "")


@functools.lru_cache(maxsize=None)
def state_dict(encoder):
    return VN.random_state_dict(SEED, grid=8, encoder=encoder)


def maps(C, H, W, n, seed, rms, offset=False):
    """[n, P, C] fp16-valued module inputs: a smooth field drifting by (1, 2) pixels per frame + 5 % noise, scaled to ``rms``; with
    ``offset`` every group of C / 32 channels gets a constant of OFFSET_RATIO x the field's std, signs alternating."""
    g = torch.Generator().manual_seed(seed)
    base = torch.randn(C, H + n + 4, W + 2 * n + 4, generator=g)
    base = F.avg_pool2d(base.unsqueeze(0), 5, stride=1, padding=2)[0] * 3.0
    x = torch.stack([base[:, 2 + i:2 + i + H, 2 + 2 * i:2 + 2 * i + W] + 0.05 * torch.randn(C, H, W, generator=g) for i in range(n)])
    x = x * (rms / float(x.pow(2).mean().sqrt()))
    if offset:
        sign = torch.tensor([1.0, -1.0]).repeat(16).repeat_interleave(C // 32)
        x = x + (OFFSET_RATIO * float(x.std()) * sign).view(1, C, 1, 1)
    return x.permute(0, 2, 3, 1).reshape(n, H * W, C).half().float()


def inputs(enc, module, row):
    (H, W), batches, offset = ROWS["1x5" if row == "1x5-batched" else row]
    C = WIDTHS[enc][module]
    return maps(C, H, W, sum(batches), 900 + 10 * module + H + W, INPUT_RMS[enc][module], offset)


@functools.lru_cache(maxsize=None)
def references(enc, module, row):
    """(x [T, P, C], float64 output, emulated output, float64 taps, emulated taps) of one (encoder, module, row); the batched row
    shares the single-frame row's.  Computed once per process and left unchanged."""
    if row == "1x5-batched":
        return references(enc, module, "1x5")
    E.set_threads()
    hw = ROWS[row][0]
    with torch.inference_mode():
        sd, x = state_dict(enc), inputs(enc, module, row)
        t64, te = {}, {}
        y64 = E.oracle64(sd, x, NET, taps=t64, module=module, hw=hw)
        ye = E.emulated(sd, x, NET, taps=te, module=module, hw=hw)
    return x, y64, ye, t64, te


def view(t):
    """[T, P, C] -> the [T, C, 1, P] map ``localised_stats`` takes: a (1, 1) cell is one pixel of one frame."""
    return t.permute(0, 2, 1).unsqueeze(2)


def tau_for(y64):
    return E.TAP_TAU_REL * float(y64.double().pow(2).mean().sqrt())


def stats(y, y64, ye, B, group=None):
    return E.localised_stats(view(y), view(y64), view(ye), E.cells_for(NET), B, tau_for(y64), group)


def check_output(y, y64, ye, label, emit=print):
    """The module's output: every pixel of every frame at A_SIDE / B_SIDE.  Prints the figures, then asserts."""
    assert y.shape == y64.shape == ye.shape, (label, y.shape, y64.shape)
    st = stats(y, y64, ye, E.B_SIDE)
    emit(f"errloc {label} out: global {st['global']:.2f} worst {st['worst']:.2f} (err {st['_gmax']:.2e} noise {st['_nmax']:.2e})")
    return E.assert_localised(st, E.A_SIDE, E.B_SIDE, tau_for(y64), label=label + " out")


def check_taps(taps, t64, te, C, label, emit=print):
    """Every tap per pixel and head (hd = C / 8 channels) at A_VDA_TAP / B_VDA_TAP.  Prints all figures, then asserts all."""
    sts = {}
    for name in E.VDA_TAPS:
        assert taps[name].shape == t64[name].shape, (label, name, taps[name].shape, t64[name].shape)
        sts[name] = stats(taps[name], t64[name], te[name], E.B_VDA_TAP, group=C // 8)
    emit(f"errloc {label} taps: " + " ".join(f"{n} {s['global']:.2f}/{s['worst']:.2f}" for n, s in sts.items()))
    for name, st in sts.items():
        E.assert_localised(st, E.A_VDA_TAP, E.B_VDA_TAP, tau_for(t64[name]), label=f"{label} tap {name}")
    return sts


# The form of the GELU inside GEGLU.  tanh GELU differs from erf GELU by less than one fp16 ulp of the products, so no bound of a few
# times the fp16 noise per region can tell them apart; but the difference is a KNOWN pattern d = value x (gelu_tanh(gate) - gelu_erf(gate))
# over the whole tap, and the projection c = <err, d> / <d, d> of the tap's error onto it is 0 for an erf kernel and 1 for a tanh one,
# with a spread of about (rms err / rms d) / sqrt(N).  The limit is the midpoint of the two hypotheses.  Measured on an MI355X over all
# cases: |c| <= 0.31 (the 1 x 1 maps, N = 3 x 4 C values; <= 0.14 on every larger map); the restated engine with tanh GELU: 0.91 .. 1.03.
GELU_FORM_LIMIT = 0.5


def gelu_form(geglu, t64, enc, module):
    """c of the ``geglu`` tap [T, P, 4 C]: value and gate come from the float64 ``ff_ln`` tap through ff.net.0.proj in float64."""
    sd, b = state_dict(enc), f"head.motion_modules.{module}.temporal_transformer.transformer_blocks.0."
    hid = F.linear(t64["ff_ln"].double(), sd[b + "ff.net.0.proj.weight"].double(), sd[b + "ff.net.0.proj.bias"].double())
    val, gate = hid.chunk(2, dim=-1)
    d = val * (F.gelu(gate, approximate="tanh") - F.gelu(gate))
    return float(((geglu.double() - t64["geglu"].double()) * d).sum() / (d * d).sum())


def check_gelu_form(taps, t64, enc, module, label, emit=print):
    c = gelu_form(taps["geglu"], t64, enc, module)
    emit(f"errloc {label} gelu form: {c:+.3f}")
    assert abs(c) < GELU_FORM_LIMIT, f"{label}: the geglu tap's error has a component {c:+.3f} along tanh GELU - erf GELU (limit {GELU_FORM_LIMIT})"
    return c

