"""Localised error bounds for the swin and cunet nets, the iw3 side nets and the iw3 depth path: worst-REGION error against a float64
oracle (helper module, not a conftest).

PSNR is a whole-image average: one 6 x 6 window of a 256 tile off by 0.1 (70x the fp16 noise floor) still reads 51 dB.  The
kernels go wrong per window (lanes, masks, tables and index arithmetic are per window / per head / per edge row), so this module
bounds the error region by region:

    err(y) = y - oracle64(x)                       (the forward in float64: the exact answer of the net)
    noise  = emulated(x) - oracle64(x)             (the reference's own fp16-autocast arithmetic: the yardstick)

and ``check_localised`` asserts, per image, (a) max|err| <= A * max|noise| and (b) in every ``cell x cell`` region of the output
(both the aligned and the half-cell-shifted partition, i.e. the windows of the plain and the shifted blocks)
region_max(err) <= B * region_max(noise) + tau.  tau is a floor for regions where the clamp flattens the output to exact 0 / 1
(there the emulation's error is 0).  Regions in the first / last row / column of an image are reported as bands of their own.

The CUNet family (``waifu2x.cunet`` / ``upcunet`` / ``vgg_7`` / ``upconv_7``, oracle/cunet.py) goes wrong per 8 x 32 output patch of a
conv workgroup, per 16 x 16 head tile, per 16-channel MFMA n-tile and per image (SE pooling, the scale table): its regions are the
cells 8 / 16 / 32 / 64 of the level-1 map in output pixels (twice that for the 2x nets), with the same constants.

The iw3 side nets (``sbs.row_flow_v3``, ``sbs.mlbw_*``, csrc/rowflow.hip on the WABlock of csrc/wa_block.hip) run one window of 4 x 4 or 3 x 3 tokens per wave and a token
is 1 row x 8 depth pixels: their regions are rectangular cells (cell_h, cell_w) with offsets (off_y, off_x), and since flows,
softmax weights and logits are not clamped the floor is relative, tau = TAP_TAU_REL x the map's rms (``tests/sidenet_cases.py``).

The iw3 depth path (``iw3.depth_anything``: csrc/depth_anything.hip, depth_mlp.hip, conv3_lds.hip; ``iw3.depth_aa``: csrc/depth_aa.hip on the WABlock of
csrc/wa_block.hip)
is pinned on its final outputs only, [B,1,h,w], with the side nets' constants and relative floor.  The depth engine goes wrong per
token (14 x 14 pixels of the map), per 4 x 4 token block (the footprint of one ``layer4_rn`` pixel pair) and per 8 x 32 conv patch of
``output_conv2.0``; DepthAA per 8 x 8 window = 16 x 16 pixels behind its centred pad, shifted by 8 pixels in blocks 0 and 2
(``tests/depth_cases.py``).

The light inpaint nets (``inpaint.light_inpaint_v1``, ``inpaint.light_video_inpaint_v1*``: csrc/light_inpaint.hip) go wrong per 16 x 16 /
8 x 8 token window (the zero-padded shifted blocks, the per-window transposed token mixing), per 8 x 32-token conv patch and per token
(the mask rule): cells (64, 64) and (32, 128) output pixels from pixel 0 (the pad is bottom / right only) with the clamped-output
constants, and the engine's debug taps per window and conv patch of their level with the tap constants.  ``preprocess`` (the masks)
runs in fp32 outside the emulation, so the token decisions are the same on all three sides (``tests/inpaint_cases.py``).  Measured on
an MI355X over the 19 cases of tests/test_gpu_inpaint_errloc.py (profiles/light_inpaint_errloc.txt): outputs worst 1.28 global / 3.44 per
region (the small video net at 12 x 72 x 136; the image net 1.20 / 1.36, 2.67 with the hot weights), taps worst 1.60 / 4.07 (``dec1``
per 16-channel group).

The Video-Depth-Anything temporal modules (``iw3.vda_temporal``: csrc/depth_temporal.hip and ``run_tmod`` of depth_anything.hip) go
wrong per pixel (the attention's workgroup tails, GroupNorm's row lanes), per head (hd = C / 8 channels) and per frame (the window
position, the ring slot): x = T consecutive frames of ONE module's input map [T, P, C], run as a stream from ``new_state()``; the
region is one pixel — cell (1, 1) of the [T, C, 1, P] view — and for the engine's debug taps one pixel and one head.  The streaming
whole net (``iw3.vda_stream``) takes T frames [T, 3, h, w] the same way, with the depth engine's cells.  ``vda_with_pe`` hands the
fp32 sinusoidal table in through the ``pos_encoder.pe`` keys: evaluated inside the emulation mode, ``pos * div`` would be rounded to
fp16 (up to 31 x 2^-11 rad) and the yardstick inflated (``tests/vda_cases.py``, ``tests/test_errloc_vda.py``).

The swin_unet_v2 debug taps (``csrc/swin_unet_v2.hip``, ``nunif_hip_swin_unet_v2_debug_taps``) go wrong per window of their block (8 x 8
or 6 x 6 tokens, starting at -ws / 2 in a shifted block, where the padded tokens are keys / values equal to the qkv bias), per head of
32 channels (``att``) and per 16-channel n-tile of an epilogue: ``v2_tap_cells`` gives each tap the cells of its own block at its own
resolution, with the tap constants (``tests/swin_v2_cases.py``, ``tests/test_errloc_swin_v2.py``).  Measured on an MI355X over the six
cases of tests/test_gpu_swin_v2_errloc.py (profiles/swin_v2_errloc.txt): taps worst 1.33 global / 2.14 per region, output 0.55 / 0.76.
"""
import math

import torch
import torch.nn.functional as F

from oracle import cunet as OC
from oracle import depth_aa as ODAA
from oracle import depth_anything_v2 as ODA
from oracle import light_inpaint as OL
from oracle import mlbw as OM
from oracle import row_flow_v3 as ORF
from oracle import swin_unet as O
from oracle import swin_unet_v2 as OV
from oracle import video_depth_anything_net as VN
from oracle.fp16_emulation import fp16_autocast_emulation, half_weights

V2_SCALE = {"waifu2x.swin_unet_v2_1x": 1, "waifu2x.swin_unet_v2_2x": 2, "waifu2x.swin_unet_v2_4x": 4}
SCALE = {"waifu2x.swin_unet_1x": 1, "waifu2x.swin_unet_2x": 2, "waifu2x.swin_unet_4x": 4, "waifu2x.swin_unet_8x": 8,
         "waifu2x.swin_unet_4xl": 4}
# swin_unet_v2: window sizes of its levels (oracle/swin_unet_v2.py: wac1 8 / 6, wac2 8 at half resolution, wac3 8); the output
# starts one level-1 token in (x[:, :, s:-s, s:-s] after the pixel shuffle)
V2_WINDOWS = ((6, 1), (8, 1), (16, 2))          # (window in level-1 tokens, level)
# the cunet engine's nets: name -> output pixels per level-1 pixel (a level-1 patch covers 2x pixels after the 4 x 4 stride-2 deconv)
CUNET_SCALE = {"waifu2x.cunet": 1, "waifu2x.upcunet": 2, "waifu2x.vgg_7": 1, "waifu2x.upconv_7": 2}
CUNET_OFFSET = {"waifu2x.cunet": 28, "waifu2x.upcunet": 36, "waifu2x.vgg_7": 7, "waifu2x.upconv_7": 14}
CUNET_CELLS = (8, 16, 32, 64)                   # kTH = 8, the 16 x 16 head tile, kTW = 32, and two patches side by side

# the iw3 side nets (csrc/rowflow.hip, wa_block.hip): one window per wave, a token = 1 row x 8 depth pixels, so a window of WS x WS tokens is a
# cell of (WS, 8 WS) output pixels.  name -> (layers, small, hole mask) for the MLBW family
ROW_FLOW = "sbs.row_flow_v3"
ROW_FLOW_CELLS = ((4, 32), (3, 24), (12, 96))   # the 4 x 4 and the 3 x 3 window, and the pad unit (12 rows x 96 columns)
MLBW = {"sbs.mlbw_l2": (2, False, False), "sbs.mlbw_l4": (4, False, False), "sbs.mlbw_l2s": (2, True, False),
        "sbs.mask_mlbw_l2": (2, False, True)}
MLBW_CELL = (4, 32)

# the iw3 depth path, final outputs only.  The depth engine: one token of the final map, a 4 x 4 token block (one layer4_rn pixel
# pair) and the 8 x 32 patch of output_conv2.0, each aligned and shifted by half a cell.  DepthAA: one 8 x 8 window after the pixel
# shuffle, starting at the centred pad's (-ph1, -pw1), and the 4-token zero-pad shift of blocks 0 and 2 (8 pixels)
DEPTH_ANYTHING, DEPTH_AA = "iw3.depth_anything", "iw3.depth_aa"
DEPTH_ANYTHING_CELLS = ((14, 14), (56, 56), (8, 32))
DEPTH_AA_CELL, DEPTH_AA_SHIFT = (16, 16), (8, 8)

# Video-Depth-Anything: one temporal module on its own map (a region = one pixel, taps: one pixel and one head), and the streaming
# net on frames (the depth engine's cells)
VDA_TEMPORAL, VDA_STREAM = "iw3.vda_temporal", "iw3.vda_stream"
VDA_TEMPORAL_CELL = (1, 1)
VDA_TAPS = ("gn", "proj_in", "ln0", "att0", "res0", "ln1", "att1", "res1", "ff_ln", "geglu", "ff", "out")
# The temporal modules' taps, per pixel and head: a region is hd = 8 .. 128 values, and the emulation's noise in 8 values is a
# poor yardstick for one of them — measured on an MI355X over the 101 cases of tests/test_gpu_vda_errloc.py at the tap constants
# (A_TAP 3.5, B_TAP 5.5): worst 3.14 global, 15.0 per region (``geglu`` at C = 64: one product of two rounded factors against a
# region whose emulated noise happened to be 4e-4; ``att`` 7.3), and the engine's arrangement restated in torch (test_errloc_vda.py)
# gives the same figures.  By the rule of the constants above — about twice the worst measured, for all cases at once (at B = 30 the
# floor tau / B is smaller and the same runs read 3.14 / 20.9; profiles/vda_temporal_errloc.txt):
A_VDA_TAP, B_VDA_TAP = 6.5, 30.0

# the light inpaint nets (csrc/light_inpaint.hip): 4 x 4 pixels per level-1 token, pad bottom / right only (origin 0).  (64, 64) output
# pixels = one 16 x 16 level-1 window = one 8 x 8 level-2 window, and the default half-cell shift is the shifted blocks' partition;
# (32, 128) = the 8 x 32-token patch of a conv workgroup at level 1.  Taps at token resolution: the window and the conv patch of the level
INPAINT_IMAGE = "inpaint.light_inpaint_v1"
INPAINT_VIDEO = ("inpaint.light_video_inpaint_v1", "inpaint.light_video_inpaint_v1_medium", "inpaint.light_video_inpaint_v1_large")
INPAINT = (INPAINT_IMAGE,) + INPAINT_VIDEO
INPAINT_CELLS = ((64, 64), (32, 128))
INPAINT_TAP_CELLS = {1: ((16, 16), (8, 32)), 2: ((8, 8), (8, 32))}

# Thresholds: about twice the worst ratios measured on an MI355X over every case of tests/test_gpu_swin_errloc.py (its docstring)
A_OUT, B_OUT, TAU_OUT = 2.5, 3.75, 5e-4          # clamped [0,1] outputs (worst 1.16 / 1.82); tau = one fp16 ulp in [0.5, 1)
A_TAP, B_TAP = 3.5, 5.5                          # NHWC debug taps per 6 x 6 window and head (worst 1.69 / 2.78)
TAP_TAU_REL = 2e-3                               # tap tau = 2e-3 x the tap's rms
# the side nets (unclamped flows, softmax weights, mask logits; tau = TAP_TAU_REL x the map's rms): about twice the worst ratios
# measured on an MI355X over every case of tests/test_gpu_sidenet_errloc.py (its docstring): 1.03 global, 1.80 per region
A_SIDE, B_SIDE = 2.1, 3.6
# fp32 kernels (delta_warp): e_hip <= K_WARP e_ref + floor over the whole map and per (8, 8) cell, e_ref = the oracle's own fp32 error.
# The floor is WARP_FLOOR_ULPS ulp of the normalised sampling coordinate (``warp_floor``); K_WARP stays at the project's 2.2 (the
# measured worst k is below half of it, and a k below 1 would ask the engine to beat the fp32 reference)
K_WARP, WARP_FLOOR_ULPS = 2.2, 1.0


def warp_floor(c):
    """The error of a bilinear sample of ``c`` [B,C,H,W] whose normalised coordinates (gx + 1, gy + 1 in [1, 2) over the right / lower
    half, align_corners) are off by WARP_FLOOR_ULPS fp32 ulp each: 2^-23 (W - 1) / 2 pixels times the steepest horizontal step, plus
    the same vertically.  Two correct fp32 evaluations differ by this much wherever one of them happens to land on an exact pixel (a
    zero flow: the oracle's fp32 error is 5.5e-8 in cells where the kernel's is 1.4e-6 = 0.6 ulp at W = 131), so a fixed 1e-6 is not
    a floor for images wider than about 60 pixels."""
    h, w = c.shape[2:]
    sx = float((c[..., :, 1:] - c[..., :, :-1]).abs().max()) if w > 1 else 0.0
    sy = float((c[..., 1:, :] - c[..., :-1, :]).abs().max()) if h > 1 else 0.0
    return WARP_FLOOR_ULPS * 2.0 ** -23 * (0.5 * (w - 1) * sx + 0.5 * (h - 1) * sy)


def vda_pe_keys(sd):
    """{``...attention_blocks.a.pos_encoder.pe``: C} of the 4 x 2 temporal attention blocks of a Video-Depth-Anything state dict."""
    out = {}
    for k, v in sd.items():
        if k.startswith("head.motion_modules.") and k.endswith("to_q.weight"):
            out[k[:-len("to_q.weight")] + "pos_encoder.pe"] = v.shape[0]
    return out


def vda_with_pe(sd, base=None):
    """``sd`` with the fp32 position table of every temporal attention block under its ``pos_encoder.pe`` key ([1, 32, C], the
    published buffer's shape), computed HERE — outside any emulation mode, as the reference's buffer is made at construction.  Keys
    that ``base`` (the state dict the weights came from) already carries are taken from it as they are."""
    out = dict(sd)
    for k, c in vda_pe_keys(sd).items():
        with torch._C.DisableTorchFunction():
            out[k] = base[k].float().clone() if base is not None and k in base else VN.positional_encoding(c).unsqueeze(0)
    return out


def _vda_temporal(sd, x, module, hw, taps):
    """T frames [T, P, C] of module ``module``'s input, one per streaming step from an empty cache -> [T, P, C]."""
    (H, W), (T, P, C) = hw, x.shape
    assert H * W == P, (hw, x.shape)
    cache, outs, per = [None, None], [], []
    for f in x:
        tp = {} if taps is not None else None
        y, cache = VN.temporal_module(sd, f"head.motion_modules.{module}.", f.reshape(1, H, W, C).permute(0, 3, 1, 2), cache, taps=tp)
        outs.append(y.permute(0, 2, 3, 1).reshape(1, P, C))
        per.append(tp)
    if taps is not None:
        taps.update({k: torch.cat([d[k] for d in per]) for k in per[0]})
    return torch.cat(outs)


def _vda_stream(sd, x):
    st = VN.new_state()
    return torch.stack([VN.infer_video_depth_one(sd, f, st) for f in x])


def _forward(sd, x, name, taps=None, no_clip=False, max_depth=0.0, infer=False, soft=None, module=None, hw=None):
    if name == VDA_TEMPORAL:
        return _vda_temporal(sd, x, module, hw, taps)
    if name == VDA_STREAM:
        assert taps is None, "the streaming net has no taps here"
        return _vda_stream(sd, x)
    if name in INPAINT:
        assert not no_clip and not infer and max_depth == 0.0 and soft is not None, "the inpaint nets take the soft mask only"
        # x: the pre-processed frames x (1 - hard mask), soft: the fp32 soft mask (``inpaint_preprocess``); taps: a dict to fill
        return (OL.forward if name == INPAINT_IMAGE else OL.video_forward)(sd, x, soft, taps=taps)
    if name == DEPTH_ANYTHING:
        assert not no_clip and not infer, "the depth engine has no no_clip / infer"
        # x: [B,3,h,w] ImageNet-normalised; taps = the four encoder blocks that feed the head (None: the checkpoint's default)
        return ODA.model_forward(sd, x, taps=taps, max_depth=max_depth).unsqueeze(1)
    if name == DEPTH_AA:
        assert taps is None and not no_clip, "DepthAA has no taps / no_clip"
        return ODAA.infer(sd, x) if infer else ODAA.forward(sd, x, clamp=False)
    assert max_depth == 0.0 and not infer, "max_depth / infer are options of the depth path"
    if name == ROW_FLOW or name in MLBW:
        assert taps is None and not no_clip, "the side nets have no taps / no_clip"
        # x: the [B,3,h,w] feature planes (depth | divergence | convergence); unclamped flows, softmax weights, mask logits
        return ORF.delta_forward(sd, x) if name == ROW_FLOW else OM.delta_forward(sd, x, MLBW[name][0])
    if name in ("waifu2x.cunet", "waifu2x.upcunet"):
        return OC.model_forward(sd, x, no_clip=no_clip, taps=taps)
    if name in ("waifu2x.vgg_7", "waifu2x.upconv_7"):
        return OC.conv_stack_forward(sd, x, taps=taps)
    assert not no_clip, "no_clip is a cunet option"
    if name in V2_SCALE:
        return OV.model_forward(sd, x, V2_SCALE[name], taps=taps)
    return torch.clamp(O.unet_forward(sd, x, O.GEOMETRY.get(name, (0, 0, 0, SCALE[name]))[3], taps=taps), 0.0, 1.0)


def inpaint_preprocess(x, mask, pre=None, taps=None):
    """``oracle.light_inpaint.preprocess`` of the frames x (any float type) and the bool hole mask: (x (1 - hard), soft).  The soft mask
    is fp32 in every precision, as in the reference (``mask.float()``, an fp32 gaussian), and it is computed OUTSIDE the fp16
    emulation: the token decision max(soft) > 0.99 and the compose weights are then the same for the oracle, the emulation and the
    engine (which blurs in fp32 too)."""
    return OL.preprocess(x, mask, taps=taps, **(pre or {}))


def oracle64(sd, x, name, taps=None, no_clip=False, **kwargs):
    """The oracle forward with the state dict and the input cast to float64 (float64 output, clamped like the wrapper).
    ``kwargs``: ``max_depth`` (the depth engine's metric head), ``infer`` (DepthAA.infer instead of forward(clamp=False)); the inpaint
    nets: ``mask`` (bool holes) and ``pre`` (the options of ``preprocess``), x = the frames as given to ``infer``."""
    if name in (VDA_TEMPORAL, VDA_STREAM):
        sd = vda_with_pe(sd, sd)
    sd64 = {k: (v.double() if v.is_floating_point() else v) for k, v in sd.items()}
    if name in INPAINT:
        xp, soft = inpaint_preprocess(x.double(), kwargs["mask"], kwargs.get("pre"), taps)
        return _forward(sd64, xp, name, taps, soft=soft)
    return _forward(sd64, x.double(), name, taps, no_clip, **kwargs)


def emulated(sd, x, name, taps=None, no_clip=False, **kwargs):
    """The reference's own GPU arithmetic: fp16 parameters, every op result rounded to fp16 (oracle/fp16_emulation.py).
    ``half_weights`` keeps every key containing ``norm`` in fp32: that is right for the ViT LayerNorms of the depth engine
    (``pretrained.blocks.*.norm1 / norm2``, ``pretrained.norm``), which autocast runs in fp32 with fp32 parameters."""
    if name in INPAINT:
        xp, soft = inpaint_preprocess(x.float(), kwargs["mask"], kwargs.get("pre"), taps)
        with fp16_autocast_emulation():
            return _forward(half_weights(sd), xp, name, taps, soft=soft)
    if name in (VDA_TEMPORAL, VDA_STREAM):
        # ``pe_inside`` (tests only): leave the table to ``temporal_module``, i.e. evaluate it inside the mode — the trap
        pe_inside = kwargs.pop("pe_inside", False)
        hw16 = half_weights(sd)
        if pe_inside:
            hw16 = {k: v for k, v in hw16.items() if not k.endswith("pos_encoder.pe")}
        else:
            hw16 = vda_with_pe(hw16, sd)          # the fp32 buffer, not rounded with the parameters
        with fp16_autocast_emulation():
            return _forward(hw16, x.float(), name, taps, no_clip, **kwargs)
    with fp16_autocast_emulation():
        return _forward(half_weights(sd), x.float(), name, taps, no_clip, **kwargs)


def depth_aa_pad(h, w):
    """(ph1, pw1): the top / left part of DepthAA's centred replicate pad to multiples of 16 (oracle/depth_aa.py forward)."""
    return (16 - h % 16) // 2, (16 - w % 16) // 2


def mlbw_pad(h, w):
    """(ph1, pw1): the top / left part of MLBW's centred replicate pad to multiples of 4 x 32 (oracle/mlbw.py delta_forward)."""
    return (4 - h % 4) // 2, (32 - w % 32) // 2


def cells_for(name, origin=0, shape=None, level=None):
    """[(cell, offset)] of the windows of every level mapped to output pixels: the aligned partition of each level.
    ``origin``: the tile-output pixel the compared map starts at (a crop of the tile output).
    The side nets have rectangular cells: entries ((cell_h, cell_w), (off_y, off_x)[, (shift_y, shift_x)]); the shift is the second
    partition ``localised_stats`` looks at (default: half a cell both ways).  row_flow_v3 pads bottom / right only (origin 0); MLBW pads
    centred, so its windows start at (-ph1, -pw1) of the ``shape`` = (h, w) output, and its shifted blocks sit 2 tokens further
    (sy / sx of nunif_hip_mlbw_create: (2, 2) tokens = (2, 16) pixels for the full nets, (0, 2) = (0, 16) for the small ones).
    The depth engine: cells (14, 14) / (56, 56) / (8, 32) from pixel 0, shifted by half a cell.  DepthAA: (16, 16) cells from
    (-ph1, -pw1) of the ``shape`` = (h, w) map (``depth_aa_pad``), the second partition 8 pixels further.
    The inpaint nets: (64, 64) and (32, 128) output pixels from pixel 0; ``level`` = 1 / 2: the cells of a tap at that token resolution."""
    if name in INPAINT:
        return [(c, (0, 0)) for c in (INPAINT_CELLS if level is None else INPAINT_TAP_CELLS[level])]
    if name == VDA_TEMPORAL:                        # [T, C, 1, P] views: every pixel of every frame is a region
        return [(VDA_TEMPORAL_CELL, (0, 0))]
    if name == VDA_STREAM:
        return [(c, (0, 0)) for c in DEPTH_ANYTHING_CELLS]
    assert level is None, "level is an option of the inpaint nets"
    if name == ROW_FLOW:
        return [(c, (0, 0)) for c in ROW_FLOW_CELLS]
    if name == DEPTH_ANYTHING:                      # no pad: tokens, token blocks and conv patches all start at pixel 0
        return [(c, (0, 0)) for c in DEPTH_ANYTHING_CELLS]
    if name == DEPTH_AA:
        ph1, pw1 = depth_aa_pad(*shape)
        return [(DEPTH_AA_CELL, ((-ph1) % DEPTH_AA_CELL[0], (-pw1) % DEPTH_AA_CELL[1]), DEPTH_AA_SHIFT)]
    if name in MLBW:
        ph1, pw1 = mlbw_pad(*shape)
        return [(MLBW_CELL, ((-ph1) % MLBW_CELL[0], (-pw1) % MLBW_CELL[1]), (0, 16) if MLBW[name][1] else (2, 16))]
    if name in CUNET_SCALE:
        s = CUNET_SCALE[name]
        return [(c * s, (-origin) % (c * s)) for c in CUNET_CELLS]
    if name in V2_SCALE:
        s = V2_SCALE[name]
        return [(ws * s, (-s - origin) % (ws * s)) for ws, _ in V2_WINDOWS]
    s = SCALE[name]
    return [(6 * s * 2 ** k, (-origin) % (6 * s * 2 ** k)) for k in range(3)]


def v2_blocks(n1=2, n2=4, n3=3):
    """{block name: (window, shifted)} of the WAC blocks of swin_unet_v2 in forward order (oracle/swin_unet_v2.py model_forward)."""
    out = {"ir.path2.2": (8, True), "ir.path2.3": (8, False)}
    for group, n, windows in (("wac1", n1, (8, 6)), ("wac2", n2, (8,) * n2), ("wac3", n3, (8,) * n3)):
        for i, sh in enumerate(OV.shift_config(n)):
            out[f"{group}.blocks.{i}"] = (windows[i], sh)
    return out


def v2_tap_cells(name, tap, blocks=None):
    """(cells, group) of the swin_unet_v2 debug tap ``tap`` of net ``name``, at the tap's own resolution.  A block's maps (``<block>``,
    ``<block>.att``): one cell per window of the block, starting at -ws / 2 where the block is shifted (``localised_stats`` adds the
    partition half a window further, so both partitions are looked at for every block); group = 32 channels (one head) for ``att``,
    16 (one MFMA n-tile of the GEMM / conv epilogues) for the outputs.  ``ir`` is the pixel-shuffled half-resolution map (windows of
    16 pixels), ``patch`` / ``down1`` / ``up1`` take the 8 x 8 windows of their level, ``residual`` the cells of the output."""
    blocks = blocks or v2_blocks()
    if tap == "residual":
        return cells_for(name), None
    if tap in ("ir", "patch", "down1", "up1"):
        return [(16 if tap == "ir" else 8, 0)], 16
    block = tap[:-len(".att")] if tap.endswith(".att") else tap
    ws, shifted = blocks[block]
    return [(ws, (-(ws // 2)) % ws if shifted else 0)], (32 if tap.endswith(".att") else 16)


def _pair(v):
    """An int cell / offset means the same on both axes; a (y, x) pair is taken as it is."""
    return (v, v) if isinstance(v, int) else (int(v[0]), int(v[1]))


def region_max(err, cell, offset=0, group=None):
    """max |err| over channels (or over each group of ``group`` channels) inside each ``cell x cell`` block, per image.
    err: [B, C, H, W].  Block boundaries sit at ``offset + k * cell``; the partial blocks at the borders are regions too.
    ``cell`` / ``offset``: an int, or (cell_h, cell_w) / (off_y, off_x) for rectangular blocks.
    Returns [B, G, nby, nbx] (G = 1 without ``group``)."""
    e = err.abs()
    b, c, h, w = e.shape
    g = c if group is None else group
    e = e.reshape(b, c // g, g, h, w).amax(2)
    (ch, cw), (oy, ox) = _pair(cell), _pair(offset)
    top, left = (ch - oy % ch) % ch, (cw - ox % cw) % cw
    bottom = (-(h + top)) % ch
    right = (-(w + left)) % cw
    e = F.pad(e, (left, right, top, bottom))                # |err| >= 0: zero padding never wins a max
    return F.max_pool2d(e, (ch, cw), (ch, cw))


def _argmax_channel(err, bi, gi, group, cell, offset, ry, rx):
    e = err[bi].abs()
    if group is not None:
        e = e[gi * group:(gi + 1) * group]
    (ch, cw), (oy, ox) = _pair(cell), _pair(offset)
    top, left = (ch - oy % ch) % ch, (cw - ox % cw) % cw
    y0, x0 = max(0, ry * ch - top), max(0, rx * cw - left)
    y1, x1 = ry * ch - top + ch, rx * cw - left + cw
    blk = e[:, y0:y1, x0:x1]
    ch = int(blk.reshape(blk.shape[0], -1).amax(1).argmax())
    return ch + (gi * group if group is not None else 0), (y0, x0)


def _band(ry, rx, ny, nx):
    parts = [n for n, hit in (("top", ry == 0), ("bottom", ry == ny - 1), ("left", rx == 0), ("right", rx == nx - 1)) if hit]
    return "+".join(parts) if parts else "interior"


def localised_stats(y, y64, yemu, cells, B=1.0, tau=0.0, group=None):
    """Per-region ratios without asserting.  ratio = region_max(err) / (region_max(noise) + tau / B): the region fails iff
    ratio > B.  Returns {"global": max|err| / max|noise|, "worst": ratio, "bands": {band: worst ratio}, "regions": [...]}"""
    err = y.double() - y64.double()
    noise = yemu.double() - y64.double()
    out = {"global": float(err.abs().max() / noise.abs().max().clamp_min(1e-30)), "worst": 0.0, "bands": {}, "regions": []}
    for cell, base, *shift in cells:
        if isinstance(cell, int):
            offsets = sorted({base % cell, (base + cell // 2) % cell})
        else:                                               # rectangular: (cell_h, cell_w), (off_y, off_x)[, (shift_y, shift_x)]
            (ch, cw), (by, bx) = _pair(cell), _pair(base)
            sy, sx = _pair(shift[0]) if shift else (ch // 2, cw // 2)
            offsets = sorted({(by % ch, bx % cw), ((by + sy) % ch, (bx + sx) % cw)})
        for off in offsets:
            r = region_max(err, cell, off, group)
            re = region_max(noise, cell, off, group)
            ratio = r / (re + tau / B)
            nb, ng, ny, nx = ratio.shape
            flat = ratio.flatten()
            k = min(5, flat.numel())
            vals, idx = flat.topk(k)
            for v, i in zip(vals.tolist(), idx.tolist()):
                bi, rem = divmod(i, ng * ny * nx)
                gi, rem = divmod(rem, ny * nx)
                ry, rx = divmod(rem, nx)
                out["regions"].append({"ratio": v, "image": bi, "group": gi, "cell": cell, "offset": off, "row": ry, "col": rx,
                                       "band": _band(ry, rx, ny, nx), "err": float(r[bi, gi, ry, rx]),
                                       "noise": float(re[bi, gi, ry, rx])})
            for bi in range(nb):
                for ry in range(ny):
                    for rx in ((0, nx - 1) if 0 < ry < ny - 1 else range(nx)):
                        band = _band(ry, rx, ny, nx)
                        out["bands"][band] = max(out["bands"].get(band, 0.0), float(ratio[bi, :, ry, rx].max()))
            if ny > 2 and nx > 2:
                out["bands"]["interior"] = max(out["bands"].get("interior", 0.0), float(ratio[:, :, 1:-1, 1:-1].max()))
            out["worst"] = max(out["worst"], float(flat.max()))
    out["regions"].sort(key=lambda d: -d["ratio"])
    out["_err"], out["_group"], out["_B"], out["_tau"] = err, group, B, tau
    out["_gmax"], out["_nmax"], out["_finite"] = float(err.abs().max()), float(noise.abs().max()), bool(torch.isfinite(y).all())
    return out


def format_regions(st, n=5):
    lines = []
    for d in st["regions"][:n]:
        ch, (py, px) = _argmax_channel(st["_err"], d["image"], d["group"], st["_group"], d["cell"], d["offset"], d["row"], d["col"])
        lines.append(f"  image {d['image']} {d['band']:>17s} region (row {d['row']}, col {d['col']}) of cell {d['cell']} offset "
                     f"{d['offset']} [pixel {py},{px}] channel {ch}: err {d['err']:.3e} noise {d['noise']:.3e} ratio {d['ratio']:.2f}")
    return "\n".join(lines)


def assert_localised(st, A, B, tau, label=""):
    """The asserts of ``check_localised`` on stats that ``localised_stats`` computed with the same ``B`` and ``tau`` (for a caller
    that prints the figures before it asserts)."""
    assert (st["_B"], st["_tau"]) == (B, tau), f"{label}: stats computed with B {st['_B']}, tau {st['_tau']}, asserted with {B}, {tau}"
    assert st["_finite"], f"{label}: non-finite values"
    gmax, nmax = st["_gmax"], st["_nmax"]
    bands = " ".join(f"{k} {v:.2f}" for k, v in sorted(st["bands"].items()))
    msg = (f"{label}: max|err| {gmax:.3e} (noise {nmax:.3e}, A {A}), worst region ratio {st['worst']:.2f} (B {B}, tau {tau}); "
           f"bands: {bands}\n" + format_regions(st))
    assert gmax <= A * nmax, msg
    assert st["worst"] <= B, msg
    return st


def check_localised(y, y64, yemu, cells, A, B, tau, group=None, label=""):
    """Assert the global bound (a) and the per-region bound (b); the message names the 5 worst regions and the band of each (c).
    y / y64 / yemu: [B, C, H, W] (NHWC maps: pass them permuted).  Returns the stats (``localised_stats``)."""
    assert y.shape == y64.shape == yemu.shape, (label, y.shape, y64.shape, yemu.shape)
    assert bool(torch.isfinite(y).all()), f"{label}: non-finite values"
    return assert_localised(localised_stats(y, y64, yemu, cells, B, tau, group), A, B, tau, label)


def summary(st):
    return {"global": round(st["global"], 3), "worst": round(st["worst"], 3),
            "bands": {k: round(v, 3) for k, v in sorted(st["bands"].items())}}


def nhwc(t):
    return t.permute(0, 3, 1, 2)


def set_threads():
    """The oracle on at most 16 threads (the machine may report many more cores than this job may use)."""
    import os
    torch.set_num_threads(max(1, min(16, os.cpu_count() or 8)))


def psnr_db(a, b):
    mse = torch.mean((a.double() - b.double()) ** 2).item()
    return 10.0 * math.log10(1.0 / (mse + 1.0e-6))


def check_render_tile(out, sd, img, name, tile, ti, tj, no_clip=False, label=""):
    """``check_net`` of tile (ti, tj) of a whole-frame render ``out`` [3, H s, W s] of ``img`` [3, H, W] by one of the cunet engine's
    nets (no blending: a tile's output lands in the frame as it is, cut at the frame's edge).  The tile's input is cut from the
    replicate-padded frame as the renderer cuts it (oracle/seam_blending.py create_config)."""
    from oracle import seam_blending as OS
    s, off = CUNET_SCALE[name], CUNET_OFFSET[name]
    cfg = OS.create_config(img.shape[1], img.shape[2], s, off, tile, 0)
    xp = F.pad(img[None], cfg["pad"], mode="replicate")[0]
    i0, j0 = ti * cfg["input_tile_step"], tj * cfg["input_tile_step"]
    o0, o1, to = ti * cfg["output_tile_step"], tj * cfg["output_tile_step"], tile * s - 2 * off
    sub = out[:, o0:o0 + to, o1:o1 + to].cpu()
    assert sub.numel() > 0, (ti, tj, out.shape)
    return check_net(sub, sd, xp[:, i0:i0 + tile, j0:j0 + tile][None], name, crop=(0, sub.shape[1], 0, sub.shape[2]),
                     label=label or f"{name} render tile ({ti},{tj})", no_clip=no_clip)


def check_net(y, sd, x, name, origin=0, crop=None, label="", no_clip=False):
    """``check_localised`` of an engine output against the float64 oracle and the emulation of the same forward.  ``crop``: the
    (row0, row1, col0, col1) window of the tile output that ``y`` holds; ``origin`` = row0 = col0 of it."""
    with torch.inference_mode():
        set_threads()
        y64, ye = oracle64(sd, x, name, no_clip=no_clip), emulated(sd, x, name, no_clip=no_clip)
    if crop is not None:
        r0, r1, c0, c1 = crop
        y64, ye = y64[..., r0:r1, c0:c1], ye[..., r0:r1, c0:c1]
    y = y.reshape(y64.shape)
    return check_localised(y, y64, ye, cells_for(name, origin), A_OUT, B_OUT, TAU_OUT, label=label or name)
