"""The cases of the light-inpaint localised checks (helper module, not a conftest): shared by ``test_errloc_inpaint.py`` (CPU, the
emulation standing in for the engine) and ``test_gpu_inpaint_errloc.py`` (the HIP engine), so that both run the same shapes.

A case is (net, (B, H, W), flip, regime, pre, masks): ``pre`` names the options of ``preprocess`` (``PRE``), ``masks`` the hole mask of
every image ("comb", or a tuple with one of "comb" / "all" / "none" per image).  The frames pad to multiples of 64 pixels, bottom /
right only and always by 1..64; a level-1 token is 4 x 4 pixels (16 x 16 windows), a level-2 token 8 x 8 (8 x 8 windows).  The shapes are
the smallest at which ``csrc/light_inpaint.hip`` or a kernel it launches takes another path:

image net (C = 96: GLU conv as 64 + 32 output slices with Cin = 64, ``up`` on the swin PatchUp kernel):
    (1, 40, 56)    pads to 64 x 64: one window per level, 64 level-2 tokens (a partial 256-thread block, a GEMM M-tail), 4 windows in
                   the shifted blocks
    (2, 64, 64)    already multiples: a full extra 64 of replicate padding; 2 images
    (1, 63, 65)    one below / one above a multiple of 64
    (1, 100, 180)  non-square, 32 x 48 level-1 tokens; also with mirror_x, with the hot weights, with closing + dilation, and under
                   the three switches
    (3, 100, 200)  3 x 32 x 64 level-1 tokens = 24 conv patches of 8 x 32: the LAST count the LDS-staged conv takes
                   (``conv3_dma_applies``: n_patches > 24); image 1 is all hole, image 2 has no hole
    (1, 1, 1)      a single pixel (a hole: every token of the padded map is masked)
    (1, 270, 480)  80 x 128 level-1 tokens = 40 conv patches > 24: the sliced GLU conv of enc1 / dec1 runs on the persistent LDS-DMA
                   kernel (level 2: 10 patches, LDS-staged).  It crosses nothing in ``launch_gemm`` (40 - 54 row blocks)
    (1, 960, 961)  the smallest frame that pads to 1024 x 1024: 65 536 level-1 tokens = 256 row blocks of ``gemm_kernel`` (from 128
                   on the output tiles are no longer split over grid.y: ny = 1, nt_chunk = 0) and 16 384 level-2 rows, the count from
                   which the K = 384 products (``down``, proj_out of enc2) take the resident-weight ``gemm_res_kernel<12,2>``; with
                   NUNIF_GEMM_BIG_M=1 the level-1 proj_out (K = 192, 65 536 rows >= the 32 768 the resident MF = 4 form needs) runs
                   resident too, which the switch cannot reach at (1, 100, 180) / 12 x 40 x 56: there it only splits the
                   192 -> 768 Linear of ``lin()`` into two launches.  256 conv patches at level 1 (LDS-DMA, below its 512-workgroup
                   cap), 64 at level 2.  Not reached by any case: the resident K = 192 form at level 2 and the patch loop of the
                   persistent conv (> 512 patches), which need frames of 2048 x 2048 / 1024 x 2048 and more
video nets, 12 frames (enc1 unshifted, enc2 = [2-D shifted, temporal, 2-D, temporal, 2-D shifted], 1 x 1 image head):
    small  (C = 96)   12 x 40 x 56: 24 conv patches (LDS-staged);  12 x 72 x 136: 96 patches (LDS-DMA), 12 x 384 level-2 tokens
    medium (C = 128)  12 x 40 x 56: GLU conv unsliced (8 tiles, Cin 64), 24 patches (LDS-staged), ``up`` on the generic GEMM, the level-2
                      conv (Cin 128, 16 tiles) on ``conv_kernel``;  12 x 72 x 136: the same conv on the LDS-DMA kernel (96 patches)
    large  (C = 192)  12 x 40 x 56: level-1 conv as 128 + 64 slices with Cin = 96 (LDS-staged), level-2 conv on ``conv_kernel`` (Cin 192),
                      HOLD = false in the LayerNorm kernels (V = 768 at level 2)

Masks: token-aligned combs, hole strips 4 pixels wide every 16 pixels (every 32 where ``pre`` dilates: a strip grows to three tokens,
which at a period of 16 would mask 75 % of them), offset per image / frame, plus horizontal bars 4 pixels high every 48 rows.  The
composed output shows the net only where the soft mask is > 0 and a token with any hole pixel is replaced by ``mask_bias``, so the
mask decides what a check can see: ``test_errloc_inpaint.py`` asserts that these masks are fit.
"""
import functools

import torch
import torch.nn.functional as F

import errloc as E
from conftest import synth_image
from oracle import light_inpaint as OL

IMAGE = E.INPAINT_IMAGE
SMALL, MEDIUM, LARGE = E.INPAINT_VIDEO
SEEDS = {IMAGE: 701, SMALL: 801, MEDIUM: 811, LARGE: 812}                 # test_light_inpaint.py
DIMS = {SMALL: (96, 1), MEDIUM: (128, 2), LARGE: (192, 2)}
PRE = {
    "plain": {},
    "close": dict(closing=True, inner_dilation=1, outer_dilation=2),
    "close_bw": dict(closing=True, inner_dilation=1, outer_dilation=1, base_width=90),   # W / 90 = 2 steps per unit at W = 180
}

IMAGE_SHAPES = [(1, 40, 56), (2, 64, 64), (1, 63, 65), (1, 100, 180), (1, 1, 1), (1, 270, 480)]
MAIN, MAIN_VIDEO = (1, 100, 180), (12, 40, 56)                            # the shapes of the switches
BATCH = (IMAGE, (3, 100, 200), False, "benign", "plain", ("comb", "all", "none"))
IMAGE_CASES = [(IMAGE, s, False, "benign", "plain", "all" if s == (1, 1, 1) else "comb") for s in IMAGE_SHAPES] + [BATCH]
IMAGE_CASES += [(IMAGE, s, True, "benign", "plain", "comb") for s in ((1, 100, 180), (1, 63, 65))]
IMAGE_CASES += [(IMAGE, MAIN, False, "hot", "plain", "comb"), (IMAGE, MAIN, False, "benign", "close", "comb"),
                (IMAGE, MAIN, True, "benign", "close_bw", "comb")]
IMAGE_CASES += [(IMAGE, (1, 960, 961), False, "benign", "plain", "comb")]
VIDEO_CASES = [(SMALL, MAIN_VIDEO, False, "benign", "plain", "comb"), (SMALL, (12, 72, 136), False, "benign", "plain", "comb"),
               (SMALL, MAIN_VIDEO, True, "benign", "close", "comb"),
               (MEDIUM, MAIN_VIDEO, False, "benign", "plain", "comb"), (MEDIUM, (12, 72, 136), False, "benign", "plain", "comb"),
               (LARGE, MAIN_VIDEO, False, "benign", "plain", "comb")]
CASES = IMAGE_CASES + VIDEO_CASES
MAIN_CASE, MAIN_VIDEO_CASE, DMA_CASE, BIGGEST = IMAGE_CASES[3], VIDEO_CASES[0], IMAGE_CASES[5], IMAGE_CASES[12]
# a comb is fit when, after ``preprocess``, this share of the frame's tokens is masked (inside the 20 % - 60 % the CPU test asserts),
# no more than FIT_MAX of the padded map's, and every (64, 64) cell of the frame holds a hole pixel
FIT_MIN, FIT_MAX = 0.22, 0.58
SWITCHES = (("NUNIF_GEMM_BIG_M", "1"), ("NUNIF_LI_CONV_SLICES", "0"), ("NUNIF_PATCHUP", "0"))


def case_id(case):
    net, (b, h, w), flip, regime, pre, masks = case
    tag = {IMAGE: "image", SMALL: "small", MEDIUM: "medium", LARGE: "large"}[net]
    return (f"{tag}-{b}x{h}x{w}" + ("-flip" if flip else "") + ("-hot" if regime == "hot" else "") + ("" if pre == "plain" else "-" + pre)
            + ("" if masks == "comb" else "-" + (masks if isinstance(masks, str) else "+".join(masks))))


def mask_kinds(case):
    b, masks = case[1][0], case[5]
    return (masks,) * b if isinstance(masks, str) else masks


def is_comb(case):
    return all(k == "comb" for k in mask_kinds(case))


def conv_patches(shape, level=1):
    """8 x 32-token conv patches of the padded map of a (B, H, W) batch (kTH x kTW of the 3 x 3 conv kernels)."""
    b, h, w = shape
    hh, ww = (h + 64 - h % 64) // (4 * level), (w + 64 - w % 64) // (4 * level)
    return b * ((hh + 7) // 8) * ((ww + 31) // 32)


@functools.lru_cache(maxsize=None)
def state_dict(net, regime="benign"):
    if net == IMAGE:
        return OL.random_state_dict(SEEDS[net], regime=regime)
    assert regime == "benign"
    dim, ratio = DIMS[net]
    return OL.video_random_state_dict(SEEDS[net], base_dim=dim, lv2_mlp_ratio=ratio)


def frames(shape, seed=40):
    """[B,3,H,W] smooth noise in [0.1, 0.9] (not flat, not saturated); every image / frame from a seed of its own."""
    b, h, w = shape
    return torch.stack([0.1 + 0.8 * synth_image(seed + i, 3, h, w) for i in range(b)])


def masked_fraction(hard, padded=False):
    """Per image: the fraction of the level-1 tokens that hold a hole pixel of ``hard`` [B,1,H,W] (0 / 1), over the tokens with a
    pixel of the frame or (``padded``) over all tokens of the replicate-padded map."""
    h, w = hard.shape[2:]
    if padded:
        return F.max_pool2d(F.pad(hard.float(), (0, 64 - w % 64, 0, 64 - h % 64), mode="replicate"), 4).flatten(1).mean(1)
    return F.max_pool2d(hard.float(), 4, ceil_mode=True).flatten(1).mean(1)


def _comb(h, w, period, ox, oy):
    ys, xs = torch.arange(h).view(h, 1), torch.arange(w).view(1, w)
    return ((xs - ox) % period < 4) | ((ys - oy) % 48 < 4)


def is_fit(hard):
    """The fitness of one image's hard mask [1,1,H,W] (``FIT_MIN`` / ``FIT_MAX``).  The bound on the padded map is an upper one only:
    a strip or bar that ends on the last column / row is replicated through the padding (at 64 x 64 that is half of the map), and
    without one the padded map of that shape is at 18 %.  The partial cells at the right / bottom edge count as cells."""
    in_frame = FIT_MIN <= float(masked_fraction(hard)) <= FIT_MAX
    in_map = float(masked_fraction(hard, padded=True)) <= FIT_MAX
    return in_frame and in_map and float(F.max_pool2d(hard, 64, 64, ceil_mode=True).min()) == 1.0


def hole_mask(shape, kinds, pre=None):
    """[B,1,H,W] bool.  comb of image i: columns [ox, ox + 4) of every ``period`` and rows [oy, oy + 4) of every 48, starting from
    ox = 4 (i + 1), oy = 8 + 4 i and moved on by whole tokens until the mask ``is_fit``."""
    b, h, w = shape
    pre = pre or {}
    period = 32 if pre else 16
    m = torch.zeros(b, 1, h, w, dtype=torch.bool)
    for i, kind in enumerate(kinds):
        if kind == "all":
            m[i] = True
        elif kind == "comb":
            for k in range(12 * (period // 4)):
                cand = _comb(h, w, period, (4 * (i + 1 + k)) % period, (8 + 4 * i + 4 * (k // (period // 4))) % 48)[None, None]
                taps = {}
                OL.preprocess(torch.zeros(1, 3, h, w), cand, taps=taps, **pre)
                if is_fit(taps["hard"]):
                    break
            else:
                raise AssertionError(f"no fit comb for image {i} of {shape}")
            m[i] = cand[0]
        else:
            assert kind == "none", kind
    return m


def inputs(case):
    """(x, mask, pre): the frames as the engine gets them, the hole mask in the frame the net runs in, the preprocess options."""
    net, shape, flip, regime, pre, masks = case
    return frames(shape), hole_mask(shape, mask_kinds(case), PRE[pre]), PRE[pre]


@functools.lru_cache(maxsize=None)
def references(case):
    """{"x", "mask", "pre", "y64", "ye", "taps64", "tapse"} of one case, computed once per process and left unchanged.  With ``flip``
    the net sees the mirrored frames and ``y64`` / ``ye`` / the taps stay in the mirrored frame: the engine's ``mirror_x`` output is
    mirrored by the caller before the comparison."""
    net, shape, flip, regime, pre, masks = case
    E.set_threads()
    with torch.inference_mode():
        sd = state_dict(net, regime)
        x, mask, opts = inputs(case)
        xm = torch.flip(x, (3,)) if flip else x
        t64, te = {}, {}
        y64 = E.oracle64(sd, xm, net, taps=t64, mask=mask, pre=opts)
        ye = E.emulated(sd, xm, net, taps=te, mask=mask, pre=opts)
        return {"x": x, "mask": mask, "pre": opts, "y64": y64, "ye": ye, "taps64": t64, "tapse": te}


def tap_names(net):
    """The fp16 maps of the net in the order the engine writes them, with their level."""
    n2 = 4 if net == IMAGE else 5
    names = [("patch", 1), ("enc1.gmlp", 1), ("enc1", 1), ("down", 2)]
    for i in range(n2):
        names += [(f"enc2.{i}.gmlp", 2), (f"enc2.{i}", 2)]
    return names + [("up", 1), ("dec1.gmlp", 1), ("dec1", 1), ("to_image", 1)]


def tau_for(y64):
    """The relative floor of the taps (unclamped maps): TAP_TAU_REL x the map's rms."""
    return E.TAP_TAU_REL * float(y64.double().pow(2).mean().sqrt())


def output_stats(y, ref, net):
    return E.localised_stats(y, ref["y64"], ref["ye"], E.cells_for(net), E.B_OUT, E.TAU_OUT)


def tap_stats(t, t64, te, net, level, group=None):
    return E.localised_stats(t, t64, te, E.cells_for(net, level=level), E.B_TAP, tau_for(t64), group)
