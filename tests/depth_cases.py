"""The cases of the depth-path localised checks (helper module, not a conftest): shared by ``test_errloc_depth.py`` (CPU, the
emulation standing in for the engine) and ``test_gpu_depth_errloc.py`` (the HIP engine), so that both run the same shapes.

The depth engine (``iw3.depth_anything``).  A case is (encoder, (B, h, w), taps, max_depth); inputs are ``synth_image`` frames,
ImageNet-normalised; Np = 1 + (h / 14)(w / 14) tokens.  ``da_attn_kernel`` walks the keys 32 per step through a ring of three LDS
slots in a loop unrolled by six, one wave per 16 queries, 128 queries per workgroup; the shapes are the smallest that meet its edges:

    h x w      B  Np   what it meets
    28 x 28    1  5    the smallest accepted input: one masked key step, stage(1) / stage(2) fully clamped, 7 of 8 waves without a query
    56 x 112   1  33   the second key step holds one key
    112 x 112  2  65   the ring of three used once, plus one key
    112 x 224  1  129  the second query block holds one query
    140 x 224  1  161  exactly six steps, the end of the unrolled loop; a query-tile tail of 1
    168 x 224  3  193  seven steps: the loop wraps; batch 3
    42 x 70    2  16   an odd 3 x 5 grid: layer4 is 2 x 3, every resize runs between unequal sizes, maps far smaller than 8 x 32
    70 x 98    2  36   the shape of test_hip_backbone_variants_vs_restatement, with its six variants (seed 620, grid 8)
    112 x 224  1  129  ViT-B: the chunk-major layer3_rn / layer4_rn and the fc2 split into K halves at a two-block sequence

ViT-L gets no case of its own beyond the variants: its float64 forward takes seconds per image.

DepthAA (``iw3.depth_aa``, seed 501, ``synth_depth(..., "smooth_edges")`` as [B,1,h,w]).  A case is ((B, h, w), mode), mode
"forward" = forward(clamp=False), "infer" = infer on values in [3, 11]:

    16 x 16  1   the centred pad is a whole 16 (8 + 8)        5 x 9    1   smaller than a window (pad 5 + 6, 3 + 4)
    33 x 47  2   pad 15 (7 + 8) and 1 (0 + 1)                 31 x 95  1   pad 1 and 1 (0 + 1 both ways)
    64 x 80  3   batch 3, a whole 16 both ways                33 x 47  2   infer
"""
import functools

import torch

import errloc as E
from conftest import synth_image
from oracle import depth_aa as ODAA
from oracle import depth_anything_v2 as ODA
from oracle.forward_warp import synth_depth

NET, AA = E.DEPTH_ANYTHING, E.DEPTH_AA
VITS_SHAPES = [(1, 28, 28), (1, 56, 112), (2, 112, 112), (1, 112, 224), (1, 140, 224), (3, 168, 224), (2, 42, 70)]
VARIANT_SHAPE = (2, 70, 98)
VARIANTS = [("vitb", None, 0.0), ("vitl", None, 0.0), ("vitl", (20, 21, 22, 23), 0.0), ("vitb", None, 20.0), ("vits", None, 80.0),
            ("vits", (8, 9, 10, 11), 0.0)]                     # test_hip_backbone_variants_vs_restatement
VITB_CASE = ("vitb", (1, 112, 224), None, 0.0)
CASES = [("vits", s, None, 0.0) for s in VITS_SHAPES] + [(e, VARIANT_SHAPE, t, m) for e, t, m in VARIANTS] + [VITB_CASE]
BATCHED = [c for c in CASES if c[1][0] > 1]                      # image b alone: sliced from the batch's cached references
NP = {(28, 28): 5, (56, 112): 33, (112, 112): 65, (112, 224): 129, (140, 224): 161, (168, 224): 193, (42, 70): 16, (70, 98): 36}

AA_SHAPES = [(1, 16, 16), (1, 5, 9), (2, 33, 47), (1, 31, 95), (3, 64, 80)]
AA_INFER = ((2, 33, 47), "infer")
AA_CASES = [(s, "forward") for s in AA_SHAPES] + [AA_INFER]

# the seed of a shape's frames: 700 + h + w unless the input conditions of test_errloc_depth.py asked for another one (70 x 98: the last
# (8, 32) patch column is 2 pixels wide, and with seeds 868 / 300 its emulation noise is 11x / 10.1x below the loudest region's)
FRAME_SEEDS = {(70, 98): 310}
MEAN = torch.tensor([0.485, 0.456, 0.406]).view(1, 3, 1, 1)
STD = torch.tensor([0.229, 0.224, 0.225]).view(1, 3, 1, 1)


def tokens(h, w):
    return 1 + (h // 14) * (w // 14)


def case_id(case):
    enc, (b, h, w), taps, max_depth = case
    return f"{enc}-{b}x{h}x{w}" + (f"-taps{taps[0]}" if taps else "") + (f"-metric{int(max_depth)}" if max_depth else "")


def aa_case_id(case):
    (b, h, w), mode = case
    return f"{b}x{h}x{w}" + ("-infer" if mode == "infer" else "")


@functools.lru_cache(maxsize=None)
def _state_dict(encoder, variant):
    return ODA.random_state_dict(620, grid=8, encoder=encoder) if variant else ODA.random_state_dict(601)


def state_dict(encoder="vits", variant=False):
    """ViT-S: seed 601 (the 37 x 37 grid of the public checkpoint); the variants' weights: seed 620, grid 8.  One object per key."""
    assert variant or encoder == "vits"
    return _state_dict(encoder, bool(variant))


def case_state_dict(case):
    return state_dict(case[0], variant=case[1] == VARIANT_SHAPE or case[0] != "vits")


@functools.lru_cache(maxsize=None)
def aa_state_dict():
    return ODAA.random_state_dict(501)


def frames(shape, seed=None):
    """[B,3,h,w] ImageNet-normalised ``synth_image`` frames."""
    b, h, w = shape
    seed = FRAME_SEEDS.get((h, w), 700 + h + w) if seed is None else seed
    return (torch.stack([synth_image(seed + i, 3, h, w) for i in range(b)]) - MEAN) / STD


def aa_input(case):
    (b, h, w), mode = case
    d = synth_depth(9 + h, b, h, w, "smooth_edges")
    return 3.0 + 8.0 * d if mode == "infer" else d


@functools.lru_cache(maxsize=None)
def references(case):
    """(x, float64 oracle output, fp16 emulation output), both [B,1,h,w], of one depth-engine case; computed once per process and
    left unchanged (the maps are small; the float64 and the fp16-valued copies of the state dict live only inside the call)."""
    enc, shape, taps, max_depth = case
    E.set_threads()
    with torch.inference_mode():
        sd, x = case_state_dict(case), frames(shape)
        return x, E.oracle64(sd, x, NET, taps=taps, max_depth=max_depth), E.emulated(sd, x, NET, taps=taps, max_depth=max_depth)


@functools.lru_cache(maxsize=None)
def aa_references(case):
    shape, mode = case
    E.set_threads()
    with torch.inference_mode():
        sd, x = aa_state_dict(), aa_input(case)
        return x, E.oracle64(sd, x, AA, infer=mode == "infer"), E.emulated(sd, x, AA, infer=mode == "infer")


def tau_for(y64):
    """The relative floor of unclamped maps: TAP_TAU_REL x the map's rms (as ``sidenet_cases.tau_for``)."""
    return E.TAP_TAU_REL * float(y64.double().pow(2).mean().sqrt())


def cells(name, shape):
    return E.cells_for(name, shape=tuple(shape[-2:]))


def stats(y, y64, ye, name, B):
    return E.localised_stats(y, y64, ye, cells(name, y64.shape), B, tau_for(y64))


def old_asserts(y, ref):
    """Today's whole-map bar of test_depth_anything.py on [B,1,h,w] maps: (psnr >= 50 and rel < 1e-2, psnr, rel)."""
    span = float(ref.max() - ref.min())
    p = E.psnr_db(y / span, ref / span)
    rel = float((y.double() - ref.double()).pow(2).mean().sqrt() / ref.double().std())
    return p >= 50.0 and rel < 1e-2, p, rel


def check(y, y64, ye, name, label, capsys=None):
    """Print the figures of one [B,1,h,w] output, then assert the bounds of the side nets on them (A_SIDE, B_SIDE, tau_for)."""
    assert y.shape == y64.shape == ye.shape and y.dtype == torch.float32, (label, y.shape, y64.shape, y.dtype)
    st = stats(y, y64, ye, name, E.B_SIDE)
    line = (f"\nerrloc {label}: global {st['global']:.2f} worst {st['worst']:.2f} (err {st['_gmax']:.2e} noise {st['_nmax']:.2e}) "
            f"bands {E.summary(st)['bands']}")
    if capsys is None:
        print(line)
    else:
        with capsys.disabled():
            print(line)
    return E.assert_localised(st, E.A_SIDE, E.B_SIDE, tau_for(y64), label=label)


def check_fresh(y, sd, x, name, label, capsys=None, **kwargs):
    """``check`` against references computed here: for inputs that are not one of the cases (``kwargs``: taps, max_depth, infer)."""
    E.set_threads()
    with torch.inference_mode():
        y64, ye = E.oracle64(sd, x, name, **kwargs), E.emulated(sd, x, name, **kwargs)
    return check(y.reshape(y64.shape), y64, ye, name, label, capsys)
