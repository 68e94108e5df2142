"""The cases of the side-net localised checks (helper module, not a conftest): shared by ``test_errloc_sidenet.py`` (CPU, the
emulation standing in for the engine) and ``test_gpu_sidenet_errloc.py`` (the HIP engine), so that both run the same shapes.

A case is (net, (B, h, w), flip, regime).  The shapes are the smallest at which ``csrc/rowflow.hip`` or the WABlock it runs
(``csrc/wa_block.hip``: ``wmha_kernel`` and the block loop) takes another path:

row_flow_v3 (pad to multiples of 12 rows x 96 columns, bottom / right only and never zero; 8 pixels per token):
    (1, 58, 104)   the fixture's shape: 60 x 24 tokens
    (2, 12, 96)    already multiples: a full extra pad block (24 x 24 tokens per image)
    (1, 11, 95)    one below: 12 x 12 tokens = 9 windows of 4 x 4 and 16 of 3 x 3 (9 % 4 = 1: a wave tail; 16 % 4 = 0)
    (3, 25, 97)    one column past 96: the second 96-column block is padding but for one pixel; 3 images
    (1, 1, 8)      a single row, a single real token
    (1, 37, 193)   odd sizes
    (4, 392, 686)  152 064 tokens = 9504 windows of 4 x 4 > 4 x 2048: the grid-stride loop of wmha_kernel<4,64> runs
MLBW (centred pad to multiples of 4 x 32, never zero; windows of 4 x 4 tokens, blocks 0 / 2 zero-pad shifted):
    (1, 58, 104)   the fixture's shape          (2, 4, 32)    already multiples: ph1 = 2, pw1 = 16
    (1, 3, 31)     one below: ph1 = 0, pw1 = 0   (1, 21, 65)   odd sizes: ph1 = 1, pw1 = 15
    (2, 128, 504)  l4 only: 2 x 33 x 16 = 1056 windows of C = 128 (1156 in the shifted blocks) > 4 x 256: the grid-stride loop of wmha_kernel<4,128> runs
"""
import functools

import torch

import errloc as E
from oracle import mlbw as OM
from oracle import row_flow_v3 as ORF
from oracle.forward_warp import synth_depth

ROW_FLOW_SHAPES = [(1, 58, 104), (2, 12, 96), (1, 11, 95), (3, 25, 97), (1, 1, 8), (1, 37, 193)]
ROW_FLOW_BIG = (4, 392, 686)
MLBW_SHAPES = [(1, 58, 104), (2, 4, 32), (1, 3, 31), (1, 21, 65)]
MLBW_BIG = (2, 128, 504)
MLBW_SEEDS = {"sbs.mlbw_l2": 402, "sbs.mlbw_l4": 404, "sbs.mlbw_l2s": 412, "sbs.mask_mlbw_l2": 431}   # test_mlbw.py / test_hole_mask.py
OUTPUTS = {E.ROW_FLOW: ("delta",), "sbs.mask_mlbw_l2": ("delta", "weight", "mask")}

ROW_FLOW_CASES = [(E.ROW_FLOW, s, f, "benign") for s in ROW_FLOW_SHAPES for f in (False, True)]
ROW_FLOW_CASES += [(E.ROW_FLOW, ROW_FLOW_BIG, False, "benign"), (E.ROW_FLOW, (1, 58, 104), False, "hot")]
MLBW_CASES = [(n, s, f, "benign") for n in E.MLBW for s in MLBW_SHAPES for f in (False, True)]
MLBW_CASES += [("sbs.mlbw_l4", MLBW_BIG, False, "benign")]
CASES = ROW_FLOW_CASES + MLBW_CASES


def case_id(case):
    net, (b, h, w), flip, regime = case
    return f"{net.split('.')[1]}-{b}x{h}x{w}" + ("-flip" if flip else "") + ("-hot" if regime == "hot" else "")


def outputs(net):
    return OUTPUTS.get(net, ("delta", "weight"))


def row_flow_windows(shape, ws):
    """Windows of ws x ws tokens in the padded row_flow_v3 map of a (B, h, w) depth batch."""
    b, h, w = shape
    hp, wq = h + (12 - h % 12), (w + (96 - w % 96)) // 8
    return b * (hp // ws) * (wq // ws)


def mlbw_windows(shape, shifted=False):
    b, h, w = shape
    hp, wq = h + (4 - h % 4), (w + (32 - w % 32)) // 8
    return b * ((hp + (4 if shifted else 0)) // 4) * ((wq + (4 if shifted else 0)) // 4)


@functools.lru_cache(maxsize=None)
def state_dict(net, regime="benign"):
    if net == E.ROW_FLOW:
        return ORF.random_state_dict(301, regime=regime)
    layers, small, hole = E.MLBW[net]
    return OM.random_state_dict(MLBW_SEEDS[net], layers, small, hole_mask=hole, regime=regime)


def planes(shape, seed=7):
    """[B,3,h,w] feature planes (depth | divergence | convergence) as apply_divergence_nn_delta builds them."""
    b, h, w = shape
    return ORF.make_input(synth_depth(seed, b, h, w, "smooth_edges"), 2.0, 0.5, max(h, w))


def as_tuple(y):
    return y if isinstance(y, tuple) else (y,)


@functools.lru_cache(maxsize=None)
def references(case):
    """(x, float64 oracle outputs, fp16 emulation outputs) of one case, computed once per process and left unchanged.  With ``flip``
    the net sees the mirrored planes and its outputs stay in the mirrored frame (the engine's delta / weight do too; its mask
    logits come back in image coordinates and are mirrored by the caller before the comparison)."""
    net, shape, flip, regime = case
    E.set_threads()
    with torch.inference_mode():
        sd, x = state_dict(net, regime), planes(shape)
        xm = torch.flip(x, (3,)) if flip else x
        return x, as_tuple(E.oracle64(sd, xm, net)), as_tuple(E.emulated(sd, xm, net))


def tau_for(y64):
    """The relative floor of the taps: unclamped maps have no exact 0 / 1, but a region's emulation error can be anything down to
    3.4e-5 where the fp16 roundings happen to cancel, and division by that would decide the ratio."""
    return E.TAP_TAU_REL * float(y64.double().pow(2).mean().sqrt())


def stats(y, y64, ye, net, shape, B):
    return E.localised_stats(y, y64, ye, E.cells_for(net, shape=shape[1:]), B, tau_for(y64))
