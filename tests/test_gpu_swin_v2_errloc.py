"""swin_unet_v2 on the HIP engine (csrc/swin_unet_v2.hip) block by block, and its window attention alone, against float64.

The net (``nunif_hip_swin_unet_v2_debug_taps``; cases and references in ``tests/swin_v2_cases.py``): 1x / 2x / 4x at the smallest
valid tile (T = 64: 48 x 48 and 24 x 24 maps, the IR blocks at 32 x 32), 2x at batch 3 (heads = 3: unit counts that leave idle waves
in the last workgroup) and at T = 112, and the loud-bias 2x net (``qkv_proj.bias`` N(0, 0.5): the padded tokens of the shifted
windows are keys / values that differ from zero).  Every tap — the IR map, ``patch``, ``down1``, ``up1``, the fp32 residual image, and
for each of the 11 WAC blocks its output and its ``att`` map (the attention before head_proj) — goes through ``errloc`` against the
float64 oracle with the fp16-autocast emulation's own tap as the yardstick: per window of the block (aligned and half-window
partitions), per head (``att``) or 16 channels, limits A_TAP / B_TAP = 3.5 / 5.5 with tau = 2e-3 x the tap's rms; the output under
A_OUT / B_OUT = 2.5 / 3.75.  ``z`` of the debug entry is bit-equal to ``forward``'s.

The attention alone (``nunif_hip_swin_unet_v2_debug_wattn``: the kernel instance and the launch of ``run_wac``) against a float64
evaluation of the same base-2 expression on the same fp16 values: e_hip <= 2.2 e_ref + half an fp16 ulp of the region's largest
reference magnitude, e_ref = that expression in fp32 torch rounded to fp16, over the whole map and per (window, head), tokens inside
the map only; bqkv and the table at O(1).  Shapes: one window of 8 (two idle waves), 8 x 8 shifted (four windows, each three quarters
padding), 16 x 24 x 3 shifted (H != W, 3 heads), 24 x 24 with 8 heads, one window of 6, and 12 x 18 x 2 with SHIFTED windows of 6
and H != W — the registered nets shift only windows of 8 and are square, so these two paths ran nowhere before.

Measured on an MI355X (tools/swin_v2_errloc.py, profiles/swin_v2_errloc.txt; ratio = engine error / bound's yardstick):
    taps, worst over the six net cases      global   per region   where
    all 27 taps                             1.33     2.14         wac3.blocks.2 / wac1.blocks.0, 2x tile 64 batch 3 (limits 3.5 / 5.5)
    the 11 att taps                         1.19     1.84         wac3.blocks.1.att / wac3.blocks.0.att, 2x tile 64 batch 3
    up1 / down1 / patch / ir / residual     1.22 / 1.02 / 0.99 / 1.00 / 0.97 global, 2.12 / 1.65 / 1.59 / 1.44 / 1.47 per region
    output                                  0.55     0.76         loud-bias (limits 2.5 / 3.75)
    the attention alone, all six shapes     0.31     0.31         of the bound (limit 1); e_hip / e_ref = 1.00: the error is the one
                                                                  output rounding, on shifted windows of 6 and on H != W as well
"""
import pytest
import torch

import errloc as E
import swin_v2_cases as S

pytestmark = pytest.mark.gpu

_MODELS = {}


def make_model(scale, weights):
    """One model per (scale, weights) for the module."""
    key = (scale, weights)
    if key not in _MODELS:
        from nunif_amd.nunif.models import create_model
        import nunif_amd.waifu2x.utils  # noqa: F401  (registers the models)
        m = create_model(S.NAMES[scale]).eval()
        m.load_state_dict(S.state_dict(scale, weights), strict=True)
        _MODELS[key] = m.to("cuda:0")
    return _MODELS[key]


def measure_net(case):
    """{"out": stats of the image with the output limits' B / tau, tap name: stats with the tap limits' B / tau}"""
    scale, tile, batch, weights = case
    x, y64, ye, t64, te = S.references(case)
    m = make_model(scale, weights)
    with torch.inference_mode():
        xd = x.to("cuda:0")
        y, taps = m.engine().debug_taps(xd)
        assert torch.equal(y, m(xd)), "debug_taps' z != forward's"
        assert list(taps) == list(t64)
    name = S.NAMES[scale]
    out = {"out": E.localised_stats(y.cpu(), y64, ye, E.cells_for(name), E.B_OUT, E.TAU_OUT)}
    for tap in t64:
        out[tap] = S.tap_stats(name, tap, taps[tap].cpu(), t64[tap], te[tap])
    return out


def assert_net(stats, label):
    for k, st in stats.items():
        print(f"{label}: {k:18s} global {st['global']:.2f} worst region {st['worst']:.2f}")
    for k, st in stats.items():
        if k == "out":
            E.assert_localised(st, E.A_OUT, E.B_OUT, E.TAU_OUT, f"{label} out")
        else:
            E.assert_localised(st, E.A_TAP, E.B_TAP, st["_tau"], f"{label} {k}")


@pytest.mark.parametrize("case", S.NET_CASES, ids=S.case_id)
def test_net_tap_by_tap(hiplib, case):
    print()
    assert_net(measure_net(case), "v2 " + S.case_id(case))


def run_wattn(case, qkv, btab, bqkv):
    from nunif_amd.waifu2x.models.swin_unet_v2 import debug_wattn
    ws, shift = case[:2]
    return debug_wattn(qkv.to("cuda:0").contiguous(), btab.to("cuda:0"), bqkv.to("cuda:0"), ws, shift)


def measure_wattn(case):
    qkv, btab, bqkv, ref64, ref32h, _ = S.wattn_references(case)
    with torch.inference_mode():
        att = run_wattn(case, qkv, btab, bqkv).cpu()
    assert att.shape == (case[5], case[2], case[3], case[4]) and att.dtype == torch.float16
    return S.wattn_stats(case, S.wattn_to_windows(case, att), ref64, ref32h)


@pytest.mark.parametrize("case", S.WATTN_CASES, ids=S.case_id)
def test_wattn_alone(hiplib, case):
    st = measure_wattn(case)
    print(f"\nwattn {S.case_id(case)}: whole map {st['global']:.3f} worst (window, head) {st['worst']:.3f} of the bound, "
          f"e_hip / e_ref {st['k']:.2f}")
    assert st["finite"]
    assert st["global"] <= 1.0 and st["worst"] <= 1.0, st


@pytest.mark.parametrize("case", [S.WATTN_CASES[2], S.WATTN_CASES[5]], ids=S.case_id)
def test_wattn_invariants(hiplib, case):
    """Image b of a batch equals the single call; two calls and two streams are bit-equal."""
    qkv, btab, bqkv = S.wattn_references(case)[:3]
    with torch.inference_mode():
        att = run_wattn(case, qkv, btab, bqkv)
        for b in range(case[5]):
            one = case[:5] + (1,)
            assert torch.equal(att[b:b + 1], run_wattn(one, qkv[b:b + 1], btab, bqkv)), b
        assert torch.equal(att, run_wattn(case, qkv, btab, bqkv))
        s = torch.cuda.Stream()
        s.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(s):
            att2 = run_wattn(case, qkv, btab, bqkv)
        s.synchronize()
        assert torch.equal(att, att2)


def test_wattn_refuses_what_run_wac_refuses(hiplib):
    """A map that is not whole windows, a window other than 8 / 6, channels that are not heads of 32: an error, no launch."""
    from nunif_amd import _hip
    for ws, shift, H, W, C in ((8, False, 12, 8, 64), (8, True, 8, 20, 64), (4, False, 8, 8, 64), (7, True, 14, 14, 64),
                               (8, False, 8, 8, 48)):
        case = (ws, shift, H, W, C, 1)
        qkv = torch.zeros(1, H, W, 3 * C, dtype=torch.float16)
        with pytest.raises(_hip.NunifHipError):
            run_wattn(case, qkv, torch.zeros(ws * ws, ws * ws), torch.zeros(3 * C))
