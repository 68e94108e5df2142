"""swin_unet / swin_unet_v2 engines in their DEFAULT configuration (no debug taps) held window by window to a float64 oracle.

``tests/errloc.py``: per image, max|y - y64| <= A * max|emu - y64| and, in every region of the windows of levels 1-3 mapped to output
pixels (aligned and half-window-shifted partitions), region_max(y - y64) <= B * region_max(emu - y64) + tau, where emu is the
reference's own fp16-autocast arithmetic (``oracle/fp16_emulation.py``).  A whole-image PSNR cannot see a single wrong window at
the bench's tile (one level-1 window off by 0.1 reads 51 dB); this check catches 4e-3 there (``tests/test_errloc.py``).

Cases: every net (swin_unet 1x / 2x / 4x / 8x / 4xl, swin_unet_v2 1x / 2x / 4x) at tiles 64 (level-3 map 12 x 12: the shift wraps
inside 2 x 2 windows), 112 and 256 (the bench tile), batches 1 / 3 / 5 (remainder windows and waves), on ``synth_image`` and on
``hot_image`` (saturated flats); the two engine switches NUNIF_BLOCK96=1 / NUNIF_ATT_WM=0; the 1x seed-303 70 x 90 render that once
exposed a one-lane-group softmax stabiliser; every debug tap window by window and head by head; the resident-weight image head of the
4x / 8x nets (NUNIF_GEMM_BIG_M lowered) bit-equal to the ring form; the window-major attention map past 2 GiB of byte offsets.

Measured on an MI355X (ratio = engine error / emulation error; worst over the cases; thresholds in ``tests/errloc.py`` at about
twice the worst: A_OUT 2.5, B_OUT 3.75, A_TAP 3.5, B_TAP 5.5):
    outputs                       global max   worst region    case of the worst region
    swin_unet 1x / 2x / 4x        1.16         1.82            2x, tile 256, batch 1, synth (1x seed-303 render 1.81)
    swin_unet 8x / 4xl            0.95         1.27            4xl, tile 64, batch 3
    swin_unet_v2 1x / 2x / 4x     0.78         1.11            v2 2x, tile 64, batch 5, hot
    NUNIF_BLOCK96=1 / ATT_WM=0    1.14         1.75            2x, tile 256, batch 3, hot, ATT_WM=0
    resident-weight image head    1.05         1.68            4x, tile 208 (bit-equal to the ring form; 8x 1.13)
    taps (2x / 4x / 4xl)          1.69         2.78            4x up2 (2x 2.65, 4xl 1.74), per 6 x 6 window and head
Every output case reads 59.0-59.9 dB, so PSNR >= 50 says nothing here that the region bound does not.
"""
import functools

import pytest
import torch

import errloc as E
from conftest import hot_image, psnr, synth_image
from oracle import seam_blending as OS
from oracle import swin_unet as O

pytestmark = pytest.mark.gpu

SWIN = {"1x": ("waifu2x.swin_unet_1x", 1), "2x": ("waifu2x.swin_unet_2x", 2), "4x": ("waifu2x.swin_unet_4x", 4),
        "8x": ("waifu2x.swin_unet_8x", 8), "4xl": ("waifu2x.swin_unet_4xl", 4),
        "v2_1x": ("waifu2x.swin_unet_v2_1x", 1), "v2_2x": ("waifu2x.swin_unet_v2_2x", 2), "v2_4x": ("waifu2x.swin_unet_v2_4x", 4)}
SEED = {"1x": 101, "2x": 102, "4x": 104, "8x": 108, "4xl": 204, "v2_1x": 41, "v2_2x": 42, "v2_4x": 44}

# (net, tile, batch, input)
CASES = [
    ("2x", 256, 1, "synth"), ("2x", 256, 3, "hot"), ("2x", 112, 5, "synth"), ("2x", 64, 3, "hot"), ("2x", 64, 5, "synth"),
    ("1x", 64, 5, "hot"), ("1x", 112, 3, "synth"), ("1x", 256, 1, "synth"),
    ("4x", 64, 3, "synth"), ("4x", 112, 1, "hot"), ("4x", 256, 1, "synth"),
    ("8x", 64, 3, "synth"), ("8x", 112, 1, "hot"),
    ("4xl", 64, 3, "synth"), ("4xl", 112, 1, "hot"),
    ("v2_1x", 64, 3, "synth"), ("v2_1x", 112, 1, "hot"),
    ("v2_2x", 64, 5, "hot"), ("v2_2x", 112, 3, "synth"), ("v2_2x", 256, 1, "synth"),
    ("v2_4x", 64, 1, "synth"), ("v2_4x", 112, 3, "hot"),
]
SWITCH_CASES = [("2x", 256, 3, "hot"), ("2x", 112, 5, "synth"), ("1x", 64, 5, "hot"), ("4x", 64, 3, "synth")]
SWITCHES = [{"NUNIF_BLOCK96": "1"}, {"NUNIF_ATT_WM": "0"}]


def _id(c):
    return "-".join(str(v) for v in c)


def state_dict(net):
    name, sf = SWIN[net]
    if net.startswith("v2"):
        from nunif_amd import synthetic
        return synthetic.swin_unet_v2_state_dict(SEED[net], sf)
    if net == "4xl":
        return O.random_state_dict(SEED[net], 4, base_dim=192, layer_norm=True)
    return O.random_state_dict(SEED[net], sf)


def make_model(net):
    from nunif_amd.nunif.models import create_model
    import nunif_amd.waifu2x.utils  # noqa: F401  (registers every waifu2x model)
    m = create_model(SWIN[net][0]).eval()
    m.load_state_dict(state_dict(net), strict=True)
    return m.to("cuda:0")


def make_input(kind, tile, batch, seed=500):
    if kind == "hot":
        return torch.stack([hot_image(seed + i, tile, tile) for i in range(batch)])
    return torch.stack([synth_image(seed + i, 3, tile, tile) for i in range(batch)])


@functools.lru_cache(maxsize=None)
def references(net, tile, batch, kind):
    """(x, float64 oracle, fp16 emulation) of one case, computed once per module."""
    E.set_threads()
    with torch.inference_mode():
        sd, x = state_dict(net), make_input(kind, tile, batch)
        return x, E.oracle64(sd, x, SWIN[net][0]), E.emulated(sd, x, SWIN[net][0])


def check(y, y64, ye, net, label, origin=0, capsys=None):
    st = E.localised_stats(y, y64, ye, E.cells_for(SWIN[net][0], origin), E.B_OUT, E.TAU_OUT)
    line = f"errloc {label}: global {st['global']:.2f} worst {st['worst']:.2f} PSNR {psnr(y, y64):.2f} bands {E.summary(st)['bands']}"
    if capsys is not None:
        with capsys.disabled():
            print("\n" + line)
    return E.check_localised(y, y64, ye, E.cells_for(SWIN[net][0], origin), E.A_OUT, E.B_OUT, E.TAU_OUT, label=label)


@pytest.mark.parametrize("case", CASES, ids=_id)
def test_default_engine_window_by_window(hiplib, capsys, case):
    net, tile, batch, kind = case
    x, y64, ye = references(*case)
    y = make_model(net)(x.to("cuda:0")).cpu()
    assert y.shape == y64.shape and y.dtype == torch.float32
    check(y, y64, ye, net, _id(case), capsys=capsys)
    assert psnr(y, y64) >= 50.0


@pytest.mark.parametrize("env", SWITCHES, ids=lambda e: ",".join(f"{k}={v}" for k, v in e.items()))
@pytest.mark.parametrize("case", SWITCH_CASES, ids=_id)
def test_engine_switches_window_by_window(hiplib, capsys, monkeypatch, env, case):
    """NUNIF_BLOCK96=1 (one kernel per C = 96 block, incl. its fused image head) and NUNIF_ATT_WM=0 (pixel-major att map) under the
    same localised check; both are read when the engine is created."""
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    net = case[0]
    x, y64, ye = references(*case)
    y = make_model(net)(x.to("cuda:0")).cpu()
    check(y, y64, ye, net, _id(case) + "-" + ",".join(env), capsys=capsys)


def test_seed303_render_window_by_window(hiplib, capsys):
    """The 1x net, seed 303, 70 x 90 frame through tiled_render (tile 64, batch 4): shifted windows whose logits differ by more
    than 16 log2-units between lane groups (test_gpu_swin.py, the softmax stabiliser)."""
    from nunif_amd.nunif.utils.render import tiled_render
    from nunif_amd.waifu2x.models import swin_unet as M
    E.set_threads()
    sd = O.random_state_dict(303, 1)
    m = M.SwinUNet().eval()
    m.load_state_dict(sd, strict=True)
    img = synth_image(71, 3, 70, 90)
    y64 = OS.tiled_render(img.double(), lambda mb: E.oracle64(sd, mb, SWIN["1x"][0]), 1, 8, 4, 64, 4)
    ye = OS.tiled_render(img, lambda mb: E.emulated(sd, mb, SWIN["1x"][0]), 1, 8, 4, 64, 4)
    y = tiled_render(img.to("cuda:0"), m.to("cuda:0"), tile_size=64, batch_size=4).cpu()
    check(y[None], y64[None], ye[None], "1x", "1x-seed303-70x90", capsys=capsys)


# ---- debug taps: every intermediate, window by window and head by head ------------------------------------------------------
def _read_taps(eng):
    from test_gpu_swin import read_taps
    return read_taps(eng)


@pytest.mark.parametrize("net", ["2x", "4x", "4xl"])
def test_taps_window_by_window(hiplib, capsys, net):
    """With taps on (the engine's tap form: the pixel-major att map, no fused block / head), each tap against the float64 oracle's
    taps with the emulation's taps as yardstick, per 6 x 6 window of its own map and per group of 16 channels (one head)."""
    from nunif_amd import _hip
    E.set_threads()
    sd = state_dict(net)
    x = make_input("synth", 64, 2, seed=21)
    t64, temu = {}, {}
    E.oracle64(sd, x, SWIN[net][0], taps=t64)
    E.emulated(sd, x, SWIN[net][0], taps=temu)
    m = make_model(net)
    eng = m.engine()
    _hip.check(hiplib.nunif_hip_swin_unet_debug_taps(eng.handle, 1))
    try:
        m(x.to("cuda:0"))
        taps = _read_taps(eng)
    finally:
        _hip.check(hiplib.nunif_hip_swin_unet_debug_taps(eng.handle, 0))
    assert len(taps) >= 31 and set(taps) <= set(t64)
    worst, lines = {}, []
    for name, ref in t64.items():
        if name not in taps:
            continue
        got = taps[name].reshape(ref.shape)
        c = ref.shape[-1]
        tau = E.TAP_TAU_REL * float(ref.pow(2).mean().sqrt())
        y, y64, ye = E.nhwc(got), E.nhwc(ref), E.nhwc(temu[name])
        st = E.localised_stats(y, y64, ye, [(6, 0)], E.B_TAP, tau, group=16 if c % 16 == 0 else None)
        worst[name] = (st["global"], st["worst"])
        lines.append(f"{name:18s} global {st['global']:.2f} worst window/head {st['worst']:.2f}")
    with capsys.disabled():
        print(f"\nerrloc taps {net}:\n" + "\n".join(lines))
    for name, ref in t64.items():
        if name in taps:
            tau = E.TAP_TAU_REL * float(ref.pow(2).mean().sqrt())
            E.check_localised(E.nhwc(taps[name].reshape(ref.shape)), E.nhwc(ref), E.nhwc(temu[name]), [(6, 0)], E.A_TAP, E.B_TAP,
                              tau, group=16 if ref.shape[-1] % 16 == 0 else None, label=f"{net} tap {name}")


# ---- size-selected paths ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("net", ["8x", "4x"])
def test_image_head_on_the_resident_weight_gemm(hiplib, capsys, monkeypatch, net):
    """Tile 208 x batch 1 = 36 864 level-1 tokens (>= the 32 768 the resident-weight GEMM needs): with NUNIF_GEMM_BIG_M lowered
    (read per launch) the K = 192 image head (8x: to_image_pre in mode 0 and to_image in mode 2 with s = 8, the 16-byte store
    branch; 4x: to_image, s = 4) runs on gemm_res_kernel.  Bit-equal to the ring form, and window by window against the oracle."""
    monkeypatch.delenv("NUNIF_GEMM_BIG_M", raising=False)
    x, y64, ye = references(net, 208, 1, "synth")
    m = make_model(net)
    ring = m(x.to("cuda:0")).cpu()
    monkeypatch.setenv("NUNIF_GEMM_BIG_M", "32768")
    res = m(x.to("cuda:0")).cpu()
    monkeypatch.delenv("NUNIF_GEMM_BIG_M")
    assert torch.equal(res, ring), f"resident-weight head != ring head: max {float((res - ring).abs().max()):.3e}"
    check(res, y64, ye, net, f"{net}-208-1-resident-head", capsys=capsys)


def test_window_major_attention_map_past_2gib(hiplib):
    """2x net, 200 tiles of 256 in one forward: 200 x 1600 level-1 windows x 6 912 bytes = 2.2 GB of window-major att map, so the
    byte offsets of the windows of tile 195 on cross 2^31 (the kernel adds them in 32 bits: unsigned below 4 GB).  Tiles before,
    across and after that offset and the last tile are bit-equal to the same tiles run at batch 8.  Memory: about 10 GB."""
    import time
    t0 = time.time()
    m = make_model("2x")
    base = make_input("synth", 256, 8, seed=900)
    idx = torch.arange(200) % 8
    x = base[idx].to("cuda:0")
    per_tile = 1600 * 6 * 36 * 16 * 2
    cross = (1 << 31) // per_tile                              # the tile whose windows straddle 2^31 bytes
    assert cross == 194
    pick = [0, 100, cross - 1, cross, cross + 1, cross + 2, 198, 199]
    y = m(x)
    ysel = y[pick].cpu()
    del y
    torch.cuda.synchronize()
    ref = m(x[pick]).cpu()
    for j, t in enumerate(pick):
        assert torch.equal(ysel[j], ref[j]), f"tile {t} of the 200-tile forward != the same tile at batch 8"
    assert time.time() - t0 < 600
