"""The cunet engine (CUNet / UpCUNet / vgg_7 / upconv_7) held patch by patch and layer by layer to a float64 oracle.

``tests/errloc.py``: per image, max|y - y64| <= A * max|emu - y64| and, in every cell of 8 / 16 / 32 / 64 level-1 pixels (x 2 for the
2x nets; aligned and half-cell-shifted partitions), region_max(y - y64) <= B * region_max(emu - y64) + tau, where emu is the
reference's own fp16-autocast arithmetic (``oracle/fp16_emulation.py``).  The kernels of this engine go wrong per 8 x 32 output patch
of a conv workgroup, per 16 x 16 head tile, per 16-channel MFMA n-tile, per K half / quarter and per image (SE pooling, the scale
table in LDS); a whole 8 x 32 patch of one channel off by 8e-3 still reads 59 dB at tile 256, this check catches 4e-3
(``tests/test_errloc_cunet.py``).  The constants are the ones accepted for swin (A_OUT 2.5, B_OUT 3.75, A_TAP 3.5, B_TAP 5.5).

Cases: (a) the default engine on every net, tiles 64 / 68 (level-1 map 64 = 2 x 32) / 100 / 140 (T % 8 != 0) / 256, batches 1 / 2 / 3 /
5 / 7 (tile 64 on both sides of the 24-patch LDS <-> DMA conv switch), ``synth_image`` and ``hot_image``, benign and ``regime="hot"``
weights; (b) every engine switch under the same check, the two that are read once per process in a child process each; (c) every
debug tap (``nunif_hip_cunet_debug_taps``: the launches are the ones of the default engine, the output is bit-equal) per cell of 8 and
32 and per 16 channels, ``z1`` with the output constants, the SE scale vectors per image and channel; (d) a result does not depend
on the tile minibatch: 1 tile against the same tile among 3, 130 tiles (past the 128 images of the up kernel's scale table) against
batches of 8; (e) a 300-tile forward whose level-1 map passes 2^31 bytes.

Measured on an MI355X (ratio = engine error / emulation error; worst over the cases):
    outputs                                global max   worst region    case of the worst region
    CUNet (incl. no_clip, hot weights)     1.06         1.17            tile 140, batch 3, hot (global: tile 64, batch 7)
    UpCUNet (incl. no_clip, hot weights)   0.58         0.57            tile 68, batch 7, synth
    vgg_7 / upconv_7                       0.91         1.25            upconv_7, tile 64, batch 7, hot
    the nine per-launch switches           0.77         0.95            upconv_7, tile 100 (CUNet / UpCUNet 0.66 / 0.86)
    SLICED=0 / CONV3_DMA_MIN (children)    0.66         0.86            CUNet, tile 256 (DMA_MIN 4 / 1000000 bit-equal to the default)
    130 tiles of 64 / 300 tiles of 256     1.06         1.10            CUNet, rows 122..129 of the 130 (bit-equal to batch 8)
    taps CUNet                             1.18         2.65            unet2.conv3 (5 x 5 map), tile 64, STEM=0 + SE_FUSE=0; unet2.x5 global
    taps UpCUNet                           1.13         1.86            unet2.up3_add, tile 100, batch 3
    taps vgg_7 / upconv_7                  1.02         1.48            upconv_7 net.10
    z1                                     0.93         1.17            CUNet tile 64
    SE scale vectors, per image + channel  not measured yet in this form (per 16 channels: 0.25 / 0.17, unet1.se2.scale)
Every output case reads 59.84-59.99 dB, so PSNR >= 50 says nothing here that the region bound does not.  A scratch build whose
conv3_dma_kernel scales the bias of one 16-channel n-tile by 1.25 in the last patch column (defects of ~5e-3 in one n-tile of the
taps) fails 19 of the 27 output cases (tile 64 at small batches runs conv3_lds_kernel instead) and all 8 tap cases, while every
PSNR stays >= 53.4 dB; the same mutation at 1.01 (2e-4, below the reference's own fp16 noise) is seen by the bit-equality tests of
``test_cunet.py`` only: defects of that size in one n-tile are outside what this check can tell from fp16 rounding.
"""
import ctypes
import functools
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from conftest import hot_image, psnr, synth_image  # first: puts the repository root on sys.path (the child process runs this file)
import errloc as E
from oracle import cunet as OC

pytestmark = pytest.mark.gpu

NAMES = {"cunet": "waifu2x.cunet", "upcunet": "waifu2x.upcunet", "vgg_7": "waifu2x.vgg_7", "upconv_7": "waifu2x.upconv_7"}
# the seeds of test_cunet.py / test_convstack.py, one per tile so that every seed runs
SEEDS = {"cunet": {64: 201, 68: 202, 100: 205, 140: 201, 256: 202}, "upcunet": {64: 203, 68: 205, 100: 203, 140: 205, 256: 203},
         "vgg_7": {64: 601, 100: 601}, "upconv_7": {64: 602, 100: 602}}

# (net, tile, batch, input, options): options "" | "no_clip" | "hot" (regime="hot" weights)
CASES = [
    ("cunet", 64, 1, "synth", ""), ("cunet", 64, 2, "hot", ""), ("cunet", 64, 7, "synth", ""), ("cunet", 68, 3, "synth", ""),
    ("cunet", 68, 5, "hot", ""), ("cunet", 100, 5, "synth", ""), ("cunet", 100, 2, "hot", "hot"), ("cunet", 140, 3, "hot", ""),
    ("cunet", 140, 2, "synth", "hot"), ("cunet", 256, 1, "synth", ""), ("cunet", 256, 2, "hot", ""),
    ("cunet", 64, 3, "hot", "no_clip"), ("cunet", 100, 1, "synth", "no_clip"), ("cunet", 140, 1, "synth", "no_clip"),
    ("upcunet", 64, 1, "synth", ""), ("upcunet", 64, 5, "hot", ""), ("upcunet", 68, 7, "synth", ""), ("upcunet", 100, 3, "hot", ""),
    ("upcunet", 140, 2, "synth", ""), ("upcunet", 256, 1, "synth", ""), ("upcunet", 64, 2, "synth", "hot"),
    ("upcunet", 68, 2, "hot", "no_clip"), ("upcunet", 100, 1, "synth", "no_clip"),
    ("vgg_7", 64, 3, "synth", ""), ("vgg_7", 100, 5, "hot", ""), ("upconv_7", 64, 7, "hot", ""), ("upconv_7", 100, 2, "synth", ""),
]
SWITCH_CASES = [("cunet", 68, 3, "synth", ""), ("upcunet", 100, 3, "hot", ""), ("cunet", 256, 1, "synth", ""), ("upconv_7", 100, 2, "synth", "")]
SWITCHES = [{"NUNIF_CONV3_DMA": "0"}, {"NUNIF_CONV3_DMA_KSPLIT": "0"}, {"NUNIF_CUNET_STEM": "0"}, {"NUNIF_CUNET_DOWN_GEMM": "0"},
            {"NUNIF_CUNET_HEAD": "0"}, {"NUNIF_CUNET_HEAD_TW": "32"}, {"NUNIF_CUNET_UP": "0"}, {"NUNIF_CUNET_SE_FUSE": "0"},
            {"NUNIF_CONV_RES": "0"}]
# read once per process (function-local statics of the library): one fresh child process each.  NUNIF_CONV3_DMA_MIN moves the
# LDS <-> DMA conv switch (default 24 patches) below and above every launch of the cases
CHILD_SWITCHES = [{"NUNIF_CUNET_SLICED": "0"}, {"NUNIF_CONV3_DMA_MIN": "4"}, {"NUNIF_CONV3_DMA_MIN": "1000000"}]
CHILD_CASES = [("cunet", 68, 3, "synth", ""), ("upcunet", 100, 3, "hot", ""), ("cunet", 256, 1, "synth", "")]
CHILD_TIMEOUT = 180
CRASH_STATUS = (134, 139, 124, 137, -6, -11, -9, -15)


def _id(c):
    return "-".join(str(v) for v in c if v != "")


def _env_id(e):
    return ",".join(f"{k}={v}" for k, v in e.items())


def state_dict(net, tile, options=""):
    seed = SEEDS[net][tile]
    if net in ("vgg_7", "upconv_7"):
        return OC.conv_stack_state_dict(seed, net)
    return OC.random_state_dict(seed, up=net == "upcunet", regime="hot" if options == "hot" else "benign")


def make_model(net, tile, options=""):
    from nunif_amd.nunif.models import create_model
    import nunif_amd.waifu2x.utils  # noqa: F401  (registers every waifu2x model)
    kwargs = {"no_clip": True} if options == "no_clip" else {}
    m = create_model(NAMES[net], **kwargs).eval()
    m.load_state_dict(state_dict(net, tile, options), strict=True)
    return m.to("cuda:0")


def make_input(kind, tile, batch, seed=700):
    if kind == "hot":
        return torch.stack([hot_image(seed + i, tile, tile) for i in range(batch)])
    return torch.stack([synth_image(seed + i, 3, tile, tile) for i in range(batch)])


@functools.lru_cache(maxsize=None)
def references(net, tile, batch, kind, options=""):
    """(x, float64 oracle, fp16 emulation) of one case, computed once per module."""
    E.set_threads()
    with torch.inference_mode():
        sd, x = state_dict(net, tile, options), make_input(kind, tile, batch)
        nc = options == "no_clip"
        return x, E.oracle64(sd, x, NAMES[net], no_clip=nc), E.emulated(sd, x, NAMES[net], no_clip=nc)


def check(y, y64, ye, net, label, capsys=None):
    """Print the figures of one output, then assert the bounds on them."""
    assert y.shape == y64.shape == ye.shape, (label, y.shape, y64.shape, ye.shape)
    st = E.localised_stats(y, y64, ye, E.cells_for(NAMES[net]), E.B_OUT, E.TAU_OUT)
    line = f"errloc {label}: global {st['global']:.2f} worst {st['worst']:.2f} PSNR {psnr(y, y64):.2f} bands {E.summary(st)['bands']}"
    if capsys is not None:
        with capsys.disabled():
            print("\n" + line)
    else:
        print(line)
    return E.assert_localised(st, E.A_OUT, E.B_OUT, E.TAU_OUT, label=label)


# ---- (a) the default engine ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", CASES, ids=_id)
def test_default_engine_patch_by_patch(hiplib, capsys, case):
    net, tile, batch, kind, options = case
    x, y64, ye = references(*case)
    y = make_model(net, tile, options)(x.to("cuda:0")).cpu()
    assert y.shape == y64.shape and y.dtype == torch.float32
    check(y, y64, ye, net, _id(case), capsys=capsys)
    assert psnr(y, y64) >= 50.0


# ---- (b) every switch ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("env", SWITCHES, ids=_env_id)
@pytest.mark.parametrize("case", SWITCH_CASES, ids=_id)
def test_engine_switches_patch_by_patch(hiplib, capsys, monkeypatch, env, case):
    """The kernel variants behind the switches that are read per launch (conv3_lds / conv3_dma without K halves, the VALU first conv +
    separate 32 -> 64 conv, conv_kernel for the stride-2 convs, the conv form and the 32-wide form of the image head, gemm_kernel for
    the up step, a separate SE scale pass, the ring form of conv_kernel) under the same localised check."""
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    net, tile, batch, kind, options = case
    x, y64, ye = references(*case)
    y = make_model(net, tile, options)(x.to("cuda:0")).cpu()
    check(y, y64, ye, net, _id(case) + "-" + _env_id(env), capsys=capsys)
    assert psnr(y, y64) >= 50.0


def _child_main(out_path):
    """Child process of ``test_process_wide_switches_in_a_child_process``: the engine outputs of CHILD_CASES under the environment
    this process was started with, saved for the parent to check."""
    out = {}
    with torch.inference_mode():
        for case in CHILD_CASES:
            net, tile, batch, kind, options = case
            x = make_input(kind, tile, batch)
            out[_id(case)] = make_model(net, tile, options)(x.to("cuda:0")).cpu()
        torch.cuda.synchronize()
    torch.save(out, out_path)


def test_process_wide_switches_in_a_child_process(hiplib, capsys, tmp_path):
    """NUNIF_CUNET_SLICED=0 (the 128 / 256-input convs with more than 64 outputs as ONE launch instead of 64-channel slices) and
    NUNIF_CONV3_DMA_MIN (the patch count from which a conv takes conv3_dma_kernel) are read once per process: each value runs in a
    fresh child process with its own time limit.  A child that faults, aborts or times out fails the test at once and no further
    child is started.  Moving the LDS <-> DMA switch must not change a bit (same MFMA order over k)."""
    default = {}
    for case in CHILD_CASES:
        net, tile, batch, kind, options = case
        default[_id(case)] = make_model(net, tile, options)(references(*case)[0].to("cuda:0")).cpu()
    for env in CHILD_SWITCHES:
        out_path = str(tmp_path / (_env_id(env).replace("=", "_") + ".pt"))
        child_env = dict(os.environ)
        child_env.update(env)
        try:
            r = subprocess.run([sys.executable, "-s", os.path.abspath(__file__), out_path], env=child_env, capture_output=True,
                               text=True, timeout=CHILD_TIMEOUT)
        except subprocess.TimeoutExpired:
            pytest.fail(f"child {_env_id(env)} ran into its {CHILD_TIMEOUT} s time limit: no further child is started")
        if r.returncode != 0:
            kind = "crashed" if r.returncode in CRASH_STATUS else "failed"
            pytest.fail(f"child {_env_id(env)} {kind} with status {r.returncode}: no further child is started\n{r.stderr[-2000:]}")
        got = torch.load(out_path)
        for case in CHILD_CASES:
            net = case[0]
            x, y64, ye = references(*case)
            y = got[_id(case)]
            check(y, y64, ye, net, _id(case) + "-" + _env_id(env), capsys=capsys)
            assert psnr(y, y64) >= 50.0
            if "NUNIF_CONV3_DMA_MIN" in env:
                assert torch.equal(y, default[_id(case)]), (_env_id(env), _id(case), float((y - default[_id(case)]).abs().max()))


# ---- (c) debug taps -----------------------------------------------------------------------------------------------------------
def read_taps(engine):
    """{name: tensor} of the engine's taps: fp16 maps flat (as float32), ``z1`` and the ``*.scale`` vectors float32."""
    from nunif_amd import _hip
    lib = _hip.lib()
    taps = {}
    i = 0
    while True:
        name = ctypes.create_string_buffer(64)
        nbytes = ctypes.c_int64(0)
        rc = lib.nunif_hip_cunet_get_tap(engine.handle, i, name, 64, None, 0, ctypes.byref(nbytes))
        if rc == 1:
            break
        _hip.check(rc)
        key = name.value.decode()
        f32 = key == "z1" or key.endswith(".scale")
        buf = np.empty(nbytes.value // (4 if f32 else 2), dtype=np.float32 if f32 else np.float16)
        _hip.check(lib.nunif_hip_cunet_get_tap(engine.handle, i, name, 64, buf.ctypes.data_as(ctypes.c_void_p), nbytes.value,
                                               ctypes.byref(nbytes)))
        assert key not in taps, key
        taps[key] = torch.from_numpy(buf.astype(np.float32))
        i += 1
    return taps


def tapped_forward(hiplib, m, x):
    """(output without taps, output with taps, taps)"""
    from nunif_amd import _hip
    plain = m(x.to("cuda:0")).cpu()
    eng = m.engine()
    _hip.check(hiplib.nunif_hip_cunet_debug_taps(eng.handle, 1))
    try:
        m(x.to("cuda:0"))                                      # a forward with taps on starts from an empty store: no duplicates below
        y = m(x.to("cuda:0")).cpu()
        taps = read_taps(eng)
    finally:
        _hip.check(hiplib.nunif_hip_cunet_debug_taps(eng.handle, 0))
    assert hiplib.nunif_hip_cunet_get_tap(eng.handle, 0, None, 0, None, 0, ctypes.byref(ctypes.c_int64(0))) == 1   # released
    return plain, y, taps


def tap_stats(name, got, ref, emu, net):
    """(stats, A, B, tau) of one tap against the float64 oracle's, the emulation's tap as yardstick."""
    if name == "z1":                                           # planar fp32, an image: the output constants and cells
        return E.localised_stats(got.reshape(ref.shape), ref, emu, E.cells_for(NAMES[net]), E.B_OUT, E.TAU_OUT), E.A_OUT, E.B_OUT, E.TAU_OUT
    tau = E.TAP_TAU_REL * float(ref.pow(2).mean().sqrt())
    if name.endswith(".scale"):                                # [B, C] fp32: every image and every channel is a region of its own
        y, y64, ye = (t.reshape(ref.shape)[:, :, None, None] for t in (got, ref, emu))
        return E.localised_stats(y, y64, ye, [(1, 0)], E.B_TAP, tau, group=1), E.A_TAP, E.B_TAP, tau
    c = ref.shape[-1]                                          # NHWC fp16 map: per cell of 8 and 32, per 16-channel n-tile
    g = got.reshape(ref.shape[:-1] + (-1,))                    # (upconv_7's first map carries 16 zero channels of padding)
    assert c % 16 == 0 and g.shape[-1] >= c and not bool(g[..., c:].any()), (name, g.shape)
    return E.localised_stats(E.nhwc(g[..., :c]), E.nhwc(ref), E.nhwc(emu), [(8, 0), (32, 0)], E.B_TAP, tau, group=16), E.A_TAP, E.B_TAP, tau


TAP_CASES = [("cunet", 64, 2, {}, 24), ("cunet", 100, 3, {}, 24), ("upcunet", 64, 2, {}, 24), ("upcunet", 100, 3, {}, 24),
             # every map exists as a launch's output: the 32-channel maps of the stems and the SE-scaled maps
             ("cunet", 64, 2, {"NUNIF_CUNET_STEM": "0", "NUNIF_CUNET_SE_FUSE": "0"}, 29),
             ("upcunet", 64, 2, {"NUNIF_CUNET_STEM": "0"}, 26),
             ("vgg_7", 64, 2, {}, 6), ("upconv_7", 100, 3, {}, 6)]


@pytest.mark.parametrize("net,tile,batch,env,n_taps", TAP_CASES, ids=lambda v: _env_id(v) if isinstance(v, dict) else str(v))
def test_taps_layer_by_layer(hiplib, capsys, monkeypatch, net, tile, batch, env, n_taps):
    """Every map a launch of the engine writes, against the float64 oracle's map of the same name.  Taps do not change which kernels
    run: the output with taps on is the output with taps off, bit for bit."""
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    E.set_threads()
    sd = state_dict(net, tile)
    x = make_input("synth", tile, batch, seed=21)
    t64, temu = {}, {}
    y64 = E.oracle64(sd, x, NAMES[net], taps=t64)
    ye = E.emulated(sd, x, NAMES[net], taps=temu)
    plain, y, taps = tapped_forward(hiplib, make_model(net, tile), x)
    assert torch.equal(y, plain), f"taps changed the output: max {float((y - plain).abs().max()):.3e}"
    assert len(taps) == n_taps and set(taps) <= set(t64), (sorted(taps), sorted(set(taps) - set(t64)))
    label = f"{net}-{tile}-{batch}" + ("-" + _env_id(env) if env else "")
    stats = {name: tap_stats(name, taps[name], t64[name], temu[name], net) for name in t64 if name in taps}
    with capsys.disabled():
        print(f"\nerrloc taps {label}:\n" + "\n".join(f"{name:16s} global {st['global']:.2f} worst cell/n-tile {st['worst']:.2f}"
                                                       for name, (st, _, _, _) in stats.items()))
    for name, (st, A, B, tau) in stats.items():
        E.assert_localised(st, A, B, tau, label=f"{label} tap {name}")
    check(y, y64, ye, net, label + "-taps-on", capsys=capsys)


# ---- (d) a result does not depend on the tile minibatch ------------------------------------------------------------------------
@pytest.mark.parametrize("net", ["cunet", "upcunet", "vgg_7"])
def test_one_tile_equals_the_same_tile_in_a_batch_of_three(hiplib, net):
    """Tile 64: 2 x 2 = 4 patches per image at level 1 of unet1 ... 16 at the 60 x 60 map; a batch of 1 keeps every launch at or below
    the 24 patches up to which a conv takes conv3_lds_kernel, a batch of 3 moves the large maps to conv3_dma_kernel."""
    m = make_model(net, 64)
    x = make_input("synth", 64, 3, seed=31)
    y3 = m(x.to("cuda:0")).cpu()
    for i in range(3):
        y1 = m(x[i:i + 1].to("cuda:0")).cpu()
        assert torch.equal(y1[0], y3[i]), f"tile {i} alone != the same tile in a batch of 3: max {float((y1[0] - y3[i]).abs().max()):.3e}"


@pytest.mark.parametrize("net", ["cunet", "upcunet"])
def test_130_tiles_equal_the_same_tiles_at_batch_8(hiplib, capsys, net):
    """130 tiles of 64 in one forward: more images than the up kernel's SE scale table holds in LDS (128).  The up step runs the
    resident kernel over groups of at most 128 images (cunet.cpp run_up) instead of leaving the whole launch to gemm_kernel, whose
    sums round differently: every row equals the same image run at batch 8, and the rows past 128 meet the oracle bound."""
    x8, y64, ye = references(net, 64, 8, "synth")
    m = make_model(net, 64)
    ref = m(x8.to("cuda:0")).cpu()
    idx = torch.arange(130) % 8
    y = m(x8[idx].to("cuda:0")).cpu()
    bad = [i for i in range(130) if not torch.equal(y[i], ref[idx[i]])]
    assert not bad, f"rows {bad[:8]}... of the 130-tile forward != the same images at batch 8 ({len(bad)} rows)"
    last = torch.arange(122, 130)                                  # images 2 .. 7, 0, 1
    check(y[last], y64[idx[last]], ye[idx[last]], net, f"{net}-64-130 rows 122..129", capsys=capsys)


# ---- (e) one map past 2^31 bytes ----------------------------------------------------------------------------------------------
def test_level1_map_past_2gib(hiplib, capsys):
    """CUNet, 300 tiles of 256 in one forward (8 distinct images, indexed modulo 8): the level-1 map is 252 x 252 x 64 fp16 = 8.13 MB
    per tile, so byte 2^31 falls inside tile 264 (the 244- and 242-wide maps of unet1 and the 236-wide one of unet2 pass it too).
    conv3_* carry 64-bit offsets, cunet_up / the 64 -> 64 patch-down kernel 32-bit unsigned byte offsets behind a 4 GiB guard.  Tiles
    before, across and after that byte and the last tile equal the same images at batch 8 and meet the oracle bound.
    Memory: about 15 GB of workspace + 0.4 GB of input / output; skipped below 20 GB free.  One forward, run once."""
    free, _ = torch.cuda.mem_get_info()
    if free < 20 << 30:
        pytest.skip(f"needs 20 GB of free device memory, {free >> 30} GB free")
    per_tile = 252 * 252 * 64 * 2
    cross = (1 << 31) // per_tile
    assert cross == 264
    x8, y64, ye = references("cunet", 256, 8, "synth")
    m = make_model("cunet", 256)
    ref = m(x8.to("cuda:0")).cpu()
    idx = torch.arange(300) % 8
    pick = [0, 150, cross - 1, cross, cross + 1, 299]
    y = m(x8.to("cuda:0")[idx.to("cuda:0")])
    ysel = y[pick].cpu()
    del y
    torch.cuda.synchronize()
    for j, t in enumerate(pick):
        assert torch.equal(ysel[j], ref[idx[t]]), f"tile {t} of the 300-tile forward != the same image at batch 8: max {float((ysel[j] - ref[idx[t]]).abs().max()):.3e}"
    sel = idx[pick]
    check(ysel, y64[sel], ye[sel], "cunet", "cunet-256-300 tiles 0/150/263/264/265/299", capsys=capsys)


if __name__ == "__main__":
    _child_main(sys.argv[1])
