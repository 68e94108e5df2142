"""CPU: ``tests/errloc.py`` on the CUNet family, with the fp16-autocast emulation standing in for the engine.

The counterpart of ``test_errloc.py``.  The clean emulation and a second legitimate fp16 evaluation order (parameters left in fp32)
pass the localised check for CUNet / UpCUNet at tiles 64 / 68 / 100 / 256 and for the conv stacks; the oracle with taps computes
what the oracle without taps computes; and a defect confined to the places where the cunet kernels go wrong — one 8 x 32 conv patch
of one channel, one 16 x 16 head tile, the last (partial) patch row / column, one image of a batch, one 16-channel n-tile of one
patch of a tap — is caught at <= 4e-3 while the whole-tensor PSNR still reads >= 50 dB.
"""
import functools

import pytest
import torch

import errloc as E
from conftest import hot_image, psnr, synth_image
from oracle import cunet as OC

NAMES = {"cunet": "waifu2x.cunet", "upcunet": "waifu2x.upcunet", "vgg_7": "waifu2x.vgg_7", "upconv_7": "waifu2x.upconv_7"}
SEED = {"cunet": 201, "upcunet": 203, "vgg_7": 601, "upconv_7": 602}        # the seeds of test_cunet.py / test_convstack.py
PSNR_MIN = 50.0
CAUGHT_AT = 4e-3                 # output defects: caught at 2e-3 and missed at 1e-3 when this was written; one step of margin


def state_dict(net, regime="benign"):
    if net in ("vgg_7", "upconv_7"):
        return OC.conv_stack_state_dict(SEED[net], net)
    return OC.random_state_dict(SEED[net], up=net == "upcunet", regime=regime)


@functools.lru_cache(maxsize=None)
def _case(net, tile, batch, kind="synth", no_clip=False, regime="benign"):
    E.set_threads()
    with torch.inference_mode():
        sd = state_dict(net, regime)
        img = (lambda i: hot_image(40 + i, tile, tile)) if kind == "hot" else (lambda i: synth_image(40 + i, 3, tile, tile))
        x = torch.stack([img(i) for i in range(batch)])
        return sd, x, E.oracle64(sd, x, NAMES[net], no_clip=no_clip), E.emulated(sd, x, NAMES[net], no_clip=no_clip)


def _check(y, y64, ye, net):
    return E.check_localised(y, y64, ye, E.cells_for(NAMES[net]), E.A_OUT, E.B_OUT, E.TAU_OUT, label=net)


def _caught(y, y64, ye, net):
    try:
        _check(y, y64, ye, net)
        return False
    except AssertionError:
        return True


CLEAN_CASES = [(net, tile, batch, kind, no_clip, regime)
               for net in ("cunet", "upcunet")
               for tile, batch, kind, no_clip, regime in ((64, 3, "synth", False, "benign"), (68, 2, "hot", False, "benign"),
                                                          (100, 2, "synth", True, "benign"), (256, 1, "synth", False, "benign"),
                                                          (64, 2, "hot", False, "hot"), (100, 1, "synth", False, "hot"))]
CLEAN_CASES += [(net, tile, 2, kind, False, "benign") for net in ("vgg_7", "upconv_7") for tile, kind in ((64, "synth"), (100, "hot"))]


@pytest.mark.parametrize("net,tile,batch,kind,no_clip,regime", CLEAN_CASES)
def test_clean_emulation_passes(net, tile, batch, kind, no_clip, regime):
    sd, x, y64, ye = _case(net, tile, batch, kind, no_clip, regime)
    st = _check(ye, y64, ye, net)
    assert st["worst"] <= 1.0 and psnr(ye, y64) >= PSNR_MIN
    # a second fp16 evaluation order: parameters left in fp32 (every op result still rounded), another noise pattern
    with E.fp16_autocast_emulation():
        y2 = E._forward(sd, x, NAMES[net], no_clip=no_clip)
    _check(y2, y64, ye, net)


@pytest.mark.parametrize("net", ["cunet", "upcunet", "vgg_7", "upconv_7"])
def test_oracle_with_taps_computes_what_the_oracle_without_taps_does(net):
    sd = state_dict(net)
    x = torch.stack([synth_image(7, 3, 64, 64), hot_image(8, 64, 64)])
    fwd = (lambda **kw: OC.conv_stack_forward(sd, x, **kw)) if net in ("vgg_7", "upconv_7") else (lambda **kw: OC.model_forward(sd, x, **kw))
    taps = {}
    assert torch.equal(fwd(taps=taps), fwd())
    t64, temu = {}, {}
    assert torch.equal(E.oracle64(sd, x, NAMES[net], taps=t64), E.oracle64(sd, x, NAMES[net]))
    assert torch.equal(E.emulated(sd, x, NAMES[net], taps=temu), E.emulated(sd, x, NAMES[net]))
    assert set(taps) == set(t64) == set(temu)
    if net in ("vgg_7", "upconv_7"):
        assert sorted(taps) == sorted(f"net.{2 * i}" for i in range(6))
        return
    assert len(taps) == 29 and {"unet1.x1", "unet1.down", "unet1.conv2.0", "unet1.conv2", "unet1.se2.scale", "unet1.up_add",
                                "unet1.x3", "z1", "unet2.x2", "unet2.up3_add", "unet2.up4_add", "unet2.x5"} <= set(taps)
    # the recorded maps are the ones the forward used: NHWC feature maps, the SE-scaled map = the pre-SE map times the scale
    # vector, z1 clamped
    z1_side = 48 if net == "cunet" else 96
    assert taps["unet1.x1"].shape == (2, 60, 60, 64) and taps["z1"].shape == (2, 3, z1_side, z1_side)
    assert taps["z1"].shape[1] == 3 and float(taps["z1"].min()) >= 0.0 and float(taps["z1"].max()) <= 1.0
    assert torch.equal(taps["unet1.x2"], taps["unet1.conv2"] * taps["unet1.se2.scale"][:, None, None, :])
    assert torch.equal(taps["unet2.x4"], taps["unet2.conv4"] * taps["unet2.se4.scale"][:, None, None, :])
    assert taps["unet1.up_add"].shape == (2, 52, 52, 64) and taps["unet1.se2.scale"].shape == (2, 64)


def test_cells():
    assert E.cells_for("waifu2x.cunet") == [(8, 0), (16, 0), (32, 0), (64, 0)] == E.cells_for("waifu2x.vgg_7")
    assert E.cells_for("waifu2x.upcunet") == [(16, 0), (32, 0), (64, 0), (128, 0)] == E.cells_for("waifu2x.upconv_7")
    assert E.cells_for("waifu2x.cunet", origin=28) == [(8, 4), (16, 4), (32, 4), (64, 36)]
    assert E.cells_for("waifu2x.swin_unet_2x") == [(12, 0), (24, 0), (48, 0)]            # the swin form is as it was


# ---- injected defects ----------------------------------------------------------------------------------------------------------
def _defects(net, h, w, b):
    """name -> (image, channel slice, row slice, col slice) of an additive defect on the output: the places one workgroup, one
    head tile or one image of the cunet kernels writes (8 x 32 conv patches, 16 x 16 head tiles; x 2 behind the 4 x 4 s2 deconv)."""
    s = E.CUNET_SCALE[NAMES[net]]
    ph, pw, ht = 8 * s, 32 * s, 16 * s
    py, px = (h // ph) // 2, (w // pw) // 2
    d = {
        "8x32 patch, one channel": (0, slice(1, 2), slice(py * ph, (py + 1) * ph), slice(px * pw, (px + 1) * pw)),
        "8x32 patch top-left, one channel": (b - 1, slice(2, 3), slice(0, ph), slice(0, pw)),
        "16x16 head tile": (0, slice(None), slice((h // ht // 2) * ht, (h // ht // 2 + 1) * ht), slice((w // ht // 2) * ht, (w // ht // 2 + 1) * ht)),
        "last patch row": (b - 1, slice(None), slice((h - 1) // ph * ph, h), slice(None)),
        "last patch column": (0, slice(None), slice(None), slice((w - 1) // pw * pw, w)),
    }
    if b > 1:
        d["one image of the batch"] = (b - 1, slice(None), slice(None), slice(None))
    return d


def _inject(ye, where, delta):
    y = ye.clone()
    bi, cs, rs, xs = where
    y[bi, cs, rs, xs] += delta
    return y


DELTAS = [1e-3 * 2 ** k for k in range(11)]          # 1e-3 .. 1.0


def _smallest(pred):
    return next((d for d in DELTAS if pred(d)), float("inf"))


# (net, tile, batch, input): the bench tile first; batches for the one-image defect; a T % 8 != 0 tile
TABLE_CASES = [("cunet", 256, 1, "synth"), ("upcunet", 256, 1, "synth"), ("cunet", 100, 3, "hot"), ("upcunet", 68, 2, "synth"),
               ("cunet", 64, 3, "synth"), ("upconv_7", 100, 2, "synth")]


def test_detection_table(capsys):
    """Smallest additive defect the localised check catches against the smallest one PSNR >= 50 dB catches.  Every defect is caught
    at <= 4e-3, names its image, and still reads >= 50 dB there."""
    rows, fails = [], []
    for net, tile, batch, kind in TABLE_CASES:
        _, _, y64, ye = _case(net, tile, batch, kind)
        for name, where in _defects(net, ye.shape[2], ye.shape[3], batch).items():
            dl = _smallest(lambda d: _caught(_inject(ye, where, d), y64, ye, net))
            dp = _smallest(lambda d: psnr(_inject(ye, where, d), y64) < PSNR_MIN)
            rows.append(f"{net:8s} tile {tile:3d} batch {batch} {kind:5s} {name:34s} localised {dl:.0e}   PSNR {dp:.0e}")
            y = _inject(ye, where, dl) if dl < 1.0 else ye
            if not (dl <= CAUGHT_AT and dp > dl and psnr(y, y64) >= PSNR_MIN):
                fails.append(rows[-1])
                continue
            with pytest.raises(AssertionError, match=f"image {where[0]} "):
                _check(y, y64, ye, net)
    with capsys.disabled():
        print("\nsmallest additive defect caught (output units, [0,1] image)\n" + "\n".join(rows))
    assert not fails, "\n".join(fails)


def test_psnr_cannot_see_a_patch_at_the_bench_tile():
    """One 8 x 32 patch of one channel off by 8e-3 at tile 256 still reads >= 59 dB (psnr() saturates at 60)."""
    _, _, y64, ye = _case("cunet", 256, 1, "synth")
    where = _defects("cunet", 200, 200, 1)["8x32 patch, one channel"]
    y = _inject(ye, where, 8e-3)
    assert psnr(y, y64) >= 59.0 and _caught(y, y64, ye, "cunet")


@pytest.mark.parametrize("net", ["cunet", "upcunet"])
def test_tap_defect_in_one_n_tile_of_one_patch_is_caught(net, capsys):
    """A tap (NHWC fp16 map of a middle layer) with ONE 16-channel n-tile of ONE 8 x 32 patch off by d, checked as the GPU test
    checks the engine's taps (cells 8 and 32, groups of 16 channels, tau = TAP_TAU_REL x rms).  The check fires as soon as
    d - n > B_TAP n + tau, n = the largest emulation error of the tap: asserted at the first step above (B_TAP + 1) n + tau, and
    that step is a small fraction of the tap's own rms (the defect is far below anything that would move the output's PSNR)."""
    sd = state_dict(net)
    x = torch.stack([synth_image(40 + i, 3, 64, 64) for i in range(2)])
    t64, temu = {}, {}
    E.oracle64(sd, x, NAMES[net], taps=t64)
    E.emulated(sd, x, NAMES[net], taps=temu)
    rows = []
    for name in ("unet1.x1", "unet1.conv2.0", "unet1.up_add", "unet2.x2", "unet2.conv3.0", "unet2.x5"):
        ref, emu = t64[name], temu[name]
        rms = float(ref.pow(2).mean().sqrt())
        tau = E.TAP_TAU_REL * rms
        n = float((emu.double() - ref).abs().max())
        h, w, c = ref.shape[1:]
        g = (c // 16) - 1

        def caught(d):
            bad = emu.clone()
            bad[1, 0:8, max(0, w - 32):w, 16 * g:16 * g + 16] += d
            try:
                E.check_localised(E.nhwc(bad), E.nhwc(ref), E.nhwc(emu), [(8, 0), (32, 0)], E.A_TAP, E.B_TAP, tau, group=16, label=name)
                return False
            except AssertionError as e:
                assert "image 1 " in str(e)
                return True
        steps = [rms * 1e-3 * 2 ** k for k in range(14)]
        d = next(s for s in steps if caught(s))
        rows.append(f"{net} {name:14s} rms {rms:.3f} noise {n:.2e} caught at {d:.2e} ({d / rms:.1%} of rms)")
        bound = (E.B_TAP + 1.0) * n + tau
        assert d <= 2.0 * bound, rows[-1]                  # the first step of the doubling ladder above the bound
        assert d <= 0.05 * rms, rows[-1]
        assert not caught(0.0)
    with capsys.disabled():
        print("\n" + "\n".join(rows))


def test_one_channel_of_an_se_scale_vector_is_a_region_of_its_own():
    """The SE scale taps ([B, C] fp32) are compared per image and channel (group=1): one channel of one image off by d is judged
    against that channel's own emulation error, so it is caught at the first step above (B_TAP + 1) n + tau, n = that entry's
    error; with the 16 channels of an n-tile pooled it would hide behind the largest error among its neighbours."""
    sd = state_dict("cunet")
    x = torch.stack([synth_image(40 + i, 3, 64, 64) for i in range(2)])
    t64, temu = {}, {}
    E.oracle64(sd, x, NAMES["cunet"], taps=t64)
    E.emulated(sd, x, NAMES["cunet"], taps=temu)
    for name in ("unet1.se2.scale", "unet2.se2.scale", "unet2.se3.scale", "unet2.se4.scale"):
        ref, emu = t64[name], temu[name]
        tau = E.TAP_TAU_REL * float(ref.pow(2).mean().sqrt())
        noise = (emu.double() - ref).abs()
        ch = int(noise[1].argmin())                            # the quietest channel: its neighbours are louder
        d = (E.B_TAP + 1.0) * float(noise[1, ch]) + 1.5 * tau
        bad = emu.clone()
        bad[1, ch] += d
        as_map = lambda t: t[:, :, None, None]                 # noqa: E731
        E.check_localised(as_map(emu), as_map(ref), as_map(emu), [(1, 0)], E.A_TAP, E.B_TAP, tau, group=1, label=name)
        with pytest.raises(AssertionError, match=f"image 1 .*channel {ch}:"):
            E.check_localised(as_map(bad), as_map(ref), as_map(emu), [(1, 0)], 1e9, E.B_TAP, tau, group=1, label=name)
