"""CPU: ``tests/errloc.py`` against injected defects, with the fp16-autocast emulation standing in for an engine.

The clean emulation passes the localised check; a defect confined to one window, one shifted window, one edge row of tokens, one
output channel of one window or one image of a batch is caught at a size where the whole-image PSNR is still >= 50 dB.  The
detection table printed by ``test_detection_table`` lists the smallest defect each criterion catches.
"""
import functools

import pytest
import torch

import errloc as E
from conftest import psnr, synth_image
from oracle import swin_unet as O

NAMES = {1: "waifu2x.swin_unet_1x", 2: "waifu2x.swin_unet_2x", 4: "waifu2x.swin_unet_4x"}
PSNR_MIN = 50.0


@functools.lru_cache(maxsize=None)
def _case(sf, tile, batch, seed):
    E.set_threads()
    with torch.inference_mode():
        sd = O.random_state_dict(100 + sf, sf)
        x = torch.stack([synth_image(seed + i, 3, tile, tile) for i in range(batch)])
        return sd, x, E.oracle64(sd, x, NAMES[sf]), E.emulated(sd, x, NAMES[sf])


def _check(y, y64, ye, sf):
    return E.check_localised(y, y64, ye, E.cells_for(NAMES[sf]), E.A_OUT, E.B_OUT, E.TAU_OUT, label=f"{sf}x")


def _caught(y, y64, ye, sf):
    try:
        _check(y, y64, ye, sf)
        return False
    except AssertionError:
        return True


# seeds x {1x, 2x, 4x} x tiles {64, 112, 256}; one seed at tile 256 keeps the CPU cost down
CLEAN_CASES = [(seed, sf, tile, batch) for sf in (1, 2, 4) for tile, batch, seeds in ((64, 3, (11, 12)), (112, 2, (11, 12)), (256, 1, (11,)))
               for seed in seeds]


@pytest.mark.parametrize("seed,sf,tile,batch", CLEAN_CASES)
def test_clean_emulation_passes(seed, sf, tile, batch):
    sd, x, y64, ye = _case(sf, tile, batch, seed)
    st = _check(ye, y64, ye, sf)
    assert st["worst"] <= 1.0 and psnr(ye, y64) >= PSNR_MIN
    # a second fp16 evaluation order: parameters left in fp32 (every op result still rounded), another noise pattern
    with E.fp16_autocast_emulation():
        y2 = E._forward(sd, x, NAMES[sf])
    _check(y2, y64, ye, sf)


def _defects(sf, h, w, b):
    """name -> (image, channel slice, row slice, col slice) of an additive defect on the output."""
    c1 = 6 * sf                                  # one level-1 window in output pixels
    ny, nx = h // c1, w // c1
    win = lambda ry, rx: (slice(ry * c1, (ry + 1) * c1), slice(rx * c1, (rx + 1) * c1))   # noqa: E731
    d = {
        "window top-left": (0, slice(None)) + win(0, 0),
        "window top-right": (0, slice(None)) + win(0, nx - 1),
        "window bottom-left": (b - 1, slice(None)) + win(ny - 1, 0),
        "window bottom-right": (b - 1, slice(None)) + win(ny - 1, nx - 1),
        "window centre": (0, slice(None)) + win(ny // 2, nx // 2),
        "shifted window": (0, slice(None), slice(c1 // 2 + c1, c1 // 2 + 2 * c1), slice(c1 // 2 + c1, c1 // 2 + 2 * c1)),
        "bottom token row": (b - 1, slice(None), slice(h - sf, h), slice(None)),
        "one channel, one window": (0, slice(1, 2)) + win(ny // 2, 1),
    }
    if b > 1:
        d["one image of the batch"] = (b - 1, slice(None), slice(None), slice(None))
    return d


def _inject(ye, where, delta):
    y = ye.clone()
    bi, cs, rs, xs = where
    y[bi, cs, rs, xs] += delta
    return y


DELTAS = [1e-3 * 1.25 ** k for k in range(40)]          # 1e-3 .. 6e-0


def _smallest(pred):
    return next((d for d in DELTAS if pred(d)), float("inf"))


# (sf, tile, batch): the bench tile first; tile 64 with a batch of 5 for the one-image defect
TABLE_CASES = [(2, 256, 1), (4, 256, 1), (2, 64, 5), (1, 112, 2)]


@pytest.mark.parametrize("sf,tile,batch", TABLE_CASES)
def test_injected_defects_are_caught_where_psnr_passes(sf, tile, batch):
    """At the smallest size the localised check catches, each defect still reads >= 50 dB."""
    _, _, y64, ye = _case(sf, tile, batch, 31)
    for name, where in _defects(sf, ye.shape[2], ye.shape[3], batch).items():
        d = _smallest(lambda d: _caught(_inject(ye, where, d), y64, ye, sf))
        assert d < 1.0, (name, "never caught")
        y = _inject(ye, where, d)
        assert psnr(y, y64) >= PSNR_MIN, (sf, tile, name, d, psnr(y, y64))
        # and the failure names the defect's image
        with pytest.raises(AssertionError, match=f"image {where[0]} "):
            _check(y, y64, ye, sf)


def test_detection_table(capsys):
    """Smallest defect caught by the localised check vs by PSNR >= 50 dB.  At the bench's tile (2x, 256) a level-1 window is
    caught about an order of magnitude below what PSNR catches."""
    rows = []
    ratios = {}
    for sf, tile, batch in TABLE_CASES:
        _, _, y64, ye = _case(sf, tile, batch, 31)
        for name, where in _defects(sf, ye.shape[2], ye.shape[3], batch).items():
            dl = _smallest(lambda d: _caught(_inject(ye, where, d), y64, ye, sf))
            dp = _smallest(lambda d: psnr(_inject(ye, where, d), y64) < PSNR_MIN)
            ratios[(sf, tile, name)] = dp / dl
            rows.append(f"{sf}x tile {tile:3d} batch {batch}  {name:24s} localised {dl:.2e}   PSNR {dp:.2e}   x{dp / dl:6.1f}")
    with capsys.disabled():
        print("\nsmallest additive defect caught (output units, [0,1] image)\n" + "\n".join(rows))
    for name in ("window top-left", "window centre", "window bottom-right", "shifted window"):
        assert ratios[(2, 256, name)] >= 8.0, (name, ratios[(2, 256, name)])
    assert all(r > 1.0 for r in ratios.values()), ratios


def test_region_max_partitions():
    """The partitions: aligned and offset blocks, partial border blocks, per-group maxima, and the reported location."""
    e = torch.zeros(2, 32, 20, 20)
    e[1, 17, 13, 2] = -3.0
    r = E.region_max(e, 6, 0)
    assert r.shape == (2, 1, 4, 4) and r[1, 0, 2, 0] == 3.0 and r.sum() == 3.0
    r = E.region_max(e, 6, 3)                       # blocks [0,3) [3,9) [9,15) [15,20)
    assert r.shape == (2, 1, 4, 4) and r[1, 0, 2, 0] == 3.0
    r = E.region_max(e, 6, 3, group=16)
    assert r.shape == (2, 2, 4, 4) and r[1, 1, 2, 0] == 3.0 and r[1, 0].sum() == 0
    base = torch.full((2, 32, 20, 20), 1e-3)
    st = E.localised_stats(base + e.abs() * 0, base * 0, base, [(6, 0)], 4.0, 0.0, group=16)
    assert st["worst"] == pytest.approx(1.0)
    y = base.clone()
    y[1, 17, 13, 2] += 1.0
    with pytest.raises(AssertionError) as ex:
        E.check_localised(y, base * 0, base, [(6, 0)], 1e9, 4.0, 0.0, group=16, label="t")
    assert "image 1" in str(ex.value) and "channel 17" in str(ex.value) and "left" in str(ex.value)
