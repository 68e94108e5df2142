"""The producers of a swin_unet frame render that list — PatchDown2 and both PatchUps — write only the tokens something behind them in the
frame reads (NUNIF_SWIN_SKIP_PAD level 3), and down2's second tap row runs on the prefetching PatchDown kernel.  Whole
frames against level 0 bit for bit, stale data of an earlier frame or geometry on the same handle, any split into minibatches, and
one down2 launch pair against the generic GEMM's.  Synthetic weights, tiles 64 / 112 / 160 (token maps of 48 / 96 / 144)."""
import ctypes

import pytest
import torch

from conftest import synth_image
from oracle import swin_unet as O

pytestmark = pytest.mark.gpu

# (tile, frame height, frame width, scale): ragged last rows and columns; the 4x net's fast stages at tile 160
FRAMES = [(64, 100, 150, 2), (64, 136, 260, 2), (112, 200, 330, 2), (160, 200, 330, 2), (160, 200, 330, 4)]


def make_model(sf, seed=102):
    from nunif_amd.waifu2x.models import swin_unet as M
    cls = {2: M.SwinUNet2x, 4: M.SwinUNet4x}[sf]
    m = cls().eval()
    m.load_state_dict(O.random_state_dict(seed, sf), strict=True)
    return m.to("cuda:0")


@pytest.fixture(scope="module")
def models(hiplib):
    return {sf: make_model(sf) for sf in (2, 4)}


def _n_tiles(tile, h, w, sf):
    from nunif_amd import _hip
    g = _hip.tile_grid(h, w, sf, 8 * sf, tile, 4 * sf)
    return g.h_blocks * g.w_blocks


@pytest.fixture(scope="module")
def level0(models):
    """the level-0 render of every frame, on handles of their own (computed once, never modified)"""
    import os
    out = {}
    old = os.environ.get("NUNIF_SWIN_SKIP_PAD")
    os.environ["NUNIF_SWIN_SKIP_PAD"] = "0"
    try:
        fresh = {sf: make_model(sf) for sf in (2, 4)}
        for tile, h, w, sf in FRAMES:
            x = synth_image(7, 3, h, w).to("cuda:0")
            out[(tile, h, w, sf)] = fresh[sf].render_frame(x, tile_size=tile, batch_size=_n_tiles(tile, h, w, sf)).clone()
    finally:
        if old is None:
            del os.environ["NUNIF_SWIN_SKIP_PAD"]
        else:
            os.environ["NUNIF_SWIN_SKIP_PAD"] = old
    return out


@pytest.mark.parametrize("tile,h,w,sf", FRAMES)
def test_level3_changes_no_bit(models, level0, monkeypatch, tile, h, w, sf):
    m = models[sf]
    x = synth_image(7, 3, h, w).to("cuda:0")
    n = _n_tiles(tile, h, w, sf)
    want = level0[(tile, h, w, sf)]
    monkeypatch.setenv("NUNIF_SWIN_SKIP_PAD", "3")
    got = m.render_frame(x, tile_size=tile, batch_size=n).clone()
    assert got.shape == (3, h * sf, w * sf) and torch.isfinite(got).all()
    assert torch.equal(got, want), "a kept pixel depends on a token a producer left out"
    monkeypatch.delenv("NUNIF_SWIN_SKIP_PAD")                                 # unset: the default is level 3
    assert torch.equal(m.render_frame(x, tile_size=tile, batch_size=n), want)
    # any split of the frame into minibatches gives the same bits
    for bs in (1, 2):
        assert torch.equal(m.render_frame(x, tile_size=tile, batch_size=bs), want), bs


@pytest.mark.parametrize("tile,h,w,sf", FRAMES)
def test_the_producers_issue_the_listed_work(models, monkeypatch, tile, h, w, sf):
    """the launchers report the work actually issued: at level 3 the listed instances run, with fewer FLOPs than whole tiles"""
    from nunif_amd import _hip
    m = models[sf]
    x = synth_image(7, 3, h, w).to("cuda:0")
    n = _n_tiles(tile, h, w, sf)
    flops = {}
    for level in ("2", "3"):
        monkeypatch.setenv("NUNIF_SWIN_SKIP_PAD", level)
        m.render_frame(x, tile_size=tile, batch_size=n)
        torch.cuda.synchronize()
        _hip.profile_enable(True)
        try:
            m.render_frame(x, tile_size=tile, batch_size=n)
            torch.cuda.synchronize()
            flops[level] = {r["name"]: r["flops"] for r in _hip.profile_read()}
        finally:
            _hip.profile_enable(False)
    assert not any("listed" in k for k in flops["2"]), sorted(flops["2"])
    listed = [k for k in flops["3"] if "listed" in k]
    assert listed or tile == 64, sorted(flops["3"])        # (a 48-token side is all read: windows of 6 and two levels of 2 x 2)
    for k in listed:
        whole = k.replace(",listed", "")
        assert whole in flops["2"] and 0 < flops["3"][k] < flops["2"][whole], (k, flops["2"].get(whole), flops["3"][k])


@pytest.mark.parametrize("geometry_change", [False, True])
def test_no_stale_token_is_read(models, level0, monkeypatch, geometry_change):
    """frame A (all ones) and then frame B (noise) on ONE handle: B equals a fresh handle's level-0 render of B"""
    monkeypatch.setenv("NUNIF_SWIN_SKIP_PAD", "3")
    for tile, h, w, sf in ((112, 200, 330, 2), (160, 200, 330, 4)):
        m = make_model(sf)
        ha, wa = (h + 60, w - 70) if geometry_change else (h, w)
        a = torch.ones(3, ha, wa, device="cuda:0")
        assert torch.isfinite(m.render_frame(a, tile_size=tile, batch_size=64)).all()
        b = synth_image(7, 3, h, w).to("cuda:0")
        got = m.render_frame(b, tile_size=tile, batch_size=_n_tiles(tile, h, w, sf))
        assert torch.equal(got, level0[(tile, h, w, sf)]), (tile, sf)


# 2 tiles of 24 x 24 outputs: 36 groups, prologue and drain only; 128 tiles: 2 304 groups on at most 256 x 8 waves, so some waves take
# a second group and the residual prefetch crosses the hand-over from one group to the next
@pytest.mark.parametrize("B", [2, 128])
@pytest.mark.parametrize("seed", [0, 1])
def test_down2_second_pass_on_the_prefetching_kernel_equals_the_gemm(models, seed, B):
    """one down2 launch pair on caller buffers: the accumulating PatchDown form against gemm_res_kernel"""
    from nunif_amd import _hip
    eng = models[2].engine()
    Ho = 24
    gen = torch.Generator().manual_seed(11 + seed)
    a = (torch.randn(B, 2 * Ho, 2 * Ho, 192, generator=gen) * 0.5).half().to("cuda:0")
    fn = _hip.lib().nunif_hip_swin_unet_down2_test
    out = {}
    for form in (0, 1):
        o = torch.full((B, Ho, Ho, 192), float("nan"), dtype=torch.float16, device="cuda:0")
        eng.call(fn, eng.handle, ctypes.c_void_p(a.data_ptr()), ctypes.c_void_p(o.data_ptr()), B, Ho, Ho, form)
        torch.cuda.synchronize()
        out[form] = o
    assert torch.isfinite(out[0]).all() and float(out[0].float().abs().max()) > 0.1
    assert torch.equal(out[1].view(torch.int16), out[0].view(torch.int16)), "the accumulating PatchDown form differs from gemm_res_kernel"
