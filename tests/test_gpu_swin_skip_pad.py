"""swin_unet frame renders leave out the windows that only feed cropped padding: the kept pixels must not change
by one bit.  Small tiles — 112 (S = 96, four windows at level 3) and 64 (S = 48, two windows at level 3, the smallest the kernels
take) — on frames of 2 x 2 and 2 x 3 tiles whose last column and row are partly filled, one of them with a last column that keeps
2 pixels; synthetic weights.  At these tiles the dependency cone of swin3's six blocks reaches all of swin1, so only swin5 skips
there; tile 160 (S = 144) is the smallest at which swin1 — the only C = 96 stage of the 4x net — leaves windows out."""
import pytest
import torch

from conftest import synth_image
from oracle import swin_unet as O

pytestmark = pytest.mark.gpu

# (tile, frame height, frame width, scale)
CASES = [(112, 130, 150, 2), (112, 100, 200, 2), (112, 130, 98, 2), (64, 60, 70, 2), (64, 50, 100, 2), (64, 60, 70, 4),
         (160, 150, 146, 2), (160, 150, 146, 4)]


def _grid(tile, h, w, sf):
    from nunif_amd import _hip
    return _hip.tile_grid(h, w, sf, 8 * sf, tile, 4 * sf)


def _listed_windows(tile, h, w, sf):
    """windows run over the whole frame by the four level-1 blocks (swin1.b0, swin1.b1, swin5.b0, swin5.b1), and of whole tiles"""
    from nunif_amd import _hip
    g = _grid(tile, h, w, sf)
    n = [0] * 4
    for t in range(g.h_blocks * g.w_blocks):
        ext = _hip.swin_tile_extents(g, t)
        for k, b in enumerate((0, 1, 12, 13)):
            ny, nx, wy, wx = ext[b]
            n[k] += (ny + wy) * (nx + wx)
    return n, g.h_blocks * g.w_blocks * ((tile - 16) // 6) ** 2


def test_the_cases_cover_ragged_lists_and_both_level1_stages():
    """what the frames below exercise, from the host function: a list whose length is no multiple of 8 (the tail kernel's last
    workgroup is partly filled, its last 32-token group half valid) and lists of swin1 as well as of swin5"""
    counts = {c: _listed_windows(*c) for c in CASES}
    assert any(n[2] % 8 and (36 * n[2]) % 32 for n, _ in counts.values())
    for c in ((160, 150, 146, 2), (160, 150, 146, 4)):
        n, whole = counts[c]
        assert 0 < n[0] < whole and 0 < n[1] < whole, (c, n, whole)
    assert all(0 < n[3] < whole for n, whole in counts.values())


def make_model(sf, seed=102):
    from nunif_amd.waifu2x.models import swin_unet as M
    cls = {2: M.SwinUNet2x, 4: M.SwinUNet4x}[sf]
    m = cls().eval()
    m.load_state_dict(O.random_state_dict(seed, sf), strict=True)
    return m.to("cuda:0")


@pytest.fixture(scope="module")
def models(hiplib):
    return {sf: make_model(sf) for sf in (2, 4)}


@pytest.mark.parametrize("tile,h,w,sf", CASES)
def test_skipping_padding_windows_changes_no_bit(models, monkeypatch, tile, h, w, sf):
    m = models[sf]
    x = synth_image(7, 3, h, w).to("cuda:0")
    g = _grid(tile, h, w, sf)
    n_tiles = g.h_blocks * g.w_blocks                 # all tiles in one minibatch
    assert n_tiles in (4, 6)
    monkeypatch.setenv("NUNIF_SWIN_SKIP_PAD", "0")
    whole = m.render_frame(x, tile_size=tile, batch_size=n_tiles).clone()
    monkeypatch.setenv("NUNIF_SWIN_SKIP_PAD", "1")
    skip = m.render_frame(x, tile_size=tile, batch_size=n_tiles).clone()
    assert skip.shape == (3, h * sf, w * sf) and torch.isfinite(skip).all()
    assert torch.equal(skip, whole), "a kept pixel depends on a skipped window"
    # the active set of a tile depends on the grid and the tile alone: any minibatch gives the same bits
    assert torch.equal(m.render_frame(x, tile_size=tile, batch_size=1), skip)
    # stale activations in the skipped regions: a larger frame first, then this one, against a handle that never saw the larger
    big = synth_image(8, 3, 2 * h, 2 * w).to("cuda:0")
    assert torch.isfinite(m.render_frame(big, tile_size=tile, batch_size=64)).all()
    again = m.render_frame(x, tile_size=tile, batch_size=n_tiles)
    fresh = make_model(sf).render_frame(x, tile_size=tile, batch_size=n_tiles)
    assert not torch.isnan(again).any()
    assert torch.equal(again, fresh) and torch.equal(again, skip)


def test_band_that_ends_inside_the_last_tile_row(models):
    m = models[2]
    x = synth_image(11, 3, 130, 150).to("cuda:0")
    ref = m.render_frame(x, tile_size=112, batch_size=4)
    xe, e = m.row_engine(x, tile_size=112, batch_size=3)
    e.render_tile_rows(xe, 0, e.h_blocks)
    y1 = e.output_tile_step * (e.h_blocks - 1) + 21            # 21 rows into the last tile row, short of the frame's end
    assert e.output_tile_step * (e.h_blocks - 1) < y1 < e.y_h
    assert torch.equal(e.stitch_rows(0, y1), ref[:, :y1])
    assert torch.equal(e.stitch_rows(y1, e.y_h), ref[:, y1:])


@pytest.mark.parametrize("tile,h,w,sf", [(112, 130, 98, 2), (160, 150, 146, 4)])
def test_the_level1_kernels_issue_less_work(models, monkeypatch, tile, h, w, sf):
    """the launchers report the work actually issued: with the switch on the C = 96 attention and tail count fewer FLOPs"""
    from nunif_amd import _hip
    m = models[sf]
    x = synth_image(7, 3, h, w).to("cuda:0")
    n, whole = _listed_windows(tile, h, w, sf)
    levels = 4 if sf == 2 else 2                                          # C = 96 blocks: swin1 and swin5; the 4x net's swin5 is C = 192
    listed = sum(n[:levels])
    flops = {}
    for on in ("0", "1"):
        monkeypatch.setenv("NUNIF_SWIN_SKIP_PAD", on)
        m.render_frame(x, tile_size=tile, batch_size=4)
        torch.cuda.synchronize()
        _hip.profile_enable(True)
        try:
            m.render_frame(x, tile_size=tile, batch_size=4)
            torch.cuda.synchronize()
            flops[on] = {r["name"]: r["flops"] for r in _hip.profile_read()}
        finally:
            _hip.profile_enable(False)
    for name in ("qkv_attn_r_kernel<96,16>", "proj_mlp_r_kernel<96,2,8,true>"):
        want = listed / (levels * whole)                              # FLOPs are proportional to the windows issued
        assert abs(flops["1"][name] / flops["0"][name] - want) < 1e-6 and want < 1, (name, flops["0"][name], flops["1"][name], want)
    for name in ("qkv_attn_r_kernel<192,32>", "proj_mlp_ws_kernel"):
        assert flops["1"][name] == flops["0"][name], name     # the C = 192 blocks run whole tiles
