"""The C = 192 blocks of a swin_unet frame render leave out the windows that only feed cropped padding (DESIGN.md §4.13b,
NUNIF_SWIN_SKIP_PAD level 2): the pixel-major attention launch runs a window list and the weight-stationary tail walks the same
tokens through a table of 16-slot groups.  One tail launch on caller buffers against the whole-tile launch, then whole frames
against levels 0 and 1: no kept bit may change.  Synthetic weights, tiles 64 .. 160."""
import ctypes

import numpy as np
import pytest
import torch

from conftest import synth_image
from oracle import swin_unet as O

pytestmark = pytest.mark.gpu

STAGES = (2, 2, 6, 2, 2)
FIRST = [0, 2, 4, 10, 12]


def make_model(sf, seed=102):
    from nunif_amd.waifu2x.models import swin_unet as M
    cls = {2: M.SwinUNet2x, 4: M.SwinUNet4x}[sf]
    m = cls().eval()
    m.load_state_dict(O.random_state_dict(seed, sf), strict=True)
    return m.to("cuda:0")


@pytest.fixture(scope="module")
def models(hiplib):
    return {sf: make_model(sf) for sf in (2, 4)}


def _grid(tile, h, w, sf):
    from nunif_amd import _hip
    return _hip.tile_grid(h, w, sf, 8 * sf, tile, 4 * sf)


def _group_tokens(groups):
    return np.array([t for g in groups for t in g.tokens()], np.int64)


# ---- one tail launch ---------------------------------------------------------------------------------------------------------------
# (side of the token map, per-tile extents (n_win_y, n_win_x, wrap_y, wrap_x) of a SHIFTED block; the unshifted case drops the wraps)
TAIL_SHAPES = {
    # 2 tiles of 24 x 24, a ragged list: 9 windows = 324 tokens = 21 groups (the last a quarter filled) on 21 workgroups, one trip
    # each: the pipeline's prologue and drain only
    "ragged24": (24, [(1, 2, 1, 1), (0, 2, 1, 1)]),
    # 3 tiles of 96 x 96 with last-column, last-row and corner extents: 17 280 tokens = 1 080 groups on 256 workgroups (>= 4 trips:
    # the full-pipe branch of the DMA wait)
    "edge96": (96, [(15, 12, 1, 1), (11, 15, 1, 1), (7, 9, 1, 1)]),
}


@pytest.mark.parametrize("shift", [3, 0])
@pytest.mark.parametrize("rev", [0, 1])
@pytest.mark.parametrize("shape", sorted(TAIL_SHAPES))
def test_listed_tail_launch_equals_the_whole_launch_on_its_tokens(models, shape, rev, shift):
    from nunif_amd import _hip
    S, ext = TAIL_SHAPES[shape]
    if shift == 0:
        ext = [(ny + 1, nx + 1, 0, 0) for ny, nx, _, _ in ext]
    B = len(ext)
    n_tok = B * S * S
    groups, n_listed = _hip.swin_tail_groups(ext, S, shift)
    listed = _group_tokens(groups)
    assert len(listed) == n_listed == len(set(listed.tolist())) and 0 < n_listed < n_tok
    if shape == "ragged24":
        assert len(groups) <= 256 and n_listed % 16
    else:
        assert len(groups) >= 4 * 256
    eng = models[2].engine()
    gen = torch.Generator().manual_seed(5)
    x0 = (torch.randn(n_tok, 192, generator=gen) * 0.5).half().to("cuda:0")
    att = (torch.randn(n_tok, 192, generator=gen) * 0.5).half().to("cuda:0")
    mask = torch.zeros(n_tok, dtype=torch.bool)
    mask[torch.from_numpy(listed)] = True
    mask = mask.to("cuda:0")
    fn = _hip.lib().nunif_hip_swin_unet_tail192_test
    stage, block = 2, 1                                # swin3.b1: any C = 192 block serves, the tail does not know its shift

    whole = x0.clone()
    eng.call(fn, eng.handle, stage, block, ctypes.c_void_p(att.data_ptr()), ctypes.c_void_p(whole.data_ptr()), n_tok, None, 0, 0, rev)
    att_nan = att.clone()
    att_nan[~mask] = float("nan")                      # an unlisted token of att must never be read
    gdev = torch.frombuffer(bytearray(bytes(groups)), dtype=torch.int32).to("cuda:0")
    assert gdev.data_ptr() % 32 == 0
    got = x0.clone()
    eng.call(fn, eng.handle, stage, block, ctypes.c_void_p(att_nan.data_ptr()), ctypes.c_void_p(got.data_ptr()), n_tok,
             ctypes.c_void_p(gdev.data_ptr()), len(groups), n_listed, rev)
    torch.cuda.synchronize()
    assert torch.isfinite(got).all() and torch.isfinite(whole).all()
    assert not torch.equal(whole[mask], x0[mask])                            # the block did something
    assert torch.equal(got[mask].view(torch.int16), whole[mask].view(torch.int16)), "a listed token differs from the whole-tile launch"
    assert torch.equal(got[~mask].view(torch.int16), x0[~mask].view(torch.int16)), "an unlisted token of x was written"


# ---- whole frames --------------------------------------------------------------------------------------------------------------------
# (tile, frame height, frame width, scale): 64 — only swin4 lists; 112 — swin3 shifted and un-shifted, and swin4; 160 at 4x — every
# C = 192 stage and the 4x net's swin5
FRAMES = [(64, 60, 70, 2), (112, 130, 98, 2), (160, 150, 146, 2), (160, 150, 146, 4)]


def _c192_work(tile, h, w, sf):
    """(listed windows, windows of whole tiles) summed over the C = 192 blocks whose stage lists (a block with nothing to leave out
    runs — and counts — whole), tokens weighted: a window is 36 tokens at every level"""
    from nunif_amd import _hip
    g = _grid(tile, h, w, sf)
    S = tile - 16
    sides = {1: S // 2, 2: S // 4, 3: S // 2}
    if sf == 4:
        sides[4] = S
    n_tiles = g.h_blocks * g.w_blocks
    ext = [_hip.swin_tile_extents(g, t) for t in range(n_tiles)]
    listed = whole = 0
    per_block = {}
    for st, side in sides.items():
        nw = side // 6
        for i in range(STAGES[st]):
            b = FIRST[st] + i
            n = sum((ny + wy) * (nx + wx) for ny, nx, wy, wx in (ext[t][b] for t in range(n_tiles))) if nw > 1 else n_tiles * nw * nw
            per_block[b] = (n, n_tiles * nw * nw)
            listed += n
            whole += n_tiles * nw * nw
    return listed, whole, per_block


def test_the_frames_cover_what_they_claim():
    _, _, pb = _c192_work(64, 60, 70, 2)
    assert all(pb[b][0] == pb[b][1] for b in range(2, 10)) and any(pb[b][0] < pb[b][1] for b in (10, 11))
    _, _, pb = _c192_work(112, 130, 98, 2)
    assert pb[6] == (56, 64) and pb[10][0] == 120 and pb[10][1] == 256
    assert any(pb[b][0] < pb[b][1] for b in (5, 7, 9)) and any(pb[b][0] < pb[b][1] for b in (4, 6, 8))
    _, _, pb = _c192_work(160, 150, 146, 4)
    assert all(any(pb[b][0] < pb[b][1] for b in range(FIRST[st], FIRST[st] + STAGES[st])) for st in (1, 2, 3, 4))


@pytest.mark.parametrize("tile,h,w,sf", FRAMES)
def test_level2_changes_no_bit(models, monkeypatch, tile, h, w, sf):
    m = models[sf]
    x = synth_image(7, 3, h, w).to("cuda:0")
    g = _grid(tile, h, w, sf)
    n_tiles = g.h_blocks * g.w_blocks
    out = {}
    for level in ("0", "1", "2"):
        monkeypatch.setenv("NUNIF_SWIN_SKIP_PAD", level)
        out[level] = m.render_frame(x, tile_size=tile, batch_size=n_tiles).clone()
    assert out["2"].shape == (3, h * sf, w * sf) and torch.isfinite(out["2"]).all()
    assert torch.equal(out["2"], out["0"]), "a kept pixel depends on a skipped window"
    assert torch.equal(out["2"], out["1"])
    monkeypatch.delenv("NUNIF_SWIN_SKIP_PAD")                                 # unset: the default is level 2
    assert torch.equal(m.render_frame(x, tile_size=tile, batch_size=n_tiles), out["2"])
    assert torch.equal(m.render_frame(x, tile_size=tile, batch_size=1), out["2"])     # any minibatch gives the same bits
    # stale activations in the skipped regions: a larger frame first on the same handle, then this one
    big = synth_image(8, 3, 2 * h, 2 * w).to("cuda:0")
    assert torch.isfinite(m.render_frame(big, tile_size=tile, batch_size=64)).all()
    again = m.render_frame(x, tile_size=tile, batch_size=n_tiles)
    assert not torch.isnan(again).any()
    assert torch.equal(again, out["2"])


@pytest.mark.parametrize("tile,h,w,sf", FRAMES)
def test_the_c192_kernels_issue_the_listed_work(models, monkeypatch, tile, h, w, sf):
    """the launchers report the work actually issued: at level 2 the FLOPs of the two C = 192 kernels are listed / whole windows"""
    from nunif_amd import _hip
    m = models[sf]
    x = synth_image(7, 3, h, w).to("cuda:0")
    listed, whole, _ = _c192_work(tile, h, w, sf)
    n_tiles = _grid(tile, h, w, sf).h_blocks * _grid(tile, h, w, sf).w_blocks
    flops = {}
    for level in ("0", "2"):
        monkeypatch.setenv("NUNIF_SWIN_SKIP_PAD", level)
        m.render_frame(x, tile_size=tile, batch_size=n_tiles)
        torch.cuda.synchronize()
        _hip.profile_enable(True)
        try:
            m.render_frame(x, tile_size=tile, batch_size=n_tiles)
            torch.cuda.synchronize()
            flops[level] = {r["name"]: r["flops"] for r in _hip.profile_read()}
        finally:
            _hip.profile_enable(False)
    want = listed / whole
    assert want < 1
    for name in ("qkv_attn_r_kernel<192,32>", "proj_mlp_ws_kernel"):
        assert abs(flops["2"][name] / flops["0"][name] - want) < 1e-6, (name, flops["0"][name], flops["2"][name], want)
