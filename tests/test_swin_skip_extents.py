"""The window extents of a swin_unet frame render (``nunif_hip_swin_unet_tile_extents``) against a brute-force
dependency propagation: a boolean "needed" mask over the tokens of one tile is pushed backwards from the pixels the stitch reads
through the real (shifted, masked) window partitions, PatchUp and PatchDown.  A needed token outside the active windows would change
a kept pixel and fails; the slack (active windows that no needed token sits in) is reported and bounded.  No GPU."""
import numpy as np
import pytest

from nunif_amd import _hip

STAGES = (2, 2, 6, 2, 2)
SHIFTS = [3 if i % 2 else 0 for k in STAGES for i in range(k)]


def _grid(h, w, scale, tile):
    return _hip.tile_grid(h, w, scale, 8 * scale, tile, 4 * scale)


def _block_back(m, shift):
    """needed mask of a block's output -> of its input, and the windows (rolled partition) that hold a needed output token"""
    S = m.shape[0]
    nw = S // 6
    if S <= 6:
        shift = 0
    r = np.roll(m, (-shift, -shift), (0, 1))                 # torchvision: roll by -shift, partition, roll back
    lab = np.zeros(S, np.int64)                              # mask regions of the rolled axis: [0, S-6), [S-6, S-3), [S-3, S)
    if shift:
        lab[S - 6:S - 3] = 1
        lab[S - 3:] = 2
    need_in = np.zeros_like(r)
    win = np.zeros((nw, nw), bool)
    for wy in range(nw):
        for wx in range(nw):
            blk = r[6 * wy:6 * wy + 6, 6 * wx:6 * wx + 6]
            if not blk.any():
                continue
            win[wy, wx] = True
            ly, lx = lab[6 * wy:6 * wy + 6], lab[6 * wx:6 * wx + 6]
            reg = ly[:, None] * 3 + lx[None, :]
            for g in np.unique(reg):                         # a query reads the keys of its own window AND mask region
                sel = reg == g
                if blk[sel].any():
                    need_in[6 * wy:6 * wy + 6, 6 * wx:6 * wx + 6][sel] = True
    return np.roll(need_in, (shift, shift), (0, 1)), win


def _brute(g, tile):
    """per block (forward order): (needed-window matrix, needed token mask of the block's OUTPUT)"""
    S = g.tile_size - 16
    ti, tj = divmod(tile, g.w_blocks)
    ny = min(g.out_tile_size, g.y_h - g.output_tile_step * ti)      # stitch_kernel: tile pixel t = Y - ostep * i, 0 <= t < To, Y < y_h
    nx = min(g.out_tile_size, g.y_w - g.output_tile_step * tj)
    px = np.zeros((S * g.scale, S * g.scale), bool)
    px[:max(ny, 0), :max(nx, 0)] = True
    m = px.reshape(S, g.scale, S, g.scale).any((1, 3))               # to_image + pixel_shuffle
    res = [None] * sum(STAGES)
    first = np.concatenate([[0], np.cumsum(STAGES)])

    def stage(st, m):
        for i in reversed(range(STAGES[st])):
            out = m
            m, win = _block_back(m, SHIFTS[first[st] + i])
            res[first[st] + i] = (win, out)
        return m

    up = lambda m: m.reshape(m.shape[0] // 2, 2, m.shape[1] // 2, 2).any((1, 3))    # PatchUp: fine token i <- coarse token i / 2
    down = lambda m: np.repeat(np.repeat(m, 2, 0), 2, 1)                            # PatchDown: coarse token j <- fine 2 j, 2 j + 1
    top_in = stage(4, m)
    e4 = stage(3, up(top_in))
    e3 = stage(2, up(e4))
    e2 = stage(1, down(e3) | e4)                                      # skip connection: both consumers
    stage(0, down(e2) | top_in)
    return res


def _active(ext, nw):
    ny, nx, wy, wx = ext
    ay = np.zeros(nw, bool)
    ax = np.zeros(nw, bool)
    ay[:ny] = True
    ax[:nx] = True
    if wy:
        ay[nw - 1] = True
    if wx:
        ax[nw - 1] = True
    return ay, ax


def _check(g, tile):
    exts = _hip.swin_tile_extents(g, tile, STAGES, SHIFTS)
    worst = 0
    S = g.tile_size - 16
    sizes = [S] * 2 + [S // 2] * 2 + [S // 4] * 6 + [S // 2] * 2 + [S] * 2
    for b, ((win, _), ext, size) in enumerate(zip(_brute(g, tile), exts, sizes)):
        ay, ax = _active(ext, size // 6)
        act = ay[:, None] & ax[None, :]
        assert not (win & ~act).any(), (tile, b, ext, "a needed window does not run")
        for a_act, need in ((ay, win.any(1)), (ax, win.any(0))):
            slack = int((a_act & ~need).sum())
            worst = max(worst, slack)
            assert slack <= 1, (tile, b, ext, slack)
    return worst


def _corner_tiles(g):
    return sorted({0, g.w_blocks - 1, (g.h_blocks - 1) * g.w_blocks, g.h_blocks * g.w_blocks - 1})


@pytest.mark.parametrize("scale", [1, 2, 4])
@pytest.mark.parametrize("tile", [64, 112, 256])
def test_extents_cover_the_brute_force_need(tile, scale):
    step = tile - 16 - 4
    keeps = [1, 7, step // 2, step]                 # input pixels the last column / row keeps beyond the first tile's reach
    worst = 0
    for k, rw in enumerate(keeps):
        rh = keeps[(k + 1) % 4]
        g = _grid(tile - 16 + rh, tile - 16 + rw, scale, tile)
        assert (g.h_blocks, g.w_blocks) == (2, 2)
        for t in range(4):
            worst = max(worst, _check(g, t))
    print(f"tile {tile} scale {scale}: worst slack {worst} window(s) per axis and block")


@pytest.mark.parametrize("h,w,scale", [(1080, 1920, 2), (2160, 3840, 2), (2160, 3840, 4)])
def test_extents_of_video_frames(h, w, scale):
    g = _grid(h, w, scale, 256)
    worst = max(_check(g, t) for t in _corner_tiles(g))
    print(f"{h}x{w} {scale}x: {g.h_blocks}x{g.w_blocks} tiles, worst slack {worst}")


@pytest.mark.parametrize("tile,scale", [(64, 1), (112, 2), (256, 4)])
def test_one_token_prefix_runs_only_the_wrap_window_of_a_shifted_block(tile, scale):
    """The shortest prefix a consumer can need is one token: a shifted block then runs its wrap window alone (n_win 0, wrap 1), an
    un-shifted one its first window.  No grid of tile_grid_init has such a tile — a last tile exists only where the frame passes
    the previous tile's reach, so the stitch reads more than blend_size pixels of it, five tokens at least — so the grid is
    edited by hand: the frame ends one token into the last column and two tokens into the last row."""
    for w in range(tile - 16 + 1, tile - 16 + 40):
        g = _grid(w, w, scale, tile)
        assert min(g.out_tile_size, g.y_w - g.output_tile_step * (g.w_blocks - 1)) > 4 * scale      # what real grids give
    g = _grid(tile - 16 + 7, tile - 16 + 7, scale, tile)
    assert (g.h_blocks, g.w_blocks) == (2, 2)
    g.y_w = g.output_tile_step + scale
    g.y_h = g.output_tile_step + 2 * scale
    ext = _hip.swin_tile_extents(g, 3)
    assert ext[-1] == (0, 0, 1, 1) and ext[-2] == (1, 1, 0, 0)
    for t in range(4):
        assert _check(g, t) == 0


def test_interior_and_full_tiles_run_whole():
    g = _grid(1080, 1920, 2, 256)
    whole = [(40, 40, 0, 0), (39, 39, 1, 1)] + [(20, 20, 0, 0), (19, 19, 1, 1)] + [(10, 10, 0, 0), (9, 9, 1, 1)] * 3 + \
            [(20, 20, 0, 0), (19, 19, 1, 1)] + [(40, 40, 0, 0), (39, 39, 1, 1)]
    assert _hip.swin_tile_extents(g, 0) == whole
    assert _hip.swin_tile_extents(g, 9 * 3 + 4) == whole
    g = _grid(112 - 16 + 92, 112 - 16 + 92, 2, 112)            # the frame fills its 2 x 2 tiles exactly
    full = _hip.swin_tile_extents(g, 3)
    assert full[0] == (16, 16, 0, 0) and full[-1] == (15, 15, 1, 1)


def test_1080p_2x_last_column_and_row():
    """Hand-derived per-axis extents of the 1080p 2x frame at tile 256 — asserted on the brute force first (it is the
    authority), then on the function: needed tokens after each block, walking backwards (swin5 33 / 36, swin4 21 / 24,
    swin3 15 .. 30, swin2 63 / 66, swin1 135 / 138 for the last column; 141 / 144, 75 / 78, 39 .. 54 (the brute force says 54 where a hand count said 60), 111 / 114, 231 / 234 for the last row)."""
    g = _grid(1080, 1920, 2, 256)
    assert (g.h_blocks, g.w_blocks, g.input_tile_step) == (5, 9, 236)
    col, row = g.w_blocks - 1, (g.h_blocks - 1) * g.w_blocks
    # windows along the axis, forward order: (n_win, wrap) per block
    want_col = [(23, 0), (22, 1), (11, 0), (10, 1), (5, 0), (4, 1), (4, 0), (3, 1), (3, 0), (2, 1), (4, 0), (3, 1), (6, 0), (5, 1)]
    want_row = [(39, 0), (38, 1), (19, 0), (18, 1), (9, 0), (8, 1), (8, 0), (7, 1), (7, 0), (6, 1), (13, 0), (12, 1), (24, 0), (23, 1)]
    for tile, axis, want in ((col, 1, want_col), (row, 0, want_row)):
        brute = _brute(g, tile)
        for (win, _), (n, wrap) in zip(brute, want):
            need = win.any(1 - axis)
            nw = need.size
            expect = np.zeros(nw, bool)
            expect[:n] = True
            if wrap:
                expect[nw - 1] = True
            assert (need == expect).all(), (tile, n, wrap)
        ext = _hip.swin_tile_extents(g, tile)
        assert [(e[axis], e[2 + axis]) for e in ext] == want
        other = 1 - axis                                      # the other axis of these tiles is whole
        assert all(e[other] + e[2 + other] == s for e, s in zip(ext, [40] * 2 + [20] * 2 + [10] * 6 + [20] * 2 + [40] * 2))
