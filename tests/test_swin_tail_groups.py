"""The token groups of the C = 192 tail of a swin_unet frame render (``nunif_hip_swin_unet_tail_groups``) against a
brute-force enumeration: the tokens of every active window of ``swin_tile_extents``, window by window through the rolled partition.
The tail works in place on x, so a token named twice would have the block applied twice, and a token named outside the windows the
attention ran would read att nobody wrote: the groups must name exactly that token set, each token once.  No GPU."""
import numpy as np
import pytest

from nunif_amd import _hip

STAGES = (2, 2, 6, 2, 2)
FIRST = np.concatenate([[0], np.cumsum(STAGES)])
SHIFTS = [3 if i % 2 else 0 for k in STAGES for i in range(k)]

GRIDS = [(64, 60, 70, 2), (112, 130, 98, 2), (112, 100, 200, 2), (160, 150, 146, 2), (160, 150, 146, 4), (256, 1080, 1920, 2)]


def _grid(tile, h, w, scale):
    return _hip.tile_grid(h, w, scale, 8 * scale, tile, 4 * scale)


def _c192_blocks(g):
    """(block index, side of its token map) of every C = 192 block: swin2..4, and swin5 of the 4x net"""
    S = g.tile_size - 16
    sides = {1: S // 2, 2: S // 4, 3: S // 2}
    if g.scale == 4:
        sides[4] = S
    return [(FIRST[st] + i, side) for st, side in sides.items() for i in range(STAGES[st])]


def _decode(groups):
    """tokens named by a table, in table order, and the count of every group"""
    a = np.frombuffer(groups, np.int32).reshape(-1, 8) if len(groups) else np.zeros((0, 8), np.int32)
    bounds = a[:, 6].view(np.uint32).astype(np.int64)
    cnt = (bounds >> 25) & 31
    firsts = np.stack([np.zeros_like(bounds)] + [(bounds >> (5 * p)) & 31 for p in range(5)], 1)
    assert (np.diff(firsts, axis=1) >= 0).all() and (a[:, 7] == 0).all()
    toks = []
    for r in range(16):
        p = (firsts <= r).sum(1) - 1
        toks.append(a[np.arange(len(a)), p].astype(np.int64) + r)
    toks = np.stack(toks, 1) if len(a) else np.zeros((0, 16), np.int64)
    live = np.arange(16)[None, :] < cnt[:, None]
    return toks[live], cnt


def _brute_tile(ext, S, shift):
    """token indices y * S + x of the active windows of one tile, enumerated window by window"""
    ny, nx, wy_, wx_ = ext
    nw = S // 6
    if S <= 6:
        shift = 0
    act = lambda n, wrap, w: w < n or (wrap and w == nw - 1)
    out = []
    t = np.arange(6)
    for wy in range(nw):
        if not act(ny, wy_, wy):
            continue
        ys = (6 * wy + shift + t) % S
        for wx in range(nw):
            if act(nx, wx_, wx):
                xs = (6 * wx + shift + t) % S
                out.append((ys[:, None] * S + xs[None, :]).ravel())
    return np.concatenate(out) if out else np.zeros(0, np.int64)


@pytest.fixture(scope="module", params=GRIDS, ids=lambda p: "t%d_%dx%d_%dx" % p)
def case(request):
    g = _grid(*request.param)
    n_tiles = g.h_blocks * g.w_blocks
    ext = [_hip.swin_tile_extents(g, t, STAGES, SHIFTS) for t in range(n_tiles)]
    return request.param, g, n_tiles, ext


def test_groups_name_the_tokens_of_the_listed_windows_once_each(case):
    _, g, n_tiles, ext = case
    for blk, S in _c192_blocks(g):
        per_tile = [_brute_tile(ext[t][blk], S, SHIFTS[blk]) for t in range(n_tiles)]
        want = np.concatenate([p + t * S * S for t, p in enumerate(per_tile)])
        assert len(np.unique(want)) == len(want)
        groups, n_tok = _hip.swin_tail_groups([ext[t][blk] for t in range(n_tiles)], S, SHIFTS[blk])
        got, cnt = _decode(groups)
        assert n_tok == len(want) == len(got), (blk, n_tok, len(want), len(got))
        assert np.array_equal(np.sort(got), np.sort(want)), blk                 # the same multiset: every token exactly once
        assert np.array_equal(got, np.sort(want)), blk                          # ... and in ascending order ([tile][y][x])
        assert ((cnt >= 1) & (cnt <= 16)).all(), blk
        assert len(cnt) == -(-len(want) // 16), (blk, len(cnt), len(want))      # only the last group is partly filled
        assert (cnt[:-1] == 16).all(), blk


def test_minibatch_splits_name_the_same_tokens_per_tile(case):
    _, g, n_tiles, ext = case
    for blk, S in _c192_blocks(g):
        whole, _ = _decode(_hip.swin_tail_groups([ext[t][blk] for t in range(n_tiles)], S, SHIFTS[blk])[0])
        for mb in (1, 2):
            parts = []
            for t0 in range(0, n_tiles, mb):
                toks, _ = _decode(_hip.swin_tail_groups([ext[t][blk] for t in range(t0, min(n_tiles, t0 + mb))], S, SHIFTS[blk])[0])
                assert ((toks >= 0) & (toks < min(mb, n_tiles - t0) * S * S)).all()
                parts.append(toks + t0 * S * S)
            assert np.array_equal(np.concatenate(parts), whole), (blk, mb)


def test_1080p_window_counts():
    """the windows needed on the 1080p 2x grid (tile 256, 45 tiles): swin2 16 929 of 18 000, swin3 4 165 / 4 165 / 4 032 / 4 032 /
    3 901 / 3 901 of 4 500, swin4 15 252 of 18 000 — 36 tokens each"""
    g = _grid(256, 1080, 1920, 2)
    n_tiles = g.h_blocks * g.w_blocks
    assert n_tiles == 45
    ext = [_hip.swin_tile_extents(g, t, STAGES, SHIFTS) for t in range(n_tiles)]
    want = [16929, 16929, 4165, 4165, 4032, 4032, 3901, 3901, 15252, 15252]
    for (blk, S), w in zip(_c192_blocks(g), want):
        groups, n_tok = _hip.swin_tail_groups([ext[t][blk] for t in range(n_tiles)], S, SHIFTS[blk])
        assert n_tok == 36 * w, (blk, n_tok // 36, w)
        assert len(groups) == -(-36 * w // 16)


def test_short_runs_still_pack_full_groups():
    """a shifted block with one window per axis next to its wrap window: runs of 3, 6 and 9 tokens, up to 5 pieces in a group"""
    for ext in ([(0, 0, 1, 1)], [(1, 0, 1, 1), (0, 1, 1, 1), (0, 0, 1, 1)], [(1, 1, 1, 1)] * 2):
        for S in (12, 24, 30):
            want = np.concatenate([_brute_tile(e, S, 3) + t * S * S for t, e in enumerate(ext)])
            got, cnt = _decode(_hip.swin_tail_groups(ext, S, 3)[0])
            assert np.array_equal(got, np.sort(want)) and len(cnt) == -(-len(want) // 16) and (cnt[:-1] == 16).all()
