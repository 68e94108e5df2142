"""What the producers of a swin_unet frame render write at NUNIF_SWIN_SKIP_PAD level 3 (``nunif_hip_swin_unet_producer_tokens``,
DESIGN.md §4.13b) against a brute-force restatement in two dimensions: from ``swin_tile_extents`` every token any listed window touches
is marked, both halves of a wrap window included, and the marks are pushed back through the 2 x 2 relations of PatchUp / PatchDown.
The table of every tile and producer must hold that set (written is a superset of read), must EQUAL the product of the set's two
axis projections (the form the builder states), and must name every token exactly once.  No GPU."""
import numpy as np
import pytest

from nunif_amd import _hip

STAGES = (2, 2, 6, 2, 2)
FIRST = [0, 2, 4, 10, 12]
SHIFTS = [3 if i % 2 else 0 for k in STAGES for i in range(k)]

# (tile, frame height, frame width, scale): ragged last rows / columns, one tile, and a frame the grid divides exactly
GRIDS = [(64, 100, 150, 2), (64, 136, 260, 2), (112, 200, 330, 2), (160, 200, 330, 2), (160, 200, 330, 4), (64, 40, 40, 2),
         (64, 32 * 3, 32 * 4, 2), (256, 1080, 1920, 2)]


def _window_marks(S, ext, shift):
    """2-D marks of one block's active windows on a side-S map"""
    nw = S // 6
    if S <= 6:
        shift = 0
    ny, nx, wy, wx = ext
    m = np.zeros((S, S), bool)
    for a in range(nw):
        if not (a < ny or (wy and a == nw - 1)):
            continue
        ys = [(6 * a + shift + t) % S for t in range(6)]
        for b in range(nw):
            if not (b < nx or (wx and b == nw - 1)):
                continue
            xs = [(6 * b + shift + t) % S for t in range(6)]
            m[np.ix_(ys, xs)] = True
    return m


def _parents(m):
    return m[0::2, 0::2] | m[0::2, 1::2] | m[1::2, 0::2] | m[1::2, 1::2]


def _children(m):
    return np.repeat(np.repeat(m, 2, 0), 2, 1)


def _brute(S, tile_ext, listed, f1_whole):
    """per producer the 2-D set of one tile: what is READ behind it in the frame"""
    sides = [S, S // 2, S // 4, S // 2, S]
    R = []
    for st in range(5):
        m = np.zeros((sides[st], sides[st]), bool)
        for i in range(FIRST[st], FIRST[st] + STAGES[st]):
            m |= _window_marks(sides[st], tile_ext[i], SHIFTS[i]) if listed[i] else True
        R.append(m)
    up1, up2 = _parents(R[4]), _parents(R[3])       # PatchUp inputs with a child that is read
    n3 = R[2] | up2                                  # down2's outputs: swin3's reads, up2's inputs
    n2 = R[1] | _children(n3) | _children(up2) | R[3] | up1     # down1's: swin2's reads, down2's parents, up2's skip tokens, up1's inputs
    n1 = R[0] | _children(n2) | _children(up1) | R[4]           # the stem's: swin1's reads, down1's parents, up1's skip tokens
    if f1_whole:
        n1 = np.ones_like(n1)
    return {"stem": n1, "down1": n2, "down2": n3, "up2": up2, "up1": up1}


def _product(m):
    return np.outer(m.any(1), m.any(0))


@pytest.mark.parametrize("tile,h,w,sf", GRIDS)
@pytest.mark.parametrize("all_listed", [True, False])
def test_tables_equal_the_brute_force_sets(tile, h, w, sf, all_listed):
    g = _hip.tile_grid(h, w, sf, 8 * sf, tile, 4 * sf)
    S = tile - 16
    n_tiles = g.h_blocks * g.w_blocks
    ext = [_hip.swin_tile_extents(g, t, STAGES, SHIFTS) for t in range(n_tiles)]
    listed = [1] * 14 if all_listed else [1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 1, 1, 1, 1]      # swin3 on whole tiles
    want = [_brute(S, ext[t], listed, sf == 4) for t in range(n_tiles)]
    for prod, side in (("down1", S // 2), ("down2", S // 4), ("up2", S // 4), ("up1", S // 2)):
        entries, n = _hip.swin_producer_tokens(ext, S, prod, STAGES, SHIFTS, listed, f1_whole=sf == 4)
        toks = np.array(entries[:n], np.int64)
        assert len(entries) % 32 == 0 and len(entries) - n < 32 and all(e == entries[n - 1] for e in entries[n:])
        assert n == len(set(toks.tolist())) and (np.diff(toks) > 0).all(), "a token is listed twice or out of order"
        got = np.zeros(n_tiles * side * side, bool)
        got[toks] = True
        got = got.reshape(n_tiles, side, side)
        for t in range(n_tiles):
            assert not (want[t][prod] & ~got[t]).any(), (prod, t, "a token that is read is not written")
            assert np.array_equal(got[t], _product(want[t][prod])), (prod, t)
    ph, pw = 24, 16
    nty, ntx = -(-S // ph), -(-S // pw)
    patches, n = _hip.swin_producer_tokens(ext, S, "stem", STAGES, SHIFTS, listed, f1_whole=sf == 4, patch=(ph, pw))
    assert n == len(patches) == len(set(patches)) and patches == sorted(patches)
    got = np.zeros((n_tiles, nty, ntx), bool)
    got.reshape(-1)[np.array(patches, np.int64)] = True
    for t in range(n_tiles):
        need = _product(want[t]["stem"])
        pad = np.zeros((nty * ph, ntx * pw), bool)
        pad[:S, :S] = need
        assert np.array_equal(got[t], pad.reshape(nty, ph, ntx, pw).any((1, 3))), ("stem", t)


def test_the_grids_leave_something_out_and_an_interior_tile_nothing():
    g = _hip.tile_grid(1080, 1920, 2, 16, 256, 8)
    ext = [_hip.swin_tile_extents(g, t, STAGES, SHIFTS) for t in range(g.h_blocks * g.w_blocks)]
    S = 240
    for prod, side in (("down1", 120), ("down2", 60), ("up2", 60), ("up1", 120)):
        _, n_all = _hip.swin_producer_tokens(ext, S, prod)
        assert n_all < len(ext) * side * side, (prod, n_all)   # the last tile row and column are mostly padding
        _, n0 = _hip.swin_producer_tokens(ext[:1], S, prod)
        assert n0 == side * side                        # tile 0 of a 1080p frame is all frame: nothing to leave out


def test_bad_arguments_are_refused():
    g = _hip.tile_grid(100, 150, 2, 16, 64, 8)
    ext = [_hip.swin_tile_extents(g, 0, STAGES, SHIFTS)]
    with pytest.raises(Exception):
        _hip.swin_producer_tokens(ext, 50, "down1")                 # not a swin_unet side
    with pytest.raises(Exception):
        _hip.swin_producer_tokens(ext, 48, "stem", patch=(0, 16))
