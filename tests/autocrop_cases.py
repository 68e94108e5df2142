"""The frames that the autocrop tests share (tests/test_autocrop_cpu.py, tests/test_gpu_autocrop.py and
tests/golden/make_golden_autocrop.py): generated from a seed on the k/255 grid, never stored.

Black kind: content uniform in 70..255, bars uniform in 0..5.  Flat kind: content uniform in 0..255, bars 128 +/- 3.  Every seed
is chosen so that each float64 statistic of the frame lies at least 0.01 from the threshold it is compared with (the CPU test
asserts it): masks and slices can then be compared with equality.

Which loop of nunif_amd/csrc/autocrop.hip a shape exercises: a wave of the row pass covers 256 columns per trip where W % 4 == 0
and 64 otherwise, a band of the black column pass is 32 rows, the flat column pass stages 256 rows per trip (64 where W % 4 != 0)
and its workgroup holds 8 columns.
"""
import torch

MODES = ("black", "black_tb", "black_lr", "flat", "flat_tb", "flat_lr")
MODS = (1, 2)
KINDS = ("black", "flat")
MARGIN = 0.01

# name: (H, W, top, bottom, left, right, seed)
CASES = {
    "s37x67": (37, 67, 5, 3, 7, 0, 1),                # odd sizes, scalar loads, two row trips, a partial column tile
    "s64x200": (64, 200, 8, 8, 0, 0, 2),              # 16-byte loads, one trip
    "s130x259": (130, 259, 0, 17, 33, 9, 3),          # scalar loads, 5 bands, 3 staging trips, 5 row trips
    "s9x300": (9, 300, 2, 0, 0, 0, 4),                # fewer rows than a band; two waves of a row workgroup past the last row
    "s270x480": (270, 480, 34, 34, 0, 0, 5),          # the letterbox of a 16:9 frame; two 16-byte row trips, two staging trips
    "s1x1": (1, 1, 0, 0, 0, 0, 6),
    "s12x1030": (12, 1030, 1, 0, 3, 2, 7),            # wider than one row trip without 16-byte loads (17 trips), 129 column tiles
    "s10x1032": (10, 1032, 0, 2, 4, 0, 8),            # ... and with them (5 trips); 258 column quads: two blocks of the band pass
    "s1100x40": (1100, 40, 7, 5, 2, 0, 9),            # taller than one staging trip (5) and one band (35 bands)
    "all_bar": (20, 36, 20, 0, 0, 0, 10),             # every row and column is a bar: slice(None)
    "no_bar": (20, 36, 0, 0, 0, 0, 11),               # none is: slice(None)
}
FIRST_SIX = ("s37x67", "s64x200", "s130x259", "s9x300", "s270x480", "s1x1")
# a batch whose frames differ in bars and content
BATCH = [(48, 84, 6, 4, 8, 0, 21), (48, 84, 0, 10, 0, 12, 22), (48, 84, 3, 3, 5, 5, 23)]
# 20 frames of one geometry; frame SEQ_PLAIN has no bars: 19 / 20 at threshold 0.95 is still a border
SEQ_SHAPE, SEQ_FRAMES, SEQ_PLAIN, SEQ_SEED = (37, 67, 5, 3, 7, 0), 20, 11, 100


def make_frame(kind, H, W, top, bottom, left, right, seed):
    """[3, H, W] float32 on the k/255 grid."""
    g = torch.Generator().manual_seed(seed * 2 + (1 if kind == "flat" else 0))
    if kind == "black":
        content = torch.randint(70, 256, (3, H, W), generator=g)
        bars = torch.randint(0, 6, (3, H, W), generator=g)
    else:
        content = torch.randint(0, 256, (3, H, W), generator=g)
        bars = torch.randint(125, 132, (3, H, W), generator=g)
    bar = torch.zeros((H, W), dtype=torch.bool)
    bar[:top] = True
    bar[H - bottom:] = bottom > 0
    bar[:, :left] = True
    bar[:, W - right:] = right > 0
    return torch.where(bar, bars, content).to(torch.float32) / 255.0


def case_frame(name, kind):
    return make_frame(kind, *CASES[name])


def batch_frames(kind):
    return torch.stack([make_frame(kind, *c) for c in BATCH])


def seq_frames(kind):
    H, W, t, b, l, r = SEQ_SHAPE
    return torch.stack([make_frame(kind, H, W, *((0, 0, 0, 0) if i == SEQ_PLAIN else (t, b, l, r)), SEQ_SEED + i)
                        for i in range(SEQ_FRAMES)])


def all_inputs(kind):
    """name -> [B, 3, H, W] for every input whose statistics are recorded."""
    out = {name: case_frame(name, kind).unsqueeze(0) for name in CASES}
    out["batch"] = batch_frames(kind)
    out["seq"] = seq_frames(kind)
    return out


def enc_slice(s):
    return [-1 if s.start is None else s.start, -1 if s.stop is None else s.stop]


def dec_slice(a):
    return slice(None if a[0] < 0 else int(a[0]), None if a[1] < 0 else int(a[1]))


STAT_KEYS = ("row_a", "row_b", "col_a", "col_b")
STAT_NAMES = {"black": ("row mean", "row maxdev", "col mean", "col maxdev"),
              "flat": ("row median", "row fraction", "col median", "col fraction")}
LIMIT, FLOOR = 2.2, 2.0 ** -23           # the project's fp32 factor; one fp32 ulp at 1.0 (the median's e_ref can be exactly 0)


def error_ratios(measured, f64, recorded):
    """``e_hip / (LIMIT * e_ref + FLOOR)`` per statistic of one input, e = the largest absolute error against float64 and
    ``recorded`` the fp32 run of the restatement.  At most 1 where the bound holds."""
    out = {}
    for k in STAT_KEYS:
        e_hip = float((measured[k].double() - f64[k]).abs().max())
        e_ref = float((torch.as_tensor(recorded[k]).double() - f64[k]).abs().max())
        out[k] = (e_hip / (LIMIT * e_ref + FLOOR), e_hip, e_ref)
    return out
