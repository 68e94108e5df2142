"""``waifu2x.wgmlp_4x`` on the HIP engine (csrc/wgmlp.hip) against ``tests/wgmlp_ref.py`` in float64, with that restatement under
the fp16 emulation as the yardstick (``errloc.check_localised``; limits: outputs — the net's image AND the kernel's output map —
2.5 / 3.75 with tau 5e-4, taps 3.5 / 5.5 with tau = 2e-3 x the tap's rms).

The fused window-gMLP kernel alone (``nunif_hip_wgmlp_debug_gmlp``): C = 128 and 256, plain and shifted, on 8 x 8 (one window;
shifted: four windows that are three-quarters padding), 16 x 24, 2 x 24 x 40 and a map with more windows than the launch has
workgroups (the grid-stride loop takes a second trip); the output and the five inner taps per 8 x 8 window, aligned and shifted by 4;
and once with the GELU's pre-activations in the far negative tail, where the erf form can be told from the tanh approximation.
The net: tiles 64 and 112, batches 1 and 3, benign and hot weights, every block tap, PSNR against the fixture, and the invariants.
``measure_gmlp`` / ``measure_net`` return the statistics the tests assert; tools/wgmlp_errloc.py runs the same cases and writes the
worst ratios to profiles/wgmlp_errloc.txt.
"""
import os

import numpy as np
import pytest
import torch

import errloc
import wgmlp_ref as R
from conftest import GOLDEN

pytestmark = pytest.mark.gpu

SEED, INPUT_SEED = 21, 5
NAME = "waifu2x.wgmlp_4x"


def _model(regime="benign", seed=SEED):
    from nunif_amd import synthetic
    sd = synthetic.wgmlp_state_dict(seed, regime)
    return sd, make_model(sd)


@pytest.fixture(scope="module")
def benign():
    return _model()


@pytest.fixture(scope="module")
def hot():
    return _model("hot")


# block index -> a level-1 (C = 128) and a level-2 (C = 256) block; their own place in the net does not matter here
GMLP_BLOCK = {128: 0, 256: 3}
# workgroups of a launch (csrc/wgmlp_host.h wgmlp_max_groups): 512 at C = 128, 256 at C = 256
GMLP_SHAPES = {128: [(1, 8, 8), (1, 16, 24), (2, 24, 40), (2, 136, 136)], 256: [(1, 8, 8), (1, 16, 24), (2, 24, 40), (2, 96, 96)]}


def make_model(sd):
    from nunif_amd.nunif.models import create_model
    import nunif_amd.waifu2x.utils  # noqa: F401
    m = create_model(NAME).eval()
    m.load_state_dict(sd)
    return m.to("cuda:0")


def measure_gmlp(sd, m, block, x, shift, with_taps):
    """The kernel alone on x [B,H,W,C]: {"out": stats with the OUTPUT limits' B / tau, tap name: stats with the tap limits' B / tau}.
    Without taps the launch is the forward's own instance of the kernel."""
    p = R.block_prefixes()[block]
    with torch.inference_mode():
        errloc.set_threads()
        y, taps = m.engine().debug_gmlp(block, x.to("cuda:0").contiguous(), shift, taps=with_taps)
        t64, te = ({}, {}) if with_taps else (None, None)
        y64, ye = R.gmlp64(sd, p, x, shift, t64), R.gmlp_emulated(sd, p, x, shift, te)
    cells = [(8, 0)]                       # localised_stats looks at the aligned partition and the one shifted by half a cell
    out = {"out": errloc.localised_stats(errloc.nhwc(y.cpu()), errloc.nhwc(y64), errloc.nhwc(ye), cells, errloc.B_OUT, errloc.TAU_OUT)}
    for k in (R.GMLP_TAPS if with_taps else ()):
        rms = float(t64[k].pow(2).mean().sqrt())
        out[k] = errloc.localised_stats(errloc.nhwc(taps[k].cpu()), errloc.nhwc(t64[k]), errloc.nhwc(te[k]), cells, errloc.B_TAP,
                                        errloc.TAP_TAU_REL * rms)
    return out


def assert_gmlp(stats, label):
    for k, st in stats.items():
        print(f"{label}: {k} global {st['global']:.2f} worst {st['worst']:.2f}")
    for k, st in stats.items():
        if k == "out":
            errloc.assert_localised(st, errloc.A_OUT, errloc.B_OUT, errloc.TAU_OUT, f"{label} out")
        else:
            errloc.assert_localised(st, errloc.A_TAP, errloc.B_TAP, st["_tau"], f"{label} {k}")


@pytest.mark.parametrize("shift", [False, True], ids=["plain", "shifted"])
@pytest.mark.parametrize("C,shape", [(c, s) for c in (128, 256) for s in GMLP_SHAPES[c]], ids=lambda v: str(v).replace(" ", ""))
def test_gmlp_kernel_alone(benign, C, shape, shift):
    """The maps with a second grid-stride trip run WITHOUT taps: that is the instance of the kernel the forward launches."""
    sd, m = benign
    B, H, W = shape
    x = R.gmlp_input(100 + C + H, B, H, W, C)
    print()
    assert_gmlp(measure_gmlp(sd, m, GMLP_BLOCK[C], x, shift, with_taps=H * W * B <= 4096),
                f"gmlp C={C} {shape} {'shifted' if shift else 'plain'}")


def gelu_tail_case(block):
    from nunif_amd import synthetic
    sd = R.gelu_tail_weights(synthetic.wgmlp_state_dict(SEED), R.block_prefixes()[block])
    return sd, make_model(sd)


@pytest.mark.parametrize("block,C", [(0, 128), (3, 256)])
def test_gmlp_kernel_gelu_tail(block, C):
    """The kernel's GELU in the far negative tail (``wgmlp_ref.gelu_tail_weights``: pre-activations in [-3.9, -3.5]), where the erf
    form and the tanh approximation differ by 12 x the tap bound (tests/test_wgmlp_cpu.py): the ``gelu`` tap, the taps before and
    after it and the output, shifted windows, same limits."""
    sd, m = gelu_tail_case(block)
    print()
    assert_gmlp(measure_gmlp(sd, m, block, R.gmlp_input(7, 1, 16, 24, C), True, with_taps=True), f"gmlp C={C} gelu tail")


# windows of the levels in output pixels: 8 level-1 tokens = 32 pixels, 8 level-2 tokens = 64; the output starts 1 token (4 pixels) in
NET_CELLS = [(32, (-4) % 32), (64, (-4) % 64)]


def measure_net(sd, m, tile, batch):
    """{"out": stats of the image, block prefix: stats of its tap}"""
    x = R.test_input(INPUT_SEED + tile + batch, batch, tile)
    with torch.inference_mode():
        errloc.set_threads()
        y, taps = m.engine().debug_taps(x.to("cuda:0"))
        assert torch.equal(y, m(x.to("cuda:0")))              # the debug entry runs the same launches
        t64, te = {}, {}
        y64, ye = R.forward64(sd, x, taps=t64), R.emulated(sd, x, taps=te)
    out = {"out": errloc.localised_stats(y.cpu(), y64, ye, NET_CELLS, errloc.B_OUT, errloc.TAU_OUT)}
    for p in R.block_prefixes():
        rms = float(t64[p].pow(2).mean().sqrt())
        out[p] = errloc.localised_stats(errloc.nhwc(taps[p].cpu()), errloc.nhwc(t64[p]), errloc.nhwc(te[p]), [(8, 0)], errloc.B_TAP,
                                        errloc.TAP_TAU_REL * rms)
    return out


@pytest.mark.parametrize("regime", ["benign", "hot"])
@pytest.mark.parametrize("tile,batch", [(64, 1), (64, 3), (112, 1), (112, 3)])
def test_net_localised(benign, hot, tile, batch, regime):
    sd, m = benign if regime == "benign" else hot
    print()
    assert_gmlp(measure_net(sd, m, tile, batch), f"wgmlp_4x tile {tile} batch {batch} {regime}")


def test_psnr_against_the_fixture(benign):
    sd, m = benign
    g = np.load(os.path.join(GOLDEN, "wgmlp.npz"))
    with torch.inference_mode():
        y = m(torch.from_numpy(g["x"]).to("cuda:0")).cpu()
    for got, ref in ((y[0], g["raw0"]), (y[1, :, :96, :96], g["raw1"])):
        psnr = errloc.psnr_db(got, torch.from_numpy(ref).clamp(0, 1))
        print(f"\nwgmlp_4x vs the reference's own class: {psnr:.2f} dB")
        assert psnr >= 50.0, psnr


def test_invariants(benign):
    sd, m = benign
    x = R.test_input(9, 3, 64).to("cuda:0")
    with torch.inference_mode():
        y = m(x)
        for b in range(3):
            assert torch.equal(y[b:b + 1], m(x[b:b + 1])), b           # image b of a batch == alone
        assert torch.equal(y, m(x))                                    # two calls
        s = torch.cuda.Stream()
        s.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(s):
            y2 = m(x)
        s.synchronize()
        assert torch.equal(y, y2)                                      # two streams
        raw = m.engine().forward(x, clamp=False)
        assert torch.equal(y, raw.clamp(0, 1)) and float(raw.min()) < 0.0 and float(raw.max()) > 1.0      # the clamp acts on both sides
        with pytest.raises((ValueError, RuntimeError)):
            m(torch.zeros(1, 3, 72, 72, device="cuda:0"))              # (72 - 16) % 48 != 0


def test_tiled_render_matches_the_restatement(benign):
    from nunif_amd.nunif.utils.render import tiled_render
    from oracle import seam_blending as OS
    sd, m = benign
    g = torch.Generator().manual_seed(4)
    img = torch.nn.functional.interpolate(torch.rand(1, 3, 27, 35, generator=g), size=(200, 264), mode="bicubic").clamp(0, 1)[0]
    with torch.inference_mode():
        errloc.set_threads()
        y1 = tiled_render(img, m, tile_size=64, batch_size=1).cpu()
        y4 = tiled_render(img, m, tile_size=64, batch_size=4).cpu()
        ref = OS.tiled_render(img, lambda mb: R.forward(sd, mb), 4, 36, 16, 64, 4)
    assert torch.equal(y1, y4)
    psnr = errloc.psnr_db(y4, ref)
    print(f"\nwgmlp_4x tiled_render 200 x 264: {psnr:.2f} dB")
    assert y4.shape == ref.shape == (3, 800, 1056) and psnr >= 50.0, psnr
