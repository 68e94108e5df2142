"""What the fused HDR planar entry (nunif_amd/csrc/hdr_planes.hip) promises on a host without a GPU: the signatures, the refusals
of the Python layers and of the C ABI (nothing is launched for a refused argument), the conditions on the seeded inputs that make
a green tests/test_gpu_hdr_planes.py mean something, and that the restatement's composition adds nothing to the pinned map."""
import ctypes
import inspect
import os
import types

import numpy as np
import pytest
import torch

import hdr_planes_ref as R
import hdr_ref
from conftest import GOLDEN


@pytest.fixture(scope="module")
def hdr(hiplib):
    from nunif_amd.nunif.utils import hdr
    return hdr


@pytest.fixture(scope="module")
def pixfmt(hiplib):
    from nunif_amd.nunif.utils import pixfmt
    return pixfmt


# ---- signatures -----------------------------------------------------------------------------------------------------------
def test_signatures(hdr):
    from nunif_amd.iw3.frame_pipeline import PipelineOps
    p = inspect.signature(hdr.hdr2sdr_planes).parameters
    assert list(p)[:5] == ["planes", "layout", "full_range", "color_trc", "output_colorspace"]
    assert p["form"].default == "chw" and p["out"].default is None and p["device"].default is None
    assert all(p[n].kind is inspect.Parameter.KEYWORD_ONLY for n in ("form", "out", "device"))
    assert p["params"].kind is inspect.Parameter.VAR_KEYWORD
    e = inspect.signature(hdr.hdr_yuv_entry).parameters
    assert list(e)[:4] == ["layout", "full_range", "color_trc", "output_colorspace"] and e["params"].kind is inspect.Parameter.VAR_KEYWORD
    assert inspect.signature(PipelineOps.__init__).parameters["hdr"].default is None


def test_hdr_entry_carries_what_the_planar_form_needs(hdr, pixfmt):
    entry = hdr.hdr_entry(R.HLG, "bt601", hlg_saturation_gain=0.5)
    assert (entry.color_trc, entry.output_colorspace, entry.params) == (R.HLG, "bt601", {"hlg_saturation_gain": 0.5})
    lay = pixfmt.PlaneLayout(R.FMT, 96, 64)
    planar = hdr.hdr_yuv_entry(lay, True, entry.color_trc, entry.output_colorspace, **entry.params)
    assert (planar.layout, planar.matrix, planar.full_range) == (lay, "bt2020", True)
    assert (planar.color_trc, planar.output_colorspace, planar.params) == (R.HLG, "bt601", {"hlg_saturation_gain": 0.5})


# ---- refusals of the Python layers ----------------------------------------------------------------------------------------
def test_hdr2sdr_planes_refusals(hdr, pixfmt):
    lay = pixfmt.PlaneLayout(R.FMT, 16, 8)
    buf = torch.zeros(lay.nbytes, dtype=torch.uint8)
    for fmt in ("yuv420p", "yuv444p"):
        other = pixfmt.PlaneLayout(fmt, 16, 8)
        with pytest.raises(ValueError, match="yuv420p10le"):
            hdr.hdr2sdr_planes(torch.zeros(other.nbytes, dtype=torch.uint8), other, False, R.PQ, "bt709")
        with pytest.raises(ValueError, match="yuv420p10le"):
            hdr.hdr_yuv_entry(other, False, R.PQ, "bt709")
    with pytest.raises(ValueError, match="color_trc"):
        hdr.hdr2sdr_planes(buf, lay, False, 17, "bt709")
    with pytest.raises(ValueError, match="output_colorspace"):
        hdr.hdr2sdr_planes(buf, lay, False, R.PQ, "bt2020")
    with pytest.raises(ValueError, match="form"):
        hdr.hdr2sdr_planes(buf, lay, False, R.PQ, "bt709", form="hwc")
    with pytest.raises(ValueError, match="nbytes"):
        hdr.hdr2sdr_planes(buf[:-1], lay, False, R.PQ, "bt709")
    with pytest.raises(ValueError, match="nbytes"):
        hdr.hdr2sdr_planes(buf.view(torch.int16), lay, False, R.PQ, "bt709")
    with pytest.raises(TypeError, match="pq_exposition"):
        hdr.hdr2sdr_planes(buf, lay, False, R.PQ, "bt709", pq_exposition=1.0)
    with pytest.raises(TypeError, match="pq_exposition"):
        hdr.hdr_yuv_entry(lay, False, R.PQ, "bt709", pq_exposition=1.0)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        hdr.hdr2sdr_planes(buf, lay, False, R.PQ, "bt709")                           # host memory that is not pinned
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        hdr.hdr2sdr_planes(buf, lay, False, R.PQ, "bt709", device="cuda:0")


def test_stream_accepts_the_one_planar_hdr_form_and_refuses_the_others(hdr):
    from nunif_amd.waifu2x.video import Waifu2xVideoStream
    ctx, args = types.SimpleNamespace(device="cuda:0"), types.SimpleNamespace(pix_fmt="yuv420p10le")
    entry = hdr.hdr_entry(R.PQ, "bt709")
    s = Waifu2xVideoStream(ctx, args, in_format="yuv420p10le", in_matrix="bt2020", hdr=entry)
    assert (s.in_format, s.in_matrix, s.hdr) == ("yuv420p10le", "bt2020", entry)
    accepted = "in_format='yuv420p10le', in_matrix='bt2020'"
    for kw in (dict(in_format="yuv420p", in_matrix="bt2020"), dict(in_format="yuv444p", in_matrix="bt2020"),     # another format
               dict(in_format="yuv420p10le", in_matrix="bt709"), dict(in_format="yuv420p10le")):                  # another matrix
        with pytest.raises(ValueError, match=accepted):
            Waifu2xVideoStream(ctx, args, hdr=entry, **kw)
    with pytest.raises(ValueError, match=accepted):                                  # a bare callable: nothing to build the entry from
        Waifu2xVideoStream(ctx, args, in_format="yuv420p10le", in_matrix="bt2020", hdr=lambda hwc, device=None: None)
    with pytest.raises(ValueError, match="rotate"):                                  # HDR with a quarter turn stays refused
        Waifu2xVideoStream(ctx, types.SimpleNamespace(pix_fmt="yuv420p10le", rotate_left=True), in_format="yuv420p10le",
                           in_matrix="bt2020", hdr=entry)


def test_pipeline_ops_hdr_is_valid_with_the_planar_hdr_form_only(hdr):
    from nunif_amd.iw3.frame_pipeline import PipelineOps
    entry = hdr.hdr_entry(R.HLG, "bt601")
    ops = PipelineOps(in_format="yuv420p10le", in_matrix="bt2020", hdr=entry)
    assert ops.hdr is entry and PipelineOps().hdr is None
    accepted = "in_format='yuv420p10le', in_matrix='bt2020'"
    for kw in (dict(in_format="yuv420p", in_matrix="bt2020"), dict(in_format="yuv420p10le", in_matrix="bt709"), dict(),
               dict(to_tensor=lambda f, device=None: f)):
        with pytest.raises(ValueError, match=accepted):
            PipelineOps(hdr=entry, **kw)
    with pytest.raises(ValueError, match=accepted):
        PipelineOps(in_format="yuv420p10le", in_matrix="bt2020", hdr=lambda hwc, device=None: None)


# ---- the C ABI's argument checks: EINVAL, nothing launched ------------------------------------------------------------------
def test_abi_refuses_what_it_does_not_cover(hiplib, pixfmt):
    from nunif_amd import _hip
    lay = pixfmt.PlaneLayout(R.FMT, 16, 8)
    buf, dst = torch.zeros(lay.nbytes, dtype=torch.uint8), torch.zeros((3, 8, 16))
    planes, params = lay._c_planes(buf), _hip.Hdr2SdrParams(110.0, 5.0, 0.9)

    def call(fmt=2, h=8, w=16, full=0, trc=16, cs=709, form=1, p=planes, prm=params, out=dst):
        return hiplib.nunif_hip_yuv_hdr_to_tensor(ctypes.byref(p) if p is not None else None, fmt, h, w, full, trc, cs,
                                                  ctypes.byref(prm) if prm is not None else None, form,
                                                  ctypes.c_void_p(out.data_ptr()) if out is not None else None, None)
    assert call(fmt=0) == -1 and call(fmt=1) == -1 and call(fmt=3) == -1
    assert call(trc=17) == -1 and call(cs=2020) == -1 and call(full=2) == -1
    assert call(h=0) == -1 and call(w=0) == -1 and call(h=8193) == -1 and call(w=8193) == -1
    assert call(form=3) == -1 and call(form=-1) == -1
    assert call(p=None) == -1 and call(prm=None) == -1 and call(out=None) == -1
    for i in range(3):
        null = lay._c_planes(buf)
        null.data[i] = None
        assert call(p=null) == -1
        short = lay._c_planes(buf)
        short.pitch[i] = (32 if i == 0 else 16) - 2                                  # one sample short of the row
        assert call(p=short) == -1
    assert b"yuv_hdr_to_tensor" in hiplib.nunif_hip_last_error()


# ---- conditions on the inputs -----------------------------------------------------------------------------------------------
def test_case_table():
    assert R.SHAPES == [(2, 2), (1, 1), (5, 7), (16, 8), (18, 33), (64, 96), (8, 8192), (8192, 2)]
    assert len(R.AXES) == 8 and len(R.CASES) == 64 and len(set(R.IDS)) == 64
    for shape in R.SHAPES:
        assert {m for s, _, m in R.CASES if s == shape} == set(R.PITCH_MODES)
    for axis in R.AXES:
        assert {m for _, a, m in R.CASES if a == axis} == set(R.PITCH_MODES)


def test_ramp_sweeps_the_whole_curve():
    planes = R.make_planes("ramp", 64, 96)
    assert set(np.unique(planes[0])) == set(range(1024)) and planes[1][0, 0] == 512
    for full in (False, True):
        codes = R.rgb48_codes(planes, full)
        top = codes[:31]                                      # neutral chroma (row 31 already blends with the lower half): r = g = b
        assert np.array_equal(top[..., 0], top[..., 1]) and np.array_equal(top[..., 0], top[..., 2])
        for c in range(3):
            distinct = np.unique(codes[..., c])
            print(f"ramp full_range={full} channel {c}: {distinct.size} distinct codes")
            assert distinct[0] == 0 and distinct[-1] == 65535 and distinct.size >= 1000


def test_wild_clamps_at_both_ends():
    import pixfmt_ref as P
    planes = R.make_planes("wild", 64, 96)
    for full in (False, True):
        v = P.yuv_to_rgb(planes, R.FMT, R.MATRIX, full, torch.float32)
        low, high = float((v < 0).float().mean()), float((v > 1).float().mean())
        print(f"wild full_range={full}: {100 * low:.1f} % below 0, {100 * high:.1f} % above 1")
        assert low >= 0.01 and high >= 0.01
        codes = R.rgb48_codes(planes, full)
        assert (codes == 0).mean() >= 0.01 and (codes == 65535).mean() >= 0.01


def test_noise_takes_both_branches_of_the_hlg_curve():
    for full in (False, True):
        x = R.rgb48_codes(R.make_planes("noise", 64, 96), full).astype(np.float32) / np.float32(65535.0)
        share = float((x <= 0.5).mean())
        print(f"noise full_range={full}: {100 * share:.1f} % of the samples on the x <= 0.5 branch")
        assert 0.10 <= share <= 0.90


# ---- the composition adds nothing to the pinned map ---------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(hdr_ref.CASES))
def test_step_three_alone_reproduces_the_reference_fixture(name):
    """The restatement's third step IS hdr_ref.hdr2sdr_ref: fed the fixture's rgb48 frames as the codes of step 2, it returns the
    live reference's integers."""
    fixture = np.load(os.path.join(GOLDEN, "hdr2sdr.npz"))
    inp, trc, cs, params = hdr_ref.CASES[name]
    codes = hdr_ref.make_input(inp)
    _, u16 = R.H.hdr2sdr_ref(codes, trc, cs, torch.float32, **params)
    assert np.array_equal(u16, fixture[name])


def test_restatement_is_its_three_steps():
    import pixfmt_ref as P
    planes = R.make_planes("noise", 18, 33)
    v, u16, codes = R.hdr_planes_ref(planes, False, R.PQ, "bt709", torch.float32)
    rgb = P.yuv_to_rgb(planes, "yuv420p10le", "bt2020", False, torch.float32, clamp=True)
    want = torch.round(rgb * 65535).permute(1, 2, 0).numpy().astype(np.uint16)
    assert np.array_equal(codes, want) and codes.dtype == np.uint16 and codes.shape == (18, 33, 3)
    assert v.shape == (18, 33, 3) and v.dtype == torch.float32 and u16.shape == (18, 33, 3) and u16.dtype == np.uint16
    v64, _, codes64 = R.hdr_planes_ref(planes, False, R.PQ, "bt709", torch.float64)
    assert v64.dtype == torch.float64 and np.array_equal(codes64, codes)           # the codes are the fp32 ones whatever step 3 runs in
