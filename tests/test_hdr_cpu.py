"""HDR -> SDR tone mapping, the parts that need no GPU: the fp32 restatement of tests/hdr_ref.py reproduces the integers the live
reference returned (tests/golden/hdr2sdr.npz), the host-side constants of the C ABI are the restatement's bit for bit, the Python
signatures are the reference's, and the inputs cover what tests/test_gpu_hdr.py relies on."""
import inspect
import os
import struct

import numpy as np
import pytest
import torch

import hdr_ref as R
from conftest import GOLDEN
from oracle import refstub


@pytest.fixture(scope="module")
def fixture():
    return np.load(os.path.join(GOLDEN, "hdr2sdr.npz"))


def _bits(v):
    return struct.unpack("<I", struct.pack("<f", float(v)))[0]


def test_fixture_holds_every_case(fixture):
    assert sorted(fixture.files) == sorted(R.CASES)
    assert len([c for c in R.CASES.values() if not c[3]]) == 12
    for name in R.CASES:
        assert fixture[name].dtype == np.uint16 and fixture[name].shape == (R.H, R.W, 3)


@pytest.mark.parametrize("name", sorted(R.CASES))
def test_fp32_restatement_equals_the_reference_integers(fixture, name):
    inp, trc, cs, params = R.CASES[name]
    _, u16 = R.hdr2sdr_ref(R.make_input(inp), trc, cs, torch.float32, **params)
    assert np.array_equal(u16, fixture[name])


@pytest.mark.parametrize("trc", [R.PQ, R.HLG])
@pytest.mark.parametrize("cs", ["bt709", "bt601"])
@pytest.mark.parametrize("params", [{}, {"pq_exposure": 60.0, "pq_white_point": 3.0, "hlg_white_point": 0.65}])
def test_abi_constants_are_the_restatements_fp32(hiplib, trc, cs, params):
    from nunif_amd.nunif.utils import hdr
    matrix, white = hdr.constants(trc, cs, **params)
    ref_matrix, ref_white = R.constants(trc, cs, torch.float32, **params)
    assert [_bits(v) for v in matrix] == [_bits(v) for v in ref_matrix.reshape(-1).tolist()]
    assert _bits(white) == _bits(ref_white.item())


def test_abi_refuses_what_it_does_not_know(hiplib):
    import ctypes
    from nunif_amd import _hip
    from nunif_amd.nunif.utils import hdr
    p = _hip.Hdr2SdrParams(110.0, 5.0, 0.9)
    m, w = (ctypes.c_float * 9)(), ctypes.c_float()
    assert _hip.lib().nunif_hip_hdr2sdr_constants(17, 709, ctypes.byref(p), m, ctypes.byref(w)) == -1
    assert _hip.lib().nunif_hip_hdr2sdr_constants(16, 2020, ctypes.byref(p), m, ctypes.byref(w)) == -1
    with pytest.raises(ValueError):
        hdr.constants(1, "bt709")
    with pytest.raises(ValueError):
        hdr.constants(R.PQ, "bt2020")
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        hdr.hdr2sdr_tensor(torch.zeros((4, 4, 3), dtype=torch.int16), R.PQ, "bt709")


@pytest.mark.skipif(not refstub.reference_available(), reason="/root/reference is not mounted here")
def test_signatures_equal_the_live_reference():
    VU = R.reference_hdr2sdr_recording()
    import nunif_amd.install as inst
    ref = inst.original("nunif.utils.video", "hdr2sdr") or VU.hdr2sdr
    from nunif_amd.nunif.utils import hdr
    from nunif_amd.nunif.utils.video import hdr2sdr
    assert inspect.signature(ref) == inspect.signature(hdr2sdr)
    ours = inspect.signature(hdr.hdr2sdr_tensor).parameters
    for name, prm in list(inspect.signature(ref).parameters.items())[1:-1]:        # all but av_frame and device
        assert ours[name].default == prm.default, name
    assert (VU.COLOR_TRC_SMPTE2084, VU.COLOR_TRC_ARIB_STD_B67, VU.COLORSPACE_BT2020) == (R.PQ, R.HLG, R.FakeFrame.colorspace)


def test_inputs_cover_what_the_gpu_test_relies_on():
    inputs = {n: R.make_input(n) for n in R.INPUTS}
    bands = np.concatenate([R.brightest_band(x).reshape(-1) for x in inputs.values()])
    assert np.array_equal(np.unique(bands), np.arange(16))                        # every band of the brightest code occurs
    codes = np.concatenate([x.reshape(-1) for x in inputs.values()])
    assert (codes == 0).any() and (codes == 65535).any()
    assert (codes <= 32767).any() and (codes >= 32768).any()                      # both sides of HLG's x <= 0.5
    for trc in (R.PQ, R.HLG):
        toe = lo = hi = gamma = False
        for x in inputs.values():
            p = dict(R.DEFAULTS)
            xs = torch.from_numpy(x.astype(np.int32)).double().permute(2, 0, 1) / 65535.0
            # the value that enters the clamp in front of the OETF, in float64
            if trc == R.PQ:
                xp = xs ** (1.0 / (2523 / 4096 * 128))
                lin = (torch.clamp(xp - 3424 / 4096, min=0) / (2413 / 4096 * 32 - 2392 / 4096 * 32 * xp)) ** (16384 / 2610)
                sdr = R._hable(lin * p["pq_exposure"], 0.02) / R._hable(torch.tensor(p["pq_white_point"]).double(), 0.02)
            else:
                lin = torch.where(xs <= 0.5, xs ** 2 / 3.0, (torch.exp((xs - 0.55991073) / 0.17883277) + 0.28466892) / 12.0)
                sdr = R._hable(lin * p["hlg_exposure"], 0.01) / R._hable(torch.tensor(p["hlg_white_point"]).double(), 0.01)
                luma = sdr[0] * 0.2126 + sdr[1] * 0.7152 + sdr[2] * 0.0722
                sdr = sdr * 0.9 + luma * (1.0 - 0.9)
            m = torch.tensor(R.MATRICES["bt709"]).double() @ sdr.reshape(3, -1)
            lo, hi = lo or bool((m < 0).any()), hi or bool((m > 1).any())         # both clamps act
            toe = toe or bool(((m > 0) & (m < 0.018)).any())                      # the linear toe of the OETF
            gamma = gamma or bool(((m >= 0.018) & (m < 1)).any())                 # and its power segment
        assert toe and gamma and lo and hi, (trc, toe, gamma, lo, hi)
