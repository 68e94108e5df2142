"""The HDR -> SDR tone mapping of ``nunif/utils/video.py`` ``hdr2sdr`` (:325-398) restated in torch, for the tests of
``nunif_amd/csrc/hdr.hip``: once in float64 (the truth) and once in fp32 with the reference's operation order (whose distance to the
truth is the yardstick for the kernel's), the seeded inputs of the cases, and stand-ins for the two PyAV objects the function
touches.  Nothing here runs on the product path."""
import sys
import types

import numpy as np
import torch

PQ, HLG = 16, 18
H, W = 32, 48
DEFAULTS = dict(pq_exposure=110.0, pq_white_point=5.0, hlg_exposure=1.2, hlg_white_point=0.8, hlg_saturation_gain=0.9)
MATRICES = {
    "bt709": [[1.6605, -0.5876, -0.0728], [-0.1246, 1.1329, -0.0083], [-0.0182, -0.1006, 1.1187]],
    "bt601": [[1.5540, -0.5143, -0.0397], [-0.1017, 1.1147, -0.0130], [-0.0163, -0.0886, 1.1049]],
}
INPUTS = ("noise", "dark", "ramp")
# name -> (input, trc, colorspace, non-default parameters); the fixture tests/golden/hdr2sdr.npz holds one uint16 frame per name
CASES = {f"{inp}_{'pq' if trc == PQ else 'hlg'}_{cs}": (inp, trc, cs, {})
         for inp in INPUTS for trc in (PQ, HLG) for cs in ("bt709", "bt601")}
CASES.update({
    "noise_hlg_bt709_gain1": ("noise", HLG, "bt709", {"hlg_saturation_gain": 1.0}),
    "noise_hlg_bt601_gain05": ("noise", HLG, "bt601", {"hlg_saturation_gain": 0.5}),
    "noise_pq_bt709_exp60_white3": ("noise", PQ, "bt709", {"pq_exposure": 60.0, "pq_white_point": 3.0}),
})


def make_input(name, h=H, w=W):
    """uint16 [h, w, 3]: full-range noise, noise below code 4096, or a grey ramp 0..65535 with a small offset per channel."""
    if name == "noise":
        return np.random.default_rng(2084).integers(0, 65536, size=(h, w, 3)).astype(np.uint16)
    if name == "dark":
        return np.random.default_rng(67).integers(0, 4096, size=(h, w, 3)).astype(np.uint16)
    if name == "ramp":
        grey = np.rint(np.linspace(0, 65535, h * w)).astype(np.int64).reshape(h, w, 1)
        return np.clip(grey + np.array([0, 37, -53]), 0, 65535).astype(np.uint16)
    raise KeyError(name)


def _hable(v, E):
    A, B, C, D, F = 0.15, 0.50, 0.10, 0.20, 0.30
    return ((v * (A * v + C * B) + D * E) / (v * (A * v + B) + D * F)) - E / F


def constants(trc, colorspace, dtype=torch.float32, device="cpu", **params):
    """(matrix [3, 3], hable_map(white point)) as tensors of ``dtype``."""
    p = dict(DEFAULTS, **params)
    white = p["pq_white_point"] if trc == PQ else p["hlg_white_point"]
    return (torch.tensor(MATRICES[colorspace], dtype=dtype, device=device),
            _hable(torch.tensor(white, dtype=dtype, device=device), 0.02 if trc == PQ else 0.01))


def hdr2sdr_ref(rgb48, trc, colorspace, dtype=torch.float32, device="cpu", **params):
    """``rgb48`` uint16 [H, W, 3] -> (the value before ``* 65535`` as [H, W, 3] of ``dtype`` on ``device``, the uint16 frame
    [H, W, 3] on the host).  ``device``: where the passes run (tools/time_hdr2sdr.py times this function as the eager route: upload, the passes,
    download of the 16-bit frame)."""
    p = dict(DEFAULTS, **params)
    codes = torch.from_numpy(rgb48.view(np.int16)).to(device)
    x = (codes.to(torch.int32) & 0xFFFF).to(dtype).permute(2, 0, 1) / 65535.0
    if trc == PQ:
        m1, m2 = 2610 / 16384, 2523 / 4096 * 128
        c1, c2, c3 = 3424 / 4096, 2413 / 4096 * 32, 2392 / 4096 * 32
        xp = torch.pow(x, 1.0 / m2)
        linear = torch.pow(torch.clamp(xp - c1, min=0) / (c2 - c3 * xp), 1.0 / m1)
        exposure, E = p["pq_exposure"], 0.02
    else:
        a, b, c = 0.17883277, 0.28466892, 0.55991073
        linear = torch.where(x <= 0.5, torch.pow(x, 2.0) / 3.0, (torch.exp((x - c) / a) + b) / 12.0)
        exposure, E = p["hlg_exposure"], 0.01
    matrix, white = constants(trc, colorspace, dtype, device, **params)
    sdr = _hable(linear * exposure, E) / white
    if trc == HLG and p["hlg_saturation_gain"] < 1.0:
        gain = p["hlg_saturation_gain"]
        luma = sdr[0] * 0.2126 + sdr[1] * 0.7152 + sdr[2] * 0.0722
        sdr = (sdr * gain) + (luma * (1.0 - gain))
    ch, h, w = sdr.shape
    out = torch.clamp(torch.mm(matrix, sdr.reshape(ch, -1)).reshape(ch, h, w), 0, 1)
    gamma = torch.where(out < 0.018, out * 4.5, 1.099 * torch.pow(out, 0.45) - 0.099).clamp(0, 1)
    u16 = (gamma * 65535).to(torch.int32).to(torch.int16).cpu().permute(1, 2, 0).contiguous().numpy().view(np.uint16)
    return gamma.permute(1, 2, 0), u16


def brightest_band(rgb48):
    """[H, W] int: which of 16 equal bands of 4096 codes the pixel's brightest input code falls into."""
    return rgb48.max(axis=2).astype(np.int64) // 4096


# ---- stand-ins for PyAV ---------------------------------------------------------------------------------------------------
class FakeFrame:
    """What ``hdr2sdr`` reads of an ``av.VideoFrame``: ``to_ndarray``, ``colorspace``, ``color_range`` and the timing fields."""
    colorspace = 9                       # BT.2020
    color_range = 1

    def __init__(self, rgb48, pts=1234, dts=1230, time_base=(1, 24000), opaque="opaque-object"):
        self.rgb48, self.pts, self.dts, self.time_base, self.opaque = rgb48, pts, dts, time_base, opaque
        self.to_ndarray_kwargs = None

    def to_ndarray(self, **kwargs):
        self.to_ndarray_kwargs = kwargs
        return self.rgb48.copy()


class RecordingVideoFrame:
    """``av.video.frame.VideoFrame``: ``from_ndarray`` keeps a copy of the array (PyAV copies it into the frame's planes)."""

    @classmethod
    def from_ndarray(cls, array, format=None):
        f = cls()
        f.array, f.format = np.array(array, copy=True), format
        return f


def fake_av_modules():
    """{module name: module} of a minimal ``av`` for ``sys.modules`` on a machine without PyAV."""
    av = types.ModuleType("av")
    video = types.ModuleType("av.video")
    frame = types.ModuleType("av.video.frame")
    reformatter = types.ModuleType("av.video.reformatter")
    frame.VideoFrame = RecordingVideoFrame
    reformatter.ColorRange = types.SimpleNamespace(MPEG=1, JPEG=2)
    reformatter.Colorspace = types.SimpleNamespace(ITU709=1, ITU601=5)
    av.video, video.frame, video.reformatter = video, frame, reformatter
    return {"av": av, "av.video": video, "av.video.frame": frame, "av.video.reformatter": reformatter}


def reference_hdr2sdr_recording():
    """The live reference's ``hdr2sdr`` (through ``oracle/refstub.py``) with ``RecordingVideoFrame`` on its stubbed
    ``av.video.frame``.  Only where the reference is mounted."""
    from oracle import refstub
    refstub.install()
    import importlib
    importlib.import_module("av.video.frame")
    sys.modules["av.video.frame"].VideoFrame = RecordingVideoFrame
    sys.modules["av"].video = sys.modules["av.video"]
    sys.modules["av.video"].frame = sys.modules["av.video.frame"]
    import nunif.utils.video as VU
    return VU
