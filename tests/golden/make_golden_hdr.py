"""Writes tests/golden/hdr2sdr.npz: the uint16 frames that the LIVE reference's ``hdr2sdr`` (nunif/utils/video.py:309-416) returns
for the cases of tests/hdr_ref.py, on the CPU.  Runs only where the reference is mounted (imported through oracle/refstub.py, with a
stand-in frame and a recording ``av.video.frame.VideoFrame``); inputs are regenerated from their seeds by the tests, so the fixture
holds the recorded outputs alone.  ``python tests/golden/make_golden_hdr.py``"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
import hdr_ref  # noqa: E402


def main():
    VU = hdr_ref.reference_hdr2sdr_recording()
    out = {}
    for name, (inp, trc, cs, params) in hdr_ref.CASES.items():
        frame = hdr_ref.FakeFrame(hdr_ref.make_input(inp))
        got = VU.hdr2sdr(frame, trc, cs, device="cpu", **params)
        assert isinstance(got, hdr_ref.RecordingVideoFrame) and got.format == "rgb48le" and got.pts == frame.pts
        assert got.array.dtype == np.uint16 and got.array.shape == (hdr_ref.H, hdr_ref.W, 3)
        out[name] = got.array
    path = os.path.join(HERE, "hdr2sdr.npz")
    np.savez_compressed(path, **out)
    print(f"wrote {path}: {len(out)} cases, {os.path.getsize(path)} bytes")


if __name__ == "__main__":
    main()
