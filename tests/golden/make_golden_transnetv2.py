"""Writes tests/golden/transnetv2.npz from the LIVE reference (run once where the reference checkout is mounted:
``python tests/golden/make_golden_transnetv2.py``).  Numeric arrays only; the 7.6 M weights are regenerated from the seed.

(a) ``a/<case>/one_hot``, ``a/<case>/many_hot``: the reference CLASS ``nunif.utils.transnetv2.TransNetV2`` with
    ``nunif_amd.synthetic.transnetv2_state_dict(WEIGHT_SEED)``, fp32 on the CPU, for every case of
    ``tests/transnetv2_ref.FIXTURE_CASES``.
(b) ``b/<n>/windows`` [windows,100] frame indices, ``b/<n>/probs`` [windows,100] the sigmoid the reference thresholded,
    ``b/<n>/set`` the sorted result: the reference's ``detect_boundary`` itself over ``detect_clip(n)``, with a stand-in
    ``nunif.utils.video`` that plays the clip in batches of 25 (PyAV is not needed), pts = 1000 + 40 * index.
"""
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

from oracle import refstub  # noqa: E402
import transnetv2_ref as R  # noqa: E402
from nunif_amd.synthetic import transnetv2_state_dict  # noqa: E402


def pts_of(i):
    return 1000 + 40 * i


def fake_video_module(clips):
    m = types.ModuleType("nunif.utils.video")

    class VideoOutputConfig:
        def __init__(self, fps=None):
            self.fps = fps

    class FrameCallbackPool:
        def __init__(self, callback, require_pts=False, batch_size=1, device=None, max_workers=0):
            self.callback, self.batch_size = callback, batch_size

    def hook_frame(video_file, callback_pool, config_callback=None, **kwargs):
        config_callback(None)
        x = clips[video_file]
        for i in range(0, x.shape[0], callback_pool.batch_size):
            j = min(i + callback_pool.batch_size, x.shape[0])
            callback_pool.callback(x[i:j], [pts_of(k) for k in range(i, j)])

    m.VideoOutputConfig, m.FrameCallbackPool, m.hook_frame = VideoOutputConfig, FrameCallbackPool, hook_frame
    m.get_fps = lambda stream: 30
    return m


def main():
    torch.manual_seed(0)
    refstub.install()
    sd = transnetv2_state_dict(R.WEIGHT_SEED)
    out = {}

    from nunif.utils.transnetv2 import TransNetV2
    model = TransNetV2()
    model.load_state_dict(sd)
    model.eval()
    with torch.inference_mode():
        for name in R.FIXTURE_CASES:
            x = R.case_frames(name)
            one, extra = model(x)
            out[f"a/{name}/one_hot"] = one[..., 0].numpy().astype(np.float32)
            out[f"a/{name}/many_hot"] = extra["many_hot"][..., 0].numpy().astype(np.float32)
            print(name, tuple(one.shape))

    clips = {f"clip{n}": R.detect_clip(n) for n in R.DETECT_LENGTHS}
    sys.modules["nunif.utils.video"] = fake_video_module(clips)
    import nunif.utils as NU
    NU.video = sys.modules["nunif.utils.video"]
    import nunif.utils.shot_boundary_detection as SBD

    record = {}

    class Recording(TransNetV2):
        def load(self, map_location="cpu"):
            self.load_state_dict(sd)
            return self

        def forward(self, x):
            one, extra = super().forward(x)
            record["windows"].append([record["index"][x[i].numpy().tobytes()] for i in range(x.shape[0])])
            record["probs"].append(torch.sigmoid(one).flatten().numpy().astype(np.float32))
            return one, extra

    SBD.TransNetV2 = Recording
    for n in R.DETECT_LENGTHS:
        clip = clips[f"clip{n}"]
        record.update(windows=[], probs=[], index={clip[i].numpy().tobytes(): i for i in range(n)})
        assert len(record["index"]) == n, "frames of the detector clip must be pairwise distinct"
        result = SBD.detect_boundary(f"clip{n}", device="cpu")
        out[f"b/{n}/windows"] = np.asarray(record["windows"], dtype=np.int32)
        out[f"b/{n}/probs"] = np.stack(record["probs"])
        out[f"b/{n}/set"] = np.asarray(sorted(result), dtype=np.int64)
        print(n, out[f"b/{n}/windows"].shape, len(result))
    np.savez_compressed(os.path.join(HERE, "transnetv2.npz"), **out)


if __name__ == "__main__":
    main()
