"""Records tests/golden/da3_disparity.npz from the live reference on the CPU in fp32: ``_forward`` of
``iw3/depth_anything_v3_model.py`` around a stand-in ``model`` that answers recorded arrays, ``DA3MonoDisparity.extract_features`` and a
seeded ``DA3MonoDisparity.forward``.  Arrays only: inputs, outputs, the ``ranks`` of every n, the seeded state dict.

    python tests/golden/make_golden_da3.py        (needs the reference tree, see oracle/refstub.py)
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import da3_ref as R  # noqa: E402
from oracle import refstub  # noqa: E402

SEED = 20
COUNT_CASES = ((0, 0), (9, 0), (9, 1), (11, 0))          # (pixels below the threshold, pixels on it) of four 8 x 8 images
RAW_COUNTS = (1, 2, 100, 101)                            # non-sky pixels of four 37 x 53 images


def count_skies():
    return torch.cat([R.sky_map(1, 8, 8, seed=30 + i, n_clear=c, on_threshold=t) for i, (c, t) in enumerate(COUNT_CASES)])


def raw_count_skies():
    return torch.cat([R.sky_map(1, 37, 53, seed=40 + i, n_clear=c) for i, c in enumerate(RAW_COUNTS)])


def main():
    refstub.install()
    from iw3.depth_anything_v3_model import _forward
    from iw3.models.da3mono_disparity import DA3MonoDisparity

    def ref_stage(depth, sky, raw):
        model = lambda x: {"depth": depth, "sky": sky}       # noqa: E731
        with torch.inference_mode():
            return _forward(model, torch.zeros(depth.shape[0], 3, 14, 14), False, raw_output=raw)

    out = {"seed": np.int64(SEED)}
    for i, (B, H, W) in enumerate(R.SHAPES):
        depth, sky = R.depth_map("noise", B, H, W, SEED), R.sky_map(B, H, W, SEED)
        out[f"stage_{i}_depth"], out[f"stage_{i}_sky"] = depth.numpy(), sky.numpy()
        out[f"stage_{i}_out"] = ref_stage(depth, sky, False).numpy()
        out[f"stage_{i}_raw"] = ref_stage(depth, sky, True).numpy()
        out[f"ranks_{H * W}"] = torch.linspace(1, H * W - 2, 62, device="cpu").long().numpy()
    depth, sky = R.depth_map("noise", 4, 8, 8, SEED + 1), count_skies()
    out["count_depth"], out["count_sky"], out["count_out"] = depth.numpy(), sky.numpy(), ref_stage(depth, sky, False).numpy()
    depth, sky = R.depth_map("noise", 4, 37, 53, SEED + 2), raw_count_skies()
    out["rawcount_depth"], out["rawcount_sky"], out["rawcount_out"] = depth.numpy(), sky.numpy(), ref_stage(depth, sky, True).numpy()

    sd = R.seeded_state_dict(SEED)
    net = DA3MonoDisparity().eval()
    net.load_state_dict(sd, strict=True)
    for k, v in sd.items():
        out["sd_" + k] = v.numpy()
    with torch.inference_mode():
        for i, (B, H, W) in enumerate(R.SHAPES):
            for kind in R.KINDS:
                x = R.depth_map(kind, B, H, W, SEED)
                out[f"x_{i}_{kind}"] = x.numpy()
                out[f"feat_{i}_{kind}"] = DA3MonoDisparity.extract_features(x).numpy()
                if kind in ("noise", "ramp_ties"):
                    out[f"fwd_{i}_{kind}"] = net(x).numpy()
                    if B == 1:
                        out[f"fwd3d_{i}_{kind}"] = net(x[0]).numpy()
    path = os.path.join(HERE, "da3_disparity.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes,", len(out), "arrays")


if __name__ == "__main__":
    main()
