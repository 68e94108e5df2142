"""Records tests/golden/zoedepth.npz:

* ``head_*``: HuggingFace transformers' ``ZoeDepthMetricDepthEstimationHead`` in float64 (and float32, the yardstick) on the seeded
  weights of ``nunif_amd.synthetic.zoedepth_head_state_dict`` and the seeded maps of ``tests/zoedepth_ref.random_inputs`` —
  only seeds, shapes and outputs are stored;
* ``prep_*``: the reference's own ``iw3.zoedepth_model.batch_preprocess`` (imported through ``oracle.refstub``: the module needs
  torchvision only for PIL inputs) on seeded frames — landscape 1080 x 1920, portrait, a frame smaller than the target, and small
  frames whose pad meets or exceeds what one reflection can give.

Run from the repository root with the reference tree mounted:  python tests/golden/make_golden_zoedepth.py
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

HEAD_SEED = 4100
HEAD_CASES = [(1, 2, 3), (2, 4, 6), (1, 3, 5), (2, 3, 5)]                # (B, bottleneck h, w)
PREP_CASES = [("landscape", 1, 1080, 1920), ("portrait", 1, 1280, 720), ("small", 2, 200, 300), ("tiny", 1, 20, 30),
              ("tiny_portrait", 1, 30, 20), ("narrow", 1, 60, 14)]     # (name, B, H, W); 30 x 20: pad_w 10 > 8 columns; 60 x 14: 24 > 8


def hf_head(dtype):
    from transformers import ZoeDepthConfig
    from transformers.models.zoedepth.modeling_zoedepth import ZoeDepthMetricDepthEstimationHead
    from nunif_amd.synthetic import zoedepth_head_state_dict
    cfg = ZoeDepthConfig(bin_configurations=[{"n_bins": 64, "min_depth": 1e-3, "max_depth": 10.0, "name": "nyu"}])
    head = ZoeDepthMetricDepthEstimationHead(cfg).to(dtype).eval()
    head.load_state_dict({k: v.to(dtype) for k, v in zoedepth_head_state_dict(HEAD_SEED, prefix="").items()}, strict=True)
    return head


def frame(seed, B, H, W):
    g = torch.Generator().manual_seed(seed)
    lo = torch.rand((B, 3, max(2, H // 16), max(2, W // 16)), generator=g)
    x = torch.nn.functional.interpolate(lo, size=(H, W), mode="bicubic", align_corners=False) * 1.2 - 0.1      # leaves [0, 1]: the clamp bites
    return (x + torch.rand((B, 3, H, W), generator=g) * 0.05).float()


def main():
    import zoedepth_ref as R
    out = {"head_seed": np.int64(HEAD_SEED), "head_cases": np.array(HEAD_CASES, dtype=np.int64)}
    with torch.inference_mode():
        h64, h32 = hf_head(torch.float64), hf_head(torch.float32)
        for i, (B, bh, bw) in enumerate(HEAD_CASES):
            oc, bt, blocks, rel = R.random_inputs(HEAD_SEED + 10 + i, B, bh, bw)
            y64 = h64(oc.double(), bt.double(), [b.double() for b in blocks], rel.double())[0]
            y32 = h32(oc, bt, blocks, rel)[0]
            out[f"head_{i}_f64"] = y64.numpy()
            if B == 1:                                      # the yardstick on the two single-image cases (file size)
                out[f"head_{i}_f32"] = y32.numpy()
        from oracle import refstub
        refstub.install()
        from iw3.zoedepth_model import batch_preprocess
        out["prep_names"] = np.array([c[0] for c in PREP_CASES])
        out["prep_shapes"] = np.array([c[1:] for c in PREP_CASES], dtype=np.int64)
        for i, (name, B, H, W) in enumerate(PREP_CASES):
            x = frame(4200 + i, B, H, W)
            y, pad_h, pad_w = batch_preprocess(x.clone(), h_height=392, v_height=518, ensure_multiple_of=14)
            out[f"prep_{i}_pads"] = np.array([pad_h, pad_w], dtype=np.int64)
            out[f"prep_{i}_shape"] = np.array(y.shape, dtype=np.int64)
            # whole maps of the small cases; of the large ones two corners that hold the pad, and a checksum
            if y.numel() <= 40000:
                out[f"prep_{i}_y"] = y.numpy()
            else:
                out[f"prep_{i}_tl"] = y[:, :, :pad_h + 8, :pad_w + 8].numpy().astype(np.float32)
                out[f"prep_{i}_br"] = y[:, :, -pad_h - 8:, -pad_w - 8:].numpy().astype(np.float32)
                out[f"prep_{i}_sum"] = np.float64(y.double().sum().item())
                # and every 64th row and column from 3 on: whole lines through all four pads and the interior
                out[f"prep_{i}_rows"] = y[:, :, 3::64].numpy().astype(np.float32)
                out[f"prep_{i}_cols"] = y[:, :, :, 3::64].numpy().astype(np.float32)
    np.savez_compressed(os.path.join(HERE, "zoedepth.npz"), **out)
    print("wrote zoedepth.npz", {k: getattr(v, "shape", None) for k, v in out.items()})


if __name__ == "__main__":
    main()
