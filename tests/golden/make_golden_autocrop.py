"""Writes tests/golden/autocrop.npz from the LIVE reference (run once where the reference checkout is mounted:
``python tests/golden/make_golden_autocrop.py``).  Results only: the frames are regenerated from their seeds by
``tests/autocrop_cases.py``.

From the reference CLASSES ``nunif.utils.autocrop.AutoCropDetector`` / ``AutoCrop`` on the CPU, fp32:
  ``<case>/<kind>/mask_tb`` [H], ``mask_lr`` [W]     ``detect_tb`` / ``detect_lr`` of every case of ``CASES`` (uint8), kind = black | flat
  ``batch/<kind>/mask_tb`` [3,H], ``mask_lr`` [3,W]  the same per frame of the batch
  ``<case>/<mode>/<mod>/slices`` [4]                 ``AutoCrop.from_image(...).get_slice()``: tb start, stop, lr start, stop; -1 = None
  ``<case>/<mode>/<mod>/pad`` [4], ``crop`` [4]      ``get_pad()``, ``get_crop()`` (x, y, width, height; all -1 = None)
  ``seq/<mode>/<mod>/slices`` [4]                    ``get_crop()`` after ``update`` over the 20-frame sequence, threshold 0.95
  ``seq/<kind>/count_tb`` [H], ``count_lr`` [W]      the border counts behind it (int32)
From the fp32 run of the restatement ``tests/autocrop_f64.py``:
  ``<input>/<kind>/row_a``, ``row_b`` [B,H], ``col_a``, ``col_b`` [B,W]   for every input of ``all_inputs`` (cases, batch, seq)
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

from oracle import refstub  # noqa: E402
import autocrop_cases as C  # noqa: E402
import autocrop_f64 as R  # noqa: E402


def main():
    refstub.install()
    from nunif.utils.autocrop import AutoCrop, AutoCropDetector

    out = {}
    with torch.inference_mode():
        for kind in C.KINDS:
            black = kind == "black"
            for name, x in C.all_inputs(kind).items():
                for k, v in R.stats(x, kind, torch.float32).items():
                    out[f"{name}/{kind}/{k}"] = v.numpy()
            for name in C.CASES:
                x = C.case_frame(name, kind)
                out[f"{name}/{kind}/mask_tb"] = AutoCropDetector.detect_tb(x, black_only=black).flatten().numpy().astype(np.uint8)
                out[f"{name}/{kind}/mask_lr"] = AutoCropDetector.detect_lr(x, black_only=black).flatten().numpy().astype(np.uint8)
            xb = C.batch_frames(kind)
            out[f"batch/{kind}/mask_tb"] = torch.stack(
                [AutoCropDetector.detect_tb(f, black_only=black).flatten() for f in xb]).numpy().astype(np.uint8)
            out[f"batch/{kind}/mask_lr"] = torch.stack(
                [AutoCropDetector.detect_lr(f, black_only=black).flatten() for f in xb]).numpy().astype(np.uint8)
        for mode in C.MODES:
            kind = mode.split("_")[0]
            for mod in C.MODS:
                for name in C.CASES:
                    ac = AutoCrop.from_image(C.case_frame(name, kind), mode=mode, mod=mod)
                    sh, sw = ac.get_slice()
                    out[f"{name}/{mode}/{mod}/slices"] = np.array(C.enc_slice(sh) + C.enc_slice(sw), dtype=np.int32)
                    out[f"{name}/{mode}/{mod}/pad"] = np.array(ac.get_pad(), dtype=np.int32)
                    out[f"{name}/{mode}/{mod}/crop"] = np.array(ac.get_crop() or (-1, -1, -1, -1), dtype=np.int32)
                det = AutoCropDetector(mode=mode, mod=mod)
                seq = C.seq_frames(kind)
                det.update(seq[:7])                       # a batch, then frame by frame: the reference treats them alike
                for f in seq[7:]:
                    det.update(f)
                sh, sw = det.get_crop()
                out[f"seq/{mode}/{mod}/slices"] = np.array(C.enc_slice(sh) + C.enc_slice(sw), dtype=np.int32)
                if mode in C.KINDS and mod == 1:
                    out[f"seq/{kind}/count_tb"] = det.border_count_tb.flatten().numpy().astype(np.int32)
                    out[f"seq/{kind}/count_lr"] = det.border_count_lr.flatten().numpy().astype(np.int32)
    path = os.path.join(HERE, "autocrop.npz")
    np.savez_compressed(path, **out)
    print(len(out), "arrays,", os.path.getsize(path), "bytes")
    print("s37x67 black mod 2:", out["s37x67/black/2/slices"], " seq black mod 2:", out["seq/black/2/slices"])


if __name__ == "__main__":
    main()
