"""Writes tests/golden/cliqa.npz: the REFERENCE classes (cliqa/models/*.py) in float64 on the CPU with
``nunif_amd.synthetic.cliqa_state_dict`` weights.  Needs the reference checkout (``oracle.refstub``).  Run from the repository root:
``python tests/golden/make_golden_cliqa.py``.

Per net and shape of tests/cliqa_f64.py: a digest of the input, the outputs (ScaleFactor's before and after its eval clamp) and a
digest (mean, mean |.|, max |.|, 64 strided samples) of the maps behind the three pools and in front of the global pools, taken by
forward hooks.  For the three small shapes (``WHOLE_TAP_SHAPES``) the whole maps are stored too, in float32, one file per net
(tests/golden/cliqa_taps_<net>.npz); the maps of the 40 x 56 and 128 x 128 cases are not (one 128 x 128 case alone would be
8 MB).  Seeds are stored, not weights.
Per selection case: the float64 ``std_score`` (the reference's function) of every patch, ``torch.topk`` indices, a digest of the
chosen patches.  ``extract_patches`` itself cannot run here (it needs torchvision's ``to_tensor``): its loop is restated around the
reference's ``std_score``.  Per net: the returns of the reference's ``predict_*`` on the (2, 128, 128)-case input as patches.
"""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

from oracle import refstub  # noqa: E402

refstub.install()
import cliqa.models as RM  # noqa: E402
import cliqa.utils as RU  # noqa: E402

import cliqa_f64 as C  # noqa: E402
from nunif_amd.synthetic import cliqa_state_dict  # noqa: E402

CLASSES = {"jpeg_quality": RM.JPEGQuality, "grain_noise_level": RM.GrainNoiseLevel, "scale_factor": RM.ScaleFactor}
PREDICT = {"jpeg_quality": RU.predict_jpeg_quality, "grain_noise_level": RU.predict_grain_noise_psnr,
           "scale_factor": RU.predict_resize_quality}


def main():
    out = {}
    for kind, cls in CLASSES.items():
        whole = {}
        out[f"{kind}.seed"] = np.array(C.SEED[kind])
        model = cls()
        model.load_state_dict(cliqa_state_dict(C.SEED[kind], kind))
        model = model.double().eval()
        got = {}
        hooks = [model.features[i].register_forward_hook(lambda m, a, o, n=n: got.__setitem__(n, o.clone()))
                 for i, n in ((6, "pool1"), (8, "pool2"), (10, "pool3"))]
        heads = [getattr(model, h) for h in C.HEADS[kind]]
        hooks += [h[2].register_forward_hook(lambda m, a, o, n=i: got.__setitem__(f"head{n}", o.clone())) for i, h in enumerate(heads)]
        for shape in C.SHAPES:
            tag = f"{kind}.{shape[0]}x{shape[1]}x{shape[2]}"
            x = C.net_input(kind, shape)
            with torch.no_grad():
                y = model(x.double())
                if kind == "scale_factor":
                    model.train(False)
                    raw = model.scale_factor_output(model.features(model.preprocess(x.double()))).view(shape[0], -1)
                    out[tag + ".raw"] = raw.numpy()
            y = y if isinstance(y, tuple) else (y,)
            out[tag + ".x"] = C.digest(x)
            for i, v in enumerate(y):
                out[f"{tag}.out{i}"] = v.numpy()
            got["head_maps"] = torch.cat([got[f"head{i}"] for i in range(len(heads))], dim=1)
            for n in C.TAPS:
                out[f"{tag}.{n}"] = C.digest(got[n])
                if shape in C.WHOLE_TAP_SHAPES:
                    whole[f"{tag}.{n}"] = got[n].float().numpy()
        for h in hooks:
            h.remove()
        np.savez_compressed(C.GOLDEN_TAPS % kind, **whole)
        print(C.GOLDEN_TAPS % kind, os.path.getsize(C.GOLDEN_TAPS % kind), "bytes")
        patches = C.net_input(kind, (2, 128, 128)).double()
        out[f"{kind}.predict"] = np.array(PREDICT[kind](model, patches), dtype=np.float64).reshape(-1)
    for case in C.SELECT:
        tag = "select.%dx%d.%d" % case
        img = C.select_image(case)
        _, patches = C.std_scores64(img)
        scores = RU.std_score(patches.double())
        _, idx = torch.topk(scores, min(case[2], scores.shape[0]))
        out[tag + ".scores"] = scores.numpy()
        out[tag + ".indices"] = idx.numpy()
        out[tag + ".patches"] = C.digest(patches[idx])
    np.savez_compressed(C.GOLDEN, **out)
    print(C.GOLDEN, os.path.getsize(C.GOLDEN), "bytes")


if __name__ == "__main__":
    main()
