"""Writes tests/golden/superpoint.npz from the LIVE reference (run once where the reference checkout is mounted:
``python tests/golden/make_golden_superpoint.py``).  Numeric arrays only; the weights are regenerated from the seed
(``nunif_amd.synthetic.superpoint_state_dict(WEIGHT_SEED)``), the inputs from tests/superpoint_f64.py.  Everything is the reference's
own class / function in fp32 on the CPU.

``sp/<case>/scores``            the score map before NMS (the class's own submodules and lines :116-128)
``sp/<case>/descriptors``       dense descriptors, the small shapes only
``sp/<case>/<tap>``             backbone block outputs (tests/superpoint_f64.TAP_CASES)
``sp/<case>/<b>/keypoints|keypoint_scores|descriptors``   ``SuperPoint(...).infer`` per image (descriptors not for s120x160)
``match/<case>/index|sim``      argmax / max of ``d1 @ d2.t()`` as ``find_match_index(..., threshold=-2, return_score_all=True)`` returns
``warp/<shape>/<params>/<padding>``   ``apply_transform`` (the 21 x 33 shape only)
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
import superpoint_f64 as R  # noqa: E402
from nunif_amd.synthetic import superpoint_state_dict  # noqa: E402


def main():
    refstub.install()
    import nunif.utils.superpoint as KU
    out = {}
    model = KU.SuperPoint(detection_threshold=R.THRESHOLD, nms_radius=R.NMS_RADIUS, remove_borders=R.REMOVE_BORDERS)
    model.load_state_dict(superpoint_state_dict(R.WEIGHT_SEED))
    model.eval()
    with torch.inference_mode():
        for name in R.CASES:
            image = R.case_image(name)
            gray = image
            if image.shape[1] == 3:
                gray = (image * image.new_tensor([0.299, 0.587, 0.114]).view(1, 3, 1, 1)).sum(1, keepdim=True)
            x = gray
            for b in range(4):
                x = model.backbone[b](x)
                if f"backbone.{b}" in R.TAP_CASES.get(name, ()):
                    out[f"sp/{name}/backbone.{b}"] = x.numpy()
            s = torch.nn.functional.softmax(model.detector(x), 1)[:, :-1]
            B, _, h, w = s.shape
            s = s.permute(0, 2, 3, 1).reshape(B, h, w, 8, 8).permute(0, 1, 3, 2, 4).reshape(B, h * 8, w * 8)
            if name != "s120x160":
                out[f"sp/{name}/scores"] = s.numpy()
            if name in R.DENSE_DESCRIPTOR_CASES:
                out[f"sp/{name}/descriptors"] = torch.nn.functional.normalize(model.descriptor(x), p=2, dim=1).numpy()
            ret = model.infer(image)
            for b, r in enumerate(ret):
                out[f"sp/{name}/{b}/keypoints"] = r["keypoints"].numpy()
                out[f"sp/{name}/{b}/keypoint_scores"] = r["keypoint_scores"].numpy()
                if name in R.DENSE_DESCRIPTOR_CASES:
                    out[f"sp/{name}/{b}/descriptors"] = r["descriptors"].numpy()
            print(name, [len(r["keypoints"]) for r in ret], float(s.max()))
        for name in R.MATCH_CASES:
            d1, d2 = R.match_inputs(name)
            i1, i2, sim = KU.find_match_index({"descriptors": d1}, {"descriptors": d2}, threshold=-2.0, return_score_all=True)
            assert torch.equal(i1, torch.arange(d1.shape[0]))
            out[f"match/{name}/index"] = i2.numpy()
            out[f"match/{name}/sim"] = sim.numpy()
        shape = "w21x33"
        x = R.warp_image(shape)
        for pname in R.WARP_PARAMS:
            shift, scale, angle, center = R.warp_params(shape, pname)
            for padding in ("zeros", "border"):
                out[f"warp/{shape}/{pname}/{padding}"] = KU.apply_transform(x, shift, scale, angle, center, padding_mode=padding).numpy()
    path = os.path.join(HERE, "superpoint.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes,", len(out), "arrays")


if __name__ == "__main__":
    main()
