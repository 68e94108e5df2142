"""Writes tests/golden/row_flow_v2.npz from the LIVE reference (run once where the reference checkout is mounted:
``python tests/golden/make_golden_row_flow_v2.py``).  Numeric arrays only: the weights are regenerated from the seed
(``nunif_amd.synthetic.row_flow_v2_state_dict(301)``), the depth and the image by ``row_flow_v2_ref.fixture_inputs()``.

The reference CLASS ``iw3.models.row_flow_v2.RowFlowV2`` (``delta_output = True``) on the CPU in fp32:
  ``sdsum``                       checksum of the state dict
  ``delta`` [2,1,58,104]          the model on the planes of divergence 2.0, convergence 0.5, width 104
  ``left``, ``right``             ``iw3.backward_warp.apply_divergence_nn_LR`` at steps 1, divergence 2.0 (image = depth size)
  ``left_s2``, ``right_s2``       image 0 at steps 2, divergence 3.0 — what ``calc_auto_warp_steps("row_flow_v2", 3.0)`` picks
  ``right_only``                  image 0, ``synthetic_view="right"``
Conditions checked here: 0.2 < std(delta) < 5, and the stepped warp differs from the single one by more than 1e-3 mean.
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
from oracle import row_flow_v3 as ORF  # noqa: E402
import row_flow_v2_ref as V  # noqa: E402
from nunif_amd.synthetic import row_flow_v2_state_dict  # noqa: E402


def main():
    refstub.install()
    torch.set_grad_enabled(False)
    from iw3.models.row_flow_v2 import RowFlowV2
    from iw3 import backward_warp as RB
    import av
    av.__version__ = "14.2.0"                      # the inert stub's version string does not parse (nunif/utils/video.py)
    from iw3.utils import calc_auto_warp_steps

    sd = row_flow_v2_state_dict(V.WEIGHT_SEED)
    m = RowFlowV2().eval()
    m.load_state_dict(sd, strict=True)
    m.delta_output = True
    depth, c = V.fixture_inputs()
    out = {"sdsum": float(sum(v.double().sum().item() for v in sd.values() if v.is_floating_point()))}
    out["delta"] = m(ORF.make_input(depth, 2.0, 0.5, 104))[:, :1]
    std = out["delta"].std().item()
    assert 0.2 < std < 5.0, std
    kw = dict(enable_amp=False)
    out["left"], out["right"] = RB.apply_divergence_nn_LR(m, c, depth, 2.0, 0.5, steps=1, synthetic_view="both", **kw)
    assert calc_auto_warp_steps("row_flow_v2", 3.0, "both") == 2
    out["left_s2"], out["right_s2"] = RB.apply_divergence_nn_LR(m, c[:1], depth[:1], 3.0, 0.5, steps=2, synthetic_view="both", **kw)
    one, _ = RB.apply_divergence_nn_LR(m, c[:1], depth[:1], 3.0, 0.5, steps=1, synthetic_view="both", **kw)
    diff = (one - out["left_s2"]).abs().mean().item()
    assert diff > 1e-3, diff
    _, out["right_only"] = RB.apply_divergence_nn_LR(m, c[:1], depth[:1], 2.0, 0.5, steps=1, synthetic_view="right", **kw)
    path = os.path.join(HERE, "row_flow_v2.npz")
    np.savez_compressed(path, **{k: (v.numpy() if torch.is_tensor(v) else np.asarray(v)) for k, v in out.items()})
    print("wrote", path, os.path.getsize(path) // 1024, "KiB; std(delta)", std, "steps-2 vs 1 mean diff", diff)


if __name__ == "__main__":
    main()
