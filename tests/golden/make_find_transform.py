"""Writes tests/golden/find_transform.npz from the LIVE reference (run once where the reference checkout is mounted:
``python tests/golden/make_find_transform.py``).  Numeric arrays only.  Everything is the reference's own
``nunif.utils.superpoint.find_transform`` in fp32 on the CPU, batch form, on the synthetic cases of tests/find_transform_ref.py.

``in/<case>/xy1 | xy2 | center | mask``    the inputs (``mask`` absent where the case passes none)
``out/<case>/shift | scale | angle``       the reference's return values
``out/<case>/trace``                       (tx, ty, scale, rotation) of every pair after every optimiser step [iteration, B, 4]:
                                           the reference does not return them, so ``torch.optim.Adam.step`` is wrapped for the
                                           call and the three parameter tensors are copied after every step
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
import find_transform_ref as R  # noqa: E402


def reference_find_transform():
    refstub.install()
    from nunif.utils import superpoint as KU
    return KU.find_transform


def run_reference(fn, name):
    """-> {key: array} of one case."""
    xy1, xy2, mask, center, kwargs = R.case_input(name)
    B = xy1.shape[0]
    steps = []
    adam_step = torch.optim.Adam.step

    def recording_step(self, *a, **k):
        ret = adam_step(self, *a, **k)
        translation, scale, rotation = [p for group in self.param_groups for p in group["params"]]
        steps.append(torch.cat([translation.detach().reshape(B, 2), scale.detach().reshape(B, 1), rotation.detach().reshape(B, 1)],
                               dim=1).clone())
        return ret

    torch.optim.Adam.step = recording_step
    try:
        with torch.enable_grad():
            shift, scale, angle, _ = fn(xy1.clone(), xy2.clone(), center.view(B, 1, 2).clone(),
                                        mask=None if mask is None else mask.clone(), **kwargs)
    finally:
        torch.optim.Adam.step = adam_step
    assert len(steps) == kwargs["iteration"]
    out = {f"in/{name}/xy1": xy1.numpy(), f"in/{name}/xy2": xy2.numpy(), f"in/{name}/center": center.numpy(),
           f"out/{name}/shift": shift.numpy(), f"out/{name}/scale": scale.numpy(), f"out/{name}/angle": angle.numpy(),
           f"out/{name}/trace": torch.stack(steps).numpy()}
    if mask is not None:
        out[f"in/{name}/mask"] = mask.numpy()
    return out


def generate():
    torch.set_num_threads(1)                      # the reference's fp32 sums do not depend on how the machine splits them
    fn = reference_find_transform()
    out = {}
    for name in R.CASES:
        out.update(run_reference(fn, name))
    return out


def main():
    out = generate()
    path = os.path.join(HERE, "find_transform.npz")
    np.savez_compressed(path, **out)
    print(f"wrote {path}: {len(out)} arrays, {os.path.getsize(path)} bytes")


if __name__ == "__main__":
    main()
