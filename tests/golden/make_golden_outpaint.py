"""Writes tests/golden/outpaint.npz from the LIVE reference (run once where the reference checkout is mounted:
``python tests/golden/make_golden_outpaint.py``).  Numeric arrays only; the weights are regenerated from the seed
(``nunif_amd.synthetic.light_outpaint_state_dict(WEIGHT_SEED)``), the inputs from tests/outpaint_f64.py.  Everything is the
reference's own class ``stlizer.models.light_outpaint_v1.LightOutpaintV1`` in fp32 on the CPU.

``out/<case>/raw``        ``infer(x, mask, max_size, composite=False)`` (tests/outpaint_f64.FIXTURE_CASES); the composite and the
                          eval forward are that map behind a ``where`` / a clamp and are derived from it by the tests
``tap/<case>/<tap>``      dct / enc / mid / dec / proj of that call (FIXTURE_TAP_CASES): outputs of ``net.dct``, ``net.enc_block``,
                          ``net.enc_block + net.proj_out``, ``net.dec_block``, ``net.to_image_biliner.proj``
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
import outpaint_f64 as R  # noqa: E402
from nunif_amd.synthetic import light_outpaint_state_dict  # noqa: E402


def reference_model(dtype=torch.float32):
    refstub.install()
    from stlizer.models.light_outpaint_v1 import LightOutpaintV1
    model = LightOutpaintV1()
    model.load_state_dict(light_outpaint_state_dict(R.WEIGHT_SEED))
    return model.eval().to(dtype)


def run_reference(model, x, mask, max_size):
    """-> (raw output, taps) of one infer call, through forward hooks."""
    got = {}
    net = model.net
    hooks = [net.dct.register_forward_hook(lambda m, i, o: got.__setitem__("dct", o)),
             net.enc_block.register_forward_hook(lambda m, i, o: got.__setitem__("enc", o)),
             net.proj_out.register_forward_hook(lambda m, i, o: got.__setitem__("proj_out", o)),
             net.dec_block.register_forward_hook(lambda m, i, o: got.__setitem__("dec", o)),
             net.to_image_biliner.proj.register_forward_hook(lambda m, i, o: got.__setitem__("proj", o))]
    with torch.inference_mode():
        z = model.infer(x.clone(), mask, max_size=max_size, composite=False)
    for h in hooks:
        h.remove()
    got["mid"] = got["enc"] + got.pop("proj_out")
    return z, got


def main():
    model = reference_model()
    out = {}
    for name in R.FIXTURE_CASES:
        x, mask = R.case_input(name)
        z, taps = run_reference(model, x, mask, R.CASES[name][3])
        out[f"out/{name}/raw"] = z.numpy()
        if name in R.FIXTURE_TAP_CASES:
            for t in R.TAPS:
                out[f"tap/{name}/{t}"] = taps[t].numpy()
        print(name, tuple(z.shape), "rms", float(z.pow(2).mean().sqrt()))
    path = os.path.join(HERE, "outpaint.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes,", len(out), "arrays")


if __name__ == "__main__":
    main()
