"""Fixture of ``waifu2x.wgmlp_4x``: ``synthetic.wgmlp_state_dict(SEED)`` loaded into the reference's OWN ``WGMLP4x`` on the CPU (fp32),
one batch of two 64 x 64 tiles -> tests/golden/wgmlp.npz with the input, the un-clamped output (the eval output is its clamp), the IR stem's map and the
outputs of three blocks (cropped).  The weights are regenerated from the seed by the tests and are not stored.

    python tests/golden/make_golden_wgmlp.py        (needs the reference tree; see oracle/refstub.py)
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

SEED, INPUT_SEED, TILE, BATCH = 21, 5, 64, 2
TAPS = ("unet.wgmlp1.blocks.1.", "unet.wgmlp2.blocks.2.", "unet.wgmlp3.blocks.2.")


def main():
    from oracle import refstub
    refstub.install()
    from waifu2x.models.wgmlp import WGMLP4x
    from nunif_amd import synthetic
    import wgmlp_ref
    torch.manual_seed(0)
    sd = synthetic.wgmlp_state_dict(SEED)
    model = WGMLP4x().eval()
    model.load_state_dict(sd, strict=True)
    x = wgmlp_ref.test_input(INPUT_SEED, BATCH, TILE)
    maps = {}
    hooks = [model.unet.ir.register_forward_hook(lambda m, i, o: maps.__setitem__("ir", o.detach()))]
    for p in TAPS:
        mod = model.get_submodule(p[:-1])
        hooks.append(mod.register_forward_hook(lambda m, i, o, p=p: maps.__setitem__(p, o.detach().permute(0, 2, 3, 1))))
    with torch.inference_mode():
        y = model(x)
        model.train()
        for h in hooks:
            h.remove()
        raw = model(x)           # training mode returns the un-clamped image (:464-465); no layer of the net depends on the mode
    assert torch.equal(y, raw.clamp(0, 1))
    # y = clamp(raw) is not stored; image 0 whole, of image 1 the top-left 96 x 96 (the file stays under the size limit of the tree)
    out = {"x": x.numpy(), "raw0": raw[0].numpy(), "raw1": raw[1, :, :96, :96].contiguous().numpy(),
           "ir": maps["ir"][:, :, 8:40, 8:40].numpy()}
    for i, p in enumerate(TAPS):
        out[f"tap{i}"] = maps[p][:, 4:20, 4:20, :32].contiguous().numpy()
    path = os.path.join(HERE, "wgmlp.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes;", {k: v.shape for k, v in out.items()})
    print("clamped fraction", float(((y <= 0) | (y >= 1)).float().mean()), "std", float(y.std()))


if __name__ == "__main__":
    main()
