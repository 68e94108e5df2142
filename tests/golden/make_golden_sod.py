"""Writes tests/golden/sod_v1.npz from the LIVE reference (run once where the reference checkout is mounted:
``python tests/golden/make_golden_sod.py``).  Numeric arrays only; the weights are regenerated from the seed
(``nunif_amd.synthetic.sod_v1_state_dict(sod_f64.WEIGHT_SEED)``), the inputs by ``tests/sod_f64.py``.

For every case of ``sod_f64.CASES``, the reference CLASS ``iw3.models.sod_v1.SODV1`` (``eval().fuse()``) on the CPU:
  ``<case>/sal32``, ``<case>/depth32``   ``infer`` in fp32;   ``<case>/sal16``   the same under CPU autocast (bfloat16 is what
  CPU autocast offers; it is the half-precision yardstick), stored as fp32
  ``<case>/hx1`` .. ``hx6``, ``hx1d``      max |fp32 tap - float64 tap| per image is small enough to keep as scalars:
                                         ``<case>/tap_err32`` [7] (the maps themselves would be 20 MB)
  ``<case>/z32``, ``<case>/z16``         ``ConvergenceEstimator.depth_position_from_ratio`` of those, pos 0.5
``empty/sal32``: scene_a with ``outconv.bias = EMPTY_OUT_BIAS`` (an empty mask).
``ema/z32``, ``ema/z16`` [8]: the estimator's per-frame values over ``sod_f64.ema_inputs()`` and ``ema/out32``, ``ema/out16`` the
reference's EMA loop (decay 0.9, resets after frames 2 and 5) over them in batches of 3, 3, 2.
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
import sod_f64 as R  # noqa: E402
from nunif_amd.synthetic import sod_v1_state_dict  # noqa: E402


def main():
    refstub.install()
    from iw3.models.sod_v1 import SODV1
    from iw3.convergence_estimator import ConvergenceEstimator

    def model(sd):
        m = SODV1()
        m.load_state_dict(sd)
        return m.eval().fuse()

    sd = sod_v1_state_dict(R.WEIGHT_SEED)
    m = model(sd)
    dpos = ConvergenceEstimator.depth_position_from_ratio
    out = {}

    def run(rgb, depth, half):
        with torch.inference_mode(), torch.autocast(device_type="cpu", dtype=torch.bfloat16, enabled=half):
            sal, d = m.infer(rgb, depth)
            z = dpos(sal, d, R.CONVERGENCE)
        return sal.float(), d.float(), z.float().flatten()

    for name, *_ in R.CASES:
        rgb, depth = R.case_inputs(name)
        sal32, d32, z32 = run(rgb, depth, False)
        sal16, _, z16 = run(rgb, depth, True)
        out[f"{name}/sal32"], out[f"{name}/depth32"], out[f"{name}/sal16"] = sal32.numpy(), d32.numpy(), sal16.numpy()
        out[f"{name}/z32"], out[f"{name}/z16"] = z32.numpy(), z16.numpy()
        # the reference's own taps: forward hooks on the stages
        taps = {}
        hooks = [getattr(m.u2netp, f"stage{i}").register_forward_hook(lambda mod, a, o, k=f"hx{i}": taps.__setitem__(k, o))
                 for i in range(1, 7)]
        hooks.append(m.u2netp.stage1d.register_forward_hook(lambda mod, a, o: taps.__setitem__("hx1d", o)))
        with torch.inference_mode():
            m.infer(rgb, depth)
        for h in hooks:
            h.remove()
        t64 = {}
        R.infer(sd, rgb, depth, taps=t64)
        names = ("hx1", "hx2", "hx3", "hx4", "hx5", "hx6", "hx1d")
        out[f"{name}/tap_err32"] = np.array([float(R.max_err_per_image(taps[k], t64[k]).max()) for k in names])
    rgb, depth = R.case_inputs("scene_a")
    m_empty = model(sod_v1_state_dict(R.WEIGHT_SEED, out_bias=R.EMPTY_OUT_BIAS))
    with torch.inference_mode():
        out["empty/sal32"] = m_empty.infer(rgb, depth)[0].float().numpy()

    rgbs, depths = R.ema_inputs()
    resets = [i in R.EMA_RESETS for i in range(R.EMA_FRAMES)]
    for tag, half in (("32", False), ("16", True)):
        z = torch.cat([run(rgbs[i:i + 1], depths[i:i + 1], half)[2] for i in range(R.EMA_FRAMES)])
        out[f"ema/z{tag}"] = z.numpy()
        est = ConvergenceEstimator.__new__(ConvergenceEstimator)          # the reference's loop, without its checkpoint download
        est.enable_ema, est.decay, est.convergence_ema = True, R.EMA_DECAY, None
        res = []
        for i0, i1 in ((0, 3), (3, 6), (6, 8)):
            zs = z[i0:i1].reshape(-1, 1, 1, 1)
            results = []
            for i in range(zs.shape[0]):                                   # convergence_estimator.py:72-80
                p = zs[i]
                if est.convergence_ema is None:
                    est.convergence_ema = p.clone()
                else:
                    est.convergence_ema = est.decay * est.convergence_ema + (1. - est.decay) * p
                results.append(est.convergence_ema.clone())
                if resets[i0 + i]:
                    est.reset()
            res.append(torch.stack(results).flatten())
        out[f"ema/out{tag}"] = torch.cat(res).numpy()
    np.savez_compressed(os.path.join(HERE, "sod_v1.npz"), **out)
    for k, v in out.items():
        print(k, v.shape, v.dtype)


if __name__ == "__main__":
    main()
