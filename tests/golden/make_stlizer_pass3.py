"""Writes tests/golden/stlizer_pass3.npz (and stlizer_pass3_n5000.npz, the one long case, so that either file stays below the size
limit for a committed file) from the LIVE reference (run once where the reference checkout is mounted:
``python tests/golden/make_stlizer_pass3.py``).  Numeric arrays only.  Everything is the reference's own
``stlizer.multipass_pipeline`` in float64 (the scene weight in fp32) on the CPU, on the synthetic cases of
tests/stlizer_pass3_ref.py.

``in/<case>/shift_x | shift_y | angle | scores``  per-frame transforms as pass 2 leaves them, mean match scores of pass 1
``ref/<case>/weight``                           ``calc_scene_weight`` (fp32)
``ref/<case>/paths``                            [3, N]: the clamped, weighted prefix sums of ``pass3`` / ``pass3_smoothing``
``ref/<case>/gaussian | savgol``                [3, N]: ``conv1d_smoothing`` of the paths (2 s at the case's fps)
``ref/<case>/taps_gaussian | taps_savgol``      ``gen_smoothing_kernel``
``ref/<case>/out3``                             [3, N]: ``grad_opt(..., iteration=3)`` with the case's penalty weight (pass 3's own unless the case names one)
``ref/<case>/out100``                           the same at ``iteration=100`` (converged cases only)
``ref/<case>/pert100``                          [8, 3, N]: ``iteration=100`` on the paths scaled by 1 + k 2^-52 (rows 0..3, k = 1..4)
                                                and 1 - k 2^-52 (rows 4..7)
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
import stlizer_pass3_ref as R  # noqa: E402

SPLIT = {"n5000": "stlizer_pass3_n5000.npz"}


def reference_module():
    refstub.install()
    import stlizer.multipass_pipeline as MP
    MP.tqdm = lambda it, **kw: it
    return MP


def run_grad_opt(MP, name, paths, weight, resolution, iteration):
    tx, ty, ta = (torch.from_numpy(paths[a].copy()).reshape(1, 1, -1) for a in range(3))
    with torch.inference_mode(False), torch.enable_grad():
        out = MP.grad_opt(tx, ty, ta, weight.clone(), resolution, iteration=iteration, penalty_weight=R.penalty_weight(name))
    return torch.stack([o.detach() for o in out]).numpy()


def run_case(MP, name):
    sx, sy, an, scores, resolution, fps = R.case_input(name)
    dev = torch.device("cpu")
    out = {f"in/{name}/shift_x": sx, f"in/{name}/shift_y": sy, f"in/{name}/angle": an, f"in/{name}/scores": scores}
    weight = MP.calc_scene_weight(scores.tolist(), device=dev)
    out[f"ref/{name}/weight"] = weight.numpy().copy()
    tsx, tsy = torch.from_numpy(sx), torch.from_numpy(sy)
    tan = torch.from_numpy(an).clamp(-MP.ANGLE_MAX_HARD, MP.ANGLE_MAX_HARD)
    paths = torch.stack([(v * weight).cumsum(dim=0) for v in (tsx, tsy, tan)]).numpy()
    out[f"ref/{name}/paths"] = paths
    for method in ("gaussian", "savgol"):
        k = R.kernel_size(R.SMOOTHING_SECONDS, fps)
        out[f"ref/{name}/taps_{method}"] = MP.gen_smoothing_kernel(method, k, dev).flatten().numpy()
        fix = MP.pass3_smoothing(tsx, tsy, tan, weight, method, R.SMOOTHING_SECONDS, fps, resolution, dev)
        out[f"ref/{name}/{method}"] = torch.stack(fix).numpy()
    out[f"ref/{name}/out3"] = run_grad_opt(MP, name, paths, weight, resolution, 3)
    if name in R.CONVERGED_CASES:
        out[f"ref/{name}/out100"] = run_grad_opt(MP, name, paths, weight, resolution, 100)
        eps = 2.0 ** -52
        scales = [1 + k * eps for k in (1, 2, 3, 4)] + [1 - k * eps for k in (1, 2, 3, 4)]
        out[f"ref/{name}/pert100"] = np.stack([run_grad_opt(MP, name, paths * s, weight, resolution, 100) for s in scales])
    return out


def main():
    torch.set_num_threads(1)
    MP = reference_module()
    files = {"stlizer_pass3.npz": {}}
    for name in R.CASES:
        files.setdefault(SPLIT.get(name, "stlizer_pass3.npz"), {}).update(run_case(MP, name))
    for fname, out in files.items():
        path = os.path.join(HERE, fname)
        np.savez_compressed(path, **out)
        print(f"wrote {path}: {len(out)} arrays, {os.path.getsize(path)} bytes")


if __name__ == "__main__":
    main()
