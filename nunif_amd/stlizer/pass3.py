"""stlizer pass 3 on the HIP engine: ``calc_scene_weight``, the smoothing filters, ``grad_opt`` and ``pass3`` of the reference's
``stlizer/multipass_pipeline.py:64-105, :272-366``, with the reference's signatures and returns (three float64 device tensors of
length N).

The reference's ``grad_opt`` is ``torch.optim.LBFGS(history_size=10, max_iter=4)`` for 100 steps over three vectors of N + 3
elements: about 400 autograd closures and a scalar read back at every ``if`` of the two-loop recursion.  Here it is a fixed
schedule of launches of ``nunif_hip_stlizer_pass3_grad_opt`` (the same decisions, taken on the device) and nothing is read back;
``pass3(..., host=True)`` then hands pass 4's per-frame loop three Python lists after one device-to-host read, where the reference
reads ``.item()`` three times per frame.

A host tensor or a CPU device raises: there is no CPU fallback, as in ``find_transform.py``.  ``nunif_amd.install()`` does not
bind this module (its table holds no ``stlizer`` module); it is the engine-side public form, like ``find_transform``.
"""
import ctypes

import numpy as np
import torch

from .. import _hip

DEFAULT_RESOLUTION = 320
MAX_FRAMES, MAX_ITERATION, MAX_TAPS = 1 << 20, 1024, 4097
REC_DOUBLES = 32
# fields of a decision record (nunif_amd/csrc/stlizer_pass3_host.h)
REC = {name: i for i, name in enumerate(
    ("active", "exit_begin", "exit_gtd", "exit_after", "accepted", "loss", "maxg", "gtd", "ys", "maxg_new", "maxdt", "dloss",
     "t", "hdiag", "head", "num_old", "niter", "stale", "xbuf", "al"))}

MAX_WORKSPACES = 8
_workspaces = {}           # (device index, stream) -> uint8 tensor, grown by size; at most MAX_WORKSPACES, oldest dropped first


def _ptr(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else None


def workspace_bytes(N, iteration=1):
    """``nunif_hip_stlizer_pass3_workspace_bytes``; raises for a shape beyond the limits."""
    n = _hip.lib().nunif_hip_stlizer_pass3_workspace_bytes(int(N), int(iteration))
    if n < 0:
        raise ValueError(f"stlizer pass 3: N={N} iteration={iteration} is outside 1 <= N <= {MAX_FRAMES}, "
                         f"1 <= iteration <= {MAX_ITERATION}")
    return n


def _workspace(device, nbytes):
    # one per device and stream, as in find_transform.py: calls on two streams may overlap
    key = (device.index, torch.cuda.current_stream(device).cuda_stream)
    ws = _workspaces.pop(key, None)
    if ws is None or ws.numel() < nbytes:
        ws = torch.empty(nbytes, dtype=torch.uint8, device=device)
    _workspaces[key] = ws
    while len(_workspaces) > MAX_WORKSPACES:
        del _workspaces[next(iter(_workspaces))]
    return ws


def _device_of(name, t):
    if not torch.is_tensor(t):
        raise RuntimeError(f"stlizer pass 3: {name} must be a tensor")
    if t.device.type != "cuda":
        raise RuntimeError(f"stlizer pass 3: {name} is on {t.device}; the HIP engine needs a ROCm device tensor and has no CPU "
                           "fallback (use stlizer.multipass_pipeline there)")
    return t.device


def _vec(name, t, device, dtype=torch.float64):
    _device_of(name, t)
    if t.device != device:
        raise RuntimeError(f"stlizer pass 3: {name} is on {t.device}, the other operands on {device}")
    return t.detach().to(dtype).reshape(-1).contiguous()


def calc_scene_weight(mean_match_scores, device=None):
    """``calc_scene_weight`` (:86-105): fp32 weights, bit-equal to the reference's."""
    if torch.is_tensor(mean_match_scores):
        score = mean_match_scores
    else:
        if device is None or torch.device(device).type != "cuda":
            raise RuntimeError(f"calc_scene_weight: device {device}; the HIP engine needs a ROCm device and has no CPU fallback")
        score = torch.tensor(mean_match_scores, dtype=torch.float32, device=device)
    dev = _device_of("mean_match_scores", score)
    if score.dtype != torch.float32 or score.ndim != 1 or score.numel() == 0:
        raise RuntimeError(f"calc_scene_weight: scores must be a non-empty 1-D fp32 tensor, got {score.dtype} {tuple(score.shape)}")
    score = score.contiguous()
    weight = torch.empty_like(score)
    with torch.cuda.device(dev):
        _hip.check(_hip.lib().nunif_hip_stlizer_scene_weight(_ptr(score), score.numel(), _ptr(weight), _hip.current_stream_ptr(dev)))
    return weight


def gaussian_taps(kernel_size):
    """``get_gaussian_kernel1d`` (nunif/modules/gaussian_filter.py:8-19) in its own expressions, float64, on the host."""
    if kernel_size == 1:
        return torch.ones((1,), dtype=torch.float64)
    sigma = kernel_size * 0.15 + 0.35
    ksize_half = (kernel_size - 1) * 0.5
    x = torch.linspace(-ksize_half, ksize_half, steps=kernel_size, dtype=torch.float64)
    kernel = torch.exp(-0.5 * (x / sigma).pow(2))
    return kernel / kernel.sum()


def gen_smoothing_kernel(name, kernel_size, device):
    """``gen_smoothing_kernel`` (:69-75): [1, 1, K] float64 taps on ``device``, built on the host."""
    if kernel_size > MAX_TAPS:
        raise ValueError(f"gen_smoothing_kernel: {kernel_size} taps; the engine's filter takes at most {MAX_TAPS}")
    if name == "gaussian":
        taps = gaussian_taps(kernel_size)
    elif name == "savgol":
        try:
            import scipy.signal
        except ImportError as e:
            raise RuntimeError("--filter savgol needs scipy (scipy.signal.savgol_coeffs), which is not installed") from e
        taps = torch.from_numpy(np.ascontiguousarray(scipy.signal.savgol_coeffs(kernel_size, polyorder=2)))
    else:
        raise NotImplementedError(f"--filter {name}")
    return taps.to(device).reshape(1, 1, -1)


def smoothing_fix(paths, taps):
    """paths [3, N] float64, taps [K] float64 (device) -> the smoothed paths minus the paths, [3, N]."""
    N, K = paths.shape[1], taps.numel()
    fix = torch.empty_like(paths)
    with torch.cuda.device(paths.device):
        _hip.check(_hip.lib().nunif_hip_stlizer_pass3_conv(_ptr(paths), N, _ptr(taps), K, _ptr(fix),
                                                          _hip.current_stream_ptr(paths.device)))
    return fix


def conv1d_smoothing(shift_x, shift_y, angle, method, smoothing_seconds, fps, device):
    """``conv1d_smoothing`` (:272-289) of three prepared paths (any shape with N elements)."""
    dev = _device_of("shift_x", shift_x)
    kernel_size = int(smoothing_seconds * float(fps))
    if kernel_size % 2 == 0:
        kernel_size = kernel_size + 1
    taps = gen_smoothing_kernel(name=method, kernel_size=kernel_size, device=dev).reshape(-1).contiguous()
    paths = torch.stack([_vec("shift_x", shift_x, dev), _vec("shift_y", shift_y, dev), _vec("angle", angle, dev)])
    fix = smoothing_fix(paths, taps)
    return fix[0], fix[1], fix[2]


def grad_opt_traced(paths, scene_weight, resolution, iteration=100, penalty_weight=1e-3, trace=False, log=False, workspace=None):
    """``grad_opt`` on prepared paths [3, N]; can also return x after every LBFGS iteration slot ``[iteration * 4, 3, N + 3]`` and
    the decision records ``[iteration * 4, 32]`` (tests), and take a caller's ``workspace`` (uint8 device tensor)."""
    dev = _device_of("paths", paths)
    if paths.dtype != torch.float64 or paths.ndim != 2 or paths.shape[0] != 3:
        raise RuntimeError(f"grad_opt: paths must be [3, N] float64, got {paths.dtype} {tuple(paths.shape)}")
    N, iteration = paths.shape[1], int(iteration)
    weight = _vec("scene_weight", scene_weight, dev, torch.float32)
    if weight.numel() != N:
        raise RuntimeError(f"grad_opt: {weight.numel()} scene weights for {N} frames")
    need = workspace_bytes(N, iteration)
    paths = paths.contiguous()
    with torch.cuda.device(dev):
        ws = workspace if workspace is not None else _workspace(dev, need)
        out = torch.empty((3, N), dtype=torch.float64, device=dev)
        tr = torch.empty((iteration * 4, 3, N + 3), dtype=torch.float64, device=dev) if trace else None
        lg = torch.empty((iteration * 4, REC_DOUBLES), dtype=torch.float64, device=dev) if log else None
        _hip.check(_hip.lib().nunif_hip_stlizer_pass3_grad_opt(
            _ptr(paths), _ptr(weight), N, float(resolution / DEFAULT_RESOLUTION), iteration, float(penalty_weight), _ptr(out),
            _ptr(ws), ws.numel(), _ptr(tr), _ptr(lg), _hip.current_stream_ptr(dev)))
    return out, tr, lg


def grad_opt(tx, ty, ta, scene_weight, resolution, iteration=100, penalty_weight=1e-3):
    """``grad_opt`` (:292-334).  The optimizer is the reference's and is not an argument: LBFGS, history 10, 4 iterations a step."""
    dev = _device_of("tx", tx)
    paths = torch.stack([_vec("tx", tx, dev), _vec("ty", ty, dev), _vec("ta", ta, dev)])
    out = grad_opt_traced(paths, scene_weight, resolution, iteration, penalty_weight)[0]
    return out[0], out[1], out[2]


def prepare(shift_x, shift_y, angle, scene_weight):
    """The angle clamped to +-90, the three per-frame values times the weight, their prefix sums (:359, :338-344) -> [3, N]."""
    dev = _device_of("shift_x", shift_x)
    sx, sy, an = _vec("shift_x", shift_x, dev), _vec("shift_y", shift_y, dev), _vec("angle", angle, dev)
    weight = _vec("scene_weight", scene_weight, dev, torch.float32)
    N = sx.numel()
    if not (sy.numel() == an.numel() == weight.numel() == N) or N == 0:
        raise RuntimeError(f"stlizer pass 3: {N}, {sy.numel()}, {an.numel()} transforms and {weight.numel()} scene weights")
    need = workspace_bytes(N, 1)
    with torch.cuda.device(dev):
        ws = _workspace(dev, need)
        paths = torch.empty((3, N), dtype=torch.float64, device=dev)
        _hip.check(_hip.lib().nunif_hip_stlizer_pass3_prepare(_ptr(sx), _ptr(sy), _ptr(an), _ptr(weight), N, _ptr(paths), _ptr(ws),
                                                             ws.numel(), _hip.current_stream_ptr(dev)))
    return paths


def pass3_smoothing(shift_x, shift_y, angle, scene_weight, method, smoothing_seconds, fps, resolution, device):
    """``pass3_smoothing`` (:337-349).  The angle limit of ``pass3`` (:359) is part of the engine's preparation: it changes nothing
    for an angle that ``pass3`` has already clamped."""
    paths = prepare(shift_x, shift_y, angle, scene_weight)
    if method in {"gaussian", "savgol"}:
        return conv1d_smoothing(paths[0], paths[1], paths[2], method, smoothing_seconds, fps, device)
    elif method == "grad_opt":
        return grad_opt(paths[0], paths[1], paths[2], scene_weight, resolution, penalty_weight=2e-3 / smoothing_seconds)


def pass3(transforms, scene_weight, fps, args, host=False):
    """``pass3`` (:352-366).  ``host=True``: three Python lists after one device-to-host read (what pass 4's per-frame loop reads)."""
    device = args.state["device"]
    if torch.device(device).type != "cuda":
        raise RuntimeError(f"pass3: device {device}; the HIP engine needs a ROCm device and has no CPU fallback")
    flat = torch.tensor([[rec[0][0] for rec in transforms], [rec[0][1] for rec in transforms], [rec[2] for rec in transforms]],
                        dtype=torch.float64).to(device)
    fixes = pass3_smoothing(flat[0], flat[1], flat[2], scene_weight, resolution=args.resolution, method=args.filter,
                            smoothing_seconds=args.smoothing, fps=fps, device=device)
    if host:
        rows = torch.stack(list(fixes)).cpu().tolist()
        return rows[0], rows[1], rows[2]
    return fixes
