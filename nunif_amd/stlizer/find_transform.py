"""stlizer pass 2 on the HIP engine: the batch form of the reference's ``find_transform`` (``nunif/utils/superpoint.py:233-327``)
and the ``pack_points`` / ``pass2`` of ``stlizer/multipass_pipeline.py:224-269`` around it.

The reference runs ``iteration`` Adam steps as a torch autograd loop, a few dozen launches per step over a few KB of data, and
``pass2`` then reads every pair's answer back with one ``.item()`` / ``.tolist()`` each.  Here a batch is ``iteration + 1`` launches
of one kernel (``nunif_hip_find_transform``, one workgroup per pair) and one device-to-host read.

``nunif_amd.install()`` does not bind this: under it ``KU.find_transform`` stays the reference's function (its non-batch CPU form
has no engine counterpart).  This module is the engine-side public form, like ``OutpaintBorder``.
"""
import ctypes

import torch

from .. import _hip

FLAG_DISABLE_SHIFT, FLAG_DISABLE_SCALE, FLAG_DISABLE_ROTATE, FLAG_SIGMA, FLAG_SIGMA_MIN = 1, 2, 4, 8, 16

MAX_WORKSPACES = 8
_workspaces = {}           # (device index, stream) -> uint8 tensor, grown by size; at most MAX_WORKSPACES, oldest dropped first


def _ptr(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else None


def workspace_bytes(B, N, iteration):
    """``nunif_hip_find_transform_workspace_bytes``; raises for a shape beyond the limits."""
    n = _hip.lib().nunif_hip_find_transform_workspace_bytes(B, N, iteration)
    if n < 0:
        raise ValueError(f"find_transform: B={B} N={N} iteration={iteration} is outside 1 <= B <= 4096, 1 <= N <= 8192, "
                         "1 <= iteration <= 1024")
    return n


def _workspace(device, nbytes):
    # One per device and stream, not per device alone: calls on two streams may overlap, and the caching allocator hands a dropped
    # block only to the stream it was allocated on, so growing or evicting one while its last call still runs is safe.  Handles of
    # short-lived streams would pile up, hence the cap.
    key = (device.index, torch.cuda.current_stream(device).cuda_stream)
    ws = _workspaces.pop(key, None)
    if ws is None or ws.numel() < nbytes:
        ws = torch.empty(nbytes, dtype=torch.uint8, device=device)
    _workspaces[key] = ws                                   # most recently used last
    while len(_workspaces) > MAX_WORKSPACES:
        del _workspaces[next(iter(_workspaces))]
    return ws


def _check_input(name, t):
    if not torch.is_tensor(t) or t.ndim != 3 or t.shape[-1] != 2:
        raise RuntimeError(f"find_transform: {name} must be a [B, N, 2] tensor: the engine has the batch form of "
                           "nunif.utils.superpoint.find_transform only (its 2-D form runs on the CPU in the reference)")
    if t.device.type != "cuda":
        raise RuntimeError(f"find_transform: {name} is on {t.device}; the HIP engine needs a ROCm device tensor and has no CPU "
                           "fallback (use nunif.utils.superpoint.find_transform there)")
    if t.dtype != torch.float32:
        raise RuntimeError(f"find_transform: {name} is {t.dtype}; nunif.utils.superpoint.find_transform optimises fp32 parameters "
                           "and the engine takes fp32 points only")


def find_transform_traced(xy1, xy2, center, mask=None, iteration=50, lr_translation=0.1, lr_scale_rotation=0.1,
                          sigma=None, sigma_min=None, sigma_max=2.0,
                          disable_shift=False, disable_scale=False, disable_rotate=False, trace=False, workspace=None):
    """``find_transform`` that can also return the (tx, ty, scale, rotation) of every pair after every step,
    ``[iteration, B, 4]`` (tests), and take a caller's ``workspace`` (uint8 device tensor)."""
    _check_input("xy1", xy1)
    _check_input("xy2", xy2)
    if xy1.shape != xy2.shape or xy1.device != xy2.device:
        raise RuntimeError(f"find_transform: xy1 {tuple(xy1.shape)} on {xy1.device} and xy2 {tuple(xy2.shape)} on {xy2.device} differ")
    device = xy1.device
    B, N, _ = xy1.shape
    iteration = int(iteration)
    xy1, xy2 = xy1.contiguous(), xy2.contiguous()
    if not torch.is_tensor(center):
        center = torch.tensor(center, dtype=torch.float32, device=device)
    center = center.to(device=device, dtype=torch.float32).reshape(-1, 2).expand(B, 2).contiguous()
    mask_u8 = None
    if mask is not None:
        if mask.shape != xy1.shape:
            raise RuntimeError(f"find_transform: mask {tuple(mask.shape)} does not match the points {tuple(xy1.shape)}")
        mask_u8 = mask.to(device=device, dtype=torch.bool).contiguous().view(torch.uint8)
    flags = ((FLAG_DISABLE_SHIFT if disable_shift else 0) | (FLAG_DISABLE_SCALE if disable_scale else 0) |
             (FLAG_DISABLE_ROTATE if disable_rotate else 0) | (FLAG_SIGMA if sigma is not None else 0) |
             (FLAG_SIGMA_MIN if sigma_min is not None else 0))
    need = workspace_bytes(B, N, iteration)
    with torch.cuda.device(device):
        ws = workspace if workspace is not None else _workspace(device, need)
        flat = torch.empty(4 * B, dtype=torch.float32, device=device)      # shift [B, 2] | scale [B] | angle [B]
        tr = torch.empty((iteration, B, 4), dtype=torch.float32, device=device) if trace else None
        _hip.check(_hip.lib().nunif_hip_find_transform(
            _ptr(xy1), _ptr(xy2), _ptr(mask_u8), _ptr(center), B, N, iteration, float(lr_translation), float(lr_scale_rotation),
            float(sigma if sigma is not None else 0.0), float(sigma_min if sigma_min is not None else 0.0), float(sigma_max), flags,
            _ptr(flat), ctypes.c_void_p(flat.data_ptr() + 8 * B), ctypes.c_void_p(flat.data_ptr() + 12 * B),
            _ptr(ws), ws.numel(), _ptr(tr), _hip.current_stream_ptr(device)))
    shift, scale, angle = flat[:2 * B].view(B, 2), flat[2 * B:3 * B].view(B, 1), flat[3 * B:].view(B, 1)
    return shift, scale, angle, center, tr


def find_transform(xy1, xy2, center, mask=None, iteration=50, lr_translation=0.1, lr_scale_rotation=0.1,
                   sigma=None, sigma_min=None, sigma_max=2.0,
                   disable_shift=False, disable_scale=False, disable_rotate=False):
    """The batch form of ``nunif.utils.superpoint.find_transform`` (:233-327): ``xy1`` / ``xy2`` [B, N, 2] fp32 on a ROCm device,
    ``center`` [B, 2] (or anything that reshapes to it), ``mask`` [B, N, 2] bool or None.  Returns ``(shift [B, 2], scale [B, 1],
    angle [B, 1] in degrees, center [B, 2])`` as device tensors, without a host synchronisation.  It needs no grad mode.  A 2-D
    input, a host tensor or another dtype raises: there is no CPU fallback."""
    return find_transform_traced(xy1, xy2, center, mask, iteration, lr_translation, lr_scale_rotation, sigma, sigma_min, sigma_max,
                                 disable_shift, disable_scale, disable_rotate)[:4]


def pack_points(batch1, batch2):
    """``multipass_pipeline.pack_points`` (:224-243): zero-padded ``[B, longest, 2]`` points of both sides and their bool mask."""
    fixed_size = max(max(pts.shape[0] for pts in batch1), max(pts.shape[0] for pts in batch2))
    packed1, packed2, masks = [], [], []
    for pts1, pts2 in zip(batch1, batch2):
        assert pts1.shape[0] == pts2.shape[0]
        n = pts1.shape[0]
        p1 = torch.zeros((fixed_size, pts1.shape[1]), dtype=pts1.dtype, device=pts1.device)
        p2 = torch.zeros((fixed_size, pts1.shape[1]), dtype=pts1.dtype, device=pts1.device)
        m = torch.zeros((fixed_size, pts1.shape[1]), dtype=torch.bool, device=pts1.device)
        p1[:n], p2[:n], m[:n] = pts1, pts2, True
        packed1.append(p1)
        packed2.append(p2)
        masks.append(m)
    return torch.stack(packed1), torch.stack(packed2), torch.stack(masks)


def pass2(points1, points2, center, resize_scale, args):
    """``multipass_pipeline.pass2`` (:246-269): the per-frame ``(shift [x, y], scale, angle, center, resize_scale)`` tuples of a
    video from pass 1's matched points, ``args.batch_size * 32`` pairs per ``find_transform`` call (``args.iteration`` steps,
    ``sigma=2.0``, ``disable_scale=True``), packed to the whole video's longest pair first.  One device-to-host read per batch."""
    device = args.state["device"]
    if len(points1) == 0:
        return []
    transforms = []
    points1, points2, masks = pack_points(points1, points2)
    batch_size = args.batch_size * 32
    for kp1, kp2, mask in zip(points1.split(batch_size), points2.split(batch_size), masks.split(batch_size)):
        kp1, kp2, mask = kp1.to(device), kp2.to(device), mask.to(device)
        center_batch = torch.tensor(center, dtype=torch.float32, device=device).view(1, 2).expand(kp1.shape[0], 2)
        shift, scale, angle, _ = find_transform(kp1, kp2, center=center_batch, mask=mask, iteration=args.iteration, sigma=2.0,
                                                disable_scale=True)
        rows = torch.cat([shift, scale, angle], dim=1).cpu().tolist()
        transforms.extend(([row[0], row[1]], row[2], row[3], center, resize_scale) for row in rows)
    return transforms
