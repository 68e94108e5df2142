"""``cliqa/utils.py`` (reference) on the HIP engine: patch selection (``extract_patches`` :36-57 with ``std_score`` :26-27) as two
launches on the device, and the ``predict_*`` functions :60-99 with the reference's signatures, return values and clamps.

``tv_score`` (:30-33) is not carried: in the reference it reads an undefined name and raises ``NameError``, so its
``predict_resize_quality`` does not work on a PIL image either; here that call selects by ``std_score`` like the other two.
``PatchDataset`` / ``create_patch_loader`` are host-side data loading and stay the reference's.

``predict_*_batch(model, patches[N,K,3,P,P])`` scores N images in one forward and returns tensors (no ``.item()`` per image); the
per-image functions are the N = 1 case of them.
"""
import ctypes

import numpy as np
import torch

from .. import _hip
from ..nunif.models import get_model_device

PATCH_SIZE = 128


def safe_pad(im, min_size):
    """:19-23 on an ``[H,W,C]`` array: reflect padding at the right / bottom of an image smaller than a patch (a host step)."""
    h, w = im.shape[:2]
    if h < min_size or w < min_size:
        im = np.pad(im, ((0, max(0, min_size - h)), (0, max(0, min_size - w)), (0, 0)), mode="reflect")
    return im


def std_score(patches):
    return torch.std(patches, dim=[2, 3]).mean(dim=1)


def select_patches(image, num_patches, patch_size=PATCH_SIZE):
    """image ``[3,H,W]`` fp32 on a ROCm device -> ``(patches [K,3,P,P], indices [K] int64, scores [n])``: the non-overlapping
    patches in row-major order (partial ones dropped), their ``std_score``, the top ``K = min(num_patches, n)`` in descending order."""
    if not (isinstance(image, torch.Tensor) and image.is_cuda):
        raise RuntimeError("cliqa patch selection runs on a ROCm device tensor; there is no CPU fallback")
    assert image.ndim == 3 and image.shape[0] == 3, "image: [3,H,W]"
    image = image.to(torch.float32).contiguous()
    _, H, W = image.shape
    if H < patch_size or W < patch_size:
        raise ValueError(f"image {H}x{W} is smaller than a patch of {patch_size}: pad it on the host (safe_pad)")
    n = (H // patch_size) * (W // patch_size)
    K = min(int(num_patches), n)
    dev = image.device
    scores = torch.empty((n,), dtype=torch.float32, device=dev)
    indices = torch.empty((K,), dtype=torch.int64, device=dev)
    patches = torch.empty((K, 3, patch_size, patch_size), dtype=torch.float32, device=dev)
    with torch.cuda.device(dev):
        _hip.check(_hip.lib().nunif_hip_cliqa_select_patches(
            ctypes.c_void_p(image.data_ptr()), H, W, int(patch_size), int(num_patches), ctypes.c_void_p(scores.data_ptr()),
            ctypes.c_void_p(indices.data_ptr()), ctypes.c_void_p(patches.data_ptr()), _hip.current_stream_ptr(dev)))
    return patches, indices, scores


def extract_patches(im, num_patches, patch_size=PATCH_SIZE, score_fn=std_score, device=None):
    """:36-57.  ``im``: a PIL image (converted and padded on the host, then uploaded to ``device``, default the current ROCm device)
    or a ``[3,H,W]`` tensor on a ROCm device (one smaller than a patch is refused).  Only ``std_score`` is built."""
    if score_fn is not std_score:
        raise NotImplementedError("cliqa.extract_patches on the HIP engine scores by std_score only")
    if not isinstance(im, torch.Tensor):
        arr = safe_pad(np.asarray(im.convert("RGB")), patch_size)
        im = torch.from_numpy(np.ascontiguousarray(arr)).to(device or "cuda").permute(2, 0, 1).float().div_(255.0)
    return select_patches(im, num_patches, patch_size)[0]


def _forward_images(model, patches):
    assert patches.ndim == 5 and patches.shape[2] == 3, "patches: [N,K,3,P,P]"
    N, K = patches.shape[:2]
    out = model(patches.to(get_model_device(model)).reshape(N * K, *patches.shape[2:]))
    return [o.float().reshape(N, K) for o in (out if isinstance(out, (tuple, list)) else (out,))]


def predict_jpeg_quality_batch(model, patches):
    """-> ``(quality [N] in [0, 100], subsampling probability [N])``."""
    quality, subsampling = _forward_images(model, patches)
    return torch.clamp(quality.mean(dim=1), 0, 100), torch.sigmoid(subsampling).mean(dim=1)


def predict_grain_noise_psnr_batch(model, patches):
    """-> PSNR ``[N]`` = 50 - noise level clamped to [0, 50]."""
    noise_level, = _forward_images(model, patches)
    return 50. - torch.clamp(noise_level.mean(dim=1), 0, 50)


def predict_resize_quality_batch(model, patches):
    """-> the smallest scale factor per image ``[N]`` (the net clamps to [1, 2]) and the resize quality ``[N]`` int64."""
    scale_factor, = _forward_images(model, patches)
    scale_factor = scale_factor.min(dim=1).values
    return scale_factor, 100 - ((scale_factor.double() - 1.0) * 100).to(torch.int64)


def _patches_of(model, x, num_patches, patch_size):
    if not isinstance(x, torch.Tensor):
        x = extract_patches(x, num_patches, patch_size, device=get_model_device(model))
    return x[None]


def predict_jpeg_quality(model, x, num_patches=8, patch_size=PATCH_SIZE):
    quality, subsampling_prob = predict_jpeg_quality_batch(model, _patches_of(model, x, num_patches, patch_size))
    quality = quality[0].item()
    subsampling_prob = subsampling_prob[0].item()

    return quality, subsampling_prob


def predict_grain_noise_psnr(model, x, num_patches=8, patch_size=PATCH_SIZE):
    psnr = predict_grain_noise_psnr_batch(model, _patches_of(model, x, num_patches, patch_size))[0].item()

    return psnr


def predict_resize_quality(model, x, num_patches=8, patch_size=PATCH_SIZE):
    scale_factor = predict_resize_quality_batch(model, _patches_of(model, x, num_patches, patch_size))[0][0].item()
    resize_quality = 100 - int((scale_factor - 1.0) * 100)

    return resize_quality
