"""The per-frame step of ``iw3 --export`` / ``--export-disparity`` on the HIP engine: what the ``_postprocess`` closures of
``bind_export_single_frame_callback`` / ``bind_export_vda_frame_callback`` do (iw3/utils.py:1374-1398 and :1438-1462, reference),
with the two PNG files of a frame encoded on the device (nunif_amd/nunif/utils/png.py) instead of by libpng on the thread pool.

The depth maps of a batch are one ``encode`` call, the source frames another; the pool only writes finished bytes to disk.  The
PyAV decode loop, ``export_config.py`` and the import side stay the reference's.
"""
from os import path

import torch

from . import _ops
from .mapper import get_mapper
from ..nunif.utils.png import MAX_BATCH, PngEncoder

IMAGE_IO_QUEUE_MAX = 100                                         # iw3/utils.py:52

_ENCODERS = {}


def _encoder(device):
    device = torch.device(device)
    if device.type == "cuda" and device.index is None:
        device = torch.device("cuda", torch.cuda.current_device())
    if device not in _ENCODERS:
        _ENCODERS[device] = PngEncoder(device)
    return _ENCODERS[device]


def _depth_text(png_info, min_depth_value, max_depth_value):
    info = dict(png_info or {})
    if min_depth_value is not None:
        info.update(iw3_min_depth_value=float(min_depth_value))
    if max_depth_value is not None:
        info.update(iw3_max_depth_value=float(max_depth_value))
    return info


def encode_normalized_depth(depth, png_info={}, min_depth_value=None, max_depth_value=None):
    """The file ``BaseDepthModel.save_normalized_depth`` writes (iw3/base_depth_model.py:197-210) as ``bytes``: ``depth``
    [1,H,W] on the device, clamped to [0,1], fp32 ``0xffff * depth`` truncated to 16 bits, the same text entries."""
    if depth.ndim != 3 or depth.shape[0] != 1:
        raise ValueError(f"a normalized depth is [1,H,W], got {tuple(depth.shape)}")
    return _encoder(depth.device).encode(depth, text=_depth_text(png_info, min_depth_value, max_depth_value))


def _encode_all(enc, x, text):
    """One ``encode`` call per form, or one per MAX_BATCH frames of a longer batch."""
    out = []
    for i in range(0, x.shape[0], MAX_BATCH):
        out += enc.encode(x[i:i + MAX_BATCH], text=text)
    return out


def _write(file_path, data):
    with open(file_path, "wb") as f:
        f.write(data)


class ExportWriter():
    """``write(frames, depths, pts_list)``: ``frames`` the uint8 source frames [H,W,3] of a batch (a list, or one [B,H,W,3]
    tensor; host frames are moved to the depth's device), ``depths`` the normalized depth maps [1,h,w] on the device, ``pts_list``
    the presentation time stamps.  ``args`` carries ``export_disparity``, ``mapper``, ``export_depth_fit`` and
    ``export_depth_only`` as in the reference."""

    def __init__(self, rgb_dir, depth_dir, pool, args, png_info=None):
        self.rgb_dir, self.depth_dir, self.pool, self.args = rgb_dir, depth_dir, pool, args
        self.png_info = dict(png_info or {})
        self.futures = []

    def _submit(self, file_path, data):
        self.futures.append(self.pool.submit(_write, file_path, data))

    def drain(self):
        for f in self.futures:
            f.result()
        self.futures.clear()

    def write(self, frames, depths, pts_list, min_depth_value=None, max_depth_value=None):
        depths = list(depths)
        if len(depths) == 0:
            return None
        frames = list(frames)
        if not (len(frames) == len(depths) == len(pts_list)):
            raise ValueError(f"{len(frames)} frames, {len(depths)} depth maps and {len(pts_list)} time stamps")
        args, device = self.args, depths[0].device
        depth = torch.stack([d.to(torch.float32) for d in depths])                 # [B,1,h,w]
        if args.export_disparity:
            depth = get_mapper(args.mapper)(depth)
        if args.export_depth_fit:
            # TF.resize(..., BILINEAR, antialias=True), iw3/utils.py:1381
            depth = _ops.resize_aa(depth, (frames[0].shape[0], frames[0].shape[1]), mode="bilinear", align_corners=False)
        enc = _encoder(device)
        text = _depth_text(self.png_info, min_depth_value, max_depth_value)
        names = [str(pts).zfill(8) + ".png" for pts in pts_list]
        for name, data in zip(names, _encode_all(enc, depth, text)):
            self._submit(path.join(self.depth_dir, name), data)
        if not args.export_depth_only:
            rgb = torch.stack([torch.as_tensor(x) for x in frames]).to(device)      # [B,H,W,3] uint8
            for name, data in zip(names, _encode_all(enc, rgb, None)):
                self._submit(path.join(self.rgb_dir, name), data)
        if len(self.futures) >= IMAGE_IO_QUEUE_MAX:
            self.drain()
        return None
