"""``to_uint8`` and ``to_jpeg_data`` of ``iw3/desktop/utils.py`` (reference :99-100, :110-123) on the HIP engine.

The reference encodes every streamed frame with ``torchvision.io.encode_jpeg``; its device route is nvjpeg, which ROCm does not
have, so there the whole uint8 frame goes to the host and through libjpeg.  Here a device frame is encoded on the device
(nunif_amd/nunif/utils/jpeg.py) and only the stream crosses.  ``gpu_jpeg=False`` or a host frame takes the host route, through
PIL's libjpeg, as the reference's ``else`` branch does with torchvision's."""
import io
import threading

import torch

from ...nunif.utils.jpeg import JpegEncoder

_jpeg_encode_lock = threading.Lock()
_encoders = {}                       # one per device, used under the lock


def to_uint8(x):
    return x.mul(255).round_().to(torch.uint8)


def _encoder(device):
    enc = _encoders.get(device)
    if enc is None:
        enc = _encoders[device] = JpegEncoder(device)
    return enc


def _host_jpeg(frame, quality):
    from PIL import Image
    bio = io.BytesIO()
    Image.fromarray(to_uint8(frame).cpu().permute(1, 2, 0).contiguous().numpy()).save(bio, "JPEG", quality=quality)
    return bio.getvalue()


def to_jpeg_data(frame, quality, tick, gpu_jpeg=True):
    with _jpeg_encode_lock:
        if gpu_jpeg and frame.device.type == "cuda":
            if frame.shape[0] != 3:
                raise ValueError(f"to_jpeg_data needs an RGB frame [3,H,W], got {tuple(frame.shape)}")
            jpeg_data = _encoder(frame.device).encode(frame, quality=quality)
        else:
            jpeg_data = _host_jpeg(frame, quality)
    return (jpeg_data, tick)
