"""``cliqa.jpeg_quality`` on the HIP engine.  Mirrors ``cliqa/models/jpeg_quality.py`` (reference) ``JPEGQuality`` :8-75: registry
name, ``state_dict`` key layout (``num_batches_tracked`` included, so a reference ``.pth`` loads unchanged and vice versa),
``preprocess`` :57-68 as a static method and ``forward`` -> ``(quality [B,1], subsampling [B,1])`` :70-75, fp32.  Inference only."""
import torch

from ...nunif.models import register_model
from ._net import CliqaNet


@register_model
class JPEGQuality(CliqaNet):
    name = "cliqa.jpeg_quality"
    kind = "jpeg_quality"

    @staticmethod
    def preprocess(x):
        r = x[:, 0:1, :, :]
        g = x[:, 1:2, :, :]
        b = x[:, 2:3, :, :]

        y = r * 0.299 + g * 0.587 + b * 0.114
        cb = (b - y) * 0.564 + 0.5
        cr = (r - y) * 0.713 + 0.5

        x = torch.cat([y, cb, cr, r, g, b], dim=1)
        x = x * 2. - 1.
        return x
