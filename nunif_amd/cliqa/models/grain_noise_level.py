"""``cliqa.grain_noise_level`` on the HIP engine.  Mirrors ``cliqa/models/grain_noise_level.py`` (reference) ``GrainNoiseLevel``
:8-58: registry name, ``state_dict`` key layout, ``preprocess`` :48-50 and ``forward`` -> noise level ``[B,1]`` :52-58, fp32.
Inference only."""
from ...nunif.models import register_model
from ._net import CliqaNet


@register_model
class GrainNoiseLevel(CliqaNet):
    name = "cliqa.grain_noise_level"
    kind = "grain_noise_level"

    @staticmethod
    def preprocess(x):
        x = x * 2. - 1.
        return x
