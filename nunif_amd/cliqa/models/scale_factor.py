"""``cliqa.scale_factor`` on the HIP engine.  Mirrors ``cliqa/models/scale_factor.py`` (reference) ``ScaleFactor`` :10-63: registry
name, ``state_dict`` key layout (its convs carry a bias as well as BatchNorm), ``preprocess`` :48-51 and the eval-mode ``forward``
-> scale factor ``[B,1]`` clamped to [1, 2] :53-63, fp32.  Inference only."""
from ...nunif.models import register_model
from ._net import CliqaNet


@register_model
class ScaleFactor(CliqaNet):
    name = "cliqa.scale_factor"
    kind = "scale_factor"

    @staticmethod
    def preprocess(x):
        x = x * 2. - 1.
        return x
