from . import light_outpaint_v1  # noqa: F401  (registers stlizer.light_outpaint_v1)
from .light_outpaint_v1 import LightOutpaintV1  # noqa: F401
