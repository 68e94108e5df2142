from .jpeg_quality import JPEGQuality
from .grain_noise_level import GrainNoiseLevel
from .scale_factor import ScaleFactor

__all__ = ["JPEGQuality", "GrainNoiseLevel", "ScaleFactor"]
