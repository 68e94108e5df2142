"""``--depth-model`` -> depth model object.  Mirrors ``iw3/depth_model_factory.py`` :10-33 (first class whose ``supported``
accepts the name) for the model families the HIP engine carries, ``ZoeD_Any_N`` / ``ZoeD_Any_K`` (the reference CLI's default;
Depth-Anything V1 under ZoeDepth's metric-bins head, ``zoedepth_model.py``) among them.  The BEiT ZoeDepth names (``ZoeD_N`` /
``ZoeD_K`` / ``ZoeD_NK``), DepthPro and DA3 are external ``torch.hub`` nets that are not restated and raise
``ValueError`` like an unknown name does in the reference."""
from .named_depth_models import DepthAnythingModel, NullDepthModel
from .video_depth_anything_model import VideoDepthAnythingModel
from .video_depth_anything_streaming_model import VideoDepthAnythingStreamingModel
from .zoedepth_model import ZoeDepthModel


def create_depth_model(model_type):
    for cls in (ZoeDepthModel, DepthAnythingModel, VideoDepthAnythingModel, VideoDepthAnythingStreamingModel, NullDepthModel):
        if cls.supported(model_type):
            return cls(model_type)
    raise ValueError(f"{model_type} is not supported")
