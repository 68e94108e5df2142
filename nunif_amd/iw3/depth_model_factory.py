"""``--depth-model`` -> depth model object.  Mirrors ``iw3/depth_model_factory.py`` :10-33 (first class whose ``supported``
accepts the name) for the model families the HIP engine carries, ``ZoeD_Any_N`` / ``ZoeD_Any_K`` (the reference CLI's default;
Depth-Anything V1 under ZoeDepth's metric-bins head, ``zoedepth_model.py``) among them.  The BEiT ZoeDepth names (``ZoeD_N`` /
``ZoeD_K`` / ``ZoeD_NK``) and DepthPro are external ``torch.hub`` nets that are not restated and raise
``ValueError`` like an unknown name does in the reference.  ``Any_V3_Mono`` / ``Any_V3_Mono_01`` resolve to the engine's wrapper
(``depth_anything_v3_model.py``): everything around the DA3 backbone runs here, the backbone itself comes from a local hub checkout."""
from .depth_anything_v3_model import DepthAnythingV3MonoModel
from .named_depth_models import DepthAnythingModel, NullDepthModel
from .video_depth_anything_model import VideoDepthAnythingModel
from .video_depth_anything_streaming_model import VideoDepthAnythingStreamingModel
from .zoedepth_model import ZoeDepthModel


def create_depth_model(model_type):
    for cls in (ZoeDepthModel, DepthAnythingModel, DepthAnythingV3MonoModel, VideoDepthAnythingModel, VideoDepthAnythingStreamingModel,
                NullDepthModel):
        if cls.supported(model_type):
            return cls(model_type)
    raise ValueError(f"{model_type} is not supported")
