from . import da3mono_disparity, depth_aa, light_inpaint_v1, light_video_inpaint_v1, mlbw, row_flow_v2, row_flow_v3, sod_v1  # noqa: F401  (registers iw3.depth_aa, sbs.row_flow_v2, sbs.row_flow_v3, sbs.mlbw, inpaint.light_inpaint_v1, iw3.sod_v1, iw3.da3mono_disparity)
from .da3mono_disparity import DA3MonoDisparity  # noqa: F401
from .depth_aa import DepthAA  # noqa: F401
from .sod_v1 import SODV1  # noqa: F401
