"""stlizer on the HIP engine: the outpaint network and the border step of pass 4 (the keypoint network, matching and the
stabilising warp are in nunif_amd/nunif/utils/superpoint.py, where the reference keeps them)."""
from .find_transform import find_transform, pack_points, pass2  # noqa: F401
from .pass3 import calc_scene_weight, conv1d_smoothing, gen_smoothing_kernel, grad_opt, pass3_smoothing  # noqa: F401  (pass3 itself: .pass3.pass3, the name is the module's)
