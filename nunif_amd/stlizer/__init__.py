"""stlizer on the HIP engine: the outpaint network and the border step of pass 4 (the keypoint network, matching and the
stabilising warp are in nunif_amd/nunif/utils/superpoint.py, where the reference keeps them)."""
from .find_transform import find_transform, pack_points, pass2  # noqa: F401
