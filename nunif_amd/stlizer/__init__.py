"""stlizer on the HIP engine: the outpaint network and the border step of pass 4 (the keypoint network, matching and the
stabilising warp are in nunif_amd/nunif/utils/superpoint.py, where the reference keeps them)."""
