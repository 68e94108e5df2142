"""ctypes binding of ``libnunif_hip.so`` (the C ABI declared in ``include/nunif_hip.h``).

There is no CPU fallback: if the library is missing or a call fails this module raises.  The library is built
in-tree by ``python -m nunif_amd.build`` (or ``__graft_entry__.build()``).
"""
import ctypes
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
# NUNIF_HIP_LIB: another build of the same ABI (same-box A/B runs of two kernel versions, tools/ab_lib.sh); never a fallback
LIB_PATH = os.environ.get("NUNIF_HIP_LIB") or os.path.join(_HERE, "libnunif_hip.so")

c_void_p, c_int32, c_int64, c_float, c_char_p, c_double, c_uint64 = (
    ctypes.c_void_p, ctypes.c_int32, ctypes.c_int64, ctypes.c_float, ctypes.c_char_p, ctypes.c_double, ctypes.c_uint64)


class NunifHipError(RuntimeError):
    def __init__(self, status, message):
        super().__init__(f"libnunif_hip error {status}: {message}")
        self.status = status


class TileGrid(ctypes.Structure):
    """``nunif_tile_grid`` — the integer outputs of SeamBlending.create_config (seam_blending.py:109-143)."""
    _fields_ = [(n, c_int32) for n in (
        "x_h", "x_w", "scale", "offset", "tile_size", "blend_size",
        "y_h", "y_w", "h_blocks", "w_blocks",
        "pad_l", "pad_r", "pad_t", "pad_b", "y_buffer_h", "y_buffer_w",
        "input_tile_step", "output_tile_step", "out_tile_size")]

    def as_config(self):
        return {"y_h": self.y_h, "y_w": self.y_w, "h_blocks": self.h_blocks, "w_blocks": self.w_blocks,
                "pad": (self.pad_l, self.pad_r, self.pad_t, self.pad_b),
                "y_buffer_h": self.y_buffer_h, "y_buffer_w": self.y_buffer_w,
                "input_tile_step": self.input_tile_step, "output_tile_step": self.output_tile_step}


class SwinBlockExtent(ctypes.Structure):
    """``nunif_swin_block_extent``: per axis (rows, columns) the leading windows of a block that run and whether its wrap window does."""
    _fields_ = [("n_win", c_int32 * 2), ("wrap", c_int32 * 2)]


class SwinTailGroup(ctypes.Structure):
    """``nunif_swin_tail_group``: up to 16 token slots of the C = 192 tail as contiguous pieces (see ``include/nunif_hip.h``)."""
    _fields_ = [("adj", c_int32 * 6), ("bounds", ctypes.c_uint32), ("reserved", ctypes.c_uint32)]

    def tokens(self):
        cnt = (self.bounds >> 25) & 31
        firsts = [0] + [(self.bounds >> (5 * p)) & 31 for p in range(5)]
        return [self.adj[max(p for p in range(6) if firsts[p] <= r)] + r for r in range(cnt)]


class TensorDesc(ctypes.Structure):
    _fields_ = [("name", c_char_p), ("data", c_void_p), ("ndim", c_int32), ("shape", c_int64 * 4)]


class ForwardWarpParams(ctypes.Structure):
    _fields_ = [("B", c_int32), ("H", c_int32), ("W", c_int32), ("divergence", c_double), ("convergence", c_double),
                ("fill", c_int32), ("synthetic_view", c_int32), ("width_base", c_int32), ("convergence_dev", c_void_p)]


class Hdr2SdrParams(ctypes.Structure):
    """``nunif_hdr2sdr_params``: exposure and white point of the curve in use, and hlg_saturation_gain (video.py:311-312)."""
    _fields_ = [("exposure", c_double), ("white_point", c_double), ("saturation_gain", c_double)]


class PixfmtPlanes(ctypes.Structure):
    """``nunif_pixfmt_planes``: the three plane pointers of a planar YUV frame and their byte pitches (PyAV's ``line_size``)."""
    _fields_ = [("data", c_void_p * 3), ("pitch", c_int64 * 3)]


class DaFeatures(ctypes.Structure):
    """``nunif_da_features``: the six NHWC fp16 maps the Depth-Anything engine leaves for ZoeDepth's head, and their sizes."""
    _fields_ = [("outconv", c_void_p), ("bottleneck", c_void_p), ("blocks", c_void_p * 4), ("bh", c_int32), ("bw", c_int32),
                ("rh", c_int32 * 4), ("rw", c_int32 * 4), ("channels", c_int32)]


class ProfRecord(ctypes.Structure):
    _fields_ = [("name", ctypes.c_char * 48), ("total_ms", c_double), ("launches", c_int64),
                ("flops", c_double), ("bytes", c_double)]


# name -> (restype, argtypes); every symbol include/nunif_hip.h declares
SIGNATURES = {
    "nunif_hip_abi_version": (c_int32, []),
    "nunif_hip_last_error": (c_char_p, []),
    "nunif_hip_tile_grid_init": (c_int32, [c_int32] * 6 + [ctypes.POINTER(TileGrid)]),
    "nunif_hip_blend_ramp": (c_int32, [c_int32, ctypes.POINTER(c_float)]),
    "nunif_hip_gather_tiles": (c_int32, [c_void_p, c_void_p, ctypes.POINTER(TileGrid), c_int32, c_int32, c_int32, c_void_p]),
    "nunif_hip_stitch_tiles": (c_int32, [c_void_p, c_void_p, ctypes.POINTER(TileGrid), c_int32, c_void_p]),
    "nunif_hip_swin_unet_create": (c_int32, [ctypes.POINTER(TensorDesc), c_int32, c_int32, ctypes.POINTER(c_void_p)]),
    "nunif_hip_swin_unet_destroy": (None, [c_void_p]),
    "nunif_hip_swin_unet_forward": (c_int32, [c_void_p, c_void_p, c_void_p, c_int32, c_int32, c_void_p]),
    "nunif_hip_swin_unet_render": (c_int32, [c_void_p, c_void_p, c_void_p, c_int32, c_int32, c_int32, c_int32, c_void_p]),
    "nunif_hip_swin_unet_render_tile_rows": (c_int32, [c_void_p, c_void_p, c_int32, c_int32, c_int32, c_int32, c_int32, c_int32, c_void_p]),
    "nunif_hip_swin_unet_tile_row_band": (c_int32, [c_void_p, c_int32, c_int32, c_int32, c_int32, c_int32, c_int32, c_void_p, c_int32, c_void_p]),
    "nunif_hip_swin_unet_stitch_rows": (c_int32, [c_void_p, c_void_p, c_int32, c_int32, c_int32, c_int32, c_int32, c_void_p]),
    "nunif_hip_swin_unet_tile_extents": (c_int32, [ctypes.POINTER(TileGrid), c_int32, ctypes.POINTER(c_int32), ctypes.POINTER(c_int32),
                                                   c_int32, ctypes.POINTER(SwinBlockExtent)]),
    "nunif_hip_swin_unet_tail_groups": (c_int32, [ctypes.POINTER(SwinBlockExtent), c_int32, c_int32, c_int32,
                                                  ctypes.POINTER(SwinTailGroup), c_int64, ctypes.POINTER(c_int64), ctypes.POINTER(c_int64)]),
    "nunif_hip_swin_unet_producer_tokens": (c_int32, [ctypes.POINTER(SwinBlockExtent), c_int32, ctypes.POINTER(c_int32), ctypes.POINTER(c_int32),
                                                      ctypes.POINTER(c_int32), c_int32, c_int32, c_int32, c_int32, c_int32,
                                                      ctypes.POINTER(ctypes.c_uint32), c_int64, ctypes.POINTER(c_int64)]),
    "nunif_hip_swin_unet_down2_test": (c_int32, [c_void_p, c_void_p, c_void_p, c_int32, c_int32, c_int32, c_int32, c_void_p]),
    "nunif_hip_swin_unet_tail192_test": (c_int32, [c_void_p, c_int32, c_int32, c_void_p, c_void_p, c_int64, c_void_p, c_int64, c_int64,
                                                   c_int32, c_void_p]),
    "nunif_hip_swin_unet_v2_create": (c_int32, [ctypes.POINTER(TensorDesc), c_int32, c_int32, ctypes.POINTER(c_void_p)]),
    "nunif_hip_swin_unet_v2_destroy": (None, [c_void_p]),
    "nunif_hip_swin_unet_v2_forward": (c_int32, [c_void_p, c_void_p, c_void_p, c_int32, c_int32, c_int32, c_void_p]),
    "nunif_hip_swin_unet_v2_debug_taps": (c_int32, [c_void_p, c_void_p, c_void_p, c_void_p, c_int32, c_int32, c_int32, c_void_p]),
    "nunif_hip_swin_unet_v2_debug_wattn": (c_int32, [c_void_p] * 4 + [c_int32] * 6 + [c_void_p]),
    "nunif_hip_wgmlp_create": (c_int32, [ctypes.POINTER(TensorDesc), c_int32, ctypes.POINTER(c_void_p)]),
    "nunif_hip_wgmlp_destroy": (None, [c_void_p]),
    "nunif_hip_wgmlp_forward": (c_int32, [c_void_p, c_void_p, c_void_p, c_int32, c_int32, c_int32, c_void_p]),
    "nunif_hip_wgmlp_debug_taps": (c_int32, [c_void_p, c_void_p, c_void_p, c_void_p, c_int32, c_int32, c_int32, c_void_p]),
    "nunif_hip_wgmlp_debug_gmlp": (c_int32, [c_void_p, c_int32, c_void_p, c_void_p] + [c_int32] * 4 + [c_void_p] * 6),
    "nunif_hip_cunet_create": (c_int32, [ctypes.POINTER(TensorDesc), c_int32, c_int32, ctypes.POINTER(c_void_p)]),
    "nunif_hip_cunet_destroy": (None, [c_void_p]),
    "nunif_hip_cunet_forward": (c_int32, [c_void_p, c_void_p, c_void_p, c_int32, c_int32, c_void_p]),
    "nunif_hip_cunet_render": (c_int32, [c_void_p, c_void_p, c_void_p, c_int32, c_int32, c_int32, c_int32, c_void_p]),
    "nunif_hip_forward_warp": (c_int32, [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p,
                                         ctypes.POINTER(ForwardWarpParams), c_void_p]),
    "nunif_hip_backward_warp": (c_int32, [c_void_p, c_void_p, c_void_p, c_void_p] + [c_int32] * 6 +
                                [c_double, c_double, c_int32, c_void_p, c_void_p]),
    "nunif_hip_row_flow_create": (c_int32, [ctypes.POINTER(TensorDesc), c_int32, ctypes.POINTER(c_void_p)]),
    "nunif_hip_row_flow_destroy": (None, [c_void_p]),
    "nunif_hip_row_flow_delta": (c_int32, [c_void_p, c_void_p, c_void_p, c_int32, c_int32, c_int32, c_int32, c_void_p]),
    "nunif_hip_row_flow_v2_create": (c_int32, [ctypes.POINTER(TensorDesc), c_int32, ctypes.POINTER(c_void_p)]),
    "nunif_hip_row_flow_v2_destroy": (None, [c_void_p]),
    "nunif_hip_row_flow_v2_delta": (c_int32, [c_void_p, c_void_p, c_void_p, c_int32, c_int32, c_int32, c_int32, c_void_p]),
    "nunif_hip_row_flow_v2_debug_taps": (c_int32, [c_void_p] * 9 + [c_int32] * 4 + [c_void_p]),
    "nunif_hip_delta_warp": (c_int32, [c_void_p, c_void_p, c_void_p] + [c_int32] * 6 + [c_double, c_int32, c_void_p]),
    "nunif_hip_mlbw_create": (c_int32, [ctypes.POINTER(TensorDesc), c_int32, ctypes.POINTER(c_void_p)]),
    "nunif_hip_mlbw_destroy": (None, [c_void_p]),
    "nunif_hip_mlbw_num_layers": (c_int32, [c_void_p]),
    "nunif_hip_mlbw_delta": (c_int32, [c_void_p, c_void_p, c_void_p, c_void_p, c_int32, c_int32, c_int32, c_int32, c_void_p]),
    "nunif_hip_light_inpaint_create": (c_int32, [ctypes.POINTER(TensorDesc), c_int32, ctypes.POINTER(c_void_p)]),
    "nunif_hip_light_inpaint_destroy": (None, [c_void_p]),
    "nunif_hip_light_inpaint_infer": (c_int32, [c_void_p, c_void_p, c_void_p, c_void_p] + [c_int32] * 6 + [c_void_p]),
    "nunif_hip_light_inpaint_infer_ex": (c_int32, [c_void_p, c_void_p, c_void_p, c_void_p] + [c_int32] * 7 + [c_void_p]),
    "nunif_hip_light_inpaint_debug_taps": (c_int32, [c_void_p, c_void_p, c_void_p, c_void_p] + [c_int32] * 7 +
                                           [ctypes.POINTER(c_void_p), c_int32, c_void_p]),
    "nunif_hip_anaglyph": (c_int32, [c_void_p, c_void_p, c_void_p, c_int32, c_int32, c_int32, c_void_p]),
    "nunif_hip_equirectangular": (c_int32, [c_void_p, c_void_p, c_int32, c_int32, c_int32, c_void_p]),
    "nunif_hip_mlbw_has_hole_mask": (c_int32, [c_void_p]),
    "nunif_hip_mlbw_delta_mask": (c_int32, [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int32, c_int32, c_int32, c_int32,
                                            c_void_p]),
    "nunif_hip_hole_mask_postprocess": (c_int32, [c_void_p, c_void_p, c_void_p] + [c_int32] * 5 + [c_float, c_int32, c_int32,
                                                  c_void_p, c_int32, c_void_p]),
    "nunif_hip_delta_weight_warp": (c_int32, [c_void_p, c_void_p, c_void_p, c_void_p] + [c_int32] * 7 +
                                    [c_double, c_int32, c_void_p]),
    "nunif_hip_depth_aa_create": (c_int32, [ctypes.POINTER(TensorDesc), c_int32, ctypes.POINTER(c_void_p)]),
    "nunif_hip_depth_aa_destroy": (None, [c_void_p]),
    "nunif_hip_depth_aa_forward": (c_int32, [c_void_p, c_void_p, c_void_p, c_int32, c_int32, c_int32, c_int32, c_void_p]),
    "nunif_hip_depth_anything_create": (c_int32, [ctypes.POINTER(TensorDesc), c_int32, ctypes.POINTER(c_void_p)]),
    "nunif_hip_depth_anything_create_ex": (c_int32, [ctypes.POINTER(TensorDesc), c_int32, ctypes.POINTER(c_int32), ctypes.c_float,
                                                     ctypes.POINTER(c_void_p)]),
    "nunif_hip_depth_anything_destroy": (None, [c_void_p]),
    "nunif_hip_depth_anything_forward": (c_int32, [c_void_p, c_void_p, c_void_p, c_void_p, c_int32, c_int32, c_int32, c_void_p]),
    "nunif_hip_depth_anything_reset_state": (c_int32, [c_void_p]),
    "nunif_hip_depth_anything_is_temporal": (c_int32, [c_void_p]),
    "nunif_hip_depth_anything_debug_temporal": (c_int32, [c_void_p, c_int32, c_void_p, c_void_p, c_int32, c_int32,
                                                          ctypes.POINTER(c_void_p), c_int32, c_void_p]),
    "nunif_hip_depth_anything_forward_features": (c_int32, [c_void_p, c_void_p, c_void_p, c_void_p, c_int32, c_int32, c_int32,
                                                            ctypes.POINTER(DaFeatures), c_void_p]),
    "nunif_hip_zoedepth_head_create": (c_int32, [ctypes.POINTER(TensorDesc), c_int32, c_float, c_float, c_float,
                                                 ctypes.POINTER(c_void_p)]),
    "nunif_hip_zoedepth_head_forward": (c_int32, [c_void_p, ctypes.POINTER(DaFeatures), c_void_p, c_void_p, c_int32, c_int32,
                                                  c_int32, c_void_p]),
    "nunif_hip_zoedepth_head_debug_taps": (c_int32, [c_void_p, c_int32, c_void_p, ctypes.POINTER(c_int32), c_void_p]),
    "nunif_hip_zoedepth_head_destroy": (None, [c_void_p]),
    "nunif_hip_zoedepth_pad_normalize": (c_int32, [c_void_p, c_void_p, c_int64] + [c_int32] * 6 + [c_void_p]),
    "nunif_hip_tta_view": (c_int32, [c_void_p, c_void_p, c_int32, c_int32, c_int32, c_int32, c_void_p]),
    "nunif_hip_tta_merge": (c_int32, [ctypes.POINTER(c_void_p), c_void_p, c_int32, c_int32, c_int32, c_void_p]),
    "nunif_hip_alpha_border_padding": (c_int32, [c_void_p, c_void_p, c_void_p, c_void_p, c_int32, c_int32, c_int32, c_void_p]),
    "nunif_hip_resize_aa": (c_int32, [c_void_p, c_void_p, c_void_p, c_int64] + [c_int32] * 7 +
                            [ctypes.POINTER(c_float), ctypes.POINTER(c_float), c_void_p]),
    "nunif_hip_dilate_edge": (c_int32, [c_void_p, c_void_p, c_void_p] + [c_int32] * 5 + [c_void_p]),
    "nunif_hip_dilate_edge_work_floats": (ctypes.c_int64, [c_int32, c_int32, c_int32]),
    "nunif_hip_minmax_normalize": (c_int32, [c_void_p, c_void_p, c_void_p, c_int32, c_int64, c_void_p]),
    "nunif_hip_mask_morphology": (c_int32, [c_void_p, c_void_p, c_void_p] + [c_int32] * 6 + [c_void_p]),
    "nunif_hip_reflection_pad2d": (c_int32, [c_void_p, c_void_p, c_int64, c_int32, c_int32, c_int32, c_int32, c_int32, c_int32,
                                             c_void_p]),
    "nunif_hip_depth_postprocess": (c_int32, [c_void_p, c_void_p, c_int64, c_float, c_int32, c_float, c_int32, c_void_p]),
    "nunif_hip_frame_to_tensor": (c_int32, [c_void_p, c_void_p, c_int32, c_int32, c_int32, c_void_p]),
    "nunif_hip_stereo_to_frame": (c_int32, [c_void_p, c_void_p, c_void_p, c_int32, c_int32, c_int32, c_int32, c_void_p]),
    "nunif_hip_stereo_compose": (c_int32, [c_void_p, c_void_p, c_void_p, c_int32, c_int32, c_int32, c_void_p]),
    "nunif_hip_rgb_noise": (c_int32, [c_void_p, c_int32, c_int32, c_int32, c_int32, c_int32, c_uint64, c_uint64, c_void_p]),
    "nunif_hip_apply_rgb_noise": (c_int32, [c_void_p, c_void_p, c_void_p, c_int64, c_double, c_double, c_int32, c_double, c_void_p]),
    "nunif_hip_grain_blend": (c_int32, [c_void_p, c_void_p, c_int64, c_double, c_int32, c_void_p]),
    "nunif_hip_grain_video_step": (c_int32, [c_void_p, c_void_p, c_void_p, c_int32, c_int32, c_int32, c_int32, c_uint64, c_uint64,
                                             c_double, c_int32, c_double, c_double, c_int32, c_double, c_void_p]),
    "nunif_hip_frame_to_tensor_rot": (c_int32, [c_void_p, c_void_p, c_int32, c_int32, c_int32, c_int32, c_void_p]),
    "nunif_hip_map_depth": (c_int32, [c_void_p, c_void_p, c_int64, c_int32, c_double, c_double, c_void_p]),
    "nunif_hip_transnetv2_create": (c_int32, [ctypes.POINTER(TensorDesc), c_int32, c_int32, ctypes.POINTER(c_void_p)]),
    "nunif_hip_transnetv2_destroy": (None, [c_void_p]),
    "nunif_hip_transnetv2_forward": (c_int32, [c_void_p, c_void_p, c_int32, c_int32, c_void_p, c_void_p, c_void_p, c_void_p]),
    "nunif_hip_sod_v1_create": (c_int32, [ctypes.POINTER(TensorDesc), c_int32, c_int32, ctypes.POINTER(c_void_p)]),
    "nunif_hip_sod_v1_destroy": (None, [c_void_p]),
    "nunif_hip_sod_v1_workspace_floats": (c_int64, [c_int32]),
    "nunif_hip_sod_v1_forward": (c_int32, [c_void_p, c_void_p, c_int32, c_int32, c_void_p, c_int32, c_int32, c_int32, c_void_p,
                                           c_void_p, c_void_p, c_void_p]),
    "nunif_hip_sod_v1_entry": (c_int32, [c_void_p, c_int32, c_int32, c_void_p, c_int32, c_int32, c_int32, c_void_p, c_void_p,
                                         c_void_p]),
    "nunif_hip_sod_v1_debug_taps": (c_int32, [c_void_p, c_void_p, c_int32, c_char_p, c_void_p, c_int64, ctypes.POINTER(c_int64),
                                              c_void_p]),
    "nunif_hip_sod_v1_depth_position": (c_int32, [c_void_p, c_void_p, c_int32, c_int64, c_double, c_void_p, c_void_p]),
    "nunif_hip_sod_v1_ema": (c_int32, [c_void_p, c_void_p, c_int32, c_void_p, c_double, c_uint64, c_void_p]),
    "nunif_hip_superpoint_create": (c_int32, [ctypes.POINTER(TensorDesc), c_int32, ctypes.POINTER(c_void_p)]),
    "nunif_hip_superpoint_destroy": (None, [c_void_p]),
    "nunif_hip_superpoint_forward": (c_int32, [c_void_p, c_void_p] + [c_int32] * 6 + [c_float, c_void_p, c_void_p, c_void_p,
                                              c_void_p]),
    "nunif_hip_superpoint_debug_taps": (c_int32, [c_void_p, c_char_p, c_void_p, c_int64, ctypes.POINTER(c_int64), c_void_p]),
    "nunif_hip_superpoint_sample": (c_int32, [c_void_p, c_int32, c_void_p, c_int32, c_void_p, c_void_p]),
    "nunif_hip_superpoint_keypoints_work_floats": (c_int64, [c_int32, c_int32, c_int32]),
    "nunif_hip_superpoint_keypoints": (c_int32, [c_void_p] + [c_int32] * 5 + [c_float] + [c_void_p] * 6),
    "nunif_hip_sample_descriptors": (c_int32, [c_void_p, c_int32, c_void_p] + [c_int32] * 4 + [c_void_p, c_void_p]),
    "nunif_hip_superpoint_match": (c_int32, [c_void_p, c_int32, c_void_p, c_int32, c_int32, c_void_p, c_void_p, c_void_p,
                                            c_void_p]),
    "nunif_hip_affine_warp": (c_int32, [c_void_p, c_void_p, c_void_p] + [c_int32] * 5 + [c_void_p]),
    "nunif_hip_outpaint_create": (c_int32, [ctypes.POINTER(TensorDesc), c_int32, ctypes.POINTER(c_void_p)]),
    "nunif_hip_outpaint_destroy": (None, [c_void_p]),
    "nunif_hip_outpaint_work_bytes": (c_int64, [c_int32] * 4),
    "nunif_hip_outpaint_infer": (c_int32, [c_void_p, c_void_p, c_void_p] + [c_int32] * 5 + [c_void_p, c_void_p, c_void_p]),
    "nunif_hip_outpaint_debug_taps": (c_int32, [c_void_p, c_void_p] + [c_int32] * 4 + [c_char_p, c_void_p, c_int64,
                                                ctypes.POINTER(c_int64), c_void_p]),
    "nunif_hip_outpaint_buffer_step": (c_int32, [c_void_p] * 4 + [c_double] + [c_int32] * 3 + [c_void_p] * 3),
    "nunif_hip_autocrop_stats": (c_int32, [c_void_p] + [c_int32] * 5 + [c_void_p, c_void_p, c_void_p, c_int64, c_void_p]),
    "nunif_hip_autocrop_debug_stats": (c_int32, [c_void_p] + [c_int32] * 5 + [c_void_p, c_void_p, c_void_p, c_int64] +
                                       [c_void_p] * 5),
    "nunif_hip_autocrop_crop_pad": (c_int32, [c_void_p, c_void_p, c_int64] + [c_int32] * 10 + [c_float, c_void_p]),
    "nunif_hip_jpeg_quant_tables": (c_int32, [c_int32, c_void_p, c_void_p]),
    "nunif_hip_jpeg_header": (c_int64, [c_int32] * 5 + [c_void_p, c_int64]),
    "nunif_hip_jpeg_max_bytes": (c_int64, [c_int32] * 4),
    "nunif_hip_jpeg_workspace_bytes": (c_int64, [c_int32] * 5),
    "nunif_hip_jpeg_encode": (c_int32, [c_void_p] + [c_int32] * 6 + [c_void_p, c_int64, c_void_p, c_void_p, c_void_p]),
    "nunif_hip_jpeg_debug_coefficients": (c_int32, [c_void_p] + [c_int32] * 5 + [c_void_p, c_void_p]),
    "nunif_hip_png_header": (c_int64, [c_int32] * 3 + [c_void_p, c_void_p, c_int32, c_void_p, c_int64]),
    "nunif_hip_png_max_bytes": (c_int64, [c_int32] * 4),
    "nunif_hip_png_workspace_bytes": (c_int64, [c_int32] * 5),
    "nunif_hip_png_encode": (c_int32, [c_void_p] + [c_int32] * 5 + [c_void_p, c_int64, c_void_p, c_void_p, c_void_p]),
    "nunif_hip_png_debug_filtered": (c_int32, [c_void_p] + [c_int32] * 4 + [c_void_p, c_void_p]),
    "nunif_hip_png_debug_codes": (c_int32, [c_void_p] + [c_int32] * 5 + [c_void_p] * 4),
    "nunif_hip_png_encode_planes": (c_int32, [c_void_p, c_void_p] + [c_int32] * 6 + [c_void_p, c_int64, c_void_p, c_void_p, c_void_p]),
    "nunif_hip_png_debug_filtered_planes": (c_int32, [c_void_p, c_void_p] + [c_int32] * 5 + [c_void_p, c_void_p]),
    "nunif_hip_hdr2sdr": (c_int32, [c_void_p, c_void_p, c_int32, c_int32, c_int32, c_int32, ctypes.POINTER(Hdr2SdrParams), c_int32,
                                    c_void_p]),
    "nunif_hip_hdr2sdr_constants": (c_int32, [c_int32, c_int32, ctypes.POINTER(Hdr2SdrParams), ctypes.POINTER(c_float),
                                              ctypes.POINTER(c_float)]),
    "nunif_hip_yuv_to_tensor": (c_int32, [ctypes.POINTER(PixfmtPlanes)] + [c_int32] * 6 + [c_void_p, c_void_p, c_void_p]),
    "nunif_hip_tensor_to_yuv": (c_int32, [c_void_p] + [c_int32] * 5 + [ctypes.POINTER(PixfmtPlanes), c_void_p]),
    "nunif_hip_pixfmt_constants": (c_int32, [c_int32] * 4 + [ctypes.POINTER(c_float), ctypes.POINTER(c_float)]),
    "nunif_hip_yuv_hdr_to_tensor": (c_int32, [ctypes.POINTER(PixfmtPlanes)] + [c_int32] * 6 + [ctypes.POINTER(Hdr2SdrParams), c_int32,
                                                                                                c_void_p, c_void_p]),
    "nunif_hip_cliqa_create": (c_int32, [ctypes.POINTER(TensorDesc), c_int32, c_int32, ctypes.POINTER(c_void_p)]),
    "nunif_hip_cliqa_destroy": (None, [c_void_p]),
    "nunif_hip_cliqa_workspace_bytes": (c_int64, [c_void_p] + [c_int32] * 4),
    "nunif_hip_cliqa_forward": (c_int32, [c_void_p, c_void_p] + [c_int32] * 4 + [c_void_p, c_int64] + [c_void_p] * 3),
    "nunif_hip_cliqa_debug_taps": (c_int32, [c_void_p, c_void_p] + [c_int32] * 4 + [c_void_p, c_int64] + [c_void_p] * 7),
    "nunif_hip_cliqa_select_patches": (c_int32, [c_void_p] + [c_int32] * 4 + [c_void_p] * 4),
    "nunif_hip_da3_disparity_workspace_bytes": (c_int64, [c_int32] * 3),
    "nunif_hip_da3_disparity": (c_int32, [c_void_p, c_void_p] + [c_int32] * 3 + [c_double, c_double, c_int32, c_void_p, c_void_p,
                                                                                 c_int64, c_void_p]),
    "nunif_hip_da3_disparity_debug_stats": (c_int32, [c_void_p, c_int32, c_void_p, c_void_p, c_void_p]),
    "nunif_hip_da3mono_features_workspace_bytes": (c_int64, [c_int32] * 3),
    "nunif_hip_da3mono_features": (c_int32, [c_void_p] + [c_int32] * 3 + [c_void_p, c_void_p, c_void_p, c_int64, c_void_p]),
    "nunif_hip_da3mono_create": (c_int32, [ctypes.POINTER(TensorDesc), c_int32, ctypes.POINTER(c_void_p)]),
    "nunif_hip_da3mono_destroy": (None, [c_void_p]),
    "nunif_hip_da3mono_workspace_bytes": (c_int64, [c_int32] * 3),
    "nunif_hip_da3mono_forward": (c_int32, [c_void_p, c_void_p] + [c_int32] * 3 + [c_void_p, c_void_p, c_void_p, c_int64, c_void_p]),
    "nunif_hip_find_transform_workspace_bytes": (c_int64, [c_int32] * 3),
    "nunif_hip_find_transform": (c_int32, [c_void_p] * 4 + [c_int32] * 3 + [c_double] * 5 + [c_int32] + [c_void_p] * 4 + [c_int64,
                                                                                                                         c_void_p, c_void_p]),
    "nunif_hip_stlizer_scene_weight": (c_int32, [c_void_p, c_int32, c_void_p, c_void_p]),
    "nunif_hip_stlizer_pass3_workspace_bytes": (c_int64, [c_int32, c_int32]),
    "nunif_hip_stlizer_pass3_prepare": (c_int32, [c_void_p] * 4 + [c_int32, c_void_p, c_void_p, c_int64, c_void_p]),
    "nunif_hip_stlizer_pass3_conv": (c_int32, [c_void_p, c_int32, c_void_p, c_int32, c_void_p, c_void_p]),
    "nunif_hip_stlizer_pass3_grad_opt": (c_int32, [c_void_p, c_void_p, c_int32, c_double, c_int32, c_double, c_void_p, c_void_p,
                                                  c_int64, c_void_p, c_void_p, c_void_p]),
    "nunif_hip_swin_unet_debug_taps":(c_int32, [c_void_p, c_int32]),
    "nunif_hip_swin_unet_get_tap": (c_int32, [c_void_p, c_int32, c_char_p, c_int32, c_void_p, c_int64,
                                              ctypes.POINTER(c_int64)]),
    "nunif_hip_cunet_debug_taps": (c_int32, [c_void_p, c_int32]),
    "nunif_hip_cunet_get_tap": (c_int32, [c_void_p, c_int32, c_char_p, c_int32, c_void_p, c_int64,
                                          ctypes.POINTER(c_int64)]),
    "nunif_hip_minmax": (c_int32, [c_void_p, c_void_p, c_int32, c_int64, c_void_p]),
    "nunif_hip_ema_scaler_push": (c_int32, [c_void_p, c_void_p, c_int32, c_int64, c_int32, c_int32, c_double, c_void_p]),
    "nunif_hip_ema_scaler_ring_minmax": (c_int32, [c_void_p, c_int32, c_void_p]),
    "nunif_hip_range_normalize": (c_int32, [c_void_p, c_void_p, c_void_p, c_int64, c_int32, c_void_p]),
    "nunif_hip_make_input_planes": (c_int32, [c_void_p, c_void_p, c_int32, c_int32, c_int32, c_double, c_double, c_int32, c_void_p, c_void_p]),
    "nunif_hip_stack": (c_int32, [ctypes.POINTER(c_void_p), c_int32, c_int64, c_void_p, c_void_p]),
    "nunif_hip_profile_enable": (c_int32, [c_int32]),
    "nunif_hip_profile_read": (c_int32, [ctypes.POINTER(ProfRecord), c_int32, c_int32]),
}

_lib = None


def lib():
    """Load (once) and return the ctypes library.  Raises if it has not been built."""
    global _lib
    if _lib is None:
        # torch bundles its own libamdhip64 (SONAME libamdhip64.so.7).  It must be in the process BEFORE this
        # library is dlopen'ed so that both bind to ONE HIP runtime (streams and pointers are shared); loading
        # /opt/rocm's copy first gives two runtimes and hipMalloc fails.
        import torch  # noqa: F401
        if not os.path.exists(LIB_PATH):
            raise RuntimeError(
                f"{LIB_PATH} not found: the HIP engine is not built. Run `python -m nunif_amd.build` "
                "(there is no CPU fallback).")
        handle = ctypes.CDLL(LIB_PATH)
        for name, (restype, argtypes) in SIGNATURES.items():
            fn = getattr(handle, name)  # AttributeError here == ABI mismatch
            fn.restype = restype
            fn.argtypes = argtypes
        _lib = handle
    return _lib


def check(status):
    if status != 0:
        raise NunifHipError(status, lib().nunif_hip_last_error().decode("utf-8", "replace"))


def current_stream_ptr(device=None):
    import torch
    return c_void_p(torch.cuda.current_stream(device).cuda_stream)


def tile_grid(x_h, x_w, scale, offset, tile_size, blend_size):
    g = TileGrid()
    check(lib().nunif_hip_tile_grid_init(x_h, x_w, scale, offset, tile_size, blend_size or 0, ctypes.byref(g)))
    return g


def swin_tile_extents(grid, tile_index, blocks_per_stage=(2, 2, 6, 2, 2), shifts=None, to_image_fused=True):
    """Windows of tile ``tile_index`` that a swin_unet frame render runs: one ``(n_win_y, n_win_x, wrap_y, wrap_x)`` per block in
    forward order (``nunif_hip_swin_unet_tile_extents``; host-only integer math)."""
    n = sum(blocks_per_stage)
    if shifts is None:
        shifts = [3 if i % 2 else 0 for k in blocks_per_stage for i in range(k)]
    per = (c_int32 * 5)(*blocks_per_stage)
    sh = (c_int32 * n)(*shifts)
    out = (SwinBlockExtent * n)()
    check(lib().nunif_hip_swin_unet_tile_extents(ctypes.byref(grid), tile_index, per, sh, 1 if to_image_fused else 0, out))
    return [(e.n_win[0], e.n_win[1], e.wrap[0], e.wrap[1]) for e in out]


def swin_tail_groups(extents, S, shift):
    """Token groups of one C = 192 block over a tile minibatch (``nunif_hip_swin_unet_tail_groups``; host-only integer math).
    ``extents``: that block's ``(n_win_y, n_win_x, wrap_y, wrap_x)`` of each tile; returns ``(ctypes array of SwinTailGroup, n_tokens)``."""
    ext = (SwinBlockExtent * len(extents))()
    for e, (ny, nx, wy, wx) in zip(ext, extents):
        e.n_win[0], e.n_win[1], e.wrap[0], e.wrap[1] = ny, nx, wy, wx
    ng, nt = c_int64(0), c_int64(0)
    check(lib().nunif_hip_swin_unet_tail_groups(ext, len(extents), S, shift, None, 0, ctypes.byref(ng), ctypes.byref(nt)))
    out = (SwinTailGroup * max(1, ng.value))()
    if ng.value:
        check(lib().nunif_hip_swin_unet_tail_groups(ext, len(extents), S, shift, out, ng.value, ctypes.byref(ng), ctypes.byref(nt)))
    return (SwinTailGroup * ng.value).from_buffer(out) if ng.value else (SwinTailGroup * 0)(), nt.value


SWIN_PRODUCERS = {"stem": 0, "down1": 1, "down2": 2, "up2": 3, "up1": 4}


def swin_producer_tokens(extents, S, producer, blocks_per_stage=(2, 2, 6, 2, 2), shifts=None, listed=None, f1_whole=False,
                         patch=(24, 16)):
    """What one producer of a frame render writes over a tile minibatch (``nunif_hip_swin_unet_producer_tokens``; host-only integer
    math).  ``extents``: per tile the list ``swin_tile_extents`` returns; ``producer``: a key of ``SWIN_PRODUCERS``.  Returns
    ``(entries, n)``: the table as the kernels walk it (token producers: filled up to whole groups of 32) and the count before the fill."""
    n_blocks = sum(blocks_per_stage)
    if shifts is None:
        shifts = [3 if i % 2 else 0 for k in blocks_per_stage for i in range(k)]
    ext = (SwinBlockExtent * (len(extents) * n_blocks))()
    for t, tile in enumerate(extents):
        assert len(tile) == n_blocks
        for i, (ny, nx, wy, wx) in enumerate(tile):
            e = ext[t * n_blocks + i]
            e.n_win[0], e.n_win[1], e.wrap[0], e.wrap[1] = ny, nx, wy, wx
    per = (c_int32 * 5)(*blocks_per_stage)
    sh = (c_int32 * n_blocks)(*shifts)
    li = (c_int32 * n_blocks)(*[1 if v else 0 for v in listed]) if listed is not None else None
    args = (ext, len(extents), per, sh, li, S, 1 if f1_whole else 0, SWIN_PRODUCERS[producer], patch[0], patch[1])
    n = c_int64(0)
    check(lib().nunif_hip_swin_unet_producer_tokens(*args, None, 0, ctypes.byref(n)))
    cap = (n.value + 31) // 32 * 32
    out = (ctypes.c_uint32 * max(1, cap))()
    check(lib().nunif_hip_swin_unet_producer_tokens(*args, out, cap, ctypes.byref(n)))
    return list(out)[:n.value if producer == "stem" else cap], n.value


def blend_ramp(blend_size):
    buf = (c_float * max(1, blend_size))()
    check(lib().nunif_hip_blend_ramp(blend_size, buf))
    return list(buf)[:blend_size]


def profile_enable(on=True):
    check(lib().nunif_hip_profile_enable(1 if on else 0))


def profile_read(reset=True):
    recs = (ProfRecord * 64)()
    n = lib().nunif_hip_profile_read(recs, 64, 1 if reset else 0)
    return [{"name": recs[i].name.decode(), "total_ms": recs[i].total_ms, "launches": recs[i].launches,
             "flops": recs[i].flops, "bytes": recs[i].bytes} for i in range(n)]
