/*
 * nunif_hip.h — C ABI of libnunif_hip.so, the MI355X (gfx950) engine under nunif's tiled-inference hot path.
 *
 * The reference (nagadomi/nunif) is pure Python on PyTorch and has no FFI of its own: the
 * drop-in boundary is a set of Python call signatures.  Each entry point below names the reference function
 * (file:line under the reference tree) whose work it replaces; nunif_amd/ mirrors the Python signatures on top
 * of these calls and INTEGRATION.md shows the binding a reference maintainer would add.
 *
 * Conventions
 *  - plain C: pointers + sizes, no torch / C++ types.  `stream` is a hipStream_t passed as void* (NULL = the
 *    null stream).  All device pointers are caller-owned (e.g. torch tensor.data_ptr()); the library owns only
 *    the weights/workspace that live inside a model handle.
 *  - every function returns 0 on success or a negative nunif_hip_status; nunif_hip_last_error() returns a
 *    thread-local message for the last failure.  No function synchronises the device unless it says so.
 *  - image tensors are planar CHW / NCHW float32 in [0,1] at the boundary, exactly like the reference.
 */
#ifndef NUNIF_HIP_H
#define NUNIF_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define NUNIF_HIP_ABI_VERSION 1

typedef enum {
    NUNIF_HIP_OK = 0,
    NUNIF_HIP_EINVAL = -1,   /* bad argument (the Python layer raises ValueError / AssertionError) */
    NUNIF_HIP_ENOMEM = -2,   /* hipMalloc failed */
    NUNIF_HIP_EHIP = -3,     /* a HIP runtime call or kernel launch failed */
    NUNIF_HIP_EMISSING = -4, /* a required weight tensor is missing from the state dict */
    NUNIF_HIP_EUNSUPPORTED = -5
} nunif_hip_status;

int nunif_hip_abi_version(void);
const char *nunif_hip_last_error(void);

/* ------------------------------------------------------------------------------------------------------------
 * Tile grid + stitcher.  Replaces nunif/utils/seam_blending.py: create_config :109-143, create_blend_filter
 * :146-153, the F.pad + tile slicing of tiled_render :82,:90, update :156-174 and get_output :39-40.
 * ---------------------------------------------------------------------------------------------------------- */
typedef struct {
    int32_t x_h, x_w, scale, offset, tile_size, blend_size;                 /* inputs */
    int32_t y_h, y_w, h_blocks, w_blocks;                                   /* create_config outputs */
    int32_t pad_l, pad_r, pad_t, pad_b, y_buffer_h, y_buffer_w;
    int32_t input_tile_step, output_tile_step;
    int32_t out_tile_size;                                                  /* tile_size*scale - 2*offset */
} nunif_tile_grid;

/* Host-only integer math; bit-exact with create_config. */
int nunif_hip_tile_grid_init(int32_t x_h, int32_t x_w, int32_t scale, int32_t offset, int32_t tile_size,
                             int32_t blend_size, nunif_tile_grid *grid);

/* Host-only: the 1-D edge ramp r[0..blend_size) (fp32) with filter F[y,x] = min(r'[y], r'[x]);
 * values are the reference's Python-double `1 - (1/(b+1))*(i+1)` rounded to fp32. */
int nunif_hip_blend_ramp(int32_t blend_size, float *ramp /* [blend_size] host */);

/* tiles[k] = replicate-padded x[:, i:i+T, j:j+T] for tile indices tile_begin .. tile_begin+n_tiles (row-major
 * over the grid).  x: [C,x_h,x_w] f32 device; tiles: [n_tiles,C,T,T] f32 device. */
int nunif_hip_gather_tiles(const float *x, float *tiles, const nunif_tile_grid *grid, int32_t channels,
                           int32_t tile_begin, int32_t n_tiles, void *stream);

/* Single-pass stitch of ALL tile outputs of a frame: for each output pixel replay the reference's running-mean
 * update over the (<=4) covering tiles in row-major tile order, crop to [y_h,y_w] and clamp to [0,1].
 * tile_out: [h_blocks*w_blocks, C, To, To] f32 device; y: [C, y_h, y_w] f32 device. */
int nunif_hip_stitch_tiles(const float *tile_out, float *y, const nunif_tile_grid *grid, int32_t channels,
                           void *stream);

/* ------------------------------------------------------------------------------------------------------------
 * waifu2x swin_unet.  Replaces waifu2x/models/swin_unet.py SwinUNetBase.forward :180-199 (+ the eval clamp of
 * the SwinUNet/SwinUNet2x/SwinUNet4x wrappers :221-226,:244-249,:281-290) and torchvision's
 * SwinTransformerBlock (imported at :9-12).
 * ---------------------------------------------------------------------------------------------------------- */
typedef struct {
    const char *name;      /* reference state_dict key, e.g. "unet.swin1.block.0.attn.qkv.weight" */
    const float *data;     /* HOST pointer, contiguous fp32 */
    int32_t ndim;
    int64_t shape[4];
} nunif_tensor_desc;

typedef struct nunif_swin_unet nunif_swin_unet;

/* Build a model from a reference-format state dict (host fp32).  Weights are repacked to MFMA-fragment-major
 * fp16 in device memory owned by the handle.  scale_factor in {1,2,4}.  The current HIP device is bound. */
int nunif_hip_swin_unet_create(const nunif_tensor_desc *tensors, int32_t n_tensors, int32_t scale_factor,
                               nunif_swin_unet **handle);
void nunif_hip_swin_unet_destroy(nunif_swin_unet *handle);

/* z = clamp(unet(x), 0, 1).  x: [B,3,T,T] f32 device, z: [B,3,(T-16)*s,(T-16)*s] f32 device; T must satisfy the
 * reference's tile_size_validator (swin_unet.py:202-205).  Workspace grows inside the handle as needed. */
int nunif_hip_swin_unet_forward(nunif_swin_unet *handle, const float *x, float *z, int32_t batch,
                                int32_t tile_size, void *stream);

/* Whole-frame render = SeamBlending.tiled_render (seam_blending.py:48-106) with this model:
 * x: [3,H,W] f32 device -> y: [3,H*s,W*s] f32 device.  The tile gather is fused into the first conv, tiles run
 * in minibatches of `batch_size`, the stitch is the single-pass kernel above. */
int nunif_hip_swin_unet_render(nunif_swin_unet *handle, const float *x, float *y, int32_t x_h, int32_t x_w,
                               int32_t tile_size, int32_t batch_size, void *stream);

/* Tile-ROW sharding of one huge image (the multi-GPU fallback of SURVEY.md §8e; the reference has no counterpart — its
 * SeamBlending.tiled_render, seam_blending.py:48-106, runs every tile on one model): the same render cut into
 *   render_tile_rows  the tiles of tile rows [row_begin, row_end) of the grid into the handle's tile store,
 *   tile_row_band     export (import_band = 0) / import (1) of output rows [row0, row0 + n_rows) of every tile of one tile row,
 *                     band = [w_blocks][3][n_rows][out_tile_size] f32 device — what neighbouring ranks exchange,
 *   stitch_rows       the single-pass stitch of output rows [y_row_begin, y_row_end) into a compact [3][rows][y_w] band.
 * Same tile grid, same tile store layout and the same stitch kernel as nunif_hip_swin_unet_render: bit-identical results.
 * The tile store is defined only where a stitch of the frame reads it: of a tile of the last tile row / column, the pixels past the
 * frame's edge are not written by a frame render (NUNIF_SWIN_SKIP_PAD: 0 whole tiles, 1 level-1 C = 96 blocks only, 2 every fast block, default 3 PatchDown2 / PatchUp as well), and a band exported by tile_row_band
 * carries whatever the store held there.  No stitch reads those pixels on either side of an exchange. */
int nunif_hip_swin_unet_render_tile_rows(nunif_swin_unet *handle, const float *x, int32_t x_h, int32_t x_w,
                                         int32_t tile_size, int32_t batch_size, int32_t row_begin, int32_t row_end,
                                         void *stream);
int nunif_hip_swin_unet_tile_row_band(nunif_swin_unet *handle, int32_t x_h, int32_t x_w, int32_t tile_size,
                                      int32_t tile_row, int32_t row0, int32_t n_rows, float *band, int32_t import_band,
                                      void *stream);
int nunif_hip_swin_unet_stitch_rows(nunif_swin_unet *handle, float *y_band, int32_t x_h, int32_t x_w, int32_t tile_size,
                                    int32_t y_row_begin, int32_t y_row_end, void *stream);

/* Which 6 x 6 windows of a tile a frame render has to run (host-only integer math; the frame entry points above use it to leave
 * out windows that only feed replicate padding the stitch crops away).  Axis 0 = rows, 1 = columns.  Per block and axis the active
 * windows are [0, n_win) plus, if `wrap`, the last window (a shifted block's wrap window, which holds tokens [0, 3)); a tile runs
 * the product of its two axes.  grid: a swin_unet grid (offset 8 * scale); blocks_per_stage[5]: blocks of swin1 .. swin5;
 * shifts / out: one entry per block in forward order (shift 0 or 3, swin_unet.py:30); to_image_fused: whether ToImage runs inside
 * the last block's tail (1x / 2x nets) — either way one token becomes scale x scale pixels, so it does not change the extents. */
typedef struct {
    int32_t n_win[2];
    int32_t wrap[2];
} nunif_swin_block_extent;
int nunif_hip_swin_unet_tile_extents(const nunif_tile_grid *grid, int32_t tile_index, const int32_t *blocks_per_stage,
                                     const int32_t *shifts, int32_t to_image_fused, nunif_swin_block_extent *out);

/* The tokens of one block's active windows as groups of at most 16 token slots, the unit of work of the C = 192 tail kernel (host-only
 * integer math, like the extents above).  ext[n_tiles]: that block's extent of each tile of a minibatch; S: side of the block's token
 * map (a multiple of 6); shift: 0 or 3.  Token = (tile * S + y) * S + x; a tile's active tokens are those of its active windows,
 * wrap window included.  They are packed in ascending order, so only the LAST group of a table is partly filled unless a group
 * would need more than 6 contiguous pieces (runs are at least 3 tokens long, so it never does).
 * A group names slot r in [0, cnt) as adj[p] + r, where p is the last piece whose first slot is <= r: bits [5 (p - 1), 5 p) of
 * `bounds` hold the first slot of piece p = 1 .. 5 (16: no such piece), bits [25, 30) hold cnt (1 .. 16).
 * out == NULL only counts; otherwise at most `cap` groups are written (more needed: an error).  n_groups / n_tokens: totals. */
typedef struct {
    int32_t adj[6];
    uint32_t bounds;
    uint32_t reserved;
} nunif_swin_tail_group;
int nunif_hip_swin_unet_tail_groups(const nunif_swin_block_extent *ext, int32_t n_tiles, int32_t S, int32_t shift,
                                    nunif_swin_tail_group *out, int64_t cap, int64_t *n_groups, int64_t *n_tokens);

/* What the producers of a frame render have to write (NUNIF_SWIN_SKIP_PAD level 3, where down2, up2 and up1 use it; host-only integer math, like the extents above): a
 * producer — the stem, PatchDown down1 / down2, PatchUp up2 / up1 — leaves a token out only if no launch of this frame reads it.
 * ext[n_tiles][n_blocks]: every block's extent of each tile of a minibatch (nunif_hip_swin_unet_tile_extents); listed[n_blocks]: 1 =
 * the block runs its active windows only, 0 = it runs whole tiles and so reads every token (NULL: all 1); S: side of the level-1
 * token map; f1_whole: 1 = something reads the whole level-1 map (proj2 of the 4x net), so the stem writes all of it.
 * Per tile and axis a stage's read set is the union of its blocks' active windows, BOTH halves of a wrap window, and a tile's set is
 * the product of its two axes; the sets follow the 2 x 2 relations back from swin5 to the stem (swin_producer_tokens_host.h has the
 * recurrence).  Written is a superset of read: no launch reads what this frame did not write.
 * Token producers (DOWN1 / DOWN2: the OUTPUT map, side S / 2 and S / 4; UP2 / UP1: the INPUT map, side S / 4 and S / 2, every listed
 * token writes its four children): out = token (tile * Ss + y) * Ss + x in ascending order, each once, then filled up to a multiple
 * of 32 entries with the last token.  STEM: out = the patches of patch_h x patch_w output tokens that hold a wanted token,
 * (tile * nty + ty) * ntx + tx with nty / ntx = patches per tile side, rounded up.  out == NULL only counts; cap: entries `out`
 * holds (fill included; fewer than needed is an error).  n_out: tokens / patches before the fill. */
enum { NUNIF_SWIN_PRODUCER_STEM = 0, NUNIF_SWIN_PRODUCER_DOWN1 = 1, NUNIF_SWIN_PRODUCER_DOWN2 = 2, NUNIF_SWIN_PRODUCER_UP2 = 3,
       NUNIF_SWIN_PRODUCER_UP1 = 4 };
int nunif_hip_swin_unet_producer_tokens(const nunif_swin_block_extent *ext, int32_t n_tiles, const int32_t *blocks_per_stage,
                                        const int32_t *shifts, const int32_t *listed, int32_t S, int32_t f1_whole, int32_t producer,
                                        int32_t patch_h, int32_t patch_w, uint32_t *out, int64_t cap, int64_t *n_out);

/* Tests only: ONE PatchDown2 launch pair on caller buffers (device memory): a [B, 2 Ho, 2 Wo, 192] fp16 -> out [B, Ho, Wo, 192] fp16,
 * the first tap row written, the second accumulated onto it.  acc_form: 1 = the second pass on the prefetching PatchDown kernel,
 * 0 = on the generic resident-weight GEMM; the two give the same bits. */
int nunif_hip_swin_unet_down2_test(nunif_swin_unet *handle, const void *a, void *out, int32_t B, int32_t Ho, int32_t Wo,
                                   int32_t acc_form, void *stream);

/* Tests only: ONE launch of the C = 192 tail of block `block` of stage `stage` (1 .. 3, or 4 on the 4x net) on caller buffers (device
 * memory): att and x are [n_tokens][192] fp16, x is updated in place.  groups == NULL: every token; else a device copy of a table
 * of nunif_hip_swin_unet_tail_groups (n_groups entries naming n_listed tokens), and only those tokens are read and written. */
int nunif_hip_swin_unet_tail192_test(nunif_swin_unet *handle, int32_t stage, int32_t block, const void *att, void *x,
                                     int64_t n_tokens, const nunif_swin_tail_group *groups, int64_t n_groups, int64_t n_listed,
                                     int32_t rev, void *stream);

/* ------------------------------------------------------------------------------------------------------------
 * waifu2x CUNet.  Replaces waifu2x/models/cunet.py CUNet.forward :183-196 (UNet1 :52-67, UNet2 :99-121, SEBlock
 * nunif/modules/attention.py:29-44).  Geometry: scale 1, offset 28, no blending (cunet.py:177).
 * ---------------------------------------------------------------------------------------------------------- */
/* waifu2x "waifu2x.swin_unet_v2_1x / _2x / _4x" (aliases winc_unet_*; waifu2x/models/swin_unet_v2.py SwinUNetV2Base :272-352,
 * the model classes :361-466): IR stem, window-MHA + conv-MLP blocks (zero-padded half-window shift, learned score bias),
 * shortcut PatchDown / PatchUp, ToImage + SourceResidual.  State dict in the reference's key layout ("unet." prefix); base_dim
 * (64 / 96 / 128), lv2_ratio and the block counts are read from the tensor shapes.
 * forward: x [B,3,T,T] f32 device -> z [B,3,T*s - 18*s, ...] f32 device (offset 9 s), clamp01 != 0 = eval-mode clamp; T must
 * satisfy the reference's tile_size_validator :355-358 ((T - 16) % 48 == 0). */
typedef struct nunif_swin_unet_v2 nunif_swin_unet_v2;
int nunif_hip_swin_unet_v2_create(const nunif_tensor_desc *tensors, int32_t n_tensors, int32_t scale_factor,
                                  nunif_swin_unet_v2 **handle);
void nunif_hip_swin_unet_v2_destroy(nunif_swin_unet_v2 *handle);
int nunif_hip_swin_unet_v2_forward(nunif_swin_unet_v2 *handle, const float *x, float *z, int32_t batch, int32_t tile_size,
                                   int32_t clamp01, void *stream);
/* tests: forward that also stores its intermediate maps as fp32, concatenated in the order they are produced (each copied by a
 * launch right after the one that produced it; z is what forward writes).  With S = T - 16, C = base_dim, C2 = the level-2 width,
 * and per WAC block two maps of the block's own resolution and width, "att" (the window attention's output, before head_proj) and
 * then the block's output:
 *   ir.path2.2 att, out   [B,T/2,T/2,64]   x 2
 *   ir.path2.3 att, out   [B,T/2,T/2,64]   x 2
 *   ir                    [B,T,T,32]       (path1 | pixel_shuffle(path2))
 *   patch                 [B,S,S,C]        (conv, crop 7, LeakyReLU)
 *   wac1.blocks.i att, out [B,S,S,C]       x 2 per block
 *   down1                 [B,S/2,S/2,C2]   (shortcut + conv)
 *   wac2.blocks.i att, out [B,S/2,S/2,C2]  x 2 per block
 *   up1                   [B,S,S,C]        (shortcut + proj + skip)
 *   wac3.blocks.i att, out [B,S,S,C]       x 2 per block
 *   residual              [B,3,O,O]        (planar like z, O = (S - 2) s: the fp32 residual image before the source residual)
 * All but the last are channels-last. */
int nunif_hip_swin_unet_v2_debug_taps(nunif_swin_unet_v2 *handle, const float *x, float *z, float *taps, int32_t batch,
                                      int32_t tile_size, int32_t clamp01, void *stream);
/* tests: the window attention of a WAC block alone (the kernel and the launch of the forward) on caller-supplied device maps.
 * qkv [B,H,W,3C] fp16 in the kernel's own convention (q already multiplied by 32^-0.5 log2 e), btab [ws^2][ws^2] f32 (the score
 * bias [query][key], multiplied by log2 e), bqkv [3C] f32 (q / k / v of a token in the zero padding of a shifted window, q scaled
 * like the map's) -> att [B,H,W,C] fp16.  ws = 8 or 6, heads of 32 channels, H and W multiples of ws; shift != 0: windows
 * offset by -ws/2 with zero-padded tokens. */
int nunif_hip_swin_unet_v2_debug_wattn(const void *qkv, const float *btab, const float *bqkv, void *att, int32_t batch,
                                       int32_t height, int32_t width, int32_t channels, int32_t window, int32_t shift, void *stream);

/* waifu2x "waifu2x.wgmlp_4x" (waifu2x/models/wgmlp.py WGMLPBase :298-353, WGMLP4x :441-470): IR / Overscan stem :126-173, window-gMLP
 * + GLU conv-MLP blocks :75-123 (nunif/modules/attention.py GMLP :621-651, WindowGMLP2d :654-693: 8 x 8 windows, zero-padded
 * half-window shift in the order of get_shift_config :289-295), shortcut PatchDown / PatchUp :176-226, ToImage + SourceResidual
 * :229-286.  State dict in the reference's key layout ("unet." prefix); only the registered geometry (base_dim 128, mlp ratios 2,
 * 3 -> 3 channels) is carried.
 * create / destroy replace WGMLP4x.__init__ :445-455; forward replaces WGMLP4x.forward :457-467 in eval mode: x [B,3,T,T] f32 device
 * -> z [B,3,4T-72,4T-72] f32 device (offset 36), clamp01 != 0 = the eval clamp :467; T must satisfy tile_size_validator :406-409
 * ((T - 16) % 48 == 0). */
typedef struct nunif_wgmlp nunif_wgmlp;
int nunif_hip_wgmlp_create(const nunif_tensor_desc *tensors, int32_t n_tensors, nunif_wgmlp **handle);
void nunif_hip_wgmlp_destroy(nunif_wgmlp *handle);
int nunif_hip_wgmlp_forward(nunif_wgmlp *handle, const float *x, float *z, int32_t batch, int32_t tile_size, int32_t clamp01,
                            void *stream);
/* tests: forward that also stores the output of every WGMLPBlock (wgmlp.py:92-101) as fp32 NHWC, concatenated in the order
 * wgmlp1.blocks.*, wgmlp2.blocks.*, wgmlp3.blocks.*: [B,S,S,128] at level 1 and [B,S/2,S/2,256] at level 2, S = T - 16. */
int nunif_hip_wgmlp_debug_taps(nunif_wgmlp *handle, const float *x, float *z, float *taps, int32_t batch, int32_t tile_size,
                               int32_t clamp01, void *stream);
/* tests: the WindowGMLP2d (attention.py:678-693 with GMLP.forward :634-651) of block `block` (0 .. 8 in the order above) alone on a
 * caller-supplied map x [B,H,W,C] f32 (C = 128 at level 1, 256 at level 2; H, W multiples of 8; rounded to fp16 on entry), plain or
 * shifted whatever the block's own place -> out [B,H,W,C] f32.  Optional (NULL: not stored) fp32 maps indexed like x: after
 * LayerNorm 1 [C], GELU [2C], LayerNorm 2 [C], the token mixing [C] and the gate [C]. */
int nunif_hip_wgmlp_debug_gmlp(nunif_wgmlp *handle, int32_t block, const float *x, float *out, int32_t batch, int32_t height,
                               int32_t width, int32_t shift, float *tap_ln1, float *tap_gelu, float *tap_ln2, float *tap_mix,
                               float *tap_gate, void *stream);

typedef struct nunif_cunet nunif_cunet;
int nunif_hip_cunet_create(const nunif_tensor_desc *tensors, int32_t n_tensors, int32_t no_clip, nunif_cunet **handle);
void nunif_hip_cunet_destroy(nunif_cunet *handle);
/* z = clamp(crop(z1,20) + unet2(z1), 0, 1), z1 = clamp(unet1(x)).  x: [B,3,T,T] f32, z: [B,3,T-56,T-56] f32; T % 4 == 0. */
int nunif_hip_cunet_forward(nunif_cunet *handle, const float *x, float *z, int32_t batch, int32_t tile_size,
                            void *stream);
/* Whole-frame tiled render (x: [3,H,W] -> y: [3,H,W]); tile gather fused into the first conv, overwrite stitch. */
int nunif_hip_cunet_render(nunif_cunet *handle, const float *x, float *y, int32_t x_h, int32_t x_w,
                           int32_t tile_size, int32_t batch_size, void *stream);

/* waifu2x image-side helpers.
 * tta_view: one of the 8 dihedral views of nunif/transforms/tta.py tta_split :20-34; view = rot90*4 + vflip*2 + hflip in
 * the reference's tuple order; x: [C,H,W] -> y: [C,H,W] (views 0-3) or [C,W,H] (views 4-7).
 * tta_merge :37-48: views[k]: the model's output for view k ([C,H,W] / [C,W,H]); out = clamp(sum of the inverse-transformed
 * views * 1/8) added in the reference's order (bit-exact).
 * alpha_border_padding: nunif/utils/alpha.py AlphaBorderPadding :32-57; rgb [3,H,W], alpha [1,H,W], work: 8*H*W floats. */
int nunif_hip_tta_view(const float *x, float *y, int32_t C, int32_t H, int32_t W, int32_t view, void *stream);
int nunif_hip_tta_merge(const float *const *views, float *out, int32_t C, int32_t H, int32_t W, void *stream);
int nunif_hip_alpha_border_padding(const float *rgb, const float *alpha, float *out, float *work, int32_t H, int32_t W,
                                   int32_t offset, void *stream);

/* ------------------------------------------------------------------------------------------------------------
 * iw3 stereo synthesis + depth post-processing.
 * ---------------------------------------------------------------------------------------------------------- */
typedef struct {
    int32_t B, H, W;          /* c: [B,3,H,W], depth: [B,1,H,W] (already at image resolution) */
    double divergence;        /* percent of the base size, as in the reference (doubles: host math is done in double) */
    double convergence;
    int32_t fill;             /* 1 = method "forward_fill" (shift_fill inpaint), 0 = "forward" (clamp) */
    int32_t synthetic_view;   /* 0 both, 1 left, 2 right */
    int32_t width_base;       /* base_size = W if 1 else max(H,W) */
    const float *convergence_dev;   /* optional [B] f32 device: a convergence per frame (iw3/utils.py:303-307, the output of the
                                       convergence estimator) read by the kernel; NULL = the scalar `convergence` above */
} nunif_forward_warp_params;

/* Replaces iw3/forward_warp.py apply_divergence_forward_warp :246-256 -> depth_order_bilinear_forward_warp
 * :140-243 (inconsistent_shift=False).  left/right: [B,3,H,W]; lmask/rmask: optional [B,1,H,W] (gen_mask2).
 * For a single-eye view the other output pointer is ignored (the caller returns the source image). */
int nunif_hip_forward_warp(const float *c, const float *depth, float *left, float *right, float *lmask,
                           float *rmask, const nunif_forward_warp_params *params, void *stream);

/* Depth-Anything-V2 ViT-S (DINOv2 ViT-S/14 + DPT head): the depth backbone that iw3/depth_anything_model.py:200-230 loads
 * through torch.hub and calls in _forward :113-119.  The network is NOT part of the reference tree; this engine follows
 * the published architecture (state-dict keys of the public checkpoint: pretrained.*, depth_head.*), see
 * oracle/depth_anything_v2.py — parity is against that restatement only.
 * x: [B,3,h,w] f32 device, ImageNet-normalised (batch_preprocess), h and w multiples of 14;
 * pos: [1 + (h/14)*(w/14)][384] f32 device = the position embedding already interpolated to this grid (host side,
 * once per resolution); depth: [B,h,w] f32 device (relu'd inverse depth, larger = nearer). */
typedef struct nunif_depth_anything nunif_depth_anything;
int nunif_hip_depth_anything_create(const nunif_tensor_desc *tensors, int32_t n_tensors, nunif_depth_anything **handle);
/* The same with the two things a checkpoint does not say: taps = the four encoder blocks that feed the DPT head (NULL: the V2
 * layout of the checkpoint's depth — 2, 5, 8, 11 of 12 blocks, 4, 11, 17, 23 of 24; Depth-Anything V1 takes the last four),
 * and max_depth > 0 for the V2 metric heads (Sigmoid x max_depth: 20 hypersim, 80 vkitti) instead of ReLU.  The geometry —
 * ViT-S / B / L (embed 384 / 768 / 1024, 12 / 24 blocks), DPT out_channels and fusion width — is read from the tensors. */
int nunif_hip_depth_anything_create_ex(const nunif_tensor_desc *tensors, int32_t n_tensors, const int32_t *taps, float max_depth,
                                       nunif_depth_anything **handle);
void nunif_hip_depth_anything_destroy(nunif_depth_anything *handle);
int nunif_hip_depth_anything_forward(nunif_depth_anything *handle, const float *x, const float *pos, float *depth,
                                     int32_t B, int32_t h, int32_t w, void *stream);
/* Video-Depth-Anything, streaming (iw3/video_depth_anything_streaming_model.py:58-103: torch.hub
 * "nagadomi/Video-Depth-Anything_iw3" `VideoDepthAnythingStreaming`; `model.infer_video_depth_one(frame)` :94 and
 * `model.reset_state()` :75).  When the tensors given to _create_ex carry `depth_head.motion_modules.{0..3}.*` (the published
 * checkpoint's `head.motion_modules.*`; the caller renames `head.` to `depth_head.`) the engine is TEMPORAL: _forward with B = 1 is
 * `infer_video_depth_one` — each of the 8 temporal attention blocks attends to the previous <= 31 frames through K / V caches the
 * engine owns — and with B > 1 it is B such calls on CONSECUTIVE frames of the stream in one pass (the reference's per-frame loop
 * :92-95 collapsed: encoder, convs and Linears run over the B frames at once, only the temporal attention steps frame by frame);
 * _reset_state starts a new window.  A change of resolution also does.
 * The network is not in the reference tree; oracle/video_depth_anything_net.py restates the published architecture, PARITY UNPINNED. */
int nunif_hip_depth_anything_reset_state(nunif_depth_anything *handle);
int nunif_hip_depth_anything_is_temporal(const nunif_depth_anything *handle);
/* TESTS ONLY: temporal module `module` (0: layer_3, 1: layer_4, 2: path_4, 3: path_3) alone on B consecutive frames of its input
 * map, with the launches of _forward.  x: [B][P][C] f32 device (rounded to fp16 on entry, C = the module's width), out: [B][P][C]
 * f32 device.  taps: NULL, or 12 f32 device pointers (NULL = skip) in the order gn, proj_in, ln0, att0, res0, ln1, att1, res1, ff_ln,
 * geglu, ff, out — the maps behind GroupNorm, proj_in, per attention block its LayerNorm, the attention kernel's output and the
 * hidden state after to_out, then ff_norm, GEGLU, the hidden state after ff.net.2 and the module's output; [B][P][C] each, geglu
 * [B][P][4 C].  The call advances the handle's window by B frames and touches only this module's K0 / V0 rings; any P > 0 is
 * accepted, and another P or another module starts a new window.  A handle driven through this entry is for tests: call
 * _reset_state before it is used for _forward again. */
int nunif_hip_depth_anything_debug_temporal(nunif_depth_anything *handle, int32_t module, const float *x, float *out, int32_t B,
                                            int32_t P, float *const *taps, int32_t n_taps, void *stream);

/* The six activations the published DepthAnythingCore hooks for ZoeDepth (iw3/zoedepth_model.py:161-164 loads
 * "DepthAnythingMetricDepth" through torch.hub; the net is not in the reference tree): the 32-channel map behind the first conv +
 * ReLU of depth_head.scratch.output_conv2 [B,h,w,32], layer4_rn [B,bh,bw,C] and the refinenet outputs r4, r3, r2, r1
 * [B,rh[i],rw[i],C] — NHWC fp16 device pointers into the engine's workspace, valid until the next call on that handle. */
typedef struct nunif_da_features {
    const void *outconv;
    const void *bottleneck;
    const void *blocks[4];
    int32_t bh, bw, rh[4], rw[4], channels;
} nunif_da_features;
/* nunif_hip_depth_anything_forward that also leaves those maps behind (per-frame engines only).  `depth` is bit for bit what
 * _forward writes. */
int nunif_hip_depth_anything_forward_features(nunif_depth_anything *handle, const float *x, const float *pos, float *depth,
                                              int32_t B, int32_t h, int32_t w, nunif_da_features *features, void *stream);

/* ZoeDepth metric-bins head over those maps (--depth-model ZoeD_Any_N / ZoeD_Any_K): replaces `model(x)['metric_depth']` and
 * torch.nan_to_num of iw3/zoedepth_model.py:23-27 `_forward`.  Tensors carry HuggingFace's
 * ZoeDepthMetricDepthEstimationHead names (softplus bin centres, un-normed attractors, 64 bins); alpha is the attractor strength
 * (gamma 2, kind "mean"), min_temp / max_temp the conditional log-binomial's temperature range. */
typedef struct nunif_zoedepth_head nunif_zoedepth_head;
int nunif_hip_zoedepth_head_create(const nunif_tensor_desc *tensors, int32_t n_tensors, float alpha, float min_temp, float max_temp,
                                   nunif_zoedepth_head **handle);
/* rel: [B,h,w] f32 device, the relative depth (same size as features->outconv); out: [B,h,w] f32 device. */
int nunif_hip_zoedepth_head_forward(nunif_zoedepth_head *handle, const nunif_da_features *features, const float *rel, float *out,
                                    int32_t B, int32_t h, int32_t w, void *stream);
/* Bin centres of the last _forward: tap 0 = seed centres, 1..4 = behind each attractor.  dst: [B,th,tw,64] f32 device or NULL;
 * dims: host {B, th, tw} or NULL. */
int nunif_hip_zoedepth_head_debug_taps(nunif_zoedepth_head *handle, int32_t tap, float *dst, int32_t *dims, void *stream);
void nunif_hip_zoedepth_head_destroy(nunif_zoedepth_head *handle);
/* Tail of batch_preprocess (iw3/zoedepth_model.py:66-83): reflection_pad2d_loop (nunif/modules/reflection_pad2d.py:49-68; a pad
 * may exceed the map), clamp(0, 1), (x - 0.5) / 0.5.  x: [planes,h,w] f32 -> y: [planes,h+top+bottom,w+left+right] f32. */
int nunif_hip_zoedepth_pad_normalize(const float *x, float *y, int64_t planes, int32_t h, int32_t w, int32_t left, int32_t right,
                                     int32_t top, int32_t bottom, void *stream);

/* iw3 "iw3.depth_aa" (iw3/models/depth_aa.py :29-95, --depth-aa): depth anti-aliasing net.  x, y: [B,1,h,w] f32 device.
 * mode 0: forward(clamp=False); 1: forward(clamp=True) (eval default); 2: infer() = tensor-wide min-max normalise,
 * forward(clamp=False), de-normalise (what BaseDepthModel.infer(depth_aa=True) calls). */
typedef struct nunif_depth_aa nunif_depth_aa;
int nunif_hip_depth_aa_create(const nunif_tensor_desc *tensors, int32_t n_tensors, nunif_depth_aa **handle);
void nunif_hip_depth_aa_destroy(nunif_depth_aa *handle);
int nunif_hip_depth_aa_forward(nunif_depth_aa *handle, const float *x, float *y, int32_t B, int32_t h, int32_t w,
                               int32_t mode, void *stream);

/* iw3 "sbs.row_flow_v3" (iw3/models/row_flow_v3.py :33-107, the default --method): a small window-attention net that
 * turns the 3-plane feature map [depth | divergence feature | convergence feature] (iw3/backward_warp.py
 * make_input_tensor :17-64) into a horizontal flow `delta` at depth resolution.  create() takes the reference
 * state dict (keys blocks.*, last_layer.1.*).  x: [B,3,h,w] f32 device, delta: [B,1,h,w] f32 device.  flip = 1 runs the
 * net on the horizontally mirrored planes (the right eye of apply_divergence_nn_delta :191-236); delta is then in
 * the mirrored frame, which is what nunif_hip_delta_warp(flip = 1) expects. */
typedef struct nunif_row_flow nunif_row_flow;
int nunif_hip_row_flow_create(const nunif_tensor_desc *tensors, int32_t n_tensors, nunif_row_flow **handle);
void nunif_hip_row_flow_destroy(nunif_row_flow *handle);
int nunif_hip_row_flow_delta(nunif_row_flow *handle, const float *x, float *delta, int32_t B, int32_t h, int32_t w,
                             int32_t flip, void *stream);

/* iw3 "sbs.row_flow_v2" (iw3/models/row_flow_v2.py :9-92, --method row_flow_v2, the previous default): seven row
 * convolutions, delta = non_overlap + overlap_residual (_forward :44-48) as _forward_delta_only :80-86 evaluates them
 * (replicate pad 28, net, crop 28 == the unpadded stack on clamped input coordinates), in ONE launch.  create() takes
 * the reference state dict (keys feature.0.*, non_overlap.*, overlap_residual.{0,2,4,6}.*, delta_scale).  x: [B,3,h,w]
 * f32 device, delta: [B,1,h,w] f32 device, any h, w >= 1.  flip as nunif_hip_row_flow_delta: the planes are read
 * mirrored and delta stays in the mirrored frame, which is what nunif_hip_delta_warp(flip = 1) expects. */
typedef struct nunif_row_flow_v2 nunif_row_flow_v2;
int nunif_hip_row_flow_v2_create(const nunif_tensor_desc *tensors, int32_t n_tensors, nunif_row_flow_v2 **handle);
void nunif_hip_row_flow_v2_destroy(nunif_row_flow_v2 *handle);
int nunif_hip_row_flow_v2_delta(nunif_row_flow_v2 *handle, const float *x, float *delta, int32_t B, int32_t h, int32_t w,
                                int32_t flip, void *stream);
/* The same launch, also writing the intermediate maps (row_flow_v2.py :15-33) as f32 [B,C,h,w] for the tests: feature
 * (16, after ReLU), the three 1x9 ReLU outputs (16, 32, 32), non_overlap (1) and overlap_residual (1). */
int nunif_hip_row_flow_v2_debug_taps(nunif_row_flow_v2 *handle, const float *x, float *delta, float *feature, float *relu1,
                                     float *relu2, float *relu3, float *non_overlap, float *residual, int32_t B, int32_t h,
                                     int32_t w, int32_t flip, void *stream);

/* Replaces iw3/backward_warp.py backward_warp :67-83 for a horizontal flow map: grid = make_grid + [delta, 0] *
 * delta_scale at (dh, dw), bilinear (align_corners) resize to (H, W), grid_sample(bilinear, border, align_corners) +
 * clamp(0,1).  flip = 1: out = flip(backward_warp(flip(c), ...)) without materialising the flips. */
int nunif_hip_delta_warp(const float *c, const float *delta, float *out, int32_t B, int32_t C, int32_t H, int32_t W,
                         int32_t dh, int32_t dw, double delta_scale, int32_t flip, void *stream);

/* iw3 "inpaint.light_inpaint_v1" (iw3/models/light_inpaint_v1.py LightInpaintV1 :53-161), the image inpaint net behind
 * MLBWInpaintImage (iw3/mlbw_inpaint.py:78-157).  create() takes the reference state dict (mask_bias, patch.0, enc1.*, down,
 * enc2.N.*, up, dec1.*, to_image.1).  infer = LightInpaintV1.infer :106-110: preprocess (optional mask_closing, horizontal
 * dilations with FINAL iteration counts, x * (1 - mask), soft mask = clamp(gaussian15(mask) + mask)) + forward with
 * skip_i2i_offset=True.  x, out: [B,3,H,W] f32 in [0,1]; mask: [B,1,H,W] uint8 (0 / 1 hole mask).
 * The same entry points serve "inpaint.light_video_inpaint_v1" (iw3/models/light_video_inpaint_v1.py LightVideoInpaintV1
 * :92-229, base_dim 96 / lv2_mlp_ratio 1; recognised by its `patch.weight` / `to_image.weight` keys): level 2 alternates
 * 8x8-window gMLPs with temporal gMLPs over the 12 frames of each pixel, so infer takes EXACTLY B = 12 consecutive frames
 * (the host pads shorter batches by repeating the first / last frame, :141-150). */
typedef struct nunif_light_inpaint nunif_light_inpaint;
int nunif_hip_light_inpaint_create(const nunif_tensor_desc *tensors, int32_t n_tensors, nunif_light_inpaint **handle);
void nunif_hip_light_inpaint_destroy(nunif_light_inpaint *handle);
int nunif_hip_light_inpaint_infer(nunif_light_inpaint *handle, const float *x, const uint8_t *mask, float *out, int32_t B,
                                  int32_t H, int32_t W, int32_t closing, int32_t inner_iter, int32_t outer_iter, void *stream);
/* mirror_x = 1: out = flip(infer(flip(x), mask)) along the width, with `mask` given in the FLIPPED frame — the nets are trained on
 * the right view, so the reference feeds the left eye mirrored (forward_left: iw3/forward_inpaint.py:29-40, iw3/mlbw_inpaint.py:
 * 60-76 flip -> infer -> flip); here the picture is read and written at column W - 1 - x instead of two flip passes over it. */
int nunif_hip_light_inpaint_infer_ex(nunif_light_inpaint *handle, const float *x, const uint8_t *mask, float *out, int32_t B,
                                     int32_t H, int32_t W, int32_t closing, int32_t inner_iter, int32_t outer_iter,
                                     int32_t mirror_x, void *stream);
/* infer_ex that also copies out the maps of the forward (tests only; the same function body as infer_ex, the copies are
 * device-to-device between its launches).  taps: n_taps = 21 device pointers, NULL = skip:
 *   0 hard, 1 soft: f32 [B,H,W];  2 mtok: u8 [B,h1,w1];  then f16 NHWC maps: 3 patch (after the mask bias), 4 enc1.gmlp (after the
 *   gMLP and its shortcuts), 5 enc1, 6 down, 7 + 2 i enc2.i.gmlp, 8 + 2 i enc2.i (i < 5; the image net has no enc2.4), 17 up
 *   (x1 + shuffle(up)), 18 dec1.gmlp, 19 dec1, 20 to_image ([B,h1,w1,48], the video nets [B,h1,w1,64] with 48 real channels).
 * Level 1: h1 = Hp / 4, w1 = Wp / 4, C = base_dim; level 2 (down, enc2.*): h1 / 2, w1 / 2, 2 C; Hp = H + 64 - H % 64 (W alike). */
int nunif_hip_light_inpaint_debug_taps(nunif_light_inpaint *handle, const float *x, const uint8_t *mask, float *out, int32_t B,
                                       int32_t H, int32_t W, int32_t closing, int32_t inner_iter, int32_t outer_iter,
                                       int32_t mirror_x, void *const *taps, int32_t n_taps, void *stream);

/* iw3 output formats.
 * anaglyph: iw3/anaglyph.py apply_anaglyph_redcyan :96-110; left, right, out: [3,H,W] f32; mode 0 color, 1 gray, 2 half-color,
 * 3 wimmer, 4 wimmer2, 5 dubois, 6 dubois2.
 * equirectangular: iw3/equirectangular.py equirectangular_projection :7-40 (VR180); c: [C,h,w] f32 -> out: [C,Hp,Wp] with
 * Hp = h + 2*((S - h)/2), Wp = w + 2*((S - w)/2), S = max(h,w) + max(h,w)/2 (the zero padding is folded into the sampler). */
int nunif_hip_anaglyph(const float *left, const float *right, float *out, int32_t H, int32_t W, int32_t mode, void *stream);
int nunif_hip_equirectangular(const float *c, float *out, int32_t C, int32_t h, int32_t w, void *stream);

/* iw3 "sbs.mlbw" (iw3/models/mlbw.py :37-247; --method mlbw_l2 / mlbw_l4 / mlbw_l2s / mlbw_l4s): multi-layer backward
 * warp.  create() takes the reference state dict (lv1_in.1, lv2.N.*, lv1_out.1); the layer count (2 / 4) and the
 * small / full block stack are read from the tensor shapes.  x: [B,3,h,w] feature planes; delta, weight: [B,L,h,w] f32
 * (weight = softmax over the L layer logits).  flip as in nunif_hip_row_flow_delta. */
typedef struct nunif_mlbw nunif_mlbw;
int nunif_hip_mlbw_create(const nunif_tensor_desc *tensors, int32_t n_tensors, nunif_mlbw **handle);
void nunif_hip_mlbw_destroy(nunif_mlbw *handle);
int32_t nunif_hip_mlbw_num_layers(const nunif_mlbw *handle);
int nunif_hip_mlbw_delta(nunif_mlbw *handle, const float *x, float *delta, float *weight, int32_t B, int32_t h, int32_t w,
                         int32_t flip, void *stream);
/* "sbs.mask_mlbw_l2" (mlbw.py:275-278; MLBW(hole_mask=True): lv1_out has 2L + 1 channels): the extra channel is the hole
 * logit map.  mask_logits: [B,1,h,w] f32, already flipped back to image coordinates when flip != 0
 * (backward_warp.py:325-327); NULL = skip it.  has_hole_mask: 1 when the loaded weights carry the extra channel. */
int32_t nunif_hip_mlbw_has_hole_mask(const nunif_mlbw *handle);
int nunif_hip_mlbw_delta_mask(nunif_mlbw *handle, const float *x, float *delta, float *weight, float *mask_logits, int32_t B,
                              int32_t h, int32_t w, int32_t flip, void *stream);
/* iw3/backward_warp.py postprocess_hole_mask :382-393 with iw3/dilation.py closing :64-71 (n_iter = 1, 3x3),
 * dilate_inner :91-103 / dilate_outer :74-88: closing of the logits at model resolution, bilinear (align_corners) resize to
 * H x W, sigmoid > threshold, then the horizontal OR-dilations.  logits: [B,1,h,w] f32; mask: [B,1,H,W] uint8 (0 / 1);
 * work: 2*B*h*w floats followed by B*H*W bytes.  inner_iter / outer_iter are the FINAL iteration counts (the caller applies the reference's
 * max(round(W / base_width * n), 1) scaling); mask[x] = OR of the thresholded map over [x - outer_iter, x + inner_iter].
 * z (optional, [B,C,H,W] f32): the "hole fill for visualize" of apply_divergence_nn_delta_weight :333-339, z *= 1 - mask. */
int nunif_hip_hole_mask_postprocess(const float *logits, uint8_t *mask, float *work, int32_t B, int32_t h, int32_t w,
                                    int32_t H, int32_t W, float threshold, int32_t inner_iter, int32_t outer_iter, float *z,
                                    int32_t C, void *stream);

/* The composite of iw3/backward_warp.py apply_divergence_nn_delta_weight :300-321: out = clamp(sum_i
 * backward_warp(c, delta_i) * weight_i).  delta: [B,L,dh,dw]; weight: [B,L,H,W] already at image resolution (the
 * reference resizes it with bilinear + antialias: nunif_hip_resize_aa).  L <= 4, C <= 4. */
int nunif_hip_delta_weight_warp(const float *c, const float *delta, const float *weight, float *out, int32_t B, int32_t C,
                                int32_t H, int32_t W, int32_t dh, int32_t dw, int32_t L, double delta_scale, int32_t flip,
                                void *stream);

/* Replaces iw3/backward_warp.py apply_divergence_grid_sample :96-121 (make_grid + backward_warp + grid_sample
 * bilinear/border/align_corners=True + clamp).  c: [B,C,H,W]; depth: [B,1,dh,dw] (grid is built at depth
 * resolution and bilinearly resized, as the reference does). */
int nunif_hip_backward_warp(const float *c, const float *depth, float *left, float *right, int32_t B, int32_t C,
                            int32_t H, int32_t W, int32_t dh, int32_t dw, double divergence, double convergence,
                            int32_t synthetic_view, void *stream, const float *convergence_dev);
/* (convergence_dev: optional [B] f32 device, a convergence per frame as in nunif_forward_warp_params; NULL = the scalar) */

/* F.interpolate(..., antialias=True) for planar fp32 maps: bilinear (bicubic=0) or bicubic a=-0.5 (bicubic=1),
 * with ATen's coordinate rules (align_corners changes only the scale when antialias is on — SURVEY.md App. C).
 * Optional fused clamp to [0,1] and (x-mean[c])/std[c] over 3-channel groups (iw3/depth_anything_model.py
 * batch_preprocess :103-109; mean3/std3 are HOST pointers or NULL).  tmp: [planes,h_in,w_out] floats. */
int nunif_hip_resize_aa(const float *x, float *y, float *tmp, int64_t planes, int32_t h_in, int32_t w_in,
                        int32_t h_out, int32_t w_out, int32_t bicubic, int32_t align_corners, int32_t clamp01,
                        const float *mean3, const float *std3, void *stream);

/* Replaces iw3/dilation.py dilate_edge :116-142.  x,y: [B,1,H,W]; work: nunif_hip_dilate_edge_work_floats(B,H,W) floats of
 * scratch (a ping-pong image + the per-workgroup range statistics that carry edge_weight's mean / std / min / max from one
 * iteration's kernel to the next: n iterations are n + 1 launches). */
int64_t nunif_hip_dilate_edge_work_floats(int32_t B, int32_t H, int32_t W);
int nunif_hip_dilate_edge(const float *x, float *y, float *work, int32_t B, int32_t H, int32_t W, int32_t n_x,
                          int32_t n_y, void *stream);

/* Per-image (x-min)/(max-min) clamped to [0,1] (iw3/depth_scaler.py minmax_normalize :4-17 with the frame's own
 * min/max, i.e. EMA off).  minmax: [B,2] device scratch that receives the order-keyed min/max. */
int nunif_hip_minmax_normalize(const float *x, float *y, float *minmax, int32_t B, int64_t n_per, void *stream);

/* EMAMinMaxScaler on the device (iw3/depth_scaler.py MinMaxBuffer :33-61, EMAMinMaxScaler.update :95-114, flush :116-133):
 * the reference's 0-dim-tensor arithmetic (amin / amax of the frame, ring insert, ring amin / amax, the EMA recurrence, the
 * `if scale > 0` host sync, (x - lo) / scale, clamp) as four kernels on a small device state block, no host round trip.
 *   nunif_hip_minmax: minmax_keys[B][2] <- order-keyed min / max of every item of x [B, n_per]
 *   nunif_hip_ema_scaler_push: one frame's keys into state = [ring 2N | min_value | max_value]; `count` is
 *     MinMaxBuffer.count before the add, `filled` whether the ring is full after it, `first` whether no EMA value exists yet
 *   nunif_hip_ema_scaler_ring_minmax: state[2N], state[2N+1] <- extrema of the ring (flush before the first EMA value)
 *   nunif_hip_range_normalize: y = clamp((x - lo) / (hi - lo)) (max_mode: clamp(x / hi)) with lohi[2] on the device */
int nunif_hip_minmax(const float *x, float *minmax_keys, int32_t B, int64_t n_per, void *stream);
int nunif_hip_ema_scaler_push(float *state, const float *minmax_keys, int32_t ring_size, int64_t count, int32_t filled,
                              int32_t first, double decay, void *stream);
int nunif_hip_ema_scaler_ring_minmax(float *state, int32_t ring_size, void *stream);
int nunif_hip_range_normalize(const float *x, float *y, const float *lohi, int64_t n, int32_t max_mode, void *stream);

/* iw3/backward_warp.py make_input_tensor :33-64 with c = None for a whole batch: out [B,3,H,W] = depth | divergence plane |
 * convergence plane, with the screen-border taper of `border_pix` columns (0: none). */
int nunif_hip_make_input_planes(const float *depth, float *out, int32_t B, int32_t H, int32_t W, double divergence_value,
                                double convergence_value, int32_t border_pix, void *stream, const float *convergence_dev);
/* (convergence_dev: optional [B] f32 device, a convergence per frame; convergence_value then is -divergence_pix and the plane of
 *  frame b holds fp32(convergence_value * convergence_dev[b] / 32), make_divergence_feature_value :24-29 with that frame's value) */

/* torch.stack of n <= 16 equally sized device buffers into dst (one launch; the per-frame tensors of a batch). */
int nunif_hip_stack(const void *const *srcs, int32_t n, int64_t bytes_each, void *dst, void *stream);

/* Stand-alone mask morphology on fp32 0/1 masks [B,H,W] (iw3/dilation.py dilate :41-46, erode :49-54, closing :57-64,
 * mask_closing :145-153, dilate_outer :67-81, dilate_inner :84-98).  op: 0 dilate x n_a (3x3 max, window clipped at the border),
 * 1 erode x n_a, 2 closing(n_iter = n_a), 3 mask_closing(n_iter = n_a) = clamp(closing + mask), 4 horizontal OR-dilation with
 * n_a steps of dilate_inner (pixel x takes x+1) and n_b steps of dilate_outer (pixel x takes x-1).  work: B*H*W floats. */
int nunif_hip_mask_morphology(const float *in, float *out, float *work, int32_t B, int32_t H, int32_t W, int32_t op,
                              int32_t n_a, int32_t n_b, void *stream);

/* VideoDepthAnything pre/post glue (iw3/video_depth_anything_model.py:51-91).
 * reflection_pad2d: nunif/modules/reflection_pad2d.py reflection_pad2d_naive :13-48 on planar fp32 [planes,H,W] -> [planes,
 *   H+top+bottom, W+left+right]; positive pads reflect without repeating the edge, negative pads crop (the F.pad(out, (-14,)*4)
 *   of _postprocess :79).
 * depth_postprocess: _postprocess :66-76 — nan_to_num, clamp(max=max_dist) when max_dist > 0, metric depth -> disparity
 *   1/(d+eps) when to_disparity, optional sign flip (the "-out" for non-disparity outputs :88-90).  In place allowed. */
int nunif_hip_reflection_pad2d(const float *x, float *y, int64_t planes, int32_t H, int32_t W, int32_t left, int32_t right,
                               int32_t top, int32_t bottom, void *stream);
int nunif_hip_depth_postprocess(const float *x, float *y, int64_t n, float max_dist, int32_t to_disparity, float eps,
                                int32_t negate, void *stream);

/* Frame edge.  frame: HWC [H,W,3] uint8 (bits=8) or uint16 (bits=16) device memory.
 * frame_to_tensor replaces nunif/utils/video.py to_tensor :218-223 (x.permute(2,0,1) / iinfo.max).
 * stereo_to_frame fuses iw3/utils.py postprocess_image :468-479 (cat + clamp) with video.py from_tensor :236-245
 * ((x*max).round().to(uint)); layout 0 = left|right, 1 = right|left (cross-eyed), 2 = left over right (top-bottom),
 * 3 = the left image alone (right may be NULL): clamp + quantise of a single frame.
 * stereo_compose is the same composition with a planar fp32 result [3,Ho,Wo]. */
int nunif_hip_frame_to_tensor(const void *frame, float *chw, int32_t H, int32_t W, int32_t bits, void *stream);
int nunif_hip_stereo_to_frame(const float *left, const float *right, void *frame, int32_t H, int32_t W,
                              int32_t layout, int32_t bits, void *stream);
int nunif_hip_stereo_compose(const float *left, const float *right, float *out, int32_t H, int32_t W,
                             int32_t layout, void *stream);

/* Film grain (waifu2x --grain) and the rotated frame entry of the waifu2x video loop.
 * The random stream is Philox-4x32-10 keyed by `seed`, with counter (x >> 2, plane * H + y, `counter`, component): a value
 * depends on (seed, counter, element coordinates) only — not on launch shape, tile order or stream.  Values differ from torch's
 * for any seed; the distribution is the reference's.  `counter` must be below 2^63.
 * rgb_noise replaces nunif/utils/rgb_noise.py rgb_noise_like :5-18 on planar fp32 [planes,H,W] (planes = 3 or B*3).
 *   component 0: the function's result for `level` (1: n1 ~ N(0,1); 2: 0.5*n1 + 0.5*up(n2), n2 ~ N(0,1) on [H/2,W/2], `up` =
 *   torch's nearest resize); 1: n1 alone; 2: up(n2) alone; 3: the n2 grid itself, out = [planes,H/2,W/2].
 * apply_rgb_noise replaces rgb_noise.py apply_rgb_noise :21-39 on n fp32 values (any shape; out may alias rgb).
 * grain_blend replaces waifu2x/ui_utils.py :169-174: buf = noise when `first` (first frame / shape change), else
 *   buf = buf*(1-speed) + noise*speed.
 * grain_video_step fuses ui_utils.py :167-177 for one frame: draw rgb_noise_like(level), update noise_buffer [3,H,W] as
 *   grain_blend does, apply_rgb_noise, then video.py from_tensor :236-245 ((x*max).round()) into the HWC frame (uint8 for
 *   bits=8, uint16 for bits=16; device or pinned host memory).  Same bytes as rgb_noise -> grain_blend -> apply_rgb_noise ->
 *   stereo_to_frame(layout 3) with the same seed and counter.
 * frame_to_tensor_rot replaces video.py to_tensor :218-223 followed by torch.rot90(x, turns, (-2,-1)) of ui_utils.py
 *   :159-162 (turns 1 = --rotate-left, 3 = --rotate-right): frame HWC [H,W,3] -> chw [3,W,H]. */
int nunif_hip_rgb_noise(float *out, int32_t planes, int32_t H, int32_t W, int32_t level, int32_t component, uint64_t seed,
                        uint64_t counter, void *stream);
int nunif_hip_apply_rgb_noise(const float *rgb, const float *noise, float *out, int64_t n, double strength, double gamma,
                              int32_t light_decay, double light_decay_strength, void *stream);
int nunif_hip_grain_blend(float *buf, const float *noise, int64_t n, double speed, int32_t first, void *stream);
int nunif_hip_grain_video_step(const float *rgb, float *noise_buffer, void *frame, int32_t H, int32_t W, int32_t bits,
                               int32_t level, uint64_t seed, uint64_t counter, double speed, int32_t first, double strength,
                               double gamma, int32_t light_decay, double light_decay_strength, void *stream);
int nunif_hip_frame_to_tensor_rot(const void *frame, float *chw, int32_t H, int32_t W, int32_t bits, int32_t turns,
                                  void *stream);

/* Pointwise depth -> disparity mappers of iw3/mapper.py :7-118.  kind: 0 identity, 1 pow2, 2 softplus01_legacy(c=p0),
 * 3 softplus01(bias=p0, scale=p1), 4 inv_softplus01(bias=p0, scale=p1), 5 distance_to_disparity(c=p0),
 * 6 shift_relative_depth(min_distance=p0, max_distance=p1). */
int nunif_hip_map_depth(const float *x, float *y, int64_t n, int32_t kind, double p0, double p1, void *stream);

/* TransNetV2 shot-boundary network (nunif/utils/transnetv2.py TransNetV2 :7-87 as `TransNetV2()` builds it: F=16, L=3, S=2,
 * D=1024, frame similarity :220-259 and colour histograms :262-316 on, many-hot head on, no mean pooling), eval mode, fp32
 * operands and accumulation (the reference runs it without autocast, nunif/utils/shot_boundary_detection.py:42).
 * create() takes the weights already packed on the host (nunif_amd/nunif/utils/transnetv2.py pack_weights), BatchNorm3d folded:
 *   b{0..2}.l{0,1}.ws  [ceil16(9*Cin)][8F']  the four branches' (1,3,3) kernels, row = (kh*3+kw)*Cin + c, column = branch*2F' + o
 *   b{..}.l{..}.wt     [4][6F'][max(F',32)]  the (3,1,1) kernels x BN scale, row = tap*2F' + c, zero-padded columns
 *   b{..}.l{..}.bias   [4F']                 BN shift
 *   proj.wt [448][128], proj.b; sim.wt / hist.wt [101][128], sim.b / hist.b; fc1.wt [4864][1024], fc1.b; cls1.w / cls2.w [1024],
 *   cls1.b / cls2.b [1]                      (Linear weights transposed to [in][out])
 * `filters` is F of the constructor; only 16 is built (NUNIF_HIP_EUNSUPPORTED otherwise).
 * forward: frames [B,T,3,27,48] f32 device, the values as the caller hands them in (the histogram branch takes int(v) >> 5 of
 * them, as the reference does); one_hot, many_hot, sigmoid_out: [B,T] f32 device, logits of cls_layer1 / cls_layer2 and
 * sigmoid(one_hot) (:45 of shot_boundary_detection.py); many_hot and sigmoid_out may be NULL.  Any T >= 1, B*T <= 4096.
 * Scratch is owned by the handle: calls on one handle must be ordered (one stream at a time). */
typedef struct nunif_transnetv2 nunif_transnetv2;
int nunif_hip_transnetv2_create(const nunif_tensor_desc *tensors, int32_t n_tensors, int32_t filters,
                                nunif_transnetv2 **handle);
void nunif_hip_transnetv2_destroy(nunif_transnetv2 *handle);
int nunif_hip_transnetv2_forward(nunif_transnetv2 *handle, const float *frames, int32_t B, int32_t T, float *one_hot,
                                 float *many_hot, float *sigmoid_out, void *stream);

/* SOD v1 saliency estimator of iw3's auto convergence (--convergence-mode sod_v1): iw3/models/sod_v1.py SODV1 :9-56 =
 * U2NETP(in_ch=6) of nunif/utils/u2netp.py :321-430 (RSU7 :44-116, RSU6 :119-182, RSU5 :185-238, RSU4 :241-284, RSU4F :287-318,
 * REBNCONV :11-35 with BatchNorm folded as fuse() :20-26 does), eval mode, fp32 operands and accumulation, net size 192.
 * create() takes the weights packed on the host (nunif_amd/iw3/models/sod_v1.py pack_weights), all fp32:
 *   <stage>.<rebnconv>.w [Cout/8][Cin][9][8]  BN-folded 3x3 kernel, (co / 8, ci, kh*3+kw, co % 8);  <stage>.<rebnconv>.b [Cout]
 *   side.w [6][64][9], side.b [6]             side1 .. side6;   outconv.w [6], outconv.b [1]
 * net_size must be 192 (MaxPool2d(ceil_mode=True) is built for even maps only; NUNIF_HIP_EUNSUPPORTED otherwise).
 * forward replaces SODV1.infer :49-56: rgb [B,3,H,W] and depth [B,1,h,w] f32 device, any H, W, h, w -> saliency [B,1,192,192]
 *   (sigmoid, u2netp.py:430) and depth_scaled [B,1,192,192] (the bilinear resize of depth, :52).  workspace: caller-owned device
 *   floats, nunif_hip_sod_v1_workspace_floats(B) of them, so that calls on different streams never share scratch.
 * entry is forward's first launch alone (:51-54 + to_feature :31-35 + the cat :41): x6 [B,6,192,192].
 * debug_taps (tests only) copies one of the maps hx1 .. hx6, hx1d (u2netp.py:368-404) of the forward that last ran on `workspace`
 *   into out ([B,64,S,S] f32 device, shape4 receives the shape).
 * depth_position replaces ConvergenceEstimator.depth_position_from_ratio (iw3/convergence_estimator.py:33-59): saliency and depth
 *   [B][n] f32 -> out [B] f32, all on the device.  ema replaces the loop of __call__ :69-82: state = {ema, has_value} on the
 *   device, bit i of reset_mask = reset_pts[i] (B <= 64). */
typedef struct nunif_sod_v1 nunif_sod_v1;
int nunif_hip_sod_v1_create(const nunif_tensor_desc *tensors, int32_t n_tensors, int32_t net_size, nunif_sod_v1 **handle);
void nunif_hip_sod_v1_destroy(nunif_sod_v1 *handle);
int64_t nunif_hip_sod_v1_workspace_floats(int32_t B);
int nunif_hip_sod_v1_forward(nunif_sod_v1 *handle, const float *rgb, int32_t H, int32_t W, const float *depth, int32_t h,
                             int32_t w, int32_t B, float *workspace, float *saliency, float *depth_scaled, void *stream);
int nunif_hip_sod_v1_entry(const float *rgb, int32_t H, int32_t W, const float *depth, int32_t h, int32_t w, int32_t B,
                           float *x6, float *depth_scaled, void *stream);
int nunif_hip_sod_v1_debug_taps(nunif_sod_v1 *handle, const float *workspace, int32_t B, const char *name, float *out,
                                int64_t capacity, int64_t *shape4, void *stream);
int nunif_hip_sod_v1_depth_position(const float *saliency, const float *depth, int32_t B, int64_t n, double pos, float *out,
                                    void *stream);
int nunif_hip_sod_v1_ema(const float *z, float *out, int32_t B, float *state, double decay, uint64_t reset_mask, void *stream);

/* stlizer's per-frame networks and warp (nunif/utils/superpoint.py), fp32 operands and accumulation throughout.
 * Inputs must be finite, with one exception: texels of the warp's image may be NaN (they propagate as in torch).  A NaN score,
 * descriptor or warp parameter is not treated as torch treats it: the NMS maximum skips a NaN where max_pool2d propagates it,
 * match returns index 0 and a NaN similarity for a row with a NaN where torch.argmax returns the NaN's index, and the warp's
 * border clamp turns a NaN coordinate into 0.
 *
 * SuperPoint :74-172 as `SuperPoint()` builds it (channels [64, 64, 128, 128, 256], descriptor_dim 256, stride 8), eval mode.
 * create() takes the weights packed on the host (nunif_amd/nunif/utils/superpoint.py pack_weights); a VGGBlock :55-71 is
 * conv -> ReLU -> BatchNorm(eps 1e-3), so the 3x3 convs carry their BN as a per-channel affine applied after the ReLU:
 *   backbone.{0..3}.{0,1}.w  [9*Cin][Cout]   row = (kh*3+kw)*Cin + c;  .bias / .scale / .shift [Cout]
 *   heads.w                  [1152][512]     detector.0 (columns 0..255) and descriptor.0 (256..511); .bias / .scale / .shift [512]
 *   detector.w               [256][96]       detector.1 with its BN folded (relu=False), 65 real columns; detector.bias [96]
 *   descriptor.w             [256][256]      descriptor.1 with its BN folded; descriptor.bias [256]
 * forward :111-149: image [B,C,H,W] f32 device, C = 3 (reduced to gray :112-114 inside the first conv's gather) or 1; H, W >= 8,
 * any size (each of the three 2x2 max-pools floors).  With h = H/8, w = W/8 (floored three times) it leaves in the handle the
 * score map [B,8h,8w] (softmax over 65, dustbin dropped, depth-to-space :122-128) and the L2-normalised dense descriptors
 * [B,h,w,256] (channels-last), then runs nunif_hip_superpoint_keypoints on the score map.  keypoints [B][8h*8w][2] f32 (x, y),
 * kp_scores [B][8h*8w] f32 and counts [B] i32 are device buffers; image b has counts[b] valid entries in the row-major order of
 * torch.where.  keypoints may be NULL (dense outputs only).  The launch plan (buffer layout of one input shape) is kept in the
 * handle and rebuilt when (B, H, W) changes; calls on one handle must be ordered (one stream at a time).
 * debug_taps copies one buffer of the last forward: "backbone.0" .. "backbone.3" (block outputs, after the pool where the block
 * has one), "heads", "descriptors" (all [B,h,w,C] channels-last), "scores", "nms" ([B,1,8h,8w]); shape4 receives the shape.
 * sample: sample_descriptors :16-27 of the last forward's dense map of image b at n keypoints (x, y) -> out [n][256]. */
typedef struct nunif_superpoint nunif_superpoint;
int nunif_hip_superpoint_create(const nunif_tensor_desc *tensors, int32_t n_tensors, nunif_superpoint **handle);
void nunif_hip_superpoint_destroy(nunif_superpoint *handle);
int nunif_hip_superpoint_forward(nunif_superpoint *handle, const float *image, int32_t B, int32_t C, int32_t H, int32_t W,
                                 int32_t nms_radius, int32_t remove_borders, float threshold, float *keypoints,
                                 float *kp_scores, int32_t *counts, void *stream);
int nunif_hip_superpoint_debug_taps(nunif_superpoint *handle, const char *name, float *out, int64_t capacity, int64_t *shape4,
                                    void *stream);
int nunif_hip_superpoint_sample(nunif_superpoint *handle, int32_t b, const float *keypoints, int32_t n, float *out,
                                void *stream);

/* batched_nms :30-45 (radius 0..8; cells outside the image count as -inf, as in max_pool2d), the remove_borders band set to -1
 * :132-137, `score > threshold` and the row-major compaction of torch.where :141-149, on score maps [B,H,W] f32.  Comparisons
 * only: exact for finite scores.  work: nunif_hip_superpoint_keypoints_work_floats(B, H, W) floats; nms_out [B,H,W] receives the suppressed map
 * (with the band); keypoints [B][H*W][2] / kp_scores [B][H*W] / counts [B] as in forward, or keypoints NULL for the map only. */
int64_t nunif_hip_superpoint_keypoints_work_floats(int32_t B, int32_t H, int32_t W);
int nunif_hip_superpoint_keypoints(const float *scores, int32_t B, int32_t H, int32_t W, int32_t nms_radius,
                                   int32_t remove_borders, float threshold, float *work, float *nms_out, float *keypoints,
                                   float *kp_scores, int32_t *counts, void *stream);

/* sample_descriptors :16-27: bilinear grid_sample (align_corners=False, zeros padding) of a channels-last dense map [h,w,C]
 * (C % 4 == 0, C <= 1024) at (kp + 0.5) / (stride * [w, h]), then the L2 norm over C; keypoints [n][2] (x, y), out [n][C]. */
int nunif_hip_sample_descriptors(const float *keypoints, int32_t n, const float *dense, int32_t h, int32_t w, int32_t C,
                                 int32_t stride, float *out, void *stream);

/* find_match_index :206-223 up to its threshold filter: for every row of d1 [n1][D] the max and argmax over j of <d1[i], d2[j]>,
 * d2 [n2][D]; on equal values the lowest j wins, as torch.argmax.  The n1 x n2 matrix is never written.  work: n1 * 8 bytes;
 * index [n1] i64, max_similarity [n1] f32.  n1, n2 >= 1, D % 4 == 0. */
int nunif_hip_superpoint_match(const float *d1, int32_t n1, const float *d2, int32_t n2, int32_t D, void *work, int64_t *index,
                               float *max_similarity, void *stream);

/* apply_transform :330-378: x, out [B,C,H,W] f32 (distinct buffers); params [B][6] f32 device = shift x, shift y, scale, angle in
 * degrees, center x, center y.  Inverse rotation / scale / shift about the center in fp32 in the reference's order, then a
 * four-tap bilinear grid_sample with align_corners=False; padding_mode 0 zeros, 1 border (NUNIF_HIP_EUNSUPPORTED otherwise). */
int nunif_hip_affine_warp(const float *x, const float *params, float *out, int32_t B, int32_t C, int32_t H, int32_t W,
                          int32_t padding_mode, void *stream);

/* stlizer --border outpaint / expand_outpaint: LightOutpaintV1 (stlizer/models/light_outpaint_v1.py) and the EMA frame buffer of
 * pass 4 (stlizer/multipass_pipeline.py:447-474), fp32 operands and accumulation throughout.  Inputs must be finite (the buffer
 * step's frames excepted: their NaN are the mask).
 *
 * create() takes the weights packed on the host (nunif_amd/stlizer/models/light_outpaint_v1.py pack_weights), all f32:
 *   dct.{0,1,2}.w [9*Cin][Cout] (row = (kh*3+kw)*Cin + c), .b [Cout]        Downsampling :54-71, channels 4 -> 8 -> 16 -> 64
 *   <blk>.mha.qkv.w [C][3C], .b [3C]    MHA.qkv_proj (nunif/modules/attention.py:106) input-major, the columns of head h at
 *                                       96 h + (q | k | v) * 32;  <blk> = enc (C 64), mid0, mid1 (C 32), dec (C 64)
 *   <blk>.mha.table [64][64]            WindowScoreBias.forward() (attention.py:408-415), one table for all heads
 *   <blk>.mha.proj.w [C][C], .b         MHA.head_proj, input-major;  <blk>.mha.mlp1.w [C][2C], .b and .mlp2.w [C][C], .b  MHABlock.mlp
 *   <blk>.pool.pw1.w [C][2C], .b        PoolBlock.mlp.0 :17, the columns of chunk j at 64 j: channels 32 j .. 32 j + 31, then C + the same
 *   <blk>.pool.dw.w [9][2C], .b [2C]    the depthwise conv :20 tap-major;  <blk>.pool.pw2.w [C][C], .b  mlp.5 :23
 *   proj_mid.w [64][32], .b; proj_out.w [32][64], .b  :95-96;  to_image.w [3][64], .b [3]  ToImageBilinaer.proj :77
 * infer: x [B,3,H,W] f32, mask [B,1,H,W] u8 (non-zero = to be painted), out [B,3,H,W] f32 (not x).  mode 0 `composite` is
 *   LightOutpaintV1.infer(composite=True) :175-204, 1 `raw` is infer(composite=False) :205-206, 2 `forward` is the eval-mode forward
 *   :164-173 on what infer's net call returns (pass max_size >= max(H, W) for the reference's forward, which never resizes).
 *   All of :175-206 and OutpaintBase.forward / _forward :115-153 run inside: the resize to max_size (new side =
 *   round-half-even(side * (max_size / long side)) in double, as Python), the 3x3 mask dilation and > 0.5 threshold, the zeroing,
 *   the replicate pad to a multiple of 64 with its mask of ones, x * (1 - mask) ONLY when a pad was needed, the net, the x8
 *   bilinear upsample, the crop, the resize back and the composite.  work: nunif_hip_outpaint_work_bytes(B, H, W, max_size) bytes
 *   of caller-owned device memory, 16-byte aligned; the handle keeps no per-call state, so calls on different streams with
 *   different work buffers may overlap.  work_bytes returns -1 for a shape infer refuses.
 * debug_taps copies one channels-last map [B,h,w,C] (h = padded height / 8) of the infer call that last wrote `work` (same B, H, W,
 *   max_size): "dct" (after the three convs :117), "enc" (:118), "mid" (after the skip add :119), "dec" (:120), all C = 64, and
 *   "proj", the 3-channel map before the upsample (:82).
 * buffer_step replaces multipass_pipeline.py:452-453 and :461-471 for a batch, one launch each: with coarse == NULL it writes
 *   out = frames with NaN -> 0 and mask0 [B,1,H,W] u8 = isnan(frames[:, 0]) (what infer takes in); with coarse [B,3,H,W] (the
 *   raw net output) it visits the frames in order per element: reset[j] != 0 sets buffer = coarse_j (:464-466; the caller sets it
 *   for the first frame ever and for scene_weight < 0.01), buffer = buffer * d + coarse_j * (1 - d) (:468-469), out_j = clamp(
 *   isnan(frames_j) ? buffer : frames_j, 0, 1) (:470-471, the mask per element).  buffer [3,H,W] f32 and reset [B] u8 are device
 *   memory; d = buffer_decay is the blend weight AFTER :456-458.  One thread owns an element across the batch: no atomics. */
typedef struct nunif_outpaint nunif_outpaint;
int nunif_hip_outpaint_create(const nunif_tensor_desc *tensors, int32_t n_tensors, nunif_outpaint **handle);
void nunif_hip_outpaint_destroy(nunif_outpaint *handle);
int64_t nunif_hip_outpaint_work_bytes(int32_t B, int32_t H, int32_t W, int32_t max_size);
int nunif_hip_outpaint_infer(nunif_outpaint *handle, const float *x, const uint8_t *mask, int32_t B, int32_t H, int32_t W,
                             int32_t max_size, int32_t mode, float *out, void *work, void *stream);
int nunif_hip_outpaint_debug_taps(nunif_outpaint *handle, const void *work, int32_t B, int32_t H, int32_t W, int32_t max_size,
                                  const char *name, float *out, int64_t capacity, int64_t *shape4, void *stream);
int nunif_hip_outpaint_buffer_step(const float *frames, const float *coarse, float *buffer, const uint8_t *reset,
                                   double buffer_decay, int32_t B, int32_t H, int32_t W, float *out, uint8_t *mask0,
                                   void *stream);

/* iw3 --autocrop (nunif/utils/autocrop.py): the letterbox detector and the crop / uncrop copy.
 * stats replaces AutoCropDetector.detect_tb :140-154 and detect_lr :156-170 (with rgb_to_y :117-138) and the accumulation of
 *   update :24-48 for a batch: x [B,3,H,W] f32 device; flat = 0 the black modes (Y clamped to the TV range, mean <= 32/255 and
 *   max |y - mean| < 16/255), 1 the flat modes (lower median as torch.median, fraction of |y - median| < 16/255 above 0.99);
 *   passes bit 0 = rows (tb), bit 1 = columns (lr); only what is asked for is computed.  Every decision is ADDED to the device
 *   counters border_count_tb [H] / border_count_lr [W] (i32; one thread owns a counter: no atomics, bit-identical on every call
 *   and stream).  A fixed number of launches whatever B, no host sync.  work: caller-owned device scratch of the black lr pass,
 *   B * ceil(H / 32) * W * 16 bytes, 16-byte aligned (unused otherwise, may be NULL).  H <= 4608, W <= 8192 (the LDS tiling of the
 *   flat modes: 8 column lines of H floats, 4 row lines of W floats); larger frames are refused.  Inputs must be finite.
 * debug_stats (tests) is stats that also writes the statistic vectors: row_a / col_a the mean (black) or median (flat), row_b /
 *   col_b the max deviation (black) or the fraction (flat), [B][H] and [B][W] f32; the counters may then be NULL.
 * crop_pad replaces AutoCrop.crop :346-354 (as a contiguous copy) and AutoCrop.uncrop :356-360 (F.pad, constant): src [N][sH][sW]
 *   and dst [N][dH][dW] f32 (N = batch x channels, distinct buffers); the window of win_h x win_w at (y0, x0) of src lands at
 *   (pad_top, pad_left) of dst, everything else of dst is pad_value.  The window must lie inside both. */
int nunif_hip_autocrop_stats(const float *x, int32_t B, int32_t H, int32_t W, int32_t flat, int32_t passes,
                             int32_t *border_count_tb, int32_t *border_count_lr, void *work, int64_t work_bytes, void *stream);
int nunif_hip_autocrop_debug_stats(const float *x, int32_t B, int32_t H, int32_t W, int32_t flat, int32_t passes,
                                   int32_t *border_count_tb, int32_t *border_count_lr, void *work, int64_t work_bytes,
                                   float *row_a, float *row_b, float *col_a, float *col_b, void *stream);
int nunif_hip_autocrop_crop_pad(const float *src, float *dst, int64_t N, int32_t sH, int32_t sW, int32_t dH, int32_t dW,
                                int32_t y0, int32_t x0, int32_t pad_top, int32_t pad_left, int32_t win_h, int32_t win_w,
                                float pad_value, void *stream);

/* iw3 desktop streaming (iw3/desktop/utils.py:99-123 to_uint8 + to_jpeg_data, called per frame at :383-389): a baseline JPEG
 * encoder on the device, so that a frame crosses to the host as its JPEG stream and not as a uint8 image.  The encoder holds no
 * weights: plain functions and a caller-owned workspace.  DESIGN.md ("JPEG frame encoder") states it step by step.
 * quant_tables, header, max_bytes and workspace_bytes are host-only arithmetic (nunif_amd/csrc/jpeg_host.h), no GPU needed.
 * quant_tables: the IJG scaling of the ITU T.81 Annex K tables for quality 1..100, baseline-clamped to 1..255 (libjpeg's
 *   jpeg_set_quality(q, TRUE)), natural (row-major) order, into luma[64] and chroma[64] (host).
 * header: SOI, APP0 (JFIF 1.01, units 0, 1:1), DQT x 2 (8 bit, zigzag), SOF0, DHT x 4 (Annex K), DRI, SOS into out (host,
 *   capacity >= 629); returns the length (629) or a negative status.
 * max_bytes: an upper bound of the stream of one frame: the header, per block its worst case of 1 660 bits, per interval the fill
 *   of its last byte, every byte counted twice (a stuffed 0xFF), and the 2-byte RSTn / EOI marker.  -1 for a refused shape.
 * workspace_bytes: the size of `workspace` for encode: coefficients [B][blocks][64] i16, two i32 per interval, and per interval
 *   a staging slot of its worst case.  -1 for a refused shape.
 * encode: rgb [B,3,H,W] f32 contiguous device memory in [0,1] (clamped; values are quantised as to_uint8 does, round half even)
 *   -> B baseline JFIF streams, stream b at out + b * capacity (device), its length in out_len[b] (device i32).  subsampling 420
 *   or 444; a restart interval of restart_mcus MCUs (1..65535; it may span MCU rows; intervals are the unit of parallelism).
 *   Four launches on `stream`, no host synchronisation, no atomics on global memory: the bytes depend on the input alone.  If
 *   capacity is smaller than the stream, out_len[b] = -1 and nothing of slot b is written; max_bytes is always enough.  workspace:
 *   workspace_bytes() bytes of device memory, 256-byte aligned; calls that overlap need their own.  1 <= H, W <= 8192, B <= 16,
 *   quality 1..100; anything else is refused.
 * debug_coefficients (tests) runs the first launch alone: the quantised coefficients in scan order, [B][mcus * blocks_per_mcu][64]
 *   i16 device memory: MCU by MCU in raster order, Y00 Y01 Y10 Y11 Cb Cr (420) or Y Cb Cr (444), each block in zigzag order. */
int nunif_hip_jpeg_quant_tables(int32_t quality, uint8_t *luma, uint8_t *chroma);
int64_t nunif_hip_jpeg_header(int32_t H, int32_t W, int32_t quality, int32_t subsampling, int32_t restart_mcus, uint8_t *out,
                              int64_t capacity);
int64_t nunif_hip_jpeg_max_bytes(int32_t H, int32_t W, int32_t subsampling, int32_t restart_mcus);
int64_t nunif_hip_jpeg_workspace_bytes(int32_t B, int32_t H, int32_t W, int32_t subsampling, int32_t restart_mcus);
int nunif_hip_jpeg_encode(const float *rgb, int32_t B, int32_t H, int32_t W, int32_t quality, int32_t subsampling,
                          int32_t restart_mcus, uint8_t *out, int64_t capacity, int32_t *out_len, void *workspace, void *stream);
int nunif_hip_jpeg_debug_coefficients(const float *rgb, int32_t B, int32_t H, int32_t W, int32_t quality, int32_t subsampling,
                                      int16_t *coef, void *stream);

/* HDR -> SDR tone mapping of one decoded frame (nunif/utils/video.py:309-416 hdr2sdr, called per frame by process_video's
 * input_reformatter :1025-1036): x / 65535 (:325), inverse EOTF (PQ :330-333, HLG :338-344), exposure (:354), Hable map over the
 * Hable map of the white point (:356-369), the HLG luma mix (:363-367), the BT.2020 -> bt709 / bt601 matrix (:372-387), clamp,
 * OETF with its linear toe (:391-395), clamp, in ONE launch.  DESIGN.md ("HDR to SDR") states how the powers are evaluated.
 * src: rgb48 HWC [H][W][3], uint16, in device memory or pinned host memory (read zero-copy).  trc: 16 (SMPTE 2084, PQ) or 18
 * (ARIB STD-B67, HLG); colorspace: 709 or 601; H, W <= 8192; anything else is refused with NUNIF_HIP_EINVAL.
 * params: exposure and white_point of the curve in use (pq_* for trc 16, hlg_* for trc 18); saturation_gain is read for HLG only.
 * form 0 (u16): dst HWC uint16 = trunc(v * 65535), what the reference's function returns (:398); device or pinned host memory.
 * form 1 (chw): dst [3][H][W] fp32 = float(trunc(v * 65535)) / 65535 by IEEE division: what VU.to_tensor (:218-223) makes of the
 *   reference's frame.
 * form 2 (debug, tests): dst HWC fp32 = v itself, the value before `* 65535`.
 * hdr2sdr_constants is host-only: the matrix (row major, 9 floats) and hable_map(white_point) in the reference's fp32 expressions,
 *   exactly the kernel's arguments. */
typedef struct nunif_hdr2sdr_params {
    double exposure, white_point, saturation_gain;
} nunif_hdr2sdr_params;
int nunif_hip_hdr2sdr(const void *src, void *dst, int32_t H, int32_t W, int32_t trc, int32_t colorspace,
                      const nunif_hdr2sdr_params *params, int32_t form, void *stream);
int nunif_hip_hdr2sdr_constants(int32_t trc, int32_t colorspace, const nunif_hdr2sdr_params *params, float *matrix,
                                float *hable_white);

/* Planar YUV <-> the CHW fp32 tensor: the two pixel-format conversions of process_video (nunif/utils/video.py), one launch each,
 * no host synchronisation, no atomics.  DESIGN.md ("Pixel formats") and csrc/pixfmt.hip state the arithmetic: ITU coefficients in
 * fp32 and linear chroma resampling for the MPEG-2 / H.264 default chroma position — deliberately not swscale's fixed point.
 * format: 0 yuv420p, 1 yuv444p (uint8), 2 yuv420p10le (uint16, 10 significant bits); matrix: 601, 709 or 2020 (non-constant
 * luminance); full_range: 0 limited, 1 full (the yuvj* formats); 1 <= H, W <= 8192; anything else is refused with NUNIF_HIP_EINVAL.
 * planes: data[i] in device memory or pinned host memory (zero-copy), pitch[i] the BYTE pitch of plane i (>= its row; PyAV's
 *   plane.line_size); chroma planes hold ceil(W / 2) x ceil(H / 2) samples at 4:2:0.  Padding bytes are never written.
 * yuv_to_tensor: frame.reformat(**rgb24_options) (:1038-1039, options of guess_rgb24_options :621-640, matrix / range of
 *   guess_colorspace :610-618 / guess_color_range :596-607) followed by to_tensor (:218-223).  dst [3][H][W] fp32 in [0, 1];
 *   form 1 (debug, tests) does not clamp.  frame (optional, form 0 only): the HWC rgb24 (8-bit formats) / rgb48 (10-bit) frame,
 *   written in the same launch; device or pinned memory.
 * tensor_to_yuv: to_frame (:259-269) followed by reformatter(new_frame) (:1084, built by configure_colorspace :763-854).  src
 *   [3][H][W] fp32, clamped to [0, 1]; codes are rounded half up and clamped to [0, 2^bits - 1].
 * pixfmt_constants is host-only: the 3 x 3 coefficients (row major) and the 3 code offsets the kernels use for (matrix,
 *   full_range, bits 8 or 10, direction 0 = yuv -> rgb: rgb = M (yuv - off); 1 = rgb -> yuv: yuv = M rgb + off). */
typedef struct nunif_pixfmt_planes {
    void *data[3];
    int64_t pitch[3];
} nunif_pixfmt_planes;
int nunif_hip_yuv_to_tensor(const nunif_pixfmt_planes *src, int32_t format, int32_t H, int32_t W, int32_t matrix,
                            int32_t full_range, int32_t form, float *dst, void *frame, void *stream);
int nunif_hip_tensor_to_yuv(const float *src, int32_t H, int32_t W, int32_t format, int32_t matrix, int32_t full_range,
                            const nunif_pixfmt_planes *dst, void *stream);
int nunif_hip_pixfmt_constants(int32_t matrix, int32_t full_range, int32_t bits, int32_t direction, float *coefficients,
                               float *offsets);

/* HDR video that enters as YUV planes (nunif_amd/csrc/hdr_planes.hip): what hdr2sdr (nunif/utils/video.py:309-416) and the to_tensor
 * behind it make of a decoded BT.2020 PQ / HLG frame, from the decoder's planes in ONE launch.  The reference's rgb48 step
 * frame.to_ndarray(format="rgb48le") (:322-325, host libswscale; the reference asserts colorspace == BT2020, :318) is yuv_to_tensor's
 * arithmetic with the bt2020 matrix, rounded to the 16-bit codes its `frame` output holds; the map (:327-398) is hdr2sdr's; form 1
 * is to_tensor (:218-223) of the mapped frame.  The result is bit-equal to nunif_hip_yuv_to_tensor(format 2, matrix 2020, frame =
 * rgb48) followed by nunif_hip_hdr2sdr on that frame; the rgb48 frame itself never exists.
 * format: must be 2 (yuv420p10le); the matrix is bt2020 by definition; full_range 0 / 1; trc 16 (PQ) or 18 (HLG); colorspace 709 or
 * 601; 1 <= H, W <= 8192; params and form (0 u16 HWC, 1 chw fp32, 2 debug HWC fp32) as for nunif_hip_hdr2sdr; planes as for
 * nunif_hip_yuv_to_tensor (device or pinned host memory, byte pitches, padding never read past a row's samples).  Anything else —
 * formats 0 / 1, a null plane, a pitch shorter than its row — is refused with NUNIF_HIP_EINVAL and nothing is launched. */
int nunif_hip_yuv_hdr_to_tensor(const nunif_pixfmt_planes *src, int32_t format, int32_t H, int32_t W, int32_t full_range,
                                int32_t trc, int32_t colorspace, const nunif_hdr2sdr_params *params, int32_t form,
                                void *dst, void *stream);

/* cliqa's image-quality nets and patch selection (nunif_amd/csrc/cliqa.hip), eval mode, fp16 operands with fp32 accumulation
 * (the reference runs them under fp16 autocast, cliqa/utils.py:65,78,91), NHWC fp16 maps.
 * create replaces the constructors and eval-mode BatchNorm of cliqa/models/jpeg_quality.py JPEGQuality :8-41 (kind 0),
 *   grain_noise_level.py GrainNoiseLevel :8-34 (kind 1) and scale_factor.py ScaleFactor :10-36 (kind 2).  It takes the weights
 *   with BatchNorm folded on the host (nunif_amd/cliqa/models/_net.py pack_weights), all fp32:
 *   conv1.w [64][Cin][3][3] (Cin 6 for kind 0, 3 otherwise), conv1.b [64]; conv2.w [128][64][3][3], conv2.b [128];
 *   rb1a / rb1b / rb2a / rb2b .w [128][128][3][3], .b [128] (the two convs of each ResBlock, nunif/modules/res_block.py:55-63);
 *   head<i>.w [256][128][3][3], head<i>.b [256], head<i>.ow [256], head<i>.ob [1] (i = 0; kind 0 also i = 1, the subsampling head).
 * forward replaces JPEGQuality.forward :70-75 (with preprocess :57-68), GrainNoiseLevel.forward :52-58 and ScaleFactor.forward
 *   :53-63 (eval: clamped to [1, 2]): x [B,3,H,W] f32 device in [0, 1], any B, any H, W >= 8 -> out0 [B] f32 (quality, noise level
 *   or scale factor), out1 [B] f32 (kind 0: subsampling logit; NULL otherwise).  The batch is walked in groups of at most `group` images
 *   (0, or more than 2^23 input pixels hold: as many as those hold; H W <= 2^26).  workspace: caller-owned device bytes,
 *   nunif_hip_cliqa_workspace_bytes(handle, B, H, W, group) of them (0 for a shape forward refuses), so that calls on different
 *   streams never share scratch; forward is told how many it got (workspace_bytes) and refuses fewer than it needs
 *   (NUNIF_HIP_EINVAL).  The layout is csrc/cliqa_host.h.  No host synchronisation, no atomics.
 * debug_taps (tests only) is forward plus the maps behind the three pools (features[6], [8], [10]: tap1 [B,H/2,W/2,128], tap2
 *   [B,H/4,W/4,128], tap3 [B,H/8,W/8,128], NHWC fp16) and the head maps in front of the global pools (after [2] of each head:
 *   head_maps [B,H/8,W/8,heads*256] f32).
 * select_patches replaces extract_patches :36-57 with std_score :26-27 for an image already on the device: image [3,H,W] f32,
 *   cut into non-overlapping patch_size x patch_size patches, row-major, partial ones dropped (n = (H / P) (W / P) <= 4096);
 *   scores [n] f32 = mean over channels of the unbiased std; indices [K] int64 and patches [K,3,P,P] f32, K = min(num_patches, n),
 *   in descending score order (equal scores: the lower index first).  An image smaller than a patch is NUNIF_HIP_EINVAL
 *   (safe_pad :19-23 is a host step).  tv_score :30-33 is not carried: it reads an undefined name in the reference. */
typedef struct nunif_cliqa nunif_cliqa;
int nunif_hip_cliqa_create(const nunif_tensor_desc *tensors, int32_t n_tensors, int32_t kind, nunif_cliqa **handle);
void nunif_hip_cliqa_destroy(nunif_cliqa *handle);
int64_t nunif_hip_cliqa_workspace_bytes(nunif_cliqa *handle, int32_t B, int32_t H, int32_t W, int32_t group);
int nunif_hip_cliqa_forward(nunif_cliqa *handle, const float *x, int32_t B, int32_t H, int32_t W, int32_t group, void *workspace,
                            int64_t workspace_bytes, float *out0, float *out1, void *stream);
int nunif_hip_cliqa_debug_taps(nunif_cliqa *handle, const float *x, int32_t B, int32_t H, int32_t W, int32_t group,
                               void *workspace, int64_t workspace_bytes, float *out0, float *out1, void *tap1, void *tap2,
                               void *tap3, float *head_maps, void *stream);
int nunif_hip_cliqa_select_patches(const float *image, int32_t H, int32_t W, int32_t patch_size, int32_t num_patches,
                                   float *scores, int64_t *indices, float *patches, void *stream);

/* iw3 --export / --export-disparity (iw3/utils.py:1366-1505 bind_export_single_frame_callback / bind_export_vda_frame_callback:
 * per frame save_image :224-244 of the 8-bit RGB source and iw3/base_depth_model.py:197-210 save_normalized_depth of the 16-bit
 * depth, both libpng on a host thread pool): a lossless PNG encoder on the device, so that a frame crosses to the host as its
 * finished PNG bytes.  No weights: plain functions and a caller-owned workspace.  DESIGN.md ("PNG frame encoder") states the
 * stream byte for byte.  header, max_bytes and workspace_bytes are host-only (nunif_amd/csrc/png_host.h), no GPU needed.
 * form: 0 = RGB 8 from [B,3,H,W] f32 (clamp, x 255, round half even, as to_uint8); 1 = RGB 8 from [B,H,W,3] u8; 2 = grey 16 from
 *   [B,1,H,W] f32 (clamp, fp32 0xffff * d, truncation, big-endian, as save_normalized_depth).
 * header: the PNG signature, IHDR and one tEXt chunk per (key, value) pair (zero-terminated Latin-1; a key holds 1..79 bytes) into
 *   out (host); returns the length or a negative status.
 * max_bytes: an upper bound of the body (the IDAT chunks and IEND) of one frame for any input: per stripe of n filtered bytes
 *   3 + 14 + 19 x 3 + 316 x 7 header bits, 15 n bits of tokens, 15 for the end of block and 3 for the stored block, filled to a
 *   byte, 4 bytes LEN / NLEN and 12 of chunk; 2 bytes of zlib header, 4 of Adler-32, 12 of IEND.  -1 for a refused shape.
 * workspace_bytes: the size of `workspace` for encode and debug_codes.  -1 for a refused shape.
 * encode: B frames -> B bodies, body b at out + b * capacity (device), its length in out_len[b] (device i32).  One IDAT chunk per
 *   stripe of stripe_rows rows (1..H; stripes are the unit of parallelism), each a dynamic-Huffman deflate block and an empty
 *   stored block; adaptive row filter (smallest sum of absolute values, lowest type on a tie); matches at the pixel distance.
 *   Five launches on `stream`, no host synchronisation, no atomics on global memory: the bytes depend on the input alone.  If
 *   capacity is smaller than the body, out_len[b] = -1 and nothing of slot b is written; max_bytes is always enough.  workspace:
 *   workspace_bytes() bytes of device memory, 256-byte aligned; calls that overlap need their own.  1 <= H, W <= 8192, B <= 16;
 *   anything else is refused.
 * Forms 4..6 (the waifu2x image route: waifu2x/ui_utils.py:42-100 process_image / process_images, nunif/utils/pil_io.py:240-323
 *   to_image / save_image) take planar fp32 colour [B,colour_channels,H,W] and, apart from it, a planar fp32 alpha [B,1,H,W], as
 *   Waifu2x.convert returns them; every plane is quantised as form 0 is (quantize256).  3 names no form and stays refused.
 *   4 = RGBA 8 (colour type 6; colour_channels 3); 5 = grey 8 (colour type 0; alpha NULL); 6 = grey + alpha 8 (colour type 4).
 *   The grey forms take colour_channels 1 (the plane itself) or 3: the three bytes of a pixel go through PIL's
 *   Image.convert("L"), (19595 R + 38470 G + 7471 B + 0x8000) >> 16, as save_image's meta["grayscale"] branch does.
 *   header, max_bytes and workspace_bytes take these forms; encode and debug_filtered refuse them: encode_planes and
 *   debug_filtered_planes are the same calls with the two source pointers, and take forms 4..6 only.  debug_codes takes them with
 *   src = one tensor [B,C+1,H,W] (C = 3 for form 4, 1 for form 6) whose last plane is the alpha, or [B,1,H,W] for form 5.
 * debug_filtered (tests) runs the first launch alone: the filtered bytes [B][H][1 + W * bpp] u8 (device), the filter type first.
 * debug_codes (tests) runs the first three launches: per stripe the histogram and the code lengths, [B][stripes][336] i32 each
 *   (device): 286 literal / length symbols, 30 distance symbols, 19 code-length symbols, one word of padding. */
int64_t nunif_hip_png_header(int32_t H, int32_t W, int32_t form, const char *const *text_keys, const char *const *text_values,
                             int32_t n_text, uint8_t *out, int64_t capacity);
int64_t nunif_hip_png_max_bytes(int32_t H, int32_t W, int32_t form, int32_t stripe_rows);
int64_t nunif_hip_png_workspace_bytes(int32_t B, int32_t H, int32_t W, int32_t form, int32_t stripe_rows);
int nunif_hip_png_encode(const void *src, int32_t form, int32_t B, int32_t H, int32_t W, int32_t stripe_rows, uint8_t *out,
                         int64_t capacity, int32_t *out_len, void *workspace, void *stream);
int nunif_hip_png_debug_filtered(const void *src, int32_t form, int32_t B, int32_t H, int32_t W, uint8_t *filtered, void *stream);
int nunif_hip_png_debug_codes(const void *src, int32_t form, int32_t B, int32_t H, int32_t W, int32_t stripe_rows, int32_t *hist,
                              int32_t *lengths, void *workspace, void *stream);
int nunif_hip_png_encode_planes(const float *colour, const float *alpha, int32_t colour_channels, int32_t form, int32_t B, int32_t H,
                                int32_t W, int32_t stripe_rows, uint8_t *out, int64_t capacity, int32_t *out_len, void *workspace,
                                void *stream);
int nunif_hip_png_debug_filtered_planes(const float *colour, const float *alpha, int32_t colour_channels, int32_t form, int32_t B,
                                        int32_t H, int32_t W, uint8_t *filtered, void *stream);

/* iw3 --depth-model Any_V3_Mono / Any_V3_Mono_01: what iw3/depth_anything_v3_model.py wraps around the Depth-Anything-3 backbone,
 * and iw3.da3mono_disparity (iw3/models/da3mono_disparity.py).  The backbone itself is an external hub net and is not part of the
 * engine.  All maps are f32 device [B][H*W] (B <= 4096, 1 <= H, W <= 8192, H * W >= 3; anything else, or a NULL or too small
 * workspace, answers NUNIF_HIP_EINVAL before anything is launched).  No entry synchronises with the host.  NaN inputs are out of
 * contract (the order-preserving keys sort them past the infinities, torch.sort puts every NaN last; a NaN sky value counts as not
 * sky, as in torch); -0.0 sorts before +0.0 where torch.sort keeps them in input order (equal as values).  Workspaces are
 * caller-owned device bytes, 16-byte aligned, of at least the size the matching *_workspace_bytes answers (-1 for a bad shape), so
 * calls on different streams never share scratch; every call clears what it uses.  Results are integer counts and per-pixel
 * formulas only: bit-equal across calls and streams.
 *
 * da3_disparity replaces _forward :33-56 for the whole batch: w = (clamp(sky, t, 1) - t) / (1 - t) (:35), sky mask = sky > t
 *   (:34), the non-sky count m on the device (:40; the reference reads it on the host per image).
 *   raw_output == 0: out = 0 where m < 10 (:41-43), else (1 / (depth + shift)) * (1 - w) (:47-49; the reference's shift is 0.2),
 *     one rounding per operation in that order.
 *   raw_output != 0: q = the 0.99 quantile of depth[~sky_mask] (:51) = a + (b - a) * frac(p) with p = 0.99 * (m - 1) and a, b
 *     the order statistics floor(p), ceil(p), found by an exact radix selection over the masked pixels (no sort, no compaction);
 *     out = min(depth * (1 - w) + w * q, q) (:52).  p and the interpolation are evaluated in double and rounded once (torch
 *     forms p in fp32, which drifts by whole ranks once m passes 2^24 / 100).  DIVERGENCE: with m == 0 the reference raises
 *     (torch.quantile of an empty tensor); the engine cannot stop the host and writes zeros.
 * da3_disparity_debug_stats (tests only): a, b, q ([B][3] f32) and m ([B] i32) of the last raw call that ran on `workspace`.
 *
 * da3mono_features replaces DA3MonoDisparity.extract_features :53-73: out [B][64] = minimum, the order statistics ranks[0..61],
 *   maximum of each image, bit-equal to indexing torch.sort's output.  ranks: 62 int64 on the DEVICE, the values of
 *   torch.linspace(1, n - 2, 62).long() (:65) computed once per n on the host by that expression; the kernels do not re-derive
 *   them (out-of-range values are clamped to [0, n - 1]).  One selection serves all 64 ranks of an image: four 8-bit levels,
 *   each one histogram pass over the map shared by every rank, whatever the values are (constant and two-valued maps included).
 *
 * da3mono: create() takes the MLP of forward :29-50 packed by nunif_amd/iw3/models/da3mono_disparity.py pack_weights, all f32:
 *   mlp.0.wt [64][128] and mlp.2.wt [128][128] (the Linear weights transposed), mlp.4.weight [2][128], mlp.{0,2,4}.bias.
 *   forward: the features, the 64 -> 128 -> 128 -> 2 MLP (SiLU, SiLU, ReLU; fp32 operands and activations, sums in double) ->
 *   (shift, sky_shift) per image, then out = 1 / ((depth == max ? depth + sky_shift : depth) + shift) with max = feature 63
 *   (:37-48; the 3-D form of the reference is B = 1). */
int64_t nunif_hip_da3_disparity_workspace_bytes(int32_t B, int32_t H, int32_t W);
int nunif_hip_da3_disparity(const float *depth, const float *sky, int32_t B, int32_t H, int32_t W, double sky_thresh, double shift,
                            int32_t raw_output, float *out, void *workspace, int64_t workspace_bytes, void *stream);
int nunif_hip_da3_disparity_debug_stats(const void *workspace, int32_t B, float *stats, int32_t *counts, void *stream);
int64_t nunif_hip_da3mono_features_workspace_bytes(int32_t B, int32_t H, int32_t W);
int nunif_hip_da3mono_features(const float *depth, int32_t B, int32_t H, int32_t W, const int64_t *ranks, float *out,
                               void *workspace, int64_t workspace_bytes, void *stream);
typedef struct nunif_da3mono nunif_da3mono;
int nunif_hip_da3mono_create(const nunif_tensor_desc *tensors, int32_t n_tensors, nunif_da3mono **handle);
void nunif_hip_da3mono_destroy(nunif_da3mono *handle);
int64_t nunif_hip_da3mono_workspace_bytes(int32_t B, int32_t H, int32_t W);
int nunif_hip_da3mono_forward(nunif_da3mono *handle, const float *depth, int32_t B, int32_t H, int32_t W, const int64_t *ranks,
                              float *out, void *workspace, int64_t workspace_bytes, void *stream);

/* stlizer pass 2: the batch form of find_transform (nunif/utils/superpoint.py:233-327, with cosine_annealing :226-230), the
 * reference's torch autograd loop of `iteration` Adam steps over translation [2], scale and rotation of every point pair set, as
 * iteration + 1 launches of one kernel on `stream`, one workgroup per pair, without a host synchronisation.  Launch s finishes the
 * Adam step s - 1 of its pair (betas 0.5 / 0.9, eps 1e-8, torch.optim.Adam's bias corrections :267; both learning rates follow
 * CosineAnnealingWarmRestarts(T_0 = iteration, eta_min = lr_scale_rotation * 1e-3) at T_cur = s - 1, :268-269) and then runs the
 * forward and the closed-form gradient of step s (:279-310); launch 0 centres and normalises the points first (:271-275: norm_scale
 * is the largest |nan_to_num(xy1 - center)| over all N x 2 entries of the pair, padded ones included); launch `iteration` writes
 * the outputs (:315-319).  The loss is a mean over the whole batch (:305, :309): every pair adds its selected-element count to the
 * step's slot of the workspace with one integer atomicAdd, and the next launch divides the pair's gradient sums by that total.
 * These are the only atomics, so the result is bit-equal across calls and streams and does not depend on the order of the pairs.
 * With sigma or sigma_min given, steps s > 0 keep the masked elements with (loss - mean) / std < sigma (:294-305), mean and
 * population standard deviation over the pair's masked losses of both coordinates; sigma follows cosine_annealing(sigma_min,
 * sigma_max, s, iteration) when sigma_min is given.  A zero std, or a pair without a masked element, selects nothing.  Parameters
 * are fp32 as in the reference; the mean, the deviation and the gradient sums are double sums in a fixed order.
 *   xy1, xy2 [B][N][2] f32 (8-byte aligned), mask [B][N][2] bytes (non-zero = valid; 2-byte aligned) or NULL for all valid,
 *   center [B][2] f32; shift_out [B][2] = translation * norm_scale, scale_out [B], angle_out [B] = rad2deg(atan2(sin r, cos r));
 *   trace, if not NULL: (tx, ty, scale, rotation) of every pair after every Adam step, [iteration][B][4] f32 (tests).
 *   flags: NUNIF_FIND_TRANSFORM_* below; sigma / sigma_min are read only when their flag is set.
 *   1 <= B <= 4096, 1 <= N <= 8192, 1 <= iteration <= 1024; anything else is refused (workspace_bytes answers -1).
 *   NaN or infinite masked points are out of contract.  In the reference the NaN loss of step 0 turns that pair's parameters NaN
 *   for good (:309-311); here sign(NaN) counts as 0 at step 0, and from step 1 on a NaN loss makes the pair's mean and deviation
 *   NaN, so the pair selects nothing and its parameters stay where step 0 left them.  Other pairs see only the changed count.
 * workspace: caller-owned device bytes, 256-byte aligned, at least workspace_bytes(B, N, iteration) =
 *   align256(4 * iteration) [the count slots, cleared by every call] + align256(96 * B) [per pair: 4 parameters, Adam m and v,
 *   norm_scale, 4 double gradient sums] + 2 * align256(8 * B * N) [the normalised xy1, xy2]; a smaller one is refused.  Calls that
 *   overlap on different streams need their own. */
enum {
    NUNIF_FIND_TRANSFORM_DISABLE_SHIFT = 1,
    NUNIF_FIND_TRANSFORM_DISABLE_SCALE = 2,
    NUNIF_FIND_TRANSFORM_DISABLE_ROTATE = 4,
    NUNIF_FIND_TRANSFORM_SIGMA = 8,
    NUNIF_FIND_TRANSFORM_SIGMA_MIN = 16
};
int64_t nunif_hip_find_transform_workspace_bytes(int32_t B, int32_t N, int32_t iteration);
int nunif_hip_find_transform(const float *xy1, const float *xy2, const uint8_t *mask_or_null, const float *center, int32_t B,
                             int32_t N, int32_t iteration, double lr_translation, double lr_scale_rotation, double sigma,
                             double sigma_min, double sigma_max, int32_t flags, float *shift_out, float *scale_out,
                             float *angle_out, void *workspace, int64_t workspace_bytes, float *trace_or_null, void *stream);

/* stlizer pass 3 (stlizer/multipass_pipeline.py, reference): everything between pass 2's per-frame transforms and pass 4's
 * per-frame fixes, on `stream`, without a host synchronisation.
 * scene_weight: calc_scene_weight (:86-105) in fp32: (score - 0.5) / 0.25 clamped to [0, 1], squared below 0.65, first and last
 *   frame 0; bit-equal to torch's.
 * pass3_prepare: the angle clamped to +-90 (:359), the three per-frame values times the fp32 weight widened to float64 and their
 *   inclusive prefix sums (:338-344) into paths [3, N]; two launches, the tile sums combined in index order.
 * pass3_conv: conv1d_smoothing (:272-289) given its taps (gen_smoothing_kernel :64-75, built on the host): replicate pad (:78-83),
 *   K-tap float64 correlation, minus the input, fix [3, N]; K odd, 1 <= K <= 4097.
 * pass3_grad_opt: grad_opt (:292-334): the paths padded by three replicated elements and (x, y only) scaled by resolution_weight =
 *   resolution / 320 (:297-302), `iteration` calls of torch.optim.LBFGS(history_size=10, max_iter=4, lr=1, tolerance_grad=1e-7,
 *   tolerance_change=1e-9, line_search_fn=None).step on the loss of :311-322 with its gradient in closed form, and the fixes
 *   (x - target) / resolution_weight (:330-332) into out [3, N].  LBFGS.step is restated decision for decision: the first step
 *   min(1, 1 / |g|_1), the memory update only when y.s > 1e-10, H_diag = y.s / y.y, the two-loop recursion in the reference's
 *   order over explicit s / y history vectors, prev_flat_grad and prev_loss carried across step calls, no re-evaluation after the
 *   4th iteration, and the five exits.  x alone is held in two doubles (the closure's differences cancel most of it); the trace
 *   is its high word.  1 + iteration * 4 * 22 + 1 launches whatever the data; nothing is read back; no float
 *   atomics: bit-equal across calls, streams and workspaces.  1 <= N <= 1048576, 1 <= iteration <= 1024, else EINVAL.
 *   trace_or_null: [iteration * 4, 3, N + 3], x after every LBFGS iteration slot (tests).
 *   log_or_null: [iteration * 4, 32] doubles, the decision record of every slot as nunif_amd/csrc/stlizer_pass3_host.h lays it
 *   out: which exit if any, the memory update taken or not, loss, g.d, max|g| and the optimizer's scalars (tests).
 * workspace: caller-owned device bytes, 256-byte aligned, at least pass3_workspace_bytes(N, iteration) (prepare: (N, 1)); the
 *   layout (records, history ring, per-launch partials) is in stlizer_pass3_host.h.  Calls that overlap on different streams need
 *   their own. */
int nunif_hip_stlizer_scene_weight(const float *scores, int32_t N, float *weight, void *stream);
int64_t nunif_hip_stlizer_pass3_workspace_bytes(int32_t N, int32_t iteration);
int nunif_hip_stlizer_pass3_prepare(const double *shift_x, const double *shift_y, const double *angle, const float *weight,
                                    int32_t N, double *paths, void *workspace, int64_t workspace_bytes, void *stream);
int nunif_hip_stlizer_pass3_conv(const double *paths, int32_t N, const double *taps, int32_t K, double *fix, void *stream);
int nunif_hip_stlizer_pass3_grad_opt(const double *paths, const float *weight, int32_t N, double resolution_weight,
                                     int32_t iteration, double penalty_weight, double *out, void *workspace,
                                     int64_t workspace_bytes, double *trace_or_null, double *log_or_null, void *stream);

/* Test hooks (tests/ only): snapshot every stage's NHWC fp16 output during the next forward calls, then read
 * them back one by one (returns 1 past the last tap).  Names match oracle.swin_unet.unet_forward(taps=...). */
int nunif_hip_swin_unet_debug_taps(nunif_swin_unet *handle, int32_t enable);
int nunif_hip_swin_unet_get_tap(nunif_swin_unet *handle, int32_t index, char *name, int32_t name_cap,
                                void *host_dst, int64_t cap_bytes, int64_t *nbytes);
/* The same for the cunet engine (CUNet / UpCUNet / vgg_7 / upconv_7): the map each launch wrote (NHWC fp16; "z1" planar fp32;
 * "*.scale" the SE vectors [B][C] fp32), copied device-side right after the launch.  Taps never change which kernels run: the
 * output with taps on equals the output with taps off.  Names match oracle.cunet.model_forward / conv_stack_forward(taps=...);
 * a map that no launch writes in the current configuration (the 32-channel map inside the fused stem) has no tap.  Every forward
 * with taps on starts from an empty store: the taps read back are those of the last forward (of a render: its last minibatch). */
int nunif_hip_cunet_debug_taps(nunif_cunet *handle, int32_t enable);
int nunif_hip_cunet_get_tap(nunif_cunet *handle, int32_t index, char *name, int32_t name_cap,
                            void *host_dst, int64_t cap_bytes, int64_t *nbytes);

/* Timing hooks for bench.py: per-kernel-class HIP-event accumulation on the launch stream. */
int nunif_hip_profile_enable(int32_t on);
/* Writes up to `cap` (name,total_ms,launches) records; returns the count. Synchronises the events. */
typedef struct { char name[48]; double total_ms; int64_t launches; double flops; double bytes; } nunif_prof_record;
int nunif_hip_profile_read(nunif_prof_record *out, int32_t cap, int32_t reset);

#ifdef __cplusplus
}
#endif
#endif /* NUNIF_HIP_H */
