"""``sbs.row_flow_v2`` restated from its architecture (helper module, not a conftest).

The net: feature = ReLU(1x3 conv 3->16); non_overlap = 1x1 conv 16->1; overlap_residual = three ReLU(1x9 conv) 16->16->32->32 and a
3x3 conv 32->1; delta = non_overlap + overlap_residual.  Every conv sits behind a replicate pad of its own radius, and the
delta-only forward replicate-pads the input by 28 first and crops 28 afterwards.

Two forms of the same function:

* ``delta_padded``  — as the model structures it: pad 28, the padded layers, crop 28.
* ``delta_clamped`` — the UNPADDED (valid) stack on the input gathered at clamped coordinates (14 columns, 1 row of halo).  Equal
  because the halo the crop leaves (28) is wider than the receptive radius (14 x 1): no kept pixel sees an inner pad.

``delta_tiled`` evaluates the clamped form tile by tile the way csrc/rowflow_v2.hip does (R x T output pixels, halo (1, 14), the
mirror of ``flip`` folded into the load) and takes kernel-shaped ``mutation``s for the localisation tests.  ``fp16=True`` emulates
the reference's fp16 autocast: weights, biases and each layer's input rounded to fp16, fp32 accumulation, each layer's output
rounded to fp16 (the sum of the two branches is an fp16 add as well).
"""
import torch
import torch.nn.functional as F

from oracle import row_flow_v3 as ORF

R, T = 5, 62                       # the kernel's band x tile (csrc/rowflow_v2.hip)
HALO_Y, HALO_X = 1, 14
CELLS = (((R, T), (0, 0)),)        # errloc cells: aligned and half-shifted band x tile
TAP_NAMES = ("feature", "relu1", "relu2", "relu3", "non_overlap", "residual")
MUTATIONS = ("halo13", "edge_replicate", "no_vhalo", "flip_taps", "no_relu2", "no_non_overlap")


WEIGHT_SEED = 301


def fixture_inputs():
    """(depth [2,1,58,104], image [2,3,58,104]) of tests/golden/row_flow_v2.npz, regenerated from their seeds."""
    from conftest import synth_image
    from oracle.forward_warp import synth_depth
    return synth_depth(3, 2, 58, 104, "smooth_edges"), torch.stack([synth_image(71, 3, 58, 104), synth_image(72, 3, 58, 104)])


def _r16(t):
    return t.half().to(t.dtype)


def _id(t):
    return t


def clamp_gather(x, y0, y1, x0, x1):
    """x[..., clamp(y0..y1-1), clamp(x0..x1-1)]: a replicate pad of any width, also wider than the map."""
    h, w = x.shape[-2:]
    iy = torch.arange(y0, y1).clamp(0, h - 1)
    ix = torch.arange(x0, x1).clamp(0, w - 1)
    return x[..., iy, :][..., ix]


def _rpad(x, l, r, t, b):
    h, w = x.shape[-2:]
    return clamp_gather(x, -t, h + b, -l, w + r)


def _params(sd, dtype, fp16):
    p = {k: v.to(dtype) for k, v in sd.items() if v.is_floating_point()}
    return {k: _r16(v) for k, v in p.items()} if fp16 else p


def _centre(t, h, w):
    dy, dx = (t.shape[-2] - h) // 2, (t.shape[-1] - w) // 2
    return t[..., dy:dy + h, dx:dx + w]


def _layers(p, x, pad, rnd, relu2=True, non_overlap=True, taps=None, fix=None):
    """The seven convs.  ``pad(t, l, r, top, bottom)`` is the pad in front of each conv (identity for the valid stack);
    ``fix(t, level)`` post-processes an activation whose halo is ``level`` columns narrower than the input's."""
    fix = fix or (lambda t, level: t)
    x = rnd(x)
    f = fix(rnd(F.relu(F.conv2d(pad(x, 1, 1, 0, 0), p["feature.0.weight"], p["feature.0.bias"]))), 1)
    no = rnd(F.conv2d(f, p["non_overlap.weight"], p["non_overlap.bias"]))
    a1 = fix(rnd(F.relu(F.conv2d(pad(f, 4, 4, 0, 0), p["overlap_residual.0.weight"], p["overlap_residual.0.bias"]))), 5)
    a2 = F.conv2d(pad(a1, 4, 4, 0, 0), p["overlap_residual.2.weight"], p["overlap_residual.2.bias"])
    a2 = fix(rnd(F.relu(a2) if relu2 else a2), 9)
    a3 = fix(rnd(F.relu(F.conv2d(pad(a2, 4, 4, 0, 0), p["overlap_residual.4.weight"], p["overlap_residual.4.bias"]))), 13)
    res = rnd(F.conv2d(pad(a3, 1, 1, 1, 1), p["overlap_residual.6.weight"], p["overlap_residual.6.bias"]))
    if taps is not None:
        taps.update(feature=f, relu1=a1, relu2=a2, relu3=a3, non_overlap=no, residual=res)
    return no, res, (rnd(_centre(no, *res.shape[-2:]) + res) if non_overlap else res)


def delta_padded(sd, x, dtype=torch.float64):
    """The model's own structure: replicate pad 28, padded layers, crop 28.  x [B,3,h,w] -> [B,1,h,w]."""
    h, w = x.shape[-2:]
    p = _params(sd, dtype, False)
    return _centre(_layers(p, _rpad(x.to(dtype), 28, 28, 28, 28), _rpad, _id)[2], h, w)


def delta_clamped(sd, x, dtype=torch.float64, fp16=False, taps=None):
    """The valid stack on the clamped input halo.  With ``taps`` (a dict) the six intermediate maps are left in it, [B,C,h,w]."""
    h, w = x.shape[-2:]
    p = _params(sd, dtype, fp16)
    xe = clamp_gather(x.to(dtype), -HALO_Y, h + HALO_Y, -HALO_X, w + HALO_X)
    out = _layers(p, xe, lambda t, *a: t, _r16 if fp16 else _id, taps=taps)[2]
    if taps is not None:
        for k in taps:
            taps[k] = _centre(taps[k], h, w)
    return out


def delta_fp32(sd, x):
    return delta_padded(sd, x, torch.float32)


def oracle64(sd, x, flip=False, taps=None):
    """float64, in the frame the kernel writes: with ``flip`` the net sees the mirrored planes and delta stays mirrored."""
    return delta_clamped(sd, torch.flip(x, (3,)) if flip else x, torch.float64, taps=taps)


def emulated(sd, x, flip=False, taps=None):
    return delta_clamped(sd, torch.flip(x, (3,)) if flip else x, torch.float32, fp16=True, taps=taps)


def delta_tiled(sd, x, flip=False, mutation=None, fp16=True, dtype=torch.float32, r=R, t=T):
    """The kernel's schedule on the CPU: per r x t tile, gather the clamped (and mirrored) halo, run the valid stack, store."""
    assert mutation is None or mutation in MUTATIONS
    B, _, h, w = x.shape
    p = _params(sd, dtype, fp16)
    rnd = _r16 if fp16 else _id
    x = x.to(dtype)
    src = x if (not flip or mutation == "flip_taps") else torch.flip(x, (3,))
    hx = 13 if mutation == "halo13" else HALO_X
    hy = 0 if mutation == "no_vhalo" else HALO_Y
    out = torch.empty((B, 1, h, w), dtype=dtype)
    for y0 in range(0, h, r):
        for x0 in range(0, w, t):
            th, tw = min(r, h - y0), min(t, w - x0)
            xe = clamp_gather(src, y0 - hy, y0 + r + hy, x0 - hx, x0 + t + hx)
            xe = F.pad(xe, (HALO_X - hx, HALO_X - hx, HALO_Y - hy, HALO_Y - hy))      # what a too narrow halo leaves: zeros
            fix = None
            if mutation == "edge_replicate":
                def fix(a, level, y0=y0, x0=x0):
                    # activations outside the image copied from the edge activation instead of computed from the clamped input
                    ys = (torch.arange(a.shape[-2]) + y0 - HALO_Y).clamp(0, h - 1) - (y0 - HALO_Y)
                    xs = (torch.arange(a.shape[-1]) + x0 - HALO_X + level).clamp(0, w - 1) - (x0 - HALO_X + level)
                    return a[..., ys.clamp(0, a.shape[-2] - 1), :][..., xs.clamp(0, a.shape[-1] - 1)]
            d = _layers(p, xe, lambda a, *pads: a, rnd, relu2=mutation != "no_relu2",
                        non_overlap=mutation != "no_non_overlap", fix=fix)[2]
            out[:, :, y0:y0 + th, x0:x0 + tw] = d[:, :, :th, :tw]
    # a kernel that mirrors the store but convolves the un-mirrored planes with un-mirrored taps computes flip(net(x))
    return torch.flip(out, (3,)) if (flip and mutation == "flip_taps") else out


# ---- NN backward-warp glue (oracle/row_flow_v3.py's grid and warp, this net's flow) -------------------------------------------
def apply_divergence_nn_delta(sd, c, depth, divergence, convergence, shift, steps=1, delta_fn=delta_fp32):
    if shift > 0:
        c, depth = torch.flip(c, (3,)), torch.flip(depth, (3,))
    B, _, H, W = depth.shape
    grid, scale = ORF.make_grid(B, W, H), torch.tensor(1.0 / (W // 2 - 1))
    depth_warp, deltas = depth, []
    for j in range(steps):
        delta = delta_fn(sd, ORF.make_input(depth_warp, divergence / steps, convergence, max(H, W)))
        delta = torch.cat([delta, torch.zeros_like(delta)], dim=1)
        deltas.append(delta)
        if j + 1 < steps:
            depth_warp = ORF.backward_warp(depth_warp, grid, delta, scale)
    z = c
    for delta in deltas:
        z = ORF.backward_warp(z, grid, delta, scale)
    return torch.flip(z, (3,)) if shift > 0 else z


def apply_divergence_nn_LR(sd, c, depth, divergence, convergence, synthetic_view="both", steps=1):
    if synthetic_view == "both":
        return (apply_divergence_nn_delta(sd, c, depth, divergence, convergence, -1, steps),
                apply_divergence_nn_delta(sd, c, depth, divergence, convergence, 1, steps))
    if synthetic_view == "right":
        return c, apply_divergence_nn_delta(sd, c, depth, divergence * 2, convergence, 1, steps)
    return apply_divergence_nn_delta(sd, c, depth, divergence * 2, convergence, -1, steps), c
