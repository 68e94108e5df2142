"""A restatement of the batch form of the reference's ``find_transform`` (nunif/utils/superpoint.py:233-327) with closed-form
gradients: no autograd, nothing imported from the reference.  It takes the batch as a whole, because the reference's loss is a mean
over the whole batch (:305, :309): every pair's gradient is divided by the batch's selected-element count of the step.

``run(..., dtype=torch.float64)`` defines truth for the tests; ``dtype=torch.float32`` is an independent fp32 implementation (torch
sums, torch's cos / sin) whose distance from truth is compared with the reference's own.  ``mutate`` names one deliberate mistake
(MUTATIONS) for the tests that show the bound would catch it.

Also the synthetic cases of tests/golden/find_transform.npz (CASES, case_input) and the error measures the CPU and GPU tests share.
"""
import math

import numpy as np
import torch

FRAME_W, FRAME_H = 568, 320
CENTER = (FRAME_W // 2, FRAME_H // 2)
BETA1, BETA2, EPS = 0.5, 0.9, 1e-8

MUTATIONS = ("pair_count", "two_sided", "sample_std", "reject_at_step0", "schedule_plus_one", "no_bias_correction",
             "norm_scale_unpadded")

# name -> (seed, point counts per pair, padded N, pass the mask, keyword arguments)
PASS2 = dict(iteration=50, sigma=2.0, disable_scale=True)
_C16 = [200 + (19 * i) % 58 for i in range(15)] + [257]            # 200 .. 257, 257 last
# pass 2's pairs are ragged.  The small ones matter: losses are non-negative and a pair with an outlier has a deviation above half
# its mean, so only a pair without one (3 .. 33 points here) can have an element below mean - sigma * std, where a two-sided
# outlier test would differ from the reference's one-sided one
_H16 = [3, 4, 5, 6, 8, 11, 16, 33] + [200 + (19 * i) % 58 for i in range(7)] + [257]
CASES = {
    "a": (11, [1], 1, True, dict(iteration=20, sigma=2.0)),
    "b": (12, [3], 3, True, dict(iteration=20, sigma=2.0)),
    "c": (100, [5, 64, 65], 65, True, dict(iteration=20, sigma=2.0)),
    "d": (104, _C16, 257, True, dict(iteration=20, sigma=2.0)),
    "e": (742, [1025] * 32, 1025, False, dict(iteration=20, sigma=2.0)),
    "f": (100, _C16, 257, True, dict(iteration=20, sigma=None)),
    "g": (100, _C16, 257, True, dict(iteration=20, sigma_min=1.0)),
    "h": (19, _H16, 257, True, dict(PASS2)),
    "i_shift": (100, _C16, 257, True, dict(iteration=50, sigma=2.0, disable_shift=True)),
    "i_rotate": (106, _C16, 257, True, dict(iteration=50, sigma=2.0, disable_rotate=True)),
    "j": (21, [40, 0, 33, 64], 64, True, dict(iteration=20, sigma=2.0)),
}
RMS_CASES = ("c", "d", "e", "f", "g", "h", "i_shift", "i_rotate")     # enough pairs for an RMS; a, b, j: the first trace steps only
EARLY_STEPS = 3


def synthetic_pairs(seed, counts, N):
    """-> xy1 [B, N, 2], xy2, mask (bool), center [B, 2].  Points uniform in the frame, moved by a shift of up to 12 px and an angle
    of up to 2 degrees about the centre, Gaussian noise of 0.3 px, 10 % replaced by uniform outliers; zero-padded to N as
    pack_points does."""
    rng = np.random.default_rng(seed)
    B = len(counts)
    xy1 = np.zeros((B, N, 2), np.float32)
    xy2 = np.zeros((B, N, 2), np.float32)
    mask = np.zeros((B, N, 2), bool)
    c = np.array(CENTER, np.float64)
    for b, n in enumerate(counts):
        p = rng.uniform(0.0, 1.0, (n, 2)) * np.array([FRAME_W, FRAME_H])
        shift = rng.uniform(-12.0, 12.0, 2)
        ang = math.radians(rng.uniform(-2.0, 2.0))
        rot = np.array([[math.cos(ang), -math.sin(ang)], [math.sin(ang), math.cos(ang)]])
        q = (p - c) @ rot.T + c + shift + rng.normal(0.0, 0.3, (n, 2))
        out = rng.uniform(0.0, 1.0, n) < 0.1
        q[out] = rng.uniform(0.0, 1.0, (int(out.sum()), 2)) * np.array([FRAME_W, FRAME_H])
        xy1[b, :n], xy2[b, :n], mask[b, :n] = p, q, True
    center = np.tile(np.array(CENTER, np.float32), (B, 1))
    return torch.from_numpy(xy1), torch.from_numpy(xy2), torch.from_numpy(mask), torch.from_numpy(center)


def case_input(name):
    """-> xy1, xy2, mask or None, center, kwargs of a case of CASES."""
    seed, counts, N, with_mask, kwargs = CASES[name]
    assert with_mask or all(n == N for n in counts)
    xy1, xy2, mask, center = synthetic_pairs(seed, counts, N)
    return xy1, xy2, mask if with_mask else None, center, dict(kwargs)


def cosine_annealing(min_v, max_v, t, max_t):
    return min_v + 0.5 * (max_v - min_v) * (1.0 + math.cos((t / max_t) * math.pi)) if max_t > t else min_v


def learning_rate(base, eta_min, t, T):
    """CosineAnnealingWarmRestarts(T_0 = T, eta_min) at T_cur = t < T."""
    return eta_min + (base - eta_min) * (1.0 + math.cos(math.pi * t / T)) / 2.0


def normalise(xy1, xy2, center, mask, dtype, mutate=None):
    """:271-275 -> normalised xy1, xy2 and norm_scale [B, 1, 1]; the maximum runs over the padded entries too."""
    c = center.to(dtype).reshape(-1, 1, 2)
    a, b = xy1.to(dtype) - c, xy2.to(dtype) - c
    mag = torch.nan_to_num(a).abs()
    if mutate == "norm_scale_unpadded" and mask is not None:
        mag = mag * mask.to(dtype)
    norm_scale = mag.amax(dim=(1, 2)).view(-1, 1, 1)
    return a / norm_scale, b / norm_scale, norm_scale


def transform(xy1n, translation, scale, rotation):
    """:282-292 with translation [B, 1, 2], scale and rotation [B, 1, 1] -> (rotated points before the scale, transformed points)."""
    rc, rs = rotation.cos(), rotation.sin()
    rot = torch.cat([xy1n[:, :, :1] * rc - xy1n[:, :, 1:] * rs, xy1n[:, :, :1] * rs + xy1n[:, :, 1:] * rc], dim=2)
    return rot, rot * scale + translation


def select(loss, mask, sigma, mutate=None, sum_dtype=None):
    """:299-305 -> the elements of the loss that count: masked and, with ``sigma``, not an outlier of their own pair (one-sided,
    population deviation; a zero deviation or an empty pair selects nothing).  ``sum_dtype``: the dtype the sums run in."""
    if sigma is None:
        return mask.clone()
    sd = sum_dtype or loss.dtype
    w = mask.to(loss.dtype)
    n = mask.sum(dim=(1, 2), keepdim=True).to(sd)
    mean = ((loss * w).to(sd).sum(dim=(1, 2), keepdim=True) / n).to(loss.dtype)
    dev = ((loss - mean) * w).to(sd)
    std = ((dev * dev).sum(dim=(1, 2), keepdim=True) / (n - 1 if mutate == "sample_std" else n)).sqrt().to(loss.dtype)
    z = (loss - mean) / std
    keep = z.abs() < sigma if mutate == "two_sided" else z < sigma          # NaN compares false
    return mask & keep


def loss_value(xy1n, xy2n, translation, scale, rotation, sel):
    """The scalar the reference differentiates: the mean of |xy' - xy2| over the batch's selected elements."""
    _, xy = transform(xy1n, translation, scale, rotation)
    return (xy - xy2n).abs()[sel].mean()


def gradient_sums(xy1n, xy2n, translation, scale, rotation, sel, sum_dtype=None):
    """Closed form: d(sum of the selected |xy' - xy2|) / d(translation [B, 2], scale [B], rotation [B]) per pair, sign(0) = 0.
    Divided by the batch's ``sel.sum()`` they are the gradient of loss_value.  ``sum_dtype``: the dtype the sums run in (and are
    returned in)."""
    sd = sum_dtype or xy1n.dtype
    rot, xy = transform(xy1n, translation, scale, rotation)
    sg = torch.sign(xy - xy2n) * sel.to(xy.dtype)
    g_t = sg.to(sd).sum(dim=1)
    g_s = (sg * rot).to(sd).sum(dim=(1, 2))
    g_r = ((sg[:, :, 1] * rot[:, :, 0]).to(sd) - (sg[:, :, 0] * rot[:, :, 1]).to(sd)).sum(dim=1) * scale.view(-1).to(sd)
    return g_t, g_s, g_r


def run(xy1, xy2, center, mask=None, iteration=50, lr_translation=0.1, lr_scale_rotation=0.1, sigma=None, sigma_min=None,
        sigma_max=2.0, disable_shift=False, disable_scale=False, disable_rotate=False, dtype=torch.float64, mutate=None, sum_dtype=None):
    """-> shift [B, 2], scale [B, 1], angle [B, 1] (degrees), center [B, 2], trace [iteration, B, 4] = (tx, ty, scale, rotation)
    after every step, all in ``dtype``.  ``dtype=torch.float32, sum_dtype=torch.float64`` is the arithmetic of the HIP kernel: fp32
    points and parameters, double sums."""
    assert mutate is None or mutate in MUTATIONS
    B = xy1.shape[0]
    if mask is None:
        mask = torch.ones(xy1.shape, dtype=torch.bool)
    xy1n, xy2n, norm_scale = normalise(xy1, xy2, center, mask, dtype, mutate)
    p = torch.zeros((B, 4), dtype=dtype)
    p[:, 2] = 1.0
    m, v = torch.zeros_like(p), torch.zeros_like(p)
    free = torch.tensor([not disable_shift, not disable_shift, not disable_scale, not disable_rotate])
    eta_min = lr_scale_rotation * 1e-3
    trace = []
    for i in range(iteration):
        t, s, r = p[:, 0:2].view(B, 1, 2), p[:, 2].view(B, 1, 1), p[:, 3].view(B, 1, 1)
        sg = None
        if (sigma_min is not None or sigma is not None) and (i > 0 or mutate == "reject_at_step0"):
            sg = cosine_annealing(sigma_min, sigma_max, i, iteration) if sigma_min is not None else sigma
        _, xy = transform(xy1n, t, s, r)
        sel = select((xy - xy2n).abs(), mask, sg, mutate, sum_dtype)
        g_t, g_s, g_r = gradient_sums(xy1n, xy2n, t, s, r, sel, sum_dtype)
        total = sel.sum(dim=(1, 2)).clamp(min=1).view(B, 1) if mutate == "pair_count" else max(int(sel.sum()), 1)
        g = (torch.cat([g_t, g_s.view(B, 1), g_r.view(B, 1)], dim=1) / total).to(dtype)
        # torch.optim.Adam, step i + 1, learning rates of T_cur = i
        k = i + 1 if mutate == "schedule_plus_one" else i
        lr = torch.tensor([learning_rate(lr_translation, eta_min, k, iteration)] * 2 +
                          [learning_rate(lr_scale_rotation, eta_min, k, iteration)] * 2, dtype=torch.float64)
        bc1, bc2 = (1.0, 1.0) if mutate == "no_bias_correction" else (1.0 - BETA1 ** (i + 1), 1.0 - BETA2 ** (i + 1))
        m_new = g - (g - m) * (1.0 - (1.0 - BETA1))
        v_new = v * BETA2 + ((1.0 - BETA2) * g) * g
        denom = v_new.sqrt() / math.sqrt(bc2) + EPS
        p_new = p + ((-(lr / bc1)).to(dtype) * m_new) / denom
        p, m, v = torch.where(free, p_new, p), torch.where(free, m_new, m), torch.where(free, v_new, v)
        trace.append(p.clone())
    shift = p[:, 0:2] * norm_scale.view(B, 1)
    angle = torch.rad2deg(torch.atan2(p[:, 3:4].sin(), p[:, 3:4].cos()))
    return shift, p[:, 2:3].clone(), angle, center.to(dtype).reshape(B, 2), torch.stack(trace)


# ---- error measures shared by the CPU and the GPU tests ------------------------------------------------------------------------
K_FACTOR = 2.2                     # the project's factor on the reference's own fp32 error
ULP = 2.0 ** -23                   # one fp32 ulp of a normalised coordinate (|xy| <= 1)


def norm_scale_of(xy1, center):
    return normalise(xy1, xy1, center, None, torch.float64)[2].view(-1)


def output_errors(got, truth):
    """(shift, scale, angle) of an implementation and of truth -> RMS over the pairs of the shift error (px, both coordinates),
    the angle error (degrees) and the scale error."""
    (s, c, a), (ts, tc, ta) = [[torch.as_tensor(x).double() for x in g[:3]] for g in (got, truth)]
    return {"shift": float((s - ts).pow(2).sum(dim=1).mean().sqrt()), "angle": float((a - ta).pow(2).mean().sqrt()),
            "scale": float((c - tc).pow(2).mean().sqrt())}


def output_floors(norm_scale):
    """One ulp of the normalised coordinate, in the units of each output."""
    ns = float(norm_scale.double().pow(2).mean().sqrt())
    return {"shift": ULP * ns, "angle": ULP * 180.0 / math.pi, "scale": ULP}


def trace_errors(got, truth, steps=EARLY_STEPS):
    """Largest |difference| of each of the four parameters over the pairs, per step, for the first ``steps`` steps: [steps, 4]."""
    return (torch.as_tensor(got).double()[:steps] - torch.as_tensor(truth).double()[:steps]).abs().amax(dim=1)


# ---- the fixture and the runs the tests share (computed once per process) -------------------------------------------------------
import functools  # noqa: E402
import os  # noqa: E402

FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "find_transform.npz")


@functools.lru_cache(maxsize=None)
def fixture():
    return dict(np.load(FIXTURE))


def fixture_input(name):
    """The recorded inputs of a case -> xy1, xy2, mask or None, center, kwargs."""
    fx = fixture()
    mask = fx.get(f"in/{name}/mask")
    return (torch.from_numpy(fx[f"in/{name}/xy1"]), torch.from_numpy(fx[f"in/{name}/xy2"]),
            None if mask is None else torch.from_numpy(mask), torch.from_numpy(fx[f"in/{name}/center"]), dict(CASES[name][4]))


def fixture_output(name):
    """The reference's own fp32 answer -> shift, scale, angle, trace."""
    fx = fixture()
    return tuple(torch.from_numpy(fx[f"out/{name}/{k}"]) for k in ("shift", "scale", "angle", "trace"))


@functools.lru_cache(maxsize=None)
def restated(name, dtype=torch.float64, mutate=None, sum_dtype=None):
    xy1, xy2, mask, center, kwargs = fixture_input(name)
    with torch.inference_mode():
        return run(xy1, xy2, center, mask, dtype=dtype, mutate=mutate, sum_dtype=sum_dtype, **kwargs)


def output_bound(name, keep=None):
    """K * e_ref + floor per output, e_ref = the fixture against float64; ``keep``: over these pairs of the case only."""
    keep = torch.arange(len(CASES[name][1])) if keep is None else torch.as_tensor(keep)
    e_ref = output_errors([t[keep] for t in fixture_output(name)[:3]], [t[keep] for t in restated(name)[:3]])
    xy1, _, _, center, _ = fixture_input(name)
    floors = output_floors(norm_scale_of(xy1, center)[keep])
    return {k: K_FACTOR * e_ref[k] + floors[k] for k in e_ref}


def output_ratio(name, got_outputs, keep=None):
    """Largest error / bound over the three outputs of an implementation's answer (all pairs of the case given), measured over the
    pairs ``keep``."""
    keep = torch.arange(len(CASES[name][1])) if keep is None else torch.as_tensor(keep)
    err = output_errors([torch.as_tensor(t)[keep] for t in got_outputs[:3]], [t[keep] for t in restated(name)[:3]])
    bound = output_bound(name, keep)
    return max(err[k] / bound[k] for k in err)


def trace_bound(name):
    """K * (the fixture's own deviation from float64) + one ulp, per early step and parameter: [EARLY_STEPS, 4].

    The ulp is that of the normalised coordinate (2^-23), not of the parameter: after one to three steps the parameters are about
    0.1 and the fixture deviates from float64 by a few 1e-9, so K times that alone would hold an implementation to the last bit of
    its cos / sin, and the floor is nearly the whole bound here (every implementation reports the same 0.15 .. 0.4 of it).  What
    the early trace is for is a wrong schedule, bias correction or rejection step, and those move the first steps by 1e-4 or more."""
    return K_FACTOR * trace_errors(fixture_output(name)[3], restated(name)[4]) + ULP


def worst_ratio(name, got_outputs, got_trace):
    """Largest error / bound of an implementation's answer for a case, over the outputs (RMS cases) and the early trace."""
    ratio = float((trace_errors(got_trace, restated(name)[4]) / trace_bound(name)).max())
    if name in RMS_CASES:
        ratio = max(ratio, output_ratio(name, got_outputs))
    return ratio


def error_table(extra=None):
    """The text of profiles/find_transform_errloc.txt: per case e_ref (the reference's fp32 against float64) and e_alt (the fp32
    restatement; torch sums / double sums) per output.  ``extra``: {label: {case: (shift, scale, angle, trace)}} of further implementations (tools/time_find_transform.py: the kernel)."""
    lines = [f"find_transform: RMS over a case's pairs of the error against the float64 restatement; bound = K * e_ref + floor, K = {K_FACTOR},",
             "floor = one fp32 ulp of the normalised coordinate in the output's unit (shift: x norm_scale px, angle: x 180 / pi degrees).",
             "e_ref: the reference's own fp32 run (tests/golden/find_transform.npz); e_alt: tests/find_transform_ref.py in fp32 with torch",
             "sums; e_alt64: the same with double sums (the kernel's arithmetic); e_gpu: the kernel.  worst: largest error / bound over the outputs (cases",
             "with enough pairs for an RMS) and the first three trace steps (every case)."]
    for name in CASES:
        lines.append(f"case {name}: B = {len(CASES[name][1])}, N = {CASES[name][2]}, {CASES[name][4]}")
        impls = {"e_ref": fixture_output(name), "e_alt": restated(name, torch.float32), "e_alt64": restated(name, torch.float32, None, torch.float64)}
        for label, per_case in (extra or {}).items():
            if name in per_case:
                impls[label] = tuple(per_case[name])
        bound = output_bound(name)
        for label, got in impls.items():
            shift, scale, angle = got[0], got[1], got[2]
            trace = got[4] if len(got) == 5 else got[3]
            e = output_errors((shift, scale, angle), restated(name))
            rms = "  ".join(f"{k} {e[k]:.3e} (bound {bound[k]:.3e})" for k in e) if name in RMS_CASES else "(too few pairs for an RMS)"
            lines.append(f"  {label:<8} {rms}  worst {worst_ratio(name, (shift, scale, angle), trace):.3f}")
    return "\n".join(lines) + "\n"


if __name__ == "__main__":
    print(error_table())          # the CPU part; tools/time_find_transform.py writes profiles/find_transform_errloc.txt with the kernel's rows
