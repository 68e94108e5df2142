"""SuperPoint keypoints, descriptor matching and the stabilising warp of stlizer on the HIP engine.

Mirrors ``nunif/utils/superpoint.py`` (reference): ``SuperPoint`` :74-203 (the constructor conf, the ``state_dict`` keys and
shapes, ``load()``, ``.to()`` / ``.eval()``, ``forward`` and ``infer`` with the reference's return structure),
``find_match_index`` :206-223, ``apply_transform`` :330-378, and ``sample_descriptors`` :16-27, ``batched_nms`` :30-45 and
``select_top_k_keypoints`` :48-52 for completeness.  The kernels are in nunif_amd/csrc/superpoint.hip: fp32 operands and
accumulation throughout.  The reference runs the net under ``torch.autocast``; an ambient autocast is ignored here (nothing goes
through torch's dispatcher).

``find_transform`` and ``cosine_annealing`` are NOT part of this module: they are an autograd Adam loop over a few hundred
points (:226-327) and stay the reference's; ``install()`` leaves them bound where they are.

Only the geometry that ``SuperPoint()`` builds (channels [64, 64, 128, 128, 256], descriptor_dim 256) exists as kernels.
"""
import ctypes
from collections import OrderedDict
from types import SimpleNamespace

import torch

from ... import _hip
from ...engine import FlatWeightsMixin, HipEngine

WEIGHTS_URL = "https://github.com/nagadomi/nunif/releases/download/0.0.0/superpoint_v6_from_tf.pth"
BN_EPS = 1e-3
CHANNELS = [64, 64, 128, 128, 256]
DESCRIPTOR_DIM = 256
PADDING_MODES = {"zeros": 0, "border": 1}


class OptionNotSupported(NotImplementedError, ValueError):
    """An option the reference accepts (and hands to torch) that has no kernel here."""


def _vgg_blocks():
    """(reference prefix, Cin, Cout, kernel size) of every VGGBlock, in the reference's order."""
    blocks = []
    chans = [1] + CHANNELS[:-1]
    for i in range(1, len(chans)):
        blocks.append((f"backbone.{i - 1}.0", chans[i - 1], chans[i], 3))
        blocks.append((f"backbone.{i - 1}.1", chans[i], chans[i], 3))
    c = CHANNELS[-1]
    blocks.append(("detector.0", chans[-1], c, 3))
    blocks.append(("detector.1", c, 65, 1))
    blocks.append(("descriptor.0", chans[-1], c, 3))
    blocks.append(("descriptor.1", c, DESCRIPTOR_DIM, 1))
    return blocks


def state_dict_shapes():
    """Reference key -> shape, in the reference's own order."""
    shapes = OrderedDict()
    for p, cin, cout, k in _vgg_blocks():
        shapes[p + ".conv.weight"] = (cout, cin, k, k)
        shapes[p + ".conv.bias"] = (cout,)
        for name in ("weight", "bias", "running_mean", "running_var"):
            shapes[p + ".bn." + name] = (cout,)
        shapes[p + ".bn.num_batches_tracked"] = ()
    return shapes


def _init_weights():
    sd = OrderedDict()
    for key, shape in state_dict_shapes().items():
        if key.endswith("num_batches_tracked"):
            sd[key] = torch.zeros((), dtype=torch.long)
        elif ".bn." in key:
            sd[key] = torch.ones(shape) if key.endswith(("bn.weight", "running_var")) else torch.zeros(shape)
        elif key.endswith(".bias"):
            sd[key] = torch.zeros(shape)
        else:
            fan_in = shape[1] * shape[2] * shape[3]
            sd[key] = torch.randn(shape) * (1.0 / fan_in) ** 0.5
    return sd


def bn_affine(sd, p):
    """BatchNorm2d(eps 1e-3) of block ``p`` in eval mode as ``y = x * scale + shift``, in float64."""
    w, b, mean, var = (sd[f"{p}.bn.{k}"].double() for k in ("weight", "bias", "running_mean", "running_var"))
    scale = w / torch.sqrt(var + BN_EPS)
    return scale, b - mean * scale


def pack_weights(sd):
    """Reference state dict -> the packed fp32 tensors ``nunif_hip_superpoint_create`` takes (layout: include/nunif_hip.h).

    A VGGBlock is conv -> ReLU -> BN: the BN of a block with a ReLU cannot be folded into its conv (the ReLU sits between) nor
    into the next conv (which pads the BN OUTPUT with zeros), so it travels as a per-channel ``scale`` / ``shift`` that the
    kernel applies after bias and ReLU.  The two 1x1 head convs have ``relu=False``: their BN folds into weight and bias.  All
    arithmetic in float64."""
    out = OrderedDict()

    def conv3(p):
        w = sd[p + ".conv.weight"].double()                       # [Cout, Cin, 3, 3] -> [(kh*3+kw)*Cin + c][Cout]
        scale, shift = bn_affine(sd, p)
        return w.permute(2, 3, 1, 0).reshape(-1, w.shape[0]), sd[p + ".conv.bias"].double(), scale, shift

    for b in range(4):
        for i in range(2):
            for name, t in zip(("w", "bias", "scale", "shift"), conv3(f"backbone.{b}.{i}")):
                out[f"backbone.{b}.{i}.{name}"] = t
    det, desc = conv3("detector.0"), conv3("descriptor.0")
    for j, name in enumerate(("w", "bias", "scale", "shift")):
        out["heads." + name] = torch.cat([det[j], desc[j]], dim=-1)
    for p, npad in (("detector", 96), ("descriptor", DESCRIPTOR_DIM)):
        w = sd[p + ".1.conv.weight"].double()[:, :, 0, 0]         # [Cout, 256]
        scale, shift = bn_affine(sd, p + ".1")
        wt = (w * scale[:, None]).t()
        bias = sd[p + ".1.conv.bias"].double() * scale + shift
        out[p + ".w"] = torch.nn.functional.pad(wt, (0, npad - wt.shape[1]))
        out[p + ".bias"] = torch.nn.functional.pad(bias, (0, npad - bias.shape[0]))
    return OrderedDict((k, v.to(torch.float32).contiguous()) for k, v in out.items())


def _ptr(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else None


def _need_device(t, what):
    if t.device.type != "cuda":
        raise RuntimeError(f"{what}: the HIP engine needs a ROCm device tensor (got {t.device}); there is no CPU fallback")


def _reference_on_host(name, t):
    """The reference's own function behind ``name`` for a tensor that is not on a ROCm device, while ``install()`` is active
    (stlizer with ``--gpu -1`` keeps its CPU path: that is the reference running its own code, not a stand-in for a kernel).
    ``None`` for a device tensor; without ``install()`` a host tensor raises."""
    if t.device.type == "cuda":
        return None
    from ...install import original
    fn = original("nunif.utils.superpoint", name)
    if fn is None:
        _need_device(t, name)
    return fn


def _keypoints_from_scores(scores, nms_radius, remove_borders, threshold, want_keypoints=True):
    """``nunif_hip_superpoint_keypoints`` on score maps ``[B, H, W]``: (nms map, keypoints, keypoint scores, counts)."""
    _need_device(scores, "keypoints")
    scores = scores.to(torch.float32).contiguous()
    B, H, W = scores.shape
    dev = scores.device
    lib = _hip.lib()
    work = torch.empty(lib.nunif_hip_superpoint_keypoints_work_floats(B, H, W), dtype=torch.float32, device=dev)
    nms = torch.empty_like(scores)
    kp = kps = counts = None
    if want_keypoints:
        kp = torch.empty((B, H * W, 2), dtype=torch.float32, device=dev)
        kps = torch.empty((B, H * W), dtype=torch.float32, device=dev)
        counts = torch.empty((B,), dtype=torch.int32, device=dev)
    with torch.cuda.device(dev):
        _hip.check(lib.nunif_hip_superpoint_keypoints(
            _ptr(scores), B, H, W, int(nms_radius), int(remove_borders or 0), float(threshold), _ptr(work), _ptr(nms),
            _ptr(kp), _ptr(kps), _ptr(counts), _hip.current_stream_ptr(dev)))
    return nms, kp, kps, counts


def batched_nms(scores, nms_radius: int):
    assert nms_radius >= 0
    shape = scores.shape
    nms = _keypoints_from_scores(scores.reshape(-1, shape[-2], shape[-1]), nms_radius, 0, 0.0, want_keypoints=False)[0]
    return nms.reshape(shape).to(scores.dtype)


def select_top_k_keypoints(keypoints, scores, k):
    if k >= len(keypoints):
        return keypoints, scores
    scores, indices = torch.topk(scores, k, dim=0, sorted=True)
    return keypoints[indices], scores


def sample_descriptors(keypoints, descriptors, s: int = 8):
    """Interpolate descriptors at keypoint locations: ``[b, n, 2]`` and ``[b, c, h, w]`` -> ``[b, c, n]`` (the reference's layout)."""
    _need_device(descriptors, "sample_descriptors")
    b, c, h, w = descriptors.shape
    dense = descriptors.to(torch.float32).permute(0, 2, 3, 1).contiguous()
    kp = keypoints.to(device=descriptors.device, dtype=torch.float32).reshape(b, -1, 2).contiguous()
    n = kp.shape[1]
    out = torch.empty((b, n, c), dtype=torch.float32, device=descriptors.device)
    with torch.cuda.device(descriptors.device):
        for i in range(b):
            _hip.check(_hip.lib().nunif_hip_sample_descriptors(
                _ptr(kp[i]), n, _ptr(dense[i]), h, w, c, int(s), _ptr(out[i]), _hip.current_stream_ptr(descriptors.device)))
    return out.transpose(1, 2).to(descriptors.dtype)


class SuperPoint(FlatWeightsMixin, torch.nn.Module):
    default_conf = {
        "nms_radius": 4,
        "max_num_keypoints": None,
        "detection_threshold": 0.005,
        "remove_borders": 4,
        "descriptor_dim": 256,
        "channels": [64, 64, 128, 128, 256],
    }

    def __init__(self, **conf):
        super().__init__()
        conf = {**self.default_conf, **conf}
        self.conf = SimpleNamespace(**conf)
        if list(self.conf.channels) != CHANNELS or self.conf.descriptor_dim != DESCRIPTOR_DIM:
            raise OptionNotSupported(
                "the HIP engine builds SuperPoint only in the geometry of SuperPoint(): channels [64, 64, 128, 128, 256], "
                "descriptor_dim 256")
        self.stride = 2 ** (len(self.conf.channels) - 2)
        self._setup_weights(_init_weights())
        self._last_numel = 0
        self.eval()

    def _make_engine(self, device):
        return HipEngine(device, pack_weights(self._weights), "nunif_hip_superpoint_create", "nunif_hip_superpoint_destroy",
                         label="SuperPoint")

    def load(self, map_location="cpu"):
        self.load_state_dict(torch.hub.load_state_dict_from_url(WEIGHTS_URL, weights_only=True, map_location=map_location))
        return self

    def _net(self, image, keypoints=True):
        """Run the engine on ``[B, C, H, W]``: (keypoints [B, cap, 2], scores [B, cap], counts [B]) on the device, or nothing with
        ``keypoints=False`` (dense outputs stay in the handle for :meth:`debug_tap`)."""
        if self.training:
            raise RuntimeError("the HIP engine is inference-only; call .eval()")
        assert torch.is_tensor(image) and image.ndim == 4 and image.shape[1] in (1, 3), "image must be [B, 1 or 3, H, W]"
        eng = self.engine()
        dev = eng.device
        x = image.to(device=dev, dtype=torch.float32).contiguous()
        B, C, H, W = x.shape
        self._last_numel = B * H * W
        cap = (H // 8) * (W // 8) * 64
        kp = kps = counts = None
        if keypoints:
            kp = torch.empty((B, cap, 2), dtype=torch.float32, device=dev)
            kps = torch.empty((B, cap), dtype=torch.float32, device=dev)
            counts = torch.empty((B,), dtype=torch.int32, device=dev)
        eng.call(_hip.lib().nunif_hip_superpoint_forward, eng.handle, _ptr(x), B, C, H, W, int(self.conf.nms_radius),
                 int(self.conf.remove_borders or 0), float(self.conf.detection_threshold), _ptr(kp), _ptr(kps), _ptr(counts))
        return kp, kps, counts

    def debug_tap(self, name):
        """A buffer of the last forward (tests): "backbone.0" .. "backbone.3", "heads", "descriptors" as ``[B, C, h, w]``,
        "scores" / "nms" as ``[B, H, W]``."""
        eng = self.engine()
        shape = (ctypes.c_int64 * 4)()
        cap = 16 * self._last_numel                               # the largest tap, backbone.0, is [B, H/2, W/2, 64]
        out = torch.empty(cap, dtype=torch.float32, device=eng.device)
        eng.call(_hip.lib().nunif_hip_superpoint_debug_taps, eng.handle, name.encode(), _ptr(out), cap, shape)
        s = list(shape)
        t = out[: s[0] * s[1] * s[2] * s[3]].reshape(s)
        if name in ("scores", "nms"):
            return t[:, 0].clone()
        return t.permute(0, 3, 1, 2).contiguous()

    def forward(self, image):
        dev = self.get_device()
        kp, kps, counts = self._net(image)
        counts = counts.tolist()                                  # the one host read per batch: the output is ragged
        b = len(counts)
        keypoints, scores, descriptors = [], [], []
        lib, eng = _hip.lib(), self.engine()
        for i in range(b):
            k, s = kp[i, :counts[i]], kps[i, :counts[i]]
            if self.conf.max_num_keypoints is not None:
                k, s = select_top_k_keypoints(k, s, self.conf.max_num_keypoints)
            k, s = k.contiguous().clone(), s.clone()              # not views: the capacity buffers are not kept alive
            d = torch.empty((k.shape[0], DESCRIPTOR_DIM), dtype=torch.float32, device=dev)
            eng.call(lib.nunif_hip_superpoint_sample, eng.handle, i, _ptr(k), k.shape[0], _ptr(d))
            keypoints.append(k)
            scores.append(s)
            descriptors.append(d)
        return {
            "keypoints": keypoints,
            "keypoint_scores": scores,
            "descriptors": descriptors,
        }

    @torch.inference_mode()
    def infer(self, x):
        if x.ndim == 3:
            x = x.unsqueeze(0)
            batch = False
        else:
            batch = True

        ret = self.forward(x)

        # convert to batch-first structure
        new_ret = []
        for i in range(x.shape[0]):
            new_ret.append({
                "keypoints": ret["keypoints"][i],
                "descriptors": ret["descriptors"][i],
                "keypoint_scores": ret["keypoint_scores"][i]
            })
        if not batch:
            new_ret = new_ret[0]

        return new_ret


def match_descriptors(d1, d2):
    """For each row of ``d1`` the argmax (int64) and max (fp32) over the rows of ``d2`` of their dot product; the ``N1 x N2``
    matrix is never materialised (``nunif_hip_superpoint_match``)."""
    _need_device(d1, "find_match_index")
    d1 = d1.to(torch.float32).contiguous()
    d2 = d2.to(device=d1.device, dtype=torch.float32).contiguous()
    n1, n2, D = d1.shape[0], d2.shape[0], d1.shape[1]
    assert d2.shape[1] == D
    index = torch.empty((n1,), dtype=torch.int64, device=d1.device)
    sim = torch.empty((n1,), dtype=torch.float32, device=d1.device)
    work = torch.empty((n1,), dtype=torch.int64, device=d1.device)
    with torch.cuda.device(d1.device):
        _hip.check(_hip.lib().nunif_hip_superpoint_match(_ptr(d1), n1, _ptr(d2), n2, D, _ptr(work), _ptr(index), _ptr(sim),
                                                         _hip.current_stream_ptr(d1.device)))
    return index, sim


@torch.inference_mode()
def find_match_index(kp1, kp2, threshold=0.5, return_score=False, return_score_all=False):
    d1 = kp1["descriptors"]
    d2 = kp2["descriptors"]
    host = _reference_on_host("find_match_index", d1)
    if host is not None:
        return host(kp1, kp2, threshold=threshold, return_score=return_score, return_score_all=return_score_all)

    if d1.shape[0] == 0 or d2.shape[0] == 0:
        # nothing to multiply: the reference's own expressions on the empty operands (they raise where torch raises)
        cosine_similarity = d1 @ d2.t()
        match_index = torch.argmax(cosine_similarity, dim=-1)
        max_similarity = torch.gather(cosine_similarity, dim=1, index=match_index.view(-1, 1)).view(-1)
    else:
        match_index, max_similarity = match_descriptors(d1, d2)
        max_similarity = max_similarity.to(d1.dtype)
    filter_index = max_similarity > threshold
    kp1_index = torch.arange(d1.shape[0], device=d1.device)[filter_index]
    kp2_index = match_index[filter_index]
    if return_score or return_score_all:
        if return_score_all:
            return kp1_index, kp2_index, max_similarity
        else:
            return kp1_index, kp2_index, max_similarity[filter_index]
    else:
        return kp1_index, kp2_index


@torch.inference_mode()
def apply_transform(x, shift, scale, angle, center, mode="bilinear", padding_mode="border"):
    # `mode` is accepted and ignored, as in the reference (:373 passes "bilinear" whatever it is)
    host = _reference_on_host("apply_transform", x)
    if host is not None:
        return host(x, shift, scale, angle, center, mode=mode, padding_mode=padding_mode)
    if padding_mode not in PADDING_MODES:
        raise OptionNotSupported(f"apply_transform: padding_mode={padding_mode!r} has no kernel (built: {sorted(PADDING_MODES)})")
    if x.ndim == 3:
        x = x.unsqueeze(0)
        host = torch.tensor([float(v) for v in list(shift)] + [float(scale), float(angle)] + [float(v) for v in list(center)],
                            dtype=torch.float32)
        assert host.numel() == 6
        params = host.to(x.device).view(1, 6)
        batch = False
    else:
        batch = True
        assert x.ndim == 4
        assert x.shape[0] == shift.shape[0] == scale.shape[0] == angle.shape[0] == center.shape[0]
        B = x.shape[0]
        params = torch.cat([t.to(device=x.device, dtype=torch.float32).reshape(B, -1) for t in (shift, scale, angle, center)],
                           dim=1).contiguous()
        assert params.shape[1] == 6
    xin = x.to(torch.float32).contiguous()
    B, C, H, W = xin.shape
    out = torch.empty_like(xin)
    with torch.cuda.device(x.device):
        _hip.check(_hip.lib().nunif_hip_affine_warp(_ptr(xin), _ptr(params), _ptr(out), B, C, H, W, PADDING_MODES[padding_mode],
                                                    _hip.current_stream_ptr(x.device)))
    out = out.to(x.dtype)
    if batch:
        return out
    else:
        return out[0]
