"""What the three cliqa nets share: the reference's ``state_dict`` key layout, the BatchNorm fold, and the model base on the HIP
engine (``nunif_hip_cliqa_*``, nunif_amd/csrc/cliqa.hip).

The nets differ in the first conv's input channels (6: YCbCr + RGB, or 3), in whether their convs carry a bias (ScaleFactor's do)
and in their heads.  The kind is read off the state-dict keys (``detect_kind``).
"""
import ctypes
import math
from collections import OrderedDict

import torch

from ...nunif.models import Model
from ... import _hip
from ...engine import FlatWeightsMixin, HipEngine

BN_EPS = 1e-5
# kind -> (engine's kind id, first-conv Cin, convs carry a bias, heads in registration order)
KINDS = OrderedDict([
    ("jpeg_quality", (0, 6, False, ("quality_output", "subsampling_output"))),
    ("grain_noise_level", (1, 3, False, ("noise_level_output",))),
    ("scale_factor", (2, 3, True, ("scale_factor_output",))),
])
# (engine name, conv key prefix, BatchNorm key prefix, Cin (None: the kind's), Cout) of the trunk, in registration order; the
# ResBlocks' convs never carry a bias (ResBlockBNReLU, nunif/modules/res_block.py:84-88)
TRUNK = (("conv1", "features.0", "features.1", None, 64), ("conv2", "features.3", "features.4", 64, 128),
         ("rb1a", "features.7.conv.0", "features.7.conv.1", 128, 128), ("rb1b", "features.7.conv.3", "features.7.conv.4", 128, 128),
         ("rb2a", "features.9.conv.0", "features.9.conv.1", 128, 128), ("rb2b", "features.9.conv.3", "features.9.conv.4", 128, 128))
TAP_NAMES = ("pool1", "pool2", "pool3", "head_maps")


def detect_kind(keys):
    keys = set(keys)
    for kind, (_, _, _, heads) in KINDS.items():
        if all(h + ".0.weight" in keys for h in heads):
            return kind
    raise ValueError("not a cliqa state dict: no quality_output / noise_level_output / scale_factor_output keys")


def _bn_shapes(sd, prefix, c):
    for name in ("weight", "bias", "running_mean", "running_var"):
        sd[f"{prefix}.{name}"] = (c,)
    sd[f"{prefix}.num_batches_tracked"] = ()


def state_dict_shapes(kind):
    """Ordered ``{key: shape}`` of the reference class's ``state_dict()``."""
    _, cin0, conv_bias, heads = KINDS[kind]
    sd = OrderedDict()
    for _, conv, bn, cin, cout in TRUNK:
        sd[conv + ".weight"] = (cout, cin or cin0, 3, 3)
        if conv_bias and not conv.startswith(("features.7", "features.9")):
            sd[conv + ".bias"] = (cout,)
        _bn_shapes(sd, bn, cout)
    for h in heads:
        sd[h + ".0.weight"] = (256, 128, 3, 3)
        if conv_bias:
            sd[h + ".0.bias"] = (256,)
        _bn_shapes(sd, h + ".1", 256)
        sd[h + ".4.weight"] = (1, 256, 1, 1)
        sd[h + ".4.bias"] = (1,)
    return sd


def init_weights(kind):
    """The reference constructors' initialisation (kaiming_normal_ fan_out for convs, BatchNorm 1 / 0, biases 0)."""
    sd = OrderedDict()
    for k, shape in state_dict_shapes(kind).items():
        if k.endswith("num_batches_tracked"):
            sd[k] = torch.zeros((), dtype=torch.long)
        elif len(shape) == 4:
            sd[k] = torch.randn(shape) * math.sqrt(2.0 / (shape[0] * shape[2] * shape[3]))
        elif k.endswith("running_var") or (k.endswith(".weight") and len(shape) == 1):
            sd[k] = torch.ones(shape)
        else:
            sd[k] = torch.zeros(shape)
    return sd


def fold_bn(sd, conv, bn):
    """Conv2d ``conv`` followed by eval-mode BatchNorm2d ``bn`` as one conv: float64 ``(weight, bias)``."""
    g = lambda n: sd[n].double()     # noqa: E731
    scale = g(bn + ".weight") / torch.sqrt(g(bn + ".running_var") + BN_EPS)
    w = g(conv + ".weight") * scale[:, None, None, None]
    b0 = g(conv + ".bias") if conv + ".bias" in sd else torch.zeros_like(scale)
    b = (b0 - g(bn + ".running_mean")) * scale + g(bn + ".bias")
    return w, b


def pack_weights(sd):
    """Reference state dict -> ``(kind, tensors)``: the fp32 tensors ``nunif_hip_cliqa_create`` takes (include/nunif_hip.h), BatchNorm
    folded in float64.  The fragment order of the MFMA operands is the engine's (csrc/host_weights.h)."""
    kind = detect_kind(sd.keys())
    packed = OrderedDict()
    for name, conv, bn, _, _ in TRUNK:
        w, b = fold_bn(sd, conv, bn)
        packed[name + ".w"], packed[name + ".b"] = w.float().contiguous(), b.float().contiguous()
    for i, h in enumerate(KINDS[kind][3]):
        w, b = fold_bn(sd, h + ".0", h + ".1")
        packed[f"head{i}.w"], packed[f"head{i}.b"] = w.float().contiguous(), b.float().contiguous()
        packed[f"head{i}.ow"] = sd[h + ".4.weight"].float().reshape(256).contiguous()
        packed[f"head{i}.ob"] = sd[h + ".4.bias"].float().reshape(1).contiguous()
    return kind, packed


class CliqaNet(FlatWeightsMixin, Model):
    """Base of the three nets.  ``group``: images per pass of the engine over a large batch (0: the engine's default)."""
    kind = None

    def __init__(self):
        super().__init__({})
        self._setup_weights(init_weights(self.kind))
        self.group = 0
        self.eval()

    def _param_filter(self, name, tensor):
        return tensor.is_floating_point() and "running_" not in name

    def _make_engine(self, device):
        kind, packed = pack_weights(self._weights)
        assert kind == self.kind
        return HipEngine(device, packed, "nunif_hip_cliqa_create", "nunif_hip_cliqa_destroy", KINDS[kind][0], label="cliqa")

    def _run(self, x, taps=False):
        if self.training:
            raise RuntimeError("the HIP engine is inference-only; call .eval()")
        eng = self.engine()
        dev, lib = eng.device, _hip.lib()
        assert x.ndim == 4 and x.shape[1] == 3, "x: [B,3,H,W]"
        x = x.to(device=dev, dtype=torch.float32).contiguous()
        B, _, H, W = x.shape
        heads = len(KINDS[self.kind][3])
        nbytes = lib.nunif_hip_cliqa_workspace_bytes(eng.handle, B, H, W, self.group)
        if nbytes <= 0:
            raise ValueError(f"cliqa: input {tuple(x.shape)} is not supported (B >= 1, H and W >= 8)")
        ws = torch.empty((nbytes,), dtype=torch.uint8, device=dev)
        outs = [torch.empty((B, 1), dtype=torch.float32, device=dev) for _ in range(heads)]
        ptr = lambda t: ctypes.c_void_p(t.data_ptr() if t is not None else None)     # noqa: E731
        args = [eng.handle, ptr(x), B, H, W, self.group, ptr(ws), nbytes, ptr(outs[0]), ptr(outs[1] if heads == 2 else None)]
        if not taps:
            eng.call(lib.nunif_hip_cliqa_forward, *args)
            return outs, None
        h1, w1 = H // 2, W // 2
        h2, w2 = h1 // 2, w1 // 2
        h3, w3 = h2 // 2, w2 // 2
        t = [torch.empty((B, h, w, 128), dtype=torch.float16, device=dev) for h, w in ((h1, w1), (h2, w2), (h3, w3))]
        t.append(torch.empty((B, h3, w3, heads * 256), dtype=torch.float32, device=dev))
        eng.call(lib.nunif_hip_cliqa_debug_taps, *args, *[ptr(v) for v in t])
        return outs, OrderedDict((n, v.permute(0, 3, 1, 2).float()) for n, v in zip(TAP_NAMES, t))

    @torch.inference_mode()
    def forward(self, x):
        outs, _ = self._run(x)
        return tuple(outs) if len(outs) == 2 else outs[0]

    @torch.inference_mode()
    def debug_taps(self, x):
        """Tests only: ``(outputs, {pool1, pool2, pool3: [B,128,h,w]; head_maps: [B,heads*256,H/8,W/8]})`` of one forward: the maps
        behind the three pools and the head maps in front of the global pools (after each head's ReLU)."""
        return self._run(x, taps=True)
