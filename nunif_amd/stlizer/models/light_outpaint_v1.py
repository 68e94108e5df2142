"""stlizer ``stlizer.light_outpaint_v1`` (the coarse outpaint net of ``--border outpaint`` / ``expand_outpaint``) on the HIP engine.

Mirrors ``stlizer/models/light_outpaint_v1.py`` (reference) ``LightOutpaintV1`` :156-206: registry name, ``i2i_*`` attributes
(scale 1, offset 0, in_channels 3, blend_size 0), ``forward(x, mask)`` in eval mode :164-173, ``infer(x, mask, max_size=640,
composite=True)`` :175-206 and the ``state_dict`` key layout of ``OutpaintBase(64, window_size=8)`` :87-113 under ``net.``
(including the ``index`` / ``delta`` buffers of the four ``WindowScoreBias``), so the released ``.pth`` loads unchanged.  The net,
both resizes of ``infer``, the pad and the composite are ``nunif_hip_outpaint_infer`` (nunif_amd/csrc/outpaint.hip): fp32 operands
and accumulation.  The reference runs ``infer`` under ``torch.autocast``; an ambient autocast is ignored here (nothing goes through
torch's dispatcher).  Training-mode forward raises.
"""
import ctypes
import math
from collections import OrderedDict

import torch

from ...nunif.models import I2IBaseModel, register_model
from ... import _hip
from ...engine import FlatWeightsMixin, HipEngine
from ...synthetic import window_score_bias_input

DIM, WINDOW, HEAD_DIM, BIAS_HIDDEN = 64, 8, 32, 16
DCT_DIMS = (4, DIM // 8, DIM // 4, DIM)
# (reference prefix under net., engine prefix, channels) of every MHABlock + PoolBlock pair, in registration order
BLOCKS = (("enc_block.0", "enc_block.1", "enc", DIM), ("mid_block.0", "mid_block.1", "mid0", DIM // 2),
          ("mid_block.2", "mid_block.3", "mid1", DIM // 2), ("dec_block.0", "dec_block.1", "dec", DIM))
MODES = {"composite": 0, "raw": 1, "forward": 2}
TAP_NAMES = ("dct", "enc", "mid", "dec", "proj")
NO_RESIZE = 2 ** 31 - 1


def state_dict_shapes():
    """Ordered ``{key: shape}`` of ``LightOutpaintV1().state_dict()`` in the reference."""
    sd = OrderedDict()
    n = WINDOW * WINDOW

    def conv(p, cout, cin, k=1, groups=1):
        sd[p + ".weight"] = (cout, cin // groups, k, k)
        sd[p + ".bias"] = (cout,)

    def linear(p, cout, cin):
        sd[p + ".weight"] = (cout, cin)
        sd[p + ".bias"] = (cout,)

    def mha_block(p, c):
        linear(p + ".mha.mha.qkv_proj", 3 * c, c)
        linear(p + ".mha.mha.head_proj", c, c)
        conv(p + ".mlp.0", 2 * c, c)
        conv(p + ".mlp.2", c, c)
        sd[p + ".bias.index"] = (n * n,)
        sd[p + ".bias.delta"] = ((2 * WINDOW - 1) ** 2, 2)
        linear(p + ".bias.to_bias.0", BIAS_HIDDEN, 2)
        linear(p + ".bias.to_bias.2", 1, BIAS_HIDDEN)

    def pool_block(p, c):
        conv(p + ".mlp.0", 2 * c, c)
        conv(p + ".mlp.3", 2 * c, 2 * c, 3, groups=2 * c)
        conv(p + ".mlp.5", c, c)

    for i in range(3):
        conv(f"net.dct.blocks.{3 * i + 1}", DCT_DIMS[i + 1], DCT_DIMS[i], 3)
    conv("net.proj_mid", DIM // 2, DIM)
    conv("net.proj_out", DIM, DIM // 2)
    for mha, pool, _, c in BLOCKS:
        mha_block("net." + mha, c)
        pool_block("net." + pool, c)
    conv("net.to_image_biliner.proj", 3, DIM)
    return sd


def _init_weights():
    index, delta = window_score_bias_input((WINDOW, WINDOW))
    sd = OrderedDict()
    for k, shape in state_dict_shapes().items():
        if k.endswith(".bias.index"):
            sd[k] = index.clone()
        elif k.endswith(".bias.delta"):
            sd[k] = delta.clone()
        elif len(shape) >= 2:
            sd[k] = torch.randn(shape) * math.sqrt(1.0 / math.prod(shape[1:]))
        else:
            sd[k] = torch.zeros(shape)
    return sd


def score_bias_table(sd, p):
    """``WindowScoreBias.forward()`` (nunif/modules/attention.py:408-415) of the block at ``p`` with ``num_heads=None``:
    ``to_bias(delta)[index]`` as one [64, 64] table, in float64 (GELU exact)."""
    g = lambda k: sd[f"{p}.bias.{k}"].double()     # noqa: E731
    hid = torch.nn.functional.gelu(g("delta") @ g("to_bias.0.weight").t() + g("to_bias.0.bias"))
    bias = hid @ g("to_bias.2.weight").t() + g("to_bias.2.bias")
    n = WINDOW * WINDOW
    return bias[sd[f"{p}.bias.index"].long()].reshape(n, n)


def pack_weights(sd):
    """Reference state dict -> the packed fp32 tensors ``nunif_hip_outpaint_create`` takes (layout: include/nunif_hip.h).  Nothing
    is folded; matrices become input-major, the qkv columns are grouped by head, the first PoolBlock conv's columns by 32-channel
    GLU chunk, and the score-bias MLP is evaluated into its table."""
    out = OrderedDict()
    for i in range(3):
        w = sd[f"net.dct.blocks.{3 * i + 1}.weight"].double()                       # [Cout, Cin, 3, 3] -> [(kh*3+kw)*Cin + c][Cout]
        out[f"dct.{i}.w"] = w.permute(2, 3, 1, 0).reshape(-1, w.shape[0])
        out[f"dct.{i}.b"] = sd[f"net.dct.blocks.{3 * i + 1}.bias"]
    for mha, pool, e, c in BLOCKS:
        m, q = "net." + mha, "net." + pool
        heads = c // HEAD_DIM
        order = torch.tensor([part * c + h * HEAD_DIM + d for h in range(heads) for part in range(3) for d in range(HEAD_DIM)])
        out[e + ".mha.qkv.w"] = sd[m + ".mha.mha.qkv_proj.weight"][order].t()
        out[e + ".mha.qkv.b"] = sd[m + ".mha.mha.qkv_proj.bias"][order]
        out[e + ".mha.table"] = score_bias_table(sd, m)
        out[e + ".mha.proj.w"] = sd[m + ".mha.mha.head_proj.weight"].t()
        out[e + ".mha.proj.b"] = sd[m + ".mha.mha.head_proj.bias"]
        out[e + ".mha.mlp1.w"] = sd[m + ".mlp.0.weight"][:, :, 0, 0].t()
        out[e + ".mha.mlp1.b"] = sd[m + ".mlp.0.bias"]
        out[e + ".mha.mlp2.w"] = sd[m + ".mlp.2.weight"][:, :, 0, 0].t()
        out[e + ".mha.mlp2.b"] = sd[m + ".mlp.2.bias"]
        chunk = torch.tensor([half * c + j * 32 + i for j in range(c // 32) for half in range(2) for i in range(32)])
        out[e + ".pool.pw1.w"] = sd[q + ".mlp.0.weight"][:, :, 0, 0][chunk].t()
        out[e + ".pool.pw1.b"] = sd[q + ".mlp.0.bias"][chunk]
        out[e + ".pool.dw.w"] = sd[q + ".mlp.3.weight"].reshape(2 * c, 9).t()
        out[e + ".pool.dw.b"] = sd[q + ".mlp.3.bias"]
        out[e + ".pool.pw2.w"] = sd[q + ".mlp.5.weight"][:, :, 0, 0].t()
        out[e + ".pool.pw2.b"] = sd[q + ".mlp.5.bias"]
    out["proj_mid.w"] = sd["net.proj_mid.weight"][:, :, 0, 0].t()
    out["proj_mid.b"] = sd["net.proj_mid.bias"]
    out["proj_out.w"] = sd["net.proj_out.weight"][:, :, 0, 0].t()
    out["proj_out.b"] = sd["net.proj_out.bias"]
    out["to_image.w"] = sd["net.to_image_biliner.proj.weight"][:, :, 0, 0]
    out["to_image.b"] = sd["net.to_image_biliner.proj.bias"]
    return OrderedDict((k, v.to(torch.float32).contiguous()) for k, v in out.items())


def _ptr(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else None


@register_model
class LightOutpaintV1(FlatWeightsMixin, I2IBaseModel):
    name = "stlizer.light_outpaint_v1"

    def __init__(self):
        super().__init__({}, scale=1, offset=0, in_channels=3, blend_size=0)
        self._setup_weights(_init_weights())
        self._last = None
        self.eval()

    def _make_engine(self, device):
        return HipEngine(device, pack_weights(self._weights), "nunif_hip_outpaint_create", "nunif_hip_outpaint_destroy",
                         label="light_outpaint_v1")

    def pack_weights(self):
        return pack_weights(self._weights)

    def _run(self, x, mask, max_size, mode):
        if self.training:
            raise RuntimeError("the HIP engine is inference-only; call .eval()")
        assert x.ndim == 4 and x.shape[1] == 3 and mask.ndim == 4 and mask.shape[1] == 1 and mask.shape[0] == x.shape[0]
        assert tuple(mask.shape[2:]) == tuple(x.shape[2:])
        eng = self.engine()
        dev = eng.device
        xin = x.to(device=dev, dtype=torch.float32).contiguous()
        m8 = (mask.to(device=dev) != 0).to(torch.uint8).contiguous()
        B, _, H, W = xin.shape
        lib = _hip.lib()
        nbytes = lib.nunif_hip_outpaint_work_bytes(B, H, W, int(max_size))
        if nbytes < 0:
            _hip.check(-1)
        work = torch.empty((nbytes + 3) // 4, dtype=torch.float32, device=dev)
        out = torch.empty_like(xin)
        eng.call(lib.nunif_hip_outpaint_infer, eng.handle, _ptr(xin), _ptr(m8), B, H, W, int(max_size), MODES[mode], _ptr(out),
                 _ptr(work))
        self._last = (work, B, H, W, int(max_size))
        return out.to(x.dtype) if x.is_floating_point() else out

    def forward(self, x, mask):
        return self._run(x, mask, NO_RESIZE, "forward")

    def infer(self, x, mask, max_size=640, composite=True):
        return self._run(x, mask, max_size, "composite" if composite else "raw")

    def debug_tap(self, name):
        """A map of the last ``infer`` / ``forward`` (tests): "dct", "enc", "mid", "dec" ``[B, 64, h, w]``, "proj" ``[B, 3, h, w]``."""
        assert self._last is not None, "no infer has run on this model"
        work, B, H, W, max_size = self._last
        eng = self.engine()
        shape = (ctypes.c_int64 * 4)()
        cap = work.numel()
        out = torch.empty(cap, dtype=torch.float32, device=eng.device)
        eng.call(_hip.lib().nunif_hip_outpaint_debug_taps, eng.handle, _ptr(work), B, H, W, max_size, name.encode(), _ptr(out), cap,
                 shape)
        s = list(shape)
        return out[: s[0] * s[1] * s[2] * s[3]].reshape(s).permute(0, 3, 1, 2).contiguous()
