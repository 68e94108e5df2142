"""The Python side of an engine: how a state dict becomes a ``nunif_hip_*`` handle, who owns that handle, and the model surface
(``state_dict`` / ``load_state_dict`` / ``parameters`` / ``deepcopy``) of a class that keeps flat fp32 master weights beside it.

A new engine subclasses :class:`HipEngine` for its C calls and mixes :class:`FlatWeightsMixin` into its model class; neither
builds a ``TensorDesc`` nor destroys a handle itself.
"""
import copy
import ctypes
from collections import OrderedDict

import torch

from . import _hip

MAX_DIMS = len(_hip.TensorDesc().shape)


def tensor_descs(tensors, skip=()):
    """name -> tensor mapping -> ``(TensorDesc array, n, keep)``.  Non-floating tensors and the names in ``skip`` are left out;
    every other tensor is described as a detached CPU float32 contiguous copy.  ``keep`` holds those copies: the array only
    points into them, so the caller keeps ``keep`` alive across the ``create`` call.  A tensor of more than four dimensions does
    not fit ``TensorDesc.shape`` and raises ``ValueError`` (no engine takes one)."""
    keep, names = [], []
    for name, t in tensors.items():
        if name in skip or not t.is_floating_point():
            continue
        if t.dim() > MAX_DIMS:
            raise ValueError(f"{name}: {t.dim()} dimensions do not fit a TensorDesc ({MAX_DIMS})")
        keep.append(t.detach().to(device="cpu", dtype=torch.float32).contiguous())
        names.append(name)
    arr = (_hip.TensorDesc * len(keep))()
    for d, name, t in zip(arr, names, keep):
        d.name, d.data, d.ndim = name.encode(), t.data_ptr(), t.dim()
        for i, s in enumerate(t.shape):
            d.shape[i] = s
    return arr, len(keep), keep


class HipEngine:
    """Owns one handle of one ``nunif_hip_<net>_create`` on one device."""
    handle = None          # so that close() holds on an instance whose __init__ did not finish

    def __init__(self, device, tensors, create, destroy, *create_args, label, skip=()):
        """``create`` / ``destroy`` name the symbols; ``create`` is called as ``create(descs, n, *create_args, &handle)``."""
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise RuntimeError(f"the {label} HIP engine needs a ROCm device (model.to('cuda:N')); no CPU fallback")
        lib = _hip.lib()
        arr, n, keep = tensor_descs(tensors, skip)
        handle = ctypes.c_void_p()
        with torch.cuda.device(self.device):
            _hip.check(getattr(lib, create)(arr, n, *create_args, ctypes.byref(handle)))
        del keep           # create has copied the weights to the device
        self._destroy = getattr(lib, destroy)
        self.handle = handle

    def close(self):
        h, self.handle = self.handle, None
        if h:
            self._destroy(h)

    def __del__(self):
        self.close()

    def call(self, fn, *args):
        """``fn(*args, stream)`` on this engine's device and torch's current stream there; raises on a non-zero status."""
        with torch.cuda.device(self.device):
            _hip.check(fn(*args, _hip.current_stream_ptr(self.device)))


class FlatWeightsMixin:
    """``nn.Module`` surface of a model whose network runs in a :class:`HipEngine`: flat fp32 master weights under the reference's
    state-dict keys in ``_weights`` and one lazily built engine in ``_engine``.  A mixin (listed before the ``nn.Module`` base)
    because TransNetV2 and SuperPoint are plain modules.  Subclasses call ``_setup_weights`` and give ``_make_engine``."""

    def _setup_weights(self, weights):
        self.register_buffer("_device_probe", torch.empty(0), persistent=False)
        self._weights = weights
        self._engine = None

    def _make_engine(self, device):
        raise NotImplementedError

    def _param_filter(self, name, tensor):
        return tensor.is_floating_point()

    def get_device(self):
        return self._device_probe.device

    def state_dict(self, *args, **kwargs):
        return OrderedDict((k, v.clone()) for k, v in self._weights.items())

    def load_state_dict(self, state_dict, strict=True, **kwargs):
        missing = [k for k in self._weights if k not in state_dict]
        unexpected = [k for k in state_dict if k not in self._weights]
        if strict and (missing or unexpected):
            raise RuntimeError(f"Error(s) in loading state_dict for {type(self).__name__}: "
                               f"missing {missing[:4]}{'...' if len(missing) > 4 else ''}, "
                               f"unexpected {unexpected[:4]}{'...' if len(unexpected) > 4 else ''}")
        for k, old in self._weights.items():
            if k in state_dict:
                v = state_dict[k].detach().to("cpu")
                if v.shape != old.shape:
                    raise RuntimeError(f"size mismatch for {k}: {tuple(v.shape)} vs {tuple(old.shape)}")
                self._weights[k] = (v.float() if v.is_floating_point() else v).clone()
        self._drop_engine()
        return torch.nn.modules.module._IncompatibleKeys(missing, unexpected)

    def parameters(self, recurse=True):
        return iter(v for k, v in self._weights.items() if self._param_filter(k, v))

    def half(self):      # storage precision is the engine's business
        return self

    def float(self):
        return self

    def _drop_engine(self):
        e, self._engine = self._engine, None
        if e is not None:
            e.close()

    def engine(self):
        dev = self.get_device()
        if self._engine is None or self._engine.device != dev:
            self._drop_engine()
            self._engine = self._make_engine(dev)
        return self._engine

    def __deepcopy__(self, memo):
        """The engine holds a ctypes handle to device state (not copyable, and a shallow copy would free it twice): the copy gets
        its own weights and NO engine — it is rebuilt lazily on the first forward."""
        new = self.__class__.__new__(self.__class__)
        memo[id(self)] = new
        for k, v in self.__dict__.items():
            new.__dict__[k] = None if k == "_engine" else copy.deepcopy(v, memo)
        return new
