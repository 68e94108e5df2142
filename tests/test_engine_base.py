"""nunif_amd/engine.py on the CPU: ``tensor_descs`` read back through its pointers, the ``HipEngine`` handle lifecycle against a
stand-in library that counts ``create`` / ``destroy``, and the ``FlatWeightsMixin`` surface of every engine-backed model class."""
import contextlib
import copy
import ctypes
import gc
import importlib
import sys

import pytest
import torch

from nunif_amd import _hip, engine
from nunif_amd.engine import FlatWeightsMixin, HipEngine, tensor_descs

pytestmark = pytest.mark.filterwarnings("error::pytest.PytestUnraisableExceptionWarning")

# the classes the models were moved from (each had its own copy of the surface); the registry must still lead to all of them
LISTED = {"SwinUNet", "SwinUNet2x", "SwinUNet4x", "SwinUNet8x", "SwinUNet1xV2", "SwinUNet2xV2", "SwinUNet4xV2", "VGG7", "UpConv7",
          "CUNet", "UpCUNet", "RowFlowV3", "MLBW", "LightInpaintV1", "LightVideoInpaintV1", "DepthAA", "SODV1", "TransNetV2",
          "SuperPoint"}


def _engine_backed_classes():
    for mod in ("waifu2x.models.swin_unet", "waifu2x.models.swin_unet_v2", "waifu2x.models.cunet", "waifu2x.models.vgg_7",
                "iw3.models"):
        importlib.import_module("nunif_amd." + mod)
    from nunif_amd.nunif.models.register import _models
    from nunif_amd.nunif.utils.superpoint import SuperPoint
    from nunif_amd.nunif.utils.transnetv2 import TransNetV2
    found = {c for c in _models.values() if isinstance(c, type) and issubclass(c, FlatWeightsMixin)} | {TransNetV2, SuperPoint}
    return sorted(found, key=lambda c: c.__name__)


CLASSES = _engine_backed_classes()


def test_every_listed_class_is_covered():
    assert LISTED <= {c.__name__ for c in CLASSES}


@contextlib.contextmanager
def no_unraisable():
    """Fails when a ``__del__`` inside the block (or at the collection that ends it) leaves an "Exception ignored"."""
    seen, old = [], sys.unraisablehook
    sys.unraisablehook = seen.append
    try:
        yield
        gc.collect()
    finally:
        sys.unraisablehook = old
    assert not seen, [repr(u.exc_value) for u in seen]


# ---- tensor_descs -----------------------------------------------------------------------------------------------------------

def read_descs(arr, n):
    out = {}
    for d in arr[:n]:
        shape = tuple(d.shape[:d.ndim])
        numel = 1
        for s in shape:
            numel *= s
        out[d.name.decode()] = (shape, ctypes.cast(d.data, ctypes.POINTER(ctypes.c_float))[:numel])
    return out


def test_tensor_descs_describe_cpu_fp32_contiguous_copies():
    g = torch.Generator().manual_seed(1)
    tensors = {"half": torch.randn(2, 3, generator=g).half(),
               "strided": torch.randn(5, 4, 3, generator=g).permute(2, 0, 1)[:, ::2],
               "scalar": torch.tensor(1.5),
               "four": torch.randn(2, 1, 3, 2, generator=g, dtype=torch.float64),
               "index": torch.arange(6),
               "left_out": torch.randn(3, generator=g)}
    assert not tensors["strided"].is_contiguous()
    arr, n, keep = tensor_descs(tensors, skip=("left_out",))
    gc.collect()                                    # the names and the data must outlive everything but arr and keep
    got = read_descs(arr, n)
    assert n == len(arr) == len(keep) == 4 and list(got) == ["half", "strided", "scalar", "four"]
    for name, (shape, values) in got.items():
        t = tensors[name]
        assert shape == tuple(t.shape)
        assert values == t.float().contiguous().reshape(-1).tolist()
    assert got["scalar"] == ((), [1.5])
    assert all(t.dtype == torch.float32 and t.is_contiguous() and t.device.type == "cpu" for t in keep)


def test_tensor_descs_refuse_more_dims_than_a_desc_holds():
    assert tensor_descs({"w": torch.zeros(1, 2, 3, 4)})[1] == 1
    with pytest.raises(ValueError, match="5 dimensions"):
        tensor_descs({"w": torch.zeros(1, 2, 3, 4, 5)})
    tensor_descs({"w": torch.zeros(1, 2, 3, 4, 5)}, skip=("w",))
    tensor_descs({"i": torch.zeros(1, 2, 3, 4, 5, dtype=torch.int64)})


def test_depth_anything_checkpoints_fit_a_desc():
    """``HipDepthAnythingV2`` used to cut shapes at four dimensions silently; nothing it is handed has more."""
    from nunif_amd.synthetic import depth_anything_v2_state_dict
    from oracle import depth_anything_v2 as ODA
    from oracle import video_depth_anything_net as OV
    sds = [ODA.random_state_dict(601), depth_anything_v2_state_dict(601), OV.random_state_dict(7)]
    for sd in sds:
        assert max(t.dim() for k, t in sd.items() if k != "pretrained.pos_embed") <= engine.MAX_DIMS == 4


# ---- HipEngine --------------------------------------------------------------------------------------------------------------

class StandInLib:
    """``create`` / ``destroy`` of any engine: counts the calls and records what ``create`` was handed."""

    def __init__(self, status=0):
        self.status, self.created, self.destroyed = status, [], []

    def nunif_hip_last_error(self):
        return b"stand-in failure"

    def __getattr__(self, name):
        if name.endswith("_destroy"):
            return lambda h: self.destroyed.append(h.value)
        if name.endswith(("_create", "_create_ex")):
            return lambda arr, n, *rest: self._create(name, arr, n, *rest)
        raise AttributeError(name)

    def _create(self, name, arr, n, *rest):
        self.created.append((name, read_descs(arr, n), rest[:-1]))
        if self.status == 0:
            rest[-1]._obj.value = 0x1000 + len(self.created)
        return self.status


@pytest.fixture
def standin(monkeypatch):
    lib = StandInLib()
    monkeypatch.setattr(_hip, "lib", lambda: lib)
    monkeypatch.setattr(torch.cuda, "device", contextlib.nullcontext)          # the device guard needs a GPU to enter
    return lib


def test_engine_refuses_a_cpu_device(standin):
    with no_unraisable():
        with pytest.raises(RuntimeError, match=r"the swin_unet HIP engine needs a ROCm device .*no CPU fallback"):
            HipEngine("cpu", {"w": torch.zeros(2)}, "x_create", "x_destroy", label="swin_unet")
    assert not standin.created and not standin.destroyed


def test_engine_creates_once_and_destroys_once(standin):
    w = torch.arange(6.0).reshape(2, 3)
    with no_unraisable():
        e = HipEngine("cuda:0", {"w": w, "i": torch.arange(3)}, "x_create", "x_destroy", 7, 2.5, label="x")
        assert e.device == torch.device("cuda:0") and e.handle.value == 0x1001
        assert standin.created == [("x_create", {"w": ((2, 3), w.reshape(-1).tolist())}, (7, 2.5))]
        e.close()
        assert e.handle is None and standin.destroyed == [0x1001]
        e.close()
        del e
    assert standin.destroyed == [0x1001]
    with no_unraisable():
        e = HipEngine("cuda:0", {"w": w}, "x_create", "x_destroy", label="x")
        del e                                        # never closed by hand: __del__ does it
    assert standin.destroyed == [0x1001, 0x1002]


def test_engine_whose_create_failed_destroys_nothing(standin):
    standin.status = 3
    with no_unraisable():
        with pytest.raises(_hip.NunifHipError, match="stand-in failure"):
            HipEngine("cuda:0", {"w": torch.zeros(2)}, "x_create", "x_destroy", label="x")
        HipEngine.__new__(HipEngine).close()         # an instance whose __init__ never ran
    assert len(standin.created) == 1 and not standin.destroyed


# ---- FlatWeightsMixin, class by class ---------------------------------------------------------------------------------------

class StubEngine:
    def __init__(self, device=torch.device("cpu")):
        self.device, self.closed = device, 0

    def close(self):
        self.closed += 1


def _changed(v, g):
    return torch.randn(v.shape, generator=g) if v.is_floating_point() else v + 1


@pytest.mark.parametrize("cls", CLASSES, ids=lambda c: c.__name__)
def test_state_dict_surface(cls):
    m = cls()
    sd = m.state_dict()
    assert list(sd) == list(m._weights) and len(sd) > 5
    # every model creates its floating weights as fp32: what made the three earlier dtype rules of load_state_dict agree
    assert all(v.dtype == torch.float32 for v in sd.values() if v.is_floating_point())
    g = torch.Generator().manual_seed(5)
    new = {k: _changed(v, g) for k, v in sd.items()}
    r = m.load_state_dict(new)
    assert not r.missing_keys and not r.unexpected_keys
    back = m.state_dict()
    assert list(back) == list(new)
    assert all(back[k].dtype == new[k].dtype and torch.equal(back[k], new[k]) for k in new)
    k0 = next(k for k, v in sd.items() if v.is_floating_point() and v.dim() > 0)
    back[k0].zero_()                                 # state_dict hands out copies,
    new[k0].zero_()                                  # and load_state_dict took one
    assert m._weights[k0].abs().sum() > 0
    m.load_state_dict({k: v.half() if v.is_floating_point() else v for k, v in sd.items()})
    assert all(m._weights[k].dtype == v.dtype and torch.equal(m._weights[k], v.half().float() if v.is_floating_point() else v)
               for k, v in sd.items())

    few = dict(list(sd.items())[5:])
    with pytest.raises(RuntimeError, match=rf"loading state_dict for {cls.__name__}: missing \[.*\]\.\.\., unexpected \[\]"):
        m.load_state_dict(few)
    with pytest.raises(RuntimeError, match=r"unexpected \['bogus'\]"):
        m.load_state_dict({**sd, "bogus": torch.zeros(1)})
    r = m.load_state_dict({**few, "bogus": torch.zeros(1)}, strict=False)
    assert r.missing_keys == list(sd)[:5] and r.unexpected_keys == ["bogus"]
    with pytest.raises(RuntimeError, match=f"size mismatch for {k0}"):
        m.load_state_dict({**sd, k0: torch.zeros(tuple(sd[k0].shape) + (2,))})

    params = list(m.parameters())
    assert params and all(p.is_floating_point() for p in params)
    if cls.__name__ == "SODV1":
        running = {v.data_ptr() for k, v in m._weights.items() if "running_" in k}
        assert running and not running & {p.data_ptr() for p in params}
    assert m.half() is m and m.float() is m


@pytest.mark.parametrize("cls", CLASSES, ids=lambda c: c.__name__)
def test_copies_and_reloads_leave_the_engine_behind(cls):
    with no_unraisable():
        m = cls()
        for training in (True, False):
            m.train(training)
            stub = m._engine = StubEngine()
            c = copy.deepcopy(m)
            assert type(c) is cls and c is not m and c._engine is None and m._engine is stub and stub.closed == 0
            assert c.training == m.training == training
            assert list(c._weights) == list(m._weights)
            assert all(torch.equal(c._weights[k], v) and c._weights[k].data_ptr() != v.data_ptr() for k, v in m._weights.items()
                       if v.numel())
            m.load_state_dict(m.state_dict())
            assert stub.closed == 1 and m._engine is None
            del c
        # one engine per device, built lazily; the old one is closed before the next is built
        built = []
        m._make_engine = lambda device: built.append(StubEngine(device)) or built[-1]
        assert m.engine() is m.engine() is built[0] and len(built) == 1 and built[0].device == m.get_device()
        m.to("meta")
        assert m.engine() is built[1] and built[1].device.type == "meta" and (built[0].closed, built[1].closed) == (1, 0)
        del m


def test_a_refused_constructor_leaves_nothing_to_clean_up():
    from nunif_amd.nunif.utils.superpoint import SuperPoint
    from nunif_amd.nunif.utils.transnetv2 import TransNetV2
    with no_unraisable():
        with pytest.raises(NotImplementedError):
            TransNetV2(use_mean_pooling=True)
        with pytest.raises(NotImplementedError):
            SuperPoint(descriptor_dim=128)


def test_downscaled_wrappers_delegate_to_their_net():
    from nunif_amd.waifu2x.models.swin_unet import SwinUNet4x
    from nunif_amd.waifu2x.models.swin_unet_v2 import SwinUNet4xV2
    for net in (SwinUNet4x(), SwinUNet4xV2()):
        w = net.to_2x()
        stub = net._engine = StubEngine()
        with no_unraisable():
            c = copy.deepcopy(w)
        assert c.net4x is not net and c.net4x._engine is None and net._engine is stub
        sd = w.state_dict()
        assert list(sd) == list(net._weights)
        w.load_state_dict(sd)
        assert stub.closed == 1 and net._engine is None
