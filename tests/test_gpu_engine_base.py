"""The engine lifecycle of nunif_amd/engine.py on the device, on one representative of each way a model used to own its handle:
VGG7 (an engine object shared with cunet), TransNetV2 (a plain ``nn.Module`` that held a raw handle and packs its weights) and
DepthAA (a registered model that held a raw handle).  Outputs are compared bit for bit between two engines built from the same
weights: both run the same kernels on the same device, so any difference is a difference in what ``create`` was handed."""
import copy
import gc
import os
import weakref

import numpy as np
import pytest
import torch

from conftest import GOLDEN
from test_engine_base import no_unraisable

pytestmark = pytest.mark.gpu


def _vgg7():
    from nunif_amd.waifu2x.models.vgg_7 import VGG7
    m = VGG7()
    sd = m.state_dict()
    sd["net.12.bias"].fill_(0.5)                     # mid-range output: the eval clamp to [0, 1] hides nothing
    x = torch.rand(1, 3, 32, 32, generator=torch.Generator().manual_seed(11))
    return m, sd, "net.12.bias", x, lambda model, inp: [model(inp)]


def _transnetv2():
    from nunif_amd.nunif.utils.transnetv2 import TransNetV2
    from nunif_amd.synthetic import transnetv2_state_dict
    x = torch.rand(1, 4, 3, 27, 48, generator=torch.Generator().manual_seed(12)) * 255

    def run(model, inp):
        one_hot, extra = model(inp)
        return [one_hot, extra["many_hot"]]
    return TransNetV2(), transnetv2_state_dict(3), "cls_layer1.bias", x, run


def _depth_aa():
    from nunif_amd.iw3.models import DepthAA
    from oracle import depth_aa as ODA
    x = torch.from_numpy(np.load(os.path.join(GOLDEN, "depth_aa.npz"))["x"])[1:2]
    # (a fresh DepthAA has a zero proj_out and passes its input through whatever the other weights are: seeded weights instead)
    return DepthAA(), ODA.random_state_dict(501), "proj_out.bias", x, lambda model, inp: [model(inp, clamp=False)]


@pytest.mark.parametrize("case", [_vgg7, _transnetv2, _depth_aa], ids=["vgg7", "transnetv2", "depth_aa"])
def test_copy_reload_and_delete(hiplib, case):
    with no_unraisable():
        m, sd, key, x, run = case()
        m.load_state_dict(sd)
        m = m.eval().to("cuda")
        x = x.to("cuda")
        y = run(m, x)
        assert all(torch.isfinite(t).all() for t in y)

        c = copy.deepcopy(m)
        assert c._engine is None and m._engine is not None
        c = c.to("cuda")
        yc = run(c, x)
        assert all(torch.equal(a, b) for a, b in zip(y, yc))
        assert m.engine().handle.value != c.engine().handle.value and m.engine().device == c.engine().device

        old = m.engine()
        sd2 = dict(sd)
        sd2[key] = sd[key] + 0.125
        m.load_state_dict(sd2)
        assert m._engine is None and old.handle is None              # closed at once, not when the last reference goes
        del old
        y2 = run(m, x)
        assert not torch.equal(y[0], y2[0])                         # the engine was rebuilt from the new weights
        assert all(torch.equal(a, b) for a, b in zip(yc, run(c, x)))      # the copy kept its own

        engines = [weakref.ref(m.engine()), weakref.ref(c.engine())]
        del m, c
        gc.collect()
        assert all(e() is None for e in engines)
        torch.cuda.synchronize()
