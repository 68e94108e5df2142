"""``nunif_amd.install()`` over the LIVE reference, stlizer's outpaint model: after ``install()`` the reference's
``create_model("stlizer.light_outpaint_v1")`` / ``load_model`` build the engine's class from the same ``.pth``, a checkpoint
round-trips both ways, ``uninstall()`` restores the reference's factory.  Nothing is computed."""
import inspect

import pytest
import torch

from oracle import refstub

NAME = "stlizer.light_outpaint_v1"
needs_reference = pytest.mark.skipif(not refstub.reference_available(), reason="the reference checkout is not mounted here")


def test_model_modules_hold_the_stlizer_entry():
    import nunif_amd.install as inst
    assert ("stlizer.models", ["nunif_amd.stlizer.models"]) in inst._MODEL_MODULES
    assert not any(mod.startswith("stlizer") for mod, _ in inst.PATCHES)
    import nunif_amd.stlizer.models  # noqa: F401
    from nunif_amd.nunif.models.register import _models
    from nunif_amd.stlizer.models import LightOutpaintV1
    assert _models[NAME] is LightOutpaintV1


@pytest.fixture()
def reference():
    refstub.install()
    import nunif_amd.install as inst
    if inst.is_installed():
        inst.uninstall()
    yield inst
    if inst.is_installed():
        inst.uninstall()


@needs_reference
def test_signatures_equal_the_live_reference(reference):
    from stlizer.models.light_outpaint_v1 import LightOutpaintV1 as Ref
    from nunif_amd.stlizer.models import LightOutpaintV1
    for method in ("__init__", "forward", "infer"):
        assert inspect.signature(getattr(Ref, method)) == inspect.signature(getattr(LightOutpaintV1, method)), method


@needs_reference
def test_install_swaps_the_registry_entry_and_a_checkpoint_round_trips(reference, tmp_path):
    inst = reference
    import stlizer.models  # noqa: F401
    from nunif.models import create_model, load_model, save_model
    from stlizer.models.light_outpaint_v1 import LightOutpaintV1 as Ref
    from nunif_amd.stlizer.models import LightOutpaintV1
    from nunif_amd.synthetic import light_outpaint_state_dict
    sd = light_outpaint_state_dict(3)
    ref = create_model(NAME)
    assert type(ref) is Ref
    ref.load_state_dict(sd)
    from_ref = str(tmp_path / "from_reference.pth")
    save_model(ref, from_ref)

    report = inst.install()
    assert NAME in report["models"]
    ours = create_model(NAME)
    assert type(ours) is LightOutpaintV1
    loaded, _ = load_model(from_ref, device_ids=[-1])               # the call of stlizer/multipass_pipeline.py:380
    assert type(loaded) is LightOutpaintV1
    back = loaded.state_dict()
    assert list(back) == list(sd) and all(torch.equal(back[k], sd[k]) for k in sd)
    from_engine = str(tmp_path / "from_engine.pth")
    from nunif_amd.nunif.models.utils import save_model as engine_save_model
    engine_save_model(loaded, from_engine)                          # the engine's own writer, the reference's file format

    inst.uninstall()
    assert type(create_model(NAME)) is Ref
    again, _ = load_model(from_engine, device_ids=[-1])
    assert type(again) is Ref
    rsd = again.state_dict()
    assert list(rsd) == list(sd) and all(torch.equal(rsd[k], sd[k]) for k in sd)
