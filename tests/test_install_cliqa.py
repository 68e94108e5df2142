"""``nunif_amd.install()`` over the LIVE reference, cliqa's models: with ``cliqa.models`` loaded the reference's ``create_model`` /
``load_model`` build the engine's classes from the same ``.pth``; without it the registry gains no name; ``uninstall()`` restores.
Nothing is computed."""
import sys

import pytest
import torch

from oracle import refstub

NAMES = ("cliqa.jpeg_quality", "cliqa.grain_noise_level", "cliqa.scale_factor")
needs_reference = pytest.mark.skipif(not refstub.reference_available(), reason="the reference checkout is not mounted here")


def test_install_tables_hold_the_cliqa_entry():
    import nunif_amd.install as inst
    assert ("cliqa.models", ["nunif_amd.cliqa.models"]) in inst._MODEL_MODULES
    assert "cliqa.models" in inst._ONLY_IF_LOADED and "cliqa" in inst._CONSUMER_ROOTS
    assert not any(mod.startswith("cliqa") for mod, _ in inst.PATCHES)       # cliqa.utils imports torchvision
    import nunif_amd.cliqa.models as M
    from nunif_amd.nunif.models.register import _models
    assert [_models[n] for n in NAMES] == [M.JPEGQuality, M.GrainNoiseLevel, M.ScaleFactor]


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
def test_install_swaps_the_registry_entries_and_a_checkpoint_loads(reference, tmp_path):
    inst = reference
    import cliqa.models as RM
    from nunif.models import create_model, get_model_device, load_model, save_model
    import nunif_amd.cliqa.models as M
    from nunif_amd.synthetic import cliqa_state_dict
    sd = cliqa_state_dict(5, "scale_factor")
    ref = create_model("cliqa.scale_factor")
    assert type(ref) is RM.ScaleFactor
    ref.load_state_dict(sd)
    path = str(tmp_path / "scale_factor.pth")
    save_model(ref, path)

    report = inst.install()
    assert all(n in report["models"] for n in NAMES)
    assert [type(create_model(n)) for n in NAMES] == [M.JPEGQuality, M.GrainNoiseLevel, M.ScaleFactor]
    loaded, _ = load_model(path, device_ids=[-1])                    # the call of cliqa/filter_low_quality_resize.py
    assert type(loaded) is M.ScaleFactor
    back = loaded.state_dict()
    assert list(back) == list(sd) and all(torch.equal(back[k], sd[k]) for k in sd)
    assert get_model_device(loaded) == torch.device("cpu")            # predict_* reach the model through this and forward

    inst.uninstall()
    assert [type(create_model(n)) for n in NAMES] == [RM.JPEGQuality, RM.GrainNoiseLevel, RM.ScaleFactor]


@needs_reference
def test_without_cliqa_loaded_the_registry_gains_no_name(reference):
    inst = reference
    saved = {k: sys.modules.pop(k) for k in list(sys.modules) if k == "cliqa" or k.startswith("cliqa.")}
    import nunif.models.register as reg
    names = {n: reg._models.pop(n) for n in NAMES if n in reg._models}
    try:
        report = inst.install()
        assert not any(n in report["models"] for n in NAMES)
        assert not any(n in reg._models for n in NAMES)
        assert "cliqa.models" not in sys.modules
        inst.uninstall()
    finally:
        reg._models.update(names)
        sys.modules.update(saved)
