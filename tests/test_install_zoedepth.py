"""``nunif_amd.install()`` over the LIVE reference, ``--depth-model ZoeD_Any_N / ZoeD_Any_K``: after ``install()`` the reference's
``iw3.depth_model_factory.create_depth_model`` (and every ``from`` copy of it) resolves the two names — ``ZoeD_Any_N`` is the CLI's
default — to the engine's ``ZoeDepthModel``, the BEiT names still raise ``ValueError`` through the patched module, and
``uninstall()`` restores the original.  Nothing is computed."""
import sys

import pytest

from oracle import refstub

pytestmark = pytest.mark.skipif(not refstub.reference_available(), reason="the reference checkout is not mounted here")

ENTRY = ("iw3.depth_model_factory", "create_depth_model")


@pytest.fixture()
def reference():
    refstub.install()
    import nunif_amd.install as inst
    if inst.is_installed():
        inst.uninstall()
    import iw3.depth_model_factory    # noqa: F401
    original = sys.modules[ENTRY[0]].create_depth_model
    yield inst, original
    if inst.is_installed():
        inst.uninstall()


def test_install_routes_the_two_names_and_uninstall_restores(reference, tmp_path, monkeypatch):
    inst, original = reference
    from nunif_amd.iw3.zoedepth_model import ZoeDepthModel
    monkeypatch.setattr(ZoeDepthModel, "model_dir", str(tmp_path))
    assert ENTRY in inst.PATCHES
    report = inst.install(strict=False)
    assert report["patched"]["iw3.depth_model_factory.create_depth_model"] >= 1
    ref_factory = sys.modules[ENTRY[0]].create_depth_model
    assert ref_factory is not original
    for name in ("ZoeD_Any_N", "ZoeD_Any_K"):
        m = ref_factory(name)
        assert isinstance(m, ZoeDepthModel) and m.is_metric() and m.get_name() == "ZoeDepth"
        assert not ZoeDepthModel.has_checkpoint_file(name)
        with pytest.raises(FileNotFoundError):
            m.load_model(name, device="cuda:0")
    for name in ("ZoeD_N", "ZoeD_K", "ZoeD_NK"):
        with pytest.raises(ValueError):
            ref_factory(name)
    inst.uninstall()
    assert sys.modules[ENTRY[0]].create_depth_model is original


def test_the_reference_cli_default_is_one_of_the_two_names(reference):
    """``iw3/utils.py`` ``create_parser``: ``--depth-model`` defaults to ``ZoeD_Any_N`` (read from the source: the module imports
    PyAV and wx-free GUI helpers that need not be importable here)."""
    import os
    import re
    text = open(os.path.join(refstub.REFERENCE_ROOT, "iw3", "utils.py")).read()
    m = re.search(r'"--depth-model".*?default="([A-Za-z0-9_]+)"', text, flags=re.S)
    from nunif_amd.iw3.zoedepth_model import ZoeDepthModel
    assert m and ZoeDepthModel.supported(m.group(1)), m and m.group(1)
