"""``nunif_amd.install()`` and iw3.desktop's frame encoder: ``iw3.desktop.utils.to_jpeg_data`` is rebound only in a process that
has loaded that module (the reference's imports wx and torchvision.io, which this suite cannot import: a stand-in module object
takes its place), ``uninstall()`` restores it, and a process without the module gets the report it got before."""
import inspect
import sys
import types

import pytest

from oracle import refstub

pytestmark = pytest.mark.skipif(not refstub.reference_available(), reason="/root/reference is not mounted here")
NAME = "iw3.desktop.utils"


@pytest.fixture()
def inst():
    refstub.install()
    import nunif_amd.install as inst
    if inst.is_installed():
        inst.uninstall()
    saved = sys.modules.pop(NAME, None)
    yield inst
    inst.uninstall()
    sys.modules.pop(NAME, None)
    if saved is not None:
        sys.modules[NAME] = saved


def test_entry_and_signature(inst):
    import nunif_amd.iw3.desktop.utils as ours
    assert (NAME, "to_jpeg_data") in inst.PATCHES and NAME in inst._PATCH_ONLY_IF_LOADED
    assert list(inspect.signature(ours.to_jpeg_data).parameters) == ["frame", "quality", "tick", "gpu_jpeg"]
    assert inspect.signature(ours.to_jpeg_data).parameters["gpu_jpeg"].default is True
    assert list(inspect.signature(ours.to_uint8).parameters) == ["x"]


def test_without_the_module_the_report_is_unchanged(inst):
    report = inst.install()
    assert NAME not in sys.modules                               # install() did not import it
    assert not any(k.startswith("iw3.desktop") for k in report["patched"])
    assert not any(str(k).startswith("iw3.desktop") for k, _ in report["skipped"])
    expected = {f"{m}.{a}" for m, a in inst.PATCHES if m not in inst._PATCH_ONLY_IF_LOADED}
    assert set(report["patched"]) == expected
    inst.uninstall()
    assert inst.install(strict=True)["patched"].keys() == report["patched"].keys()


def test_a_loaded_module_is_rebound_and_restored(inst):
    import nunif_amd.iw3.desktop.utils as ours

    def reference_to_jpeg_data(frame, quality, tick, gpu_jpeg=True):
        raise AssertionError("the reference's encoder must not run while installed")

    stand_in = types.ModuleType(NAME)
    stand_in.to_jpeg_data = reference_to_jpeg_data
    stand_in.to_uint8 = lambda x: x
    sys.modules[NAME] = stand_in
    report = inst.install()
    assert report["patched"][NAME + ".to_jpeg_data"] == 1
    assert stand_in.to_jpeg_data is ours.to_jpeg_data
    assert inst.original(NAME, "to_jpeg_data") is reference_to_jpeg_data
    inst.uninstall()
    assert stand_in.to_jpeg_data is reference_to_jpeg_data
