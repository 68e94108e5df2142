"""``nunif_amd.install()`` over the LIVE reference, the shot-boundary network: after ``install()`` the reference's
``nunif.utils.transnetv2.TransNetV2`` is the engine's class (so its own ``detect_boundary`` and ``nunif/cli/split_video.py`` build
it), ``uninstall()`` restores the original.  Nothing is computed."""
import inspect
import sys

import pytest

from oracle import refstub

pytestmark = pytest.mark.skipif(not refstub.reference_available(), reason="the reference checkout is not mounted here")

ENTRY = ("nunif.utils.transnetv2", "TransNetV2")


@pytest.fixture()
def reference():
    refstub.install()
    import nunif_amd.install as inst
    if inst.is_installed():
        inst.uninstall()
    import nunif.utils.transnetv2    # noqa: F401
    original = sys.modules[ENTRY[0]].TransNetV2
    yield inst, original
    if inst.is_installed():
        inst.uninstall()


def test_patches_hold_the_entry_and_not_the_pyav_module():
    import nunif_amd.install as inst
    assert ENTRY in inst.PATCHES
    assert not any(mod == "nunif.utils.shot_boundary_detection" for mod, _ in inst.PATCHES)


def test_constructor_signature_equals_the_live_reference(reference):
    from nunif_amd.nunif.utils.transnetv2 import TransNetV2
    _, original = reference
    assert inspect.signature(original.__init__) == inspect.signature(TransNetV2.__init__)


def test_install_rebinds_the_class_and_uninstall_restores_it(reference):
    inst, original = reference
    from nunif_amd.nunif.utils.transnetv2 import TransNetV2
    report = inst.install()
    assert sys.modules[ENTRY[0]].TransNetV2 is TransNetV2
    assert report["patched"]["nunif.utils.transnetv2.TransNetV2"] >= 1
    inst.uninstall()
    assert sys.modules[ENTRY[0]].TransNetV2 is original
