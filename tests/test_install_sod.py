"""``nunif_amd.install()`` over the LIVE reference, auto convergence: after ``install()`` the reference's
``iw3.convergence_estimator.ConvergenceEstimator`` is the engine's class and ``iw3.sod_v1`` / ``iw3.dsod_v1`` build the engine's
net; ``uninstall()`` restores the originals.  Nothing is computed."""
import inspect
import sys

import pytest

from oracle import refstub

pytestmark = pytest.mark.skipif(not refstub.reference_available(), reason="the reference checkout is not mounted here")

ENTRY = ("iw3.convergence_estimator", "ConvergenceEstimator")


@pytest.fixture()
def reference():
    refstub.install()
    import nunif_amd.install as inst
    if inst.is_installed():
        inst.uninstall()
    import iw3.convergence_estimator    # noqa: F401
    original = sys.modules[ENTRY[0]].ConvergenceEstimator
    yield inst, original
    if inst.is_installed():
        inst.uninstall()


def test_constructor_keeps_the_reference_parameters(reference):
    from nunif_amd.iw3.convergence_estimator import ConvergenceEstimator
    _, original = reference
    ref = list(inspect.signature(original.__init__).parameters.values())
    ours = list(inspect.signature(ConvergenceEstimator.__init__).parameters.values())
    assert ours[:len(ref)] == ref
    for name in ("reset", "depth_position_from_ratio", "__call__"):
        assert list(inspect.signature(getattr(original, name)).parameters) == \
            list(inspect.signature(getattr(ConvergenceEstimator, name)).parameters)


def test_install_rebinds_the_class_and_the_models_and_uninstall_restores(reference):
    inst, original = reference
    from nunif_amd.iw3.convergence_estimator import ConvergenceEstimator
    from nunif_amd.iw3.models.sod_v1 import SODV1
    assert ENTRY in inst.PATCHES
    report = inst.install()
    assert sys.modules[ENTRY[0]].ConvergenceEstimator is ConvergenceEstimator
    assert report["patched"]["iw3.convergence_estimator.ConvergenceEstimator"] >= 1
    assert "iw3.sod_v1" in report["models"] and "iw3.dsod_v1" in report["models"]
    from nunif.models import create_model
    assert isinstance(create_model("iw3.sod_v1"), SODV1) and isinstance(create_model("iw3.dsod_v1"), SODV1)
    inst.uninstall()
    assert sys.modules[ENTRY[0]].ConvergenceEstimator is original
