"""The public names of nunif_amd/stlizer/pass3.py against the LIVE reference's ``stlizer.multipass_pipeline``: the same parameters
in the same order with the same defaults.  ``pass3`` alone has one more, the keyword ``host=False`` at the end.

``nunif_amd.install()`` does not bind these names (tests/test_install_outpaint.py and tests/test_install_superpoint.py pin that its
table holds no ``stlizer`` module), so there is no rebinding to test here."""
import inspect

import pytest

from oracle import refstub

needs_reference = pytest.mark.skipif(not refstub.reference_available(), reason="the reference checkout is not mounted here")
SAME = ("calc_scene_weight", "gen_smoothing_kernel", "conv1d_smoothing", "grad_opt", "pass3_smoothing")


@pytest.fixture(scope="module")
def reference():
    refstub.install()
    import stlizer.multipass_pipeline as MP
    return MP


@needs_reference
@pytest.mark.parametrize("name", SAME)
def test_signature_equals_the_live_references(reference, name):
    from nunif_amd.stlizer import pass3 as P
    assert inspect.signature(getattr(P, name)) == inspect.signature(getattr(reference, name))


@needs_reference
def test_pass3_adds_only_the_host_keyword(reference):
    from nunif_amd.stlizer import pass3 as P
    ours = list(inspect.signature(P.pass3).parameters.values())
    assert ours[:-1] == list(inspect.signature(reference.pass3).parameters.values())
    assert ours[-1].name == "host" and ours[-1].default is False


def test_install_leaves_pass3_to_the_reference():
    import nunif_amd.install as inst
    assert not any(mod.startswith("stlizer") for mod, _ in inst.PATCHES)
