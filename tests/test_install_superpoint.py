"""``nunif_amd.install()`` over the LIVE reference, stlizer's names: after ``install()`` the reference's
``nunif.utils.superpoint.SuperPoint`` / ``find_match_index`` / ``apply_transform`` are the engine's (stlizer reaches them through
``import nunif.utils.superpoint as KU`` and ``KU.<name>``), ``find_transform`` stays the reference's, ``uninstall()`` restores the
originals.  Nothing is computed."""
import importlib
import inspect
import sys

import pytest

from oracle import refstub

MODULE = "nunif.utils.superpoint"
NAMES = ("SuperPoint", "find_match_index", "apply_transform")


def test_patches_hold_the_three_entries_and_not_the_pipeline_module():
    import nunif_amd.install as inst
    for name in NAMES:
        assert (MODULE, name) in inst.PATCHES
    assert (MODULE, "find_transform") not in inst.PATCHES
    assert not any(mod.startswith("stlizer") for mod, _ in inst.PATCHES)
    assert "stlizer" in inst._CONSUMER_ROOTS


def test_module_says_what_stays_the_references():
    import nunif_amd.nunif.utils.superpoint as ours
    assert not hasattr(ours, "find_transform") and not hasattr(ours, "cosine_annealing")
    assert "find_transform" in ours.__doc__


needs_reference = pytest.mark.skipif(not refstub.reference_available(), reason="the reference checkout is not mounted here")


@pytest.fixture()
def reference():
    refstub.install()
    import nunif_amd.install as inst
    if inst.is_installed():
        inst.uninstall()
    ref = importlib.import_module(MODULE)
    originals = {n: getattr(ref, n) for n in NAMES + ("find_transform",)}
    yield inst, ref, originals
    if inst.is_installed():
        inst.uninstall()


@needs_reference
def test_signatures_equal_the_live_reference(reference):
    import nunif_amd.nunif.utils.superpoint as ours
    _, ref, originals = reference
    for name in ("find_match_index", "apply_transform"):
        assert inspect.signature(inspect.unwrap(originals[name])) == inspect.signature(inspect.unwrap(getattr(ours, name))), name
    for name in ("sample_descriptors", "batched_nms", "select_top_k_keypoints"):
        assert inspect.signature(getattr(ref, name)) == inspect.signature(getattr(ours, name)), name
    for method in ("__init__", "forward", "load", "infer"):
        assert (inspect.signature(inspect.unwrap(getattr(originals["SuperPoint"], method)))
                == inspect.signature(inspect.unwrap(getattr(ours.SuperPoint, method)))), method
    assert ours.SuperPoint.default_conf == originals["SuperPoint"].default_conf


@needs_reference
def test_install_rebinds_ku_access_and_uninstall_restores_it(reference):
    inst, ref, originals = reference
    import nunif_amd.nunif.utils.superpoint as ours
    report = inst.install()
    import nunif.utils.superpoint as KU                 # the import form of stlizer/multipass_pipeline.py
    for name in NAMES:
        assert getattr(KU, name) is getattr(ours, name), name
        assert report["patched"][f"{MODULE}.{name}"] >= 1
    assert KU.find_transform is originals["find_transform"]
    assert KU.SuperPoint(detection_threshold=0.01).conf.detection_threshold == 0.01
    inst.uninstall()
    for name in NAMES:
        assert getattr(sys.modules[MODULE], name) is originals[name], name


def test_host_tensors_raise_without_install():
    import torch
    import nunif_amd.install as inst
    import nunif_amd.nunif.utils.superpoint as ours
    if inst.is_installed():
        inst.uninstall()
    d = {"descriptors": torch.eye(4, 8)}
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ours.find_match_index(d, d)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ours.apply_transform(torch.zeros(1, 4, 4), [0, 0], 1.0, 0.0, [2, 2])


@needs_reference
def test_host_tensors_go_to_the_references_own_function_while_installed(reference):
    """stlizer with ``--gpu -1``: the re-bound names keep the reference's CPU path."""
    import torch
    inst, ref, originals = reference
    g = torch.Generator().manual_seed(1)
    d1 = {"descriptors": torch.nn.functional.normalize(torch.randn(5, 16, generator=g), dim=1)}
    d2 = {"descriptors": torch.cat([d1["descriptors"][[3, 1]], torch.nn.functional.normalize(torch.randn(4, 16, generator=g), dim=1)])}
    x = torch.rand(3, 9, 11, generator=g)
    want_m = originals["find_match_index"](d1, d2, return_score_all=True)
    want_w = originals["apply_transform"](x, [1.5, -0.5], 1.0, 3.0, [5, 4], padding_mode="reflection")
    inst.install()
    import nunif.utils.superpoint as KU
    got_m = KU.find_match_index(d1, d2, return_score_all=True)
    assert all(torch.equal(a, b) for a, b in zip(got_m, want_m))
    assert torch.equal(KU.apply_transform(x, [1.5, -0.5], 1.0, 3.0, [5, 4], padding_mode="reflection"), want_w)
