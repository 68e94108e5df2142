"""``nunif_amd.install()`` and ``waifu2x.wgmlp_4x``: under install the reference's registry resolves the name to the engine class, and
``uninstall()`` puts the reference's own class back."""
import sys

import pytest


def test_install_resolves_wgmlp_to_the_engine_and_uninstall_restores():
    from oracle import refstub
    if not refstub.reference_available():
        pytest.skip("needs the reference tree")
    refstub.install()
    import nunif_amd
    from nunif_amd import install as inst
    import waifu2x.models  # noqa: F401  (the reference registers its own WGMLP4x)
    registry = sys.modules["nunif.models.register"]._models
    original = registry["waifu2x.wgmlp_4x"]
    assert original.__module__ == "waifu2x.models.wgmlp"
    report = inst.install()
    try:
        assert "waifu2x.wgmlp_4x" in report["models"]
        from nunif.models import create_model
        m = create_model("waifu2x.wgmlp_4x")
        assert type(m).__module__ == "nunif_amd.waifu2x.models.wgmlp" and (m.i2i_scale, m.i2i_offset, m.i2i_blend_size) == (4, 36, 16)
    finally:
        inst.uninstall()
    assert registry["waifu2x.wgmlp_4x"] is original
    assert nunif_amd is not None
