"""``nunif_amd.install()`` over the LIVE reference, ``sbs.row_flow_v2``: the reference knows the name, so after ``install()`` its
registry builds the engine's class (and ``load_model`` of a v2 ``.pth`` with it); ``uninstall()`` restores the reference's own
factory.  Nothing is computed."""
import pytest

from oracle import refstub

pytestmark = pytest.mark.skipif(not refstub.reference_available(), reason="the reference checkout is not mounted here")


@pytest.fixture()
def inst():
    refstub.install()
    import nunif_amd.install as inst
    if inst.is_installed():
        inst.uninstall()
    import iw3.models    # noqa: F401
    yield inst
    if inst.is_installed():
        inst.uninstall()


def test_install_builds_the_engine_class_and_uninstall_restores(inst, tmp_path):
    from iw3.models.row_flow_v2 import RowFlowV2 as Ref
    from nunif.models import create_model, load_model, save_model
    from nunif_amd.iw3.models.row_flow_v2 import RowFlowV2
    from nunif_amd.synthetic import row_flow_v2_state_dict
    assert isinstance(create_model("sbs.row_flow_v2"), Ref)
    ref = Ref().eval()
    ref.load_state_dict(row_flow_v2_state_dict(301), strict=True)
    path = str(tmp_path / "iw3_row_flow_v2_20240130.pth")
    save_model(ref, path)
    report = inst.install()
    assert "sbs.row_flow_v2" in report["models"]
    assert isinstance(create_model("sbs.row_flow_v2"), RowFlowV2)
    m, _ = load_model(path, weights_only=True)
    assert isinstance(m, RowFlowV2) and all(bool((m.state_dict()[k] == v).all()) for k, v in ref.state_dict().items())
    inst.uninstall()
    assert isinstance(create_model("sbs.row_flow_v2"), Ref)
