"""sbs.row_flow_v2 without a GPU: the restatement (tests/row_flow_v2_ref.py) against the reference fixture, the clamped form
against the padded form, the model surface (keys, attributes, .pth round trip, refusals, factory, method name), and the
localised check of tests/test_gpu_row_flow_v2.py against kernel-shaped mutations of the restatement (the fp16 emulation stands in
for the kernel, after tests/test_errloc_sidenet.py)."""
import os
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import errloc as E
import row_flow_v2_ref as V
import sidenet_cases as S
from conftest import GOLDEN, sd_checksum
from oracle import refstub
from oracle import row_flow_v3 as ORF
from oracle.forward_warp import synth_depth

from nunif_amd.synthetic import row_flow_v2_state_dict


@pytest.fixture(scope="module")
def g():
    return {k: torch.from_numpy(v) for k, v in np.load(os.path.join(GOLDEN, "row_flow_v2.npz")).items()}


@pytest.fixture(scope="module")
def sd():
    return row_flow_v2_state_dict(V.WEIGHT_SEED)


def _planes(b, h, w, seed=3):
    return ORF.make_input(synth_depth(seed, b, h, w, "smooth_edges"), 2.0, 0.5, 104)


def test_fp32_restatement_matches_reference_fixture(g, sd):
    assert sd_checksum(sd) == pytest.approx(float(g["sdsum"]), rel=1e-12)
    depth, c = V.fixture_inputs()
    delta = V.delta_fp32(sd, ORF.make_input(depth, 2.0, 0.5, 104))
    assert delta.shape == g["delta"].shape == (2, 1, 58, 104) and (delta - g["delta"]).abs().max().item() <= 2e-5
    assert 0.2 < g["delta"].std().item() < 5.0                     # the fixture's flow really moves pixels
    left, right = V.apply_divergence_nn_LR(sd, c, depth, 2.0, 0.5)
    assert (left - g["left"]).abs().max().item() <= 2e-4 and (right - g["right"]).abs().max().item() <= 2e-4
    ls, rs = V.apply_divergence_nn_LR(sd, c[:1], depth[:1], 3.0, 0.5, steps=2)
    assert (ls - g["left_s2"]).abs().max().item() <= 2e-4 and (rs - g["right_s2"]).abs().max().item() <= 2e-4
    one, _ = V.apply_divergence_nn_LR(sd, c[:1], depth[:1], 3.0, 0.5, steps=1)
    assert (one - ls).abs().mean().item() > 1e-3                   # the stepped warp really differs from the single one
    lo, ro = V.apply_divergence_nn_LR(sd, c[:1], depth[:1], 2.0, 0.5, synthetic_view="right")
    assert lo is not None and (ro - g["right_only"]).abs().max().item() <= 2e-4


@pytest.mark.parametrize("shape", [(1, 1, 8), (1, 3, 31), (2, 58, 104)])
def test_clamped_form_equals_padded_form_in_float64(sd, shape):
    x = _planes(*shape)
    a, b = V.delta_padded(sd, x), V.delta_clamped(sd, x)
    assert a.dtype == torch.float64 and a.shape == b.shape == (shape[0], 1) + shape[1:]
    assert (a - b).abs().max().item() <= 1e-12
    # and tile by tile, as the kernel schedules it (float64, no rounding): the same numbers
    assert (V.delta_tiled(sd, x, fp16=False, dtype=torch.float64) - b).abs().max().item() <= 1e-12


def test_calc_auto_warp_steps_knows_v2():
    from nunif_amd.iw3.utils import calc_auto_warp_steps
    assert calc_auto_warp_steps("row_flow_v2", 3.0, "both") == 2 and calc_auto_warp_steps("row_flow_v2", 2.5, "both") is None


@pytest.mark.skipif(not refstub.reference_available(), reason="the reference checkout is not mounted here")
def test_key_layout_and_attributes_match_the_live_class(sd, tmp_path):
    refstub.install()
    from iw3.models.row_flow_v2 import RowFlowV2 as Ref
    from nunif.models import load_model as ref_load, save_model as ref_save
    from nunif_amd.iw3.models.row_flow_v2 import RowFlowV2
    from nunif_amd.nunif.models import load_model, save_model
    ref, ours = Ref().eval(), RowFlowV2().eval()
    rsd, osd = ref.state_dict(), ours.state_dict()
    assert list(rsd) == list(osd) and all(rsd[k].shape == osd[k].shape and rsd[k].dtype == osd[k].dtype for k in rsd)
    for attr in ("name", "i2i_scale", "i2i_offset", "i2i_in_channels", "i2i_blend_size", "delta_output"):
        assert getattr(ref, attr) == getattr(ours, attr), attr
    assert float(ours.delta_scale) == float(ref.delta_scale)
    # a .pth written by either tree loads in the other, strict
    ref.load_state_dict(sd, strict=True)
    ours.load_state_dict(sd, strict=True)
    p_ref, p_ours = str(tmp_path / "ref.pth"), str(tmp_path / "ours.pth")
    ref_save(ref, p_ref)
    save_model(ours, p_ours)
    m, _ = load_model(p_ref, weights_only=True)
    assert isinstance(m, RowFlowV2) and all(torch.equal(m.state_dict()[k], sd[k]) for k in sd)
    m, _ = ref_load(p_ours, weights_only=True)
    assert isinstance(m, Ref) and all(torch.equal(m.state_dict()[k], sd[k]) for k in sd)


def test_state_dict_round_trip_and_registry(sd, tmp_path):
    from nunif_amd.iw3 import models  # noqa: F401
    from nunif_amd.nunif.models import create_model, load_model, save_model
    m = create_model("sbs.row_flow_v2").eval()
    assert (m.name, m.i2i_scale, m.i2i_offset, m.i2i_in_channels, m.i2i_blend_size) == ("sbs.row_flow_v2", 1, 28, 8, 4)
    assert set(m.state_dict()) == set(sd)
    m.load_state_dict(sd, strict=True)
    with pytest.raises(RuntimeError):
        m.load_state_dict({k: v for k, v in sd.items() if k != "non_overlap.bias"}, strict=True)
    path = str(tmp_path / "iw3_row_flow_v2.pth")
    save_model(m, path)
    m2, _ = load_model(path, weights_only=True)
    assert type(m2) is type(m) and all(torch.equal(m2.state_dict()[k], sd[k]) for k in sd)


def test_forward_refusals(sd):
    from nunif_amd.iw3.models.row_flow_v2 import RowFlowV2
    m = RowFlowV2().eval()
    with pytest.raises(NotImplementedError, match="delta_output"):
        m(torch.rand(1, 8, 16, 16))
    m.delta_output = True
    with pytest.raises(ValueError):
        m(torch.rand(1, 4, 16, 16))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        m(torch.rand(1, 3, 16, 16))                 # a CPU-resident model has no engine
    m.train()
    with pytest.raises(RuntimeError, match="inference-only"):
        m.infer_delta(torch.rand(1, 3, 16, 16))


def test_factory_loader_resolves_the_file_and_the_name_stays_refused(sd, tmp_path):
    from nunif_amd.iw3 import stereo_model_factory as F
    from nunif_amd.iw3.models.row_flow_v2 import RowFlowV2
    from nunif_amd.nunif.models import save_model
    assert F.ROW_FLOW_V2 == "iw3_row_flow_v2_20240130.pth"
    with pytest.raises(FileNotFoundError, match="iw3_row_flow_v2_20240130.pth"):
        F.load_row_flow_v2_model(-1, model_dir=str(tmp_path))
    os.makedirs(tmp_path / "checkpoints")
    m = RowFlowV2()
    m.load_state_dict(sd, strict=True)
    save_model(m, str(tmp_path / "checkpoints" / F.ROW_FLOW_V2))
    m = F.load_row_flow_v2_model(-1, model_dir=str(tmp_path))
    assert isinstance(m, RowFlowV2) and m.delta_output is True and not m.training
    assert all(torch.equal(m.state_dict()[k], sd[k]) for k in sd)
    with pytest.raises(NotImplementedError, match="load_row_flow_v2_model"):
        F.create_stereo_model("row_flow_v2", 2.0, -1, model_dir=str(tmp_path))
    with pytest.raises(NotImplementedError, match="load_row_flow_v2_model"):
        F.load_row_flow_model("row_flow_v2", -1, model_dir=str(tmp_path))


def test_apply_divergence_accepts_the_method_name():
    """The name reaches the NN branch (which asks for the side model) instead of 'not on the HIP engine yet'."""
    from nunif_amd.iw3.utils import apply_divergence
    args = SimpleNamespace(mapper="none", convergence=0.5, divergence=2.0, method="row_flow_v2", synthetic_view="both",
                           warp_steps=None, stereo_width=None, preserve_screen_border=False, disable_amp=False)
    with pytest.raises(ValueError, match="needs a side model"):
        apply_divergence(torch.rand(1, 1, 8, 8), torch.rand(1, 3, 8, 8), args, side_model=None)


# ---- the localised check of the GPU file, against mutations of the restatement ----------------------------------------------------
MUT_SHAPE, MUT_FLIP = (2, 58, 104), True


@pytest.fixture(scope="module")
def mut_refs(sd):
    E.set_threads()
    x = _planes(*MUT_SHAPE, seed=7)
    return x, V.oracle64(sd, x, MUT_FLIP), V.emulated(sd, x, MUT_FLIP)


def _check(y, y64, ye, label):
    return E.check_localised(y, y64, ye, V.CELLS, E.A_SIDE, E.B_SIDE, S.tau_for(y64), label=label)


def test_the_unmutated_tile_schedule_passes_the_localised_check(sd, mut_refs):
    x, y64, ye = mut_refs
    y = V.delta_tiled(sd, x, MUT_FLIP)
    assert torch.equal(y, ye)                       # tiles with a clamped halo ARE the whole-image net, bit for bit
    _check(y, y64, ye, "tiled")
    # an fp32-stem / fp32-head variant (what the kernel does: fewer roundings than the emulation) passes as well
    _check(V.delta_tiled(sd, x, MUT_FLIP, fp16=False), y64, ye, "tiled fp32")


@pytest.mark.parametrize("mutation", V.MUTATIONS)
def test_kernel_shaped_mutations_fail_the_localised_check(sd, mut_refs, mutation):
    x, y64, ye = mut_refs
    y = V.delta_tiled(sd, x, MUT_FLIP, mutation=mutation)
    with pytest.raises(AssertionError):
        _check(y, y64, ye, mutation)
