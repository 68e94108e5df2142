"""The iw3 depth path on the HIP engine held cell by cell to a float64 oracle: the Depth-Anything encoder + DPT head
(``csrc/depth_anything.hip``, ``depth_mlp.hip``, ``conv3_lds.hip``) and the DepthAA net that runs on its output
(``csrc/depth_aa.hip``; its blocks: ``wmha8_kernel`` of ``csrc/wa_block.hip``).

``tests/errloc.py``: per image, max|y - y64| <= A_SIDE * max|emu - y64| and, in every cell of (14, 14) / (56, 56) / (8, 32) output
pixels (the depth engine: one token, a 4 x 4 token block, the conv patch of ``output_conv2.0``; aligned and shifted by half a cell) or
of (16, 16) pixels starting at the centred pad's (-ph1, -pw1) (DepthAA: one 8 x 8 window; aligned and shifted by 8 like blocks 0 and
2), region_max(y - y64) <= B_SIDE * region_max(emu - y64) + tau, tau = 2e-3 x the map's rms; emu is the reference's own fp16-autocast
arithmetic (``oracle/fp16_emulation.py``).  A_SIDE / B_SIDE = 2.1 / 3.6 are the side nets' constants, not tuned to this engine.
Only final outputs are pinned.  Cases and why: ``tests/depth_cases.py``; ``test_errloc_depth.py`` shows on the CPU what this check
catches and what it cannot.  The measured ratios: ``profiles/depth_errloc.txt``.

Every test runs one process (but for the one child that ``NUNIF_DA_MLP_SPLIT=0``, read once per process, needs), one stream and one
engine at a time: ``engine`` drops the previous engine before it builds the next.
"""
import gc
import json
import os
import subprocess
import sys

import pytest
import torch

import depth_cases as D
from oracle import depth_aa as ODAA

pytestmark = pytest.mark.gpu

_ENGINE = {}


@pytest.fixture(scope="module", autouse=True)
def _no_engine_outlives_the_module():
    yield
    _drop_engines()


def _drop_engines():
    if _ENGINE:
        torch.cuda.synchronize()
        for e in _ENGINE.values():
            e.close()
        _ENGINE.clear()
        gc.collect()


def engine(case, fresh=False):
    """The one live depth engine of this process: the case's (weights, taps, max_depth)."""
    from nunif_amd.iw3.depth_anything_v2 import HipDepthAnythingV2
    enc, shape, taps, max_depth = case
    key = (enc, D.case_state_dict(case) is D.state_dict("vits"), taps, max_depth)
    if fresh or key not in _ENGINE:
        _drop_engines()
        _ENGINE[key] = HipDepthAnythingV2(D.case_state_dict(case), "cuda:0", taps=taps, max_depth=max_depth)
    return _ENGINE[key]


def run(net, x):
    """[B,1,h,w] on the CPU (the copy synchronises: nothing of this call is in flight when the next one starts)."""
    return net(x.to("cuda:0")).cpu().unsqueeze(1)


# ---- the depth engine -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", D.CASES, ids=D.case_id)
def test_depth_anything_cell_by_cell(hiplib, capsys, case):
    x, y64, ye = D.references(case)
    net = engine(case)
    y = run(net, x)
    D.check(y, y64, ye, D.NET, D.case_id(case), capsys)
    assert torch.equal(run(net, x), y), "a second call on the same input gave other bytes"


@pytest.mark.parametrize("case", D.BATCHED, ids=D.case_id)
def test_image_b_of_a_batch_alone_passes_the_same_check(hiplib, capsys, case):
    """Not required to be bit-equal to the batched call: the MLP form (split pair / one block per tile) is picked from B * Np."""
    x, y64, ye = D.references(case)
    net = engine(case)
    for b in range(case[1][0]):
        y = run(net, x[b:b + 1].contiguous())
        D.check(y, y64[b:b + 1], ye[b:b + 1], D.NET, f"{D.case_id(case)} image {b} alone", capsys)


SWITCH_CASES = [("vits", (1, 56, 112), None, 0.0), ("vits", (3, 168, 224), None, 0.0)]


@pytest.mark.parametrize("switch", ["NUNIF_DA_MLP", "NUNIF_CONV3_LDS", "NUNIF_DA_BRANCH_STREAMS"])
@pytest.mark.parametrize("case", SWITCH_CASES, ids=D.case_id)
def test_switched_off_forms_pass_the_same_check(hiplib, capsys, monkeypatch, case, switch):
    """The two gemm launches behind the fused MLP, the gather form of the 3 x 3 convs, the reassemble branches on the main stream."""
    x, y64, ye = D.references(case)
    monkeypatch.setenv(switch, "0")
    net = engine(case, fresh=True)                                     # NUNIF_CONV3_LDS also decides the engine's weight layout
    try:
        D.check(run(net, x), y64, ye, D.NET, f"{D.case_id(case)} {switch}=0", capsys)
    finally:
        _drop_engines()


def test_vitb_tap_major_convs_pass_the_same_check(hiplib, capsys, monkeypatch):
    """ViT-B at 112 x 224 with ``NUNIF_CONV3_CM=0`` (read per engine): layer3_rn / layer4_rn on the tap-major conv3_lds_kernel."""
    x, y64, ye = D.references(D.VITB_CASE)
    monkeypatch.setenv("NUNIF_CONV3_CM", "0")
    net = engine(D.VITB_CASE, fresh=True)
    try:
        D.check(run(net, x), y64, ye, D.NET, f"{D.case_id(D.VITB_CASE)} NUNIF_CONV3_CM=0", capsys)
    finally:
        _drop_engines()


SPLIT_OFF_CASES = [("vits", (1, 28, 28), None, 0.0), ("vits", (1, 112, 224), None, 0.0), ("vits", (3, 168, 224), None, 0.0)]
_CHILD = r"""
import json, os, sys, torch
sys.path.insert(0, os.getcwd()); sys.path.insert(0, os.path.join(os.getcwd(), "tests"))
import depth_cases as D
import errloc as E
from nunif_amd.iw3.depth_anything_v2 import HipDepthAnythingV2
with torch.inference_mode():
    net = HipDepthAnythingV2(D.state_dict("vits"), "cuda:0")
    for case in [c for c in D.CASES if c[0] == "vits" and c[3] == 0.0 and c[2] is None and D.tokens(*c[1][1:]) in (5, 129, 193)]:
        x, y64, ye = D.references(case)
        y = net(x.to("cuda:0")).cpu().unsqueeze(1)
        st = D.stats(y, y64, ye, D.NET, E.B_SIDE)
        print("STATS " + json.dumps({"case": D.case_id(case), "finite": st["_finite"], "err": st["_gmax"], "noise": st["_nmax"], "worst": st["worst"],
                                     "summary": E.summary(st), "worst_regions": E.format_regions(st, 3)}), flush=True)
print("OK")
"""


def test_one_block_mlp_form_passes_the_same_check(hiplib, capsys):
    """``NUNIF_DA_MLP_SPLIT=0`` (da_mlp_kernel, one workgroup per 64 tokens, at every size) is read once per process: one fresh
    child runs Np = 5, 129 and 193 and prints its per-case figures, which are asserted here."""
    import errloc as E
    _drop_engines()
    env = dict(os.environ, NUNIF_DA_MLP_SPLIT="0")
    r = subprocess.run([sys.executable, "-c", _CHILD], env=env, capture_output=True, text=True, timeout=300,
                       cwd=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    assert r.returncode == 0 and "OK" in r.stdout, (r.stdout[-2000:], r.stderr[-2000:])
    got = [json.loads(line[6:]) for line in r.stdout.splitlines() if line.startswith("STATS ")]
    assert [g["case"] for g in got] == [D.case_id(c) for c in SPLIT_OFF_CASES]
    for g in got:
        with capsys.disabled():
            print(f"\nerrloc {g['case']} NUNIF_DA_MLP_SPLIT=0: global {g['summary']['global']:.2f} worst {g['summary']['worst']:.2f} "
                  f"(err {g['err']:.2e} noise {g['noise']:.2e}) bands {g['summary']['bands']}")
        assert g["finite"], g
        assert g["err"] <= E.A_SIDE * g["noise"], g
        assert g["worst"] <= E.B_SIDE, g


# ---- DepthAA ----------------------------------------------------------------------------------------------------------------------
def depth_aa():
    from nunif_amd.iw3.models import DepthAA
    _drop_engines()
    m = DepthAA().eval()
    m.load_state_dict(D.aa_state_dict(), strict=True)
    return m.to("cuda:0")


@pytest.mark.parametrize("case", D.AA_CASES, ids=D.aa_case_id)
def test_depth_aa_window_by_window(hiplib, capsys, case):
    shape, mode = case
    x, y64, ye = D.aa_references(case)
    m = depth_aa()
    xg = x.to("cuda:0")
    if mode == "infer":
        assert float(x.min()) >= 3.0 and float(x.max()) <= 11.0 and float(x.max() - x.min()) > 4.0
        y = m.infer(xg).cpu()
        D.check(y, y64, ye, D.AA, D.aa_case_id(case), capsys)
        assert torch.equal(m.infer(xg).cpu(), y)
        return
    y = m(xg, clamp=False).cpu()
    D.check(y, y64, ye, D.AA, D.aa_case_id(case), capsys)
    assert torch.equal(m(xg, clamp=False).cpu(), y), "a second call on the same input gave other bytes"
    assert torch.equal(m(xg).cpu(), y.clamp(0, 1)), "the clamped forward is not clamp(unclamped, 0, 1)"
    for b in range(shape[0] if shape[0] > 1 else 0):
        one = m(xg[b:b + 1].contiguous(), clamp=False).cpu()
        D.check(one, y64[b:b + 1], ye[b:b + 1], D.AA, f"{D.aa_case_id(case)} image {b} alone", capsys)


def test_depth_aa_constant_map_through_infer(hiplib):
    """max - min = 0: the reference's (x - min) / 0 goes through ``nan_to_num`` and the result is the constant itself."""
    x = torch.full((2, 1, 33, 47), 7.25)
    want = ODAA.infer(D.aa_state_dict(), x)
    assert torch.equal(want, x)
    assert torch.equal(depth_aa().infer(x.to("cuda:0")).cpu(), want)
