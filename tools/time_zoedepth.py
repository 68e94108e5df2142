"""Time ``--depth-model ZoeD_Any_N`` (nunif_amd.iw3.zoedepth_model, zoedepth_head.hip) at the 1080p-derived size: B = 4 frames of
1080 x 1920 -> 392 x 700 after ``batch_preprocess``, seeded ViT-L weights under the metric-bins head.

    python tools/time_zoedepth.py [--batch 4 --rounds 7 --inner 3] > profiles/zoedepth.txt

HIP-event windows; every round runs all variants one after the other (alternating, so that clock and thermal drift hits them
alike); median of the rounds with min and max.  Variants: the head alone on the engine; the eager restatement of the head
(tests/zoedepth_ref.py) under fp16 autocast on the same maps; the core alone (``Any_L`` geometry without the head); core + head; the
whole ``ZoeDepthModel.infer``; ``DepthAnythingModel("Any_L").infer`` on the same frames.  A last, untimed head call runs under the
engine's profiler and lists the head's launches by kernel, so that the attractor stages' share is known.
"""
import argparse
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
os.environ.setdefault("NUNIF_PROF_TAGS", "1")


def window(fn, inner):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(inner):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / inner


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=4)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--inner", type=int, default=3)
    ap.add_argument("--encoder", default="vitl")
    a = ap.parse_args()
    import zoedepth_ref as R
    from nunif_amd import _hip
    from nunif_amd.iw3.depth_model_factory import create_depth_model
    from nunif_amd.iw3.zoedepth_model import HEAD_PREFIX, batch_preprocess
    from nunif_amd.synthetic import depth_anything_v2_state_dict, zoedepth_head_state_dict
    dev = "cuda:0"
    torch.set_num_threads(16)
    core_sd = depth_anything_v2_state_dict(4400, encoder=a.encoder, features=256)
    sd = dict(core_sd)
    sd.update(zoedepth_head_state_dict(4401))
    head_sd = {k[len(HEAD_PREFIX):]: v.to(dev) for k, v in sd.items() if k.startswith(HEAD_PREFIX)}
    zoe = create_depth_model("ZoeD_Any_N").load(gpu=0, state_dict=sd)
    anyl = create_depth_model("Any_L").load(gpu=0, state_dict=core_sd)
    net = zoe.model
    frames = torch.rand(a.batch, 3, 1080, 1920, generator=torch.Generator().manual_seed(1)).to(dev)
    with torch.inference_mode():
        xp, pad_h, pad_w = batch_preprocess(frames)
        rel, feats = net.forward_features(xp)
        # the head's six maps for both head variants: seeded stand-ins of the core's shapes (time does not depend on the values)
        g = torch.Generator().manual_seed(2)
        H, W = xp.shape[2:]
        oc = torch.randn(a.batch, 32, H, W, generator=g).relu().half().to(dev)
        bt = torch.randn(a.batch, 256, feats.bh, feats.bw, generator=g).half().to(dev)
        blocks = [torch.randn(a.batch, 256, feats.rh[i], feats.rw[i], generator=g).half().to(dev) for i in range(4)]
        f2, keep = net.head.features_from_maps(oc, bt, blocks)
        relc = rel.clone()

        def eager_head():
            with torch.autocast(device_type="cuda", dtype=torch.float16):
                return torch.nan_to_num(R.head_forward(head_sd, oc, bt, blocks, relc))

        variants = [
            ("head, engine (zoedepth_head.hip)", lambda: net.head.forward(f2, relc)),
            ("head, eager restatement, fp16 autocast", eager_head),
            ("core alone (Depth-Anything V1 %s, no head)" % a.encoder, lambda: net.core(xp)),
            ("core + head (forward_features + head)", lambda: net(xp)),
            ("ZoeDepthModel.infer, 1080p frames", lambda: zoe.infer(frames, tta=False, edge_dilation=2)),
            ("DepthAnythingModel('Any_L').infer, 1080p frames", lambda: anyl.infer(frames, tta=False, edge_dilation=2)),
        ]
        for _, fn in variants:                       # warm-up: allocations, autotuned paths, clocks
            for _ in range(2):
                fn()
        torch.cuda.synchronize()
        times = {name: [] for name, _ in variants}
        for _ in range(a.rounds):
            for name, fn in variants:
                times[name].append(window(fn, a.inner))
        print(f"ZoeD_Any_N, B = {a.batch}, 1080 x 1920 -> {H} x {W} (pad {pad_h} / {pad_w}), encoder {a.encoder}, seeded weights; "
              f"{torch.cuda.get_device_name(0)}")
        print(f"HIP-event windows of {a.inner} calls, {a.rounds} alternating rounds: median ms per call (min, max)")
        for name, _ in variants:
            t = times[name]
            print(f"  {name:52s} {statistics.median(t):9.3f}  ({min(t):.3f}, {max(t):.3f})")
        he, ee = statistics.median(times[variants[0][0]]), statistics.median(times[variants[1][0]])
        co, ch = statistics.median(times[variants[2][0]]), statistics.median(times[variants[3][0]])
        print(f"  head engine / eager: {he / ee:.3f};  head's share of core + head: {(ch - co) / ch:.3f}")
        _hip.profile_enable(True)
        net.head.forward(f2, relc)
        torch.cuda.synchronize()
        recs = _hip.profile_read()
        _hip.profile_enable(False)
        total = sum(r["total_ms"] for r in recs) or 1.0
        print("one head call under the engine's profiler (serialises launches), by kernel:")
        for r in sorted(recs, key=lambda r: -r["total_ms"]):
            print(f"  {r['name']:28s} {r['launches']:3d} launches {r['total_ms'] * 1000:9.1f} us  {100 * r['total_ms'] / total:5.1f} %")


if __name__ == "__main__":
    main()
