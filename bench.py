#!/usr/bin/env python3
"""Benchmark of the nunif hot path on MI355X.  Headline: waifu2x swin_unet 2x, tile 256, synthetic 1080p frames.

    python bench.py [--gpus N] [--steps K] [--warmup W] [--dump-outputs DIR] [--full]

``--gpus N`` with N > 1 and no rendezvous in the environment RE-LAUNCHES this script as N ranks (one per GPU) through
``python -m torch.distributed.run --nnodes=1 --nproc-per-node N --master-addr 127.0.0.1``; launched by torchrun (the
driver's form) it reads RANK / LOCAL_RANK / WORLD_SIZE / MASTER_* from the environment.  Backend: ``nccl`` (= RCCL).

A *step* is one full tiled render (gather -> 45 tiles through the net -> stitch) of ``--streams`` 1080p frames per
rank, the input frames already resident in HBM.  Frames are independent, so ranks shard frames with no data-path
collective (weak scaling: every rank renders K steps).  ``value`` = input megapixels of all ranks / wall time (barrier +
``torch.cuda.synchronize()`` on both sides, max over ranks), the metric BASELINE.json names ("MPix" = source-frame
pixels).  The default K gives a timed region of >= 3 s.

A plain run sets up, warms up, times the K steps and prints ONE JSON line on rank 0 with the contract fields (``metric``,
``value``, ``unit``, ``higher_is_better``, ``dtype``, ``ms_per_step`` = wall milliseconds of one timed step) and figures derived
from them.  ``--dump-outputs DIR`` then writes the frames of the last timed step (``dump_outputs``); inputs and weights are
seeded, so two builds run with the same arguments can be compared output for output.

``--full`` runs every other leg after the timed region and adds to the line (the ``--no-*`` switches drop single legs)
  roofline      — the dominant kernel (largest share of HIP-event time; classes are kernel symbols): algorithmic FLOPs or
                  bytes per launch / measured average launch duration, against the MI355X peak that bounds it
                  (arithmetic intensity vs the 2.5 PFLOP/s / 8 TB/s ridge); ``traffic`` = HBM bytes per launch from the
                  newest committed rocprofv3 PMC passes that contain THIS build's kernel (profiles/, FETCH_SIZE x2 +
                  WRITE_SIZE, KiB units), null otherwise
  single_stream — the same frames one at a time on one stream (the per-kernel numbers are measured this way)
  gathered      — N > 1: the same frames through ``nunif_amd.parallel.render_sharded``: every finished frame is quantised
                  on the device (HIP kernel) and sent to rank 0 with a non-blocking point-to-point transfer (RCCL over
                  xGMI) that overlaps the next render; rate = frames DELIVERED to rank 0 / wall time
  iw3           — BASELINE config 4 on one GPU: uint8 1080p frames in HBM -> FrameCallbackPool -> Depth-Anything-V2 ViT-S
                  geometry -> forward_fill / row_flow_v3 -> SBS uint8, with the forward-warp kernel's own HBM roofline
                  (40 B / pixel) and the CPU oracle of forward_fill + dilate_edge timed beside it
  scale4x_4k    — BASELINE config 3 on one GPU: swin_unet 4x on a 4K frame (170 tiles of 256)
  cunet         — north_star's second waifu2x generator: BASELINE configs[0] geometry (512 x 512, 9 tiles) and a 1080p frame,
                  dominant conv kernel's roofline, PSNR vs the CPU oracle
  config5       — BASELINE configs[4] shape on one GPU: 4K, VDA-streaming wrapper (per-frame ViT-S stand-in, named as such) +
                  mask-MLBW backward warp + 12-frame video inpaint
  cpu_baseline  — the CPU oracle (oracle/, a torch-fp32 port of the reference path) on the host cores: thread count and tile
                  minibatch swept over {8, 32, physical} x {1, 4}, then warm-up + median of 3 with the best
"""
import argparse
import json
import math
import os
import re
import socket
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

FRAME_H, FRAME_W = 1080, 1920
TILE = 256
MFMA_PEAK_TFLOPS = 2500.0   # dense fp16/bf16, MI355X_MICROARCH.md "Peak BF16/FP16 MFMA"
HBM_PEAK_GBS = 8000.0       # spec (≈6.3 TB/s achievable)


def parse_args():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=220)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--batch-size", type=int, default=int(os.environ.get("NUNIF_BENCH_BATCH", "45")),
                    help="tiles per model launch (the reference's tile minibatch; results do not depend on it)")
    ap.add_argument("--streams", type=int, default=int(os.environ.get("NUNIF_BENCH_STREAMS", "2")),
                    help="frames rendered CONCURRENTLY per step, one HIP stream + one engine handle each (a step then "
                         "covers this many frames; the tails of one frame's kernels overlap the other frame's work)")
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--no-host-frames", action="store_true",
                    help="skip the extra (reported, never `value`) PCIe-inclusive measurement through the pinned frame ring")
    ap.add_argument("--no-iw3", action="store_true", help="skip the iw3 (config 4) sub-record")
    ap.add_argument("--no-4k", action="store_true", help="skip the 4K 4x (config 3) sub-record")
    ap.add_argument("--no-cunet", action="store_true", help="skip the cunet (config 1 geometry) sub-record")
    ap.add_argument("--no-config5", action="store_true", help="skip the 4K VDA-wrapper + mask-MLBW + video-inpaint (config 5) sub-record")
    ap.add_argument("--full", action="store_true",
                    help="after the headline, also run every other leg (single stream, per-kernel roofline, host frames, 4K / cunet / "
                         "iw3 / config 5 sub-records, CPU baseline, the N > 1 delivery legs); the --no-* switches select among them")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="write the frames the last timed step rendered to DIR/<name>.npy (float32; a fixed seeded sample of each)")
    args = ap.parse_args()
    if args.steps < 1:
        ap.error("--steps must be at least 1")
    return args


def emit(result):
    """Print THE line.  ``ok`` is false whenever a leg recorded an error (``errors``); the return value is the exit code rank 0
    leaves with after the line is out — a failed leg must not look like a clean run to a driver that only checks rc."""
    result["ok"] = not result.get("errors")
    print(json.dumps(result), flush=True)
    return 0 if result["ok"] else 3


def relaunch_as_ranks(args):
    """``python bench.py --gpus N`` without a rendezvous: become ``torch.distributed.run`` with N local ranks."""
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    env = dict(os.environ)
    env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={args.gpus}",
           "--master-addr", "127.0.0.1", "--master-port", str(port), os.path.abspath(__file__)] + sys.argv[1:]
    os.execvpe(cmd[0], cmd, env)


GATHER_TIMEOUT_S = 420          # watchdog of the N > 1 legs behind the headline (delivery, iw3, cunet; see main)
CPU_WHOLE_FRAME_BUDGET_S = 40   # cpu_baseline times a whole 1080p frame on the host when the crop predicts at most this
DUMP_FLOATS = 12 * 2 ** 20      # --dump-outputs: float32 elements over all files of all ranks (48 MiB)
DUMP_SEED = 20240611


def dump_outputs(path, outs, rank, world):
    """Write the frames of the last timed step as ``path/out_rank<r>_stream<k>.npy`` (float32, flattened).  A frame larger than its
    share of DUMP_FLOATS is written as a sample: the elements at DUMP_SEED's sorted random positions, the same on every run with the
    same arguments, so two builds can be compared file for file."""
    import numpy as np
    import torch
    os.makedirs(path, exist_ok=True)
    share = DUMP_FLOATS // (world * len(outs))
    for k, y in enumerate(outs):
        flat = y.detach().reshape(-1)
        if flat.numel() > share:
            idx = torch.randperm(flat.numel(), generator=torch.Generator().manual_seed(DUMP_SEED))[:share].sort().values
            flat = flat[idx.to(flat.device)]
        np.save(os.path.join(path, f"out_rank{rank}_stream{k}.npy"), flat.float().cpu().numpy())


def synth_frame(seed, h, w):
    import torch
    g = torch.Generator().manual_seed(seed)
    low = torch.rand(1, 3, h // 16 + 1, w // 16 + 1, generator=g)
    up = torch.nn.functional.interpolate(low, size=(h, w), mode="bilinear", align_corners=False)[0]
    return torch.clamp(up * 0.8 + 0.2 * torch.rand(3, h, w, generator=g), 0, 1)


def physical_cores():
    try:
        import psutil
        n = psutil.cpu_count(logical=False)
        if n:
            return int(n)
    except Exception:
        pass
    return max(1, (os.cpu_count() or 2) // 2)


def median_time(fn, repeats=3):
    """One untimed warm-up call, then the median wall time of ``repeats`` calls."""
    out = fn()
    ts = []
    for _ in range(repeats):
        t0 = time.perf_counter()
        out = fn()
        ts.append(time.perf_counter() - t0)
    return statistics.median(ts), out


def cpu_baseline(sd, frame):
    """The oracle's tiled_render on a crop of the same frame (4 tiles of 256).  128 threads on 36-token ``bmm``s is
    oversubscription (round-2 verdict), so the thread count and the tile minibatch are SWEPT first — one warm-up + one timed
    pass each over {8, 32, physical cores} x {minibatch 1, 4} — and the best setting is then timed as the median of 3."""
    import torch
    from oracle import seam_blending as OS
    from oracle import swin_unet as O
    phys = physical_cores()
    crop = frame[:, :476, :476].contiguous()        # 2x2 tiles of 256 (input step 236 + 2 x 8 offset rows), same tile size
    fn = lambda mb: O.model_forward(sd, mb)         # noqa: E731
    sweep = {}
    for threads in sorted({min(8, phys), min(32, phys), phys}):
        for mb in (1, 4):
            torch.set_num_threads(threads)
            OS.tiled_render(crop, fn, 2, 16, 8, TILE, mb)
            t0 = time.perf_counter()
            OS.tiled_render(crop, fn, 2, 16, 8, TILE, mb)
            sweep[(threads, mb)] = time.perf_counter() - t0
    (threads, mb), _ = min(sweep.items(), key=lambda kv: kv[1])
    torch.set_num_threads(threads)
    dt, out = median_time(lambda: OS.tiled_render(crop, fn, 2, 16, 8, TILE, mb), repeats=3)
    frame_s = dt / 4 * 45
    value, whole, whole_out = crop.shape[1] * crop.shape[2] / 1e6 / dt, None, None
    sample = (f"oracle tiled_render of a 476x476 crop of the bench frame (4 tiles of 256, minibatch {mb}), best of a threads x "
              f"minibatch sweep ({threads} threads), 1 warm-up + median of 3 passes, {dt:.2f} s per pass "
              f"(= {frame_s:.0f} s per 1080p frame of 45 tiles")
    if frame_s <= CPU_WHOLE_FRAME_BUDGET_S:
        # BASELINE.md section 4 asks for ONE WHOLE FRAME when it fits: a single timed pass (everything is warm after the sweep)
        t0 = time.perf_counter()
        whole_out = OS.tiled_render(frame, fn, 2, 16, 8, TILE, mb)        # kept: the GPU frame at the timed configuration is compared with it
        whole = time.perf_counter() - t0
        value = frame.shape[1] * frame.shape[2] / 1e6 / whole
        sample += f"); `value` is the WHOLE 1080p frame (45 tiles) timed once with that setting: {whole:.1f} s"
    else:
        sample += f", above the {CPU_WHOLE_FRAME_BUDGET_S}-s budget for timing it whole: `value` is the crop's rate)"
    return {"value": round(value, 5), "unit": "MPix/s", "cores": threads, "kind": "port",
            "physical_cores": phys, "tile_minibatch": mb,
            "sweep_s_per_pass": {f"{t}thr_mb{b}": round(v, 2) for (t, b), v in sorted(sweep.items())},
            "whole_1080p_frame_estimate_s": round(frame_s, 1),
            "whole_1080p_frame_s": round(whole, 2) if whole is not None else None,
            "sample": sample + "; tools/cpu_ref_vs_port.py gives the reference / port ratio measured in the build container"}, crop, out, whole_out


# PMC summaries of workloads other than the headline bench: the same kernel symbol runs other shapes there, so they are looked up
# by name only (profiles/<tag>_pmc_{FETCH,WRITE}_SIZE.txt, written by tools/profile_cunet.sh / tools/profile_config5.sh)
WORKLOAD_PMC = {"cunet": "r05c", "config5": "r05f", "scale4x_4k": "r06k"}


def pmc_traffic_bytes(symbol, only=None):
    """HBM bytes per launch of ``symbol`` from the newest committed PMC summaries (profiles/rNN_pmc_*.txt) that list it; ``only``
    names the one summary set to read (a workload of its own, WORKLOAD_PMC)."""
    def per_launch(path):
        key = re.sub(r"[^A-Za-z0-9]", "", symbol.split("<")[0])
        args = re.findall(r"\d+", symbol.split("<", 1)[1]) if "<" in symbol else []
        if not os.path.exists(path):
            return None
        for line in open(path):
            name = line.split(" launches=")[0]
            flat = re.sub(r"[^A-Za-z0-9]", "", name)
            # demangled "ns::kernel<6, 4>(…)" or mangled "_ZN5nunif15proj_mlp_kernelILi96ELi4EEE…"
            if key in flat and all((f"Li{a}E" in name) or re.search(rf"[<,]\s*{a}\s*[,>]", name) for a in args):
                m = re.search(r"per_launch=([0-9.]+)", line)
                if m:
                    return float(m.group(1)) * 1024.0
        return None
    pdir = os.path.join(ROOT, "profiles")
    rounds = sorted({re.match(r"(r\d\d[a-z]{0,2})_pmc_FETCH_SIZE", f).group(1) for f in os.listdir(pdir)
                     if re.match(r"r\d\d[a-z]{0,2}_pmc_FETCH_SIZE", f)}) if os.path.isdir(pdir) else []
    rounds = [only] if only else [r for r in rounds if r not in WORKLOAD_PMC.values()]
    for r in reversed(rounds):
        fetch = per_launch(os.path.join(pdir, f"{r}_pmc_FETCH_SIZE.txt"))
        write = per_launch(os.path.join(pdir, f"{r}_pmc_WRITE_SIZE.txt"))
        if fetch is not None and write is not None:
            return 2.0 * fetch + write, r      # FETCH_SIZE reports half of a wide coalesced read on gfx950
    return None, None


def kernel_table(recs, n_frames):
    classes = []
    total = sum(r["total_ms"] for r in recs) or 1.0
    for r in sorted(recs, key=lambda r: -r["total_ms"]):
        sec = r["total_ms"] * 1e-3
        classes.append({"kernel": r["name"], "share": round(r["total_ms"] / total, 4),
                        "avg_us": round(1e3 * r["total_ms"] / max(1, r["launches"]), 2),
                        "launches_per_frame": r["launches"] // max(1, n_frames),
                        "tflops": round(r["flops"] / sec / 1e12, 2) if sec else 0.0,
                        "gbs": round(r["bytes"] / sec / 1e9, 1) if sec else 0.0})
    return classes


def roofline_of(rec, with_pmc=True, pmc_set=None):
    n = max(1, rec["launches"])
    avg_s = rec["total_ms"] * 1e-3 / n
    flops_l, bytes_l = rec["flops"] / n, rec["bytes"] / n
    intensity = flops_l / bytes_l if bytes_l else float("inf")
    ridge = MFMA_PEAK_TFLOPS * 1e12 / (HBM_PEAK_GBS * 1e9)
    traffic, src = pmc_traffic_bytes(rec["name"], pmc_set) if with_pmc else (None, None)
    if intensity >= ridge:
        ach = flops_l / avg_s / 1e12
        roof = {"kernel": rec["name"], "bound": "mfma", "achieved": round(ach, 2), "peak": MFMA_PEAK_TFLOPS,
                "unit": "TFLOP/s", "frac": round(ach / MFMA_PEAK_TFLOPS, 4)}
    else:
        ach = bytes_l / avg_s / 1e9
        roof = {"kernel": rec["name"], "bound": "hbm", "achieved": round(ach, 1), "peak": HBM_PEAK_GBS,
                "unit": "GB/s", "frac": round(ach / HBM_PEAK_GBS, 4)}
    roof.update({"traffic": traffic, "traffic_source": f"profiles/{src}_pmc_*" if src else None,
                 "avg_launch_us": round(avg_s * 1e6, 2), "launches": n, "algorithmic_flops_per_launch": flops_l,
                 "algorithmic_bytes_per_launch": bytes_l,
                 "flop_per_byte": round(intensity, 1) if math.isfinite(intensity) else None})
    if flops_l:
        roof.update({"achieved_tflops": round(flops_l / avg_s / 1e12, 2),
                     "mfma_frac": round(flops_l / avg_s / 1e12 / MFMA_PEAK_TFLOPS, 4)})
    return roof


# ---- iw3 (BASELINE config 4) on one GPU ------------------------------------------------------------------------------------
class DeviceFrame:
    """A decoded frame that already sits in HBM as HWC uint8 (PCIe stays out of the timed region)."""

    def __init__(self, data, pts):
        self.data, self.pts = data, pts


def iw3_record(dev, with_cpu):
    import torch
    from nunif_amd import _hip
    from nunif_amd.iw3 import utils as U
    from nunif_amd.iw3.base_depth_model import CallableDepthModel
    from nunif_amd.iw3.depth_anything_v2 import HipDepthAnythingV2
    from nunif_amd.iw3.frame_pipeline import FrameCallbackPool, PipelineOps, bind_batch_frame_callback
    from nunif_amd.iw3.models.row_flow_v3 import RowFlowV3
    from nunif_amd.synthetic import depth_anything_v2_state_dict, row_flow_v3_state_dict, synth_depth

    H, W, batch, n_frames = FRAME_H, FRAME_W, 4, 96
    depth_model = CallableDepthModel(HipDepthAnythingV2(depth_anything_v2_state_dict(601), str(dev)))
    depth_model.load(gpu=dev.index or 0)
    side = RowFlowV3().eval()
    side.load_state_dict(row_flow_v3_state_dict(301))
    side = side.to(dev)
    side.delta_output = True
    g = torch.Generator().manual_seed(5)
    frames = [(synth_frame(900 + i, H, W) * 255).round().to(torch.uint8).permute(1, 2, 0).contiguous().to(dev) for i in range(4)]

    def run(method, n):
        a = argparse.Namespace(batch_size=batch, mapper="none", convergence=0.5, divergence=2.0, method=method,
                               synthetic_view="both", warp_steps=None, stereo_width=None, preserve_screen_border=False,
                               disable_amp=False, edge_dilation=2, pix_fmt="yuv420p", state={"device": dev})
        depth_model.reset()
        depth_model.enable_ema(0.75, buffer_size=4)
        ops = PipelineOps(to_tensor=lambda frame, device=None: U.to_tensor(frame.data, device=device))
        cb, pre = bind_batch_frame_callback(depth_model, side, {n // 2}, a, ops=ops)
        pool = FrameCallbackPool(frame_callback=cb, preprocess_callback=pre, batch_size=batch, device=str(dev), max_workers=2,
                                 max_batch_queue=3, require_pts=True, require_flush=True, ops=ops)
        n_out = 0
        torch.cuda.synchronize(dev)
        t0 = time.perf_counter()
        for i in range(n):
            r = pool(DeviceFrame(frames[i % len(frames)], i))
            n_out += len(r) if r else 0
        n_out += len(pool(None))
        torch.cuda.synchronize(dev)
        dt = time.perf_counter() - t0
        assert n_out == n, (n_out, n)
        return dt / n

    rec = {"config": "BASELINE configs[3]: uint8 1080p frames in HBM -> FrameCallbackPool -> bind_batch_frame_callback "
                     f"(batch {batch}, Depth-Anything-V2 ViT-S geometry with random-init weights — engine pinned against HuggingFace "
                     "transformers' DepthAnythingForDepthEstimation, tests/golden/depth_anything_hf.npz, "
                     "EMA 0.75 x 4-frame look-ahead, one scene cut, edge_dilation 2) -> stereo -> SBS uint8",
           "frame": [H, W], "frames": n_frames, "batch": batch, "unit": "input MPix/s"}
    for method in ("forward_fill", "row_flow_v3"):
        run(method, 2 * batch)
        dt = min(run(method, n_frames) for _ in range(2))
        rec[method] = {"ms_per_frame": round(dt * 1e3, 3), "fps": round(1 / dt, 1), "value": round(H * W / dt / 1e6, 1)}
    # the forward-warp kernel on its own: algorithmic 40 B / pixel (read rgb + depth once, write two eyes)
    from nunif_amd.iw3.forward_warp import apply_divergence_forward_warp
    from nunif_amd.iw3.dilation import dilate_edge
    c = torch.stack([synth_frame(910 + i, H, W) for i in range(2)]).to(dev)
    d = synth_depth(1, 2, H, W, "smooth_edges").to(dev)
    dsmall = synth_depth(2, 2, 392, 686, "smooth_edges").to(dev) * 5
    fw = lambda: apply_divergence_forward_warp(c, d, 2.0, 0.5, method="forward_fill", width_base=False)      # noqa: E731
    for _ in range(3):
        fw()
        dilate_edge(dsmall, 2)
    torch.cuda.synchronize(dev)
    _hip.profile_read(reset=True)
    _hip.profile_enable(True)
    for _ in range(20):
        fw()
    torch.cuda.synchronize(dev)
    recs = {r["name"]: r for r in _hip.profile_read(reset=True)}
    _hip.profile_enable(False)
    if "forward_warp" in recs:
        roof = roofline_of(recs["forward_warp"], with_pmc=True)
        roof["kernel"] = "forward_warp_kernel"
        roof["workload"] = "forward_fill, both eyes, 2 x 1080p per launch, divergence 2.0"
        rec["roofline"] = roof
    t0 = time.perf_counter()
    for _ in range(50):
        dilate_edge(dsmall, 2)
    torch.cuda.synchronize(dev)
    rec["dilate_edge_us_per_call"] = round((time.perf_counter() - t0) / 50 * 1e6, 1)
    # the reference's own depth harness (iw3/depth_anything_model.py _bench :289-308: model.infer on a 4 x 1080p batch, 20
    # calls, FPS) for the three published geometries, random-init weights (parity unpinned)
    x4 = torch.stack([synth_frame(920 + i, H, W) for i in range(4)]).to(dev)
    rec["depth_infer_fps"] = {"protocol": "BaseDepthModel.infer(x[4,3,1080,1920]) -> [4,1,392,686], 20 calls after 2 warm-ups "
                                          "(reference _bench: Any_L, B = 4, N = 20)"}
    for enc in ("vits", "vitb", "vitl"):
        dm = CallableDepthModel(HipDepthAnythingV2(depth_anything_v2_state_dict(601, grid=37, encoder=enc), str(dev)))
        dm.load(gpu=dev.index or 0)
        for _ in range(2):
            dm.infer(x4)
        torch.cuda.synchronize(dev)
        t0 = time.perf_counter()
        for _ in range(20):
            dm.infer(x4)
        torch.cuda.synchronize(dev)
        rec["depth_infer_fps"][enc] = round(20 * 4 / (time.perf_counter() - t0), 1)
        del dm
    if with_cpu:
        from oracle import dilation as OD
        from oracle import forward_warp as OF
        cores = physical_cores()
        torch.set_num_threads(cores)
        cc, dc, dsc = c[:1].cpu(), d[:1].cpu(), dsmall[:1].cpu()
        dt, _ = median_time(lambda: (OD.dilate_edge(dsc, 2), OF.forward_warp(cc, dc, 2.0, 0.5, fill=True)), repeats=3)
        rec["cpu_baseline"] = {"value": round(H * W / 1e6 / dt, 3), "unit": "MPix/s", "cores": cores, "kind": "port",
                               "sample": "oracle dilate_edge(392x686 depth, 2 iterations) + forward_fill of one whole 1080p "
                                         f"frame (both eyes), 1 warm-up + median of 3, {dt:.2f} s per pass; the depth "
                                         "network is external to the reference and not part of `value` — "
                                         "`with_depth_net` adds it"}
        # ... and the frame with its depth network on the same cores: batch_preprocess (antialiased resize to 392 x 686, normalise) +
        # the ViT-S / DPT restatement (oracle/depth_anything_v2.py, pinned against HuggingFace), swept over thread counts like the
        # swin baseline (one frame; 128 threads oversubscribe the 1 372-token GEMMs)
        from oracle import depth_anything_v2 as ODA
        from oracle import depth_pre as ODP
        sd_d = depth_anything_v2_state_dict(601)
        best = None
        for th in sorted({min(8, cores), min(32, cores), cores}):
            torch.set_num_threads(th)
            run = lambda: ODA.model_forward(sd_d, ODP.batch_preprocess(cc))       # noqa: E731
            run()
            t0 = time.perf_counter()
            run()
            t = time.perf_counter() - t0
            if best is None or t < best[0]:
                best = (t, th)
        rec["cpu_baseline"]["with_depth_net"] = {
            "value": round(H * W / 1e6 / (dt + best[0]), 3), "unit": "MPix/s", "depth_net_s": round(best[0], 2),
            "depth_net_threads": best[1],
            "sample": "the same pass + batch_preprocess + the Depth-Anything-V2 ViT-S restatement on one 1080p frame "
                      "(best of 8 / 32 / all-core thread counts, 1 warm-up + 1 timed pass)"}
    return rec


def iw3_sharded_leg(dist, world, rank, dev, barrier, frames_per_rank=48, batch=4, depth_model=None, stereo_fn=None,
                    frame_hw=None, make_frame=None):
    """BASELINE's second metric at N GPUs (configs[3]: iw3 DepthAnythingV2 ViT-S + forward_warp SBS, 1080p, frame-parallel): ONE
    stream of ``frames_per_rank * world`` frames through ``stereo_frames_sharded`` — batch b on rank b mod N, the EMA look-ahead
    replayed across the ranks from an all-gather of two scalars per frame, finished SBS uint8 frames gathered to rank 0.  Timed
    between barriers, MAX over ranks; ``value`` = whole-stream input MPix/s.  ``depth_model`` / ``stereo_fn`` / ``make_frame``:
    stand-ins for the gloo unit test (tests/test_parallel_gloo.py); defaults: the HIP engine as in ``iw3_record``."""
    import torch
    from nunif_amd.iw3.frame_pipeline import stereo_frames_sharded
    H, W = frame_hw or (FRAME_H, FRAME_W)
    n = frames_per_rank * world
    n -= n % batch
    infer_kwargs = None
    if depth_model is None:
        infer_kwargs = {"edge_dilation": 2}
        from nunif_amd.iw3 import utils as U
        from nunif_amd.iw3.base_depth_model import CallableDepthModel
        from nunif_amd.iw3.depth_anything_v2 import HipDepthAnythingV2
        from nunif_amd.iw3.frame_pipeline import PipelineOps
        from nunif_amd.synthetic import depth_anything_v2_state_dict
        depth_model = CallableDepthModel(HipDepthAnythingV2(depth_anything_v2_state_dict(601), str(dev)))
        depth_model.load(gpu=dev.index or 0)
        a = argparse.Namespace(batch_size=batch, mapper="none", convergence=0.5, divergence=2.0, method="forward_fill",
                               synthetic_view="both", warp_steps=None, stereo_width=None, preserve_screen_border=False,
                               disable_amp=False, edge_dilation=2, pix_fmt="yuv420p", state={"device": dev})
        ops = PipelineOps()

        def stereo_fn(xs, ds, reset_pts):
            left, right = U.apply_divergence(ds, xs, a, None, reset_pts=reset_pts)
            return [ops.stereo_out(left[i], right[i], a) for i in range(left.shape[0])]
    make_frame = make_frame or (lambda i: synth_frame(900 + i % 4, H, W).to(dev))
    mine = {i for b in range(rank, n // batch, world) for i in range(b * batch, (b + 1) * batch)}
    pool = {}
    frames = [None] * n
    for i in sorted(mine):                                   # a rank holds only the frames of its own batches, resident in HBM
        if i % 4 not in pool:
            pool[i % 4] = make_frame(i)
        frames[i] = pool[i % 4]
    cuts = {n // 2}

    def one_pass():
        depth_model.reset()
        depth_model.enable_ema(0.75, buffer_size=4)
        return stereo_frames_sharded(frames, list(range(n)), cuts, depth_model, stereo_fn, batch, dst=0, infer_kwargs=infer_kwargs)

    with torch.inference_mode():
        one_pass()                                           # warm-up (collectives initialised, workspaces allocated)
        barrier()
        t0 = time.perf_counter()
        out = one_pass()
        barrier()
    dt = time.perf_counter() - t0
    t = torch.tensor([dt], dtype=torch.float64, device=dev)
    dist.all_reduce(t, op=dist.ReduceOp.MAX)
    dt = float(t.item())
    if rank != 0:
        return None
    return {"config": "BASELINE configs[3] at N GPUs: ONE 1080p stream, Depth-Anything-V2 ViT-S geometry (random-init) + forward_fill "
                      f"+ SBS uint8, batch {batch}, EMA 0.75 x 4-frame look-ahead, one scene cut, edge_dilation 2; "
                      "stereo_frames_sharded: batch b on rank b mod N, per round one all-gather of [batch, 2] floats per rank "
                      "and one gather of finished frames to rank 0 (inside the timed region)",
            "frame": [H, W], "frames": n, "frames_delivered": len(out), "batch": batch, "world": world, "unit": "input MPix/s",
            "scaling": "weak", "ms_per_frame": round(1e3 * dt / n, 3), "fps": round(n / dt, 1),
            "value": round(H * W * n / dt / 1e6, 1)}


def cunet_sharded_leg(dist, world, rank, dev, barrier, frames_per_rank=16, render_fn=None, frame=None):
    """north_star's second generator at N GPUs: every rank renders its own 1080p frames with waifu2x cunet (tile 256, whole frame in
    one minibatch), no collective inside the timed region; ``value`` = all ranks' input MPix/s over the MAX of the ranks' times.
    ``render_fn`` / ``frame``: stand-ins of the CPU launcher rehearsal (``dry_standins``)."""
    import torch
    m = None
    if render_fn is None:
        from nunif_amd.nunif.models import create_model
        from nunif_amd.nunif.utils.render import tiled_render
        import nunif_amd.waifu2x.models.cunet  # noqa: F401
        from nunif_amd.synthetic import cunet_state_dict
        m = create_model("waifu2x.cunet").eval()
        m.load_state_dict(cunet_state_dict(201))
        m = m.to(dev)

        def render_fn(f):
            return tiled_render(f, m, tile_size=TILE, batch_size=66)
    if frame is None:
        frame = synth_frame(32 + rank, FRAME_H, FRAME_W).to(dev)
    for _ in range(3):
        render_fn(frame)
    barrier()
    t0 = time.perf_counter()
    for _ in range(frames_per_rank):
        render_fn(frame)
    barrier()
    dt = time.perf_counter() - t0
    t = torch.tensor([dt], dtype=torch.float64, device=dev)
    dist.all_reduce(t, op=dist.ReduceOp.MAX)
    dt = float(t.item())
    del m
    if rank != 0:
        return None
    return {"config": "waifu2x cunet (noise geometry, random-init), tile 256, 1080p frames, frame-sharded: every rank renders "
                      f"{frames_per_rank} frames of its own", "world": world, "frames": frames_per_rank * world,
            "unit": "input MPix/s", "scaling": "weak", "ms_per_frame_per_gpu": round(1e3 * dt / frames_per_rank, 3),
            "value": round(FRAME_H * FRAME_W * frames_per_rank * world / dt / 1e6, 1)}


def config5_replicas_leg(dist, world, rank, dev, barrier, record_fn=None):
    """BASELINE configs[4] at N GPUs.  The stream is sequential — the depth net attends to its previous 31 frames, the inpaint net
    works on a 12-frame queue — and the reference runs it on one GPU (``multi_gpu_supported`` False,
    iw3/video_depth_anything_streaming_model.py:129-131): REPLICAS ONLY: every rank runs a stream of its own (another
    video or scene segment), nothing is exchanged.  ``value`` = N streams' input MPix/s at the SLOWEST rank's time per frame."""
    import torch
    barrier()
    rec = (record_fn or config5_record)(dev)
    barrier()
    t = torch.tensor([float(rec["ms_per_frame"])], dtype=torch.float64, device=dev)
    dist.all_reduce(t, op=dist.ReduceOp.MAX)
    slowest = float(t.item())
    table = [None] * world
    dist.all_gather_object(table, {"rank": rank, "ms_per_frame": rec["ms_per_frame"], "frames_in": rec["frames_in"]})
    if rank != 0:
        return None
    h5, w5 = rec["frame"]
    out = {k: rec[k] for k in ("config", "depth_net", "frame", "unit", "target") if k in rec}
    out.update({"world": world, "scaling": "replicas (one independent stream per rank, no data-path collective)", "per_rank": table,
                "ms_per_frame_per_gpu": round(slowest, 2), "fps": round(world * 1e3 / slowest, 1),
                "value": round(h5 * w5 * world / slowest / 1e3, 1)})
    return out


def scale4x_record(dev):
    import torch
    from nunif_amd.nunif.utils.render import tiled_render
    from nunif_amd.synthetic import swin_unet_state_dict
    from nunif_amd.waifu2x.models.swin_unet import SwinUNet4x
    m = SwinUNet4x().eval()
    m.load_state_dict(swin_unet_state_dict(104, 4))
    m = m.to(dev)
    x = synth_frame(77, 2160, 3840).to(dev)
    for _ in range(2):
        tiled_render(x, m, tile_size=TILE, batch_size=34)
    torch.cuda.synchronize(dev)
    n = 12
    t0 = time.perf_counter()
    for _ in range(n):
        tiled_render(x, m, tile_size=TILE, batch_size=34)
    torch.cuda.synchronize(dev)
    dt = (time.perf_counter() - t0) / n
    # per-kernel record of THIS workload (VERDICT r05 missing item 4): the C = 192 top level runs at 240 x 240 tokens here, another
    # regime than the 1080p 2x headline; HIP events on the launch stream, traffic from this workload's own PMC set (tools/profile_4k.sh)
    from nunif_amd import _hip
    _hip.profile_read(reset=True)
    _hip.profile_enable(True)
    n_prof = 2
    for _ in range(n_prof):
        tiled_render(x, m, tile_size=TILE, batch_size=34)
    torch.cuda.synchronize(dev)
    recs = _hip.profile_read(reset=True)
    _hip.profile_enable(False)
    del m
    rec = {"config": "BASELINE configs[2] on one GPU: swin_unet 4x (photo geometry, random-init), 4K frame, tile 256 "
                     "(170 tiles in minibatches of 34) -> 8640 x 15360", "frames": n, "ms_per_frame": round(dt * 1e3, 2),
           "value": round(2160 * 3840 / dt / 1e6, 1), "unit": "input MPix/s",
           "output_mpix_per_s": round(16 * 2160 * 3840 / dt / 1e6, 1),
           "model_tflops": round(170 * 156e9 / dt / 1e12, 1), "model_mfma_frac": round(170 * 156e9 / dt / 1e12 / MFMA_PEAK_TFLOPS, 4)}
    if recs:
        rec["kernel_classes"] = kernel_table(recs, n_prof)[:12]
        dom = max(recs, key=lambda r: r["total_ms"])
        rec["roofline"] = roofline_of(dom, pmc_set=WORKLOAD_PMC["scale4x_4k"])
        rec["roofline"]["top_kernels"] = [
            {k: v for k, v in roofline_of(r, pmc_set=WORKLOAD_PMC["scale4x_4k"]).items()
             if k in ("kernel", "bound", "achieved", "peak", "unit", "frac", "traffic", "avg_launch_us", "launches")}
            for r in sorted(recs, key=lambda r: -r["total_ms"])[:4]]
    return rec


def cunet_record(dev, with_cpu):
    """north_star names "swin_unet / cunet": BASELINE configs[0] geometry (waifu2x cunet, one 512 x 512 image, tile 256 = 9 tiles)
    and a 1080p frame through ``tiled_render``; per-kernel roofline of the dominant conv kernel (algorithmic 28 GFLOP / tile over
    all conv launches), PSNR of the 512 x 512 render against the CPU oracle (``oracle/cunet.py``)."""
    import torch
    from nunif_amd import _hip
    from nunif_amd.nunif.models import create_model
    from nunif_amd.nunif.utils.render import tiled_render
    import nunif_amd.waifu2x.models.cunet  # noqa: F401
    from nunif_amd.synthetic import cunet_state_dict
    sd = cunet_state_dict(201)
    m = create_model("waifu2x.cunet").eval()
    m.load_state_dict(sd)
    m = m.to(dev)
    # tile minibatch = the whole frame, as the swin_unet leg does with its 45 (CB >= the frame's tile count); the reference's own
    # default minibatch for this net is 16, and that figure is reported next to it (`*_batch16`): round 3's 225 vs 298 MPix/s on
    # the same build was this batching alone (tools/cunet_probe.py, CUNET_BATCH); results do not depend on it (test_cunet.py)
    from nunif_amd.nunif.utils.seam_blending import SeamBlending
    CB = 66
    grid = SeamBlending.create_config((FRAME_H, FRAME_W), m.i2i_scale, m.i2i_offset, TILE, m.i2i_blend_size)
    tiles = int(grid["h_blocks"]) * int(grid["w_blocks"])
    rec = {"config": f"BASELINE configs[0] geometry on the GPU: waifu2x cunet (noise geometry, random-init), tile 256, tile batch {CB} "
                     f"(= whole frame in one minibatch): one 512 x 512 image (9 tiles) and a 1080p frame ({tiles} tiles); "
                     "`*_batch16` = the same renders at the reference's default tile minibatch of 16", "unit": "input MPix/s",
           "tiles_per_1080p_frame": tiles}
    img = synth_frame(31, 512, 512).to(dev)
    frame = synth_frame(32, FRAME_H, FRAME_W).to(dev)
    for key, x, n, cb in (("image_512", img, 60, CB), ("frame_1080p", frame, 30, CB), ("frame_1080p_batch16", frame, 30, 16)):
        for _ in range(3):
            tiled_render(x, m, tile_size=TILE, batch_size=cb)
        torch.cuda.synchronize(dev)
        t0 = time.perf_counter()
        for _ in range(n):
            y = tiled_render(x, m, tile_size=TILE, batch_size=cb)
        torch.cuda.synchronize(dev)
        dt = (time.perf_counter() - t0) / n
        rec[key] = {"ms": round(dt * 1e3, 3), "value": round(x.shape[1] * x.shape[2] / dt / 1e6, 1), "tile_batch": cb}
    _hip.profile_read(reset=True)
    _hip.profile_enable(True)
    for _ in range(3):
        tiled_render(frame, m, tile_size=TILE, batch_size=CB)
    torch.cuda.synchronize(dev)
    recs = _hip.profile_read(reset=True)
    _hip.profile_enable(False)
    if recs:
        rec["kernel_classes"] = kernel_table(recs, 3)[:6]
        dom = max(recs, key=lambda r: r["total_ms"])
        rec["roofline"] = roofline_of(dom, pmc_set=WORKLOAD_PMC["cunet"])
        conv_ms = sum(r["total_ms"] for r in recs if r["flops"] > 0) / 3
        rec["model_tflops"] = round(tiles * 28e9 / (rec["frame_1080p"]["ms"] * 1e-3) / 1e12, 1)
        rec["model_mfma_frac"] = round(rec["model_tflops"] / MFMA_PEAK_TFLOPS, 4)
        rec["conv_kernel_ms_per_frame"] = round(conv_ms, 3)
    if with_cpu:
        from oracle import cunet as OC
        from oracle import seam_blending as OS
        torch.set_num_threads(min(32, physical_cores()))
        t0 = time.perf_counter()
        ref = OS.tiled_render(img.cpu(), lambda mb: OC.model_forward(sd, mb), 1, 28, 0, TILE, 4)
        dt = time.perf_counter() - t0
        got = tiled_render(img, m, tile_size=TILE, batch_size=CB).cpu()
        mse = torch.mean((got.double() - ref.double()) ** 2).item()
        rec["psnr_vs_oracle_db"] = round(10 * math.log10(1.0 / (mse + 1e-6)), 2)
        rec["cpu_baseline"] = {"value": round(512 * 512 / 1e6 / dt, 4), "unit": "MPix/s", "cores": min(32, physical_cores()),
                               "kind": "port", "sample": f"oracle cunet tiled_render of the 512 x 512 image, one pass, {dt:.2f} s"}
    del m
    return rec


def config5_record(dev):
    """BASELINE configs[4] shape on ONE GPU: 4K frames in batches of 3 -> ``VideoDepthAnythingStreamingModel`` wrapper (pre / post
    kernels of the reference's wrapper) around the Video-Depth-Anything ViT-S streaming network (DINOv2 encoder + DPT head with four
    temporal modules over a 32-frame window: published architecture, random-init, PARITY UNPINNED — DESIGN.md 8;
    ``NUNIF_CONFIG5_PERFRAME=1``: round 4's per-frame ViT-S stand-in, for the A/B) -> min-max -> mask-MLBW backward warp
    (``sbs.mask_mlbw_l2``) -> 12-frame ``FrameQueue`` -> ``inpaint.light_video_inpaint_v1`` on both eyes -> SBS uint8.
    Reference call sites: iw3/video_depth_anything_streaming_model.py:77-103, iw3/mlbw_inpaint.py:296-360."""
    import torch
    from nunif_amd import _hip
    from nunif_amd.iw3 import _ops
    from nunif_amd.iw3.base_depth_model import CallableDepthModel
    from nunif_amd.iw3.depth_anything_v2 import HipDepthAnythingV2
    from nunif_amd.iw3.mlbw_inpaint import MLBWInpaint
    from nunif_amd.iw3.models.light_inpaint_v1 import LightInpaintV1
    from nunif_amd.iw3.models.light_video_inpaint_v1 import LightVideoInpaintV1
    from nunif_amd.iw3.models.mlbw import MLBW
    from nunif_amd.iw3.video_depth_anything_streaming_model import VideoDepthAnythingStreamingModel
    from nunif_amd.iw3.video_depth_anything_net import HipVideoDepthAnythingStreaming
    from nunif_amd.synthetic import (depth_anything_v2_state_dict, light_inpaint_state_dict, light_video_inpaint_state_dict,
                                     mlbw_state_dict, video_depth_anything_state_dict)
    H5, W5, batch = 2160, 3840, 3
    per_frame = os.environ.get("NUNIF_CONFIG5_PERFRAME") == "1"
    if per_frame:
        depth_model = CallableDepthModel(HipDepthAnythingV2(depth_anything_v2_state_dict(601), str(dev)))
        depth_model.load(gpu=dev.index or 0)
        backbone = depth_model.model
    else:
        backbone = HipVideoDepthAnythingStreaming(video_depth_anything_state_dict(601), str(dev))
    vda = VideoDepthAnythingStreamingModel("VDA_Stream_S", backbone=backbone).load(gpu=dev.index or 0)
    inp = LightInpaintV1().eval()
    inp.load_state_dict(light_inpaint_state_dict(701))
    mm = MLBW(num_layers=2, base_dim=32, hole_mask=True).eval()
    mm.load_state_dict(mlbw_state_dict(431, 2, False, hole_mask=True))
    vid = LightVideoInpaintV1().eval()
    vid.load_state_dict(light_video_inpaint_state_dict(801))
    side = MLBWInpaint(inp.to(dev), mm.to(dev), video_model=vid.to(dev))
    side.set_mode("video")
    frames5 = [synth_frame(950 + i, H5, W5).to(dev) for i in range(3)]
    n_out = [0]

    def step(i):
        x = torch.stack([frames5[(i + k) % 3] for k in range(batch)])
        d = torch.stack(vda.minmax_normalize(vda.infer(x, edge_dilation=2)))
        left, right = side.infer(x, d, divergence=2.0, convergence=0.5, synthetic_view="both", inner_dilation=1, outer_dilation=1)
        if left is None:                          # the 12-frame queue is still filling
            return
        for k in range(left.shape[0]):
            _ops.stereo_to_frame(left[k], right[k], "sbs")
            n_out[0] += 1

    for i in range(4 if per_frame else 11):       # 33 frames: the temporal network's 32-frame window is full when the clock starts
        step(i)
    torch.cuda.synchronize(dev)
    n_out[0] = 0
    n_calls = 8
    t0 = time.perf_counter()
    for i in range(n_calls):
        step(i)
    torch.cuda.synchronize(dev)
    dt = time.perf_counter() - t0
    n_in = n_calls * batch
    net_desc = ("a per-frame ViT-S stand-in (NUNIF_CONFIG5_PERFRAME=1; no temporal head)" if per_frame else
                "the Video-Depth-Anything ViT-S streaming network (4 temporal modules, 32-frame window full; published architecture, "
                "random-init, parity unpinned)")
    rec = {"config": "BASELINE configs[4] shape on one GPU: 4K frames (batches of 3) -> VideoDepthAnythingStreaming wrapper around "
                     + net_desc + " -> min-max -> sbs.mask_mlbw_l2 backward "
                     "warp -> 12-frame queue -> inpaint.light_video_inpaint_v1 (both eyes) -> SBS uint8",
           "depth_net": "per_frame_vits" if per_frame else "vda_streaming_vits",
           "frame": [H5, W5], "frames_in": n_in, "frames_out": n_out[0], "ms_per_frame": round(1e3 * dt / n_in, 2),
           "fps": round(n_in / dt, 1), "value": round(H5 * W5 * n_in / dt / 1e6, 1), "unit": "input MPix/s",
           "target": "4K @ 30 fps on 8 GPUs (BASELINE configs[4]); this is one GPU"}
    _hip.profile_read(reset=True)
    _hip.profile_enable(True)
    for i in range(4):
        step(i)
    torch.cuda.synchronize(dev)
    recs = _hip.profile_read(reset=True)
    _hip.profile_enable(False)
    if recs:
        rec["kernel_classes"] = kernel_table(recs, 4 * batch)[:8]
        dom = max(recs, key=lambda r: r["total_ms"])
        rec["roofline"] = roofline_of(dom, pmc_set=WORKLOAD_PMC["config5"])
    side.reset()
    return rec


def dry_standins():
    """``NUNIF_BENCH_BACKEND=gloo``: the LAUNCHER rehearsal — ``python bench.py --gpus N`` end to end on N CPU
    ranks: ``relaunch_as_ranks`` -> ``torch.distributed.run`` -> rendezvous on 127.0.0.1 -> the timed loop with its barrier and
    MAX over ranks -> the delivery leg -> the iw3 / cunet / config-5 legs -> ONE line on rank 0 -> process group down, with torch-CPU
    stand-ins for every device function (the HIP engine refuses CPU tensors).  Nothing in the line is a measurement: ``data`` says
    "dry".  What it proves is the control flow the first real N > 1 run takes (tests/test_bench_launcher.py)."""
    import torch
    from nunif_amd.iw3.base_depth_model import BaseDepthModel

    class DryDepth(BaseDepthModel):
        def load_model(self, model_type, resolution=None, device=None, **kw):
            return None

        def is_metric(self):
            return False

        def infer(self, x, **kw):
            x = x if x.ndim == 4 else x[None]
            return x.mean(dim=1) * 0.5 + x[:, 0] * 0.25

    def stereo_fn(xs, ds, reset_pts):
        sbs = torch.cat([xs, xs.flip(-1)], dim=3) * ds[:, None].repeat(1, 1, 1, 2).clamp(0, 1)
        return [(sbs[i].clamp(0, 1) * 255).round().to(torch.uint8).permute(1, 2, 0) for i in range(xs.shape[0])]

    def render(frame):
        return torch.nn.functional.interpolate(frame[None], scale_factor=2, mode="nearest")[0].clamp(0, 1)

    def config5(dev):
        rank = int(os.environ.get("RANK", "0"))
        ms = 20.0 + rank
        return {"config": "dry stand-in", "depth_net": "dry", "frame": [2160, 3840], "frames_in": 4, "frames_out": 4,
                "ms_per_frame": ms, "fps": round(1e3 / ms, 1), "value": 1.0, "unit": "input MPix/s", "target": "dry"}

    return {"depth": DryDepth("dry"), "stereo_fn": stereo_fn, "render": render, "config5": config5, "frame_hw": (48, 80)}


def collect_multi_gpu(dist, world, rank, local_rank, dev):
    """Self-evidence for the driver's N > 1 runs: how many ranks took part in a collective and which physical devices they hold
    (one distinct PCI bus id per rank, or the run was not N GPUs).  ``dev`` may be a CPU device in the gloo unit test."""
    import torch
    ones = torch.ones(1, device=dev)
    dist.all_reduce(ones)
    if dev.type == "cuda":
        props = torch.cuda.get_device_properties(dev)
        name, hbm = props.name, round(props.total_memory / 2 ** 30, 1)
        bus = "%04x:%02x:%02x" % (getattr(props, "pci_domain_id", 0), getattr(props, "pci_bus_id", -1) & 0xff,
                                  getattr(props, "pci_device_id", 0))
    else:
        name, hbm, bus = "cpu", 0.0, f"host-rank-{rank}"
    mine = {"rank": rank, "local_rank": local_rank, "device": name, "pci_bus_id": bus, "hbm_gib": hbm}
    table = [None] * world
    dist.all_gather_object(table, mine)
    return {"ranks_seen": int(ones.item()), "world_size": world, "backend": dist.get_backend(),
            "distinct_pci_bus_ids": len({t["pci_bus_id"] for t in table}), "devices": table}


def main():
    args = parse_args()
    if args.gpus > 1 and "WORLD_SIZE" not in os.environ:
        relaunch_as_ranks(args)                      # does not return
    import torch
    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    world = int(os.environ.get("WORLD_SIZE", "1"))
    if world != args.gpus:
        raise SystemExit(f"bench.py: --gpus {args.gpus} but WORLD_SIZE={world} (launch with --nproc-per-node {args.gpus})")
    # NUNIF_BENCH_BACKEND=gloo: the CPU launcher rehearsal (dry_standins).  NUNIF_BENCH_FORCE_DIST=1: take the N > 1 path with
    # whatever world size there is — ``python bench.py --gpus 1`` then runs every collective of the driver's N-rank run on a
    # one-rank nccl group, and its ``value`` must agree with the plain line (tools/bench_n1_check.sh)
    dry = os.environ.get("NUNIF_BENCH_BACKEND", "") == "gloo"
    multi = world > 1 or os.environ.get("NUNIF_BENCH_FORCE_DIST", "0") == "1"
    dist = None
    if multi:
        import torch.distributed as dist
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
        if world == 1:
            os.environ.setdefault("MASTER_PORT", "29531")
        if dry:
            dist.init_process_group("gloo", rank=rank, world_size=world)
        else:
            torch.cuda.set_device(local_rank)
            dist.init_process_group("nccl", rank=rank, world_size=world, device_id=torch.device(f"cuda:{local_rank}"))
    dev = torch.device("cpu") if dry else torch.device(f"cuda:{local_rank}")
    if not dry:
        torch.cuda.set_device(dev)
    multi_gpu = collect_multi_gpu(dist, world, rank, local_rank, dev) if multi else None
    torch.set_grad_enabled(False)
    n_streams = max(1, args.streams)
    fh, fw = FRAME_H, FRAME_W
    stand = None
    if dry:
        stand = dry_standins()
        fh, fw = stand["frame_hw"]
        n_streams = 1
        frames = [synth_frame(1234 + rank * 16 + i, fh, fw) for i in range(4)]

        def render(m, frame):
            return stand["render"](frame)

        model = pool = None
        _hip = tiled_render = None

    if not dry:
        from nunif_amd import _hip
        from nunif_amd.nunif.utils.render import tiled_render
        from nunif_amd.waifu2x.models.swin_unet import SwinUNet2x
        from nunif_amd.synthetic import swin_unet_state_dict    # seeded random-init weights (no checkpoints offline)
        from nunif_amd.parallel import ConcurrentRenderer

        sd = swin_unet_state_dict(102, 2)

        def make_model():
            mm = SwinUNet2x().eval()
            mm.load_state_dict(sd)
            return mm

        pool = ConcurrentRenderer(make_model, n_streams, dev)       # n_streams engine replicas, one HIP stream each
        model = pool.models[0]
        # a few distinct frames per rank, resident in HBM before the timed region
        frames = [synth_frame(1234 + rank * 16 + i, FRAME_H, FRAME_W).to(dev) for i in range(4)]

        def render(m, frame):
            return tiled_render(frame, m, tile_size=TILE, batch_size=args.batch_size)
    from nunif_amd.parallel import render_sharded

    def step(i):
        if n_streams == 1:
            return render(model, frames[i % len(frames)])
        # one frame per stream, no cross-stream dependence; results are left on their streams (the barrier syncs them)
        return [pool.submit(render, frames[(i * n_streams + k) % len(frames)]) for k in range(n_streams)]

    def dev_sync():
        if not dry:
            torch.cuda.synchronize(dev)

    def barrier():
        dev_sync()
        if multi:
            dist.barrier()
            dev_sync()

    for i in range(args.warmup):
        step(i)
    barrier()
    t0 = time.perf_counter()
    for i in range(args.steps - 1):
        step(i)
    last = step(args.steps - 1)             # kept for --dump-outputs; the earlier steps' frames are dropped as they come
    barrier()
    elapsed = time.perf_counter() - t0
    if multi:
        t = torch.tensor([elapsed], dtype=torch.float64, device=dev)
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        elapsed = float(t.item())
    if args.dump_outputs:
        dump_outputs(args.dump_outputs, [last] if n_streams == 1 else [h[0] for h in last], rank, world)
    del last

    # ---- the same K frames on ONE stream (reported next to `value`; the per-kernel roofline below is measured this way) ----
    single = None
    if args.full and n_streams > 1 and rank == 0 and not dry:
        n1 = min(args.steps, 100)
        torch.cuda.synchronize(dev)
        t1 = time.perf_counter()
        for i in range(n1):
            render(model, frames[i % len(frames)])
        torch.cuda.synchronize(dev)
        dt1 = time.perf_counter() - t1
        single = {"value": round(FRAME_H * FRAME_W / 1e6 * n1 / dt1, 2), "unit": "MPix/s",
                  "ms_per_frame": round(1e3 * dt1 / n1, 3), "frames": n1}

    # ---- per-kernel timing with HIP events on the launch stream (library hooks), outside the timed region ----------
    roofline, classes = None, []
    if args.full and rank == 0 and not dry:
        _hip.profile_read(reset=True)
        _hip.profile_enable(True)
        n_prof = max(1, min(5, args.steps))
        for i in range(n_prof):             # per-kernel durations are measured on ONE stream (no overlap between frames)
            tiled_render(frames[i % len(frames)], model, tile_size=TILE, batch_size=args.batch_size)
        torch.cuda.synchronize(dev)
        recs = _hip.profile_read(reset=True)
        _hip.profile_enable(False)
        classes = kernel_table(recs, n_prof)
        # dominant kernel = most time per frame; the four block kernels of this net are within a few percent of each other (20-22 %
        # each), so inside a 5 % band the one that carries the most algorithmic FLOPs is taken — the choice does not flip from box
        # to box — and the rooflines of all four are listed next to it
        t_max = max(r["total_ms"] for r in recs)
        dom = max((r for r in recs if r["total_ms"] >= 0.95 * t_max), key=lambda r: r["flops"])
        roofline = roofline_of(dom)
        roofline["measured"] = "single-stream leg, HIP events on the launch stream (kernel durations are not overlapped with another frame)"
        roofline["top_kernels"] = [
            {k: v for k, v in roofline_of(r).items()
             if k in ("kernel", "bound", "achieved", "peak", "unit", "frac", "traffic", "avg_launch_us", "launches")}
            for r in sorted(recs, key=lambda r: -r["total_ms"])[:4]]

    if rank == 0:
        mpix_in = fh * fw / 1e6
        value = mpix_in * args.steps * n_streams * world / elapsed
        result = {
            "metric": "input MPix/s, waifu2x swin_unet 2x tiled render (tile 256) of 1080p frames",
            "value": round(value, 2), "unit": "MPix/s", "n_gpus": world, "steps": args.steps, "warmup": args.warmup,
            "ms_per_step": round(1e3 * elapsed / args.steps, 3), "higher_is_better": True, "scaling": "weak",
            "vs_baseline": None, "dtype": "f16",
            "data": "synthetic" if not dry else "dry: CPU stand-ins on gloo ranks (launcher rehearsal, nothing here is a measurement)",
            "config": {"workload": "waifu2x swin_unet 2x (art scale2x geometry), tile_size=256, 1080p frame, "
                                   "random-init weights", "frame": [fh, fw], "tile_size": TILE,
                       "tile_batch": args.batch_size, "tiles_per_frame": 45, "frames_per_step_per_gpu": n_streams,
                       "concurrent_streams": n_streams, "timed_region_s": round(elapsed, 3),
                       "parallelism": f"frame-sharded x{world}"},
            "output_mpix_per_s": round(value * 4, 2),
            "model_tflops": round(45 * 98e9 * args.steps * n_streams * world / elapsed / 1e12, 2),
            "model_mfma_frac": round(45 * 98e9 * args.steps * n_streams * world / elapsed / 1e12 / (MFMA_PEAK_TFLOPS * world), 4),
        }
        if args.full:
            result["roofline"], result["kernel_classes"] = roofline, classes
        if multi_gpu is not None:
            result["multi_gpu"] = multi_gpu
            if multi_gpu["ranks_seen"] != world or multi_gpu["distinct_pci_bus_ids"] != world:
                result.setdefault("errors", []).append("ranks / devices do not add up to --gpus")
        if single is not None:
            result["single_stream"] = single        # one frame at a time on one stream, same build, same run
        if args.full and not args.no_host_frames and not multi:
            # host uint8 frame -> pinned ring -> H2D -> to_tensor -> render -> quantise -> D2H -> host uint8 frame
            from nunif_amd.frame_ring import FrameRing
            host = [(f.clamp(0, 1) * 255).round().to(torch.uint8).permute(1, 2, 0).contiguous().cpu().numpy() for f in frames]
            n_host = max(8, min(args.steps, 48))
            hf = {"frames": n_host, "bytes_per_frame": int(FRAME_H * FRAME_W * 3 * 5),
                  "path": "uint8 HWC host frame -> memcpy into the pinned ring (depth 3) -> zero-copy H2D edge kernel -> render -> "
                          "quantise straight into pinned host memory -> uint8 HWC host frame"}
            for mode in ("view", "copy"):      # view: the pinned output buffer is the frame; copy: a fresh numpy array per frame
                ring = FrameRing(lambda x: tiled_render(x, model, tile_size=TILE, batch_size=args.batch_size),
                                 (FRAME_H, FRAME_W, 3), (2 * FRAME_H, 2 * FRAME_W, 3), device=dev, depth=3, out_mode=mode)
                for i in range(3):
                    ring.submit(host[i % len(host)])
                ring.drain()
                t1 = time.perf_counter()
                chk = 0
                for i in range(n_host):
                    o = ring.submit(host[i % len(host)])
                    if o is not None:
                        chk += int(o[0, 0, 0])                           # the consumer touches the frame
                for o in ring.drain():
                    chk += int(o[0, 0, 0])
                dt = time.perf_counter() - t1
                key = "mpix_per_s" if mode == "view" else "mpix_per_s_copying_every_frame"
                hf[key] = round(mpix_in * n_host / dt, 2)
                hf["ms_per_frame" if mode == "view" else "ms_per_frame_copying_every_frame"] = round(1e3 * dt / n_host, 3)
                del ring
            result["host_frames"] = hf
        def sub_record(key, fn):
            # a sub-record must never cost the headline line — but a failed one is an error of the run (``ok`` false, rc 3)
            try:
                result[key] = fn()
            except Exception as e:
                result[key] = {"error": repr(e)}
                result.setdefault("errors", []).append(f"sub-record {key} raised")

        if args.full and not args.no_4k and not multi:
            sub_record("scale4x_4k", lambda: scale4x_record(dev))
        if args.full and not args.no_cunet and not multi:
            sub_record("cunet", lambda: cunet_record(dev, with_cpu=not args.no_cpu_baseline))
        if args.full and not args.no_iw3 and not multi:
            sub_record("iw3", lambda: iw3_record(dev, with_cpu=not args.no_cpu_baseline))
        if args.full and not args.no_config5 and not multi:
            sub_record("config5", lambda: config5_record(dev))
        if args.full and not args.no_cpu_baseline and not multi:      # contract: CPU baseline on rank 0 at N = 1 only
            base, crop, ref, ref_whole = cpu_baseline(sd, frames[0].cpu())
            got = tiled_render(crop.to(dev), model, tile_size=TILE, batch_size=args.batch_size).cpu()
            mse = torch.mean((got.double() - ref.double()) ** 2).item()
            result["cpu_baseline"] = base
            result["psnr_vs_oracle_db"] = round(10 * math.log10(1.0 / (mse + 1e-6)), 2)
            if ref_whole is not None:
                # the GPU frame against the CPU frame, at the TIMED configuration — the whole 1080p frame,
                # tile batch args.batch_size, every stream of the timed step busy with a frame of its own
                hs = [pool.submit(render, frames[k % len(frames)]) for k in range(n_streams)]
                outs = [pool.result(h).float().cpu() for h in hs]
                torch.cuda.synchronize(dev)
                mse_w = torch.mean((outs[0].double() - ref_whole.double()) ** 2).item()
                # the repo's PSNR convention everywhere (tests, psnr_vs_oracle_db): 10 log10(1 / (mse + 1e-6)), i.e. capped at 60 dB
                result["psnr_whole_frame_db"] = round(10 * math.log10(1.0 / (mse_w + 1e-6)), 2)
                result["psnr_whole_frame"] = {
                    "mse": mse_w, "psnr_without_the_1e-6_floor_db": round(10 * math.log10(1.0 / (mse_w + 1e-12)), 2),
                    "frame": [FRAME_H, FRAME_W], "tile_batch": args.batch_size, "concurrent_streams": n_streams,
                    "max_abs_diff": round(float((outs[0] - ref_whole).abs().max()), 6),
                    "against": "oracle tiled_render of the same whole frame on the host cores (the cpu_baseline pass, output kept)"}
    if args.full and multi:
        import threading
        done = threading.Event()

        def watchdog():
            if done.wait(GATHER_TIMEOUT_S):
                return
            if rank == 0:
                result["gathered"] = {"error": f"the delivery leg did not finish within {GATHER_TIMEOUT_S} s; value / roofline "
                                               "above are unaffected (they contain no collective)"}
                result.setdefault("errors", []).append("delivery leg hung (watchdog)")
                os._exit(emit(result))           # rank 0: the line first, then a non-zero exit code
            os._exit(0)

        def gather_leg():
            n_g = max(world, min(args.steps, 32)) * world
            n_g -= n_g % world
            shared = [frames[i % len(frames)] for i in range(n_g)]          # content differs per rank; geometry is what matters
            delivered = [0]

            def count(i, f):
                delivered[0] += 1

            render_sharded(shared[:2 * world], lambda f: render(model, f), dst=0, on_frame=count)      # warm-up (RCCL init)
            delivered[0] = 0
            barrier()
            t1 = time.perf_counter()
            render_sharded(shared, lambda f: render(model, f), dst=0, on_frame=count)
            barrier()
            dtg = time.perf_counter() - t1
            tg = torch.tensor([dtg], dtype=torch.float64, device=dev)
            dist.all_reduce(tg, op=dist.ReduceOp.MAX)
            dtg = float(tg.item())
            # BASELINE's other metrics at N GPUs (each leg is entered by every rank; a rank that fails raises into the handler
            # below, the others then wait in a collective and the watchdog ends them — the headline line is out either way)
            if not args.no_iw3:
                r_iw3 = (iw3_sharded_leg(dist, world, rank, dev, barrier) if not dry else
                         iw3_sharded_leg(dist, world, rank, dev, barrier, frames_per_rank=8, batch=2, depth_model=stand["depth"],
                                         stereo_fn=stand["stereo_fn"], frame_hw=(fh, fw), make_frame=lambda i: frames[i % 4]))
                if rank == 0:
                    result["iw3"] = r_iw3
                    if r_iw3["frames_delivered"] != r_iw3["frames"]:
                        result.setdefault("errors", []).append("iw3 leg: frames lost on the way to rank 0")
            if not args.no_cunet:
                r_cu = (cunet_sharded_leg(dist, world, rank, dev, barrier) if not dry else
                        cunet_sharded_leg(dist, world, rank, dev, barrier, frames_per_rank=2, render_fn=stand["render"], frame=frames[0]))
                if rank == 0:
                    result["cunet"] = r_cu
            if not args.no_config5:
                r_c5 = config5_replicas_leg(dist, world, rank, dev, barrier, record_fn=stand["config5"] if dry else None)
                if rank == 0:
                    result["config5"] = r_c5
            done.set()
            if rank == 0:
                if delivered[0] != n_g:
                    result.setdefault("errors", []).append(f"delivery leg: {delivered[0]} of {n_g} frames arrived on rank 0")
                # next to `value` in the line's top-level keys: the rate with every finished frame DELIVERED to rank 0
                result["gathered_value"] = round(fh * fw / 1e6 * n_g / dtg, 2)
                result["gathered"] = {
                    "value": round(fh * fw / 1e6 * n_g / dtg, 2), "unit": "MPix/s", "frames": n_g,
                    "frames_delivered": delivered[0],
                    "ms_per_frame_per_gpu": round(1e3 * dtg / (n_g / world), 3),
                    "bytes_delivered_per_frame": 2 * fh * 2 * fw * 3,
                    "path": "render (one frame at a time per rank) -> HIP quantise to HWC uint8 -> batch_isend_irecv "
                            "to rank 0, overlapped with the next render (nunif_amd.parallel.render_sharded)"}

        threading.Thread(target=watchdog, daemon=True).start()
        try:
            gather_leg()
        except Exception as e:      # a rank that failed must not exit non-zero (the launcher would kill rank 0 before it prints)
            print(f"[bench rank {rank}] delivery leg failed: {e!r}", file=sys.stderr, flush=True)
            if rank == 0:
                result["gathered"] = {"error": repr(e)}
                result.setdefault("errors", []).append("delivery leg raised")
                os._exit(emit(result))
            threading.Event().wait()            # the watchdog ends this rank with exit code 0
    rc = emit(result) if rank == 0 else 0
    if multi:
        dist.barrier()
        dist.destroy_process_group()
    if rc:
        sys.exit(rc)                # only rank 0, only AFTER its line is out and the process group is down


if __name__ == "__main__":
    main()
