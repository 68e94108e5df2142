#!/bin/bash
# per-kernel-class time per frame at several tile batches (single stream): does a working set inside the 256 MB memory-side
# cache make the level-1 (C = 96) kernels faster per token?
#     bash tools/batch_sweep.sh <out dir>
OUT=${1:?usage: bash tools/batch_sweep.sh <out dir>}
mkdir -p "$OUT"
for b in ${BATCHES:-45 15 9 5}; do
  python bench.py --full --steps 12 --warmup 3 --no-cpu-baseline --no-host-frames --no-iw3 --no-4k --streams 1 --batch-size $b > "$OUT/bs_$b.json" 2> "$OUT/bs_$b.err"
  python - "$OUT/bs_$b.json" <<PY
import json, sys
r=json.loads(open(sys.argv[1]).read().strip().splitlines()[-1])
print("batch $b  MPix/s", r["value"], " ms/frame", r["ms_per_step"])
for c in r["kernel_classes"][:8]:
    print("    %-40s launches/frame %4d avg_us %8.1f  per-frame ms %.3f  TF %.0f GB/s %.0f" % (c["kernel"][:40], c["launches_per_frame"], c["avg_us"], c["avg_us"] * c["launches_per_frame"] * 1e-3, c["tflops"], c["gbs"]))
PY
done
