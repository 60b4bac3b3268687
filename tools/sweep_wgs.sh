#!/bin/bash
# Sweep the accumulate kernel's workgroup-count target (SECEDO_TARGET_WGS) on one workload.
wl=${1:-C2}; shift
for w in "$@"; do
  line=$(SECEDO_TARGET_WGS=$w python bench.py --workload $wl --steps 20 --warmup 3 --full --no-cpu-baseline 2>/dev/null)
  python - "$w" "$line" <<'PY'
import json, sys
d = json.loads(sys.argv[2])
print("target_wgs", sys.argv[1], "ms/step %.4f kernel_ms %.4f frac %.3f" % (d["ms_per_step"], d["roofline"]["kernel_ms"], d["roofline"]["frac"]))
PY
done
