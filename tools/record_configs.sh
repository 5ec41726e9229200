#!/bin/bash
# the bench line at the non-default single-GPU configurations: 3 runs each, the median run's JSON is kept (the boxes are shared:
# single runs swing by 2x when neighbours saturate the host CPUs)
R=${GRAFT_REPO_ROOT:-/root/repo}
O=$R/gpurun_out/prof_r2
mkdir -p $O
cd /tmp && export TMPDIR=/tmp
rec() {  # name, args...
  name=$1; shift
  for i in 1 2 3; do timeout 400 python $R/bench.py "$@" > /tmp/rec_$i.json 2>/dev/null; done
  python - "$O/$name.json" <<'PY'
import json, sys
runs = []
for i in (1, 2, 3):
    try:
        line = open("/tmp/rec_%d.json" % i).read().strip().splitlines()[-1]
        runs.append((json.loads(line)["value"], line))
    except Exception:
        pass
runs.sort()
v, line = runs[len(runs) // 2]
d = json.loads(line)
d["runs_samples_per_s"] = [r[0] for r in runs]
open(sys.argv[1], "w").write(json.dumps(d) + "\n")
print(sys.argv[1].split("/")[-1], [r[0] for r in runs])
PY
}
echo "loadavg $(cut -d' ' -f1-3 /proc/loadavg)"
rec r2_bench_r101 --config r101 --steps 30 --full --no-cpu-baseline
rec r2_bench_openocc_f32 --config openocc --steps 10 --warmup 2 --full
rec r2_bench_openocc_bf16 --config openocc --dtype bf16 --steps 10 --warmup 2 --full
rec r2_bench_stress200 --config stress200 --steps 6 --warmup 1 --full --no-cpu-baseline
