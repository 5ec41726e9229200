"""Time the LiDAR-only trunk (SECOND3D + SECOND3DFPN, eval mode) at the size of projects/configs/coocc_nusc/coocc_lidar.py
([1,128,8,100,100], layer_nums [5,5,5], seeded weights) on the HIP engine against the torch restatement of
tests/ref_second3d.py on the same GPU in fp32 (MIOpen; ``torch.backends.cudnn.benchmark`` left at its default) -- what a user of
that config had before by injecting torch modules.

    python tools/bench_lidar_trunk.py [--calls 50] [--warmup 10] [--windows 3] [--out profiles/lidar_trunk_bench.json]
    python tools/bench_lidar_trunk.py --only hip --calls 5      # the program to put after `rocprofv3 --kernel-trace --stats --`

Same process, alternating windows: HIP events around ``calls`` calls after ``warmup`` calls, ``windows`` windows per side, median.
Prints one JSON line; ratio = baseline / HIP per window (>= 1.0: the HIP trunk is at least as fast).  Needs the GPU: no fallback."""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--windows", type=int, default=3)
    ap.add_argument("--only", choices=["hip", "torch"], default=None)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_lidar_trunk needs the MI355X: there is no CPU fallback")
    from co_occ_amd import core, lidar_trunk as lt, registry, synth
    import ref_second3d
    dev = torch.device("cuda:0")
    c = synth.SECOND3D_CASES["full"]
    bcfg, ncfg = synth.second3d_cfg(c["layer_nums"])
    b, n = registry.BACKBONES.build(bcfg), registry.NECKS.build(ncfg)
    sdb, sdn = synth.second3d_weights(b, n, c["seed"])
    b.load_state_dict(sdb), n.load_state_dict(sdn)
    b, n = b.to(dev).eval(), n.to(dev).eval()
    rb, rn = ref_second3d.build(bcfg, ncfg, sdb, sdn)
    rb, rn = rb.to(dev), rn.to(dev)
    x = synth.second3d_input(c["grid_zyx"], seed=c["seed"]).to(dev)

    def hip():
        return lt.run_trunk(b, n, x).t

    def base():
        return rn(list(rb(x)))

    def window(fn):
        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        s.record()
        for _ in range(a.calls):
            fn()
        e.record()
        torch.cuda.synchronize()
        return s.elapsed_time(e) / a.calls

    sides = [("hip", hip), ("torch", base)] if a.only is None else [(a.only, hip if a.only == "hip" else base)]
    ms = {k: [] for k, _ in sides}
    with torch.no_grad():
        if a.only is None:
            err = float((hip().view(100, 100, 8, 128).permute(3, 2, 1, 0) - base()[0]).abs().max() / base().abs().max())
        for _, fn in sides:
            for _ in range(a.warmup):
                fn()
        torch.cuda.synchronize()
        for _ in range(a.windows):
            for k, fn in sides:
                ms[k].append(window(fn))
    core.check_h2_overflow()
    med = lambda v: sorted(v)[len(v) // 2]
    res = dict(workload="coocc_lidar trunk [1,128,8,100,100] layer_nums [5,5,5]", engine=core.CONV_ENGINE, calls=a.calls,
               warmup=a.warmup, ms_per_call={k: [round(t, 4) for t in v] for k, v in ms.items()},
               median_ms={k: round(med(v), 4) for k, v in ms.items()}, direct_form_gflop=626.0)
    if a.only is None:
        res["ratio_per_window"] = [round(t / h, 3) for h, t in zip(ms["hip"], ms["torch"])]
        res["max_rel_diff_vs_torch"] = err
        res["at_least_as_fast_in_every_window"] = all(r >= 1.0 for r in res["ratio_per_window"])
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
