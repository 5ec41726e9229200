"""Time one training step (forward + backward) of the LiDAR-only trunk -- SECOND3D + SECOND3DFPN under ``train()``,
``lidar_trunk.run_trunk_train`` -- at the size of projects/configs/coocc_nusc/coocc_lidar.py ([1,128,8,100,100], layer_nums
[5,5,5], seeded weights) against torch-ROCm autograd of the plain ``nn`` restatement (tests/ref_second3d.py: nn.Conv3d /
nn.ConvTranspose3d / nn.BatchNorm3d through MIOpen, fp32) on the same GPU, and the parts alone from the package's per-launch
event timer: the strided data gradients by residue class, ``k_wgrad`` on the 3x3x1 layers, and ``coocc_fpn_sum_bwd`` as a share of
the HBM roofline computed from its bytes.

    python tools/bench_trunk_train.py [--steps 20] [--warmup 5] [--windows 5] [--out profiles/trunk_train_bench.json]
                                      [--kernels profiles/trunk_train_kernels.txt]
    python tools/bench_trunk_train.py --only hip --steps 3      # the program to put after `rocprofv3 --kernel-trace --stats --`

Same process, alternating windows: HIP events around ``steps`` steps after ``warmup`` steps, ``windows`` windows per side; median
and min / max per side, ratio = torch / HIP per window.  The parts come from a separate pass with the event timer on (every timed
launch costs an event pair: that pass is not the step time).  Prints one JSON line.  Needs the GPU: no fallback."""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

HBM_PEAK = 8.0e12          # bytes / s, MI355X HBM3E


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--only", choices=["hip", "torch"], default=None)
    ap.add_argument("--out", default=None)
    ap.add_argument("--kernels", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_trunk_train needs the MI355X: there is no CPU fallback")
    from co_occ_amd import core, lidar_trunk as lt, registry, synth
    import ref_second3d
    dev = torch.device("cuda:0")
    c = synth.SECOND3D_CASES["full"]
    bcfg, ncfg = synth.second3d_cfg(c["layer_nums"])
    b, n = registry.BACKBONES.build(bcfg), registry.NECKS.build(ncfg)
    sdb, sdn = synth.second3d_weights(b, n, c["seed"])
    b.load_state_dict(sdb), n.load_state_dict(sdn)
    b, n = b.to(dev).train(), n.to(dev).train()
    rb, rn = ref_second3d.build(bcfg, ncfg, sdb, sdn)
    rb, rn = rb.to(dev).train(), rn.to(dev).train()
    x = synth.second3d_input(c["grid_zyx"], seed=c["seed"]).to(dev)
    Z, Y, X = c["grid_zyx"]
    gout = torch.randn(1, 128, Z, Y, X, generator=torch.Generator().manual_seed(1)).to(dev)
    grows = gout.permute(0, 4, 3, 2, 1).reshape(-1, 128).contiguous()
    hip_params = list(b.parameters()) + list(n.parameters())
    ref_params = list(rb.parameters()) + list(rn.parameters())

    def hip():
        for p in hip_params:
            p.grad = None
        xd = x.detach().requires_grad_()
        out = lt.run_trunk_train(b, n, xd)
        out.t.backward(grows)
        return out.t, xd.grad

    def base():
        for p in ref_params:
            p.grad = None
        xd = x.detach().requires_grad_()
        y = rn(list(rb(xd)))
        y.backward(gout)
        return y, xd.grad

    def window(fn):
        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        s.record()
        for _ in range(a.steps):
            fn()
        e.record()
        torch.cuda.synchronize()
        return s.elapsed_time(e) / a.steps

    sides = [("hip", hip), ("torch", base)] if a.only is None else [(a.only, hip if a.only == "hip" else base)]
    ms = {k: [] for k, _ in sides}
    res = dict(workload="coocc_lidar trunk train step (fwd + bwd) [1,128,8,100,100] layer_nums [5,5,5]", engine=core.CONV_ENGINE,
               forms="direct split-f16 forward / stride-1 dgrad, fp32-MFMA strided dgrad by class and k_wgrad", steps=a.steps,
               warmup=a.warmup)
    torch_cannot = []
    if a.only is None:
        try:
            y, dx = base()
            o, dxh = hip()
            rel = lambda g, w: float((g - w).abs().max() / w.abs().max().clamp(min=1.0))
            res["max_rel_diff_vs_torch"] = dict(out=rel(o.view(X, Y, Z, 128).permute(3, 2, 1, 0), y[0]), dx=rel(dxh, dx),
                                                dw_first=rel(b.blocks[0][0].weight.grad, rb.blocks[0][0].weight.grad))
        except RuntimeError as e:
            torch_cannot.append(str(e).splitlines()[0][:200])
            sides = [("hip", hip)]
    res["torch_cannot_run"] = torch_cannot
    for _, fn in sides:
        for _ in range(a.warmup):
            fn()
    torch.cuda.synchronize()
    for _ in range(a.windows):
        for k, fn in sides:
            ms[k].append(window(fn))
    core.check_h2_overflow()
    med = lambda v: sorted(v)[len(v) // 2]
    res["ms_per_step"] = {k: [round(t, 4) for t in v] for k, v in ms.items() if v}
    res["median_ms"] = {k: round(med(v), 4) for k, v in ms.items() if v}
    res["min_max_ms"] = {k: [round(min(v), 4), round(max(v), 4)] for k, v in ms.items() if v}
    if ms.get("torch") and ms.get("hip"):
        res["ratio_per_window"] = [round(t / h, 3) for h, t in zip(ms["hip"], ms["torch"])]
    if a.only in (None, "hip"):
        # the parts: every C-ABI call between event pairs (level 2), a pass of its own
        core.TIMER.enabled, core.TIMER.only = 2, None
        core.TIMER.reset()
        nparts = 5
        for _ in range(nparts):
            hip()
        torch.cuda.synchronize()
        table = core.TIMER.summary()
        core.TIMER.enabled = False
        core.TIMER.reset()
        per = lambda k: dict(launches_per_step=table[k]["launches"] / nparts, ms_per_step=round(table[k]["ms"] / nparts, 4),
                             work_per_step=table[k]["work"] / nparts) if k in table else None
        parts = {k: per(k) for k in ("conv_dgrad", "k_gemm_h2 conv_dgrad", "k_gemm_h2 conv_fwd", "k_wgrad", "k_fpn_sum", "k_fpn_sum_bwd")}
        fb = parts["k_fpn_sum_bwd"]
        if fb:      # work = bytes: dout read once + every written level
            fb["bytes"] = fb.pop("work_per_step")
            fb["us_per_launch"] = round(1e3 * fb["ms_per_step"] / fb["launches_per_step"], 2)
            fb["share_of_hbm_peak"] = round(fb["bytes"] / HBM_PEAK / (fb["ms_per_step"] * 1e-3), 4)
        for k in ("conv_dgrad", "k_gemm_h2 conv_dgrad", "k_gemm_h2 conv_fwd", "k_wgrad"):
            if parts[k]:
                parts[k]["tflops"] = round(parts[k].pop("work_per_step") / (parts[k]["ms_per_step"] * 1e-3) / 1e12, 2)
        res["parts"] = parts
        if a.kernels:
            with open(a.kernels, "w") as f:
                f.write("# %s\n# per-launch event timer, level 2 (every C-ABI call), %d steps; ms and launches per step\n" % (res["workload"], nparts))
                f.write("# a named region (k_*, conv_*) CONTAINS the coocc_* call it wraps: both lines show that launch; no total\n")
                f.write("%-34s %9s %10s\n" % ("region", "launches", "ms/step"))
                for k, v in sorted(table.items(), key=lambda kv: -kv[1]["ms"]):
                    f.write("%-34s %9.1f %10.4f\n" % (k, v["launches"] / nparts, v["ms"] / nparts))
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
