"""Forward + backward of the eight OccHead loss terms: eager co_occ_amd/losses.py against the device path (csrc/occ_loss.hip) on the
same GPU, per stage, with launch counts.  Writes profiles/occ_losses_bench.json (or --out).

Timing: every shape is warmed up, the two paths alternate inside one process, every stage is bracketed by device events on the
stream (the eager path's own host reads sit inside its brackets -- they are part of what it costs), the median of --iters rounds is
reported with the min / max spread.  Launch counts come from a separate profiled round (torch.profiler device activities), never
from a timed one; where the profiler gives nothing the count is reported as null (not measured).

    python tools/bench_occ_losses.py [--iters 30] [--warmup 5] [--out profiles/occ_losses_bench.json]
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np
import torch

import co_occ_amd as pkg
from co_occ_amd import losses as L

NCLS = 17
FINE_TOPK, CASCADE = 15000, 2                  # the r50 config: 8 fine points per selected coarse voxel
SIZES = {"r50_100x100x8": (100, 100, 8), "openocc_128x128x10": (128, 128, 10)}
STAGES = ("pool_labels", "coarse_fwd", "coarse_bwd", "fine_fwd", "fine_bwd")


def inputs(grid, dev, seed=0):
    g = np.random.default_rng(seed)
    h, w, d = grid
    r = CASCADE
    rows = torch.from_numpy(g.standard_normal((h * w * d, NCLS), dtype=np.float32) * 2).to(dev)
    gt = g.integers(1, NCLS, (1, h * r, w * r, d * r)).astype(np.uint8)
    gt[g.random(gt.shape) < 0.8] = 0
    gt[g.random(gt.shape) < 0.02] = 255
    n = FINE_TOPK * r ** 3
    coord = np.stack([g.integers(0, h * r, n), g.integers(0, w * r, n), g.integers(0, d * r, n)])
    fine = torch.from_numpy(g.standard_normal((n, NCLS), dtype=np.float32) * 2).to(dev)
    return dict(rows=rows, grid=grid, gt=torch.from_numpy(gt).to(dev), fine=fine, coord=torch.from_numpy(coord).to(dev))


def head_for(grid, dev, device_losses):
    head = pkg.build_head(dict(type='OccHead', in_channels=[32] * 2, out_channel=NCLS, num_level=2, soft_weights=True,
                               norm_cfg=dict(type='BN3d', requires_grad=True), cascade_ratio=CASCADE, sample_from_voxel=True,
                               sample_from_img=True, final_occ_size=[v * CASCADE for v in grid], empty_idx=0))
    head.device_losses = device_losses
    return head


def step(head, s, mark):
    """One forward + backward of the eight terms, ``mark(stage)`` called at every stage boundary."""
    h, w, d = s["grid"]
    rows = s["rows"].clone().requires_grad_(True)
    fine = s["fine"].clone().requires_grad_(True)
    logits = rows.view(1, h, w, d, NCLS).permute(0, 4, 1, 2, 3)          # what forward_train hands over
    mark(None)
    if head.device_losses:
        target = L.pool_labels_device(s["gt"], h, w, d, 0, num_cls=NCLS, dtype=torch.uint8)
    else:
        target = L.pool_labels(s["gt"], h, w, d, 0, num_cls=NCLS)
    mark("pool_labels")
    if head.device_losses:
        lc = head._loss_terms_device(L.occ_loss_terms_device(logits, target, head._class_weights_on(rows.device), 0), "c_0")
    else:
        lc = head._loss_terms(logits, target, "c_0", head.class_weights.to(logits))
    tc = sum(lc.values())
    mark("coarse_fwd")
    tc.backward()
    mark("coarse_bwd")
    lf = head.loss_point(s["coord"], fine, s["gt"], "fine")
    tf = sum(lf.values())
    mark("fine_fwd")
    tf.backward()
    mark("fine_bwd")
    return dict(lc, **lf), rows.grad, fine.grad


def timed(head, s):
    ev = []

    def mark(stage):
        e = torch.cuda.Event(enable_timing=True)
        e.record()
        ev.append((stage, e))
    step(head, s, mark)
    torch.cuda.synchronize()
    return {stage: ev[i - 1][1].elapsed_time(e) for i, (stage, e) in enumerate(ev) if stage is not None}


def launches(head, s):
    try:
        from torch.profiler import ProfilerActivity, profile
        with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
            step(head, s, lambda stage: None)
            torch.cuda.synchronize()
        n = sum(1 for e in prof.events() if str(getattr(e, "device_type", "")).endswith("CUDA") and not e.name.lower().startswith("memcpy")
                and not e.name.lower().startswith("memset"))
        c = sum(1 for e in prof.events() if str(getattr(e, "device_type", "")).endswith("CUDA") and e.name.lower().startswith("memcpy dtoh"))
        return dict(kernels=n or None, dtoh_copies=c if n else None)
    except Exception as exc:                      # not measured
        return dict(kernels=None, dtoh_copies=None, note="profiler unavailable: %s" % type(exc).__name__)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "occ_losses_bench.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_occ_losses: needs the GPU (a CPU timing says nothing about it)")
    dev = torch.device("cuda:0")
    result = dict(device=torch.cuda.get_device_name(0), iters=a.iters, warmup=a.warmup, classes=NCLS,
                  fine_points=FINE_TOPK * CASCADE ** 3, timing="device events per stage, median of iters, paths alternating", sizes={})
    for name, grid in SIZES.items():
        s = inputs(grid, dev)
        heads = {"eager": head_for(grid, dev, False), "device": head_for(grid, dev, True)}
        for _ in range(a.warmup):
            for h in heads.values():
                timed(h, s)
        rounds = {k: [] for k in heads}
        for _ in range(a.iters):
            for k, h in heads.items():
                rounds[k].append(timed(h, s))
        # the two paths on the same inputs: values and gradients side by side
        (le, ge, fe), (ld, gd, fd) = step(heads["eager"], s, lambda st: None), step(heads["device"], s, lambda st: None)
        entry = dict(grid=list(grid), rows=int(s["rows"].shape[0]))
        for k in heads:
            per = {st: [r[st] for r in rounds[k]] for st in STAGES}
            tot = [sum(r.values()) for r in rounds[k]]
            entry[k] = dict(stages_ms={st: round(statistics.median(v), 4) for st, v in per.items()},
                            total_ms=dict(median=round(statistics.median(tot), 4), min=round(min(tot), 4), max=round(max(tot), 4)),
                            launches=launches(heads[k], s))
        entry["eager_over_device"] = round(entry["eager"]["total_ms"]["median"] / entry["device"]["total_ms"]["median"], 3)
        entry["max_rel_value_diff"] = max(abs(float(ld[k].detach()) - float(le[k].detach())) / max(1.0, abs(float(le[k].detach()))) for k in le)
        entry["coarse_grad_max_diff_over_max"] = float((gd - ge).abs().max() / ge.abs().max())
        entry["fine_grad_max_diff_over_max"] = float((fd - fe).abs().max() / fe.abs().max())
        result["sizes"][name] = entry
        print(name, json.dumps(entry))
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(result, fh, indent=1, sort_keys=True)
        fh.write("\n")
    print("wrote", a.out)


if __name__ == "__main__":
    main()
