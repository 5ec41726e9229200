"""Forward + backward of the DepthNet depth loss (``ViewTransformerLiftSplatShootVoxel.get_depth_loss``): the eager torch path against
the device path (csrc/depth_loss.hip, ``device_depth_loss=True``) on the same GPU, with launch counts.  Writes
profiles/depth_loss_bench.json (or --out).

Timing: every shape is warmed up, the two paths alternate inside one process, every call (forward + backward) is bracketed by device
events on the stream (the eager path's own host reads sit inside its brackets -- they are part of what it costs), the median of
--iters rounds is reported with the min / max spread.  ``host_ms`` is the host clock from the call to its return WITHOUT a final
synchronise: how long the host is held (the eager path waits for its two device->host reads there; the device path only enqueues).
Launch counts come from a separate profiled round (torch.profiler device activities), never from a timed one; where the profiler
gives nothing the count is reported as null (not measured).

    python tools/bench_depth_loss.py [--iters 30] [--warmup 5] [--out profiles/depth_loss_bench.json]
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np
import torch

from co_occ_amd.view_transformer import ViewTransformerLiftSplatShootVoxel

CAMS, DS, DBOUND, D = 6, 16, [2.0, 58.0, 0.5], 112
SIZES = {"r50_6x256x704": (256, 704), "r101_6x896x1600": (896, 1600)}


def inputs(size, dev, seed=0):
    g = np.random.default_rng(seed)
    H, W = size
    depth = (g.uniform(0.5, 70.0, (1, CAMS, H, W)) * (g.random((1, CAMS, H, W)) < 0.05)).astype(np.float32)      # a sparse LiDAR sweep
    logits = g.standard_normal((CAMS, D, H // DS, W // DS), dtype=np.float32) * 2
    return dict(gt=torch.from_numpy(depth).to(dev), preds=torch.from_numpy(logits).to(dev).softmax(1))


def module_for(size, dev, device_depth_loss):
    vt = ViewTransformerLiftSplatShootVoxel(grid_config=dict(xbound=[-50, 50, 1.0], ybound=[-50, 50, 1.0], zbound=[-5, 3, 1.0], dbound=DBOUND),
                                            data_config=dict(input_size=size), downsample=DS, depth_net=torch.nn.Identity(),
                                            device_depth_loss=device_depth_loss)
    assert vt.D == D
    return vt.to(dev)


def step(vt, s):
    leaf = s["preds"].clone().requires_grad_(True)
    loss = vt.get_depth_loss(s["gt"], leaf)
    loss.backward()
    return loss.detach(), leaf.grad


def timed(vt, s):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    e0.record()
    step(vt, s)
    e1.record()
    host = (time.perf_counter() - t0) * 1e3
    torch.cuda.synchronize()
    return e0.elapsed_time(e1), host


def launches(vt, s):
    try:
        from torch.profiler import ProfilerActivity, profile
        with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
            step(vt, s)
            torch.cuda.synchronize()
        dev_ev = [e for e in prof.events() if str(getattr(e, "device_type", "")).endswith("CUDA")]
        kern = [e.name for e in dev_ev if not e.name.lower().startswith(("memcpy", "memset"))]
        # host-side runtime calls that block until the device has caught up: synchronous copies (the device->host reads) and stream
        # synchronisation; asynchronous copies (the clone of the probabilities) and the round's own final synchronise are not
        waits = [e.name for e in prof.events() if not str(getattr(e, "device_type", "")).endswith("CUDA") and "async" not in e.name.lower()
                 and e.name.lower().startswith(("hipmemcpy", "cudamemcpy", "hipstreamsynchronize", "cudastreamsynchronize"))]
        if not kern:
            return dict(kernels=None, host_waits=None, note="the profiler recorded no device activity")
        return dict(kernels=len(kern), host_waits=len(waits), host_wait_calls=sorted(set(waits)),
                    package_kernels=sorted(set(k for k in kern if "k_depth" in k)))
    except Exception as exc:                      # not measured
        return dict(kernels=None, host_waits=None, note="profiler unavailable: %s" % type(exc).__name__)


def spread(v):
    return dict(median=round(statistics.median(v), 4), min=round(min(v), 4), max=round(max(v), 4))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "depth_loss_bench.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_depth_loss: needs the GPU (a CPU timing says nothing about it)")
    dev = torch.device("cuda:0")
    result = dict(device=torch.cuda.get_device_name(0), iters=a.iters, warmup=a.warmup, cameras=CAMS, downsample=DS, bins=D,
                  timing="device events per call (forward + backward, clone of the probabilities included), median of iters, paths "
                         "alternating; host_ms = host clock until the call returns, no final synchronise", sizes={})
    for name, size in SIZES.items():
        s = inputs(size, dev)
        mods = {"eager": module_for(size, dev, False), "device": module_for(size, dev, True)}
        for _ in range(a.warmup):
            for vt in mods.values():
                timed(vt, s)
        rounds = {k: [] for k in mods}
        for _ in range(a.iters):
            for k, vt in mods.items():
                rounds[k].append(timed(vt, s))
        (le, ge), (ld, gd) = step(mods["eager"], s), step(mods["device"], s)
        entry = dict(input_size=list(size), pixels=CAMS * (size[0] // DS) * (size[1] // DS),
                     depth_map_bytes=4 * CAMS * size[0] * size[1])
        for k, vt in mods.items():
            entry[k] = dict(call_ms=spread([r[0] for r in rounds[k]]), host_ms=spread([r[1] for r in rounds[k]]), launches=launches(vt, s))
        entry["eager_over_device"] = round(entry["eager"]["call_ms"]["median"] / entry["device"]["call_ms"]["median"], 3)
        entry["rel_value_diff"] = abs(float(ld) - float(le)) / max(1.0, abs(float(le)))
        entry["grad_max_diff_over_max"] = float((gd - ge).abs().max() / ge.abs().max())
        result["sizes"][name] = entry
        print(name, json.dumps(entry))
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(result, fh, indent=1, sort_keys=True)
        fh.write("\n")
    print("wrote", a.out)


if __name__ == "__main__":
    main()
