"""The parameter update of the full r50 multi-modal detector: torch's ``clip_grad_norm_`` + ``torch.optim.AdamW`` (at its defaults,
and with ``fused=True``) against ``co_occ_amd.optim.AdamW(max_grad_norm=5)`` (csrc/optim.hip) on the same GPU, with launch counts.
Writes profiles/optim_bench.json (or --out).

The parameter set is every trainable tensor of the detector built from ``synth.model_cfg()`` with the LiDAR encoder, the HIP image
encoder (ResNet-50 + SECONDFPN, trained) and the HIP DepthNet (trained) on.  Groups are one per parameter, as mmcv's
``DefaultOptimizerConstructor`` makes them under a ``paramwise_cfg`` (``norm_decay_mult=0`` on the norm layers), lr 1e-4, weight decay
0.01, ``max_norm=5``.  Gradients are seeded and random, the same values for every path; every path owns its copy of the parameters.

Timing: every path is warmed up, the paths alternate inside one process, every call (clip + step) is bracketed by device events on
the stream, the median of --iters rounds is reported with the min / max spread.  ``host_ms`` is the host clock from the call to its
return WITHOUT a final synchronise: how long the host is held.  The torch paths do not include the ``float(grad_norm)`` host read of
mmcv's ``OptimizerHook``.  Launch counts come from a separate profiled round (torch.profiler device activities), never from a timed
one; where the profiler gives nothing the count is reported as null (not measured).

    python tools/bench_optim.py [--iters 20] [--warmup 3] [--out profiles/optim_bench.json]
"""
import argparse
import json
import os
import re
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch

import co_occ_amd as pkg
from co_occ_amd import optim, synth

LR, WD, MAX_NORM = 1e-4, 0.01, 5.0
HBM_PEAK_GBS = 8000.0          # HBM3E spec


def detector():
    cfg = synth.model_cfg()
    cfg["img_view_transformer"].update(depth_net='hip', train_depth_net=True)
    cfg.update(synth.lidar_cfg())
    bb = dict(type='ResNet', depth=50, num_stages=4, out_indices=(0, 1, 2, 3), frozen_stages=0, norm_cfg=dict(type='BN', requires_grad=True),
              norm_eval=False, style='pytorch')
    nk = dict(type='SECONDFPN', in_channels=[256, 512, 1024, 2048], upsample_strides=[0.25, 0.5, 1, 2], out_channels=[128, 128, 128, 128])
    return pkg.build_detector(cfg, img_backbone=bb, img_neck=nk, hip_image_encoder=True, train_image_encoder=True)


def shapes_and_decay(det):
    """[(shape, weight decay)] of the trainable tensors: one group per parameter, no decay on the norm layers."""
    out = []
    for m in det.modules():
        norm = isinstance(m, (torch.nn.modules.batchnorm._BatchNorm, torch.nn.GroupNorm, torch.nn.LayerNorm))
        for p in m.parameters(recurse=False):
            if p.requires_grad:
                out.append((tuple(p.shape), 0.0 if norm else WD))
    return out


def make_path(kind, spec, dev, seed=0):
    g = torch.Generator(device=dev).manual_seed(seed)
    params = [torch.nn.Parameter(torch.randn(s, generator=g, device=dev) * 0.05) for s, _ in spec]
    for p in params:
        p.grad = torch.randn(p.shape, generator=g, device=dev) * 1e-3
    groups = [dict(params=[p], lr=LR, weight_decay=wd) for p, (_, wd) in zip(params, spec)]
    if kind == "device":
        opt = optim.AdamW(groups, lr=LR, weight_decay=WD, max_grad_norm=MAX_NORM)
        return dict(params=params, opt=opt, step=opt.step)
    opt = torch.optim.AdamW(groups, lr=LR, weight_decay=WD, **(dict(fused=True) if kind == "torch_fused" else {}))

    def step():
        torch.nn.utils.clip_grad_norm_(params, MAX_NORM)
        opt.step()
    return dict(params=params, opt=opt, step=step)


def timed(path):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    e0.record()
    path["step"]()
    e1.record()
    host = (time.perf_counter() - t0) * 1e3
    torch.cuda.synchronize()
    return e0.elapsed_time(e1), host


def launches(path):
    try:
        from torch.profiler import ProfilerActivity, profile
        with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
            path["step"]()
            torch.cuda.synchronize()
        dev_ev = [e for e in prof.events() if str(getattr(e, "device_type", "")).endswith("CUDA")]
        # device-side records that are not kernels: copies, fills, and the span torch's step hook annotates ("Optimizer.step#...")
        kern = [e for e in dev_ev if not e.name.lower().startswith(("memcpy", "memset")) and "Optimizer.step#" not in e.name]
        copies = [e for e in dev_ev if e.name.lower().startswith("memcpy")]
        if not kern:
            return dict(kernels=None, note="the profiler recorded no device activity")
        ours = [e for e in kern if "k_optim" in e.name]
        out = dict(kernels=len(kern), copies=len(copies), package_kernels=sorted(set(re.search(r"k_optim_\w+", e.name).group(0) for e in ours)))
        if len(kern) <= 16:
            out["other_kernels"] = sorted(e.name[:80] for e in kern if "k_optim" not in e.name)
        if ours:
            out["package_kernel_ms"] = round(sum(getattr(e, "device_time", 0.0) or 0.0 for e in ours) / 1e3, 4)
        return out
    except Exception as exc:                      # not measured
        return dict(kernels=None, note="profiler unavailable: %s" % type(exc).__name__)


def spread(v):
    return dict(median=round(statistics.median(v), 4), min=round(min(v), 4), max=round(max(v), 4))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "optim_bench.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_optim: needs the GPU (a CPU timing says nothing about it)")
    dev = torch.device("cuda:0")
    spec = shapes_and_decay(detector())
    elements = sum(int(torch.Size(s).numel()) for s, _ in spec)
    paths = {k: make_path(k, spec, dev) for k in ("torch", "torch_fused", "device")}
    for _ in range(a.warmup):
        for p in paths.values():
            timed(p)
    rounds = {k: [] for k in paths}
    for _ in range(a.iters):
        for k, p in paths.items():
            rounds[k].append(timed(p))
    chunks = int(optim.chunk_table([int(torch.Size(s).numel()) for s, _ in spec]).shape[0])
    result = dict(device=torch.cuda.get_device_name(0), iters=a.iters, warmup=a.warmup, tensors=len(spec), groups=len(spec),
                  elements=elements, lr=LR, weight_decay=WD, max_norm=MAX_NORM, chunk=optim.chunk_size(), chunks=chunks,
                  timing="device events per call (clip + step), median of iters, paths alternating; host_ms = host clock until the "
                         "call returns, no final synchronise; the torch paths without the hook's float(grad_norm) host read",
                  paths={})
    for k, p in paths.items():
        result["paths"][k] = dict(call_ms=spread([r[0] for r in rounds[k]]), host_ms=spread([r[1] for r in rounds[k]]),
                                  launches=launches(p))
    d = result["paths"]["device"]
    table_bytes = len(spec) * optim.TENSOR_DTYPE.itemsize + chunks * 16
    moved = 32 * elements + 2 * table_bytes + 16 * chunks        # 4 (norm) + 16 read + 12 written per element; tables; partials
    d["bytes_moved"] = moved
    d["table_bytes"] = table_bytes
    ms = d["launches"].get("package_kernel_ms") or d["call_ms"]["median"]
    d["hbm_time_ms"] = ms
    d["hbm_time_from"] = "profiled kernel time" if d["launches"].get("package_kernel_ms") else "device events of the call"
    d["achieved_gbs"] = round(moved / ms / 1e6, 1)
    d["hbm_peak_gbs"] = HBM_PEAK_GBS
    d["share_of_hbm_peak"] = round(moved / ms / 1e6 / HBM_PEAK_GBS, 4)
    for k in ("torch", "torch_fused"):
        result[k + "_over_device"] = dict(call=round(result["paths"][k]["call_ms"]["median"] / d["call_ms"]["median"], 3),
                                          host=round(result["paths"][k]["host_ms"]["median"] / d["host_ms"]["median"], 3))
    # the three paths stepped the same number of times from the same start on the same gradients
    pd, pt = paths["device"]["params"], paths["torch"]["params"]
    result["max_rel_diff_to_torch"] = max(float((x.detach() - y.detach()).abs().max() / y.detach().abs().max()) for x, y in zip(pd, pt))
    print(json.dumps(result))
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(result, fh, indent=1, sort_keys=True)
        fh.write("\n")
    print("wrote", a.out)


if __name__ == "__main__":
    main()
