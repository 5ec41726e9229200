"""The LiDAR depth map kernel (co_occ_amd/depth_maps.py, csrc/depth_maps.hip): 34 720 points (one nuScenes key frame) x 6 cameras of
the synthetic rig into 6 x 256 x 704 (r50) and 6 x 896 x 1600 (r101) maps, against
  (a) the zero fill alone (the same entry point with no points): what is left is the kernel;
  (b) the same computation as eager torch ops on the same GPU: the projection's broadcast matmuls, the valid test, rounding and
      ``scatter_reduce_(amin)``, with its launch count.  It is NOT bit-equal (the GPU matmul contracts and reorders): the number of
      differing pixels is recorded;
  (c) what it replaces: the reference's torch CPU code (broadcast matmuls, sort per camera, indexed assignment) on one host core, and
      the pinned-host upload of the N x H x W fp32 maps compared with the upload of the [P,5] cloud.
Writes profiles/depth_maps_bench.json (or --out).

Timing: every shape and path is warmed up, the device paths alternate inside one process; a timed window is --reps back-to-back calls
bracketed by device events on the stream (a single call of tens of microseconds is below what an event pair resolves), reported per
call as the median of --iters windows with the min / max spread.  The host path is timed with the host clock.  Bytes are computed
from the shapes.  Launch counts come from a separate profiled round, never from a timed one; where the profiler gives nothing the
count is null.

    python tools/bench_depth_maps.py [--iters 30] [--reps 20] [--warmup 5] [--host-iters 3] [--out profiles/depth_maps_bench.json]
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import numpy as np
import torch

import depth_map_refs as D
import image_input_refs as R
from co_occ_amd import depth_maps as DM

P, N = 34720, 6
SHAPES = {"r50_6x256x704": R.R50, "r101_6x896x1600": R.R101}
HBM_MEASURED = 6.29e12


def torch_eager(points, inv_rots, trans, intrins, post_rots2, post_trans2, H, W):
    """The projection and the minimum per pixel as plain torch ops on the device; no host read (invalid pairs go to a spare slot)."""
    n = trans.shape[0]
    q = points[:, None, :3] - trans[None]
    cam = torch.matmul(inv_rots[None], q[..., None])
    img = torch.matmul(intrins[None], cam)[..., 0]
    d = img[..., 2]
    uv = img[..., :2] / d[..., None]
    uv = torch.matmul(post_rots2[None], uv[..., None])[..., 0] + post_trans2[None]
    u, v = uv[..., 0], uv[..., 1]
    ok = (u >= 0) & (v >= 0) & (u <= W - 1) & (v <= H - 1) & (d > 0)
    cell = (torch.arange(n, device=points.device)[None] * H + v.round().long()) * W + u.round().long()
    cell = torch.where(ok, cell, torch.full_like(cell, n * H * W))
    maps = torch.full((n * H * W + 1,), float("inf"), device=points.device)
    maps.scatter_reduce_(0, cell.reshape(-1), torch.where(ok, d, torch.full_like(d, float("inf"))).reshape(-1), "amin")
    maps = maps[:-1]
    return torch.where(torch.isinf(maps), torch.zeros_like(maps), maps).view(n, H, W)


def host_path(points, mats, H, W):
    u, v, d = D.torch_projection(points, *mats)
    return D.torch_maps(u, v, d, H, W)[0]


def device_window(fn, reps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps


def launches(fn, marker):
    try:
        from torch.profiler import ProfilerActivity, profile
        with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
            fn()
            torch.cuda.synchronize()
        dev_ev = [e for e in prof.events() if str(getattr(e, "device_type", "")).endswith("CUDA")]
        kern = [e.name for e in dev_ev if not e.name.lower().startswith(("memcpy", "memset"))]
        fills = [e.name for e in dev_ev if e.name.lower().startswith("memset")]
        if not dev_ev:
            return dict(kernels=None, note="the profiler recorded no device activity")
        return dict(kernels=len(kern), memsets=len(fills), package_kernels=sorted(set(k for k in kern if marker in k)))
    except Exception as exc:                      # not measured
        return dict(kernels=None, note="profiler unavailable: %s" % type(exc).__name__)


def spread(v):
    return dict(median=round(statistics.median(v), 5), min=round(min(v), 5), max=round(max(v), 5))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=30)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--host-iters", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "depth_maps_bench.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_depth_maps: needs the GPU (a CPU timing says nothing about it)")
    dev = torch.device("cuda:0")
    torch.set_num_threads(1)
    cloud = D.cloud(P, seed=1, C=5)
    cloud_pinned = torch.from_numpy(cloud).pin_memory()
    points = cloud_pinned.to(dev)
    none = torch.empty((0, 5), device=dev)
    result = dict(device=torch.cuda.get_device_name(0), iters=a.iters, reps=a.reps, warmup=a.warmup, host_iters=a.host_iters, cameras=N,
                  points=P, point_floats=5, host_threads=torch.get_num_threads(), host_cpus_usable=len(os.sched_getaffinity(0)),
                  timing="device events around reps back-to-back calls, per call, median of iters windows, the device paths alternating; "
                         "host path: host clock, one thread", shapes={})
    for name, cfg in SHAPES.items():
        H, W = cfg['input_size']
        mats = D.rig(cfg)
        table = DM.camera_table(*mats).to(dev)
        out = torch.empty((N, H, W), device=dev)
        inv, trans, intrins = mats[0].inverse().to(dev), mats[1].to(dev), mats[2].to(dev)
        pr2, pt2 = mats[3][:, :2, :2].contiguous().to(dev), mats[4][:, :2].contiguous().to(dev)
        paths = {"fill_and_kernel": lambda: DM.points_to_depth_maps(points, table, (H, W), out=out),
                 "fill_alone": lambda: DM.points_to_depth_maps(none, table, (H, W), out=out),
                 "torch_eager": lambda: torch_eager(points, inv, trans, intrins, pr2, pt2, H, W)}
        for _ in range(a.warmup):
            for fn in paths.values():
                device_window(fn, a.reps)
        rounds = {k: [] for k in paths}
        for _ in range(a.iters):
            for k, fn in paths.items():
                rounds[k].append(device_window(fn, a.reps))
        entry = dict(map_bytes=N * H * W * 4, point_bytes=int(cloud.nbytes), table_bytes=N * DM.CAM_FLOATS * 4)
        for k, fn in paths.items():
            entry[k] = dict(call_ms=spread(rounds[k]), launches=launches(fn, "k_points_to_depth_maps"))
        fk, fa, te = (entry[k]["call_ms"]["median"] for k in ("fill_and_kernel", "fill_alone", "torch_eager"))
        entry["kernel_ms_by_difference"] = round(fk - fa, 5)
        entry["fill_alone"]["hbm_fraction_of_measured_copy"] = round(entry["map_bytes"] / (fa * 1e-3) / HBM_MEASURED, 4)
        entry["torch_eager_over_fill_and_kernel"] = round(te / fk, 3)
        got = paths["fill_and_kernel"]().clone()
        eager = paths["torch_eager"]()
        entry["written_pixels"] = int((got != 0).sum())
        entry["torch_eager"]["bit_equal_to_kernel"] = bool(torch.equal(eager, got))
        entry["torch_eager"]["differing_pixels"] = int((eager != got).sum())
        want = D.restatement(cloud, *[m.numpy() for m in mats], (H, W))
        entry["fill_and_kernel"]["bit_equal_to_restatement"] = bool(np.array_equal(got.cpu().numpy().view(np.uint32), want.view(np.uint32)))
        # (c) the host path and the two uploads
        host = []
        for _ in range(a.host_iters):
            t0 = time.perf_counter()
            ref = host_path(cloud, mats, H, W)
            host.append((time.perf_counter() - t0) * 1e3)
        entry["host_torch_reference"] = dict(call_ms=spread(host), threads=1,
                                             pixels_differing_from_kernel=int((ref != got.cpu()).sum()))
        maps_pinned = ref.pin_memory()
        ups = {"maps_upload": lambda: maps_pinned.to(dev, non_blocking=True), "points_upload": lambda: cloud_pinned.to(dev, non_blocking=True)}
        for _ in range(2):
            for fn in ups.values():
                device_window(fn, 1)
        ur = {k: [] for k in ups}
        for _ in range(10):
            for k, fn in ups.items():
                ur[k].append(device_window(fn, 1))
        entry["maps_upload"] = dict(call_ms=spread(ur["maps_upload"]), bytes=entry["map_bytes"])
        entry["points_upload"] = dict(call_ms=spread(ur["points_upload"]), bytes=entry["point_bytes"])
        del maps_pinned
        result["shapes"][name] = entry
        print(name, json.dumps(entry))
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(result, fh, indent=1, sort_keys=True)
        fh.write("\n")
    print("wrote", a.out)


if __name__ == "__main__":
    main()
