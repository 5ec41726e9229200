"""The occupancy ground-truth loaders (co_occ_amd/occ_gt.py, csrc/occ_gt.hip) from host arrays to device tensors:
  a_200x200x16      LoadOccupancy, 60 000 rows (no masks exist in this form)
  b_200x200x16      LoadOccupancy2, 60 000 rows, six cameras at 256 x 704, without and with cal_visible
  b_512x512x40      LoadOccupancy2, 300 000 rows, six cameras at 896 x 1600, without and with cal_visible
  c_512x512x40      LoadNuscOccupancyAnnotations, 34 720 labelled points (no masks exist in this form)
every one with the 34 720-point cloud (aabb, points_occ).  Per case: the call from host arrays (row packing and checks on the host, one
staged upload, the kernels) as device time between two events and as host wall time, the launches, the bytes uploaded; against what
it replaces: the vectorised numpy restatement (tests/occ_gt_refs.py) on one host core, and the pinned upload of the dense volume in
the reference's dtype.  Writes profiles/occ_gt_bench.json (or --out).

Timing: every case is warmed up; a timed window is one call bracketed by device events on the stream after a synchronise, reported as
the median of --iters windows with the min / max spread.  The host path is timed with the host clock on one thread.  Launch counts
come from a separate profiled call, never from a timed one; where the profiler gives nothing the count is null.

    python tools/bench_occ_gt.py [--iters 20] [--warmup 3] [--host-iters 3] [--out profiles/occ_gt_bench.json]
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
import occ_gt_refs as G
from co_occ_amd import occ_gt as OG

P = 34720
SMALL_GRID, SMALL_RANGE = (200, 200, 16), [-50.0, -50.0, -5.0, 50.0, 50.0, 3.0]
BIG_GRID, BIG_RANGE = (512, 512, 40), [-51.2, -51.2, -5.0, 51.2, 51.2, 3.0]


def spread(v):
    return dict(median=round(statistics.median(v), 4), min=round(min(v), 4), max=round(max(v), 4))


def window(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    e0.record()
    fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1), (time.perf_counter() - t0) * 1e3


def launches(fn):
    try:
        from torch.profiler import ProfilerActivity, profile
        with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
            fn()
            torch.cuda.synchronize()
        dev_ev = [e for e in prof.events() if str(getattr(e, "device_type", "")).endswith("CUDA")]
        if not dev_ev:
            return dict(kernels=None, note="the profiler recorded no device activity")
        low = [e.name.lower() for e in dev_ev]
        return dict(kernels=sum(not n.startswith(("memcpy", "memset")) for n in low), memsets=sum(n.startswith("memset") for n in low),
                    copies=sum(n.startswith("memcpy") for n in low))
    except Exception as exc:                      # not measured
        return dict(kernels=None, note="profiler unavailable: %s" % type(exc).__name__)


def twelve(cfg, dev):
    H, W = cfg['input_size']
    mats = D.rig(cfg)
    imgs = torch.zeros(6, 3, H, W, device=dev)
    return (imgs,) + tuple(m.to(dev) for m in mats) + (None, None, None, None, None, imgs.shape[-2:]), [m.numpy() for m in mats], (H, W)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--host-iters", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "occ_gt_bench.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_occ_gt: needs the GPU (a CPU timing says nothing about it)")
    dev = torch.device("cuda:0")
    torch.set_num_threads(1)
    cloud, pose = D.cloud(P, seed=1, C=5), G.pose_fields(1)
    seg = G.seg_bytes(P, G.LEARNING_MAP, seed=2)
    bda = np.eye(3, dtype=np.float32)
    occ_small = G.rows(60000, 4, SMALL_GRID, seed=3, label_col=3)
    occ_small_b = G.rows(60000, 4, (SMALL_GRID[2], SMALL_GRID[1], SMALL_GRID[0]), seed=4)
    occ_big = np.concatenate([G.distinct_rows(240000, BIG_GRID, seed=5), G.rows(60000, 4, (40, 512, 512), seed=6)])
    t50, m50, s50 = twelve(R.R50, dev)
    t101, m101, s101 = twelve(R.R101, dev)
    lm = G.LEARNING_MAP
    cases = {}

    def add(name, loader, call, host, dense):
        cases[name] = (loader, call, host, dense)

    la = OG.LoadOccupancy(grid_size=list(SMALL_GRID), pc_range=SMALL_RANGE, device=dev)
    add("a_200x200x16", la, lambda: la(occ_small, cloud, pose), lambda: G.load_occupancy(occ_small, SMALL_GRID),
        np.zeros(SMALL_GRID, np.float64))
    for tag, grid, rng, occ, tw, mats, size in (("b_200x200x16", SMALL_GRID, SMALL_RANGE, occ_small_b, t50, m50, s50),
                                                ("b_512x512x40", BIG_GRID, BIG_RANGE, occ_big, t101, m101, s101)):
        for masks in (False, True):
            lb = OG.LoadOccupancy2(grid_size=list(grid), pc_range=rng, cal_visible=masks, learning_map=lm, device=dev)

            def host(grid=grid, rng=rng, occ=occ, mats=mats, size=size, masks=masks):
                out = [G.load_occupancy2(occ, grid, rng, bda, 0, G.vote_sorted)]
                if masks:
                    out.append(G.img_visible_mask(occ, grid, rng, bda, mats, size[0], size[1], G.vote_sorted, G.zbuffer_sorted))
                    out.append(G.lidar_visible_mask(cloud, grid, rng, G.vote_sorted))
                return out
            add(tag + ("_masks" if masks else ""), lb, lambda lb=lb, occ=occ, tw=tw: lb(occ, cloud, seg, pose, img_inputs=tw, lidar_points=cloud),
                host, np.zeros((4 if masks else 1,) + tuple(grid), np.uint8))
    lc = OG.LoadNuscOccupancyAnnotations(grid_size=list(BIG_GRID), point_cloud_range=BIG_RANGE, learning_map=lm, device=dev)
    add("c_512x512x40", lc, lambda: lc(cloud, seg, pose), lambda: G.nusc_annotations(cloud, seg, lm, bda, BIG_GRID, BIG_RANGE, 17, G.vote_sorted),
        np.zeros(BIG_GRID, np.int64))

    result = dict(device=torch.cuda.get_device_name(0), iters=a.iters, warmup=a.warmup, host_iters=a.host_iters, points=P,
                  host_threads=torch.get_num_threads(), host_cpus_usable=len(os.sched_getaffinity(0)),
                  timing="one call from host arrays per window: device events and the host clock around it, median of iters windows; "
                         "host restatement: host clock, one thread", cases={})
    for name, (loader, call, host, dense) in cases.items():
        for _ in range(a.warmup):
            window(call)
        dev_ms, wall_ms = zip(*[window(call) for _ in range(a.iters)])
        entry = dict(device_ms=spread(dev_ms), host_wall_ms=spread(wall_ms), launches=launches(call), uploaded_bytes=int(loader._stage.last_bytes),
                     dense_bytes=int(dense.nbytes), dense_dtype=str(dense.dtype))
        ht = []
        for _ in range(a.host_iters):
            t0 = time.perf_counter()
            host()
            ht.append((time.perf_counter() - t0) * 1e3)
        entry["host_numpy_restatement_ms"] = dict(spread(ht), threads=1)
        pinned = torch.from_numpy(dense).pin_memory()
        up = lambda: pinned.to(dev, non_blocking=True)
        for _ in range(2):
            window(up)
        entry["dense_upload_ms"] = spread([window(up)[0] for _ in range(10)])
        del pinned
        result["cases"][name] = entry
        print(name, json.dumps(entry))
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(result, fh, indent=1, sort_keys=True)
        fh.write("\n")
    print("wrote", a.out)


if __name__ == "__main__":
    main()
