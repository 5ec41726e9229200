"""The multi-sweep cloud (co_occ_amd/sweeps.py, csrc/sweeps.hip) at the workload's size: a key frame and ten sweeps of 34 720 rows
(load_dim 5), use_dim [0,1,2,4], remove_close off and on.  Per mode:
  (a) loader_call     LoadPointsFromMultiSweeps from host arrays to a synchronised cloud on the device, host clock: the raw clouds laid
                      into the pinned buffer, one copy, the launches (with remove_close: the read of the count);
  (b) upload_to_cloud the same call between two device events (what the stream sees from the upload to the cloud), and
      kernels         merge_sweeps alone on a raw buffer and a table that are on the device already;
  (c) numpy_then_upload  what it replaces: the literal numpy step (tests/sweep_refs.literal: float64 matmul, +=, concatenate, the column
                      pick) on ONE host core, then the pinned upload of the merged [P,4] cloud, host clock to a synchronise; the two parts
                      are also given apart;
  (d) torch_eager     the same computation as eager torch ops on the same GPU from the raw buffer on the device (float64 matmul per
                      sweep, boolean indexing for remove_close, cat), with its launch count.  It is NOT the restatement's order of
                      operations: the number of differing values is recorded.
Writes profiles/sweeps_bench.json (or --out).

Timing: every path is warmed up and the paths alternate inside one process.  Device windows are --reps back-to-back calls between two
events (a single call of tens of microseconds is below what an event pair resolves), reported per call as the median of --iters
windows with the min / max spread; host-clock paths end in a synchronise and are reported per call the same way.  Bytes are computed
from the shapes.  Launch counts come from a separate profiled call, never from a timed one; where the profiler gives nothing the
count is null.

    python tools/bench_sweeps.py [--iters 30] [--reps 20] [--warmup 5] [--host-iters 10] [--out profiles/sweeps_bench.json]
"""
import os

os.environ["OPENBLAS_NUM_THREADS"] = "1"          # (c) is one host core; set before numpy loads its BLAS
os.environ["MKL_NUM_THREADS"] = "1"
os.environ["OMP_NUM_THREADS"] = "1"

import argparse
import json
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import numpy as np
import torch

import sweep_refs as S
from co_occ_amd import sweeps as SW

USE_DIM = [0, 1, 2, 4]


def torch_eager(raw, bounds, Rs, ts_, dts, remove_close):
    segs = []
    for k, (a, b) in enumerate(bounds):
        s = raw[a:b].clone()
        if k == 0:
            s[:, 4] = 0
        else:
            if remove_close:
                s = s[~((s[:, 0].abs() < 1.0) & (s[:, 1].abs() < 1.0))]
            s[:, :3] = (s[:, :3].double() @ Rs[k - 1].T).float()
            s[:, :3] = (s[:, :3].double() + ts_[k - 1]).float()
            s[:, 4] = dts[k - 1]
        segs.append(s)
    return torch.cat(segs)[:, USE_DIM].contiguous()


def device_window(fn, reps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps


def host_window(fn, reps):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(reps):
        fn()
        torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3 / reps


def launches(fn, marker):
    try:
        from torch.profiler import ProfilerActivity, profile
        with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
            fn()
            torch.cuda.synchronize()
        dev_ev = [e for e in prof.events() if str(getattr(e, "device_type", "")).endswith("CUDA")]
        kern = [e.name for e in dev_ev if not e.name.lower().startswith(("memcpy", "memset"))]
        copies = [e.name for e in dev_ev if e.name.lower().startswith("memcpy")]
        if not dev_ev:
            return dict(kernels=None, note="the profiler recorded no device activity")
        return dict(kernels=len(kern), copies=len(copies), package_kernels=sorted(set(k for k in kern if marker in k)))
    except Exception as exc:                      # not measured
        return dict(kernels=None, note="profiler unavailable: %s" % type(exc).__name__)


def spread(v):
    return dict(median=round(statistics.median(v), 5), min=round(min(v), 5), max=round(max(v), 5))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=30)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--host-iters", type=int, default=10)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "sweeps_bench.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_sweeps: needs the GPU (a CPU timing says nothing about it)")
    dev = torch.device("cuda:0")
    torch.set_num_threads(1)
    points, sweeps, ts = S.make("workload")
    choices = np.arange(10)
    clouds = [points] + [s['points'] for s in sweeps]
    bounds = list(zip(np.cumsum([0] + [len(c) for c in clouds[:-1]]).tolist(), np.cumsum([len(c) for c in clouds]).tolist()))
    raw_host = np.concatenate(clouds)
    raw = torch.from_numpy(raw_host).to(dev)
    Rs = [torch.from_numpy(s['sensor2lidar_rotation']).to(dev) for s in sweeps]
    ts_ = [torch.from_numpy(s['sensor2lidar_translation']).to(dev) for s in sweeps]
    dts = [float(np.float32(ts - s['timestamp'] / 1e6)) for s in sweeps]
    result = dict(device=torch.cuda.get_device_name(0), iters=a.iters, reps=a.reps, warmup=a.warmup, host_iters=a.host_iters,
                  segments=len(clouds), rows_per_segment=len(points), load_dim=5, use_dim=USE_DIM, host_threads=torch.get_num_threads(),
                  host_cpus_usable=len(os.sched_getaffinity(0)),
                  timing="device events around reps back-to-back calls, or the host clock around calls that each end in a synchronise; per "
                         "call, median of the windows, the paths alternating; numpy on one thread", modes={})
    for rc in (False, True):
        load = SW.LoadPointsFromMultiSweeps(remove_close=rc, device=dev)
        table = SW.sweep_table(len(points), sweeps, ts, choices, remove_close=rc).to(dev)
        out = torch.empty((table.total, 4), device=dev)
        count = torch.empty(1, dtype=torch.int32, device=dev)
        merged = S.literal(points, sweeps, ts, choices, remove_close=rc)
        merged_pinned = torch.from_numpy(merged).pin_memory()

        def numpy_then_upload():
            m = S.literal(points, sweeps, ts, choices, remove_close=rc)
            merged_pinned[:len(m)].copy_(torch.from_numpy(m))
            return merged_pinned[:len(m)].to(dev, non_blocking=True)
        dev_paths = {"upload_to_cloud": lambda: load(points, sweeps, ts),
                     "kernels": lambda: SW.merge_sweeps(raw, table, USE_DIM, out=out, count=count),
                     "torch_eager": lambda: torch_eager(raw, bounds, Rs, ts_, dts, rc),
                     "merged_upload": lambda: merged_pinned.to(dev, non_blocking=True)}
        host_paths = {"loader_call": lambda: load(points, sweeps, ts), "numpy_then_upload": numpy_then_upload,
                      "numpy_alone": lambda: S.literal(points, sweeps, ts, choices, remove_close=rc)}
        for _ in range(a.warmup):
            for fn in dev_paths.values():
                device_window(fn, a.reps)
        for fn in host_paths.values():
            host_window(fn, 2)
        rounds = {k: [] for k in list(dev_paths) + list(host_paths)}
        for _ in range(a.iters):
            for k, fn in dev_paths.items():
                rounds[k].append(device_window(fn, a.reps))
        for _ in range(a.host_iters):
            for k, fn in host_paths.items():
                rounds[k].append(host_window(fn, 3))
        cloud, extras = load(points, sweeps, ts)
        entry = dict(rows_in=int(table.in_rows), rows_out=int(cloud.shape[0]), upload_bytes=int(extras["upload_bytes"]),
                     merged_bytes=int(merged.nbytes), kernel_bytes_moved=int(table.in_rows * 20 + cloud.shape[0] * 16))
        for k in rounds:
            entry[k] = dict(call_ms=spread(rounds[k]), clock="device events" if k in dev_paths else "host clock to a synchronise")
        entry["kernels"]["launches"] = launches(dev_paths["kernels"], "k_sweeps")
        entry["upload_to_cloud"]["launches"] = launches(dev_paths["upload_to_cloud"], "k_sweeps")
        entry["torch_eager"]["launches"] = launches(dev_paths["torch_eager"], "k_sweeps")
        eager = dev_paths["torch_eager"]()
        entry["torch_eager"]["values_differing_from_kernel"] = (int((eager != cloud).sum()) if eager.shape == cloud.shape
                                                                 else "shape %s" % (tuple(eager.shape),))
        want = S.restatement(points, sweeps, ts, choices, remove_close=rc)[0]
        entry["bit_equal_to_restatement"] = bool(S.same(cloud.cpu().numpy(), want))
        entry["literal_numpy_bit_equal_to_restatement"] = bool(S.same(merged, want))
        lc, nu = entry["loader_call"]["call_ms"]["median"], entry["numpy_then_upload"]["call_ms"]["median"]
        entry["numpy_then_upload_over_loader_call"] = round(nu / lc, 3)
        entry["torch_eager_over_kernels"] = round(entry["torch_eager"]["call_ms"]["median"] / entry["kernels"]["call_ms"]["median"], 3)
        result["modes"]["remove_close" if rc else "plain"] = entry
        print("remove_close" if rc else "plain", json.dumps(entry))
        del merged_pinned
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(result, fh, indent=1, sort_keys=True)
        fh.write("\n")
    print("wrote", a.out)


if __name__ == "__main__":
    main()
