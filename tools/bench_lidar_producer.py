"""What the LiDAR producer (co_occ_amd/lidar.py: Voxelization -> HardSimpleVFE -> SparseLiDAREnc8x) costs the HOST per sample, at the size
of coocc_multi_r50_256x704.py:121-134: sparse shape 800 x 800 x 64, max_voxels 120 000, a synthetic 11 x 34 720-point cloud.

The producer stops for the host four times per sample (the voxel count, and one output count per down-convolution) and is issued launch
by launch, so the serving loop cannot capture it.  Nobody had measured what that costs; this tool does, per sample:
  host_ms        host wall time from the call to its return: how long the submitting thread is held
  device_ms      time between two device events bracketing the call: the span on the stream, waits for the host included
  blocked_ms     of host_ms, the time spent inside the device -> host reads (a separate set of windows, with the reads instrumented)
  host_reads / abi_calls / conv_launches     counted in a separate call, never in a timed one
  level_counts   active voxels per resolution
Every figure is a median over --iters windows with min / max / quartiles; every window starts after a synchronise, on a warmed-up path.
A run without a GPU is refused: a time taken on the CPU says nothing about this path.  Writes profiles/lidar_producer_bench.json (--out).

    python tools/bench_lidar_producer.py [--iters 30] [--warmup 5] [--points 381920] [--out profiles/lidar_producer_bench.json]
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch

SWEEPS, POINTS_PER_SWEEP = 11, 34720


def spread(v):
    """median / min / max / quartiles of a list of samples, rounded to 0.1 us (values in ms)."""
    v = sorted(float(x) for x in v)
    q = statistics.quantiles(v, n=4) if len(v) >= 2 else [v[0]] * 3
    return dict(median=round(statistics.median(v), 4), min=round(v[0], 4), max=round(v[-1], 4), p25=round(q[0], 4), p75=round(q[2], 4),
                n=len(v))


def require_gpu():
    if not torch.cuda.is_available():
        raise SystemExit("bench_lidar_producer: no GPU -- the producer runs on the GPU only and a CPU timing says nothing about it")


class Probe:
    """Counts (and times) what the calling thread does inside a block: device -> host reads through ``Tensor.item`` / ``tolist``,
    C-ABI calls through ``_lib.call`` and convolution launches through ``_lib.conv_fwd``.  Not used in the timed windows."""

    def __init__(self):
        self.reads, self.blocked_s, self.abi_calls, self.conv_launches = 0, 0.0, 0, 0

    def __enter__(self):
        from co_occ_amd import _lib
        self._lib = _lib
        self._item, self._tolist, self._conv = torch.Tensor.item, torch.Tensor.tolist, _lib.conv_fwd
        self._fns = dict(_lib._fns)
        probe = self

        def timed(fn):
            def inner(t, *a, **k):
                t0 = time.perf_counter()
                try:
                    return fn(t, *a, **k)
                finally:
                    probe.reads += 1
                    probe.blocked_s += time.perf_counter() - t0
            return inner

        def counted(fn):
            def inner(*a):
                probe.abi_calls += 1
                return fn(*a)
            return inner

        def conv(desc, device):
            probe.conv_launches += 1
            return probe._conv(desc, device)

        torch.Tensor.item, torch.Tensor.tolist = timed(self._item), timed(self._tolist)
        for name, fn in self._fns.items():
            _lib._fns[name] = counted(fn)
        _lib.conv_fwd = conv
        return self

    def __exit__(self, *exc):
        torch.Tensor.item, torch.Tensor.tolist = self._item, self._tolist
        self._lib._fns.update(self._fns)
        self._lib.conv_fwd = self._conv
        return False


def build(dev, seed=0):
    from co_occ_amd import lidar as L, synth
    cfg = synth.lidar_cfg()
    mods = (L.Voxelization(**cfg["pts_voxel_layer"]), L.VOXEL_ENCODERS.build(dict(cfg["pts_voxel_encoder"])),
            L.MIDDLE_ENCODERS.build(dict(cfg["pts_middle_encoder"])))
    mods[2].load_state_dict(synth.random_state_dict(mods[2].state_dict(), seed=seed))
    return tuple(m.to(dev).eval() for m in mods), cfg


def producer(mods, pts):
    vox, vfe, enc = mods
    voxels, coors, num = vox(pts)
    return enc(vfe(voxels, num, coors), coors, 1), coors


def level_counts(mods, coors):
    from co_occ_amd import lidar as L
    cur, counts = L.SparseRows(None, coors, mods[2].sparse_shape_xyz[::-1]), [int(coors.shape[0])]
    for _ in range(3):
        co, shape, _ = cur.downsample(3, 2, 1)
        counts.append(int(co.shape[0]))
        cur = L.SparseRows(None, co, shape)
    return counts


def window(fn):
    """(host ms until the call returns, device ms between events around it); starts and ends synchronised."""
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    e0.record()
    fn()
    host = (time.perf_counter() - t0) * 1e3
    e1.record()
    torch.cuda.synchronize()
    return host, e0.elapsed_time(e1)


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--iters", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--points", type=int, default=SWEEPS * POINTS_PER_SWEEP)
    ap.add_argument("--seed", type=int, default=8)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "lidar_producer_bench.json"))
    a = ap.parse_args(argv)
    require_gpu()
    from co_occ_amd import core, synth
    dev = torch.device("cuda:0")
    mods, cfg = build(dev)
    pts = synth.lidar_points(n=a.points, seed=a.seed).to(dev)
    run = lambda: producer(mods, pts)
    with torch.no_grad():
        for _ in range(max(1, a.warmup)):
            out, coors = run()
        torch.cuda.synchronize()
        core.check_h2_overflow()
        counts = level_counts(mods, coors)
        with Probe() as p:                                   # counted in a call of its own
            run()
            torch.cuda.synchronize()
        plain = [window(run) for _ in range(a.iters)]
        blocked = []
        for _ in range(a.iters):                             # the same windows with the reads instrumented
            with Probe() as q:
                window(run)
            blocked.append(q.blocked_s * 1e3)
    result = dict(device=torch.cuda.get_device_name(0), torch=torch.__version__, iters=a.iters, warmup=a.warmup, points=int(pts.shape[0]),
                  sparse_shape_xyz=list(cfg["pts_middle_encoder"]["sparse_shape_xyz"]), max_voxels=list(cfg["pts_voxel_layer"]["max_voxels"]),
                  level_counts=counts, volume=list(out["x"].shape), host_reads=p.reads, abi_calls=p.abi_calls, conv_launches=p.conv_launches,
                  host_ms=spread([h for h, _ in plain]), device_ms=spread([d for _, d in plain]), blocked_ms=spread(blocked))
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    print(json.dumps(result))
    return result


if __name__ == "__main__":
    main()
