"""What the data-parallel arena path of ``co_occ_amd.optim.AdamW`` costs on ONE GPU: the r50 multi-modal detector's
trainable tensors (tools/bench_optim.py's set), the clipped step through the arena (``dp_always``: pack, flag check, norm and update
from the arena, no collective) against two baselines measured in the same run, the paths alternating:

  plain          ``optim.AdamW(max_grad_norm=5)`` without a group: the single-rank path.  arena - plain is what the arena costs.
  torch_flatten  torch's way to make one flat averaged buffer: ``torch._foreach_div_`` on (persistent) clones of the gradients,
                 then ``torch.cat`` of their flattened views.  The clones are made once, outside the timed region.

and the pack launch alone (with its table upload), at world = 8 (the division) and world = 1 (the copy).  The all-reduce itself is
NOT timed anywhere here: it cannot be on one GPU.  Writes profiles/optim_dp_bench.json (or --out).

Timing as in tools/bench_optim.py: device events around every call, median of --iters rounds with the min / max spread; host_ms is
the host clock until the call returns, without a final synchronise.  Per-kernel times come from a round of their own with device
events right around each launch (``kernels``, ``pack_kernel``): a call's time includes the host filling and uploading the tables.

    python tools/bench_optim_dp.py [--iters 20] [--warmup 3] [--out profiles/optim_dp_bench.json]
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

import torch

import bench_optim as B
from co_occ_amd import _lib, optim

WORLD = 8


def make_arena_path(spec, dev):
    path = B.make_path("device", spec, dev)
    path["opt"].dp_always = True
    return path


def make_pack_path(arena_path, world):
    """The pack launch alone, into the arena path's own arena (its next step packs again)."""
    red = arena_path["opt"]._reducer
    sources = [p.grad for p in red.tensors]
    return dict(step=lambda: red.pack(sources, world).done())


def make_flatten_path(spec, dev, world):
    g = torch.Generator(device=dev).manual_seed(1)
    clones = [torch.randn(s, generator=g, device=dev) * 1e-3 for s, _ in spec]
    out = {}

    def step():
        torch._foreach_div_(clones, float(world))
        out["flat"] = torch.cat([c.reshape(-1) for c in clones])
    return dict(step=step, out=out)


def kernel_times(paths, pack_key, iters):
    """A round of its own, never a timed one: device events right around every launch (the library's per-launch timer), so the
    table fill and upload stay outside.  {kernel: ms per launch} of the arena step's kernels, and of the pack launch at world = 8."""
    out = {}
    for key in ("arena", pack_key):
        _lib.TIMER.enabled, _lib.TIMER.only = 1, ("k_optim",)
        _lib.TIMER.reset()
        for _ in range(iters):
            paths[key]["step"]()
        torch.cuda.synchronize()
        summary = _lib.TIMER.summary()
        _lib.TIMER.enabled, _lib.TIMER.only = False, None
        _lib.TIMER.reset()
        out[key] = {k: dict(launches_per_call=v["launches"] // iters, ms=round(v["ms"] / v["launches"], 4),
                            gbs=round(v["work"] / v["ms"] / 1e6, 1)) for k, v in sorted(summary.items())}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "optim_dp_bench.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_optim_dp: needs the GPU (a CPU timing says nothing about it)")
    dev = torch.device("cuda:0")
    spec = B.shapes_and_decay(B.detector())
    numels = [int(torch.Size(s).numel()) for s, _ in spec]
    elements = sum(numels)
    paths = dict(plain=B.make_path("device", spec, dev), arena=make_arena_path(spec, dev))
    B.timed(paths["arena"])                             # the first arena step: layout and arena
    B.timed(paths["plain"])                             # ... and the same number of steps on the plain path
    paths["pack_world%d" % WORLD] = make_pack_path(paths["arena"], WORLD)
    paths["pack_world1"] = make_pack_path(paths["arena"], 1)
    paths["torch_flatten"] = make_flatten_path(spec, dev, WORLD)
    for _ in range(a.warmup):
        for p in paths.values():
            B.timed(p)
    rounds = {k: [] for k in paths}
    for _ in range(a.iters):
        for k, p in paths.items():
            rounds[k].append(B.timed(p))
    # both optimizers stepped the same number of times from the same start on the same gradients: the arena path is the plain path's
    # bits (compared here, before the kernel round steps the arena path alone)
    pa, pb = paths["plain"]["params"], paths["arena"]["params"]
    same_bits = all(torch.equal(x.detach().view(torch.int32), y.detach().view(torch.int32)) for x, y in zip(pa, pb))
    kernels = kernel_times(paths, "pack_world%d" % WORLD, a.iters)
    chunks = int(optim.chunk_table(numels).shape[0])
    lay = optim.arena_layout(numels)
    table_bytes = len(spec) * optim.TENSOR_DTYPE.itemsize + chunks * 16
    result = dict(device=torch.cuda.get_device_name(0), iters=a.iters, warmup=a.warmup, tensors=len(spec), elements=elements,
                  chunk=optim.chunk_size(), chunks=chunks, arena_elements=lay.total, arena_bytes=4 * lay.total, world_for_division=WORLD,
                  max_norm=B.MAX_NORM, hbm_peak_gbs=B.HBM_PEAK_GBS,
                  timing="device events per call, median of iters, paths alternating in one process; host_ms = host clock until the call "
                         "returns, no final synchronise; pack_* = one k_optim_pack launch with its table upload",
                  collective="NOT timed: one GPU.  The arena path ran with dp_always (pack, flag check, norm and update from the "
                             "arena; no all-reduce)",
                  paths={})
    for k in paths:
        result["paths"][k] = dict(call_ms=B.spread([r[0] for r in rounds[k]]), host_ms=B.spread([r[1] for r in rounds[k]]))
    for k in ("pack_world%d" % WORLD, "pack_world1"):
        d = result["paths"][k]
        d["bytes_moved"] = 8 * elements + 2 * table_bytes          # 4 read + 4 written per element; the tables uploaded and read
        d["achieved_gbs"] = round(d["bytes_moved"] / d["call_ms"]["median"] / 1e6, 1)
        d["share_of_hbm_peak"] = round(d["bytes_moved"] / d["call_ms"]["median"] / 1e6 / B.HBM_PEAK_GBS, 4)
    fl = result["paths"]["torch_flatten"]
    fl["bytes_moved"] = 16 * elements                              # the division reads and writes 4 + 4, the cat reads and writes 4 + 4
    fl["achieved_gbs"] = round(fl["bytes_moved"] / fl["call_ms"]["median"] / 1e6, 1)
    plain, arena = result["paths"]["plain"]["call_ms"]["median"], result["paths"]["arena"]["call_ms"]["median"]
    pack = result["paths"]["pack_world%d" % WORLD]["call_ms"]["median"]
    result["kernels"] = kernels                                    # events right around each launch, in a round of their own
    pk = kernels["pack_world%d" % WORLD]["k_optim_pack"]
    result["pack_kernel"] = dict(ms=pk["ms"], bytes_moved=8 * elements, achieved_gbs=pk["gbs"],
                                 share_of_hbm_peak=round(pk["gbs"] / B.HBM_PEAK_GBS, 4),
                                 note="8 B per element over the launch alone (no table fill or upload), world = %d" % WORLD)
    result["arena_minus_plain_ms"] = round(arena - plain, 4)
    result["arena_over_plain"] = round(arena / plain, 4)
    result["torch_flatten_over_pack"] = round(fl["call_ms"]["median"] / pack, 3)
    result["host_arena_over_plain"] = round(result["paths"]["arena"]["host_ms"]["median"] / result["paths"]["plain"]["host_ms"]["median"], 3)
    result["arena_equals_plain_bitwise"] = same_bits
    print(json.dumps(result))
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(result, fh, indent=1, sort_keys=True)
        fh.write("\n")
    print("wrote", a.out)


if __name__ == "__main__":
    main()
