"""The occupancy pictures (co_occ_amd/visualize.py, csrc/occ_views.hip) at the reference's picture sizes -- six camera views of
480 x 270 at 4 x 4 samples a pixel, the driving view of 1920 x 1080 and columns 460:1460 of the bird's-eye view at 2 x 2: 25.1 M
samples -- on a synthetic volume of about 5 % fill (half of a ground layer plus scattered voxels):
  200x200x16    the nuScenes grid: brick flags in LDS, column words read from memory (the default: 80 KiB of masks exceed the
                16 KiB budget), and a second time with both staged in LDS (``lds_budget_bytes`` = 80 KiB, two workgroups a CU)
  512x512x40    the OpenOccupancy grid: brick flags in LDS, column words read from memory
Per grid: the prepare launch, the three cast launches (cameras, driving view, bird's-eye window) and the whole
``draw_nusc_occupancy`` call (kernels, the copy of the pictures to the host, the composition; no files); the mask reads the walks
took, counted per sample by the kernel in a separate untimed call, and the share of them that LDS served (brick flags always, column
words where they are staged); and
for scale the numpy brute-force restatement (tests/occ_view_refs.py) on one host core, timed on 256 samples of the driving view and
scaled to the picture's sample count.  Writes profiles/occ_views_bench.json (or --out).

Timing: every step is warmed up; a timed window is one call bracketed by device events on the stream after a synchronise (the whole
call: the host clock), reported as the median of --iters windows with the min / max spread.

    python tools/bench_occ_views.py [--iters 10] [--warmup 2] [--out profiles/occ_views_bench.json]
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

import occ_view_refs as R
from co_occ_amd import visualize as VZ

# name -> (shape, ground layer, scattered share, lds_budget_bytes)
GRIDS = {"200x200x16": ((200, 200, 16), 2, 0.02, 0), "200x200x16_words_in_lds": ((200, 200, 16), 2, 0.02, 81920),
         "512x512x40": ((512, 512, 40), 5, 0.0375, 0)}
PC_RANGE = [-51.2, -51.2, -5.0, 51.2, 51.2, 3.0]


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


def volume(shape, ground, scatter, seed):
    rng = np.random.default_rng(seed)
    fill = rng.random(shape) < scatter
    fill[:, :, ground] |= rng.random(shape[:2]) < 0.5
    return np.where(fill, rng.integers(1, 17, size=shape), 0).astype(np.uint8)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "occ_views_bench.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_occ_views: needs the GPU (a CPU timing says nothing about it)")
    dev = torch.device("cuda:0")
    cam2lidar = R.rig(1.5, 1.8)
    cams = VZ.view_cameras(cam2lidar)
    (cw, ch), (pw, ph), (b0, b1) = VZ.CAM_IMG_SIZE, VZ.PRED_IMG_SIZE, VZ.BEV_WINDOW
    samples = 6 * cw * ch * 16 + pw * ph * 4 + (b1 - b0) * ph * 4
    result = dict(device=torch.cuda.get_device_name(0), iters=a.iters, warmup=a.warmup, samples_per_picture=samples,
                  timing="one call per window: device events (whole call: host clock) around it after a synchronise, median of iters windows "
                         "with min / max", grids={})
    for name, (shape, ground, scatter, budget) in GRIDS.items():
        lab = volume(shape, ground, scatter, 7)
        origin, vs = VZ.grid_of(list(shape), PC_RANGE)
        labels = torch.from_numpy(lab).to(dev)
        draw, masks = VZ.prepare(labels)
        steps = {
            "prepare": lambda: VZ.prepare(labels),
            "cast_6_cameras_480x270_s4": lambda d=False: VZ.cast_views(draw, masks, VZ.view_rows(cams[:6]), origin, vs, (cw, ch), 4, None, d, budget),
            "cast_driving_1920x1080_s2": lambda d=False: VZ.cast_views(draw, masks, VZ.view_rows(cams[6:7]), origin, vs, (pw, ph), 2, None, d, budget),
            "cast_birds_eye_1000x1080_s2": lambda d=False: VZ.cast_views(draw, masks, VZ.view_rows(cams[7:8], b0), origin, vs, (b1 - b0, ph), 2,
                                                                          (pw, ph), d, budget),
        }
        entry = dict(fill=round(float(((draw > 0) & (draw < 20)).float().mean()), 4), mask_bytes=int(masks.numel()))
        for key, fn in steps.items():
            for _ in range(a.warmup):
                window(fn)
            entry[key + "_device_ms"] = spread([window(fn)[0] for _ in range(a.iters)])
        flags = words = 0
        for key, fn in list(steps.items())[1:]:                       # counted in calls of their own, never in a timed one
            out = fn(True)
            flags, words, where = flags + int(out.reads[..., 0].sum()), words + int(out.reads[..., 1].sum()), out.cell_bits
            del out
        lds = flags + (words if where == "lds" else 0)
        entry["mask_reads"] = dict(brick_flags=flags, column_words=words, column_words_from=where, per_sample=round((flags + words) / samples, 2),
                                   lds_share=round(lds / max(1, flags + words), 4))
        whole = lambda: VZ.draw_nusc_occupancy(None, labels, origin, vs, cam2lidar=cam2lidar, lds_budget_bytes=budget)
        for _ in range(a.warmup):
            window(whole)
        entry["draw_nusc_occupancy_wall_ms"] = spread([window(whole)[1] for _ in range(a.iters)])
        # for scale only: the brute-force restatement, one core, 256 samples of the driving view
        torch.set_num_threads(1)
        d = draw.cpu().numpy()
        rng = np.random.default_rng(1)
        gx, gy = rng.integers(0, pw * 2, 256), rng.integers(0, ph * 2, 256)
        t0 = time.perf_counter()
        R.cast_samples(d, origin, vs, R.view_rows(cams[6:7])[0], gx, gy, 2, pw, ph, chunk=32)
        dt = time.perf_counter() - t0
        entry["numpy_brute_force_one_core"] = dict(ms_per_256_samples=round(dt * 1e3, 1), scaled_to_the_picture_hours=round(dt / 256 * samples / 3600, 1),
                                                   note="every sample against every drawn cube; for scale only")
        result["grids"][name] = entry
        print(name, json.dumps(entry))
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(result, fh, indent=1, sort_keys=True)
        fh.write("\n")
    print("wrote", a.out)


if __name__ == "__main__":
    main()
