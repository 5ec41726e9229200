"""Per-kernel times of the render evaluation (csrc/render_eval.hip) and of its yardstick, the torch-on-GPU restatement of the same
reference lines (tests/render_eval_ref.py), from one kernel trace per map size.

    rocprofv3 --kernel-trace --stats -d OUT/r50 -- python tools/time_render_eval.py run r50
    rocprofv3 --kernel-trace --stats -d OUT/r101 -- python tools/time_render_eval.py run r101
    python tools/time_render_eval.py report OUT > profiles/render_eval_kernels.txt

``run`` launches, on seeded maps resident in HBM, ITERS times the HIP pair (stats with gt_depth, then panels) and ITERS times the
restatement (PSNR per view, panels, masked squared depth error), and prints the event-timed mean of each as a cross-check.
``report`` reads the traces: the median duration of each HIP kernel over its launches, the achieved share of the 8 TB/s HBM peak from
the bytes the kernels must move (stats: 28 B per pixel read; panels: 28 B read + 9 B written), and the restatement's kernel time per
iteration (its launches cut into ITERS equal groups, the median of the group sums)."""
import csv
import glob
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

SIZES = {"r50": (6, 256, 704), "r101": (6, 896, 1600)}
ITERS = 24
HBM_PEAK = 8.0e12
BYTES = {"k_render_eval_part": 28.0, "k_render_panels": 37.0}       # per pixel


def run(name):
    import torch
    import render_eval_ref as R
    from co_occ_amd import evaluation as E
    assert torch.cuda.is_available(), "the timing needs the GPU"
    dev = torch.device("cuda:0")
    N, H, W = SIZES[name]
    g = torch.Generator().manual_seed(1)
    rgbs = (torch.rand(N, H, W, 3, generator=g) * 1.4 - 0.2).to(dev)
    gt_img = (torch.rand(N, 3, H, W, generator=g) * 1.6 - 0.3).to(dev)
    depths = (torch.rand(N, H, W, generator=g) * 56 + 2).to(dev)
    gt_depth = torch.rand(N, H, W, generator=g) * 58 + 1
    gt_depth[torch.rand(N, H, W, generator=g) < 0.4] = 0
    gt_depth = gt_depth.to(dev)
    torch.cuda.synchronize()

    def hip():
        return E.render_eval(rgbs, depths, gt_img, gt_depth, panels=True)

    def restatement():
        return R.psnr(rgbs, gt_img), R.panels(rgbs, depths, gt_img), R.depth_error(depths, gt_depth)
    a, b = hip(), restatement()                        # same answer before any timing
    assert torch.equal(a["panels"], b[1]), "HIP panels differ from the restatement's on the GPU"
    assert float((a["psnr"] - b[0][0]).abs().max()) <= 1e-4 * max(1.0, float(b[0][0].abs().max()))
    for what, fn in (("hip pair", hip), ("torch restatement", restatement)):
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(ITERS):
            fn()
        e1.record()
        torch.cuda.synchronize()
        print("%s %-18s %8.1f us per iteration (events around %d iterations, tracer attached)" % (name, what, e0.elapsed_time(e1) * 1e3 / ITERS, ITERS))


def _rows(d):
    files = glob.glob(os.path.join(d, "**", "*kernel_trace.csv"), recursive=True)
    assert files, "no kernel trace under " + d
    rows = []
    for f in files:
        for r in csv.DictReader(open(f)):
            rows.append((int(r["Start_Timestamp"]), int(r["End_Timestamp"]) - int(r["Start_Timestamp"]), r["Kernel_Name"]))
    return sorted(rows)


def _median(v):
    v = sorted(v)
    return v[len(v) // 2] if len(v) % 2 else 0.5 * (v[len(v) // 2 - 1] + v[len(v) // 2])


def report(out):
    print("Render evaluation kernels (csrc/render_eval.hip) and the torch-on-GPU restatement of the same reference lines")
    print("(tests/render_eval_ref.py): rocprofv3 --kernel-trace --stats, one run per size, no counters in the same run.")
    print("Median over the launches; share of the 8 TB/s HBM peak from 28 B (stats) / 37 B (panels) per pixel.\n")
    for name, (N, H, W) in SIZES.items():
        rows = _rows(os.path.join(out, name))
        pix = N * H * W
        mine = {}
        for _, dur, k in rows:
            for key in ("k_render_eval_part", "k_render_eval_final", "k_render_panels"):
                if key in k:
                    mine.setdefault(key, []).append(dur)
        # the restatement: every other kernel after the first HIP launch of the timed loops; the check and the timed loop
        # launch ITERS + 1 identical iterations
        first = min(s for s, _, k in rows if "k_render_eval_part" in k)
        other = [dur for s, dur, k in rows if s > first and "k_render" not in k]
        per = len(other) // (ITERS + 1)
        groups = [sum(other[i * per:(i + 1) * per]) for i in range(ITERS + 1)] if per else [0]
        print("%s maps %d x %d x %d (%.2f Mpixel)" % (name, N, H, W, pix / 1e6))
        pair = 0.0
        for key in ("k_render_eval_part", "k_render_eval_final", "k_render_panels"):
            med = _median(mine[key])
            pair += med
            share = ("   %5.2f TB/s = %4.1f %% of the HBM peak" % (BYTES[key] * pix / med / 1e3, 100 * BYTES[key] * pix / (med * 1e-9) / HBM_PEAK)) if key in BYTES else ""
            print("  %-22s %4d launches   median %9.1f us%s" % (key, len(mine[key]), med / 1e3, share))
        rest = _median(groups)
        print("  %-22s %4d kernels per iteration   median of the per-iteration sums %9.1f us" % ("torch restatement", per, rest / 1e3))
        print("  HIP pair (sum of the three medians) %9.1f us   restatement / HIP pair = %.1f x\n" % (pair / 1e3, rest / pair))


if __name__ == "__main__":
    if sys.argv[1] == "run":
        run(sys.argv[2])
    else:
        report(sys.argv[2])
