"""Per-kernel times of the SSIM of the rendered colour maps (csrc/render_ssim.hip) and of its yardstick, the torch-on-GPU
restatement of the same definition (tests/render_ssim_ref.py ``ssim_torch``: five ``avg_pool2d(7, stride=1)`` passes per view plus
the pointwise chain), from one kernel trace per map size.

    rocprofv3 --kernel-trace --stats --output-format csv -d OUT/r50 -- python tools/time_render_ssim.py run r50
    rocprofv3 --kernel-trace --stats --output-format csv -d OUT/r101 -- python tools/time_render_ssim.py run r101
    python tools/time_render_ssim.py report OUT > profiles/render_ssim_kernels.txt

``run`` launches, on seeded maps resident in HBM, ITERS + 1 times the HIP pair and then ITERS + 1 times the restatement (the first
of each is the check that both give the same answer), and prints the event-timed mean of each as a cross-check.  ``report`` reads
the traces: the median duration of each HIP kernel over its launches, the achieved share of the 8 TB/s HBM peak from the bytes the
pass must move (24 B per pixel: rgbs and gt_img once), and the restatement's kernel time per iteration (its launches cut into
ITERS + 1 equal groups, the median of the group sums)."""
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
BYTES_PER_PIXEL = 24.0
MINE = ("k_render_ssim_part", "k_render_ssim_final")


def run(name):
    import torch
    import render_ssim_ref as S
    from co_occ_amd import evaluation as E
    assert torch.cuda.is_available(), "the timing needs the GPU"
    dev = torch.device("cuda:0")
    N, H, W = SIZES[name]
    g = torch.Generator().manual_seed(1)
    rgbs = (torch.rand(N, H, W, 3, generator=g) * 1.4 - 0.2).to(dev)
    gt_img = (torch.rand(N, 3, H, W, generator=g) * 1.6 - 0.3).to(dev)
    torch.cuda.synchronize()

    def hip():
        return E.render_ssim(rgbs, gt_img)

    def restatement():
        return S.ssim_torch(rgbs, gt_img)
    a, b = hip(), restatement()                        # same answer before any timing
    err = float((a[:, E.RS_SSIM].float() - b[0]).abs().max())
    assert err <= 1e-4, "HIP SSIM differs from the restatement's on the GPU: %.3e" % err
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
    print("SSIM of the rendered colour maps (csrc/render_ssim.hip) and the torch-on-GPU restatement of the same definition")
    print("(tests/render_ssim_ref.py ssim_torch): rocprofv3 --kernel-trace --stats, one run per size, no counters in the same run.")
    print("Median over the launches; share of the 8 TB/s HBM peak at 24 B per pixel (rgbs and gt_img read once), for both sides.\n")
    for name, (N, H, W) in SIZES.items():
        rows = _rows(os.path.join(out, name))
        pix = N * H * W
        mine = {}
        for _, dur, k in rows:
            for key in MINE:
                if key in k:
                    mine.setdefault(key, []).append(dur)
        # the restatement: every other kernel after the first HIP launch; the check and the timed loop launch ITERS + 1 identical
        # iterations
        first = min(s for s, _, k in rows if MINE[0] in k)
        other = [dur for s, dur, k in rows if s > first and "k_render_ssim" not in k]
        per = len(other) // (ITERS + 1)
        groups = [sum(other[i * per:(i + 1) * per]) for i in range(ITERS + 1)] if per else [0]
        share = lambda ns: "%5.2f TB/s = %4.1f %% of the HBM peak" % (BYTES_PER_PIXEL * pix / ns / 1e3, 100 * BYTES_PER_PIXEL * pix / (ns * 1e-9) / HBM_PEAK)
        print("%s maps %d x %d x %d (%.2f Mpixel, %.1f MB at 24 B per pixel)" % (name, N, H, W, pix / 1e6, BYTES_PER_PIXEL * pix / 1e6))
        pair = 0.0
        for key in MINE:
            med = _median(mine[key])
            pair += med
            print("  %-22s %4d launches   median %9.1f us" % (key, len(mine[key]), med / 1e3))
        rest = _median(groups)
        print("  HIP pair               2 launches per call   sum of the two medians %9.1f us   %s" % (pair / 1e3, share(pair)))
        print("  torch restatement   %4d launches per call   median of the per-call sums %9.1f us   %s" % (per, rest / 1e3, share(rest)))
        print("  restatement / HIP pair = %.1f x   (%s)\n" % (rest / pair, "the pair is below the yardstick" if pair < rest
                                                                 else "THE PAIR IS NOT BELOW THE YARDSTICK"))


if __name__ == "__main__":
    if sys.argv[1] == "run":
        run(sys.argv[2])
    else:
        report(sys.argv[2])
