"""The camera img_inputs kernel (co_occ_amd/image_inputs.py, csrc/image_inputs.hip) at the two configuration shapes, 6 x 900 x 1600
frames -> 6 x 3 x 256 x 704 (r50: resize 0.44, crop) and -> 6 x 3 x 896 x 1600 (r101: crop only), against
  (a) what it replaces: Pillow + numpy + torch on this host for the same six frames, one thread, and the pinned-host upload of the
      resulting fp32 tensor compared with the upload of the frame bytes;
  (b) the nearest plain-torch expression on the same GPU: bytes -> float, F.interpolate(mode='bicubic', antialias=True), crop, / 255.
      It is NOT bit-equal to Pillow (no uint8 rounding between the passes, float coefficients); its largest difference is recorded.
Writes profiles/image_inputs_bench.json (or --out).

Timing: every shape is warmed up, the device paths alternate inside one process, every call is bracketed by device events on the
stream, the median of --iters rounds is reported with the min / max spread.  The host path is timed with the host clock
(--host-iters rounds).  Bytes are computed from the shapes: the source rectangle the kept pixels' taps span, the fp32 planes and the
canvas; the HBM fraction is those bytes over the median device time over 8.0 TB/s (spec) and 6.29 TB/s (measured float4 copy).
Launch counts come from a separate profiled round, never from a timed one; where the profiler gives nothing the count is null.

    python tools/bench_image_inputs.py [--iters 30] [--warmup 5] [--host-iters 5] [--out profiles/image_inputs_bench.json]
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
import torch.nn.functional as F

from co_occ_amd import image_inputs as II

N, HS, WS = 6, 900, 1600
SHAPES = {"r50_6x256x704": dict(input_size=(256, 704)), "r101_6x896x1600": dict(input_size=(896, 1600))}
HBM_SPEC, HBM_MEASURED = 8.0e12, 6.29e12


def params(input_size):
    cfg = dict(input_size=input_size, crop_h=(0.0, 0.0), resize_test=0.0)
    return II.sample_augmentation(cfg, HS, WS, False)


def traffic(plan):
    """Bytes the kernel has to move: per camera the source rectangle its kept pixels' taps span, the fp32 planes, the canvas."""
    read = 0
    for (newW, newH), crop, _ in plan.cams:
        span = []
        for size, new, lo, hi in ((WS, newW, crop[0], crop[2]), (HS, newH, crop[1], crop[3])):
            a, b = max(lo, 0), min(hi, new)
            if a >= b:
                span.append(0)
            elif new == size:
                span.append(b - a)
            else:
                bounds = II.pillow_coeffs(size, new)[0]
                span.append(int(bounds[b - 1].sum() - bounds[a, 0]))
        read += span[0] * span[1] * 3
    written = plan.N * plan.fH * plan.fW * (3 * 4 + 3)
    return read, written


def torch_expression(frames, resize_dims, crop):
    x = frames.permute(0, 3, 1, 2).float()
    newW, newH = resize_dims
    if (newH, newW) != tuple(x.shape[-2:]):
        x = F.interpolate(x, size=(newH, newW), mode='bicubic', antialias=True, align_corners=False)
    return x[:, :, crop[1]:crop[3], crop[0]:crop[2]].contiguous() / 255.


def host_path(frames_np, resize_dims, crop):
    """The reference's per-camera work: Image.resize, crop, (no flip), rotate(0), np.array -> torch float, permute, / 255, stack."""
    from PIL import Image
    imgs = []
    for f in frames_np:
        img = Image.fromarray(f).resize(resize_dims).crop(crop).rotate(0)
        imgs.append(torch.tensor(np.array(img)).float().permute(2, 0, 1).contiguous() / 255.)
    return torch.stack(imgs)


def device_timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1)


def launches(fn, marker):
    try:
        from torch.profiler import ProfilerActivity, profile
        with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
            fn()
            torch.cuda.synchronize()
        dev_ev = [e for e in prof.events() if str(getattr(e, "device_type", "")).endswith("CUDA")]
        kern = [e.name for e in dev_ev if not e.name.lower().startswith(("memcpy", "memset"))]
        if not kern:
            return dict(kernels=None, note="the profiler recorded no device activity")
        return dict(kernels=len(kern), package_kernels=sorted(set(k for k in kern if marker in k)))
    except Exception as exc:                      # not measured
        return dict(kernels=None, note="profiler unavailable: %s" % type(exc).__name__)


def spread(v):
    return dict(median=round(statistics.median(v), 4), min=round(min(v), 4), max=round(max(v), 4))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--host-iters", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "image_inputs_bench.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_image_inputs: needs the GPU (a CPU timing says nothing about it)")
    dev = torch.device("cuda:0")
    torch.set_num_threads(1)
    frames_np = np.random.default_rng(0).integers(0, 256, (N, HS, WS, 3), dtype=np.uint8)
    frames_pinned = torch.from_numpy(frames_np).pin_memory()
    frames = frames_pinned.to(dev)
    result = dict(device=torch.cuda.get_device_name(0), iters=a.iters, warmup=a.warmup, host_iters=a.host_iters, cameras=N,
                  frame_size=[HS, WS], host_threads=torch.get_num_threads(), host_cpus_usable=len(os.sched_getaffinity(0)),
                  timing="device events per call, median of iters, the two device paths alternating; host path: host clock, one thread",
                  shapes={})
    for name, shape in SHAPES.items():
        resize, resize_dims, crop, flip, _ = params(shape["input_size"])
        plan = II.ResizePlan(HS, WS, [(resize_dims, crop, flip)] * N, shape["input_size"], device=dev)
        out = torch.empty((N, 3) + tuple(shape["input_size"]), device=dev)
        canvas = torch.empty((N,) + tuple(shape["input_size"]) + (3,), dtype=torch.uint8, device=dev)
        paths = {"kernel": lambda: II.frames_to_imgs(frames, plan, out=out, canvas=canvas),
                 "torch_expression": lambda: torch_expression(frames, resize_dims, crop)}
        for _ in range(a.warmup):
            for fn in paths.values():
                device_timed(fn)
        rounds = {k: [] for k in paths}
        for _ in range(a.iters):
            for k, fn in paths.items():
                rounds[k].append(device_timed(fn))
        read, written = traffic(plan)
        entry = dict(resize=resize, resize_dims=list(resize_dims), crop=list(crop), bytes_read=read, bytes_written=written)
        for k, fn in paths.items():
            entry[k] = dict(call_ms=spread(rounds[k]), launches=launches(fn, "k_frames"))
        t = entry["kernel"]["call_ms"]["median"] * 1e-3
        entry["kernel"]["hbm_fraction_of_spec"] = round((read + written) / t / HBM_SPEC, 4)
        entry["kernel"]["hbm_fraction_of_measured_copy"] = round((read + written) / t / HBM_MEASURED, 4)
        entry["torch_expression_over_kernel"] = round(entry["torch_expression"]["call_ms"]["median"] / entry["kernel"]["call_ms"]["median"], 3)
        got = paths["torch_expression"]()
        entry["torch_expression"]["bit_equal_to_kernel"] = bool(torch.equal(got, out))
        entry["torch_expression"]["max_abs_diff_in_bytes"] = float("%.4g" % (float((got - out).abs().max()) * 255))
        # (a) the host path and the two uploads
        try:
            host = []
            for _ in range(a.host_iters):
                t0 = time.perf_counter()
                want = host_path(frames_np, resize_dims, crop)
                host.append((time.perf_counter() - t0) * 1e3)
            entry["host_pillow_numpy_torch"] = dict(call_ms=spread(host), threads=1)
            entry["kernel"]["bit_equal_to_host_path"] = bool(torch.equal(out.cpu(), want))
            fp32_pinned = want.pin_memory()
            ups = {"fp32_upload": lambda: fp32_pinned.to(dev, non_blocking=True), "bytes_upload": lambda: frames_pinned.to(dev, non_blocking=True)}
            for _ in range(2):
                for fn in ups.values():
                    device_timed(fn)
            ur = {k: [] for k in ups}
            for _ in range(a.host_iters * 2):
                for k, fn in ups.items():
                    ur[k].append(device_timed(fn))
            entry["fp32_upload"] = dict(call_ms=spread(ur["fp32_upload"]), bytes=int(want.numel() * 4))
            entry["bytes_upload"] = dict(call_ms=spread(ur["bytes_upload"]), bytes=int(frames_np.size))
            del fp32_pinned
        except ImportError as exc:
            entry["host_pillow_numpy_torch"] = dict(call_ms=None, note="not measured: %s" % exc)
        result["shapes"][name] = entry
        print(name, json.dumps(entry))
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(result, fh, indent=1, sort_keys=True)
        fh.write("\n")
    print("wrote", a.out)


if __name__ == "__main__":
    main()
