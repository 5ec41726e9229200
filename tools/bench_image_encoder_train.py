"""Time one training step (forward + backward) of the image encoder (``image_encoder.ResNet`` + ``image_encoder.SECONDFPN`` with
``train_enabled``, ``train()``, seeded weights) at the two sizes of the coocc_nusc configs -- 6 cameras x 256 x 704 with ResNet-50,
6 x 896 x 1600 with ResNet-101 --, each with ``frozen_stages`` 0 (the reference configs: the fused stem stays on the path) and -1
(the stem trains: StemConvFn + BN + MaxPoolRowsFn), and in the same process on the same GPU the same network as plain torch modules
(tests/ref_image_encoder.py ``TorchResNet`` / ``TorchSECONDFPN`` in ``train()``, eager fp32, TF32 off, the same parts frozen).

    python tools/bench_image_encoder_train.py [--calls 5] [--warmup 2] [--windows 3] [--sizes r50_6x256x704,...]
                                              [--out profiles/image_encoder_train_bench.json]

Per case: ms of forward + backward (loss = sum of the neck's output; HIP events around ``calls`` steps after ``warmup``, ``windows``
windows, median and spread), the peak of ``torch.cuda.max_memory_allocated`` over one step for both (``with_cp`` is ignored: this is
the activation memory without checkpointing), the torch run's ms and the ratio HIP / torch.  Per size the three kernels of
csrc/img_stem_train.hip alone, with their bytes / flops against the HBM and fp32 peaks.  Prints one JSON line."""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

SIZES = {"r50_6x256x704": (50, 6, 256, 704), "r101_6x896x1600": (101, 6, 896, 1600)}
NECK = dict(in_channels=[256, 512, 1024, 2048], upsample_strides=[0.25, 0.5, 1, 2], out_channels=[128] * 4)
FP32_PEAK_TFLOPS = 157.3      # fp32 vector peak (spec)
HBM_PEAK_GBS = 8000.0         # HBM3E spec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--windows", type=int, default=3)
    ap.add_argument("--sizes", default=",".join(SIZES))
    ap.add_argument("--frozen", default="0,-1")
    ap.add_argument("--no-torch", action="store_true", help="skip the eager torch run")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "image_encoder_train_bench.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_image_encoder_train needs the MI355X: there is no CPU fallback")
    import ref_image_encoder as R
    from co_occ_amd import core, image_encoder as IE
    from co_occ_amd._lib import call, load, ptr
    dev = torch.device("cuda:0")
    torch.backends.cudnn.allow_tf32 = False
    torch.backends.cuda.matmul.allow_tf32 = False

    def window(fn, calls):
        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        s.record()
        for _ in range(calls):
            fn()
        e.record()
        torch.cuda.synchronize()
        return s.elapsed_time(e) / calls

    def timed(fn, calls=None):
        calls = calls or a.calls
        for _ in range(a.warmup):
            fn()
        torch.cuda.synchronize()
        v = sorted(window(fn, calls) for _ in range(a.windows))
        return dict(median_ms=round(v[len(v) // 2], 4), min_ms=round(v[0], 4), max_ms=round(v[-1], 4))

    def peak_mib(fn):
        torch.cuda.synchronize()
        torch.cuda.empty_cache()
        torch.cuda.reset_peak_memory_stats()
        base = torch.cuda.memory_allocated()
        fn()
        torch.cuda.synchronize()
        return dict(peak_mib=round(torch.cuda.max_memory_allocated() / 2 ** 20, 1), resident_before_mib=round(base / 2 ** 20, 1))

    def step_of(bb, nk, x):
        params = [p for m in (bb, nk) for p in m.parameters()]

        def step():
            for p in params:
                p.grad = None
            out = nk(bb(x))[0]
            out.sum().backward()
        return step

    res = dict(workload="image_encoder.ResNet + SECONDFPN, train(), forward + backward, seeded weights, 6 cameras",
               engine=core.CONV_ENGINE, calls=a.calls, warmup=a.warmup, windows=a.windows, torch_version=torch.__version__, sizes={})
    for name in a.sizes.split(","):
        depth, BN, H, W = SIZES[name]
        x = R.fixture_images(BN, H, W, depth + 2).to(dev)
        rec = dict(depth=depth, image=[BN, 3, H, W], cases={})
        sdb = R.fixture_state_dict(IE.ResNet(depth=depth).state_dict(), depth)
        sdn = R.fixture_state_dict(IE.SECONDFPN(**NECK).state_dict(), depth + 1, R.transposed_keys(NECK["upsample_strides"]))
        for frozen in [int(v) for v in a.frozen.split(",")]:
            bb, nk = IE.ResNet(depth=depth, frozen_stages=frozen, norm_eval=False), IE.SECONDFPN(**NECK)
            bb.load_state_dict(sdb)
            nk.load_state_dict(sdn)
            bb, nk = bb.to(dev), nk.to(dev)
            bb.train_enabled = nk.train_enabled = True
            bb.train(), nk.train()
            step = step_of(bb, nk, x)
            case = dict(hip_memory=peak_mib(step), hip=timed(step))
            core.check_h2_overflow()
            del bb, nk, step
            torch.cuda.empty_cache()
            if not a.no_torch:
                tb, tn = R.TorchResNet(depth), R.TorchSECONDFPN(NECK["in_channels"], NECK["out_channels"], NECK["upsample_strides"])
                tb.load_state_dict(sdb)
                tn.load_state_dict(sdn)
                tb, tn = tb.to(dev).train(), tn.to(dev).train()
                if frozen >= 0:
                    for m in [tb.conv1, tb.bn1] + [getattr(tb, "layer%d" % i) for i in range(1, frozen + 1)]:
                        m.eval()
                        m.requires_grad_(False)
                step = step_of(tb, tn, x)
                case["torch_memory"] = peak_mib(step)
                case["torch_eager_fp32"] = timed(step)
                case["ratio_hip_over_torch"] = round(case["hip"]["median_ms"] / case["torch_eager_fp32"]["median_ms"], 4)
                del tb, tn, step
                torch.cuda.empty_cache()
            rec["cases"]["frozen_stages=%d" % frozen] = case
            print(name, frozen, json.dumps(case), file=sys.stderr, flush=True)
        # the three new kernels alone
        Hc, Wc = (H - 1) // 2 + 1, (W - 1) // 2 + 1
        Hp, Wp = (Hc - 1) // 2 + 1, (Wc - 1) // 2 + 1
        pre = torch.randn(BN * Hc * Wc, 64, device=dev)
        pooled = torch.empty(BN * Hp * Wp, 64, device=dev)
        dyp = torch.randn(BN * Hp * Wp, 64, device=dev)
        dx = torch.empty_like(pre)
        dw = torch.empty(147, 64, device=dev)
        nb = int(load().coocc_img_stem_wgrad_ws(BN, H, W))
        ws = torch.empty(nb // 4, device=dev)
        kern = dict(
            maxpool2d_rows=(lambda: call("coocc_maxpool2d_rows", ptr(pre), 64, BN, Hc, Wc, 64, ptr(pooled), 64, None),
                            9.0 * pooled.numel(), 4.0 * (pre.numel() + pooled.numel())),
            maxpool2d_rows_bwd=(lambda: call("coocc_maxpool2d_rows_bwd", ptr(pre), 64, ptr(dyp), 64, BN, Hc, Wc, 64, ptr(dx), 64),
                                0.0, 4.0 * (2 * pre.numel() + dyp.numel())),
            img_stem_wgrad=(lambda: call("coocc_img_stem_wgrad", ptr(x), BN, H, W, ptr(pre), 64, 64, ptr(dw), ptr(ws), nb),
                            2.0 * BN * Hc * Wc * 64 * 147, 4.0 * (x.numel() + pre.numel()) + 2.0 * nb))
        rec["kernels"] = {}
        for k, (fn, flops, nbytes) in kern.items():
            t = timed(fn, calls=20)
            ms = t["median_ms"]
            rec["kernels"][k] = dict(t, flops=flops, bytes=nbytes, tflops=round(flops / ms / 1e9, 2),
                                     of_fp32_peak=round(flops / ms / 1e9 / FP32_PEAK_TFLOPS, 4), gbs=round(nbytes / ms / 1e6, 1),
                                     of_hbm_peak=round(nbytes / ms / 1e6 / HBM_PEAK_GBS, 4))
        rec["kernels"]["img_stem_wgrad"]["partials"] = nb // (147 * 64 * 4)
        print(name, json.dumps(rec["kernels"]), file=sys.stderr, flush=True)
        res["sizes"][name] = rec
        del x, pre, pooled, dyp, dx, ws
        torch.cuda.empty_cache()
    core.check_h2_overflow()
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
