"""Time the image encoder (``image_encoder.ResNet`` + ``image_encoder.SECONDFPN``, eval mode, seeded weights) at the two sizes of the
coocc_nusc configs -- 6 cameras x 256 x 704 with ResNet-50, 6 x 896 x 1600 with ResNet-101 -- and, in the same process on the same
GPU, the same network as plain torch modules in eager fp32 (tests/ref_image_encoder.py ``TorchResNet`` / ``TorchSECONDFPN`` with the
same weights, ``torch.backends.cudnn.allow_tf32 = False``): what a user would otherwise inject as a module.

    python tools/bench_image_encoder.py [--calls 10] [--warmup 3] [--windows 3] [--out profiles/image_encoder_bench.json]

Per size: ms of backbone + neck (Rows end to end), of the backbone, the neck and the stem kernel alone (HIP events around ``calls``
forwards after ``warmup``, ``windows`` windows, median and spread, as tools/bench_depth_net.py), the torch run's ms and the ratio
HIP / torch, the stem's flops and bytes against the fp32 and HBM peaks, and the per-kernel table of one forward (``core.TIMER``
level 2: per kernel the launches, the median summed time and its share; the event pairs perturb the stream, so it is a breakdown,
not a second measurement of the total).  Prints one JSON line."""
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
    ap.add_argument("--calls", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--windows", type=int, default=3)
    ap.add_argument("--sizes", default=",".join(SIZES))
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "image_encoder_bench.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_image_encoder needs the MI355X: there is no CPU fallback")
    import ref_image_encoder as R
    from co_occ_amd import core, image_encoder as IE
    dev = torch.device("cuda:0")
    torch.backends.cudnn.allow_tf32 = False
    torch.backends.cuda.matmul.allow_tf32 = False

    def window(fn):
        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        s.record()
        for _ in range(a.calls):
            fn()
        e.record()
        torch.cuda.synchronize()
        return s.elapsed_time(e) / a.calls

    def timed(fn):
        for _ in range(a.warmup):
            fn()
        torch.cuda.synchronize()
        v = sorted(window(fn) for _ in range(a.windows))
        return dict(median_ms=round(v[len(v) // 2], 4), min_ms=round(v[0], 4), max_ms=round(v[-1], 4))

    def kernel_table(fn):
        passes = []
        for _ in range(a.windows):
            core.TIMER.enabled, core.TIMER.only = 2, None
            core.TIMER.reset()
            fn()
            torch.cuda.synchronize()
            passes.append(core.TIMER.summary())
            core.TIMER.enabled = False
            core.TIMER.reset()
        inner = ("coocc_wino_input", "coocc_wino_output", "coocc_img_stem", "coocc_fpn_sum")      # run inside a named region
        rows = {}
        for t in [t for t in passes[0] if not t.startswith(inner)]:
            ms = sorted(p[t]["ms"] for p in passes if t in p)
            rows[t] = dict(launches=passes[0][t]["launches"], ms=round(ms[len(ms) // 2], 4))
        total = sum(r["ms"] for r in rows.values())
        for r in rows.values():
            r["share"] = round(r["ms"] / total, 4)
        return dict(sum_ms=round(total, 4), launches=sum(r["launches"] for r in rows.values()),
                    kernels=dict(sorted(rows.items(), key=lambda kv: -kv[1]["ms"])))

    res = dict(workload="image_encoder.ResNet + SECONDFPN, eval, seeded weights, 6 cameras", engine=core.CONV_ENGINE, calls=a.calls,
               warmup=a.warmup, windows=a.windows, torch_version=torch.__version__, sizes={})
    with torch.no_grad():
        for name in a.sizes.split(","):
            depth, BN, H, W = SIZES[name]
            bb, nk = IE.ResNet(depth=depth), IE.SECONDFPN(**NECK)
            sdb = R.fixture_state_dict(bb.state_dict(), depth)
            sdn = R.fixture_state_dict(nk.state_dict(), depth + 1, R.transposed_keys(NECK["upsample_strides"]))
            bb.load_state_dict(sdb)
            nk.load_state_dict(sdn)
            bb, nk = bb.to(dev).eval(), nk.to(dev).eval()
            x = R.fixture_images(BN, H, W, depth + 2).to(dev)
            readers = nk.reader_packs()
            stem = bb._packed()["stem"]
            first = bb._readers_of(bb._packed()["layers"][0][0])
            feats = bb.forward_rows(x, readers=readers)
            out = nk.forward_rows(feats)
            torch.cuda.synchronize()
            core.check_h2_overflow()
            rec = dict(depth=depth, image=[BN, 3, H, W], out=[out.B, out.C, out.X, out.Y],
                       encoder=timed(lambda: IE.run_image_encoder(bb, nk, x)),
                       backbone=timed(lambda: bb.forward_rows(x, readers=readers)),
                       neck=timed(lambda: nk.forward_rows(feats)),
                       stem=timed(lambda: IE.stem_rows(x, stem, twin_for=first)))
            Hc, Wc = (H - 1) // 2 + 1, (W - 1) // 2 + 1
            Hp, Wp = (Hc - 1) // 2 + 1, (Wc - 1) // 2 + 1
            flops = 2.0 * BN * Hc * Wc * 64 * 147
            nbytes = 4.0 * BN * 3 * H * W + 4.0 * BN * Hp * Wp * 64 * (2 if core.wants_h2_twin(IE.stem_rows(x, stem), first) else 1)
            ms = rec["stem"]["median_ms"]
            rec["stem_roofline"] = dict(flops=flops, bytes=nbytes, tflops=round(flops / ms / 1e9, 2),
                                        of_fp32_peak=round(flops / ms / 1e9 / FP32_PEAK_TFLOPS, 4), gbs=round(nbytes / ms / 1e6, 1),
                                        of_hbm_peak=round(nbytes / ms / 1e6 / HBM_PEAK_GBS, 4),
                                        unfused_conv_map_bytes=4.0 * BN * Hc * Wc * 64)
            rec["kernel_table"] = kernel_table(lambda: IE.run_image_encoder(bb, nk, x))
            # the same network as plain torch modules, eager fp32, same process
            tb, tn = R.TorchResNet(depth), R.TorchSECONDFPN(NECK["in_channels"], NECK["out_channels"], NECK["upsample_strides"])
            tb.load_state_dict(sdb)
            tn.load_state_dict(sdn)
            tb, tn = tb.to(dev).eval(), tn.to(dev).eval()
            want = tn(tb(x))[0]
            got = IE.rows_as_bchw(out)
            rec["max_rel_diff_vs_torch"] = float((got - want).abs().max() / want.abs().max())
            rec["torch_eager_fp32"] = timed(lambda: tn(tb(x)))
            rec["torch_backbone"] = timed(lambda: tb(x))
            rec["ratio_hip_over_torch"] = round(rec["encoder"]["median_ms"] / rec["torch_eager_fp32"]["median_ms"], 4)
            res["sizes"][name] = rec
            print(name, json.dumps({k: rec[k] for k in ("encoder", "backbone", "neck", "stem", "torch_eager_fp32", "ratio_hip_over_torch")}),
                  file=sys.stderr, flush=True)
            del bb, nk, tb, tn, feats, out, want, got, x
            torch.cuda.empty_cache()
    core.check_h2_overflow()
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
