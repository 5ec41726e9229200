"""Time ``SparseEncoderHD`` (co_occ_amd/lidar_hd.py, eval mode, seeded weights) at the size of projects/configs/coocc_nusc/coocc_lidar.py:
a synthetic cloud that fills the 120 000-voxel cap on the [65, 800, 800] grid.  There is no upstream number on this hardware (spconv
v1 does not build on ROCm) and no earlier path in this package, so nothing is compared against; ``SparseLiDAREnc8x`` on the same
cloud is recorded as scale only.

    python tools/bench_sparse_hd.py [--calls 20] [--warmup 5] [--windows 3] [--out profiles/sparse_hd_bench.json]

Per configuration (split-f16 engine with the 16-wide stage carried 32 wide, the same on 16-wide fp32-MFMA rows, fp32 engine):
ms per sample of the encoder (HIP events around ``calls`` calls after ``warmup`` calls, ``windows`` windows, median and spread), and
its pieces, each timed on its own in the same way: the GEMM launches up to ``conv_out`` over prebuilt rule books
(``SparseEncoderHD.run_layers``) and the dense write (the volume's clear + ``conv_out``'s scattering GEMM, ``dense_output``).  The rule
books (index maps, flags, compaction, tables; ``rule_books``, with the bytes cleared per sample and its three host reads) and
voxelise + VFE do not depend on the engine and are timed once.  Prints one JSON line."""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--windows", type=int, default=3)
    ap.add_argument("--points", type=int, default=400000)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_sparse_hd needs the MI355X: there is no CPU fallback")
    import co_occ_amd as pkg
    from co_occ_amd import core, lidar, lidar_hd, synth
    dev = torch.device("cuda:0")
    cfg = synth.model_cfg_lidar()
    vl = pkg.Voxelization(**cfg["pts_voxel_layer"]).eval()
    vfe = pkg.HardSimpleVFE(num_features=4)
    m = lidar_hd.SparseEncoderHD(**{k: v for k, v in cfg["pts_middle_encoder"].items() if k != "type"})
    m.load_state_dict(synth.random_state_dict(m.state_dict(), seed=12))
    m = m.to(dev).eval()
    enc8 = lidar.MIDDLE_ENCODERS.build(synth.lidar_cfg()["pts_middle_encoder"])
    enc8.load_state_dict(synth.random_state_dict(enc8.state_dict(), seed=13))
    enc8 = enc8.to(dev).eval()
    pts = synth.lidar_points(a.points, seed=3).to(dev)

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

    with torch.no_grad():
        def producer():
            voxels, coors, num = vl(pts)
            return vfe(voxels, num, coors), coors
        feats, coors = producer()
        coors8 = coors.clone()
        coors8[:, 0].clamp_(max=63)                  # the 8x encoder's grid is [64, 800, 800]

        D, H, W = m.out_shape()
        levels = m.rule_books(coors)
        res = dict(workload="coocc_lidar SparseEncoderHD [65,800,800], %d voxels" % coors.shape[0], calls=a.calls, warmup=a.warmup,
                   windows=a.windows, active_per_level=[lv.M for lv in levels], voxelise_vfe=timed(producer),
                   rule_books=timed(lambda: m.rule_books(coors)), configs={})
        # index maps + flag volumes cleared per sample (the rule books do not depend on the engine)
        res["rule_books"]["bytes_cleared"] = sum(lv.cleared_bytes for lv in m.rule_books(coors))
        res["dense_volume_bytes"] = W * H * D * m.output_channels * 4
        # the first level's index map alone (full memset of 65 x 800 x 800 int32 + the scatter of its voxels)
        from co_occ_amd._lib import call, ptr
        map0 = core.stream_buffer(dev, "hd_map", 65 * 800 * 800, torch.int32)
        res["index_map_level0"] = dict(timed(lambda: call("coocc_sparse_index_map", ptr(coors), coors.shape[0], 65, 800, 800, ptr(map0))),
                                       bytes=4 * 65 * 800 * 800)
        for name, engine, wide in (("h2_wide32", "h2", True), ("h2_fp32_first_stage", "h2", False), ("f32", "f32", False)):
            core.CONV_ENGINE, m.wide16 = engine, wide
            f = m.run_layers(feats, levels)
            # each piece timed on its own over prebuilt inputs: gemms = every layer up to conv_out (one launch each) on prebuilt rule
            # books; dense_write = the dense volume's clear + conv_out's scattering GEMM; sample = the whole forward
            t = dict(sample=timed(lambda: m(feats, coors, 1)), gemms=timed(lambda: m.run_layers(feats, levels)),
                     dense_write=timed(lambda: m.dense_output(f, levels)), bytes_cleared=m.last_cleared_bytes)
            if wide or engine == "f32":
                t["SparseLiDAREnc8x_sample"] = timed(lambda: enc8(feats, coors8, 1))
            res["configs"][name] = t
        core.CONV_ENGINE, m.wide16 = "h2", lidar_hd.WIDE16
    core.check_h2_overflow()
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
