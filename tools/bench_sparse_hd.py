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
voxelise + VFE do not depend on the engine and are timed once.  Prints one JSON line.

    python tools/bench_sparse_hd.py --train [--out profiles/sparse_hd_train_bench.json]

``--train``: one forward + backward of the module under ``train()`` (``train_enabled``) on the same cloud, timed the same way, for
COOCC_HD_TRAIN_H2 1 / 0 (split-f16 against fp32-MFMA rule-book GEMMs) x COOCC_HD_DGRAD_CLASSES 1 / 0 (the strided dgrad per residue
class against one 27-tap launch over the full transposed book); and on their own: the transposed books of the three
down-convolutions from ``coocc_sparse_dgrad_table3`` (with and without the class lists' sort, host read and gathers) against
``lidar._inverse_table`` on the same forward books, and a training-mode BN1d forward per level with the split-f16 twin written by
its apply pass (``coocc_bn_apply_ex``) against the apply pass followed by ``coocc_rows_to_h2``.  ``wgrad``: per distinct layer shape
that qualifies for the split-f16 rule-book weight gradient (pad4(Cin) % 32 == 0, Cout % 32 == 0), ``coocc_conv_wgrad`` (fp32 MFMA)
against ``coocc_conv_wgrad_h2t`` on the same operands and the level's own book, in alternating windows, with the share of the f16
MFMA peak (the three split products of every live book entry over 2.5 PFLOP/s) and of the HBM peak (live entries x row bytes +
dacc + the slabs written and read back, over 8 TB/s) the new kernel reaches; and the step with COOCC_HD_WGRAD_H2=1 beside the same
step with 0 in the same alternating windows (``--out profiles/sparse_hd_wgrad_bench.json``)."""
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
    ap.add_argument("--train", action="store_true", help="time the training step (forward + backward) instead of inference")
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

    def timed_alternating(fns):
        """``timed`` for several functions at once: one window of each in turn, ``windows`` times over."""
        for fn in fns:
            for _ in range(a.warmup):
                fn()
        torch.cuda.synchronize()
        v = [[] for _ in fns]
        for _ in range(a.windows):
            for i, fn in enumerate(fns):
                v[i].append(window(fn))
        v = [sorted(w) for w in v]
        return [dict(median_ms=round(w[len(w) // 2], 4), min_ms=round(w[0], 4), max_ms=round(w[-1], 4)) for w in v]

    if a.train:
        with torch.no_grad():
            voxels, coors, num = vl(pts)
            feats = vfe(voxels, num, coors)
        res = train_bench(a, m, feats, coors, timed, timed_alternating)
        core.check_h2_overflow()
        line = json.dumps(res)
        print(line)
        if a.out:
            with open(a.out, "w") as f:
                f.write(line + "\n")
        return

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


F16_MFMA_PEAK, HBM_PEAK = 2.5e15, 8.0e12          # MI355X: dense f16 MFMA FLOP/s, HBM3E bytes/s (both spec)


def hd_layers(m, levels):
    """(SparseConvV1, its forward book [taps, rows out], rows in) of every convolution of the module, in forward order."""
    from co_occ_amd import lidar_hd
    it = iter(levels)
    cur = next(it)
    out = [(m.conv_input[0], cur.table(m.conv_input[0].kernel), cur.M)]
    for st in m.encoder_layers:
        for mod in st:
            if isinstance(mod, lidar_hd.SparseBasicBlockHD):
                out += [(mod.conv1, cur.table((3, 3, 3)), cur.M), (mod.conv2, cur.table((3, 3, 3)), cur.M)]
            elif mod[0].subm:
                out.append((mod[0], cur.table(mod[0].kernel), cur.M))
            else:
                n_in = cur.M
                cur = next(it)
                out.append((mod[0], cur.down, n_in))
    out.append((m.conv_out[0], cur.table((1, 1, 1)), cur.M))
    return out


def h2t_slices(Mo, Cin, Cout, taps, ws_floats):
    """The row slices coocc_conv_wgrad_h2t cuts (csrc/wgrad_h2t.hip): what its slabs cost in bytes."""
    items = (taps + 1) // 2 * (Cin // 32) * (Cout // 64) if Cout % 64 == 0 else (taps + 2) // 3 * (Cin // 32) * (Cout // 32)
    wgs = (items + 3) // 4
    n = min((512 + wgs - 1) // wgs, (Mo + 255) // 256, ws_floats // (taps * Cin * Cout), 4096)
    mslice = ((Mo + n - 1) // n + 15) // 16 * 16
    return (Mo + mslice - 1) // mslice


def wgrad_bench(m, levels, timed_alternating):
    from co_occ_amd import core, lidar
    from co_occ_amd._lib import call, ptr
    recs, seen = [], {}
    for conv, table, n_in in hd_layers(m, levels):
        taps, Mo = table.shape
        Cp, Cout = lidar._pad4(conv.cin), conv.cout
        key = (Mo, n_in, Cp, Cout, taps)
        if Cp % 32 or Cout % 32 or not Mo:
            continue
        if key in seen:
            seen[key]["layers"] += 1
            continue
        dev = table.device
        x, dacc = torch.randn(n_in, Cp, device=dev), torch.randn(Mo, Cout, device=dev)
        one = torch.ones(2, device=dev)
        dw_a, dw_b = torch.empty(Cout, Cp, taps, device=dev), torch.empty(Cout, Cp, taps, device=dev)
        ws = core.workspace(dev)

        def f32():
            call("coocc_conv_wgrad", ptr(x), n_in, Cp, ptr(dacc), Cout, ptr(table), Mo, Cp, Cout, taps, ptr(dw_a), 0, ptr(ws), ws.numel())

        def h2t():
            call("coocc_conv_wgrad_h2t", ptr(x), n_in, Cp, ptr(dacc), Cout, ptr(table), Mo, Cp, Cout, taps, ptr(one), ptr(dw_b), 0, ptr(ws),
                 ws.numel())
        t32, th = timed_alternating([f32, h2t])
        live = int((table >= 0).sum())
        nsl = h2t_slices(Mo, Cp, Cout, taps, ws.numel())
        nbytes = live * Cp * 4 + Mo * Cout * 4 + 2 * nsl * taps * Cp * Cout * 4
        sec = th["median_ms"] * 1e-3
        rec = dict(rows_out=Mo, rows_in=n_in, Cin=Cp, Cout=Cout, taps=taps, layers=1, live_share=round(live / (taps * Mo), 4),
                   coocc_conv_wgrad=t32, coocc_conv_wgrad_h2t=th, speedup=round(t32["median_ms"] / th["median_ms"], 3),
                   slices=nsl, f16_mfma_peak_fraction=round(3 * 2.0 * live * Cp * Cout / sec / F16_MFMA_PEAK, 5),
                   hbm_peak_fraction=round(nbytes / sec / HBM_PEAK, 4), bytes=nbytes,
                   max_diff_rel=float((dw_a - dw_b).abs().max() / dw_a.abs().max().clamp_min(1e-30)))
        seen[key] = rec
        recs.append(rec)
    return recs


def train_bench(a, m, feats, coors, timed, timed_alternating):
    from co_occ_amd import autograd as ag, core, lidar, lidar_hd
    from co_occ_amd._lib import call, ptr
    dev = feats.device
    m.train()
    m.train_enabled = True
    gout = torch.randn(1, m.output_channels, *m.out_shape(), device=dev)

    def step():
        m.zero_grad(set_to_none=True)
        (m(feats, coors, 1) * gout).sum().backward()

    def forward_only():
        with torch.no_grad():
            m(feats, coors, 1)
    levels = m.rule_books(coors, transposed=True)
    res = dict(workload="coocc_lidar SparseEncoderHD [65,800,800] under train(), %d voxels" % coors.shape[0], calls=a.calls, warmup=a.warmup,
               windows=a.windows, active_per_level=[lv.M for lv in levels], step={}, transposed_books=[], bn_forward=[])
    old = core.CONV_ENGINE, lidar_hd.HD_TRAIN_H2, lidar_hd.HD_DGRAD_CLASSES, lidar_hd.HD_WGRAD_H2
    core.CONV_ENGINE, lidar_hd.HD_WGRAD_H2 = "h2", False
    for h2 in (1, 0):
        for classes in (1, 0):
            lidar_hd.HD_TRAIN_H2, lidar_hd.HD_DGRAD_CLASSES = bool(h2), bool(classes)
            res["step"]["train_h2=%d dgrad_classes=%d" % (h2, classes)] = dict(forward_backward=timed(step), forward=timed(forward_only))
    # the split-f16 rule-book weight gradient: the step with the knob on and off in the same alternating windows
    lidar_hd.HD_TRAIN_H2, lidar_hd.HD_DGRAD_CLASSES = True, False

    def step_knob(on):
        def fn():
            lidar_hd.HD_WGRAD_H2 = on
            step()
        return fn
    t_on, t_off = timed_alternating([step_knob(True), step_knob(False)])
    res["step"]["train_h2=1 dgrad_classes=0 wgrad_h2=1"] = dict(forward_backward=t_on, forward_backward_wgrad_h2_0_same_windows=t_off)
    core.CONV_ENGINE, lidar_hd.HD_TRAIN_H2, lidar_hd.HD_DGRAD_CLASSES, lidar_hd.HD_WGRAD_H2 = old
    res["wgrad"] = wgrad_bench(m, levels, timed_alternating)
    # the transposed book of every down-convolution: the device kernel from geometry (alone, and with the class lists) against the
    # boolean-mask construction of lidar._inverse_table on the same forward book
    downs = [mod[0] for st in m.encoder_layers for mod in st if isinstance(mod, lidar_hd._ConvModule) and not mod[0].subm]
    for conv, lo, hi in zip(downs, levels[:-1], levels[1:]):
        k, s, p = conv.kernel, conv.stride, conv.padding
        got = lidar_hd.dgrad_books(lo, hi, k, s, p, by_class=False)[0]
        assert torch.equal(got, lidar._inverse_table(hi.down, lo.M)), "the two constructions disagree"
        res["transposed_books"].append(dict(
            rows_in=lo.M, rows_out=hi.M, stride=list(s), padding=list(p),
            dgrad_table3=timed(lambda: lidar_hd.dgrad_books(lo, hi, k, s, p, by_class=False)),
            dgrad_table3_with_class_lists=timed(lambda: lidar_hd.dgrad_books(lo, hi, k, s, p, by_class=True)),
            inverse_table_torch=timed(lambda: lidar._inverse_table(hi.down, lo.M))))
    # a training-mode BN1d forward (statistics + apply) per level at that level's width
    for lv, C in zip(levels, [m.base_channels] + [conv.cout for conv in downs]):
        if C % 32 or not lv.M:
            continue
        x = torch.randn(lv.M, C, device=dev)
        bn = torch.nn.BatchNorm1d(C, eps=1e-3, momentum=0.01).to(dev).train()
        twin = torch.empty_like(x)

        def fused():
            with torch.no_grad():
                ag.BatchNormRowsFn.apply(x, bn.weight, bn.bias, None, bn, True, None, twin)

        def separate():
            with torch.no_grad():
                y = ag.BatchNormRowsFn.apply(x, bn.weight, bn.bias, None, bn, True, None)
                call("coocc_rows_to_h2", ptr(y), C, lv.M, C, 1.0, ptr(twin))
        res["bn_forward"].append(dict(rows=lv.M, C=C, fused_twin=timed(fused), apply_then_rows_to_h2=timed(separate)))
    return res


if __name__ == "__main__":
    main()
