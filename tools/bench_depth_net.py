"""Time ``depth_net.DepthNet(512, 512, 128, 112)`` (eval mode, seeded weights) at the two sizes of the coocc_nusc configs: the r50
map (6 cameras x 16 x 44) and the r101 map (6 x 56 x 100).  Nothing on this hardware ran the module before (the reference's class
needs mmcv's DCN), so nothing is compared against; the file is the record.

    python tools/bench_depth_net.py [--calls 20] [--warmup 5] [--windows 3] [--out profiles/depth_net_bench.json]

Per size: ms per forward issued eagerly and as one captured-graph replay (HIP events around ``calls`` forwards after ``warmup``,
``windows`` windows, median and spread, as tools/bench_sparse_hd.py), and the per-kernel table: every launch of one forward timed by
its own HIP-event pair (``core.TIMER`` level 2), per kernel the median over ``windows`` passes of its summed time, its launches and
its share of the summed kernel time.  The event pairs perturb the stream, so the kernel times are a breakdown, not a second
measurement of the total.  The Winograd transforms appear under their region names (k_wino_in / k_wino_out); the entry points they
wrap are left out of the table so nothing is counted twice.  Prints one JSON line.

    python tools/bench_depth_net.py --train [--out profiles/depth_net_train_bench.json]

``--train``: the same module with ``train_enabled`` under ``train()`` (batch statistics, dropout p = 0.5), one step = forward +
backward of sum(out * r) with respect to every parameter and x, issued eagerly (capturing the step in a graph is not built), same
protocol.  The record also names the shares of the sampler's backward (k_dcn_cols_bwd) and of the dilated branches' dgrad / wgrad.
No earlier training number exists, so nothing is compared."""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SIZES = {"r50_6x16x44": (6, 16, 44), "r101_6x56x100": (6, 56, 100)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--windows", type=int, default=3)
    ap.add_argument("--train", action="store_true", help="time forward + backward under train() (train_enabled)")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if a.out is None:
        a.out = os.path.join(ROOT, "profiles", "depth_net_train_bench.json" if a.train else "depth_net_bench.json")
    if not torch.cuda.is_available():
        raise SystemExit("bench_depth_net needs the MI355X: there is no CPU fallback")
    from co_occ_amd import core, depth_net, synth
    dev = torch.device("cuda:0")
    net = depth_net.DepthNet(512, 512, 128, 112)
    net.load_state_dict(synth.random_state_dict(net.state_dict(), seed=12))
    net = net.to(dev).eval()

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
        # entry points that run inside a named region (the Winograd transforms; in training the weight gradients and the sampler's
        # backward) are left out: their region is the row
        inner = ("coocc_wino_input", "coocc_wino_output")
        if a.train:
            inner += ("coocc_conv_wgrad", "coocc_wino_wgrad", "coocc_dcn_cols_bwd")
        tags = [t for t in passes[0] if not t.startswith(inner)]
        rows = {}
        for t in tags:
            ms = sorted(p[t]["ms"] for p in passes if t in p)
            rows[t] = dict(launches=passes[0][t]["launches"], ms=round(ms[len(ms) // 2], 4))
        total = sum(r["ms"] for r in rows.values())
        for r in rows.values():
            r["share"] = round(r["ms"] / total, 4)
        return dict(sum_ms=round(total, 4), kernels=dict(sorted(rows.items(), key=lambda kv: -kv[1]["ms"])))

    if a.train:
        return train(a, net, dev, timed, kernel_table)
    res = dict(workload="DepthNet(512, 512, 128, 112), eval, seeded weights", engine=core.CONV_ENGINE, calls=a.calls, warmup=a.warmup,
               windows=a.windows, dcn_chunk_rows=depth_net.DCN_CHUNK_ROWS, sizes={})
    with torch.no_grad():
        for name, (BN, H, W) in SIZES.items():
            g = torch.Generator().manual_seed(H)
            x = torch.randn(BN, 512, H, W, generator=g).to(dev)
            mlp = torch.randn(1, BN, 27, generator=g).to(dev)
            fn = lambda: net(x, mlp)
            rec = dict(rows=BN * H * W, eager=timed(fn))
            s = torch.cuda.Stream(device=dev)
            s.wait_stream(torch.cuda.current_stream(dev))
            with torch.cuda.stream(s):
                fn()
                torch.cuda.synchronize()
                graph = torch.cuda.CUDAGraph()
                with torch.cuda.graph(graph, stream=s):
                    out = fn()
            torch.cuda.current_stream(dev).wait_stream(s)
            keep = core.stream_scratch(dev, s)
            rec["graph_replay"] = timed(graph.replay)
            rec["graph_equals_eager"] = bool(torch.equal(out, fn()))
            rec["finite"] = bool(torch.isfinite(out).all())
            del graph, keep
            rec["kernel_table"] = kernel_table(fn)
            res["sizes"][name] = rec
    finish(a, res)


def finish(a, res):
    from co_occ_amd import core
    core.check_h2_overflow()
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


def train(a, net, dev, timed, kernel_table):
    from co_occ_amd import core, depth_net
    net.train_enabled = True
    net.train()
    params = [p for p in net.parameters()]
    res = dict(workload="DepthNet(512, 512, 128, 112), train() with train_enabled, dropout p = 0.5, seeded weights: forward + backward",
               engine=core.CONV_ENGINE, calls=a.calls, warmup=a.warmup, windows=a.windows, dcn_chunk_rows=depth_net.DCN_CHUNK_ROWS,
               sizes={})
    for name, (BN, H, W) in SIZES.items():
        g = torch.Generator().manual_seed(H)
        x = torch.randn(BN, 512, H, W, generator=g).to(dev).requires_grad_(True)
        mlp = torch.randn(1, BN, 27, generator=g).to(dev)
        r = torch.randn(BN, 112 + 128, H, W, generator=g).to(dev)

        def step():
            for p in params:
                p.grad = None
            x.grad = None
            out = net(x, mlp)
            out.backward(r)
            return out

        def forward():
            with torch.no_grad():
                return net(x, mlp)
        rec = dict(rows=BN * H * W, step=timed(step), forward_only=timed(forward))
        out = step()
        rec["finite"] = bool(torch.isfinite(out).all() and torch.isfinite(x.grad).all() and all(torch.isfinite(p.grad).all() for p in params))
        kt = kernel_table(step)
        rec["kernel_table"] = kt
        k = kt["kernels"]
        share = lambda pred: round(sum(v["share"] for t, v in k.items() if pred(t)), 4)
        rec["shares"] = dict(k_dcn_cols_bwd=share(lambda t: t == "k_dcn_cols_bwd"),
                             dcn_gemms=share(lambda t: t.endswith(("dcn_fwd", "dcn_dgrad")) or t == "k_wgrad<dcn>"),
                             dilated_dgrad=share(lambda t: t.endswith("sparse_hd_dgrad")),
                             dilated_wgrad=share(lambda t: "<sparse hd table>" in t))
        res["sizes"][name] = rec
        del x, r, out
        torch.cuda.empty_cache()
    finish(a, res)


if __name__ == "__main__":
    main()
