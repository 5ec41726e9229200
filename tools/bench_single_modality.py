"""What the captured dense stage buys the two models without a fuser -- the camera-only ``COOCC_Ray`` (``occ_fuser=None``) and the
LiDAR-only ``COOCC_Ray_L`` -- and what the one-launch voxel-only fine branch (csrc/fine_vox.hip) costs next to the launches it replaces.

Three models, each alternating eager and captured windows within one process:
  camera       grid 100 x 100 x 8, 6 cameras, 56 x 100 maps, D 112, render off (coocc_cam_r101_896x1600.py)
  lidar        100 x 100 x 8, coarse only (coocc_lidar.py as configured)
  lidar_fine   the same with ``sample_from_voxel=True``: the voxel cascade (the foreground share is what the seeded weights give; reported)
Per model, in ms per sample, medians over --windows synchronised windows with min / max:
  eager_ms      ``simple_test`` with ``graph_simple_test=False``: the launches as they always were (the baseline)
  captured_ms   ``simple_test`` with the captured dense stage
  host_ms       host time to issue one sample on the captured route (``submit`` + ``result(wait=False)``: copy-in, slot fill, one
                graph launch), the device synchronised outside the window
  pipelined     ``apis.pipelined_test`` over windows of 16 samples: ms per sample and samples / s
``coocc_fine_vox`` at 100 x 100 x 8, 15 % foreground, ncls 17, device-event time per window: the kernel alone, the kernel with its Q GEMM,
and the eager voxel-only fine branch at the same foreground list (sample 128 channels, Linear, GroupNorm, Linear); achieved bytes / s
of the kernel over V 256 B + 8 n (4 ncls + 24) B as a share of the 8 TB/s HBM peak.
A run without a GPU is refused.  Writes profiles/single_modality_serving.json (--out).

    python tools/bench_single_modality.py [--windows 30] [--warmup 3] [--out profiles/single_modality_serving.json]
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch

HBM_PEAK = 8.0e12
FMAP, NCAM, GRID = (56, 100), 6, (100, 100, 8)
PIPE_WINDOW = 16


def spread(v):
    v = sorted(float(x) for x in v)
    return dict(median=round(statistics.median(v), 4), min=round(v[0], 4), max=round(v[-1], 4), n=len(v))


def require_gpu():
    if not torch.cuda.is_available():
        raise SystemExit("bench_single_modality: no GPU -- the serving loop and its kernels run on the GPU only and a CPU timing says "
                         "nothing about them")


def _build(cfg, dev, seed):
    import co_occ_amd as pkg
    from co_occ_amd import synth
    model = pkg.build_detector(cfg)
    model.load_state_dict(synth.random_state_dict(model.state_dict(), seed=seed))
    return model.to(dev).eval()


def build(which, dev):
    """(model, [precomputed dict, ...]) of one of the three models."""
    from co_occ_amd import synth
    X, Y, Z = GRID
    if which == "camera":
        cfg = synth.model_cfg(C=128, final_occ_size=(2 * X, 2 * Y, 2 * Z), input_size=(FMAP[0] * 16, FMAP[1] * 16), rendering=False)
        cfg.update(occ_fuser=None, external_encoders=True)
        model = _build(cfg, dev, 0)
        pcs = []
        for seed in (4000, 4013):
            rig = synth.camera_rig(NCAM, (FMAP[0] * 16, FMAP[1] * 16), seed=1234)
            cams = tuple(rig[k].to(dev) for k in ("rots", "trans", "intrins", "post_rots", "post_trans", "bda"))
            depth, ctx = synth.lift_inputs(NCAM, model.img_view_transformer.D, FMAP, 128, seed=seed)
            pcs.append(dict(depth=depth.to(dev), ctx=ctx.to(dev), cams=cams, img_feats=[synth.image_feats(NCAM, FMAP, 512, seed=seed).to(dev)],
                            transform=tuple(t.to(dev) if torch.is_tensor(t) else t for t in synth.rig_transform(rig))))
        return model, pcs
    cfg = synth.model_cfg_lidar()
    cfg.update(external_encoders=True)
    cfg["pts_bbox_head"].update(sample_from_voxel=which == "lidar_fine")
    model = _build(cfg, dev, 0)
    return model, [dict(pts_voxel_feats=synth.voxel_inputs(GRID, C=128, seed=s)[1].to(dev)) for s in (50, 51)]


def wall(fn):
    """ms from a synchronised start until the device has finished what ``fn`` issued."""
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3


def host_issue(pipe, fr):
    """ms the host needs to issue one sample on the captured route; the device is synchronised outside the window."""
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    pipe.submit(fr).result(wait=False)
    ms = (time.perf_counter() - t0) * 1e3
    torch.cuda.synchronize()
    return ms


def bench_model(which, dev, windows, warmup):
    from co_occ_amd import apis, core
    model, pcs = build(which, dev)
    call = lambda i: model.simple_test(precomputed=pcs[i % len(pcs)])
    eager, captured, host = [], [], []
    with torch.no_grad():
        for flag in (False, True):
            model.graph_simple_test = flag
            for i in range(max(1, warmup)):
                call(i)
        torch.cuda.synchronize()
        core.check_h2_overflow()
        assert model._pipe1 is not None and model.graph_unavailable is None, model.graph_unavailable
        out = call(0)
        fine = out.get("output_voxels_fine")
        fg = None if fine is None else fine[0].shape[0] / 8.0 / (GRID[0] * GRID[1] * GRID[2])
        pipe = model._pipe1[1]
        fr = model.serving_frame(precomputed=pcs[0])
        for i in range(windows):                              # eager and captured alternate, one window each
            model.graph_simple_test = False
            eager.append(wall(lambda: call(i)))
            model.graph_simple_test = True
            captured.append(wall(lambda: call(i)))
            host.append(host_issue(pipe, fr))
        # the pipelined loop: time stamps at every yield, windows of PIPE_WINDOW samples behind a first window that pays the capture
        n = PIPE_WINDOW * (windows + 1)
        stamps, stats = [], {}
        for _ in apis.pipelined_test(model, (dict(precomputed=pcs[i % len(pcs)]) for i in range(n)), stats=stats):
            stamps.append(time.perf_counter())
        torch.cuda.synchronize()
    per = [(stamps[k + PIPE_WINDOW] - stamps[k]) * 1e3 / PIPE_WINDOW for k in range(PIPE_WINDOW - 1, n - PIPE_WINDOW, PIPE_WINDOW)]
    res = dict(eager_ms=spread(eager), captured_ms=spread(captured), host_ms=spread(host), pipelined_ms_per_sample=spread(per),
               pipelined_samples_per_s=round(1e3 / statistics.median(per), 2), pipelined_stats=stats,
               foreground_share=None if fg is None else round(fg, 4))
    e, c = res["eager_ms"], res["captured_ms"]
    res["captured_beats_eager_by_more_than_eagers_spread"] = bool(e["median"] - c["median"] > e["max"] - e["min"])
    return res


def event_ms(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1)


def bench_kernel(dev, windows, warmup, share=0.15, ncls=17):
    from co_occ_amd import core
    from co_occ_amd._lib import call, host_i32, ptr
    model, _ = build("lidar_fine", dev)
    head = model.pts_bbox_head
    X, Y, Z = GRID
    V = X * Y * Z
    g = torch.Generator().manual_seed(3)
    rows = core.Rows(torch.randn(V, 128, generator=g).to(dev), 1, X, Y, Z, 128)
    n = int(V * share)
    lin = torch.sort(torch.randperm(V, generator=g)[:n])[0].int().to(dev)
    cnt = torch.tensor([n], dtype=torch.int32, device=dev)
    p = head._packed()
    final = host_i32([2 * X, 2 * Y, 2 * Z])
    xyz, logits = torch.empty(3 * 8 * n, device=dev, dtype=torch.int64), torch.empty(8 * n, ncls, device=dev)
    q = core.linear_rows(rows.t, p["f0_nb"], in_C=128)
    gn = head.fine_mlp[1]

    def kernel():
        head._fine_vox(rows, q, lin, n, cnt, xyz, logits)

    def with_q():
        head._fine_vox(rows, core.linear_rows(rows.t, p["f0_nb"], in_C=128), lin, n, cnt, xyz, logits)

    def eager():                                              # occ_head.py's order, as OccHead._fine runs it for this head
        feat = torch.empty(8 * n, 128, device=dev)
        call("coocc_fine_sample_voxel", ptr(rows.t), 128, X, Y, Z, ptr(lin), n, 2, final, ptr(xyz), ptr(feat), 128)
        h = core.linear_rows(feat, p["fine0"])
        call("coocc_groupnorm_rows", ptr(h), 8 * n, 64, 64, gn.num_groups, ptr(gn.weight.detach()), ptr(gn.bias.detach()), float(gn.eps), 1)
        return core.linear_rows(h, p["fine3"])
    t = dict(kernel=[], with_q=[], eager=[])
    with torch.no_grad():
        for _ in range(max(1, warmup)):
            kernel(), with_q(), eager()
        for _ in range(windows):
            t["eager"].append(event_ms(eager))
            t["with_q"].append(event_ms(with_q))
            t["kernel"].append(event_ms(kernel))
    core.check_h2_overflow()
    nbytes = V * 256 + 8 * n * (4 * ncls + 24)
    res = dict(grid=list(GRID), foreground=n, ncls=ncls, fine_vox_ms=spread(t["kernel"]), fine_vox_with_q_gemm_ms=spread(t["with_q"]),
               eager_fine_branch_ms=spread(t["eager"]), bytes=nbytes)
    bps = nbytes / (res["fine_vox_ms"]["median"] * 1e-3)
    res.update(bytes_per_s=round(bps, 1), share_of_hbm_peak=round(bps / HBM_PEAK, 4))
    e, k = res["eager_fine_branch_ms"], res["fine_vox_with_q_gemm_ms"]
    res["no_slower_than_eager_by_eagers_spread"] = bool(k["median"] <= e["median"] + (e["max"] - e["min"]))
    return res


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--windows", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--models", default="camera,lidar,lidar_fine")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "single_modality_serving.json"))
    a = ap.parse_args(argv)
    require_gpu()
    dev = torch.device("cuda:0")
    result = dict(device=torch.cuda.get_device_name(0), torch=torch.__version__, windows=a.windows, warmup=a.warmup, grid=list(GRID),
                  cameras=NCAM, fmap=list(FMAP), pipelined_window=PIPE_WINDOW, models={})
    for which in [m for m in a.models.split(",") if m]:
        result["models"][which] = bench_model(which, dev, a.windows, a.warmup)
        torch.cuda.empty_cache()
    result["coocc_fine_vox"] = bench_kernel(dev, a.windows, a.warmup)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    print(json.dumps(result))
    return result


if __name__ == "__main__":
    main()
