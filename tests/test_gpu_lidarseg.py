"""LiDAR-segmentation point predictions (``points_occ``) on the MI355X: ``coocc_lidarseg_points`` against the unmodified reference
(tests/golden/lidarseg.npz, tools/gen_golden_lidarseg.py) and against torch on a full configs[1] scene, and the reference entry
points that carry it -- ``OccHead.forward_lidarseg``, ``COOCC_Ray.simple_test`` (captured and eager), ``apis.pipelined_test``,
``COOCC_Ray.forward_train`` -- plus the co-runner guard of the new kernel."""
import os
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from util import assert_close

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from co_occ_amd import evaluation as E  # noqa: E402

pytestmark = pytest.mark.gpu
_M = {}


def golden_probs(g, case):
    """The fixture's probabilities of case (a), or of case (b): (a)'s with the rows zeros padding changes replaced."""
    if case == "a":
        return g["a_probs"]
    b = g["a_probs"].copy()
    b[g["b_probs_rows"]] = g["b_probs_at_rows"]
    return b


def _head(padding_mode="border", pc_range=None):
    from co_occ_amd.head import OccHead
    kw = dict(point_cloud_range=list(pc_range)) if pc_range is not None else {}
    return OccHead(in_channels=[64], out_channel=17, norm_cfg=dict(type='BN3d'), padding_mode=padding_mode, **kw)


def _model(dev):
    if not _M:
        import bench
        bench.CFGNAME[0] = "r50"
        model, _ = bench.build_model("r50", dev)
        model.test_rendering = True
        _M.update(bench=bench, model=model, samples=[bench.make_inputs("r50", 4000 + 13 * i, dev, model) for i in range(8)])
        g = torch.Generator().manual_seed(5)
        _M["gts"] = [torch.randint(0, 17, (1, 200, 200, 16), generator=g).to(dev) for _ in range(8)]
    return _M["bench"], _M["model"], _M["samples"], _M["gts"]


def _points(n, seed, dev):
    """synth.lidar_points with column 3 (intensity there) replaced by labels in {0..16, 255}."""
    from co_occ_amd import synth
    p = synth.lidar_points(n, seed)
    g = torch.Generator().manual_seed(seed + 1)
    lab = torch.randint(0, 18, (n,), generator=g).float()
    lab[lab == 17] = 255.0
    p[:, 3] = lab
    return p.to(dev)


# ------------------------------------------------------------------ kernel vs the unmodified reference
@pytest.mark.parametrize("case,padding", [("a", "border"), ("b", "zeros")])
def test_kernel_equals_reference_eval(dev, golden, case, padding):
    g = golden("lidarseg")
    logits = torch.from_numpy(g["a_logits"]).to(dev)
    pts = torch.from_numpy(g["a_points"]).to(dev)
    n = pts.shape[0]
    probs = torch.empty(n, 17, device=dev)
    labels = torch.empty(n, dtype=torch.int64, device=dev)
    hist = torch.empty(256, dtype=torch.int64, device=dev)
    E.lidarseg_points(logits, pts, g["pc_range"], padding, probs=probs, labels=labels, hist=hist)
    assert torch.equal(labels.cpu(), torch.from_numpy(g[case + "_labels"]))
    assert np.array_equal(hist.view(16, 16).cpu().numpy(), g[case + "_hist"])
    assert_close(probs.cpu(), golden_probs(g, case), tol=1e-5, what="lidarseg probs (%s)" % case)
    # the head: the range from img_metas, and the same from its own point_cloud_range when the metas lack it
    head = _head(padding, pc_range=g["pc_range"]).to(dev).eval()
    p1 = head.forward_lidarseg(logits, [pts], [dict(pc_range=g["pc_range"].tolist())])
    p2 = head.forward_lidarseg(logits, [pts], None)
    assert torch.equal(p1, probs) and torch.equal(p2, probs)


def test_kernel_equals_reference_train_batch_of_two(dev, golden):
    g = golden("lidarseg")
    logits = torch.from_numpy(g["c_logits"]).to(dev)
    pts = [torch.from_numpy(g["c_points0"]).to(dev), torch.from_numpy(g["c_points1"]).to(dev)]
    head = _head().to(dev).train()
    res = head.forward_lidarseg(logits, pts, [dict(pc_range=g["pc_range"].tolist())])
    assert set(res) == {"point_mean_iou"}
    v = res["point_mean_iou"]
    assert v.is_cuda and v.dtype == torch.float64 and v.dim() == 0
    assert abs(float(v) - float(g["c_point_mean_iou"])) <= 1e-12
    n0, n1 = pts[0].shape[0], pts[1].shape[0]
    labels = torch.empty(n0 + n1, dtype=torch.int64, device=dev)
    hist = torch.empty(256, dtype=torch.int64, device=dev)
    E.lidarseg_points(logits[0], pts[0], g["pc_range"], train=True, labels=labels[:n0], hist=hist)
    E.lidarseg_points(logits[1], pts[1], g["pc_range"], train=True, labels=labels[n0:], hist=hist, accumulate=True)
    assert torch.equal(labels.cpu(), torch.from_numpy(g["c_labels"]))
    assert np.array_equal(hist.view(16, 16).cpu().numpy(), g["c_hist"])


# ------------------------------------------------------------------ kernel vs torch on a full scene
def _torch_probs(pred, pts, rng, dtype):
    lg = pred.detach().to("cpu", dtype).contiguous()
    r = torch.tensor(rng, dtype=torch.float32).to(dtype)
    q = ((pts[:, :3].cpu().to(dtype) - r[:3]) / (r[3:] - r[:3])) * 2 - 1
    s = F.grid_sample(lg, q[:, [2, 1, 0]].view(1, 1, 1, -1, 3), mode='bilinear', padding_mode='border', align_corners=True)
    return torch.softmax(s.squeeze().t(), dim=1)


def test_kernel_equals_torch_on_a_full_scene_both_layouts(dev):
    bench, model, samples, _ = _model(dev)
    head = model.pts_bbox_head
    with torch.no_grad():
        model.graph_simple_test = False
        pred = model.simple_test(**bench.simple_test_kwargs(samples[0]))["pred_c"]
    rng = head.lidarseg_range(None)
    pts = _points(35000, 17, dev)
    n = pts.shape[0]
    want32 = _torch_probs(pred, pts, rng, torch.float32)
    want64 = _torch_probs(pred, pts, rng, torch.float64)
    top = torch.topk(want32[:, 1:], 2, dim=1).values
    clear = (top[:, 0] - top[:, 1]) > 1e-5
    want_labels = torch.argmax(want32[:, 1:], dim=1) + 1
    print("\nlidarseg vs torch: %d of %d points have a top-2 probability margin <= 1e-5" % (int((~clear).sum()), n))
    assert int((~clear).sum()) <= 0.001 * n
    results = []
    for layout, lg in (("rows", pred), ("ncdhw", pred.contiguous())):
        probs = torch.empty(n, 17, device=dev)
        labels = torch.empty(n, dtype=torch.int64, device=dev)
        hist = torch.empty(256, dtype=torch.int64, device=dev)
        E.lidarseg_points(lg, pts, rng, "border", probs=probs, labels=labels, hist=hist)
        e32 = assert_close(probs.cpu(), want32, tol=1e-5, what="probs vs torch fp32 (%s)" % layout)
        e64 = float((probs.cpu().double() - want64).abs().max())
        print("%s: max |p - torch fp32| %.2e, max |p - fp64| %.2e" % (layout, e32, e64))
        lab = labels.cpu()
        assert torch.equal(lab[clear], want_labels[clear]), layout
        assert lab.min() >= 1 and lab.max() <= 16
        ref_hist = E.fast_hist_crop(lab.numpy(), pts[:, 3].cpu().numpy().astype(int), np.arange(16))
        assert np.array_equal(hist.view(16, 16).cpu().numpy(), ref_hist), layout
        results.append((probs, labels, hist))
    assert all(torch.equal(a, b) for a, b in zip(results[0], results[1])), "the two layouts give different bits"


# ------------------------------------------------------------------ simple_test / pipelined_test / forward_train
def _plain_keys_equal(a, b, tag):
    for k, v in a.items():
        w = b[k]
        if torch.is_tensor(v):
            assert torch.equal(v, w), "%s: %s differs" % (tag, k)
        elif isinstance(v, np.ndarray):
            assert np.array_equal(v, w), "%s: %s differs" % (tag, k)
        elif isinstance(v, (list, tuple)) and v and torch.is_tensor(v[0]):
            assert all(torch.equal(x, y) for x, y in zip(v, w)), "%s: %s differs" % (tag, k)


def _snapshot(out):
    return {k: (v.clone() if torch.is_tensor(v) else [t.clone() for t in v] if isinstance(v, list) and v and torch.is_tensor(v[0])
                else v.copy() if isinstance(v, np.ndarray) else v) for k, v in out.items()}


def _check_lidarseg_keys(model, out, pts, metas, tag):
    assert out["output_points"].is_cuda and out["output_points"].dtype == torch.int64, tag
    assert isinstance(out["evaluation_semantic"], np.ndarray) and out["evaluation_semantic"].shape == (16, 16), tag
    assert out["evaluation_semantic"].dtype == np.int64, tag
    assert torch.equal(out["target_points"], torch.cat(pts, dim=0)), tag
    probs = model.pts_bbox_head.forward_lidarseg(out["pred_c"], pts, metas)
    direct = torch.argmax(probs[:, 1:], dim=1) + 1
    assert torch.equal(out["output_points"], direct), tag
    hist = E.fast_hist_crop(direct.cpu().numpy(), torch.cat(pts)[:, 3].cpu().numpy().astype(int), np.arange(16))
    assert np.array_equal(out["evaluation_semantic"], hist), tag
    assert int(hist.sum()) > 1000, tag


@pytest.mark.parametrize("graph", [True, False])
def test_simple_test_with_points_occ(dev, graph):
    bench, model, samples, gts = _model(dev)
    head = model.pts_bbox_head
    metas = [dict(pc_range=head.point_cloud_range.tolist())]
    pts = [_points(20000, 31, dev)]
    with torch.no_grad():
        model.graph_simple_test = graph
        for gt in (gts[1], None):
            kw = dict(bench.simple_test_kwargs(samples[1]), gt_occ=gt, img_metas=metas)
            plain = _snapshot(model.simple_test(**kw))
            out = model.simple_test(points_occ=pts, **kw)
            assert set(out) == set(plain) | {"output_points", "target_points", "evaluation_semantic"}
            _plain_keys_equal(plain, out, "graph=%s gt=%s" % (graph, gt is not None))
            assert ("SSC_metric" in out) == (gt is not None)
            _check_lidarseg_keys(model, out, pts, metas, "graph=%s gt=%s" % (graph, gt is not None))
    model.graph_simple_test = True
    if graph:
        assert model._pipe1 is not None and model.graph_unavailable is None, model.graph_unavailable


def test_pipelined_test_with_and_without_points_occ(dev):
    from co_occ_amd import apis
    bench, model, samples, gts = _model(dev)
    metas = [dict(pc_range=model.pts_bbox_head.point_cloud_range.tolist())]
    data = []
    for i, (s, g) in enumerate(zip(samples, gts)):
        d = dict(precomputed=bench.simple_test_kwargs(s)["precomputed"], gt_occ=g, img_metas=metas)
        if i % 3 != 1:
            d["points_occ"] = [_points(12000 + 500 * i, 100 + i, dev)]
        data.append(d)
    with torch.no_grad():
        model.graph_simple_test = False
        ref = [_snapshot(model.simple_test(**d)) for d in data]
    model.graph_simple_test = True
    n = 0
    for i, (d, res) in enumerate(apis.pipelined_test(model, iter(data), slots=4, dense_streams=2)):
        assert d is data[i]
        want = ref[i]
        assert set(res) >= set(want) - {"fine_count"}, sorted(set(want) - set(res))
        assert ("output_points" in res) == ("points_occ" in d), i
        for k in ("pred_c", "pred_f", "output_points", "target_points"):
            if k in want:
                assert torch.equal(res[k], want[k]), "sample %d: %s" % (i, k)
        assert torch.equal(res["output_voxels_fine"][0], want["output_voxels_fine"][0]), "sample %d: fine outputs" % i
        assert torch.equal(res["output_coords_fine"][0], want["output_coords_fine"][0]), "sample %d: fine coords" % i
        for k in ("SC_metric", "SSC_metric", "SSC_metric_fine", "evaluation_semantic"):
            if k in want:
                assert np.array_equal(res[k], want[k]), "sample %d: %s" % (i, k)
        n += 1
    assert n == 8


def test_forward_train_reports_point_mean_iou(dev, monkeypatch):
    bench, model, samples, gts = _model(dev)
    s, head = samples[2], model.pts_bbox_head
    monkeypatch.setattr(model, "use_rendering", False)
    seen = []
    orig = head.forward_lidarseg
    monkeypatch.setattr(head, "forward_lidarseg", lambda ov, p, m=None: (seen.append(ov.detach().clone()), orig(ov, p, m))[1])
    pts = [_points(30000, 7, dev)]
    pts[0] = torch.cat([pts[0], pts[0][:, 3:4]], 1)                 # 5 columns: the train target is the LAST one
    pts[0][:, 3] = 3.0
    kw = dict(img_inputs=(None,) + tuple(s["transform"]), gt_occ=gts[2],
              precomputed=dict(img_voxel_feats=s["img"], pts_voxel_feats=s["pts"], img_feats=s["img_feats"]))
    model.train()
    try:
        plain = model.forward_train(generator=torch.Generator(device=dev).manual_seed(0), **kw)
        losses = model.forward_train(generator=torch.Generator(device=dev).manual_seed(0), points_occ=pts,
                                     img_metas=[dict(pc_range=head.point_cloud_range.tolist())], **kw)
    finally:
        model.eval()
    assert set(losses) == set(plain) | {"point_mean_iou"}
    for k in plain:
        assert_close(losses[k].detach().cpu(), plain[k].detach().cpu(), tol=1e-4, what=k)
    v = losses["point_mean_iou"]
    assert v.is_cuda and v.dtype == torch.float64 and v.dim() == 0
    # host reference (occ_head.py:357-379) on the logits the head was given
    lg = seen[0].cpu().contiguous()
    r = head.point_cloud_range
    q = ((pts[0][:, :3].cpu() - r[:3]) / (r[3:] - r[:3])) * 2 - 1
    sl = F.grid_sample(lg, q[:, [2, 1, 0]].view(1, 1, 1, -1, 3), mode='bilinear', padding_mode='border', align_corners=True)
    cls = (torch.argmax(sl.squeeze().t()[:, 1:], dim=1) + 1).numpy()
    hist = E.fast_hist_crop(cls, pts[0][:, -1].long().cpu().numpy(), np.arange(16))
    with np.errstate(divide="ignore", invalid="ignore"):
        want = np.nanmean(E.per_class_iu(hist))
    assert abs(float(v) - want) <= 1e-12, (float(v), want)


# ------------------------------------------------------------------ co-runner guard
def test_lidarseg_launch_is_bit_stable_beside_the_mfma_corunner(dev, tmp_path_factory):
    import test_gpu_corunner as C
    S = C._scene(dev)
    m, s = S["model"], S["s"]
    with torch.no_grad():
        pred = m.pts_bbox_head(voxel_feats=S["sem"], img_feats=s["img_feats"], transform=s["transform"])["output_voxels"][0]
    rng = m.pts_bbox_head.lidarseg_range(None)
    pts = _points(35000, 23, dev)
    n = pts.shape[0]

    def fn():
        probs = torch.empty(n, 17, device=dev)
        labels = torch.empty(n, dtype=torch.int64, device=dev)
        hist = torch.empty(256, dtype=torch.int64, device=dev)
        E.lidarseg_points(pred, pts, rng, "border", probs=probs, labels=labels, hist=hist)
        return [probs, labels, hist]
    ref, got = C._run_beside(S, fn, n=20, corunner=C._mfma_corunner(tmp_path_factory.getbasetemp()))
    assert C._count_differing(ref, got) == 0
