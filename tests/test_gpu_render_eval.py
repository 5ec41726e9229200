"""Render evaluation on the MI355X: ``coocc_render_eval_stats`` / ``coocc_render_panels`` against the fixture of the unmodified
reference (tests/golden/render_eval.npz, tools/gen_golden_render_eval.py) and, at sizes the fixture cannot cover, against the torch
restatement that tests/test_render_eval_host.py pins to that fixture (tests/render_eval_ref.py, run on the CPU); the calls that carry
it -- ``COOCC_Ray.simple_test`` (captured and eager), ``apis.pipelined_test``, ``RenderEvaluator``, ``apis.save_rendered_panels`` --
determinism, and the co-runner guard of the new kernels.

Bounds.  Panels, depth extrema and the valid-pixel count are compared bit for bit.  PSNR: the project's rule
|a - b| <= 1e-4 max(1, |ref|) (tests/util.py) against the fp32 reference, and no further from the float64 evaluation than 1.5 x the
fp32 reference's own distance (the anchor factor of DESIGN section 4); where the reference is the restatement and not the fixture, that
distance is floored at one fp32 rounding, 2^-24 |psnr| (a reference that happens to be exact would otherwise demand more than the
fp32 result type can hold).  Squared depth error (fp64 sums of n non-negative terms, added in another order than the reference's):
relative difference <= n 2^-53, the worst case of any summation order."""
import os
import sys

import numpy as np
import pytest
import torch

from util import TOL

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import render_eval_ref as R  # noqa: E402
from co_occ_amd import apis, evaluation as E  # noqa: E402

pytestmark = pytest.mark.gpu
RENDER_KEYS = {"psnr", "psnr_mean", "depth_sq_err", "depth_valid"}


def _np(v):
    return v.detach().cpu().numpy() if torch.is_tensor(v) else np.asarray(v)


def _check_psnr(got, ref32, ref64, what, floor=False):
    """The two PSNR bounds of the module docstring; prints both errors before asserting.  ``ref64 = None`` (the mean over the
    views: an fp32 accumulation on both sides, whose float64 distance says nothing about the kernel): the project's rule alone."""
    got, ref32 = _np(got).astype(np.float64).reshape(-1), _np(ref32).astype(np.float64).reshape(-1)
    e_rule = float(np.abs(got - ref32).max() / max(1.0, np.abs(ref32).max()))
    if ref64 is None:
        print("\n[psnr] %-34s vs fp32 reference %.3e (rule %.0e)" % (what, e_rule, TOL))
        assert e_rule <= TOL, "%s: %.3e against the fp32 reference" % (what, e_rule)
        return
    ref64 = _np(ref64).reshape(-1)
    e_got, e_ref = np.abs(got - ref64), np.abs(ref32 - ref64)
    if floor:
        e_ref = np.maximum(e_ref, 2.0 ** -24 * np.abs(ref64))
    print("\n[psnr] %-34s vs fp32 reference %.3e (rule %.0e) | vs float64: kernel %s, fp32 reference %s"
          % (what, e_rule, TOL, np.array2string(e_got, precision=2), np.array2string(e_ref, precision=2)))
    assert e_rule <= TOL, "%s: %.3e against the fp32 reference" % (what, e_rule)
    assert (e_got <= 1.5 * e_ref).all(), "%s: further from float64 than 1.5 x the fp32 reference: %s vs %s" % (what, e_got, e_ref)


def _check_depth_error(sq, nv, depths, gt_depth, what):
    want_sq, want_nv = R.depth_error(depths.cpu(), gt_depth.cpu())
    assert np.array_equal(_np(nv), want_nv.numpy()), what
    n = depths[0].numel()
    e = float(np.abs(_np(sq) / want_sq.numpy() - 1).max())
    print("[depth] %-33s relative difference of the fp64 sums %.2e (bound %.2e)" % (what, e, n * 2.0 ** -53))
    assert e <= n * 2.0 ** -53, what


def _random_maps(N, H, W, seed, dev):
    g = torch.Generator().manual_seed(seed)
    rgbs = torch.rand(N, H, W, 3, generator=g) * 1.4 - 0.2
    gt_img = torch.rand(N, 3, H, W, generator=g) * 1.6 - 0.3
    depths = torch.rand(N, H, W, generator=g) * 56 + 2
    depths[1] = 11.5                                                  # a constant view: dmax == dmin
    gt_depth = torch.rand(N, H, W, generator=g) * 58 + 1
    gt_depth[torch.rand(N, H, W, generator=g) < 0.4] = 0
    return tuple(t.to(dev) for t in (rgbs, depths, gt_img, gt_depth))


# ------------------------------------------------------------------ kernels vs the unmodified reference
def test_kernels_equal_the_reference_on_the_golden_maps(dev, golden):
    g = golden("render_eval")
    rgbs, depths, gt_img, gt_depth = (torch.from_numpy(g[k]).to(dev) for k in ("rgbs", "depths", "gt_img", "gt_depth"))
    res = E.render_eval(rgbs, depths, gt_img, gt_depth, panels=True)
    assert all(torch.is_tensor(v) and v.is_cuda for v in res.values())
    assert res["panels"].dtype == torch.uint8 and np.array_equal(_np(res["panels"]), g["panels"])
    assert res["depth_min"].dtype == torch.float32
    assert np.array_equal(_np(res["depth_min"]), g["depth_min"]) and np.array_equal(_np(res["depth_max"]), g["depth_max"])
    assert g["depth_min"][1] == g["depth_max"][1] and (g["rgbs"] > 1).any() and (g["rgbs"] < 0).any()    # the views the issue names
    assert res["psnr"].dtype == torch.float32 and res["psnr"].shape == (3,)
    _check_psnr(res["psnr"], g["psnr"], g["psnr64"], "golden, per view")
    _check_psnr(res["psnr_mean"], g["psnr_mean"], None, "golden, mean")
    assert np.array_equal(_np(res["depth_valid"]), g["depth_valid"]) and res["depth_valid"].dtype == torch.int64
    assert np.abs(_np(res["depth_sq_err"]) / g["depth_sq_err64"] - 1).max() <= 32 * 48 * 2.0 ** -53
    assert np.abs(_np(res["stats"][:, E.RE_SQ_RGB]) / g["sq_rgb64"] - 1).max() <= 3 * 32 * 48 * 2.0 ** -53
    # without gt_depth: no depth keys; a zero error gives +inf, as upstream
    res = E.render_eval(rgbs, depths, gt_img)
    assert set(res) == {"psnr", "psnr_mean", "depth_min", "depth_max", "stats"}
    same = E.render_eval(rgbs, depths, rgbs.permute(0, 3, 1, 2).contiguous())
    assert torch.isinf(same["psnr"]).all() and (same["psnr"] > 0).all()


def test_one_pixel_form_on_sizes_and_addresses_the_vector_form_does_not_take(dev, golden):
    """W = 46 (not a multiple of 4) and maps at a 4-byte offset: the kernels fall back to one pixel per thread; same bytes."""
    g = golden("render_eval")
    cpu = [torch.from_numpy(g[k]) for k in ("rgbs", "depths", "gt_img", "gt_depth")]
    crop = [cpu[0][:, :, :46].contiguous(), cpu[1][:, :, :46].contiguous(), cpu[2][:, :, :, :46].contiguous(), cpu[3][:, :, :46].contiguous()]

    def shifted(t):                                                   # the same values at an address that is 4 mod 16
        buf = torch.empty(t.numel() + 1, device=dev)
        buf[1:] = t.reshape(-1).to(dev)
        return buf[1:].view(t.shape)
    for what, maps in (("W = 46", [t.to(dev) for t in crop]), ("4-byte offset", [shifted(t) for t in cpu])):
        ref = crop if what == "W = 46" else cpu
        res = E.render_eval(*maps, panels=True)
        assert np.array_equal(_np(res["panels"]), R.panels(ref[0], ref[1], ref[2]).numpy()), what
        _check_psnr(res["psnr"], R.psnr(ref[0], ref[2])[0], R.psnr64(ref[0], ref[2]), what, floor=True)
        _check_depth_error(res["depth_sq_err"], res["depth_valid"], ref[1], ref[3], what)
    assert np.array_equal(_np(res["panels"]), g["panels"])            # the offset maps are the golden maps


# ------------------------------------------------------------------ the r101 map size, determinism
def test_r101_map_size_equals_the_restatement_and_two_runs_are_bit_equal(dev):
    N, H, W = 6, 896, 1600
    rgbs, depths, gt_img, gt_depth = _random_maps(N, H, W, 3, dev)
    a = E.render_eval(rgbs, depths, gt_img, gt_depth, panels=True)
    b = E.render_eval(rgbs, depths, gt_img, gt_depth, panels=True)
    assert torch.equal(a["stats"].view(torch.int64), b["stats"].view(torch.int64)), "two runs of the stats differ"
    assert torch.equal(a["panels"], b["panels"]), "two runs of the panels differ"
    c = [t.cpu() for t in (rgbs, depths, gt_img, gt_depth)]
    assert a["panels"].shape == (N, H, 3 * W, 3)
    assert torch.equal(a["panels"].cpu(), R.panels(c[0], c[1], c[2])), "r101 panels differ from the CPU bytes"
    assert torch.equal(a["depth_min"].cpu(), c[1].flatten(1).min(1).values) and torch.equal(a["depth_max"].cpu(), c[1].flatten(1).max(1).values)
    p32, mean32 = R.psnr(c[0], c[2])
    p64 = R.psnr64(c[0], c[2])
    _check_psnr(a["psnr"], p32, p64, "r101 maps, per view", floor=True)
    _check_psnr(a["psnr_mean"], mean32, None, "r101 maps, mean")
    _check_depth_error(a["depth_sq_err"], a["depth_valid"], c[1], c[3], "r101 maps")


# ------------------------------------------------------------------ simple_test / pipelined_test
def _scene_model(dev):
    import test_gpu_lidarseg as L
    bench, model, samples, gts = L._model(dev)
    return L, bench, model, samples, gts


def _ground_truth(shape, seed, dev):
    """A seeded image in [0, 1] [1,N,3,H,W] and a depth map [1,N,H,W] with invalid (0) pixels for maps of ``shape`` [N,H,W]."""
    N, H, W = shape
    g = torch.Generator().manual_seed(seed)
    imgs = torch.rand(1, N, 3, H, W, generator=g)
    gd = torch.rand(1, N, H, W, generator=g) * 50 + 1
    gd[torch.rand(1, N, H, W, generator=g) < 0.5] = 0
    return imgs.to(dev), gd.to(dev)


def _check_render_keys(out, imgs, gd, what):
    """The keys of a host-side result against the restatement applied to the maps the same call returned."""
    rgbs, depths = out["rgbs"].cpu(), out["depths"].cpu()
    gi = imgs[0].cpu()
    assert isinstance(out["psnr"], np.ndarray) and out["psnr"].dtype == np.float32 and out["psnr"].shape == (rgbs.shape[0],)
    assert out["psnr_mean"].dtype == np.float32 and out["psnr_mean"].shape == ()
    p32, mean32 = R.psnr(rgbs, gi)
    p64 = R.psnr64(rgbs, gi)
    _check_psnr(out["psnr"], p32, p64, what + ", per view", floor=True)
    _check_psnr(out["psnr_mean"], mean32, None, what + ", mean")
    assert out["depth_valid"].dtype == np.int64 and out["depth_sq_err"].dtype == np.float64
    _check_depth_error(out["depth_sq_err"], out["depth_valid"], depths, gd[0], what)


@pytest.mark.parametrize("graph", [True, False])
def test_simple_test_adds_the_render_keys_and_changes_nothing_else(dev, graph, tmp_path):
    L, bench, model, samples, gts = _scene_model(dev)
    s = samples[3]
    try:
        with torch.no_grad():
            model.graph_simple_test = graph
            kw = dict(bench.simple_test_kwargs(s), gt_occ=gts[3])
            shape = model.simple_test(**kw)["depths"].shape
            imgs, gd = _ground_truth(shape, 77, dev)
            kw.update(img=(imgs,) + tuple(s["transform"]), gt_depths=gd)
            assert model.render_eval is False
            plain = L._snapshot(model.simple_test(**kw))
            assert not (RENDER_KEYS & set(plain))
            model.render_eval = True
            out = model.simple_test(**kw)
            assert set(out) == set(plain) | RENDER_KEYS
            L._plain_keys_equal(plain, out, "graph=%s" % graph)       # the rest of the result, bit for bit
            _check_render_keys(out, imgs, gd, "simple_test graph=%s" % graph)
            # a depth ground truth of another size is not taken; without an image nothing is added
            small = model.simple_test(**dict(kw, gt_depths=gd[:, :, ::2]))
            assert set(small) == set(plain) | {"psnr", "psnr_mean"} and np.array_equal(small["psnr"], out["psnr"])
            assert set(model.simple_test(**dict(kw, img=None))) == set(plain)
            # metrics_on_device: the same bits as device tensors
            model.metrics_on_device = True
            on_dev = model.simple_test(**kw)
            for k in RENDER_KEYS:
                assert torch.is_tensor(on_dev[k]) and on_dev[k].is_cuda, k
                assert np.array_equal(_np(on_dev[k]), out[k]) and _np(on_dev[k]).dtype == out[k].dtype, k
            # the panels of the same result: the CPU's bytes
            paths, panels = apis.save_rendered_panels(out, str(tmp_path), gt_img=imgs[0])
            assert len(paths) == shape[0] and all(os.path.getsize(p) > 0 for p in paths)
            assert np.array_equal(panels, R.panels(out["rgbs"].cpu(), out["depths"].cpu(), imgs[0].cpu()).numpy())
    finally:
        model.render_eval, model.metrics_on_device, model.graph_simple_test = False, False, True


def test_pipelined_test_gives_the_eager_keys_and_the_evaluator_their_mean(dev):
    L, bench, model, samples, gts = _scene_model(dev)
    try:
        model.render_eval = True
        with torch.no_grad():
            model.graph_simple_test = False
            shape = model.simple_test(**bench.simple_test_kwargs(samples[0]))["depths"].shape
            data = []
            for i in range(5):
                imgs, gd = _ground_truth(shape, 500 + i, dev)
                d = dict(precomputed=bench.simple_test_kwargs(samples[i])["precomputed"], gt_occ=gts[i],
                         img=(imgs,) + tuple(samples[i]["transform"]))
                if i != 2:
                    d["gt_depths"] = gd
                data.append(d)
            ref = [L._snapshot(model.simple_test(**d)) for d in data]
        model.graph_simple_test = True
        ev, n = E.RenderEvaluator(device=dev), 0
        for i, (d, res) in enumerate(apis.pipelined_test(model, iter(data), slots=4, dense_streams=2)):
            want = ref[i]
            assert (RENDER_KEYS & set(res)) == (RENDER_KEYS & set(want)) == (RENDER_KEYS if i != 2 else {"psnr", "psnr_mean"}), i
            for k in RENDER_KEYS & set(want):
                assert res[k].dtype == want[k].dtype and np.array_equal(res[k], want[k]), "sample %d: %s" % (i, k)
            for k in {"SC_metric", "SSC_metric", "SSC_metric_fine"} & set(want):
                assert np.array_equal(res[k], want[k]), "sample %d: %s" % (i, k)
            assert torch.equal(res["rgbs"], want["rgbs"]) and torch.equal(res["depths"], want["depths"]), i
            ev.update(res["rgbs"], res["depths"], d["img"][0][0], d["gt_depths"][0] if "gt_depths" in d else None)
            n += 1
        assert n == 5
        s = ev.summary()
        assert s["views"] == 5 * shape[0]
        assert abs(s["psnr_mean"] - np.mean([r["psnr"].astype(np.float64).mean() for r in ref])) <= 1e-12 * abs(s["psnr_mean"])
        sq = sum(r["depth_sq_err"].sum() for r in ref if "depth_sq_err" in r)
        nv = sum(int(r["depth_valid"].sum()) for r in ref if "depth_valid" in r)
        assert s["depth_valid"] == nv and abs(s["depth_sq_err"] / sq - 1) <= 1e-12
    finally:
        model.render_eval, model.graph_simple_test = False, True


# ------------------------------------------------------------------ the depth-only variant
def test_depth_only_detector_reports_the_depth_keys_and_no_psnr(dev):
    """COOCC_Ray_L (no rgb head): depth-only maps, the depth ground truth at gt_depths[-2] -> depth keys; ``psnr`` absent, not NaN."""
    import co_occ_amd as pkg
    import co_occ_amd.synth as synth
    import test_gpu_corunner as C
    S = C._scene(dev)
    m, s = S["model"], S["s"]
    with torch.no_grad():
        out = m.decode(S["vf"], S["gemo"], s["img_feats"], s["transform"], render=True, depth_only=True)
    assert out["rgbs"] is None and out["depths"] is not None
    det = pkg.build_detector(synth.model_cfg_lidar(rendering=True), external_encoders=True)
    assert isinstance(det, pkg.COOCC_Ray_L) and det.render_eval is False
    imgs, gd = _ground_truth(out["depths"].shape, 9, dev)
    gts = [None, gd, None]                                            # gt_depths[-2], as coocc_ray_lidar.py:507 reads it
    assert not (RENDER_KEYS & set(det.finish_test_result(out, gt_img=imgs[0], gt_depths=gts)))
    det.render_eval = True
    res = det.finish_test_result(out, gt_img=imgs[0], gt_depths=gts)
    assert (RENDER_KEYS & set(res)) == {"depth_sq_err", "depth_valid"}
    _check_depth_error(res["depth_sq_err"], res["depth_valid"], out["depths"], gd[0], "depth-only")
    assert not (RENDER_KEYS & set(det.finish_test_result(out, gt_img=imgs[0], gt_depths=None)))
    direct = E.render_eval(None, out["depths"], None, gd[0])
    assert "psnr" not in direct and np.array_equal(_np(direct["depth_sq_err"]), res["depth_sq_err"])
    with pytest.raises(ValueError):
        E.render_eval(None, out["depths"], None, panels=True)


# ------------------------------------------------------------------ co-runner guard
@pytest.mark.parametrize("corunner", ["h2p", "wino", "mfma"])
def test_render_eval_kernels_are_bit_stable_beside_matrix_core_work(dev, corunner, tmp_path_factory):
    """The stats + panel kernels 20 times beside the split-f16 layers and beside the MFMA-only kernel: the bits of the kernels alone."""
    import test_gpu_corunner as C
    S = C._scene(dev)
    rgbs, depths, gt_img, gt_depth = _random_maps(6, 256, 704, 21, dev)

    def fn():
        r = E.render_eval(rgbs, depths, gt_img, gt_depth, panels=True)
        return [r["stats"], r["panels"]]
    co = C._mfma_corunner(tmp_path_factory.getbasetemp()) if corunner == "mfma" else corunner
    ref, got = C._run_beside(S, fn, n=20, corunner=co)
    assert len(got) == 20 and C._count_differing(ref, got) == 0
