"""SSIM of the rendered colour maps on the MI355X: ``coocc_render_eval_ssim`` (csrc/render_ssim.hip) against the float64 definition
of the test tree (tests/render_ssim_ref.py ``ssim64``, which tests/test_render_ssim_host.py checks against a second float64 form and
against values worked out by hand), and the calls that carry it -- ``evaluation.render_ssim`` / ``render_eval(ssim=True)``,
``COOCC_Ray.simple_test`` (captured and eager), ``apis.pipelined_test``, ``RenderEvaluator`` -- determinism, and the co-runner guard
of the new kernels.

Bounds.  The channel means (block columns 0-2, float64): within 1e-9 of ``ssim64``.  Derived, not measured: the products of fp32
values are exact in fp64, the 49-term sums carry at most 49 x 2^-53 relative error each, and the cancellation in uxx - ux^2
(uxx <= 4 for |values| <= 2) stands against C2 = (0.03 x 2)^2 = 3.6e-3, which gives about 4 x 49 x 2^-53 / 3.6e-3 = 6e-12 per
window; the bound leaves two orders.  The view's value (column 3) is exactly float32((c0 + c1 + c2) / 3) of the block's own
columns, the mean over the views (column 4) exactly their sequential fp32 sum / N.  Against skimage's own fp32 chain (``ssim32``):
the project's rule |a - b| <= 1e-4 max(1, |ref|) (tests/util.py).  The kernel's tile is 16 x 64 windows (RS_TH, RS_TW): the edge
shapes below are one window short of, exactly at, and one past a tile edge in both directions."""
import os
import sys

import numpy as np
import pytest
import torch

from util import TOL

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import render_ssim_ref as S  # noqa: E402
from co_occ_amd import apis, evaluation as E  # noqa: E402

pytestmark = pytest.mark.gpu
TH, TW = 16, 64                                    # csrc/render_ssim.hip RS_TH, RS_TW
SSIM_KEYS = {"ssim", "ssim_mean"}
BOUND64 = 1e-9


def _np(v):
    return v.detach().cpu().numpy() if torch.is_tensor(v) else np.asarray(v)


def _random_maps(N, H, W, seed, dev):
    """Seeded maps with values outside [0, 1] (|values| <= 2), as tests/test_gpu_render_eval.py ``_random_maps``."""
    g = torch.Generator().manual_seed(seed)
    rgbs = torch.rand(N, H, W, 3, generator=g) * 1.4 - 0.2
    gt_img = torch.rand(N, 3, H, W, generator=g) * 1.6 - 0.3
    return rgbs.to(dev), gt_img.to(dev)


def _seq_mean32(vals):
    total = np.float32(0)
    for s in np.asarray(vals, dtype=np.float32):
        total = np.float32(total + s)
    return np.float32(total / np.float32(len(vals)))


def _check_block(block, rgbs, gt_img, what, R=2.0, fp32_chain=True):
    """Every column of an SSIM block against the float64 definition; prints the distances before asserting."""
    assert block.dtype == torch.float64 and block.is_cuda and tuple(block.shape) == (rgbs.shape[0], E.RENDER_SSIM_SLOTS)
    b = _np(block)
    x, y = _np(rgbs), _np(gt_img)
    N, H, W = x.shape[:3]
    ref64 = S.ssim64(x, y, R)
    e64 = float(np.abs(b[:, :3] - ref64).max())
    line = "\n[ssim] %-40s channel means vs float64 %.3e (bound %.0e)" % (what, e64, BOUND64)
    if fp32_chain:
        s32, mean32 = S.ssim32(x, y, R)
        e_rule = float(np.abs(b[:, E.RS_SSIM] - s32).max() / max(1.0, np.abs(s32).max()))
        e_k, e_r = np.abs(b[:, E.RS_SSIM] - ref64.mean(1)), np.abs(s32.astype(np.float64) - ref64.mean(1))
        line += " | view value vs fp32 chain %.3e (rule %.0e) | vs float64: kernel %s, fp32 chain %s" % (
            e_rule, TOL, np.array2string(e_k, precision=2), np.array2string(e_r, precision=2))
    print(line)
    assert np.isfinite(b).all(), what
    assert e64 <= BOUND64, "%s: channel means %.3e from float64" % (what, e64)
    assert np.array_equal(b[:, E.RS_SSIM], S.view_ssim(b[:, :3]).astype(np.float64)), what + ": column 3 is not float32((c0+c1+c2)/3)"
    assert (b[:, E.RS_SSIM_MEAN] == np.float64(_seq_mean32(b[:, E.RS_SSIM]))).all(), what + ": column 4"
    assert (b[:, E.RS_COUNT] == (H - 6) * (W - 6)).all() and (b[:, E.RS_RANGE] == R).all() and (b[:, 7] == 0).all(), what
    if fp32_chain:
        assert e_rule <= TOL, "%s: %.3e against the fp32 chain" % (what, e_rule)
        assert abs(float(b[0, E.RS_SSIM_MEAN]) - float(mean32)) <= TOL * max(1.0, abs(float(mean32))), what
    return ref64


# ------------------------------------------------------------------ the kernel against the float64 definition
def test_golden_maps(dev, golden):
    g = golden("render_eval")
    rgbs, gt_img = torch.from_numpy(g["rgbs"]).to(dev), torch.from_numpy(g["gt_img"]).to(dev)
    assert (g["rgbs"] > 1).any() and (g["rgbs"] < 0).any() and (g["gt_img"] > 1).any() and (g["gt_img"] < 0).any()
    block = E.render_ssim(rgbs, gt_img)
    _check_block(block, rgbs, gt_img, "golden 3 x 32 x 48")
    k = E.render_ssim_keys(block)
    assert set(k) == {"ssim", "ssim_mean", "ssim_channels"} and all(v.is_cuda for v in k.values())
    assert k["ssim"].dtype == torch.float32 and k["ssim"].shape == (3,) and k["ssim_mean"].dtype == torch.float32 and k["ssim_mean"].dim() == 0
    assert k["ssim_channels"].dtype == torch.float64 and k["ssim_channels"].shape == (3, 3)
    assert np.array_equal(_np(k["ssim"]).astype(np.float64), _np(block[:, E.RS_SSIM]))
    # ``out``: the block is written where the caller says
    out = torch.full((3, 8), -1.0, dtype=torch.float64, device=dev)
    assert E.render_ssim(rgbs, gt_img, out=out) is out and torch.equal(out.view(torch.int64), block.view(torch.int64))


EDGE_SHAPES = [(2, 7, 7), (2, 7, 8), (2, 8, 7), (3, 32, 46), (2, 23, 72), (2, 39, 132)] + \
              [(1, h, w) for h in (TH + 5, TH + 6, TH + 7) for w in (TW + 5, TW + 6, TW + 7)]


@pytest.mark.parametrize("shape", EDGE_SHAPES, ids=lambda s: "%dx%dx%d" % s)
def test_smallest_and_edge_shapes(dev, shape):
    """One window; W not a multiple of 4 (one-element loads); one window short of, at, and past a tile edge in H and in W; a second
    tile column of 8 staged columns (W = 72) and of 68 (W = 132)."""
    N, H, W = shape
    rgbs, gt_img = _random_maps(N, H, W, 100 + H * W, dev)
    _check_block(E.render_ssim(rgbs, gt_img), rgbs, gt_img, "%d x %d x %d" % shape)


def test_maps_at_a_4_byte_offset_take_the_one_element_loads(dev, golden):
    g = golden("render_eval")

    def shifted(a):                                                   # the same values at an address that is 4 mod 16
        t = torch.from_numpy(a)
        buf = torch.empty(t.numel() + 1, device=dev)
        buf[1:] = t.reshape(-1).to(dev)
        assert buf[1:].data_ptr() % 16 == 4
        return buf[1:].view(t.shape)
    rgbs, gt_img = shifted(g["rgbs"]), shifted(g["gt_img"])
    block = E.render_ssim(rgbs, gt_img)
    _check_block(block, rgbs, gt_img, "golden at a 4-byte offset")
    aligned = E.render_ssim(torch.from_numpy(g["rgbs"]).to(dev), torch.from_numpy(g["gt_img"]).to(dev))
    assert torch.equal(block.view(torch.int64), aligned.view(torch.int64)), "the two load forms give different bits"


def test_a_view_with_more_partials_than_one_wave_has_lanes(dev):
    N, H, W = 2, 300, 520
    assert ((H - 6 + TH - 1) // TH) * ((W - 6 + TW - 1) // TW) > 64
    rgbs, gt_img = _random_maps(N, H, W, 8, dev)
    _check_block(E.render_ssim(rgbs, gt_img), rgbs, gt_img, "2 x 300 x 520")


def test_special_values(dev):
    rgbs, gt_img = _random_maps(3, 40, 70, 12, dev)
    same = E.render_ssim(rgbs, rgbs.permute(0, 3, 1, 2).contiguous())
    assert float((same[:, :3] - 1).abs().max()) <= 1e-12 and torch.equal(same[:, E.RS_SSIM], torch.ones_like(same[:, 0]))
    const = rgbs.clone()
    const[1] = 0.375                                                  # a constant view: zero variance and covariance
    block = E.render_ssim(const, gt_img)
    assert torch.isfinite(block).all()
    _check_block(block, const, gt_img, "a constant view")
    zero = torch.zeros_like(rgbs)
    assert torch.equal(E.render_ssim(zero, zero.permute(0, 3, 1, 2).contiguous())[:, :4], torch.ones(3, 4, dtype=torch.float64, device=dev))
    two, one = E.render_ssim(rgbs, gt_img), E.render_ssim(rgbs, gt_img, data_range=1.0)
    assert float((two[:, :3] - one[:, :3]).abs().min()) > 1e-6, "data_range has no effect"
    _check_block(one, rgbs, gt_img, "data_range = 1", R=1.0)
    _check_block(two, rgbs, gt_img, "data_range = 2", R=2.0)
    for bad in (0.0, -1.0, float("inf"), float("nan")):
        with pytest.raises(ValueError, match="data_range"):
            E.render_ssim(rgbs, gt_img, data_range=bad)


def test_r101_map_size_equals_float64_and_two_runs_are_bit_equal(dev):
    N, H, W = 6, 896, 1600
    rgbs, gt_img = _random_maps(N, H, W, 3, dev)
    a, b = E.render_ssim(rgbs, gt_img), E.render_ssim(rgbs, gt_img)
    assert torch.equal(a.view(torch.int64), b.view(torch.int64)), "two runs differ"
    _check_block(a, rgbs, gt_img, "r101 maps 6 x 896 x 1600", fp32_chain=False)


def test_render_eval_adds_exactly_the_ssim_keys(dev, golden):
    g = golden("render_eval")
    rgbs, depths, gt_img, gt_depth = (torch.from_numpy(g[k]).to(dev) for k in ("rgbs", "depths", "gt_img", "gt_depth"))
    today = {"psnr", "psnr_mean", "depth_min", "depth_max", "depth_sq_err", "depth_valid", "stats"}
    plain = E.render_eval(rgbs, depths, gt_img, gt_depth)
    assert set(plain) == today and set(E.render_eval(rgbs, depths, gt_img, gt_depth, ssim=False)) == today
    res = E.render_eval(rgbs, depths, gt_img, gt_depth, ssim=True)
    assert set(res) == today | {"ssim", "ssim_mean", "ssim_stats"}
    for k in today:
        assert torch.equal(res[k], plain[k]), k
    direct = E.render_ssim(rgbs, gt_img)
    assert torch.equal(res["ssim_stats"].view(torch.int64), direct.view(torch.int64))
    assert res["ssim"].dtype == torch.float32 and res["ssim"].is_cuda and torch.equal(res["ssim"], direct[:, E.RS_SSIM].float())
    assert torch.equal(res["ssim_mean"], direct[0, E.RS_SSIM_MEAN].float())
    one = E.render_eval(rgbs, depths, gt_img, ssim=True, data_range=1.0, panels=True, stream=torch.cuda.Stream(device=dev))
    torch.cuda.synchronize()
    assert set(one) == (today - {"depth_sq_err", "depth_valid"}) | {"ssim", "ssim_mean", "ssim_stats", "panels"}
    assert torch.equal(one["ssim_stats"].view(torch.int64), E.render_ssim(rgbs, gt_img, 1.0).view(torch.int64))
    with pytest.raises(ValueError, match="ssim needs rgbs"):
        E.render_eval(None, depths, None, gt_depth, ssim=True)
    ev = E.RenderEvaluator(device=dev)
    ev.update(rgbs, depths, gt_img, gt_depth)
    assert "ssim_mean" not in ev.summary()
    ev.update(rgbs, depths, gt_img, gt_depth, ssim=True)
    s = ev.summary()
    assert s["views"] == 6 and abs(s["ssim_mean"] - _np(direct[:, E.RS_SSIM]).mean()) <= 1e-15


# ------------------------------------------------------------------ simple_test / pipelined_test
def _scene_model(dev):
    import test_gpu_lidarseg as L
    bench, model, samples, gts = L._model(dev)
    return L, bench, model, samples, gts


def _images(shape, seed, dev):
    N, H, W = shape
    g = torch.Generator().manual_seed(seed)
    imgs = torch.rand(1, N, 3, H, W, generator=g)
    gd = torch.rand(1, N, H, W, generator=g) * 50 + 1
    gd[torch.rand(1, N, H, W, generator=g) < 0.5] = 0
    return imgs.to(dev), gd.to(dev)


def _want_keys(out, imgs):
    """``ssim`` / ``ssim_mean`` of the maps a call returned, from the kernel called directly."""
    b = _np(E.render_ssim(out["rgbs"], imgs[0]))
    return b[:, E.RS_SSIM].astype(np.float32), np.float32(b[0, E.RS_SSIM_MEAN])


@pytest.mark.parametrize("graph", [True, False])
def test_simple_test_adds_ssim_and_changes_nothing_else(dev, graph):
    L, bench, model, samples, gts = _scene_model(dev)
    s = samples[3]
    try:
        with torch.no_grad():
            model.graph_simple_test = graph
            kw = dict(bench.simple_test_kwargs(s), gt_occ=gts[3])
            shape = model.simple_test(**kw)["depths"].shape
            imgs, gd = _images(shape, 77, dev)
            kw.update(img=(imgs,) + tuple(s["transform"]), gt_depths=gd)
            assert model.render_ssim is False
            model.render_ssim = True                                  # without render_eval: no effect
            assert not (SSIM_KEYS & set(model.simple_test(**kw)))
            model.render_eval, model.render_ssim = True, False
            plain = L._snapshot(model.simple_test(**kw))
            assert not (SSIM_KEYS & set(plain)) and "psnr" in plain
            model.render_ssim = True
            out = model.simple_test(**kw)
            assert set(out) == set(plain) | SSIM_KEYS
            L._plain_keys_equal(plain, out, "graph=%s" % graph)       # every other value, bit for bit
            want, want_mean = _want_keys(out, imgs)
            assert isinstance(out["ssim"], np.ndarray) and out["ssim"].dtype == np.float32 and out["ssim"].shape == (shape[0],)
            assert out["ssim_mean"].dtype == np.float32 and out["ssim_mean"].shape == ()
            assert np.array_equal(out["ssim"], want) and out["ssim_mean"] == want_mean
            if graph:                                                 # the values themselves, once: against float64
                _check_block(E.render_ssim(out["rgbs"], imgs[0]), out["rgbs"], imgs[0], "simple_test maps", fp32_chain=False)
            assert set(model.simple_test(**dict(kw, img=None))) == set(plain) - {"psnr", "psnr_mean", "depth_sq_err", "depth_valid"}
            model.metrics_on_device = True
            on_dev = model.simple_test(**kw)
            for k in SSIM_KEYS:
                assert torch.is_tensor(on_dev[k]) and on_dev[k].is_cuda, k
                assert np.array_equal(_np(on_dev[k]), out[k]) and _np(on_dev[k]).dtype == out[k].dtype, k
    finally:
        model.render_eval, model.render_ssim, model.metrics_on_device, model.graph_simple_test = False, False, False, True


def test_pipelined_test_gives_the_eager_values_and_the_evaluator_their_mean(dev):
    L, bench, model, samples, gts = _scene_model(dev)
    render_keys = {"psnr", "psnr_mean", "depth_sq_err", "depth_valid"} | SSIM_KEYS
    try:
        model.render_eval = model.render_ssim = True
        with torch.no_grad():
            model.graph_simple_test = False
            shape = model.simple_test(**bench.simple_test_kwargs(samples[0]))["depths"].shape
            data = []
            for i in range(4):
                imgs, gd = _images(shape, 600 + i, dev)
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
            assert (render_keys & set(res)) == (render_keys & set(want)) == (render_keys if i != 2 else render_keys - {"depth_sq_err", "depth_valid"}), i
            for k in render_keys & set(want):
                assert res[k].dtype == want[k].dtype and np.array_equal(res[k], want[k]), "sample %d: %s" % (i, k)
            for k in {"SC_metric", "SSC_metric", "SSC_metric_fine"} & set(want):
                assert np.array_equal(res[k], want[k]), "sample %d: %s" % (i, k)
            ev.update(res["rgbs"], res["depths"], d["img"][0][0], ssim=True)
            n += 1
        assert n == 4
        s = ev.summary()
        assert s["views"] == 4 * shape[0]
        assert abs(s["ssim_mean"] - np.mean([r["ssim"].astype(np.float64) for r in ref])) <= 1e-14
        # with render_ssim off the loop reports what it did before
        model.render_ssim = False
        for i, (d, res) in enumerate(apis.pipelined_test(model, iter(data[:3]), slots=4, dense_streams=2)):
            assert not (SSIM_KEYS & set(res)) and np.array_equal(res["psnr"], ref[i]["psnr"]), i
            if i != 2:
                assert np.array_equal(res["depth_sq_err"], ref[i]["depth_sq_err"]), i
    finally:
        model.render_eval, model.render_ssim, model.graph_simple_test = False, False, True


def test_depth_only_detector_accepts_the_key_and_reports_no_ssim(dev):
    """COOCC_Ray_L has no rgb head: ``render_ssim=True`` is taken and never adds a key."""
    import co_occ_amd as pkg
    import co_occ_amd.synth as synth
    import test_gpu_corunner as C
    Sc = C._scene(dev)
    m, s = Sc["model"], Sc["s"]
    with torch.no_grad():
        out = m.decode(Sc["vf"], Sc["gemo"], s["img_feats"], s["transform"], render=True, depth_only=True)
    det = pkg.build_detector(synth.model_cfg_lidar(rendering=True), external_encoders=True, render_eval=True, render_ssim=True)
    assert isinstance(det, pkg.COOCC_Ray_L) and det.render_eval is True and det.render_ssim is True
    imgs, gd = _images(out["depths"].shape, 9, dev)
    res = det.finish_test_result(out, gt_img=imgs[0], gt_depths=[None, gd, None])
    assert not (SSIM_KEYS & set(res)) and "depth_sq_err" in res and "psnr" not in res


# ------------------------------------------------------------------ co-runner guard
@pytest.mark.parametrize("corunner", ["h2p", "wino", "mfma"])
def test_ssim_kernels_are_bit_stable_beside_matrix_core_work(dev, corunner, tmp_path_factory):
    """The SSIM pair 20 times beside the split-f16 layers and beside the MFMA-only kernel: the bits of the kernels alone."""
    import test_gpu_corunner as C
    Sc = C._scene(dev)
    rgbs, gt_img = _random_maps(6, 256, 704, 21, dev)
    co = C._mfma_corunner(tmp_path_factory.getbasetemp()) if corunner == "mfma" else corunner
    ref, got = C._run_beside(Sc, lambda: [E.render_ssim(rgbs, gt_img)], n=20, corunner=co)
    assert len(got) == 20 and C._count_differing(ref, got) == 0
