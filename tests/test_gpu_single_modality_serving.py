"""The serving API for the two models without a fuser -- the camera-only ``COOCC_Ray`` (``occ_fuser=None``) and the LiDAR-only
``COOCC_Ray_L``: ``model.serving`` / ``simple_test`` with the captured dense stage / ``apis.pipelined_test`` against the eager
launches on the same frames, bit for bit."""
import os
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

pytestmark = pytest.mark.gpu

FMAP, NCAM = (16, 44), 1


def _build(cfg, dev, seed):
    import co_occ_amd as pkg
    from co_occ_amd import synth
    model = pkg.build_detector(cfg)
    model.load_state_dict(synth.random_state_dict(model.state_dict(), seed=seed))
    return model.to(dev).eval()


def camera_model(dev, grid, render):
    from co_occ_amd import synth
    X, Y, Z = grid
    cfg = synth.model_cfg(C=128, final_occ_size=(2 * X, 2 * Y, 2 * Z), input_size=(FMAP[0] * 16, FMAP[1] * 16), rendering=render)
    cfg.update(occ_fuser=None, external_encoders=True)
    cfg["img_view_transformer"]["grid_config"].update(xbound=[-X / 2.0, X / 2.0, 1.0], ybound=[-Y / 2.0, Y / 2.0, 1.0],
                                                      zbound=[-5.0, -5.0 + Z, 1.0])
    return _build(cfg, dev, 3)


def lidar_model(dev, fine=False, final=(100, 100, 8)):
    from co_occ_amd import synth
    cfg = synth.model_cfg_lidar()
    cfg.update(external_encoders=True)
    cfg["pts_bbox_head"].update(final_occ_size=list(final), sample_from_voxel=bool(fine))
    return _build(cfg, dev, 4)


def camera_frame(model, dev, seed):
    from co_occ_amd import synth
    rig = synth.camera_rig(NCAM, (FMAP[0] * 16, FMAP[1] * 16), seed=1234)          # one rig for every frame
    cams = tuple(rig[k].to(dev) for k in ("rots", "trans", "intrins", "post_rots", "post_trans", "bda"))
    depth, ctx = synth.lift_inputs(NCAM, model.img_view_transformer.D, FMAP, 128, seed=seed)
    transform = tuple(t.to(dev) if torch.is_tensor(t) else t for t in synth.rig_transform(rig))
    return dict(depth=depth.to(dev), ctx=ctx.to(dev), cams=cams, img_feats=[synth.image_feats(NCAM, FMAP, 512, seed=seed).to(dev)],
                transform=transform)


def lidar_frame(dev, seed, grid=(50, 50, 4)):
    from co_occ_amd import synth
    return dict(pts=synth.voxel_inputs(grid, C=128, seed=seed, p_pts=0.3)[1].to(dev))


def eager_camera(model, fr, render):
    vt = model.img_view_transformer
    vol = vt.lift_splat(fr["depth"], fr["ctx"], cams=fr["cams"])
    gemo = vt.get_geometry(*fr["cams"]) if render else None
    return model.forward_hot_path(vol, None, gemo, fr["img_feats"], fr["transform"], render=render)


KEYS = ("pred_c", "pred_f", "rgbs", "depths")


def grab(out, n_fine=None):
    d = {k: out[k].clone() for k in KEYS if out.get(k) is not None}
    if out.get("output_voxels_fine") is not None:
        fine, xyz = out["output_voxels_fine"][0], out["output_coords_fine"][0]
        if n_fine is not None:                       # capacity-sized outputs of the captured form: [3][n] packed at the start
            fine, xyz = fine[:n_fine], xyz.reshape(-1)[:3 * n_fine].view(3, n_fine)
        d["fine"], d["fine_xyz"] = fine.clone(), xyz.reshape(3, -1).clone()
    return d


def same(a, b, tag):
    assert sorted(a) == sorted(b), "%s: keys %s vs %s" % (tag, sorted(a), sorted(b))
    for k in a:
        assert torch.equal(a[k], b[k]), "%s: %s differs" % (tag, k)


def serve(model, frames, order, **kw):
    """``order`` (indices into ``frames``) through a 2-slot pipeline; the grabbed outputs, fine parts trimmed by the device count."""
    pipe = model.serving(frames[order[0]], slots=2, dense_streams=1, **kw)
    got = []
    try:
        for i in order:
            out = pipe.submit(frames[i]).result(wait=True)
            cnt = out.get("fine_count")
            got.append((grab(out, None if cnt is None else int(cnt.item()) * 8), cnt))
        assert pipe.fallbacks == 0
    finally:
        pipe.close()
    return got


def test_camera_only_frames_through_two_slots_equal_eager(dev):
    model = camera_model(dev, (50, 50, 4), render=False)
    frames = [camera_frame(model, dev, 4000), camera_frame(model, dev, 4013)]
    with torch.no_grad():
        ref = [grab(eager_camera(model, f, False)) for f in frames]
        torch.cuda.synchronize()
        got = serve(model, frames, (0, 1, 0), render=False)
    for (g, cnt), i in zip(got, (0, 1, 0)):
        assert int(cnt.item()) > 0
        same(ref[i], g, "frame %d" % i)
    assert "pred_f" in ref[0] and "fine" in ref[0] and not torch.equal(ref[0]["pred_c"], ref[1]["pred_c"])


def test_camera_only_with_the_render_block_and_a_pooled_volume_frame(dev):
    model = camera_model(dev, (100, 100, 8), render=True)
    frames = [camera_frame(model, dev, 4100), camera_frame(model, dev, 4113)]
    with torch.no_grad():
        ref = [grab(eager_camera(model, f, True)) for f in frames]
        torch.cuda.synchronize()
        got = serve(model, frames, (0, 1, 0), render=True)
        for (g, _), i in zip(got, (0, 1, 0)):
            assert "rgbs" in g and "depths" in g
            same(ref[i], g, "frame %d" % i)
        # the same frame as an already pooled volume (+ the geometry tensor the render block then reads)
        vt, f = model.img_view_transformer, frames[1]
        vol = vt.lift_splat(f["depth"], f["ctx"], cams=f["cams"]).contiguous()
        pooled = dict(img_voxel_feats=vol, img_feats=f["img_feats"], transform=f["transform"], gemo=vt.get_geometry(*f["cams"]))
        (g, _), = serve(model, [pooled], (0,), render=True)
    same(ref[1], g, "pooled volume")


def test_lidar_only_as_configured_has_no_fine_branch(dev):
    model = lidar_model(dev)
    frames = [lidar_frame(dev, 50), lidar_frame(dev, 51)]
    with torch.no_grad():
        ref = [model.forward_hot_path(None, f["pts"]) for f in frames]
        assert all(r["pred_f"] is None for r in ref)
        ref = [grab(r) for r in ref]
        torch.cuda.synchronize()
        got = serve(model, frames, (0, 1, 0))
    for (g, cnt), i in zip(got, (0, 1, 0)):
        assert cnt is None and "pred_f" not in g
        same(ref[i], g, "frame %d" % i)
    assert not torch.equal(ref[0]["pred_c"], ref[1]["pred_c"])


def _result(res):
    d = {k: res[k].clone() for k in ("pred_c", "pred_f", "output_voxels") if res.get(k) is not None}
    d.update({k: torch.as_tensor(res[k]).clone() for k in res if k.startswith(("SC_metric", "SSC_metric"))})
    if res.get("output_voxels_fine") is not None:
        d["fine"], d["fine_xyz"] = res["output_voxels_fine"][0].clone(), res["output_coords_fine"][0].reshape(3, -1).clone()
    return d


def _case(dev, which):
    """(model, four ``precomputed`` dicts) of the models of the first and the third test."""
    if which == "camera":
        cam = camera_model(dev, (50, 50, 4), render=False)
        return cam, [dict(camera_frame(cam, dev, 4200 + 13 * i)) for i in range(4)]
    return lidar_model(dev), [dict(pts_voxel_feats=lidar_frame(dev, 60 + i)["pts"]) for i in range(4)]


@pytest.mark.parametrize("which", ["camera", "lidar"])
def test_simple_test_takes_the_captured_route(dev, which):
    name, (model, pcs) = which, _case(dev, which)
    gt = torch.randint(0, 17, (1, 100, 100, 8), generator=torch.Generator().manual_seed(5)).to(dev)
    with torch.no_grad():
        model.graph_simple_test = False
        ref = _result(model.simple_test(precomputed=pcs[0], gt_occ=gt))
        assert model._pipe1 is None
        model.graph_simple_test = True
        got = _result(model.simple_test(precomputed=pcs[0], gt_occ=gt))
    assert model._pipe1 is not None and model.graph_unavailable is None, model.graph_unavailable
    same(ref, got, name)
    assert int(ref["SSC_metric"].sum()) > 0


@pytest.mark.parametrize("which", ["camera", "lidar"])
def test_pipelined_test_equals_per_sample_calls(dev, which):
    from co_occ_amd import apis
    name, (model, pcs) = which, _case(dev, which)
    # 100 x 100 x 8: the camera model's fine grid.  The LiDAR-only model has no fine branch, so no ground-truth grid sends a sample
    # to the eager decode: its last sample carries a 200 x 200 x 16 one (the metrics kernel resamples pred_c)
    g = torch.Generator().manual_seed(6)
    sizes = [(100, 100, 8)] * 3 + [(200, 200, 16) if which == "lidar" else (100, 100, 8)]
    data = [dict(precomputed=pc, gt_occ=torch.randint(0, 17, (1,) + s, generator=g).to(dev)) for pc, s in zip(pcs, sizes)]
    with torch.no_grad():
        model.graph_simple_test = False
        ref = [_result(model.simple_test(**d)) for d in data]
        model.graph_simple_test = True
    stats, n = {}, 0
    for i, (d, res) in enumerate(apis.pipelined_test(model, iter(data), slots=3, dense_streams=2, stats=stats)):
        assert d is data[i]
        same(ref[i], _result(res), "%s sample %d" % (name, i))
        n += 1
    assert n == 4 and stats["fallbacks"] == 0 and stats["eager_samples"] == 0, stats


def test_weight_change_recaptures_the_camera_only_pipeline(dev):
    model = camera_model(dev, (50, 50, 4), render=False)
    frames = [camera_frame(model, dev, 4300)]
    pipe = model.serving(frames[0], slots=2, dense_streams=1, render=False)
    try:
        with torch.no_grad():
            before = grab(pipe.submit(frames[0], copy=True).result())
            model.pts_bbox_head.occ_pred_conv[3].weight.mul_(1.5)
            want = grab(eager_camera(model, frames[0], False))
            torch.cuda.synchronize()
            out = pipe.submit(frames[0]).result()
            after = grab(out, int(out["fine_count"].item()) * 8)
        assert pipe.recaptures == 1
        same(want, after, "after the edit")
        assert not torch.equal(before["pred_c"], after["pred_c"])
    finally:
        pipe.close()
