"""Serving the models without a fuser, the parts that need no GPU: which slot a model gets and its shapes, which frame forms a
model takes, and that the measuring tool refuses to run without a GPU."""
import importlib.util
import os

import pytest
import torch

from conftest import ROOT
import co_occ_amd as pkg
from co_occ_amd import core, graph, serving, synth
from co_occ_amd.fuser import SearchSlot


@pytest.fixture(scope="module")
def models():
    cam = synth.model_cfg(rendering=False)
    cam.update(occ_fuser=None, external_encoders=True)
    return dict(camera=pkg.build_detector(cam).eval(), lidar=pkg.build_detector(synth.model_cfg_lidar(), external_encoders=True).eval(),
                fused=pkg.build_detector(synth.model_cfg(C=64, rendering=False), external_encoders=True).eval())


def test_voxel_slot_is_one_rows_buffer():
    s = graph.VoxelSlot(128, (5, 3, 2), "cpu")
    assert (s.grid, s.C, s.V) == ((5, 3, 2), 128, 30) and tuple(s.t.shape) == (30, 128) and s.t.dtype == torch.float32
    assert s.device == torch.device("cpu") and not hasattr(s, "counts") and not hasattr(s, "cat4")
    r = s.rows()
    assert isinstance(r, core.Rows) and r.persistent and (r.B, r.X, r.Y, r.Z, r.C, r.coff, r.stride) == (1, 5, 3, 2, 128, 0, 128)
    assert r.t.data_ptr() == s.t.data_ptr() and s.rows() is not r            # a fresh Rows per call, the same static buffer
    v = r.as_ncdhw()
    assert tuple(v.shape) == (1, 128, 5, 3, 2) and v.data_ptr() == s.t.data_ptr()
    s.t[7, 3] = 2.5                                                         # row (x, y, z) = (1, 0, 1)
    assert float(v[0, 3, 1, 0, 1]) == 2.5
    for bad in ((0, 3, 2), (5, 3, -1)):
        with pytest.raises(ValueError):
            graph.VoxelSlot(128, bad, "cpu")
    with pytest.raises(ValueError):
        graph.VoxelSlot(0, (5, 3, 2), "cpu")


def test_make_slot_follows_the_model(models):
    cam = graph.make_slot(models["camera"], (4, 4, 2), "cpu")
    assert isinstance(cam, graph.VoxelSlot) and cam.C == models["camera"].img_view_transformer.numC_Trans == 128
    vol = torch.zeros(1, 96, 4, 4, 2)
    lid = graph.make_slot(models["lidar"], (4, 4, 2), "cpu", example=dict(pts=vol))
    assert isinstance(lid, graph.VoxelSlot) and (lid.C, lid.V) == (96, 32)
    with pytest.raises(ValueError, match="LiDAR volume"):
        graph.make_slot(models["lidar"], (4, 4, 2), "cpu")
    fused = graph.make_slot(models["fused"], (4, 4, 2), "cpu")
    assert isinstance(fused, SearchSlot) and fused.C == 64 and tuple(fused.cat4.shape) == (32, 256)
    assert fused.device == cam.device == torch.device("cpu")               # what DenseGraph.capture asks either slot for


def test_fill_volume_checks_the_shape():
    s = graph.VoxelSlot(8, (2, 2, 2), "cpu")
    with pytest.raises(ValueError, match="fill_volume"):
        graph.fill_volume(s, torch.zeros(1, 8, 2, 2, 3))
    vol = torch.arange(64, dtype=torch.float32).view(1, 2, 2, 2, 8).permute(0, 4, 1, 2, 3)       # channels-last already: one flat copy
    graph.fill_volume(s, vol)
    assert torch.equal(s.rows().as_ncdhw(), vol)


def test_frame_forms(models):
    t = torch.zeros(1)
    lifted, pooled = dict(depth=t, ctx=t, cams=(t,) * 6, img_feats=[t], transform=(t,)), dict(img_voxel_feats=t, img_feats=[t], transform=(t,))
    cam, lid, fused = models["camera"], models["lidar"], models["fused"]
    assert serving.check_frame(cam, lifted) == serving.check_frame(cam, pooled) == serving.check_frame(cam, dict(pooled, gemo=t)) == "camera"
    assert serving.check_frame(lid, dict(pts=t)) == serving.check_frame(lid, dict(points=t)) == "lidar"
    assert serving.check_frame(fused, dict(lifted, pts=t)) == serving.check_frame(fused, dict(pooled, points=t)) == "fused"
    # keys that are present and None count as absent (``serving_frame`` fills every key)
    assert serving.check_frame(lid, dict(pts=t, depth=None, img_voxel_feats=None, img_feats=None, transform=None)) == "lidar"
    for model, fr, why in ((cam, dict(lifted, pts=t), "both"), (cam, dict(img_feats=[t]), "neither"), (lid, {}, "neither"),
                           (cam, dict(depth=t, ctx=t), "cams"), (cam, dict(depth=t, cams=(t,) * 6), "ctx"),
                           (lid, lifted, "view transformer"), (fused, lifted, "LiDAR"), (fused, dict(pts=t), "camera")):
        with pytest.raises(ValueError, match=why):
            serving.check_frame(model, fr)


def test_serving_frame_needs_neither_points_nor_images(models):
    t = torch.zeros(1)
    fr = models["lidar"].serving_frame(precomputed=dict(pts_voxel_feats=t))
    assert fr["pts"] is t and fr["img_feats"] is None and fr["transform"] is None and fr["cams"] is None
    fr = models["camera"].serving_frame(precomputed=dict(img_voxel_feats=t, img_feats=[t], transform=(t,) * 7))
    assert fr["pts"] is None and fr["img_voxel_feats"] is t and len(fr["cams"]) == 6


def test_heads_say_whether_they_have_a_fine_branch(models):
    assert models["camera"].pts_bbox_head.has_fine_branch and not models["lidar"].pts_bbox_head.has_fine_branch


def test_tool_refuses_without_a_gpu_and_writes_nothing(tmp_path, monkeypatch):
    spec = importlib.util.spec_from_file_location("bench_single_modality", os.path.join(ROOT, "tools", "bench_single_modality.py"))
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    out = tmp_path / "single.json"
    with pytest.raises(SystemExit) as e:
        tool.main(["--windows", "1", "--out", str(out)])
    assert "no GPU" in str(e.value) and not out.exists()
    s = tool.spread([3.0, 1.0, 2.0])
    assert (s["median"], s["min"], s["max"], s["n"]) == (2.0, 1.0, 3.0, 3)
