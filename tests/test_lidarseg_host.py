"""Host half of the lidarseg feature (points_occ): the metric helpers against the fixture made by the unmodified reference
(tools/gen_golden_lidarseg.py -> tests/golden/lidarseg.npz), the nuScenes lidarseg submission writer, and the C-ABI entry point
(declared, exported, validating its arguments before any launch).  No GPU needed."""
import ctypes
import json
import os

import numpy as np
import pytest

from co_occ_amd import _lib, apis, evaluation as E


def golden_probs(g, case):
    """The fixture's probabilities of case (a), or of case (b): (a)'s with the rows zeros padding changes replaced."""
    if case == "a":
        return g["a_probs"]
    b = g["a_probs"].copy()
    b[g["b_probs_rows"]] = g["b_probs_at_rows"]
    return b


def _target_eval(points):
    return points[:, 3].astype(int)                  # coocc_ray.py:697: gt[:, 3].astype(np.int)


@pytest.mark.parametrize("case", ["a", "b"])
def test_fast_hist_crop_reproduces_the_reference_eval_matrix(golden, case):
    g = golden("lidarseg")
    hist = E.fast_hist_crop(g[case + "_labels"], _target_eval(g["a_points"]), np.arange(16))
    assert hist.shape == (16, 16) and hist.dtype == np.int64
    assert np.array_equal(hist, g[case + "_hist"])
    assert hist.sum() > 1000                         # the fixture's labels include 0, 17, 255 and -1: those rows are dropped
    # the labels are argmax(probs[:, 1:]) + 1 of the stored probabilities
    assert np.array_equal(np.argmax(golden_probs(g, case)[:, 1:], axis=1) + 1, g[case + "_labels"])


def test_per_class_iu_and_point_mean_iou_reproduce_the_reference_train_metric(golden):
    g = golden("lidarseg")
    target = np.concatenate([g["c_points0"][:, -1], g["c_points1"][:, -1]]).astype(np.int64)
    hist = E.fast_hist_crop(g["c_labels"], target, np.arange(16))
    assert np.array_equal(hist, g["c_hist"])
    with np.errstate(divide="ignore", invalid="ignore"):
        miou = np.nanmean(E.per_class_iu(hist))
    assert abs(miou - float(g["c_point_mean_iou"])) <= 1e-12
    # the torch restatement used on the device gives the same number on the host
    import torch
    dev_form = E.point_mean_iou(torch.from_numpy(hist))
    assert dev_form.dtype == torch.float64 and dev_form.dim() == 0
    assert abs(float(dev_form) - float(g["c_point_mean_iou"])) <= 1e-12


def test_lidarseg_metrics_host_half(golden):
    g = golden("lidarseg")
    m = E.lidarseg_metrics(g["a_hist"] + g["b_hist"])
    assert np.array_equal(m["hist"], g["a_hist"] + g["b_hist"])
    assert len(m["class_ious"]) == 16
    with np.errstate(divide="ignore", invalid="ignore"):
        assert m["mIoU"] == float(np.nanmean(E.per_class_iu(g["a_hist"] + g["b_hist"])))
    assert np.isnan(E.lidarseg_metrics(np.zeros((16, 16), np.int64))["mIoU"])


def test_save_nuscenes_lidarseg_submission_writes_the_reference_files(tmp_path):
    import torch
    labels = torch.tensor([1, 16, 3, 255 + 1, 7], dtype=torch.int64)      # 256 wraps to 0 in uint8, as numpy's astype does
    f = apis.save_nuscenes_lidarseg_submission(labels, str(tmp_path), dict(lidar_token="abc123"))
    assert f == os.path.join(str(tmp_path), "lidarseg", "test", "abc123_lidarseg.bin")
    assert np.array_equal(np.fromfile(f, dtype=np.uint8), np.array([1, 16, 3, 0, 7], np.uint8))
    meta = json.load(open(os.path.join(str(tmp_path), "test", "submission.json")))
    assert meta == {"meta": {"use_lidar": False, "use_camera": True, "use_radar": False, "use_map": False, "use_external": False}}
    # a second sample adds its .bin and leaves the meta file as it is
    apis.save_nuscenes_lidarseg_submission(np.array([2, 2]), str(tmp_path), dict(lidar_token="def"))
    assert sorted(os.listdir(os.path.join(str(tmp_path), "lidarseg", "test"))) == ["abc123_lidarseg.bin", "def_lidarseg.bin"]
    assert os.path.getsize(os.path.join(str(tmp_path), "lidarseg", "test", "def_lidarseg.bin")) == 2


def test_lidarseg_entry_point_is_declared_exported_and_validates_before_launching():
    assert "coocc_lidarseg_points" in _lib.SIGNATURES
    src = open(os.path.join(os.path.dirname(_lib.__file__), "..", "include", "coocc_hip.h")).read()
    assert "int coocc_lidarseg_points(" in src
    lib = _lib.load()
    fn = lib.coocc_lidarseg_points
    one = ctypes.c_void_p(16)              # a non-null dummy address: validation never dereferences device pointers
    rng = (ctypes.c_float * 6)(-40, -40, -1, 40, 40, 5.4)

    def call(C=17, n=10, stride=4, cols=4, label_col=3, pad=1, mode=0, probs=None, hist=one):
        return fn(one, 1, 17, 17 * 20, 17 * 400, C, 20, 20, 4, one, n, stride, cols, label_col, rng, pad, mode, probs, one, 0,
                  hist, None)
    for kw, word in ((dict(C=16), b"C == 17"), (dict(C=33), b"C <= 32"), (dict(pad=2), b"padding_mode"), (dict(mode=2), b"mode"),
                     (dict(cols=2, stride=2), b"point_cols"), (dict(label_col=4), b"label_col"), (dict(mode=1, probs=one), b"eval-mode")):
        assert call(**kw) == -1, kw
        assert word in lib.coocc_last_error(), (kw, lib.coocc_last_error())


def test_reflection_padding_is_rejected():
    import torch
    from co_occ_amd.head import OccHead
    head = OccHead(in_channels=[64], out_channel=17, norm_cfg=dict(type='BN3d'), padding_mode='reflection').eval()
    with pytest.raises(NotImplementedError):
        head.forward_lidarseg(torch.zeros(1, 17, 4, 4, 2), [torch.zeros(3, 4)])
