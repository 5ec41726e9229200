"""Host half of ``SparseEncoderHD`` training (``lidar_hd``'s differentiable forward, the detectors' ``train_sparse_encoder_hd``
option): the option is opt-in and leaves defaults and state_dicts alone, the new entry points are declared, exported, bound and
validate before launching, and the float64 training-mode restatement the GPU tests are judged by (tests/ref_sparse_hd_train.py) is
itself checked -- against the eval-mode restatement, against torch's BatchNorm1d, and by finite differences.  No GPU needed."""
import ctypes
import os
import re
import sys
import types

import numpy as np
import pytest
import torch

import co_occ_amd as pkg
import co_occ_amd.synth as synth
from co_occ_amd import _lib, lidar_hd, registry
from co_occ_amd.lidar_hd import SparseEncoderHD

from conftest import ROOT
import ref_sparse_hd as R
import ref_sparse_hd_train as RT

NEW = ("coocc_sparse_dgrad_table3", "coocc_bn_apply_ex")
SMALL = dict(in_channels=4, sparse_shape=[5, 5, 5], base_channels=4, output_channels=8, encoder_channels=((4,), (8, 8)),
             encoder_paddings=((1,), ((0, 1, 1), 1)), encoder_strides=(2, 2), block_type='conv_module')


# ----------------------------------------------------------------------------- the option
def test_default_module_and_detector_are_unchanged():
    m = SparseEncoderHD(in_channels=4, sparse_shape=[21, 21, 27])
    assert m.train_enabled is False
    with pytest.raises(NotImplementedError, match=r"train\(\) forward"):
        m.train()(torch.zeros(2, 4), torch.zeros(2, 3, dtype=torch.int32), 1)
    det = pkg.build_detector(synth.model_cfg_lidar(), sparse_encoder_hd=True)
    assert det.train_sparse_encoder_hd is False and det.pts_middle_encoder.train_enabled is False
    with pytest.raises(NotImplementedError, match=r"train\(\) forward"):
        det.pts_middle_encoder.train()(torch.zeros(2, 4), torch.zeros(2, 3, dtype=torch.int32), 1)
    with pytest.raises(NotImplementedError, match="SyncBN"):
        SparseEncoderHD(in_channels=4, sparse_shape=[21, 21, 27], norm_cfg=dict(type='SyncBN', eps=1e-3, momentum=0.01))


def test_the_key_is_accepted_and_changes_no_state_dict():
    plain = pkg.build_detector(synth.model_cfg_lidar(), sparse_encoder_hd=True)
    det = pkg.build_detector(synth.model_cfg_lidar(), sparse_encoder_hd=True, train_sparse_encoder_hd=True, train_lidar_trunk=True)
    assert isinstance(det, pkg.COOCC_Ray_L) and det.train_sparse_encoder_hd and det.pts_middle_encoder.train_enabled is True
    assert "train_sparse_encoder_hd" not in det.ignored_cfg_keys
    assert list(det.state_dict()) == list(plain.state_dict())
    assert {k: tuple(v.shape) for k, v in det.state_dict().items()} == {k: tuple(v.shape) for k, v in plain.state_dict().items()}
    # as a config key
    cfg = dict(synth.model_cfg_lidar(), sparse_encoder_hd=True, train_sparse_encoder_hd=True)
    assert pkg.build_detector(cfg).pts_middle_encoder.train_enabled is True
    # the fusion detector takes the key and has no such encoder
    fus = pkg.build_detector(synth.model_cfg(), external_encoders=True, train_sparse_encoder_hd=True)
    assert type(fus).__name__ == "COOCC_Ray" and fus.train_sparse_encoder_hd and "train_sparse_encoder_hd" not in fus.ignored_cfg_keys
    # CPU tensors are refused by the training path as by inference: no fallback
    enc = det.pts_middle_encoder.train()
    with pytest.raises(_lib.CooccError, match="GPU only"):
        enc(torch.zeros(2, 4), torch.zeros(2, 3, dtype=torch.int32), 1)
    with pytest.raises(NotImplementedError, match="batch size"):
        enc(torch.zeros(2, 4), torch.zeros(2, 3, dtype=torch.int32), 2)


class _FakeRegistry:
    def __init__(self):
        self.module_dict = {}

    def register_module(self, name=None, force=False, module=None):
        self.module_dict[name] = module
        return module


def test_register_into_mmdet_takes_the_key(monkeypatch):
    mb, m3b = types.ModuleType("mmdet.models.builder"), types.ModuleType("mmdet3d.models.builder")
    mb.DETECTORS = _FakeRegistry()
    for n in ("BACKBONES", "NECKS", "HEADS", "FUSION_LAYERS", "VOXEL_ENCODERS", "MIDDLE_ENCODERS"):
        setattr(m3b, n, _FakeRegistry())
    for name, mod in (("mmdet", types.ModuleType("mmdet")), ("mmdet.models", types.ModuleType("mmdet.models")),
                      ("mmdet.models.builder", mb), ("mmdet3d", types.ModuleType("mmdet3d")),
                      ("mmdet3d.models", types.ModuleType("mmdet3d.models")), ("mmdet3d.models.builder", m3b)):
        monkeypatch.setitem(sys.modules, name, mod)
    sys.modules["mmdet.models"].builder = mb
    sys.modules["mmdet3d.models"].builder = m3b
    with pytest.raises(ValueError, match="sparse_encoder_hd=True"):
        pkg.register_into_mmdet(train_sparse_encoder_hd=True)
    assert pkg.register_into_mmdet(detectors=True, sparse_encoder_hd=True, train_sparse_encoder_hd=True) is True
    enc_cls = m3b.MIDDLE_ENCODERS.module_dict["SparseEncoderHD"]
    assert enc_cls.__name__ == "SparseEncoderHD" and issubclass(enc_cls, SparseEncoderHD)
    enc = enc_cls(in_channels=4, sparse_shape=[21, 21, 27])
    assert enc.train_enabled is True and list(enc.state_dict()) == list(SparseEncoderHD(in_channels=4, sparse_shape=[21, 21, 27]).state_dict())
    det_cls = mb.DETECTORS.module_dict["COOCC_Ray_L"]
    cfg = {k: v for k, v in synth.model_cfg_lidar().items() if k != "type"}
    det = det_cls(sparse_encoder_hd=True, **cfg)
    assert det.train_sparse_encoder_hd and not det.train_lidar_trunk and det.pts_middle_encoder.train_enabled
    assert not det_cls(sparse_encoder_hd=True, train_sparse_encoder_hd=False, **cfg).pts_middle_encoder.train_enabled
    both = registry.trunk_training_detector(True, True)(sparse_encoder_hd=True, **cfg)
    assert both.train_lidar_trunk and both.train_sparse_encoder_hd


# ----------------------------------------------------------------------------- the C entry points
def test_new_entry_points_are_declared_exported_and_bound():
    hdr = open(os.path.join(ROOT, "include", "coocc_hip.h")).read()
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for name in NEW:
        assert re.search(r"\bint\s+%s\s*\(" % name, hdr), "not declared: " + name
        assert hasattr(lib, name), "not exported: " + name
        assert name in _lib.SIGNATURES, "not in the ctypes table: " + name
    assert len(_lib.SIGNATURES["coocc_sparse_dgrad_table3"][1]) == 21 and len(_lib.SIGNATURES["coocc_bn_apply_ex"][1]) == 13
    assert "sparse_train.hip" in __import__("co_occ_amd.build", fromlist=["sources"]).sources()


def test_new_entry_points_validate_before_launching():
    lib = _lib.load()
    one = ctypes.c_void_p(16)
    k3, s2, p011 = (3, 3, 3), (2, 2, 2), (0, 1, 1)
    ok = (2, 4, 4)                                     # (6 + 0 - 3) / 2 + 1, (7 + 2 - 3) / 2 + 1 twice
    assert lib.coocc_sparse_dgrad_table3(one, 4, 6, 7, 7, *k3, *s2, *p011, *ok, None, one, None, None) == -1       # no index map
    assert b"sparse_dgrad_table3" in lib.coocc_last_error()
    assert lib.coocc_sparse_dgrad_table3(None, 4, 6, 7, 7, *k3, *s2, *p011, *ok, one, one, None, None) == -1
    assert lib.coocc_sparse_dgrad_table3(one, -1, 6, 7, 7, *k3, *s2, *p011, *ok, one, one, None, None) == -1
    assert lib.coocc_sparse_dgrad_table3(one, 4, 6, 7, 7, 3, 0, 3, *s2, *p011, *ok, one, one, None, None) == -1 and b"kernel" in lib.coocc_last_error()
    assert lib.coocc_sparse_dgrad_table3(one, 4, 6, 7, 7, *k3, 2, 2, 0, *p011, *ok, one, one, None, None) == -1 and b"stride" in lib.coocc_last_error()
    assert lib.coocc_sparse_dgrad_table3(one, 4, 6, 7, 7, *k3, *s2, *p011, 3, 4, 4, one, one, None, None) == -1 and b"output grid" in lib.coocc_last_error()
    assert lib.coocc_sparse_dgrad_table3(one, 4, 65, 8000, 8000, *k3, *s2, *p011, 32, 4000, 4000, one, one, None, None) == -1
    assert b"2^31" in lib.coocc_last_error()
    assert lib.coocc_sparse_dgrad_table3(None, 0, 6, 7, 7, *k3, *s2, *p011, *ok, one, None, None, None) == 0       # no rows: nothing to launch
    f = 1e-3
    assert lib.coocc_bn_apply_ex(one, 0, 32, one, one, one, one, f, None, 1, one, None, None) == -1 and b"bn_apply_ex" in lib.coocc_last_error()
    assert lib.coocc_bn_apply_ex(one, 8, 30, one, one, one, one, f, None, 1, one, None, None) == -1                # C % 4
    assert lib.coocc_bn_apply_ex(one, 8, 16, one, one, one, one, f, None, 1, one, one, None) == -1 and b"twin" in lib.coocc_last_error()
    assert lib.coocc_bn_apply_ex(ctypes.c_void_p(20), 8, 32, one, one, one, one, f, None, 1, one, None, None) == -1 and b"aligned" in lib.coocc_last_error()


def test_live_taps_of_a_residue_class():
    k3 = (3, 3, 3)
    sizes = sorted(len(lidar_hd.class_taps(c, k3, (2, 2, 2))) for c in range(8))
    assert sizes == [1, 2, 2, 2, 4, 4, 4, 8] and sum(sizes) == 27
    assert lidar_hd.class_taps(0, k3, (2, 2, 2)) == [0, 2, 6, 8, 18, 20, 24, 26] and lidar_hd.class_taps(7, k3, (2, 2, 2)) == [13]
    assert lidar_hd.class_taps(0, k3, (1, 1, 1)) == list(range(27))
    assert lidar_hd.class_taps(3, k3, (1, 4, 4)) == [] and len(lidar_hd.class_taps(1 * 4 + 2, k3, (1, 4, 4))) == 3      # rx = 3: no tap


# ----------------------------------------------------------------------------- the judge itself
def _small_case(cfg, n, seed):
    m = SparseEncoderHD(**cfg)
    sd = synth.random_state_dict(m.state_dict(), seed=seed)
    coors = R.random_voxels(tuple(cfg["sparse_shape"]), n, seed)
    g = torch.Generator().manual_seed(seed)
    return sd, coors, torch.randn(len(coors), cfg["in_channels"], generator=g, dtype=torch.float64), m.out_shape(), g


@pytest.mark.parametrize("kind", ["conv_module", "basicblock"])
def test_training_restatement_with_its_batch_statistics_frozen_is_the_eval_restatement(kind):
    """One large batch at momentum 1: the running statistics BECOME the batch statistics (the variance with Bessel's n / (n - 1),
    which is undone here with the recorded row counts), and ``ref_sparse_hd.encoder_forward`` -- eval mode -- on them must then
    reproduce the training-mode output."""
    cfg = dict(in_channels=4, sparse_shape=[21, 21, 27]) if kind == "conv_module" else \
        dict({k: v for k, v in synth.model_cfg_lidar()["pts_middle_encoder"].items() if k != "type"}, sparse_shape=[21, 21, 27])
    sd, coors, feats, _, _ = _small_case(cfg, 1500, 21)
    sd64 = {k: v.double() if v.is_floating_point() else v for k, v in sd.items()}
    with torch.no_grad():
        y, mask, stats, counts = RT.encoder_forward_train(sd64, cfg, feats, coors, momentum=1.0)
    assert min(counts.values()) >= 2 and set(stats) == {k for k in sd if "running" in k or "num_batches" in k}
    frozen = dict(sd64)
    for k, v in stats.items():
        n = counts[k.rsplit(".", 1)[0]]
        frozen[k] = v * ((n - 1) / n) if k.endswith("running_var") else v
        if k.endswith("num_batches_tracked"):
            assert int(v) == int(sd[k]) + 1
    want, wmask = R.encoder_forward(frozen, cfg, feats, coors)
    assert torch.equal(mask, wmask) and float((y - want).abs().max()) <= 1e-9 * max(1.0, float(want.abs().max()))


def test_training_restatement_normalises_like_torch_batchnorm1d():
    """The first layer's norm against nn.BatchNorm1d.train() on the active rows: output and the running update at momentum 0.01."""
    g = torch.Generator().manual_seed(3)
    coors = R.random_voxels((5, 6, 7), 60, 3)
    rows = torch.randn(60, 8, generator=g, dtype=torch.float64) * 3 + 1
    bn = torch.nn.BatchNorm1d(8, eps=1e-3, momentum=0.01).double().train()
    with torch.no_grad():
        bn.weight.copy_(torch.rand(8, generator=g) + 0.5), bn.bias.copy_(torch.randn(8, generator=g))
        bn.running_mean.copy_(torch.randn(8, generator=g)), bn.running_var.copy_(torch.rand(8, generator=g) + 0.5)
    sd = {"n." + k: v.detach().clone() for k, v in bn.state_dict().items()}
    x, mask = R.to_dense(rows, coors, (5, 6, 7))
    stats, counts = {}, {}
    with torch.no_grad():
        y = RT.bn_rows_train(x, mask, sd, "n", 1e-3, 0.01, stats, counts)
        want = bn(rows)
    c = torch.as_tensor(coors).long()
    assert counts["n"] == 60 and float((y[0, :, c[:, 0], c[:, 1], c[:, 2]].t() - want).abs().max()) < 1e-12
    assert float(y.abs().sum() - y[0, :, c[:, 0], c[:, 1], c[:, 2]].abs().sum()) == 0.0
    assert float((stats["n.running_mean"] - bn.running_mean).abs().max()) < 1e-14
    assert float((stats["n.running_var"] - bn.running_var).abs().max()) < 1e-14 and int(stats["n.num_batches_tracked"]) == 1


def test_training_restatement_gradients_against_finite_differences():
    """The judge's own gradients: central differences of the float64 loss on a 5 x 5 x 5 grid with 40 voxels, a down-convolution
    with (0,1,1) padding included; every input feature and a sample of every parameter."""
    cfg = SMALL
    sd, coors, feats, oshape, g = _small_case(cfg, 40, 8)
    gout = torch.randn(1, cfg["output_channels"], *oshape, generator=g, dtype=torch.float64)
    r = RT.evaluate(sd, cfg, feats, coors, gout, torch.float64)
    assert sorted(set(r["counts"].values()))[0] >= 4, r["counts"]
    sd64 = {k: v.double() if v.is_floating_point() else v for k, v in sd.items()}

    def loss(over=None, f=feats):
        with torch.no_grad():
            return float((RT.encoder_forward_train(dict(sd64, **(over or {})), cfg, f, coors)[0] * gout).sum())
    h = 1e-6
    worst = 0.0
    rs = np.random.RandomState(0)
    for i, j in zip(rs.randint(0, len(coors), 12), rs.randint(0, 4, 12)):
        d = torch.zeros_like(feats)
        d[i, j] = h
        fd = (loss(f=feats + d) - loss(f=feats - d)) / (2 * h)
        worst = max(worst, abs(fd - float(r["dfeats"][i, j])) / max(1.0, abs(fd)))
    for k, v in sd64.items():
        if k + ".grad" not in r:
            continue
        flat = v.reshape(-1)
        for idx in rs.randint(0, flat.numel(), 3):
            d = torch.zeros_like(flat)
            d[idx] = h
            fd = (loss({k: (flat + d).view_as(v)}) - loss({k: (flat - d).view_as(v)})) / (2 * h)
            worst = max(worst, abs(fd - float(r[k + ".grad"].reshape(-1)[idx])) / max(1.0, abs(fd)))
    print("[sparse_hd train] finite differences: worst relative deviation %.3e" % worst)
    assert worst <= 1e-6
