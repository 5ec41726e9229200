"""Host half of LiDAR-trunk training (``lidar_trunk.run_trunk_train``, the detector's ``train_lidar_trunk`` option): the option
builds and leaves the state_dict alone, the default-built detector still refuses, CPU tensors are refused, and the two new entry
points are declared, exported, bound and validate their arguments before launching.  No GPU needed."""
import ctypes
import os
import re

import pytest
import torch

import co_occ_amd as pkg
from co_occ_amd import _lib, lidar_trunk as lt, registry, synth

from conftest import ROOT

NEW = ("coocc_conv_tap_table3", "coocc_fpn_sum_bwd")


def test_detector_builds_with_the_option_and_keeps_its_state_dict_keys():
    plain = pkg.build_detector(synth.model_cfg_lidar(), external_encoders=True)
    det = pkg.build_detector(synth.model_cfg_lidar(), external_encoders=True, train_lidar_trunk=True)
    assert isinstance(det, pkg.COOCC_Ray_L) and det.train_lidar_trunk and not plain.train_lidar_trunk
    assert list(det.state_dict()) == list(plain.state_dict())
    assert {k: tuple(v.shape) for k, v in det.state_dict().items()} == {k: tuple(v.shape) for k, v in plain.state_dict().items()}
    # the fusion detector takes the key and has no such trunk to train
    fus = pkg.build_detector(synth.model_cfg(), external_encoders=True, train_lidar_trunk=True)
    assert type(fus).__name__ == "COOCC_Ray" and fus.train_lidar_trunk and "train_lidar_trunk" not in fus.ignored_cfg_keys
    # the class register_into_mmdet(detectors=True, train_lidar_trunk=True) writes under the reference name: the option on by default
    cls = registry.trunk_training_detector()
    assert cls.__name__ == "COOCC_Ray_L" and issubclass(cls, pkg.COOCC_Ray_L)
    cfg = {k: v for k, v in synth.model_cfg_lidar().items() if k != "type"}
    assert cls(external_encoders=True, **cfg).train_lidar_trunk and not cls(external_encoders=True, train_lidar_trunk=False, **cfg).train_lidar_trunk
    with pytest.raises(ValueError, match="detectors=True"):
        registry.register_into_mmdet(train_lidar_trunk=True)


def test_default_detector_still_refuses_middle_feats_in_forward_train():
    det = pkg.build_detector(synth.model_cfg_lidar(), external_encoders=True).train()
    with pytest.raises(NotImplementedError, match="pts_middle_feats"):
        det.forward_train(precomputed=dict(pts_middle_feats=synth.second3d_input((2, 8, 8))))
    # with the option on the call gets as far as the trunk, which has no CPU path
    det = pkg.build_detector(synth.model_cfg_lidar(), external_encoders=True, train_lidar_trunk=True).train()
    with pytest.raises(_lib.CooccError, match="GPU only"):
        det.forward_train(precomputed=dict(pts_middle_feats=synth.second3d_input((2, 8, 8))))


def test_run_trunk_train_refuses_cpu_tensors_and_module_forwards_still_refuse_train():
    bcfg, ncfg = synth.second3d_cfg((1, 1, 1))
    b, n = registry.BACKBONES.build(bcfg).train(), registry.NECKS.build(ncfg).train()
    x = synth.second3d_input((2, 8, 8))
    with pytest.raises(_lib.CooccError, match="GPU only"):
        lt.run_trunk_train(b, n, x)
    with pytest.raises(_lib.CooccError, match="GPU only"):
        lt.run_trunk_train(b, n, x.requires_grad_())
    with pytest.raises(ValueError, match="B,C,Z,Y,X"):
        lt.run_trunk_train(b, n, torch.zeros(4, 4))
    with pytest.raises(NotImplementedError, match="train"):
        b(x)
    with pytest.raises(NotImplementedError, match="train"):
        n([x])


def test_new_entry_points_are_declared_exported_and_bound():
    hdr = open(os.path.join(ROOT, "include", "coocc_hip.h")).read()
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for name in NEW:
        assert re.search(r"\bint\s+%s\s*\(" % name, hdr), "not declared: " + name
        assert hasattr(lib, name), "not exported: " + name
        assert name in _lib.SIGNATURES, "not in the ctypes table: " + name
    assert len(_lib.SIGNATURES["coocc_conv_tap_table3"][1]) == 19 and len(_lib.SIGNATURES["coocc_fpn_sum_bwd"][1]) == 11
    assert "trunk_train.hip" in __import__("co_occ_amd.build", fromlist=["sources"]).sources()


def test_new_entry_points_validate_before_launching():
    lib = _lib.load()
    one = ctypes.c_void_p(16)
    # output extents that are not (n + 2p - k)/s + 1: (9 + 2 - 3)/4 + 1 = 3, not 2
    assert lib.coocc_conv_tap_table3(1, 9, 7, 2, 2, 2, 2, 3, 3, 1, 4, 4, 1, 1, 1, 0, 0, one, None) == -1
    assert b"conv_tap_table3" in lib.coocc_last_error() and b"extents" in lib.coocc_last_error()
    assert lib.coocc_conv_tap_table3(1, 9, 7, 2, 3, 2, 2, 3, 3, 1, 4, 4, 0, 1, 1, 0, 0, one, None) == -1          # stride 0
    assert lib.coocc_conv_tap_table3(1, 9, 7, 2, 3, 2, 2, 3, 3, 1, 4, 4, 1, 1, 1, 0, 1, None, None) == -1          # no table
    dups = (ctypes.c_void_p * 4)(None, 32, 48, 0)
    assert lib.coocc_fpn_sum_bwd(one, 128, dups, (ctypes.c_int * 4)(1, 2, 3, 0), 3, 1, 8, 8, 2, 128, None) == -1
    assert b"strides" in lib.coocc_last_error()
    assert lib.coocc_fpn_sum_bwd(one, 128, dups, (ctypes.c_int * 4)(1, 2, 4, 0), 3, 1, 6, 8, 2, 128, None) == -1
    assert b"multiple" in lib.coocc_last_error()
    assert lib.coocc_fpn_sum_bwd(one, 128, dups, (ctypes.c_int * 4)(1, 2, 4, 0), 5, 1, 8, 8, 2, 128, None) == -1
    assert lib.coocc_fpn_sum_bwd(one, 126, dups, (ctypes.c_int * 4)(1, 2, 4, 0), 3, 1, 8, 8, 2, 126, None) == -1      # C % 4
    alias = (ctypes.c_void_p * 4)(16, 0, 0, 0)
    assert lib.coocc_fpn_sum_bwd(one, 128, alias, (ctypes.c_int * 4)(1, 0, 0, 0), 1, 1, 8, 8, 2, 128, None) == -1
    assert b"aliases" in lib.coocc_last_error()
    # every level skipped: nothing to launch, no error
    none = (ctypes.c_void_p * 4)(None, None, None, None)
    assert lib.coocc_fpn_sum_bwd(one, 128, none, (ctypes.c_int * 4)(1, 1, 0, 0), 2, 1, 8, 8, 2, 128, None) == 0
