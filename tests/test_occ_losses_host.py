"""The device OccHead losses, host half (no GPU): the three entry points exist in the library, the header and the ctypes table and
validate before launching; the option is off by default, reaches the head from both detectors and the registry, and a default head
never touches the new entry points; the fixtures of tests/test_gpu_occ_losses.py respect the Lovasz exclusion budget; the float64
yardstick (tests/ref_occ_losses.py) reproduces tests/golden/losses.npz."""
import ctypes
import sys
import types

import numpy as np
import pytest
import torch

import co_occ_amd as pkg
import co_occ_amd.synth as synth
from co_occ_amd import _lib, autograd as ag, losses as L, registry
from oracle import cases

import ref_occ_losses as R
import test_abi

ENTRY_POINTS = ("coocc_pool_labels", "coocc_occ_loss_fwd", "coocc_occ_loss_bwd")
one = ctypes.c_void_p(256)          # a non-null aligned dummy address: validation never dereferences device pointers


def test_entry_points_are_exported_declared_and_bound():
    lib = ctypes.CDLL(_lib.LIB_PATH)
    fns = test_abi.header_functions()
    for name in ENTRY_POINTS + ("coocc_occ_loss_ws",):
        assert hasattr(lib, name), "missing export " + name
        assert name in fns, name + " is not declared in include/coocc_hip.h"
        assert name in _lib.SIGNATURES and len(_lib.SIGNATURES[name][1]) == fns[name], name
    assert issubclass(ag.OccLossFn, torch.autograd.Function)


def _fwd(lib, logits=one, C=17, ld=17, P=100):
    return lib.coocc_occ_loss_fwd(logits, P, C, ld, one, None, 0, 0, 0, None, None, 0, one, one, one, one, 1 << 30, None)


def _bwd(lib, logits=one, C=17, ld=17, P=100):
    return lib.coocc_occ_loss_bwd(logits, P, C, ld, one, None, 0, one, one, one, one, C, None)


def test_entry_points_validate_before_launching():
    """COOCC_EINVAL (-1) with the entry point's own name, before any launch (so without a GPU)."""
    lib = _lib.load()
    for call, name in ((_fwd, b"occ_loss_fwd"), (_bwd, b"occ_loss_bwd")):
        assert call(lib, C=33, ld=33) == -1 and name in lib.coocc_last_error() and b"33" in lib.coocc_last_error()
        assert call(lib, logits=None) == -1 and name in lib.coocc_last_error() and b"null" in lib.coocc_last_error()
        assert call(lib, ld=16) == -1 and name in lib.coocc_last_error()            # a row shorter than its classes
        assert call(lib, P=0) == -1 and name in lib.coocc_last_error()
    assert lib.coocc_pool_labels(one, 1, 4, 4, 2, 3, 0, 17, one, None) == -1
    assert b"pool_labels" in lib.coocc_last_error() and b"ratio 3" in lib.coocc_last_error()
    assert lib.coocc_pool_labels(None, 1, 4, 4, 2, 2, 0, 17, one, None) == -1 and b"pool_labels" in lib.coocc_last_error()
    # the coordinate form needs somewhere to put the gathered labels
    rc = lib.coocc_occ_loss_fwd(one, 100, 17, 17, one, one, 4, 4, 4, None, None, 0, one, one, one, one, 1 << 30, None)
    assert rc == -1 and b"occ_loss_fwd" in lib.coocc_last_error()
    # a workspace below coocc_occ_loss_ws is refused as COOCC_ENOMEM
    need = lib.coocc_occ_loss_ws(6000, 17)
    assert need > 6000 * 17 * 24
    rc = lib.coocc_occ_loss_fwd(one, 6000, 17, 17, one, None, 0, 0, 0, None, None, 0, one, one, one, one, need - 512, None)
    assert rc == -3 and b"occ_loss_fwd" in lib.coocc_last_error()


def test_device_functions_refuse_cpu_tensors_by_name():
    logits, gt, fine, coord = cases.loss_inputs(cases.LOSS_CASE)
    with pytest.raises(_lib.CooccError, match="occ_loss_terms_device"):
        L.occ_loss_terms_device(logits, L.pool_labels(gt, *logits.shape[2:]))
    with pytest.raises(_lib.CooccError, match="pool_labels_device"):
        L.pool_labels_device(gt, *logits.shape[2:])


def _head(c):
    return pkg.build_head(dict(type='OccHead', in_channels=[32] * 2, out_channel=c["ncls"], num_level=2, soft_weights=True,
                               norm_cfg=dict(type='BN3d', requires_grad=True), cascade_ratio=c["ratio"], sample_from_voxel=True,
                               sample_from_img=True, final_occ_size=[v * c["ratio"] for v in c["coarse"]], empty_idx=0))


def test_option_is_off_by_default_and_reaches_the_head_from_both_detectors():
    assert _head(cases.LOSS_CASE).device_losses is False
    m = pkg.build_detector(synth.model_cfg())
    assert m.device_occ_losses is False and m.pts_bbox_head.device_losses is False
    m = pkg.build_detector(dict(synth.model_cfg(), device_occ_losses=True))
    assert m.device_occ_losses is True and m.pts_bbox_head.device_losses is True
    lcfg = dict(synth.model_cfg(), type='COOCC_Ray_L', occ_fuser=None)
    ml = pkg.build_detector(lcfg, external_encoders=True)
    assert ml.device_occ_losses is False and ml.pts_bbox_head.device_losses is False
    ml = pkg.build_detector(lcfg, external_encoders=True, device_occ_losses=True)
    assert type(ml).__name__ == "COOCC_Ray_L" and ml.pts_bbox_head.device_losses is True


def test_default_head_never_reaches_the_device_entry_points(golden, monkeypatch):
    """test_boundary's loss case with the three entry points booby-trapped: the default path is the eager one, untouched."""
    def trap(orig):
        def call(name, *a):
            if name in ENTRY_POINTS:
                raise AssertionError("a default OccHead called " + name)
            return orig(name, *a)
        return call
    import co_occ_amd.head as head_mod
    for mod in (_lib, ag, head_mod):
        monkeypatch.setattr(mod, "call", trap(mod.call))
    g = golden("losses")
    c = cases.LOSS_CASE
    logits, gt, fine, coord = cases.loss_inputs(c)
    out = _head(c).loss(output_voxels=[logits], output_coords_fine=[coord], output_voxels_fine=[fine], target_voxels=gt)
    keys = [k for k in g.files if k.startswith("loss_")]
    assert set(out) == set(keys) and len(keys) == 8
    for k in keys:
        assert abs(float(out[k]) - float(g[k])) <= 2e-5 * max(1.0, abs(float(g[k]))), (k, float(out[k]), float(g[k]))
    with pytest.raises(AssertionError, match="coocc_pool_labels"):           # the trap itself works
        _lib.call("coocc_pool_labels")


class _FakeRegistry:
    def __init__(self):
        self.module_dict = {}

    def register_module(self, name=None, force=False, module=None):
        self.module_dict[name] = module
        return module


def test_register_into_mmdet_registers_detectors_with_the_option_on(monkeypatch):
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
    with pytest.raises(ValueError, match="detectors=True"):
        pkg.register_into_mmdet(device_occ_losses=True)
    assert pkg.register_into_mmdet(detectors=True) is True
    assert mb.DETECTORS.module_dict["COOCC_Ray"] is pkg.COOCC_Ray                    # default registration: unchanged classes
    assert pkg.register_into_mmdet(detectors=True, device_occ_losses=True) is True
    cfg = {k: v for k, v in synth.model_cfg().items() if k != "type"}
    for name, kw in (("COOCC_Ray", {}), ("COOCC_Ray_L", dict(occ_fuser=None, external_encoders=True))):
        cls = mb.DETECTORS.module_dict[name]
        assert cls.__name__ == name and issubclass(cls, getattr(pkg, name)) and cls is not getattr(pkg, name)
        assert cls(**dict(cfg, **kw)).pts_bbox_head.device_losses is True
        assert cls(**dict(cfg, device_occ_losses=False, **kw)).pts_bbox_head.device_losses is False
    assert pkg.build_detector(synth.model_cfg()).pts_bbox_head.device_losses is False   # this package's own registry: untouched
    # together with the trunk-training option: both defaults on
    assert pkg.register_into_mmdet(detectors=True, train_lidar_trunk=True, device_occ_losses=True) is True
    m = mb.DETECTORS.module_dict["COOCC_Ray_L"](**dict(cfg, occ_fuser=None, external_encoders=True))
    assert m.train_lidar_trunk is True and m.pts_bbox_head.device_losses is True


@pytest.mark.parametrize("name", list(R.FIXTURES))
def test_fixture_respects_the_lovasz_exclusion_budget(name):
    """At most 0.1 % of the gradient tensor may be excluded as 'rank not decided at fp32 precision' (tests/test_gpu_occ_losses.py)."""
    r = R.reference(name)
    assert r["ex"].shape == (r["P"], r["C"])
    share = r["ex"].sum() / r["ex"].size
    assert share <= R.MAX_EXCLUDED_SHARE, "%s: %d of %d elements (%.3f %%) excluded" % (name, r["ex"].sum(), r["ex"].size, 100 * share)
    assert np.isfinite(r["v64"]).all() and all(np.isfinite(g).all() for g in r["g64"])
    assert not r["ex"][r["labels"].numpy() == 255].any()


def test_exclusion_rule_marks_opposite_status_near_ties_only():
    rows = torch.log(torch.tensor([[0.7, 0.3], [0.300004, 0.699996], [0.7, 0.3], [0.1, 0.9]], dtype=torch.float64))
    ex = R.lovasz_exclusions(rows, torch.tensor([0, 1, 0, 255]))
    # class 0: errors 0.3 (fg), 0.300004 (bg), 0.3 (fg): rows 0-2 tie across status; the ignored row never counts
    assert ex[:3].all() and not ex[3].any()
    assert not R.lovasz_exclusions(rows, torch.tensor([0, 0, 0, 255])).any()          # same status: no exclusion


def test_float64_yardstick_reproduces_the_reference_golden(golden):
    g = golden("losses")
    logits, gt, fine, coord = cases.loss_inputs(cases.LOSS_CASE)
    out, pooled = R.head_loss(logits, gt, fine, coord, torch.float64)
    assert np.array_equal(pooled.numpy(), g["pooled_target"])
    keys = [k for k in g.files if k.startswith("loss_")]
    assert set(out) == set(keys) and len(keys) == 8
    for k in keys:
        assert abs(out[k] - float(g[k])) <= 2e-5 * max(1.0, abs(float(g[k]))), (k, out[k], float(g[k]))
