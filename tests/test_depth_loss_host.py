"""The device DepthNet depth loss, host half (no GPU): the four entry points exist in the library, the header and the ctypes table
and validate before launching; the option is off by default and reaches the view transformer from the detectors and the registry;
'kld' stays refused in both modes; the float64 yardstick (tests/ref_depth_loss.py) evaluated in float32 is today's eager
``get_depth_loss``, its labels are ``get_downsampled_gt_depth``'s bits, and the fixtures hold what they claim to."""
import ctypes
import inspect
import sys
import types

import numpy as np
import pytest
import torch

import co_occ_amd as pkg
import co_occ_amd.synth as synth
from co_occ_amd import _lib, autograd as ag, registry
from co_occ_amd.losses import depth_labels_device, depth_loss_device
from co_occ_amd.view_transformer import ViewTransformerLiftSplatShootVoxel

import ref_depth_loss as R
import test_abi

ENTRY_POINTS = ("coocc_depth_labels", "coocc_depth_bce_ws", "coocc_depth_bce", "coocc_depth_bce_bwd")
one = ctypes.c_void_p(256)          # a non-null aligned dummy address: validation never dereferences device pointers


# ----------------------------------------------------------------------------- ABI
def test_entry_points_are_exported_declared_and_bound():
    lib = ctypes.CDLL(_lib.LIB_PATH)
    fns = test_abi.header_functions()
    for name in ENTRY_POINTS:
        assert hasattr(lib, name), "missing export " + name
        assert name in fns, name + " is not declared in include/coocc_hip.h"
        assert name in _lib.SIGNATURES and len(_lib.SIGNATURES[name][1]) == fns[name], name
    assert issubclass(ag.DepthLossFn, torch.autograd.Function)


def _labels(lib, gt=one, H=32, W=48, ds=16, D=112, vals=one, labels=one):
    return lib.coocc_depth_labels(gt, 2, H, W, ds, 1.75, 0.5, D, vals, labels, None)


def _bce(lib, prob=one, D=112, ws=one, ws_bytes=1 << 20, stats=one, h=2):
    return lib.coocc_depth_bce(prob, one, 2, D, h, 3, 1.0, one, stats, ws, ws_bytes, None)


def _bwd(lib, prob=one, D=112, gout=one, h=2):
    return lib.coocc_depth_bce_bwd(prob, one, 2, D, h, 3, 1.0, one, gout, one, None)


def test_entry_points_validate_before_launching():
    """COOCC_EINVAL (-1) with the entry point's own name, before any launch (so without a GPU)."""
    lib = _lib.load()
    bad = lambda rc, name: rc == -1 and name in lib.coocc_last_error()
    for kw in (dict(gt=None), dict(vals=None), dict(labels=None), dict(H=33), dict(W=40), dict(ds=3), dict(ds=0), dict(ds=64), dict(ds=-16),
               dict(D=0)):
        assert bad(_labels(lib, **kw), b"depth_labels"), kw
    assert _labels(lib, gt=None) == -1 and b"null" in lib.coocc_last_error()
    assert _labels(lib, ds=3) == -1 and b"ds = 3" in lib.coocc_last_error()
    for kw in (dict(prob=None), dict(ws=None), dict(stats=None), dict(D=0), dict(h=0)):
        assert bad(_bce(lib, **kw), b"depth_bce"), kw
    need = lib.coocc_depth_bce_ws(6 * 16 * 44, 112)
    assert need >= 8 * 17 * 15                                          # 17 pixel blocks x (14 bin slices + the counts)
    rc = lib.coocc_depth_bce(one, one, 6, 112, 16, 44, 1.0, one, one, one, need - 1, None)
    assert bad(rc, b"depth_bce") and b"workspace" in lib.coocc_last_error()
    for kw in (dict(prob=None), dict(gout=None), dict(D=0), dict(h=0)):
        assert bad(_bwd(lib, **kw), b"depth_bce_bwd"), kw


def test_device_functions_refuse_cpu_tensors_by_name():
    f = R.reference("ragged_ds4")
    with pytest.raises(_lib.CooccError, match="depth_labels_device"):
        depth_labels_device(f["gt"], f["ds"], f["dbound"], f["D"])
    with pytest.raises(_lib.CooccError, match="depth_loss_device"):
        depth_loss_device(f["preds"], f["gt"], f["ds"], f["dbound"], f["D"], f["weight"])


# ----------------------------------------------------------------------------- option plumbing
def test_option_is_off_by_default_everywhere():
    for fn in (ViewTransformerLiftSplatShootVoxel.__init__, pkg.COOCC_Ray.__init__, pkg.COOCC_Ray_L.__init__, registry.register_into_mmdet):
        assert inspect.signature(fn).parameters["device_depth_loss"].default is False
    assert list(inspect.signature(registry.register_into_mmdet).parameters)[-1] == "device_depth_loss"
    assert R.module(R.reference("ragged_ds4")).device_depth_loss is False
    m = pkg.build_detector(synth.model_cfg())
    assert m.device_depth_loss is False and m.img_view_transformer.device_depth_loss is False


def test_detector_option_reaches_the_view_transformer():
    m = pkg.build_detector(dict(synth.model_cfg(), device_depth_loss=True))
    assert m.device_depth_loss is True and m.img_view_transformer.device_depth_loss is True
    assert "device_depth_loss" not in m.ignored_cfg_keys
    # a LiDAR-only detector has no view transformer: the key is taken and ignored
    lcfg = dict(synth.model_cfg(), type='COOCC_Ray_L', occ_fuser=None, img_view_transformer=None)
    ml = pkg.build_detector(lcfg, external_encoders=True, device_depth_loss=True)
    assert type(ml).__name__ == "COOCC_Ray_L" and ml.img_view_transformer is None and "device_depth_loss" not in ml.ignored_cfg_keys


@pytest.mark.parametrize("on", [False, True])
def test_kld_is_refused_in_both_modes(on):
    f = R.reference("ragged_ds4")
    vt = R.module(f)
    vt.loss_depth_type, vt.device_depth_loss = 'kld', on
    with pytest.raises(NotImplementedError, match="kld"):
        vt.get_depth_loss(f["gt"], f["preds"])


class _FakeRegistry:
    def __init__(self):
        self.module_dict = {}

    def register_module(self, name=None, force=False, module=None):
        self.module_dict[name] = module
        return module


def test_register_into_mmdet_registers_the_option_on(monkeypatch):
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
    vt_name = "ViewTransformerLiftSplatShootVoxel"
    vt_cfg = {k: v for k, v in synth.model_cfg()["img_view_transformer"].items() if k != "type"}
    assert pkg.register_into_mmdet() is True
    assert m3b.NECKS.module_dict[vt_name] is ViewTransformerLiftSplatShootVoxel      # default registration: the unchanged class
    # without detectors=True: the module alone (the reference's detector calls its get_depth_loss)
    assert pkg.register_into_mmdet(device_depth_loss=True) is True
    cls = m3b.NECKS.module_dict[vt_name]
    assert cls.__name__ == vt_name and issubclass(cls, ViewTransformerLiftSplatShootVoxel) and cls is not ViewTransformerLiftSplatShootVoxel
    assert cls(**dict(vt_cfg, depth_net=torch.nn.Identity())).device_depth_loss is True
    assert cls(**dict(vt_cfg, depth_net=torch.nn.Identity(), device_depth_loss=False)).device_depth_loss is False
    assert pkg.build_neck(dict(synth.model_cfg()["img_view_transformer"], depth_net=torch.nn.Identity())).device_depth_loss is False
    # on top of hip_depth_net / train_depth_net: a subclass of what those options produced
    assert pkg.register_into_mmdet(hip_depth_net=True, train_depth_net=True, device_depth_loss=True) is True
    v = m3b.NECKS.module_dict[vt_name](**vt_cfg)
    assert v.device_depth_loss is True and type(v.depth_net).__name__ == "DepthNet" and v.depth_net.train_enabled is True
    # detectors=True: both detectors with the option on, on top of the device_occ_losses and trunk-training wrappers
    assert pkg.register_into_mmdet(detectors=True, train_lidar_trunk=True, device_occ_losses=True, device_depth_loss=True) is True
    cfg = {k: v for k, v in synth.model_cfg().items() if k != "type"}
    cls = mb.DETECTORS.module_dict["COOCC_Ray"]
    assert cls.__name__ == "COOCC_Ray" and issubclass(cls, pkg.COOCC_Ray) and cls is not pkg.COOCC_Ray
    m = cls(**cfg)
    assert m.device_depth_loss is True and m.img_view_transformer.device_depth_loss is True and m.pts_bbox_head.device_losses is True
    m = cls(**dict(cfg, device_depth_loss=False))
    assert m.device_depth_loss is False and m.img_view_transformer.device_depth_loss is False
    ml = mb.DETECTORS.module_dict["COOCC_Ray_L"](**dict(cfg, occ_fuser=None, external_encoders=True))
    assert ml.device_depth_loss is True and ml.train_lidar_trunk is True and ml.pts_bbox_head.device_losses is True
    assert pkg.build_detector(synth.model_cfg()).img_view_transformer.device_depth_loss is False   # this package's own registry: untouched


# ----------------------------------------------------------------------------- the restatement and its fixtures
@pytest.mark.parametrize("name", list(R.FIXTURES))
def test_restatement_in_float32_is_the_eager_loss(name):
    f = R.reference(name)
    floor = 2e-5 * max(1.0, abs(f["v64"]))
    assert abs(f["v32"] - f["ve"]) <= floor, (f["v32"], f["ve"])
    for g32, ge, g64 in zip(f["g32"], f["ge"], f["g64"]):
        assert g32.shape == ge.shape == tuple(f["preds"].shape) and np.isfinite(ge).all() and np.isfinite(g64).all()
        assert np.abs(g32 - ge).max() <= 2e-5 * np.abs(g64).max()
    assert np.isfinite(f["v64"]) and abs(f["v64"] - f["ve"]) <= floor


@pytest.mark.parametrize("name", list(R.FIXTURES) + list(R.LABEL_ONLY))
def test_restatement_labels_are_the_eager_bits(name):
    f = R.reference(name) if name in R.FIXTURES else R.label_case(name)
    vals, lab = R.labels_fp32(f["gt"], f["ds"], f["dbound"], f["D"])
    evals, elab = R.eager_labels(f)
    assert vals.dtype == evals.dtype == torch.float32 and torch.equal(vals.view(torch.int32), evals.view(torch.int32))
    assert torch.equal(lab, elab) and int(lab.max()) <= f["D"] and int(lab.min()) >= 0


@pytest.mark.parametrize("name", list(R.FIXTURES))
def test_fixture_has_foreground_unless_it_is_empty(name):
    f = R.reference(name)
    n_fg = int((f["labels"] > 0).sum())
    if name == "empty":
        assert n_fg == 0 and f["v64"] == 0.0 and f["ve"] == 0.0 and all(not g.any() for g in f["g64"] + f["ge"])
    else:
        assert n_fg > 0 and f["v64"] > 0.0 and any(g.any() for g in f["g64"])


def test_fixture_shapes_are_the_ones_named():
    px = lambda n: tuple(R.reference(n)["labels"].shape)
    assert px("edges") == (2, 2, 3) and px("ragged_63px_D110") == (3, 3, 7) and px("ragged_264px_D7") == (6, 4, 11)
    assert R.reference("ragged_ds1")["ds"] == 1 and R.reference("ragged_ds4")["ds"] == 4
    assert not R.reference("strided")["preds"].is_contiguous()


def test_edges_holds_the_hand_placed_patches():
    f = R.reference("edges")
    for (b, i, j), (what, want) in R.EDGE_PATCHES.items():
        assert int(f["labels"][b, i, j]) == want, (what, int(f["labels"][b, i, j]), float(f["vals"][b, i, j]))
    assert len(R.EDGE_PATCHES) == f["labels"].numel()
    v = f["vals"]
    assert float(v[0, 1, 2]) == 112.0 and float(v[1, 0, 0]) == 113.0 and float(v[1, 0, 2]) == 0.0 and float(v[0, 1, 0]) < 0.0
    assert 0.0 < float(v[0, 0, 2]) < 1.0 and float(v[0, 0, 0]) > 113.0


def test_saturated_holds_the_clamped_elements():
    f = R.reference("saturated")
    lab, p = f["labels"], f["preds"]
    n_fg = int((lab > 0).sum())
    at_label = torch.gather(p, 1, (lab.clamp(min=1) - 1)[:, None])[:, 0][lab > 0]
    assert n_fg > 0 and bool((at_label == 0.0).all()) and int((p == 1.0).sum()) == n_fg
    assert f["v64"] >= 200.0 * f["weight"] - 1e-9                       # two elements of 100 in every pixel's sum, over n_fg
    assert np.isfinite(f["g64"][0]).all() and np.abs(f["g64"][0]).max() == pytest.approx(1e12 * f["weight"] / n_fg, rel=1e-12)
