"""The image encoder's training option, host side (no GPU): the opt-in wiring of the detector and of ``register_into_mmdet``, the
new C entry points in the header and the ctypes table, and the stage-freezing bookkeeping of ``ResNet.train()``."""
import inspect

import pytest
import torch

from co_occ_amd import _lib, image_encoder as IE, registry
from test_abi import header_functions
from test_image_encoder_host import NECK, R50, _mini_detector


def test_the_option_needs_this_packages_encoder():
    with pytest.raises(ValueError, match="hip_image_encoder=True"):
        _mini_detector(img_backbone=dict(R50), img_neck=dict(NECK), external_encoders=True, train_image_encoder=True)
    with pytest.raises(ValueError, match="hip_image_encoder=True"):          # an injected module is not ours either
        _mini_detector(img_backbone=torch.nn.Identity(), img_neck=dict(NECK), hip_image_encoder=True, train_image_encoder=True)
    with pytest.raises(ValueError, match="hip_image_encoder=True"):
        registry.register_into_mmdet(train_image_encoder=True)
    import co_occ_amd as pkg
    for cls in (pkg.COOCC_Ray, pkg.COOCC_Ray_L):
        assert inspect.signature(cls.__init__).parameters["train_image_encoder"].default is False
    assert inspect.signature(registry.register_into_mmdet).parameters["train_image_encoder"].default is False


def test_detector_sets_train_enabled_on_both_modules():
    off = _mini_detector(img_backbone=dict(R50), img_neck=dict(NECK), hip_image_encoder=True)
    assert not off.train_image_encoder and not off.img_backbone.train_enabled and not off.img_neck.train_enabled
    off.train()
    assert off.img_backbone.bn1.training and off.img_backbone.conv1.weight.requires_grad       # frozen_stages=0 is inert without it
    det = _mini_detector(img_backbone=dict(R50), img_neck=dict(NECK), hip_image_encoder=True, train_image_encoder=True)
    assert det.train_image_encoder and det.img_backbone.train_enabled and det.img_neck.train_enabled
    assert "train_image_encoder" not in det.ignored_cfg_keys
    det.train()
    bb = det.img_backbone
    assert not bb.bn1.training and not bb.conv1.weight.requires_grad and bb.layer1.training and bb.layer1[0].conv1.weight.requires_grad
    assert [k for k in det.state_dict() if k.startswith(("img_backbone.", "img_neck."))] == \
        [k for k in off.state_dict() if k.startswith(("img_backbone.", "img_neck."))]
    with pytest.raises(_lib.CooccError, match="GPU only"):                  # the train() forward is reached; it has no CPU path
        bb(torch.zeros(1, 3, 32, 32))
    with pytest.raises(NotImplementedError, match=r"\.eval\(\)"):
        off.img_backbone(torch.zeros(1, 3, 32, 32))


def test_registered_classes_have_the_option_on():
    bb_cls, nk_cls = registry.training_image_encoder()
    assert bb_cls.__name__ == "ResNet" and nk_cls.__name__ == "SECONDFPN"
    assert issubclass(bb_cls, IE.ResNet) and issubclass(nk_cls, IE.SECONDFPN)
    bb = bb_cls(**{k: v for k, v in R50.items() if k != "type"})
    nk = nk_cls(**{k: v for k, v in NECK.items() if k != "type"})
    assert bb.train_enabled and nk.train_enabled
    assert not bb.bn1.training and not bb.conv1.weight.requires_grad          # frozen at construction, as mmdet does
    assert not IE.ResNet(depth=50).train_enabled and not IE.SECONDFPN().train_enabled


def test_new_entry_points_in_header_and_table():
    fns = header_functions()
    want = {"coocc_maxpool2d_rows": 10, "coocc_maxpool2d_rows_bwd": 11, "coocc_img_stem_wgrad": 11, "coocc_img_stem_wgrad_ws": 3}
    for name, n in want.items():
        assert fns.get(name) == n and name in _lib.SIGNATURES and len(_lib.SIGNATURES[name][1]) == n, name
    lib = _lib.load()
    # partial [147][64] sums: one per 8 x 16 tile of the convolution map, 512 at the most -- a function of the shape only
    assert lib.coocc_img_stem_wgrad_ws(1, 7, 7) == 147 * 64 * 4
    assert lib.coocc_img_stem_wgrad_ws(1, 36, 68) == 3 * 3 * 147 * 64 * 4
    assert lib.coocc_img_stem_wgrad_ws(6, 256, 704) == 512 * 147 * 64 * 4 == lib.coocc_img_stem_wgrad_ws(6, 896, 1600)
    assert lib.coocc_img_stem_wgrad_ws(0, 7, 7) == 0


def _modes(bb):
    """(modules in eval mode, parameters out of the gradient), by name."""
    return ({k for k, m in bb.named_modules() if k and not m.training and not list(m.children())},
            {k for k, p in bb.named_parameters() if not p.requires_grad})


def _under(bb, prefixes):
    mods = {k for k, m in bb.named_modules() if k and not list(m.children()) and k.startswith(prefixes)}
    prms = {k for k, p in bb.named_parameters() if k.startswith(prefixes)}
    return mods, prms


@pytest.mark.parametrize("frozen", [-1, 0, 2])
def test_train_bookkeeping_follows_mmdet(frozen):
    bb = IE.ResNet(depth=50, frozen_stages=frozen, norm_eval=False)
    bb.train()
    assert _modes(bb) == (set(), set())                                       # option off: nothing touched
    bb.train_enabled = True
    bb.train()
    prefixes = tuple(["conv1", "bn1"] + ["layer%d." % i for i in range(1, frozen + 1)]) if frozen >= 0 else ("\0",)
    assert _modes(bb) == _under(bb, prefixes)
    assert bb.training and (frozen < 0) == bb.bn1.training
    bb.eval()
    assert not any(m.training for m in bb.modules())
    bb.train()                                                               # ... and back
    assert _modes(bb) == _under(bb, prefixes)


def test_norm_eval_and_frozen_norm_parameters():
    bb = IE.ResNet(depth=50, frozen_stages=-1, norm_eval=True, norm_cfg=dict(type='BN', requires_grad=False))
    bb.train()
    assert _modes(bb) == (set(), set())
    bb.train_enabled = True
    bb.train()
    ev, fr = _modes(bb)
    bns = {k for k, m in bb.named_modules() if isinstance(m, torch.nn.BatchNorm2d)}
    assert ev == bns and len(bns) == 53
    assert fr == {k + s for k in bns for s in (".weight", ".bias")}
    IE._check_trainable_norms(bb)                                             # frozen affine parameters: accepted
    bb = IE.ResNet(depth=50, frozen_stages=0, norm_eval=True)
    bb.train_enabled = True
    bb.train()
    with pytest.raises(NotImplementedError, match="requires_grad"):
        IE._check_trainable_norms(bb)
    nk = IE.SECONDFPN(norm_cfg=dict(type='BN', eps=1e-3, momentum=0.01, requires_grad=False))
    nk.train()
    assert all(p.requires_grad for p in nk.parameters())
    nk.train_enabled = True
    nk.train()
    assert {k for k, p in nk.named_parameters() if not p.requires_grad} == {"deblocks.%d.1.%s" % (i, s) for i in range(3)
                                                                           for s in ("weight", "bias")}
