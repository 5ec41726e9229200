"""The image encoder's host side (no GPU): state_dict keys against the torch restatement, the constructor's refusals, the detector's
opt-in wiring, and the restatement of SECONDFPN against the reference file's own float64 run (tests/golden/image_neck.npz,
tools/gen_image_encoder_golden.py)."""
import numpy as np
import pytest
import torch

import ref_image_encoder as R
from co_occ_amd import image_encoder as IE
from co_occ_amd import registry

R50 = dict(type='ResNet', depth=50, num_stages=4, out_indices=(0, 1, 2, 3), frozen_stages=0, norm_cfg=dict(type='BN', requires_grad=True),
           norm_eval=False, style='pytorch', pretrained='ckpts/resnet50-0676ba61.pth')
NECK = dict(type='SECONDFPN', in_channels=[256, 512, 1024, 2048], upsample_strides=[0.25, 0.5, 1, 2], out_channels=[128, 128, 128, 128])


def shapes(m):
    return {k: tuple(v.shape) for k, v in m.state_dict().items()}


@pytest.mark.parametrize("depth,entries", [(50, 318), (101, 624)])
def test_resnet_state_dict_matches_restatement(depth, entries):
    ours, ref = IE.IMAGE_BACKBONES.build(dict(R50, depth=depth)), R.TorchResNet(depth)
    assert shapes(ours) == shapes(ref) and len(shapes(ours)) == entries
    ref.load_state_dict(ours.state_dict(), strict=True)
    ours.load_state_dict(ref.state_dict(), strict=True)
    for k in ("conv1.weight", "bn1.running_var", "layer1.0.downsample.0.weight", "layer1.0.downsample.1.num_batches_tracked",
              "layer%d.%d.conv3.weight" % (3, IE.ARCH[depth][2] - 1), "layer4.2.bn3.bias"):
        assert k in ours.state_dict(), k


def test_neck_state_dict_matches_restatement():
    ours = IE.IMAGE_NECKS.build(NECK)
    ref = R.TorchSECONDFPN(NECK["in_channels"], NECK["out_channels"], NECK["upsample_strides"])
    assert shapes(ours) == shapes(ref) and len(shapes(ours)) == 24
    ref.load_state_dict(ours.state_dict(), strict=True)
    ours.load_state_dict(ref.state_dict(), strict=True)
    assert ours.deblocks[0][1].eps == 1e-3
    assert tuple(ours.deblocks[0][0].weight.shape) == (128, 256, 4, 4) and isinstance(ours.deblocks[0][0], torch.nn.Conv2d)
    assert tuple(ours.deblocks[1][0].weight.shape) == (128, 512, 2, 2)
    assert tuple(ours.deblocks[2][0].weight.shape) == (1024, 128, 1, 1) and isinstance(ours.deblocks[2][0], torch.nn.ConvTranspose2d)
    assert tuple(ours.deblocks[3][0].weight.shape) == (2048, 128, 2, 2)
    conv = IE.SECONDFPN(in_channels=[64, 64], out_channels=[32, 32], upsample_strides=[1, 2], use_conv_for_no_stride=True)
    assert isinstance(conv.deblocks[0][0], torch.nn.Conv2d) and tuple(conv.deblocks[0][0].weight.shape) == (32, 64, 1, 1)


@pytest.mark.parametrize("kw", [dict(depth=18), dict(depth=34), dict(style='caffe'), dict(deep_stem=True), dict(avg_down=True),
                                dict(dcn=dict(type='DCN', deform_groups=1)), dict(plugins=[dict(cfg=dict(type='x'))]),
                                dict(dilations=(1, 1, 2, 4)), dict(norm_cfg=dict(type='GN', num_groups=32)), dict(in_channels=4),
                                dict(stem_channels=32), dict(some_new_option=1)])
def test_resnet_refuses_what_is_not_built(kw):
    with pytest.raises(NotImplementedError) as e:
        IE.ResNet(**dict(dict(depth=50), **kw))
    assert list(kw)[0] in str(e.value)


def test_resnet_accepts_and_ignores_the_inert_arguments():
    m = IE.ResNet(depth=50, pretrained='x.pth', init_cfg=dict(type='Pretrained', checkpoint='y'), frozen_stages=2, norm_eval=True,
                  with_cp=True, zero_init_residual=False, norm_cfg=dict(type='SyncBN', requires_grad=False))
    assert len(m.state_dict()) == 318
    m.init_weights()


def test_the_classes_are_not_in_the_default_registries():
    assert "ResNet" not in registry.BACKBONES and "SECONDFPN" not in registry.NECKS
    assert IE.IMAGE_BACKBONES.get("ResNet") is IE.ResNet and IE.IMAGE_NECKS.get("SECONDFPN") is IE.SECONDFPN


def _mini_detector(**kw):
    import co_occ_amd as pkg
    from co_occ_amd import synth
    return pkg.build_detector(synth.model_cfg(C=32, block_inplanes=(32, 64, 128, 256), out_channels=32, rendering=False), **kw)


def test_detector_without_the_option_behaves_as_before(monkeypatch):
    import sys
    monkeypatch.setitem(sys.modules, "mmdet3d", None)          # mmdet3d's registries do not import (as on every machine of ours)
    with pytest.raises(ImportError) as e:
        _mini_detector(img_backbone=dict(R50), img_neck=dict(NECK))
    assert "upstream of the MI355X hot path" in str(e.value) and "'ResNet'" in str(e.value)
    det = _mini_detector(img_backbone=dict(R50), img_neck=dict(NECK), external_encoders=True)
    assert det.img_backbone is None and det.img_neck is None and det.hip_image_encoder is False


def test_detector_with_the_option_builds_ours():
    det = _mini_detector(img_backbone=dict(R50), img_neck=dict(NECK), hip_image_encoder=True)
    assert isinstance(det.img_backbone, IE.ResNet) and isinstance(det.img_neck, IE.SECONDFPN)
    keys = [k for k in det.state_dict() if k.startswith(("img_backbone.", "img_neck."))]
    assert len(keys) == 318 + 24                       # the readers hook adds no module to the backbone
    inst = torch.nn.Identity()
    det = _mini_detector(img_backbone=inst, img_neck=dict(NECK), hip_image_encoder=True)
    assert det.img_backbone is inst and isinstance(det.img_neck, IE.SECONDFPN)
    # only ResNet / SECONDFPN dicts are taken; any other type resolves as without the option
    det = _mini_detector(img_backbone=dict(type='SwinTransformer'), hip_image_encoder=True, external_encoders=True)
    assert det.img_backbone is None


def test_load_state_dict_drops_the_packs():
    m = IE.ResNet(depth=50)
    m._packs._key, m._packs._val = ["stale"], object()
    m.load_state_dict(m.state_dict())
    assert m._packs._val is None


def test_restatement_reproduces_the_reference_neck(golden):
    g = golden("image_neck")
    sd = {k[3:]: torch.from_numpy(g[k]).double() for k in g.files if k.startswith("sd/")}
    assert len(sd) == 24
    xs = [torch.from_numpy(g["x%d" % i]).double() for i in range(4)]
    out = R.second_fpn(xs, sd, list(g["strides"]))[0]
    want = torch.from_numpy(g["out"])
    assert want.dtype == torch.float64 and tuple(want.shape) == (2, 128, 2, 4)
    assert float((out - want).abs().max()) <= 1e-12 * max(1.0, float(want.abs().max()))
    # ... and the plain torch module with the same keys is the same function
    mod = R.TorchSECONDFPN([32, 64, 128, 256], [32] * 4, [0.25, 0.5, 1, 2]).double().eval()
    mod.load_state_dict(sd, strict=True)
    with torch.no_grad():
        assert float((mod(xs)[0] - want).abs().max()) <= 1e-12 * max(1.0, float(want.abs().max()))
    assert np.isfinite(g["out"]).all() and float(np.abs(g["out"]).max()) > 0.1
