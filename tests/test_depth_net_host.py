"""DepthNet without a GPU: the restatement (tests/ref_depth_net.py) against the fixture made from the reference's own wiring
(tests/golden/depthnet.npz, tools/gen_depthnet_golden.py), the two independent forms of the deformable convolution against each
other, the module's state_dict against the reference's keys, the opt-in wiring and the refusals."""
import pytest
import torch
import torch.nn.functional as F

import co_occ_amd as pkg
import ref_depth_net as R
from co_occ_amd import _lib, depth_net as dn, registry


@pytest.fixture(scope="module")
def fix(golden):
    z = golden("depthnet")
    sd = {k[3:]: torch.from_numpy(z[k]) for k in z.files if k.startswith("sd/")}
    return sd, {k: torch.from_numpy(z[k]) for k in z.files if not k.startswith("sd/")}


def _dcn_case(seed, H, W, sigma, integer=False, C=16):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(2, C, H, W, generator=g, dtype=torch.float64)
    off = torch.randn(2, 18, H, W, generator=g, dtype=torch.float64) * sigma
    if integer:
        off = off.round()
    w = torch.randn(C, C // 4, 3, 3, generator=g, dtype=torch.float64)
    return x, off, w


@pytest.mark.parametrize("sigma,integer", [(1.0, False), (3.0, False), (20.0, False), (3.0, True)])
def test_the_two_dcn_forms_agree(sigma, integer):
    x, off, w = _dcn_case(3, 7, 11, sigma, integer)
    a, b = R.dcn(x, off, w, form="gather"), R.dcn(x, off, w, form="grid")
    assert float((a - b).abs().max()) <= 1e-12 * max(1.0, float(a.abs().max()))
    if sigma == 20.0:
        py, px = R.tap_positions(off)
        outside = (py <= -1) | (py >= 7) | (px <= -1) | (px >= 11)
        assert 0.2 < float(outside.double().mean()) < 1.0
        assert float(R.dcn_cols_gather(x, off).permute(0, 2, 3, 4, 1)[outside].abs().max()) == 0.0


def test_dcn_with_zero_offsets_is_the_grouped_convolution():
    x, off, w = _dcn_case(4, 7, 11, 0.0)
    want = F.conv2d(x, w, padding=1, groups=4)
    for form in ("gather", "grid"):
        assert float((R.dcn(x, off * 0, w, form=form) - want).abs().max()) <= 1e-12


def test_restatement_reproduces_the_fixture(fix):
    sd, t = fix
    for form in ("gather", "grid"):
        out = R.depth_net(sd, t["x"].double(), t["mlp_input"].double(), form=form)
        assert out.shape == t["out"].shape
        assert float((out - t["out"]).abs().max()) <= 1e-12
    a = R.aspp(t["aspp_in"], R.cast(sd, torch.float64), "depth_conv.3")
    assert float((a - t["aspp_out"]).abs().max()) <= 1e-12


def test_state_dict_is_the_references(fix):
    sd, _ = fix
    net = dn.DepthNet(32, 32, 16, 24)
    own = net.state_dict()
    assert len(own) == 107 and set(own) == set(sd)
    assert {k: tuple(v.shape) for k, v in own.items()} == {k: tuple(v.shape) for k, v in sd.items()}
    res = net.load_state_dict(sd, strict=True)
    assert not res.missing_keys and not res.unexpected_keys
    assert torch.equal(net.depth_conv[4].conv_offset.weight, sd["depth_conv.4.conv_offset.weight"])
    fresh = dn.DepthNet(32, 32, 16, 24).depth_conv[4].conv_offset
    assert float(fresh.weight.detach().abs().max()) == 0.0 and float(fresh.bias.detach().abs().max()) == 0.0      # zero-initialised, as DeformConv2dPack


def _vt(**kw):
    return pkg.ViewTransformerLiftSplatShootVoxel(
        grid_config={'xbound': [-8., 8., 2.], 'ybound': [-8., 8., 2.], 'zbound': [-2., 2., 2.], 'dbound': [2.0, 10.0, 1.0]},
        data_config={'input_size': (64, 96)}, numC_input=32, numC_Trans=16, downsample=16, **kw)


def test_opt_in_builds_the_hip_module():
    vt = _vt(depth_net='hip')
    assert isinstance(vt.depth_net, dn.DepthNet)
    d = vt.depth_net
    assert (d.in_channels, d.mid_channels, d.context_channels, d.depth_channels, d.cam_channels) == (32, 32, 16, vt.D, 27)
    assert sum(k.startswith("depth_net.") for k in vt.state_dict()) == 107


def test_other_depth_net_values_behave_as_before():
    import torch.nn as nn
    stub = nn.Conv2d(4, 4, 1)
    assert _vt(depth_net=stub).depth_net is stub
    for v in (None, 'reference', 'HIP'):
        vt = _vt(depth_net=v)
        assert vt.depth_net is None                      # no reference plugin / mmcv here: today's path
        x = torch.zeros(1, 1, 32, 4, 6)
        with pytest.raises(NotImplementedError, match="DepthNet"):
            vt.lift((x,) + (None,) * 7)
        with pytest.raises(NotImplementedError, match="DepthNet"):
            vt.forward((x,) + (None,) * 7)


def test_cpu_input_and_train_are_refused():
    net = dn.DepthNet(32, 32, 16, 24)
    x, m = torch.zeros(2, 32, 5, 7), torch.zeros(1, 2, 27)
    with pytest.raises(NotImplementedError, match="training"):
        net(x, m)
    net.eval()
    with pytest.raises(_lib.CooccError, match="GPU only"):
        net(x, m)


def test_register_into_mmdet_without_mmdet():
    try:
        import mmdet  # noqa: F401
        import mmdet3d  # noqa: F401
        have = True
    except Exception:
        have = False
    assert registry.register_into_mmdet(hip_depth_net=True) is have
    cls = registry.hip_depth_net_view_transformer()
    assert cls.__name__ == "ViewTransformerLiftSplatShootVoxel" and issubclass(cls, pkg.ViewTransformerLiftSplatShootVoxel)
    vt = cls(grid_config={'xbound': [-8., 8., 2.], 'ybound': [-8., 8., 2.], 'zbound': [-2., 2., 2.], 'dbound': [2.0, 10.0, 1.0]},
             data_config={'input_size': (64, 96)}, numC_input=32, numC_Trans=16, downsample=16)
    assert isinstance(vt.depth_net, dn.DepthNet)
