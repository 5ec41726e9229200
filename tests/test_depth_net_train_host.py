"""DepthNet's training path without a GPU: the train-mode restatement (tests/ref_depth_net_train.py) against the fixture made from
the reference's own wiring under train() (tests/golden/depthnet_train.npz, tools/gen_depthnet_train_golden.py), the unchanged
state_dict, the opt-in wiring and the refusals."""
import pytest
import torch

import co_occ_amd as pkg
import ref_depth_net as R
import ref_depth_net_train as T
from co_occ_amd import _lib, depth_net as dn, registry


@pytest.fixture(scope="module")
def fix(golden):
    z = golden("depthnet_train")
    return {k: torch.from_numpy(z[k]) for k in z.files}


@pytest.fixture(scope="module")
def seeded():
    return T.seeded_state_dict(dn.DepthNet(*T.ARGS).state_dict()), T.seeded_inputs()


def _close(a, b, what):
    assert a.shape == b.shape, what
    assert float((a - b).abs().max()) <= 1e-10 * max(1.0, float(b.abs().max())), what


def test_restatement_reproduces_the_train_fixture(fix, seeded):
    sd, (x, mlp, r) = seeded
    o = T.run(sd, x, mlp, r, torch.float64)
    assert set(fix) == {"out", "dx"} | {p + k for k in T.GOLDEN_BNS for p in ("rm/", "rv/")} | {"grad/" + k for k in T.GOLDEN_GRADS}
    _close(o["out"], fix["out"], "output")
    _close(o["dx"], fix["dx"], "input gradient")
    for k in T.GOLDEN_GRADS:
        _close(o["grads"][k], fix["grad/" + k], "gradient of " + k)
    for k in T.GOLDEN_BNS:
        _close(o["stats"][k][0], fix["rm/" + k], "running_mean of " + k)
        _close(o["stats"][k][1], fix["rv/" + k], "running_var of " + k)
    assert tuple(fix["rm/bn"].shape) == (27,)                    # BatchNorm1d(cam_channels): no padded entry
    # the step moved the statistics (momentum 0.1 towards the batch's) and train() differs from eval() on the same weights
    assert float((fix["rm/depth_conv.3.bn1"] - sd["depth_conv.3.bn1.running_mean"].double()).abs().max()) > 1e-3
    assert float((R.depth_net(sd, x.double(), mlp.double()) - fix["out"]).abs().max()) > 1e-2


def test_a_given_dropout_mask_scales_the_kept_elements(seeded):
    sd, (x, mlp, r) = seeded
    sd64 = R.cast(sd, torch.float64)
    a = torch.randn(2, 32, 8, 10, generator=torch.Generator().manual_seed(1), dtype=torch.float64)
    mask = torch.rand(2, 32, 8, 10, generator=torch.Generator().manual_seed(2)) >= 0.5
    base, kept = T.aspp(a, sd64, "depth_conv.3"), T.aspp(a, sd64, "depth_conv.3", mask=mask, p=0.5)
    assert torch.equal(kept, base * mask * 2.0)


def test_state_dict_keys_are_unchanged_and_training_is_off_by_default(golden):
    z = golden("depthnet")
    ref_keys = {k[3:] for k in z.files if k.startswith("sd/")}
    net = dn.DepthNet(*T.ARGS)
    assert len(net.state_dict()) == 107 and set(net.state_dict()) == ref_keys
    aspp = net.depth_conv[3]
    assert isinstance(aspp.dropout, torch.nn.Dropout) and aspp.dropout.p == 0.5 and not list(aspp.dropout.parameters())
    assert net.train_enabled is False
    x, m = torch.zeros(2, 32, 5, 7), torch.zeros(1, 2, 27)
    with pytest.raises(NotImplementedError, match="training") as e:
        net(x, m)
    assert "train_enabled" in str(e.value) and "train_depth_net" in str(e.value)
    with pytest.raises(NotImplementedError, match="training"):
        net.forward_rows(None, m)


def _vt(cls=None, **kw):
    return (cls or pkg.ViewTransformerLiftSplatShootVoxel)(
        grid_config={'xbound': [-8., 8., 2.], 'ybound': [-8., 8., 2.], 'zbound': [-2., 2., 2.], 'dbound': [2.0, 10.0, 1.0]},
        data_config={'input_size': (64, 96)}, numC_input=32, numC_Trans=16, downsample=16, **kw)


def test_option_wiring():
    assert _vt(depth_net='hip').depth_net.train_enabled is False
    assert _vt(depth_net='hip', train_depth_net=True).depth_net.train_enabled is True
    with pytest.raises(ValueError, match="depth_net='hip'"):
        _vt(train_depth_net=True)
    with pytest.raises(ValueError, match="hip_depth_net=True"):
        registry.register_into_mmdet(train_depth_net=True)
    assert _vt(registry.hip_depth_net_view_transformer()).depth_net.train_enabled is False
    cls = registry.hip_depth_net_view_transformer(train_depth_net=True)
    assert cls.__name__ == "ViewTransformerLiftSplatShootVoxel"
    assert _vt(cls).depth_net.train_enabled is True
    assert _vt(cls, train_depth_net=False).depth_net.train_enabled is False
    try:
        import mmdet  # noqa: F401
        import mmdet3d  # noqa: F401
        have = True
    except Exception:
        have = False
    assert registry.register_into_mmdet(hip_depth_net=True, train_depth_net=True) is have


def test_one_camera_map_is_refused_under_train():
    net = dn.DepthNet(*T.ARGS)
    net.train_enabled = True
    with pytest.raises(ValueError, match="more than one camera"):
        net(torch.zeros(1, 32, 5, 7), torch.zeros(1, 1, 27))
    with pytest.raises(ValueError, match="more than 1 value"):          # torch's own refusal, restated
        T.aspp(torch.zeros(1, 32, 5, 7, dtype=torch.float64), R.cast(T.seeded_state_dict(net.state_dict()), torch.float64), "depth_conv.3")
    with pytest.raises(_lib.CooccError, match="GPU only"):              # two maps pass the check and reach the device test
        net(torch.zeros(2, 32, 5, 7), torch.zeros(1, 2, 27))
    net.eval()
    with pytest.raises(_lib.CooccError, match="GPU only"):
        net(torch.zeros(1, 32, 5, 7), torch.zeros(1, 1, 27))


def test_new_entry_points_validate_before_launching():
    import ctypes
    lib = _lib.load()
    one = ctypes.c_void_p(16)
    rc = lib.coocc_dcn_cols_bwd(one, 32, one, 20, 2, 5, 7, 32, 4, 60, 20, one, one, one, None)          # rows 60..80 of a 70-row map
    assert rc == -1 and b"dcn_cols_bwd" in lib.coocc_last_error()
    rc = lib.coocc_dcn_cols_bwd(one, 32, one, 16, 2, 5, 7, 32, 4, 0, 20, one, one, one, None)           # fewer than 18 offset columns
    assert rc == -1 and b"dcn_cols_bwd" in lib.coocc_last_error()
    rc = lib.coocc_se_gate2_bwd(one, 6, 2, 35, 6, one, one, one, one, one, one, one, None, 0, None)
    assert rc == -1 and b"se_gate2_bwd" in lib.coocc_last_error()
    rc = lib.coocc_se_gate2_bwd(one, 64, 2, 35, 64, one, one, one, one, one, one, one, None, 0, None)   # fast path without workspace
    assert rc == -1 and b"workspace" in lib.coocc_last_error()
    assert lib.coocc_se_gate2_bwd_ws(2, 65, 64) == 8 * 2 * 2 * 2 * 64
    rc = lib.coocc_cam_add(None, one, 2, 35, 6, one, 1.0, None)
    assert rc == -1 and b"cam_add" in lib.coocc_last_error()
    rc = lib.coocc_dropout_rows(one, ctypes.c_void_p(2), 4, 8, 2.0, one, None)
    assert rc == -1 and b"dropout_rows" in lib.coocc_last_error()
    rc = lib.coocc_cam_sum(one, 4, 2, 35, 8, one, None, 0, None)
    assert rc == -1 and b"cam_sum" in lib.coocc_last_error()
