"""Host half of the LiDAR-only trunk (SECOND3D + SECOND3DFPN): registry surface and state_dict maps against the fixture made by the
unmodified reference modules (tools/gen_golden_second3d.py -> tests/golden/second3d.npz), the torch restatement against the same
fixture, the weight reorder / deconvolution packing against a direct numpy evaluation, and the refused variants.  No GPU needed."""
import ctypes

import numpy as np
import pytest
import torch

from co_occ_amd import _lib, core, registry, synth
from co_occ_amd.lidar_trunk import SECOND3D, SECOND3DFPN

import ref_second3d

STORED = ("small", "config")


def _maps(g, case, tag):
    return dict(zip(g["%s_%s_keys" % (case, tag)].tolist(), g["%s_%s_shapes" % (case, tag)].tolist()))


def _shape_map(m):
    return {k: ",".join(str(d) for d in v.shape) for k, v in m.state_dict().items()}


@pytest.mark.parametrize("case", STORED)
def test_registry_builds_the_config_and_state_dict_maps_match_the_reference(golden, case):
    g = golden("second3d")
    bcfg, ncfg = synth.second3d_cfg(synth.SECOND3D_CASES[case]["layer_nums"])
    kept = dict(bcfg["conv_cfg"]), dict(ncfg["extra_conv"])
    b, n = registry.BACKBONES.build(bcfg), registry.NECKS.build(ncfg)
    assert isinstance(b, SECOND3D) and isinstance(n, SECOND3DFPN)
    assert (bcfg["conv_cfg"], ncfg["extra_conv"]) == kept, "the caller's config dicts are left as they were"
    assert _shape_map(b) == _maps(g, case, "backbone")
    assert _shape_map(n) == _maps(g, case, "neck")
    assert list(b.state_dict()) == g[case + "_backbone_keys"].tolist() and list(n.state_dict()) == g[case + "_neck_keys"].tolist()
    sd = n.state_dict()
    assert tuple(sd["deblocks.0.0.weight"].shape) == (128, 128, 1, 1, 1) and tuple(sd["deblocks.2.0.weight"].shape) == (512, 128, 1, 4, 4)


def test_default_constructors_and_cascade_follow_the_reference():
    b = SECOND3D()
    assert b.is_cascade and b.kernel == (1, 3, 3) and [blk[0].in_channels for blk in b.blocks] == [128, 128, 128]
    assert [len(blk) for blk in b.blocks] == [12, 18, 18] and b.blocks[0][0].stride == (1, 2, 2) and b.blocks[0][0].padding == (0, 1, 1)
    assert all(m.bias is None for m in b.modules() if isinstance(m, torch.nn.Conv3d))
    # without a "bias" key the conv layers keep nn.Conv3d's default, as build_conv_layer leaves it (second3d.py:54-60)
    bb = SECOND3D(layer_nums=[1, 1, 1], conv_cfg=dict(type="Conv3d"))
    assert "blocks.0.0.bias" in bb.state_dict() and "blocks.2.3.bias" in bb.state_dict()
    rb = ref_second3d.RefSECOND3D(layer_nums=[1, 1, 1], conv_cfg=dict(type="Conv3d"))
    assert {k: tuple(v.shape) for k, v in bb.state_dict().items()} == {k: tuple(v.shape) for k, v in rb.state_dict().items()}
    assert SECOND3DFPN(init_cfg=dict(type="Kaiming", layer="ConvTranspose3d")).init_cfg == dict(type="Kaiming", layer="ConvTranspose3d")
    before = bb.blocks[0][0].weight.clone()
    bb.init_weights()                                                   # Kaiming on request, not in the constructor
    assert not torch.equal(before, bb.blocks[0][0].weight) and float(bb.blocks[0][0].bias.abs().max()) == 0.0
    n = SECOND3DFPN()
    assert all(isinstance(d[0], torch.nn.ConvTranspose3d) for d in n.deblocks) and not hasattr(n, "extra_blocks")
    assert tuple(n.deblocks[0][0].weight.shape) == (128, 256, 1, 1, 1)


@pytest.mark.parametrize("case", STORED)
def test_restatement_reproduces_the_reference_outputs(golden, case):
    g = golden("second3d")
    assert float(g[case + "_restatement_delta"]) == 0.0          # what the tool measured between the two: the bound used here
    c = synth.SECOND3D_CASES[case]
    bcfg, ncfg = synth.second3d_cfg(c["layer_nums"])
    b, n = ref_second3d.build(bcfg, ncfg)
    sdb, sdn = synth.second3d_weights(b, n, c["seed"])
    b.load_state_dict(sdb), n.load_state_dict(sdn)
    torch.set_num_threads(1)
    feats, y = ref_second3d.run(b, n, synth.second3d_input(c["grid_zyx"], seed=c["seed"]))
    for i, f in enumerate(feats):
        assert np.array_equal(f.numpy(), g["%s_feat%d" % (case, i)]), "backbone output %d" % i
    assert np.array_equal(y.numpy(), g[case + "_neck"])
    assert tuple(y.shape) == (1, 128) + tuple(c["grid_zyx"])


def test_tap_reorder_matches_a_direct_evaluation():
    """zyx_weight + the (dx*ky + dy)*kz + dz tap order: the conv evaluated from the reordered taps on (b, x, y, z) rows equals
    torch's conv3d on the [B,C,Z,Y,X] volume."""
    rs = np.random.RandomState(3)
    w = torch.from_numpy(rs.randn(5, 4, 1, 3, 3))                      # [N, C, kz, ky, kx]
    x = torch.from_numpy(rs.randn(1, 4, 2, 6, 7))                      # [B, C, Z, Y, X]
    want = torch.nn.functional.conv3d(x, w, stride=(1, 2, 2), padding=(0, 1, 1))     # [1, 5, 2, 3, 4]
    wr = core.zyx_weight(w)
    assert tuple(wr.shape) == (5, 4, 3, 3, 1)
    pc = core.PackedConv(wr.float(), kernel=(3, 3, 1), strides=(2, 2, 1))
    assert pc.taps == 9 and pc.kernel == (3, 3, 1) and pc.pads == (1, 1, 0) and pc.aniso
    assert core.out_dims(7, 6, 2, pc) == (4, 3, 2)
    taps = wr.reshape(5, 4, 9).numpy()                                  # tap t = (dx*3 + dy)*1 + dz
    xs = x.permute(0, 4, 3, 2, 1).numpy()[0]                            # [X, Y, Z, C]
    got = np.zeros((4, 3, 2, 5))
    for ox in range(4):
        for oy in range(3):
            for oz in range(2):
                for dx in range(3):
                    for dy in range(3):
                        ix, iy = ox * 2 - 1 + dx, oy * 2 - 1 + dy
                        if 0 <= ix < 7 and 0 <= iy < 6:
                            got[ox, oy, oz] += taps[:, :, dx * 3 + dy] @ xs[ix, iy, oz]
    assert np.allclose(got, want[0].permute(3, 2, 1, 0).numpy(), atol=1e-12)
    assert pc._w_raw is None                                            # strided: never on the Winograd path
    p1 = core.PackedConv(wr.float(), kernel=(3, 3, 1))
    assert p1._w_raw is not None and p1.wino_kz == 1 and core.PackedConv(torch.zeros(4, 4, 3, 3, 3), ksize=3, pad=1).wino_kz == 3


def test_wino_pack_of_a_3x3x1_layer_has_one_z_tap():
    w = torch.randn(8, 32, 3, 3, 1)
    pc = core.PackedConv(w, kernel=(3, 3, 1))
    U = pc.wino_pack(4)
    lib = _lib.load()
    assert U.shape == (36, lib.coocc_conv_pack_weights(None, 8, 32, 1, 0, None))
    G = core.PackedConv._wino_G(4)
    want = torch.einsum("pa,qb,ncab->pqnc", G, G, w[..., 0].double()).reshape(36, 8, 32).float()
    ref = torch.zeros_like(U)
    for p in range(36):
        a = want[p].contiguous().view(8, 32, 1)
        lib.coocc_conv_pack_weights(ctypes.c_void_p(a.data_ptr()), 8, 32, 1, 0, ctypes.c_void_p(ref[p].data_ptr()))
    assert torch.equal(U, ref)
    assert pc.wino_h2_pack(4).shape[:3] == (36, 1, 1)                   # [points][chunks = 1][taps = 1]...


@pytest.mark.parametrize("s", [1, 2, 4])
def test_deconv_packing_matches_conv_transpose3d(s):
    rs = np.random.RandomState(s)
    w = torch.from_numpy(rs.randn(6, 3, 1, s, s))                      # [Cin, Cout, 1, s, s]
    x = torch.from_numpy(rs.randn(1, 6, 2, 3, 2))                      # [B, Cin, Z, Y, X]
    want = torch.nn.functional.conv_transpose3d(x, w, stride=(1, s, s))            # [1, 3, 2, 3 s, 2 s]
    g = core.deconv_weight(w, s)
    assert tuple(g.shape) == (s * s * 3, 6)
    rows = x.permute(0, 4, 3, 2, 1).reshape(-1, 6)                     # (x, y, z) order
    u = (rows @ g.t()).view(2, 3, 2, s * s, 3)                        # [X, Y, Z, child, Cout]
    got = torch.zeros(2 * s, 3 * s, 2, 3, dtype=torch.float64)
    for X in range(2 * s):
        for Y in range(3 * s):
            got[X, Y] = u[X // s, Y // s, :, (X % s) * s + Y % s]
    assert torch.allclose(got, want[0].permute(3, 2, 1, 0), atol=1e-12)


def test_refused_variants_name_themselves():
    bcfg, ncfg = synth.second3d_cfg((1, 1, 1))
    with pytest.raises(NotImplementedError, match="Conv2d"):
        SECOND3D(**dict({k: v for k, v in bcfg.items() if k != "type"}, conv_cfg=dict(type="Conv2d", kernel=(3, 3), bias=False)))
    with pytest.raises(NotImplementedError, match="GN"):
        SECOND3D(**dict({k: v for k, v in bcfg.items() if k != "type"}, norm_cfg=dict(type="GN", num_groups=32)))
    nk = {k: v for k, v in ncfg.items() if k != "type"}
    with pytest.raises(NotImplementedError, match="GN"):
        SECOND3DFPN(**dict(nk, norm_cfg=dict(type="GN", num_groups=32)))
    with pytest.raises(NotImplementedError, match="sep_kernel"):
        SECOND3DFPN(**dict(nk, extra_conv=dict(type="Conv3d", num_conv=1, sep_kernel=(3, 1, 1), bias=False)))
    with pytest.raises(NotImplementedError, match="use_for_distill"):
        SECOND3DFPN(**dict(nk, use_for_distill=True))
    with pytest.raises(NotImplementedError, match="upsample type"):
        SECOND3DFPN(**dict(nk, upsample_cfg=dict(type="nearest")))
    with pytest.raises(NotImplementedError, match="differs from its stride"):
        SECOND3DFPN(**dict(nk, upsample_cfg=dict(type="deconv3d", bias=False, kernel_size=(1, 3, 3))))
    with pytest.raises(NotImplementedError, match="upsample stride"):
        SECOND3DFPN(**dict(nk, upsample_strides=[1, 2, 0.5]))
    with pytest.raises(NotImplementedError, match="Conv2d"):
        SECOND3DFPN(**dict(nk, conv_cfg=dict(type="Conv2d", bias=False)))
    b, n = registry.BACKBONES.build(bcfg), registry.NECKS.build(ncfg)
    x = synth.second3d_input((2, 8, 8))
    with pytest.raises(NotImplementedError, match="train"):
        b.train()(x)
    with pytest.raises(NotImplementedError, match="train"):
        n.train()([x])
    with pytest.raises(_lib.CooccError, match="GPU only"):
        b.eval()(x)


def test_detector_builds_the_trunk_from_the_config():
    import co_occ_amd as pkg
    det = pkg.build_detector(synth.model_cfg_lidar(), external_encoders=True)
    assert isinstance(det, pkg.COOCC_Ray_L) and isinstance(det.pts_backbone, SECOND3D) and isinstance(det.pts_neck, SECOND3DFPN)
    assert det.pts_middle_encoder is None                               # SparseEncoderHD stays upstream
    with pytest.raises(NotImplementedError, match="pts_middle_feats"):
        det.extract_pts_feat([torch.zeros(4, 5)])


def test_new_entry_points_validate_before_launching():
    lib = _lib.load()
    one = ctypes.c_void_p(16)
    ups = (ctypes.c_void_p * 4)(16, 16, 16, 0)
    assert lib.coocc_fpn_sum(ups, (ctypes.c_int * 4)(1, 2, 3, 0), 3, 1, 8, 8, 2, 128, one, 128, None, None) == -1
    assert b"strides" in lib.coocc_last_error()
    assert lib.coocc_fpn_sum(ups, (ctypes.c_int * 4)(1, 2, 4, 0), 3, 1, 6, 8, 2, 128, one, 128, None, None) == -1
    assert b"multiple" in lib.coocc_last_error()
    assert lib.coocc_fpn_sum(ups, (ctypes.c_int * 4)(1, 2, 4, 0), 5, 1, 8, 8, 2, 128, one, 128, None, None) == -1
    assert lib.coocc_zyx_to_rows(one, one, 1, 126, 2, 8, 8, 126, 0, None) == -1 and b"zyx_to_rows" in lib.coocc_last_error()
    d = _lib.ConvDesc(sx=-1)
    assert [n for n, _ in _lib.ConvDesc._fields_][-3:] == ["sx", "sy", "sz"] and d.sx == -1
