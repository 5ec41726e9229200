"""``SparseEncoderHD`` on the HIP sparse engine, CPU half: state_dict surface against a list derived from upstream's constructor,
the float64 restatement (tests/ref_sparse_hd.py) against two independent forms, refusals, argument validation of the new C entry
points, the opt-in wiring.  spconv v1 cannot be built here, so no fixture comes from the unmodified module (ref_sparse_hd.py)."""
import ctypes
import sys
import types

import numpy as np
import pytest
import torch

import co_occ_amd as pkg
import co_occ_amd.synth as synth
from co_occ_amd import _lib, lidar, lidar_hd
from co_occ_amd.lidar_hd import SparseEncoderHD
from oracle import ref_lidar

import ref_sparse_hd as R


def _config_cfg(**kw):
    cfg = {k: v for k, v in synth.model_cfg_lidar()["pts_middle_encoder"].items() if k != "type"}
    cfg.update(kw)
    return cfg


_DEFAULT = dict(in_channels=4, sparse_shape=[65, 800, 800])          # the constructor defaults: block_type='conv_module'


@pytest.mark.parametrize("cfg", [_config_cfg(), _DEFAULT], ids=["basicblock", "conv_module"])
def test_state_dict_keys_and_shapes_equal_upstreams_constructor(cfg):
    m = SparseEncoderHD(**cfg)
    got = {k: tuple(v.shape) for k, v in m.state_dict().items()}
    want = R.expected_state_dict_shapes(cfg)
    assert set(got) == set(want), (sorted(set(got) - set(want))[:5], sorted(set(want) - set(got))[:5])
    assert got == want
    assert got["conv_input.0.weight"] == (3, 3, 3, 4, 16) and got["conv_out.0.weight"][:3] == (1, 1, 1)
    # an upstream checkpoint (its keys, v1 weight shapes) loads strictly
    m.load_state_dict(synth.random_state_dict({k: torch.zeros(s) for k, s in want.items()}, seed=3), strict=True)
    assert m.out_shape() == ((8, 100, 100) if cfg.get("block_type") == "basicblock" else (15, 200, 200))


def test_config_keys_are_the_ones_the_issue_lists():
    keys = set(R.expected_state_dict_shapes(_config_cfg()))
    for k in ("conv_input.0.weight", "conv_input.1.running_var", "encoder_layers.encoder_layer1.0.conv1.weight",
              "encoder_layers.encoder_layer1.0.bn1.weight", "encoder_layers.encoder_layer3.1.conv2.weight",
              "encoder_layers.encoder_layer3.1.bn2.bias", "encoder_layers.encoder_layer3.2.0.weight",
              "encoder_layers.encoder_layer3.2.1.running_mean", "conv_out.0.weight", "conv_out.1.num_batches_tracked"):
        assert k in keys, k
    assert "encoder_layers.encoder_layer2.0.0.weight" in R.expected_state_dict_shapes(_DEFAULT)


# ----------------------------------------------------------------------------- the restatement against two independent forms
_CUBIC = [((3, 3, 3), (1, 1, 1), (1, 1, 1), True), ((3, 3, 3), (2, 2, 2), (1, 1, 1), False), ((3, 3, 3), (1, 1, 1), (1, 1, 1), False),
          ((3, 3, 3), (2, 2, 2), (0, 0, 0), False), ((1, 1, 1), (1, 1, 1), (0, 0, 0), False)]
_PER_AXIS = [((3, 3, 3), (2, 2, 2), (0, 1, 1)), ((3, 3, 3), (1, 1, 1), (0, 1, 1)), ((3, 3, 3), (2, 1, 2), (1, 0, 1)), ((1, 3, 3), (1, 2, 2), (0, 1, 1))]


def _case(shape, cin, cout, k, seed):
    coors = np.unique(np.concatenate([R.edge_voxels(shape), R.random_voxels(shape, 40, seed)]), axis=0)
    g = torch.Generator().manual_seed(seed)
    feats = torch.randn(len(coors), cin, generator=g, dtype=torch.float64)
    w = torch.randn(*k, cin, cout, generator=g, dtype=torch.float64)
    return coors, feats, w


def _dense_rows(y, mask):
    idx = mask[0, 0].nonzero()                                          # ascending (z,y,x)
    return y[0][:, idx[:, 0], idx[:, 1], idx[:, 2]].t(), idx.numpy()


@pytest.mark.parametrize("k,s,p,subm", _CUBIC)
def test_restated_cubic_layers_equal_the_vendored_v1_rule_book(k, s, p, subm):
    """Every cubic layer form of the module against ``oracle.ref_lidar.spconv_v1_conv`` (imported, unmodified): the same active
    set exactly, values to float rounding (that function evaluates in float32)."""
    shape = (12, 10, 14)
    coors, feats, w = _case(shape, 3, 5, k, seed=11)
    x, mask = R.to_dense(feats, coors, shape)
    y, m2 = R.conv_layer(x, mask, w, k, s, p, subm)
    got, got_c = _dense_rows(y, m2)
    want, want_c, want_shape = ref_lidar.spconv_v1_conv(feats.float(), coors, list(shape), w.float(), k=k[0], s=s[0], p=p[0], subm=subm)
    order = np.lexsort((want_c[:, 2], want_c[:, 1], want_c[:, 0]))
    assert list(y.shape[2:]) == list(want_shape)
    assert np.array_equal(got_c, want_c[order]), "active sets differ"
    assert float((got - want[order].double()).abs().max()) <= 1e-5 * max(1.0, float(got.abs().max()))


@pytest.mark.parametrize("k,s,p", _PER_AXIS + [(k, s, p) for k, s, p, subm in _CUBIC if not subm])
def test_restated_layers_equal_the_brute_force_and_the_scatter_rule_books(k, s, p):
    """The per-axis forms (and the cubic ones again) against the rule book written from the definition i = o*s - p + t and the one
    built the way spconv does (per-axis getValidOutPos): active sets and tables identical, values to fp64 rounding."""
    shape = (12, 10, 15)
    coors, feats, w = _case(shape, 3, 4, k, seed=13)
    x, mask = R.to_dense(feats, coors, shape)
    y, m2 = R.conv_layer(x, mask, w, k, s, p, False)
    got, got_c = _dense_rows(y, m2)
    vb, cb, sb = R.rulebook_conv(feats, coors, shape, w, k, s, p, book=R.brute_book)
    vs, cs, ss = R.rulebook_conv(feats, coors, shape, w, k, s, p, book=R.scatter_book)
    assert tuple(sb) == tuple(ss) == tuple(y.shape[2:])
    assert np.array_equal(got_c, cb) and np.array_equal(cb, cs), "active sets differ"
    assert np.array_equal(R.brute_book(coors, shape, k, s, p)[1], R.scatter_book(coors, shape, k, s, p)[1]), "rule books differ"
    lin = (cb[:, 0] * sb[1] + cb[:, 1]) * sb[2] + cb[:, 2]
    assert np.array_equal(R.active_outputs(coors, shape, k, s, p), lin), "the vectorised active set differs"
    scale = max(1.0, float(vb.abs().max()))
    assert float((got - vb).abs().max()) <= 1e-12 * scale and float((vb - vs).abs().max()) <= 1e-12 * scale


def test_an_input_that_reaches_no_output_is_dropped_by_all_three_forms():
    """Padding 0 on an even extent: z = 5 of a 6-plane grid lies in no window of k3 / s2 / p(0,1,1)."""
    shape, k, s, p = (6, 7, 7), (3, 3, 3), (2, 2, 2), (0, 1, 1)
    coors = np.asarray([[5, 3, 3], [1, 2, 2]], np.int32)
    outs, table, osz = R.brute_book(coors, shape, k, s, p)
    assert osz == (2, 4, 4) and (table != 0).all() and (table == 1).any()
    assert R.valid_out_pos((5, 3, 3), k, s, p, osz) == []
    assert np.array_equal(R.scatter_book(coors, shape, k, s, p)[1], table)
    _, m2 = R.conv_layer(*R.to_dense(torch.ones(2, 1, dtype=torch.float64), coors, shape), torch.ones(3, 3, 3, 1, 1, dtype=torch.float64), k, s, p,
                         False)
    assert np.array_equal(m2[0, 0].nonzero().numpy(), outs)
    assert len(R.brute_book(coors[:1], shape, k, s, p)[0]) == 0


# ----------------------------------------------------------------------------- refusals
def test_refused_variants_name_themselves():
    cfg = _config_cfg()
    with pytest.raises(NotImplementedError, match="order"):
        SparseEncoderHD(**dict(cfg, order=('act', 'conv', 'norm')))
    with pytest.raises(NotImplementedError, match="keep_depth"):
        SparseEncoderHD(**dict(cfg, keep_depth=False))
    with pytest.raises(NotImplementedError, match="fp16_enabled"):
        SparseEncoderHD(**dict(cfg, fp16_enabled=True))
    with pytest.raises(NotImplementedError, match="GN"):
        SparseEncoderHD(**dict(cfg, norm_cfg=dict(type='GN', num_groups=4)))
    with pytest.raises(NotImplementedError, match="SyncBN"):
        SparseEncoderHD(**dict(cfg, norm_cfg=dict(type='SyncBN')))
    with pytest.raises(AssertionError):
        SparseEncoderHD(**dict(cfg, block_type='bottleneck'))
    m = SparseEncoderHD(**cfg)
    f, c = torch.zeros(3, 4), torch.zeros(3, 4, dtype=torch.int32)
    with pytest.raises(NotImplementedError, match="train"):
        m.train()(f, c, 1)
    m.eval()
    with pytest.raises(NotImplementedError, match="batch size 2"):
        m(f, c, 2)
    with pytest.raises(_lib.CooccError, match="GPU only"):
        m(f, c, 1)


def test_feature_width_mismatch_states_both_numbers():
    """coocc_lidar.py pairs HardSimpleVFE(num_features=5) with in_channels=4: refused, never sliced."""
    m = SparseEncoderHD(**_config_cfg()).eval()
    with pytest.raises(ValueError, match=r"5 channels.*in_channels = 4"):
        m(torch.zeros(3, 5), torch.zeros(3, 3, dtype=torch.int32), 1)


def test_packs_permute_v1_weights_into_the_engines_tap_major_layout():
    """[kd,kh,kw,Cin,Cout] -> [Cout, taps, Cin] through core.PackedConv / lib_pack; channels zero-padded with exact-zero epilogue."""
    conv = lidar_hd.SparseConvV1(3, 5, (1, 3, 3), stride=(1, 2, 2), padding=(0, 1, 1))
    bn = torch.nn.BatchNorm1d(5, eps=1e-3).eval()
    bn.load_state_dict(synth.random_state_dict(bn.state_dict(), seed=2))
    pc = conv.packed(bn, 4, 8)
    assert (pc.Cout, pc.Cin, pc.taps) == (8, 4, 9)
    w = pc._w_taps                                                       # [Cout, Cin, taps] on the host
    want = conv.weight.detach().permute(4, 3, 0, 1, 2).reshape(5, 3, 9)
    assert torch.equal(w[:5, :3], want) and float(w[5:].abs().max()) == 0 and float(w[:, 3:].abs().max()) == 0
    assert float(pc.scale[5:].abs().max()) == 0 and float(pc.bias[5:].abs().max()) == 0
    s = bn.weight.double() / torch.sqrt(bn.running_var.double() + 1e-3)
    assert torch.allclose(pc.scale[:5].double(), s, rtol=1e-6)


# ----------------------------------------------------------------------------- the C boundary
def test_per_axis_entry_points_validate_before_launching():
    lib = _lib.load()
    one = ctypes.c_void_p(16)
    k3, s2, p011 = (3, 3, 3), (2, 2, 2), (0, 1, 1)
    assert lib.coocc_sparse_conv_table3(one, 4, 6, 7, 7, *k3, *s2, *p011, None, one, None) == -1
    assert b"sparse_conv_table3" in lib.coocc_last_error()
    assert lib.coocc_sparse_conv_table3(one, 4, 6, 7, 7, 3, 0, 3, *s2, *p011, one, one, None) == -1 and b"kernel" in lib.coocc_last_error()
    assert lib.coocc_sparse_conv_table3(one, 4, 6, 7, 7, *k3, 2, 2, 0, *p011, one, one, None) == -1 and b"stride" in lib.coocc_last_error()
    assert lib.coocc_sparse_conv_table3(one, 4, 65, 8000, 8000, *k3, *s2, *p011, one, one, None) == -1 and b"2^31" in lib.coocc_last_error()
    assert lib.coocc_sparse_conv_table3(one, -1, 6, 7, 7, *k3, *s2, *p011, one, one, None) == -1
    assert lib.coocc_sparse_down_flags3(one, 4, 6, 7, 7, *k3, *s2, *p011, 2, 4, 4, None, None) == -1
    assert b"sparse_down_flags3" in lib.coocc_last_error()
    # the output extents are checked against (in + 2 p - k) / s + 1 per axis: pad 0 on z gives 2 planes, not 3
    assert lib.coocc_sparse_down_flags3(one, 4, 6, 7, 7, *k3, *s2, *p011, 3, 4, 4, one, None) == -1 and b"output grid" in lib.coocc_last_error()
    assert lib.coocc_sparse_down_flags3(one, 4, 6, 7, 7, *k3, *s2, 0, -1, 1, 2, 4, 4, one, None) == -1 and b"padding" in lib.coocc_last_error()
    assert lib.coocc_sparse_down_flags3(one, 4, 2, 7, 7, *k3, *s2, *p011, 0, 4, 4, one, None) == -1       # kernel larger than the padded extent
    assert lib.coocc_sparse_down_flags3(one, 4, 65, 8000, 8000, *k3, *s2, *p011, 32, 4000, 4000, one, None) == -1 and b"2^31" in lib.coocc_last_error()


# ----------------------------------------------------------------------------- opt-in wiring
def test_the_opt_in_default_leaves_the_middle_encoder_upstream():
    det = pkg.build_detector(synth.model_cfg_lidar(), external_encoders=True)
    assert det.pts_middle_encoder is None and det.sparse_encoder_hd is False
    assert "SparseEncoderHD" not in lidar.MIDDLE_ENCODERS
    with pytest.raises(NotImplementedError):
        pkg.build_detector(synth.model_cfg_lidar())                                     # not deferred: refused at construction, as before
    det = pkg.build_detector(synth.model_cfg_lidar(), sparse_encoder_hd=True)
    assert isinstance(det.pts_middle_encoder, SparseEncoderHD) and det.pts_middle_encoder.out_shape() == (8, 100, 100)
    assert any(k.startswith("pts_middle_encoder.conv_input.0.") for k in det.state_dict())
    # COOCC_Ray takes the key too, but its extract_pts_feat reads the 8x / 4x encoders' dict: the combination refuses by name
    with pytest.raises(NotImplementedError, match="COOCC_Ray_L"):
        pkg.build_detector(dict(synth.model_cfg(), pts_middle_encoder=synth.model_cfg_lidar()["pts_middle_encoder"]), sparse_encoder_hd=True)
    # the 8x encoder's route is untouched by the option
    with8x = pkg.build_detector(dict(synth.model_cfg(), **synth.lidar_cfg()), sparse_encoder_hd=True)
    assert isinstance(with8x.pts_middle_encoder, lidar.SparseLiDAREnc8x)


class _FakeRegistry:
    def __init__(self):
        self.module_dict = {}

    def register_module(self, name=None, force=False, module=None):
        if name in self.module_dict and not force:
            raise KeyError(name)
        self.module_dict[name] = module
        return module


def test_register_into_mmdet_swaps_sparse_encoder_hd_only_on_request(monkeypatch):
    mb, m3b = types.ModuleType("mmdet.models.builder"), types.ModuleType("mmdet3d.models.builder")
    mb.DETECTORS = _FakeRegistry()
    for n in ("BACKBONES", "NECKS", "HEADS", "FUSION_LAYERS", "VOXEL_ENCODERS", "MIDDLE_ENCODERS"):
        setattr(m3b, n, _FakeRegistry())
    m3b.MIDDLE_ENCODERS.module_dict["SparseEncoderHD"] = "reference class"
    for name, mod in (("mmdet", types.ModuleType("mmdet")), ("mmdet.models", types.ModuleType("mmdet.models")),
                      ("mmdet.models.builder", mb), ("mmdet3d", types.ModuleType("mmdet3d")),
                      ("mmdet3d.models", types.ModuleType("mmdet3d.models")), ("mmdet3d.models.builder", m3b)):
        monkeypatch.setitem(sys.modules, name, mod)
    sys.modules["mmdet.models"].builder = mb
    sys.modules["mmdet3d.models"].builder = m3b
    assert pkg.register_into_mmdet() is True
    assert m3b.MIDDLE_ENCODERS.module_dict["SparseEncoderHD"] == "reference class"
    assert m3b.MIDDLE_ENCODERS.module_dict["SparseLiDAREnc8x"] is pkg.SparseLiDAREnc8x
    assert pkg.register_into_mmdet(sparse_encoder_hd=True) is True
    assert m3b.MIDDLE_ENCODERS.module_dict["SparseEncoderHD"] is SparseEncoderHD
    assert "COOCC_Ray" not in mb.DETECTORS.module_dict
