"""csrc/head_tail_h2.hip: the two two-layer pointwise chains that end OccHead's coarse stage, one launch each with the hidden
activation in LDS, through the C ABI.

* ``coocc_head_pred_h2`` against the four launches it replaces (``coocc_conv_fwd`` of the merged occ_pred_conv[0] | Q layer ->
  ``coocc_rows_to_h2`` of the 64 hidden channels -> ``coocc_conv_fwd`` of occ_pred_conv[3] -> ``coocc_argmax_flags``) and
  ``coocc_head_soft_h2`` against its two ``coocc_conv_fwd`` launches: BIT-equal logits, Q, flags, wlogit and (on request) hidden
  columns, at ragged row counts around the 128-row tile and its 32- / 64-row sub-blocks, with a device-side row count below the
  capacity (rows past it keep their sentinel), 1..32 output columns, an input row stride above 128 channels, all-zero rows,
  exact ties and a last-class maximum for the flag, and at a row count large enough that the reference's first layer is the
  pointwise kernel k_gemm_h2p (>= 256 tiles) instead of k_gemm_h2w.
* against float64: the fused kernels' error may not exceed the layer-by-layer path's error against the same reference.
* the operand-range guard: a hidden activation outside the f16 range raises the flag in both forms.
* OccHead.forward_coarse_rows on a 16 x 16 x 4 grid with the switch on and off: every output bit-equal.
"""
import pytest
import torch

from co_occ_amd import _lib, core
from co_occ_amd._lib import call, ptr
from util import errors, kernels

pytestmark = pytest.mark.gpu

SENTINEL = -777.25
_I32 = torch.int32


def _bits(a, b):
    """Bit patterns equal (NaN == NaN, -0 != +0)."""
    if a.is_floating_point():
        return a.shape == b.shape and torch.equal(a.contiguous().view(_I32), b.contiguous().view(_I32))
    return torch.equal(a, b)


def _layers(dev, nout, seed, kind="pred", bias2=True):
    """(layer 1 with folded BN, layer 2) of one chain with seeded weights; pred: 128 -> 128 (ReLU on 64) -> nout, soft: 128 -> 64 -> nout."""
    g = torch.Generator().manual_seed(seed)
    n1 = 128 if kind == "pred" else 64
    l1 = core.PackedConv((torch.randn(n1, 128, 1, 1, 1, generator=g) * 0.09).to(dev), ksize=1)
    l1.scale = (0.5 + torch.rand(n1, generator=g)).to(dev).contiguous()
    l1.bias = (torch.randn(n1, generator=g) * 0.3).to(dev).contiguous()
    b = (torch.randn(nout, generator=g) * 0.2).to(dev) if bias2 else None
    l2 = core.PackedConv((torch.randn(nout, 64, 1, 1, 1, generator=g) * 0.12).to(dev), bias=b, ksize=1)
    return l1, l2


def _input(dev, rows, stride, seed):
    """fp32 rows [rows, stride] (a fifth of them all zero) and their H2 rows."""
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(rows, stride, generator=g) * (torch.rand(rows, 1, generator=g) < 0.8).float()
    x = x.to(dev)
    xh = torch.empty_like(x)
    call("coocc_rows_to_h2", ptr(x), stride, rows, stride, 1.0, ptr(xh))
    return x, xh


def _gemm(dev, in_, in_stride, w, pc, rows, Cin, out, relu, mfma):
    d = core.conv_desc(dev, in_=ptr(in_), w=ptr(w), out=ptr(out), scale=ptr(pc.scale), bias=ptr(pc.bias), M=rows, Cin=Cin, Cout=pc.Cout, taps=1,
                       in_stride=in_stride, out_stride=out.shape[1], B=1, Xi=rows, Yi=1, Zi=1, Xo=rows, Yo=1, Zo=1, ksize=1, stride=1,
                       relu=relu, mfma_dtype=mfma, alpha=1.0)
    _lib.conv_fwd(d, dev)


def _buffers(dev, cap, l1, l2):
    f = lambda *s: torch.full(s, SENTINEL, device=dev)
    return dict(hid=f(cap, l1.Cout), out=f(cap, l2.Cout), flags=torch.full((cap,), 9, device=dev, dtype=torch.uint8))


def pred_layerwise(dev, xh, stride, rows, cap, l1, l2, empty_idx):
    """Today's four launches on the first ``rows`` rows of capacity-sized, sentinel-filled buffers."""
    o = _buffers(dev, cap, l1, l2)
    _gemm(dev, xh, stride, l1.h2_pack(), l1, rows, 128, o["hid"], 64, 3)
    hh = torch.empty(rows, 64, device=dev)
    call("coocc_rows_to_h2", ptr(o["hid"]), 128, rows, 64, 1.0, ptr(hh))
    _gemm(dev, hh, 64, l2.h2_pack(), l2, rows, 64, o["out"], 0, 3)
    call("coocc_argmax_flags", ptr(o["out"]), rows, l2.Cout, l2.Cout, empty_idx, ptr(o["flags"]))
    return o


def pred_fused(dev, xh, stride, cap, l1, l2, empty_idx, count=None, hidden=True):
    o = _buffers(dev, cap, l1, l2)
    cnt = torch.tensor([count], device=dev, dtype=_I32) if count is not None else None
    call("coocc_head_pred_h2", ptr(xh), stride, cap, ptr(cnt), ptr(l1.h2_pack()), ptr(l1.scale), ptr(l1.bias), ptr(o["hid"]), 128, int(hidden),
         ptr(l2.h2_pack()), ptr(l2.bias), l2.Cout, ptr(o["out"]), l2.Cout, empty_idx, ptr(o["flags"]))
    return o


def soft_layerwise(dev, xh, stride, rows, cap, l1, l2):
    o = _buffers(dev, cap, l1, l2)
    _gemm(dev, xh, stride, l1.h2_pack(), l1, rows, 128, o["hid"], 1, 3)
    _gemm(dev, o["hid"], 64, l2.w, l2, rows, 64, o["out"], 0, 0)
    return o


def soft_fused(dev, xh, stride, cap, l1, l2, count=None, hidden=True):
    o = _buffers(dev, cap, l1, l2)
    cnt = torch.tensor([count], device=dev, dtype=_I32) if count is not None else None
    call("coocc_head_soft_h2", ptr(xh), stride, cap, ptr(cnt), ptr(l1.h2_pack()), ptr(l1.scale), ptr(l1.bias), ptr(o["hid"]) if hidden else None,
         64 if hidden else 0, ptr(l2.w), ptr(l2.bias), l2.Cout, ptr(o["out"]), l2.Cout)
    return o


def _same_pred(a, b, hidden=True):
    assert _bits(a["out"], b["out"]), "logits differ"
    assert _bits(a["hid"][:, 64:], b["hid"][:, 64:]), "Q differs"
    assert torch.equal(a["flags"], b["flags"]), "flags differ"
    if hidden:
        assert _bits(a["hid"][:, :64], b["hid"][:, :64]), "hidden columns differ"
    else:
        assert bool((b["hid"][:, :64] == SENTINEL).all()), "hidden columns written without being asked for"


# (rows, capacity, device count or None, input stride in channels)
SHAPES = [(1, 1, None, 128), (63, 63, None, 128), (64, 64, None, 128), (65, 65, None, 128), (127, 127, None, 128), (128, 128, None, 128),
          (129, 129, None, 128), (300, 300, None, 128), (130, 384, 130, 128), (300, 300, None, 160), (32769, 32769, None, 128)]


@pytest.mark.parametrize("rows,cap,count,stride", SHAPES)
def test_pred_chain_is_bit_equal_to_its_four_launches(dev, rows, cap, count, stride):
    for ncls in ((1, 17, 18, 32) if rows in (129, 300) and stride == 128 else (17,)):
        l1, l2 = _layers(dev, ncls, 100 + ncls, bias2=ncls != 18)
        _, xh = _input(dev, cap, stride, rows + ncls)
        want = pred_layerwise(dev, xh, stride, rows, cap, l1, l2, 0)
        _same_pred(want, pred_fused(dev, xh, stride, cap, l1, l2, 0, count))
        _same_pred(want, pred_fused(dev, xh, stride, cap, l1, l2, 0, count, hidden=False), hidden=False)
        assert bool((want["out"][rows:] == SENTINEL).all()) and bool((want["flags"][rows:] == 9).all())
    torch.cuda.synchronize()
    core.check_h2_overflow()


@pytest.mark.parametrize("rows,cap,count,stride", SHAPES)
def test_soft_chain_is_bit_equal_to_its_two_launches(dev, rows, cap, count, stride):
    for L in ((1, 4, 32) if rows in (129, 300) and stride == 128 else (4,)):
        l1, l2 = _layers(dev, L, 200 + L, kind="soft", bias2=L != 1)
        _, xh = _input(dev, cap, stride, rows + L)
        want = soft_layerwise(dev, xh, stride, rows, cap, l1, l2)
        got = soft_fused(dev, xh, stride, cap, l1, l2, count)
        assert _bits(want["out"], got["out"]), "wlogit differs"
        assert _bits(want["hid"], got["hid"]), "hidden columns differ"
        got = soft_fused(dev, xh, stride, cap, l1, l2, count, hidden=False)
        assert _bits(want["out"], got["out"]), "wlogit differs (hidden not requested)"
    torch.cuda.synchronize()
    core.check_h2_overflow()


@pytest.mark.parametrize("case", ["ties", "last"])
def test_flags_resolve_ties_and_a_last_class_maximum_as_the_argmax_kernel(dev, case):
    """Classes 0 and 5 share their weights and bias (exact ties, often at the maximum: the first one wins) / the last class carries
    a bias that makes it the maximum of every row; both with the empty class on either side of the tie."""
    ncls, rows = 17, 300
    l1, l2 = _layers(dev, ncls, 7)
    w = l2._w_taps.clone()                                 # [ncls, 64, 1] on the host
    b = l2.bias.cpu().clone()
    if case == "ties":
        w[1:] *= 0.02                                      # the other classes: logits near their bias of -1
        b[:] = -1.0
        b[0] = 0.5
        w[5], b[5] = w[0], b[0]
    else:
        b[ncls - 1] = 100.0
    l2 = core.PackedConv(w.view(ncls, 64, 1, 1, 1).to(dev), bias=b.to(dev), ksize=1)
    _, xh = _input(dev, rows, 128, 3)
    for empty_idx in (0, 5, ncls - 1):
        want = pred_layerwise(dev, xh, 128, rows, rows, l1, l2, empty_idx)
        got = pred_fused(dev, xh, 128, rows, l1, l2, empty_idx)
        _same_pred(want, got)
        assert torch.equal(got["flags"].bool(), got["out"].argmax(1) != empty_idx) or case == "ties"      # torch does not promise the first maximum
    lg = got["out"]
    if case == "ties":
        assert _bits(lg[:, 0], lg[:, 5])
        assert int((lg[:, 0] == lg.max(1).values).sum()) > rows // 4, "the tie is rarely the maximum: the case tests nothing"
        assert int(pred_fused(dev, xh, 128, rows, l1, l2, 5)["flags"][lg[:, 0] == lg.max(1).values].min()) == 1      # class 0 wins, not 5
    else:
        assert bool((lg.argmax(1) == ncls - 1).all())


def test_fused_chains_against_float64_within_the_layerwise_paths_error(dev):
    """300 rows per kernel against the float64 evaluation of the same two layers: the bound is the error of the launches the
    kernel replaces against the same reference (the fused kernel is bit-equal, so it cannot exceed it)."""
    rows = 300
    for kind, nout in (("pred", 17), ("soft", 4)):
        l1, l2 = _layers(dev, nout, 31, kind=kind)
        x, xh = _input(dev, rows, 128, 17)
        w1 = l1._w_taps[:, :, 0].double()
        hid = (x.cpu().double() @ w1.t()) * l1.scale.cpu().double() + l1.bias.cpu().double()
        hid = torch.relu(hid[:, :64])
        ref = hid @ l2._w_taps[:, :, 0].double().t() + l2.bias.cpu().double()
        if kind == "pred":
            old, new = pred_layerwise(dev, xh, 128, rows, rows, l1, l2, 0), pred_fused(dev, xh, 128, rows, l1, l2, 0)
        else:
            old, new = soft_layerwise(dev, xh, 128, rows, rows, l1, l2), soft_fused(dev, xh, 128, rows, l1, l2)
        e_old, e_new = errors(old["out"], ref), errors(new["out"], ref)
        print("[prec] head tail %-4s fused e_max %.3e e_rms %.3e | layer-by-layer e_max %.3e e_rms %.3e" % ((kind,) + e_new + e_old))
        assert e_new[0] <= e_old[0] and e_new[1] <= e_old[1]
        assert e_old[0] < 1e-5          # ... and that path is an fp32-accurate one (split-f16 operands: ~2^-22 per product)


def test_hidden_activation_outside_the_f16_range_raises_the_guard(dev):
    """Inputs in range, a folded-BN scale of 1e6: the hidden activation leaves the split-f16 operand range -- the conversion pass
    of the layer-by-layer form flags it, and so must the kernel that keeps it in LDS."""
    rows = 200
    l1, l2 = _layers(dev, 17, 5)
    _, xh = _input(dev, rows, 128, 9)
    torch.cuda.synchronize()
    core.check_h2_overflow()                      # clean start: the inputs are in range
    pred_fused(dev, xh, 128, rows, l1, l2, 0)
    torch.cuda.synchronize()
    core.check_h2_overflow()                      # ordinary activations: no flag
    l1.scale = l1.scale * 1.0e6
    for form in (lambda: pred_layerwise(dev, xh, 128, rows, rows, l1, l2, 0), lambda: pred_fused(dev, xh, 128, rows, l1, l2, 0, hidden=False)):
        form()
        torch.cuda.synchronize()
        with pytest.raises(_lib.CooccError):
            core.check_h2_overflow()
        core.check_h2_overflow()                  # the check cleared the flag


def test_forward_coarse_rows_is_bit_equal_with_the_switch_on_and_off(dev, monkeypatch):
    """OccHead.forward_coarse_rows on a 16 x 16 x 4 grid (four levels, soft weights, the merged occ_pred_conv[0] | Q layer) with the
    one-launch tails and with the layer-by-layer launches: features, twin, Q, soft-weighted mix, logits and flags bit-equal.  The
    split-f16 threshold is lowered so that the 1024-row layers take the kernels they take at the flagship's 80 000 rows."""
    import co_occ_amd as pkg
    import co_occ_amd.synth as synth
    from co_occ_amd import head as H
    monkeypatch.setattr(core, "H2_DIRECT_MIN_FLOPS", 1.0e6)      # 128 -> 128 / 64 and 64 -> 17 on the split-f16 engine, 64 -> 4 not
    head = pkg.build_head(dict(type='OccHead', norm_cfg=dict(type='BN3d'), soft_weights=True, cascade_ratio=2, sample_from_voxel=True,
                               sample_from_img=True, final_occ_size=[32, 32, 8], fine_topk=15000, empty_idx=0, num_level=4,
                               in_channels=[256] * 4, out_channel=17, point_cloud_range=[-50, -50, -5.0, 50, 50, 3.0]))
    head.load_state_dict(synth.random_state_dict(head.state_dict(), seed=21))
    head = head.to(dev).eval()
    g = torch.Generator().manual_seed(4)
    feats = [torch.randn(1, 256, *s, generator=g).to(dev) for s in ((16, 16, 4), (8, 8, 2), (4, 4, 1), (2, 2, 1))]
    res = {}
    for on in (True, False):
        monkeypatch.setattr(H, "HEAD_TAIL_FUSED", on)
        with torch.no_grad(), kernels() as names:
            out, occ = head.forward_coarse_rows(feats)
            flags = occ.aux["flags"] if occ.aux else None
            if flags is None:
                flags = torch.empty(occ.t.shape[0], device=dev, dtype=torch.uint8)
                call("coocc_argmax_flags", ptr(occ.t), occ.t.shape[0], occ.C, occ.stride, 0, ptr(flags))
        assert (("k_head_pred_h2" in names) and ("k_head_soft_h2" in names)) == on, sorted(names)
        res[on] = [out.t, out.h2, out.aux["q"], occ.t, flags]
    torch.cuda.synchronize()
    core.check_h2_overflow()
    for a, b, what in zip(res[True], res[False], ("out_voxel_feats", "their H2 twin", "Q", "logits", "flags")):
        assert _bits(a, b), what
    assert 0 < int(res[True][4].sum()) < res[True][4].numel(), "all voxels on one side of the foreground test: the flags test nothing"
