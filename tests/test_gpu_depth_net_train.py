"""DepthNet's training path on the HIP engine (co_occ_amd/depth_net.py, the training kernels of csrc/depthnet.hip) against float64.

Judging rule: every tensor is judged by ``util.assert_precise`` against the float64 torch-autograd result of the train-mode
restatement (tests/ref_depth_net_train.py; tests/ref_depth_net.py for the single operations), with the float32 CPU autograd of the
same restatement as the fp32 anchor (and, where the kernel under test is a split-f16 GEMM, the split emulation of that GEMM) and the
project's C_MAX / C_RMS.  That holds for the whole-block tensors (train-mode ASPP, the whole module) as well: none needed the looser
``util.assert_close`` (DESIGN.md 10 records the measured ratios).

The sampler's offsets are multiples of 2^-10 with |off| <= 32 wherever the offset gradient is judged: the fp32 sample position then
equals the float64 one, so ``floor`` -- where the offset gradient is discontinuous -- cannot differ between kernel and judge."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import co_occ_amd as pkg
import ref_depth_net as R
import ref_depth_net_train as T
import util
from co_occ_amd import core, depth_net as dn, synth
from co_occ_amd._lib import call, ptr
from co_occ_amd.core import Rows
from util import TOL, assert_precise, gemm_refs, precision, rel_err, split_mm

pytestmark = pytest.mark.gpu
G = 4


def rows_of(x):
    """[BN,C,H,W] -> channels-last rows [BN*H*W, C]."""
    return x.permute(0, 2, 3, 1).reshape(-1, x.shape[1]).contiguous()


def as_rows(x, dev):
    BN, C, H, W = x.shape
    return Rows(rows_of(x).float().to(dev), BN, H, W, 1, C)


def bits_equal(a, b):
    return a.shape == b.shape and torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


def leaf(t, dtype):
    """A fresh leaf of ``t`` in ``dtype`` (``t.to`` of the same dtype would hand back ``t`` itself)."""
    return t.detach().to(dtype).clone().requires_grad_(True)


def quant(off):
    """Multiples of 2^-10 in [-32, 32]."""
    return (off.clamp(-32, 32) * 1024).round() / 1024


class Judge:
    """Collects every miss of a test before failing, so that one run reports all of a block's tensors."""

    def __init__(self):
        self.fails = []

    def precise(self, got, r64, r32, what, rs=None):
        st = precision(got, r64, r32, rs, what=what)
        if not st["ok"]:
            self.fails.append("%s: ratio %.2f / %.2f" % (what, st["ratio_max"], st["ratio_rms"]))
        return st

    def done(self):
        assert not self.fails, "\n".join(self.fails)


# ------------------------------------------------------------------ 1. the sampler's backward alone
def _offsets(kind, BN, H, W, g):
    if kind == "zero":
        return torch.zeros(BN, 18, H, W)
    if kind == "integer":                       # the right-derivative rule
        return quant((torch.randn(BN, 18, H, W, generator=g) * 3).round())
    if kind == "fractional":                    # fractional parts in [1/8, 7/8]
        return quant((torch.randn(BN, 18, H, W, generator=g) * 3).floor() + 0.125 + 0.75 * torch.rand(BN, 18, H, W, generator=g))
    if kind == "far":                           # many taps outside
        return quant(torch.randn(BN, 18, H, W, generator=g) * 20)
    assert kind == "hand"
    off = quant(torch.randn(BN, 18, H, W, generator=g))
    ys = torch.arange(H, dtype=torch.float32).view(1, H, 1)
    xs = torch.arange(W, dtype=torch.float32).view(1, 1, W)
    off[:, 0] = -0.5 - (ys - 1)                 # tap 0 (i = 0): row position -0.5: between the padding row and row 0
    off[:, 2] = (H - 0.25) - (ys - 1)           # tap 1 (i = 0): row position H - 0.25: between the last row and the padding
    off[:, 9] = -0.75 - xs                      # tap 4 (j = 1): column position -0.75
    off[:, 11] = (W - 0.5) - (xs + 1)           # tap 5 (j = 2): column position W - 0.5
    off[:, 1], off[:, 3], off[:, 8], off[:, 10] = 1.0, 0.0, 0.0, 0.0       # their other coordinate: the pixel's own column / row
    return off


def _sampler_ref(x, off, dcols, dtype):
    xx, oo = leaf(x, dtype), leaf(off, dtype)
    cols = R.cols_as_rows(R.dcn_cols_gather(xx, oo), G)
    (cols * dcols.to(dtype)).sum().backward()
    return rows_of(xx.grad), rows_of(oo.grad)


def _sampler_dev(dev, x, off, dcols, chunks, stride=20):
    BN, C, H, W = x.shape
    M = BN * H * W
    xr = as_rows(x, dev)
    offr = F.pad(rows_of(off).float(), (0, stride - 18), value=7.0).to(dev)          # the columns past 18 are never read
    dx = torch.zeros(M, C, device=dev)
    doff = torch.full((M, stride), float("nan"), device=dev)
    for m0, n in chunks:
        dc = dcols[:, m0:m0 + n].contiguous().float().to(dev)
        call("coocc_dcn_cols_bwd", xr.data(), xr.stride, ptr(offr), stride, BN, H, W, C, G, m0, n, ptr(dc), ptr(dx),
             ptr(doff, offset=m0 * stride))
    return dx.cpu(), doff.cpu()


@pytest.mark.parametrize("kind", ["zero", "integer", "fractional", "far", "hand"])
@pytest.mark.parametrize("C,H,W,chunks", [(32, 5, 7, ((0, 27), (27, 27), (54, 16))), (288, 6, 5, ((0, 23), (23, 23), (46, 14)))])
def test_sampler_backward(dev, C, H, W, chunks, kind):
    BN = 2
    M, K = BN * H * W, 9 * C // G
    assert sum(n for _, n in chunks) == M and all(M % n for _, n in chunks)
    g = torch.Generator().manual_seed(C + H + len(kind))
    x = torch.randn(BN, C, H, W, generator=g)
    dcols = torch.randn(G, M, K, generator=g)
    off = _offsets(kind, BN, H, W, g)
    assert torch.equal(off, quant(off)) and float(off.abs().max()) <= 32
    dx64, do64 = _sampler_ref(x, off, dcols, torch.float64)
    dx32, do32 = _sampler_ref(x, off, dcols, torch.float32)
    dx, doff = _sampler_dev(dev, x, off, dcols, chunks)
    what = "C=%d %dx%d %s" % (C, H, W, kind)
    assert float(doff[:, 18:].abs().max()) == 0.0, "doff columns from 18 up are 0"
    j = Judge()
    j.precise(doff[:, :18], do64, do32, "sampler doff " + what)
    j.precise(dx, dx64, dx32, "sampler dx " + what)
    py, px = R.tap_positions(off.double())
    outside = rows_of((py <= -1) | (py >= H) | (px <= -1) | (px >= W))                # [M, 9]
    if kind == "far":
        assert 0.2 < float(outside.double().mean()) < 1.0
    if kind == "hand":
        assert not outside[:, [0, 1, 4, 5]].any()                                      # in (-1, 0) and (H-1, H): inside the cut
    if outside.any():
        assert float(doff[:, :18].reshape(M, 9, 2)[outside].abs().max()) == 0.0, "a tap outside the map has an exactly zero offset gradient"
    dx2, doff2 = _sampler_dev(dev, x, off, dcols, chunks)
    assert bits_equal(doff, doff2), "doff is deterministic"
    # adjoint identity in float64 on the host: <dcols, cols(x)> = <dx, x>.  A target element receives at most one term per (pixel,
    # tap) of its camera -- n <= 9 H W fp32 products, each rounded and added in fp32: |error| <= (n + 1) 2^-24 sum |terms|
    cols = R.cols_as_rows(R.dcn_cols_gather(x.double(), off.double()), G)
    lhs, rhs = float((cols * dcols.double()).sum()), float((dx.double() * rows_of(x).double()).sum())
    mass = float((R.cols_as_rows(R.dcn_cols_gather(x.double().abs(), off.double()), G) * dcols.double().abs()).sum())
    assert abs(lhs - rhs) <= (9 * H * W + 1) * 2.0 ** -24 * mass, "adjoint identity %s: %.6e vs %.6e" % (what, lhs, rhs)
    j.done()


def test_sampler_backward_of_a_nan_offset_is_zero(dev):
    BN, C, H, W = 2, 32, 5, 7
    g = torch.Generator().manual_seed(3)
    x, dcols = torch.randn(BN, C, H, W, generator=g), torch.randn(G, 70, 72, generator=g)
    off = torch.zeros(BN, 18, H, W)
    off[:, 8:10] = float("nan")                                     # the centre tap
    dx, doff = _sampler_dev(dev, x, off, dcols, ((0, 70),))
    assert float(doff[:, 8:10].abs().max()) == 0.0 and bool(torch.isfinite(doff).all()) and bool(torch.isfinite(dx).all())
    dcols0 = dcols.clone()
    dcols0.view(G, 70, 9, 8)[:, :, 4] = 0                           # dx equals that of the other eight taps alone
    dx64, _ = _sampler_ref(x, torch.zeros(BN, 18, H, W), dcols0, torch.float64)
    dx32, _ = _sampler_ref(x, torch.zeros(BN, 18, H, W), dcols0, torch.float32)
    assert_precise(dx, dx64, dx32, what="sampler dx, NaN centre tap")


# ------------------------------------------------------------------ 2. DcnRowsFn
def _dcn_case(mid):
    BN, H, W = 2, 6, 8
    g = torch.Generator().manual_seed(mid)
    x = torch.randn(BN, mid, H, W, generator=g)
    off = quant(torch.randn(BN, 18, H, W, generator=g) * 2)
    w = torch.randn(mid, mid // G, 3, 3, generator=g) / (3 * (mid // G) ** 0.5)
    w = w * torch.tensor([1.0, 2.0, 0.5, 4.0]).repeat_interleave(mid // G).view(mid, 1, 1, 1)
    r = torch.randn(BN, mid, H, W, generator=g)
    refs = {}
    for dt in (torch.float64, torch.float32):
        xx, oo, ww = (leaf(t, dt) for t in (x, off, w))
        out = R.dcn(xx, oo, ww, form="gather")
        (out * r.to(dt)).sum().backward()
        refs[dt] = dict(out=rows_of(out.detach()), dx=rows_of(xx.grad), doff=rows_of(oo.grad), dw=ww.grad)
    return x, off, w, r, refs


def _dcn_dev(dev, x, off, w, r):
    xd = rows_of(x).to(dev).requires_grad_(True)
    od = F.pad(rows_of(off), (0, 2)).to(dev).requires_grad_(True)
    wd = w.to(dev).requires_grad_(True)
    with util.kernels() as names:
        out = dn.DcnRowsFn.apply(xd, od, wd, tuple(x.shape[:1]) + tuple(x.shape[2:]), G)
        out.backward(rows_of(r).to(dev))
    return dict(out=out.detach().cpu(), dx=xd.grad.cpu(), doff=od.grad.cpu(), dw=wd.grad.cpu()), names


@pytest.mark.parametrize("mid", [32, 128])
def test_dcn_rows_fn(dev, mid, monkeypatch):
    x, off, w, r, refs = _dcn_case(mid)
    r64, r32 = refs[torch.float64], refs[torch.float32]
    K = 9 * mid // G
    monkeypatch.setattr(dn, "DCN_CHUNK_ROWS", 40)                   # 96 rows: chunks of 40, 40, 16
    got, names = _dcn_dev(dev, x, off, w, r)
    h2 = any(n.startswith("k_gemm_h2 dcn_fwd") for n in names)
    assert h2 == (K % 32 == 0 and core.CONV_ENGINE == "h2"), names                 # K = 72: fp32 MFMA; K = 288: split-f16
    assert sum(v for n, v in names.items() if n == "k_dcn_cols_bwd") == 3, names
    rs = None
    if h2:
        c32 = R.cols_as_rows(R.dcn_cols_gather(x, off), G)
        cg = mid // G
        wg = w.reshape(G, cg, cg, 9).permute(0, 3, 2, 1).reshape(G, 9 * cg, cg)
        rs = torch.cat([split_mm(c32[k], wg[k]).float() for k in range(G)], 1)
    j = Judge()
    j.precise(got["out"], r64["out"], r32["out"], "DcnRowsFn mid=%d out" % mid, rs)
    j.precise(got["dx"], r64["dx"], r32["dx"], "DcnRowsFn mid=%d dx" % mid)
    j.precise(got["doff"][:, :18], r64["doff"], r32["doff"], "DcnRowsFn mid=%d doff" % mid)
    j.precise(got["dw"], r64["dw"], r32["dw"], "DcnRowsFn mid=%d dW (chunks of 40)" % mid)
    assert float(got["doff"][:, 18:].abs().max()) == 0.0
    monkeypatch.setattr(dn, "DCN_CHUNK_ROWS", 8192)
    whole, names = _dcn_dev(dev, x, off, w, r)
    assert sum(v for n, v in names.items() if n == "k_dcn_cols_bwd") == 1, names
    j.precise(whole["dw"], r64["dw"], r32["dw"], "DcnRowsFn mid=%d dW (one chunk)" % mid)
    assert bits_equal(whole["out"], got["out"]) and bits_equal(whole["doff"], got["doff"])
    core.check_h2_overflow()
    j.done()


# ------------------------------------------------------------------ 3. the dilated branches
def _transpose(table, n_in):
    """[taps, Mo] forward table -> [taps, n_in]: the output row that reads input i through tap t, or -1 (brute force)."""
    inv = np.full((table.shape[0], n_in), -1, np.int64)
    t, o = np.nonzero(table >= 0)
    inv[t, table[t, o]] = o
    return inv


def test_mirrored_rows_are_the_transposed_table(dev):
    BN, H, W, d = 2, 5, 7, 2
    table = dn.neighbour_table(BN, H, W, d, dev)
    tb = table.cpu().numpy()
    assert (tb >= 0).any(1).all()
    assert np.array_equal(_transpose(tb, BN * H * W), table.flip(0).cpu().numpy())
    for taps in ((3, 4, 5), (1, 4, 7)):                              # a symmetric live subset mirrors within itself
        sub = tb[list(taps)]
        assert np.array_equal(_transpose(sub, BN * H * W), sub[::-1])


@pytest.mark.parametrize("d", dn.ASPP_DILATIONS)
def test_dilated_branch_under_train(dev, d):
    BN, H, W, C = 2, 14, 20, 32
    g = torch.Generator().manual_seed(d)
    x = torch.randn(BN, C, H, W, generator=g) * torch.tensor([1.0, 3.0]).view(2, 1, 1, 1)
    w = torch.randn(C, C, 3, 3, generator=g) / (3 * C ** 0.5)
    r = torch.randn(BN, C, H, W, generator=g)
    refs = {}
    for dt in (torch.float64, torch.float32):
        xx, ww = leaf(x, dt), leaf(w, dt)
        out = F.conv2d(xx, ww, dilation=d, padding=d)
        (out * r.to(dt)).sum().backward()
        refs[dt] = (rows_of(out.detach()), rows_of(xx.grad), ww.grad)
    taps = dn.live_taps(H, W, d)
    assert taps == ((3, 4, 5) if d == 18 else dn.ALL_TAPS)           # d = 18 on 14 rows: only the horizontal taps are live
    table = dn.neighbour_table(BN, H, W, d, dev)[list(taps)].contiguous()
    xd = rows_of(x).to(dev).requires_grad_(True)
    wd = torch.nn.Parameter(w.to(dev))
    with util.kernels() as names:
        y = dn.dilated_train(xd, wd, table, taps)
        y.backward(rows_of(r).to(dev))
    assert tuple(wd.grad.shape) == (C, C, 3, 3)
    # split-f16 anchors of the three GEMMs (the engine SparseConvV1Fn runs them on when the training flags allow it)
    xp, rp = F.pad(x.double(), (d, d, d, d)), F.pad(r.double(), (d, d, d, d))
    sh = lambda t, i, j: rows_of(t[:, :, i * d:i * d + H, j * d:j * d + W])
    f64, _, fs = gemm_refs([(sh(xp, t // 3, t % 3), w[:, :, t // 3, t % 3].double().t()) for t in taps])
    d64, _, ds = gemm_refs([(sh(rp, 2 - t // 3, 2 - t % 3), w[:, :, t // 3, t % 3].double()) for t in taps])
    assert float((f64 - refs[torch.float64][0]).abs().max()) <= 1e-12 * float(f64.abs().max())
    assert float((d64 - refs[torch.float64][1]).abs().max()) <= 1e-12 * float(d64.abs().max())
    ws = torch.zeros(C, C, 3, 3, dtype=torch.float64)
    for t in taps:
        ws[:, :, t // 3, t % 3] = split_mm(rows_of(r).t(), sh(xp, t // 3, t % 3).float())
    h2 = any(n.startswith("k_gemm_h2") for n in names)
    j = Judge()
    j.precise(y.detach().cpu(), refs[torch.float64][0], refs[torch.float32][0], "dilated d=%d forward" % d, fs if h2 else None)
    j.precise(xd.grad.cpu(), refs[torch.float64][1], refs[torch.float32][1], "dilated d=%d dx" % d, ds if h2 else None)
    j.precise(wd.grad.cpu(), refs[torch.float64][2], refs[torch.float32][2], "dilated d=%d dW" % d, ws.float() if h2 else None)
    for t in range(9):
        if t not in taps:
            assert float(wd.grad[:, :, t // 3, t % 3].abs().max()) == 0.0, "the weight slice of dead tap %d has an exactly zero gradient" % t
            assert float(refs[torch.float64][2][:, :, t // 3, t % 3].abs().max()) == 0.0
    core.check_h2_overflow()
    j.done()


# ------------------------------------------------------------------ 4. gates, camera means / vectors, dropout
@pytest.mark.parametrize("BN,H,W,C", [(2, 5, 7, 4), (3, 9, 11, 36), (2, 9, 30, 64)])
def test_gate_backward(dev, BN, H, W, C):
    assert (H * W) % 256
    g = torch.Generator().manual_seed(C + BN)
    x = torch.randn(BN, C, H, W, generator=g)
    ga, gb = torch.randn(BN, C, generator=g) * 2, torch.randn(BN, C, generator=g) * 2
    ra, rb = torch.randn(BN, C, H, W, generator=g), torch.randn(BN, C, H, W, generator=g)
    refs = {}
    for dt in (torch.float64, torch.float32):
        xx, a, b = (leaf(t, dt) for t in (x, ga, gb))
        ((xx * torch.sigmoid(a)[:, :, None, None] * ra.to(dt)).sum() + (xx * torch.sigmoid(b)[:, :, None, None] * rb.to(dt)).sum()).backward()
        refs[dt] = (rows_of(xx.grad), a.grad, b.grad)

    def run():
        xd, ad, bd = (t.to(dev).requires_grad_(True) for t in (rows_of(x), ga, gb))
        oa, ob = dn.SeGate2Fn.apply(xd, ad, bd, BN, H * W)
        torch.autograd.backward([oa, ob], [rows_of(ra).to(dev), rows_of(rb).to(dev)])
        return xd.grad.cpu(), ad.grad.cpu(), bd.grad.cpu()
    got, again = run(), run()
    j = Judge()
    for k, nm in enumerate(("dx", "dga", "dgb")):
        j.precise(got[k], refs[torch.float64][k], refs[torch.float32][k], "gate backward %s BN=%d %dx%d C=%d" % (nm, BN, H, W, C))
        assert bits_equal(got[k], again[k]), "the gate gradients are deterministic"
    j.done()


@pytest.mark.parametrize("BN,H,W,C", [(2, 5, 7, 4), (3, 9, 11, 36), (2, 9, 30, 64)])
def test_camera_mean_vector_and_dropout(dev, BN, H, W, C):
    g = torch.Generator().manual_seed(C * BN)
    x = torch.randn(BN, C, H, W, generator=g)
    v = torch.randn(BN, C, generator=g)
    rm, ry = torch.randn(BN, C, generator=g), torch.randn(BN, C, H, W, generator=g)
    j = Judge()
    # camera means: every row of camera b receives rm[b] / HW
    xd = rows_of(x).to(dev).requires_grad_(True)
    mean = dn.CamMeanFn.apply(xd, BN, H * W)
    mean.backward(rm.to(dev))
    j.precise(mean.detach().cpu(), x.double().mean((2, 3)), x.mean((2, 3)), "camera means")
    want = (rm.double() / (H * W))[:, :, None, None].expand(BN, C, H, W)
    j.precise(xd.grad.cpu(), rows_of(want), rows_of((rm / (H * W))[:, :, None, None].expand(BN, C, H, W)), "camera means, backward")
    # camera vector: y = x + v[camera]; dv = the camera's column sums of dy
    xd, vd = rows_of(x).to(dev).requires_grad_(True), v.to(dev).requires_grad_(True)
    y = dn.CamAddFn.apply(xd, vd, BN, H * W)
    y.backward(rows_of(ry).to(dev))
    assert torch.equal(y.detach().cpu(), rows_of(x + v[:, :, None, None])), "one fp32 addition per element"
    assert bits_equal(xd.grad.cpu(), rows_of(ry))
    j.precise(vd.grad.cpu(), ry.double().sum((2, 3)), ry.sum((2, 3)), "camera vector, dv")
    # dropout with a given mask: exact
    mask = torch.rand(BN * H * W, C, generator=g) >= 0.5
    for p in (0.5, 0.25):
        xd = rows_of(x).to(dev).requires_grad_(True)
        y = dn.DropoutRowsFn.apply(xd, mask.to(dev), p)
        y.backward(rows_of(ry).to(dev))
        s = torch.tensor(1.0 / (1.0 - p), dtype=torch.float32)
        assert torch.equal(y.detach().cpu(), rows_of(x) * mask * s) and torch.equal(xd.grad.cpu(), rows_of(ry) * mask * s)
    xd = rows_of(x).to(dev)
    assert dn.dropout_rows(xd, 0.0) is xd                             # p == 0 skips the kernel
    j.done()


# ------------------------------------------------------------------ 5. train-mode ASPP and the whole module
# Every tensor of the two blocks stays under the precise judge (largest measured ratios: DESIGN.md 10), so none is judged at TOL.


def _grab(net, prefix=""):
    return {prefix + k: v.grad.detach().cpu() for k, v in net.named_parameters() if v.grad is not None}


def _stats(net, prefix=""):
    out = {}
    for k, m in net.named_modules():
        if isinstance(m, (torch.nn.BatchNorm1d, torch.nn.BatchNorm2d)):
            out[prefix + k] = (m.running_mean.detach().cpu().clone(), m.running_var.detach().cpu().clone(), int(m.num_batches_tracked))
    return out


@pytest.mark.parametrize("mid,H,W", [(32, 8, 10), (128, 14, 20)])
def test_aspp_under_train(dev, mid, H, W):
    BN = 2
    torch.manual_seed(mid)
    net = dn.DepthNet(mid, mid, 16, 24)
    aspp = net.depth_conv[3]
    sd = synth.random_state_dict(aspp.state_dict(), seed=mid + 1)
    aspp.load_state_dict(sd)
    aspp.dropout.p = 0.0
    net = net.to(dev).train()
    g = torch.Generator().manual_seed(H * W)
    x = torch.randn(BN, mid, H, W, generator=g) * torch.tensor([1.0, 2.0]).view(2, 1, 1, 1)
    r = torch.randn(BN, mid, H, W, generator=g)
    refs = {}
    for dt in (torch.float64, torch.float32):
        p = {"a." + k: (v.to(dt).clone().requires_grad_(not k.split(".")[-1].startswith(("running", "num"))) if v.is_floating_point() else v)
             for k, v in sd.items()}
        xx, st = leaf(x, dt), {}
        out = T.aspp(xx, p, "a", st)
        (out * r.to(dt)).sum().backward()
        refs[dt] = dict(out=rows_of(out.detach()), dx=rows_of(xx.grad), stats=st,
                        grads={k[2:]: v.grad for k, v in p.items() if v.is_floating_point() and v.requires_grad})
    xd = rows_of(x).to(dev).requires_grad_(True)
    y = net._aspp_train(xd, (BN, H, W))
    y.backward(rows_of(r).to(dev))
    r64, r32 = refs[torch.float64], refs[torch.float32]
    what = "ASPP train mid=%d %dx%d " % (mid, H, W)
    j = Judge()
    j.precise(y.detach().cpu(), r64["out"], r32["out"], what + "out")
    j.precise(xd.grad.cpu(), r64["dx"], r32["dx"], what + "dx")
    grads = _grab(aspp)
    assert set(grads) == set(r64["grads"])
    for k in sorted(grads):
        j.precise(grads[k], r64["grads"][k], r32["grads"][k], what + "grad " + k)
    stats = _stats(aspp)
    assert {"a." + k for k in stats} == set(r64["stats"]) and len(stats) == 6
    for k, (rm, rv, nb) in stats.items():
        assert nb == 1
        j.precise(rm, r64["stats"]["a." + k][0], r32["stats"]["a." + k][0], what + "running_mean " + k)
        j.precise(rv, r64["stats"]["a." + k][1], r32["stats"]["a." + k][1], what + "running_var " + k)
    core.check_h2_overflow()
    j.done()


_MOD = {}


def _module_case(mid):
    """(args, state dict, x, mlp_input, r, {dtype: the restatement's step}) -- computed once per width."""
    if mid not in _MOD:
        if mid == 32:
            args, (x, mlp, r) = T.ARGS, T.seeded_inputs()
        else:
            args = (128, 128, 32, 24)
            x, mlp, r = T.seeded_inputs(args, 2, 14, 20, seed=5)
        sd = T.seeded_state_dict(dn.DepthNet(*args).state_dict(), seed=T.SEED if mid == 32 else 6)
        _MOD[mid] = (args, sd, x, mlp, r, {dt: T.run(sd, x, mlp, r, dt) for dt in (torch.float64, torch.float32)})
    return _MOD[mid]


def _step(dev, args, sd, x, mlp, r, p=0.0, seed=None):
    net = dn.DepthNet(*args)
    net.load_state_dict(sd, strict=True)
    net.train_enabled = True
    net.depth_conv[3].dropout.p = p
    net = net.to(dev).train()
    if seed is not None:
        net.dropout_generator = torch.Generator(device=dev).manual_seed(seed)
    xd = x.to(dev).requires_grad_(True)
    out = net(xd, mlp.to(dev))
    (out * r.to(dev)).sum().backward()
    return net, out.detach().cpu(), xd.grad.cpu()


@pytest.mark.parametrize("mid", [32, 128])
def test_module_under_train(dev, mid, golden):
    args, sd, x, mlp, r, refs = _module_case(mid)
    r64, r32 = refs[torch.float64], refs[torch.float32]
    net, out, dx = _step(dev, args, sd, x, mlp, r)
    assert tuple(out.shape) == (2, args[3] + args[2]) + tuple(x.shape[2:])            # the shapes of eval
    what = "DepthNet train mid=%d " % mid
    j = Judge()
    j.precise(out, r64["out"], r32["out"], what + "out")
    j.precise(dx, r64["dx"], r32["dx"], what + "dx")
    grads = _grab(net)
    assert set(grads) == set(r64["grads"]) == {k for k, _ in net.named_parameters()}
    for k in sorted(grads):
        j.precise(grads[k], r64["grads"][k], r32["grads"][k], what + "grad " + k)
    stats = _stats(net)
    assert set(stats) == set(r64["stats"])
    for k, (rm, rv, nb) in stats.items():
        assert nb == 1 and tuple(rm.shape) == tuple(sd[k + ".running_mean"].shape)
        j.precise(rm, r64["stats"][k][0], r32["stats"][k][0], what + "running_mean " + k)
        j.precise(rv, r64["stats"][k][1], r32["stats"][k][1], what + "running_var " + k)
    if mid == 32:                                                                     # ... and the reference's own wiring
        z = golden("depthnet_train")
        f = {k: torch.from_numpy(z[k]) for k in z.files}
        j.precise(out, f["out"], r32["out"], what + "out vs the fixture")
        j.precise(dx, f["dx"], r32["dx"], what + "dx vs the fixture")
        for k in T.GOLDEN_GRADS:
            j.precise(grads[k], f["grad/" + k], r32["grads"][k], what + "grad %s vs the fixture" % k)
        for k in T.GOLDEN_BNS:
            j.precise(stats[k][0], f["rm/" + k], r32["stats"][k][0], what + "running_mean %s vs the fixture" % k)
            j.precise(stats[k][1], f["rv/" + k], r32["stats"][k][1], what + "running_var %s vs the fixture" % k)
    core.check_h2_overflow()
    j.done()


# gradients that do not pass through the deformable convolution's dx (the one atomics-based sum of the path)
_FIXED_ORDER = ("depth_conv.5.", "depth_conv.4.", "context_conv.", "context_mlp.", "context_se.")


def test_dropout_step_is_reproducible_outside_the_dcn_dx_path(dev):
    args, sd, x, mlp, r, refs = _module_case(32)
    runs = [_step(dev, args, sd, x, mlp, r, p=0.5, seed=77) for _ in range(2)]
    (na, oa, _), (nb, ob, _) = runs
    assert bits_equal(oa, ob)
    ga, gb = _grab(na), _grab(nb)
    fixed = [k for k in ga if k.startswith(_FIXED_ORDER)]
    assert len(fixed) == 15
    for k in fixed:
        assert bits_equal(ga[k], gb[k]), k
    for k, (rm, rv, n) in _stats(na).items():
        assert bits_equal(rm, _stats(nb)[k][0]) and bits_equal(rv, _stats(nb)[k][1]), k
    for k in ga:                                                     # the rest: equal up to the order of the atomic additions
        assert rel_err(ga[k], gb[k]) <= TOL, k
    M, mid = x.shape[0] * x.shape[2] * x.shape[3], args[1]
    mask = torch.rand((M, mid), device=dev, generator=torch.Generator(device=dev).manual_seed(77)) >= 0.5
    assert 0.45 < float(mask.float().mean()) < 0.55                  # roughly half of the mask is set
    _, o0, _ = _step(dev, args, sd, x, mlp, r)
    assert not bits_equal(o0, oa)
    _, oc, _ = _step(dev, args, sd, x, mlp, r, p=0.5, seed=78)
    assert not bits_equal(oc, oa)


# ------------------------------------------------------------------ 6. end to end: the view transformer trains its DepthNet
def _vt(**kw):
    return pkg.ViewTransformerLiftSplatShootVoxel(
        grid_config={'xbound': [-8., 8., 2.], 'ybound': [-8., 8., 2.], 'zbound': [-2., 2., 2.], 'dbound': [2.0, 10.0, 1.0]},
        data_config={'input_size': (64, 96)}, numC_input=32, numC_Trans=16, downsample=16, depth_net='hip', **kw)


def test_view_transformer_trains_its_depth_net(dev):
    torch.manual_seed(5)
    vt = _vt(train_depth_net=True)
    with torch.no_grad():
        vt.depth_net.depth_conv[4].conv_offset.weight.normal_(0.0, 0.02)
    vt.depth_net.depth_conv[3].dropout.p = 0.0
    vt = vt.to(dev).train()
    rig = synth.camera_rig(ncam=2, input_size=(64, 96))
    cams = tuple(rig[k].to(dev) for k in ("rots", "trans", "intrins", "post_rots", "post_trans", "bda"))
    g = torch.Generator().manual_seed(6)
    x = torch.randn(1, 2, 32, 4, 6, generator=g).to(dev)
    mlp = torch.randn(1, 2, 27, generator=g).to(dev)
    gt = (torch.rand(1, 2, 64, 96, generator=g) * 8 + 2).to(dev)
    inp = (x,) + cams + (mlp,)
    vt.eval()
    with torch.no_grad():
        before = vt.lift(inp)                                        # the eval packs exist before the weights change
    vt.train()

    def loss_of():
        bev, dp, _, _ = vt.forward(inp)
        assert tuple(bev.shape) == (1, 16, 8, 8, 2) and tuple(dp.shape) == (2, vt.D, 4, 6)
        return vt.get_depth_loss(gt, dp) + bev.sum()
    params = dict(vt.depth_net.named_parameters())
    loss = loss_of()
    loss.backward()
    for k, p in params.items():
        assert p.grad is not None and bool(torch.isfinite(p.grad).all()), k
    norm = float(torch.sqrt(sum((p.grad.double() ** 2).sum() for p in params.values())))
    assert norm > 0
    with torch.no_grad():
        for p in params.values():
            p.add_(p.grad, alpha=-1e-2 / norm)                       # one SGD step of length 1e-2 in parameter space
    after = loss_of()
    assert float(after) < float(loss), "one SGD step lowers the loss: %.6f -> %.6f" % (float(loss), float(after))
    # eval() afterwards: the packs follow the updated weights (PackCache) -- the bits of a fresh eval-only module with those weights
    vt.eval()
    fresh = _vt().to(dev).eval()
    fresh.load_state_dict(vt.state_dict())
    with torch.no_grad():
        a, b = vt.lift(inp), fresh.lift(inp)
    assert bits_equal(a[0], b[0]) and bits_equal(a[1], b[1])
    assert not bits_equal(a[1], before[1])
    # with the option off the same call still raises
    with pytest.raises(NotImplementedError, match="training"):
        fresh.train().forward(inp)
    core.check_h2_overflow()


# ------------------------------------------------------------------ 7. co-runner guard
@pytest.mark.parametrize("corunner", ["h2p", "wino"])
@pytest.mark.parametrize("stage", ["se_gate2_bwd", "dcn_cols_bwd doff"])
def test_new_kernels_are_bit_stable_beside_split_f16_gemms(dev, stage, corunner):
    import test_gpu_corunner as CR
    gb = torch.Generator().manual_seed(11)
    xb = core.to_rows(torch.randn(1, 128, 100, 100, 8, generator=gb).to(dev))
    S = dict(xb=xb, pc1=core.PackedConv((torch.randn(128, 128, 1, 1, 1, generator=gb) * 0.05).to(dev), ksize=1, pad=0),
             pc3=core.PackedConv((torch.randn(128, 128, 3, 3, 3, generator=gb) * 0.02).to(dev), ksize=3, pad=1),
             s0=torch.cuda.Stream(device=dev), s1=torch.cuda.Stream(device=dev))
    with torch.no_grad():
        core.conv_rows(xb, S["pc1"], relu=False)
        core.conv_rows(xb, S["pc3"], relu=False)
    BN, C, H, W = 6, 128, 16, 44
    M = BN * H * W
    x = torch.randn(M, C, generator=gb).to(dev)
    if stage == "se_gate2_bwd":
        ga, gbt, da, db = (torch.randn(s, generator=gb).to(dev) for s in ((BN, C), (BN, C), (M, C), (M, C)))

        def fn():
            xd, a, b = x.clone().requires_grad_(True), ga.clone().requires_grad_(True), gbt.clone().requires_grad_(True)
            with torch.enable_grad():
                oa, ob = dn.SeGate2Fn.apply(xd, a, b, BN, H * W)
                torch.autograd.backward([oa, ob], [da, db])
            return [xd.grad, a.grad, b.grad]
    else:
        off = F.pad(quant(torch.randn(M, 18, generator=gb) * 2), (0, 2)).to(dev)
        dcols = torch.randn(G, M, 9 * C // G, generator=gb).to(dev)
        xr = Rows(x, BN, H, W, 1, C)

        def fn():
            dx, doff = torch.zeros(M, C, device=dev), torch.empty(M, 20, device=dev)
            call("coocc_dcn_cols_bwd", xr.data(), xr.stride, ptr(off), 20, BN, H, W, C, G, 0, M, ptr(dcols), ptr(dx), ptr(doff))
            return [doff]
    torch.cuda.synchronize()
    ref, got = CR._run_beside(S, fn, corunner=corunner)
    bad = CR._count_differing(ref, got)
    assert bad == 0, "%s beside %s: %d of %d calls differ from the run alone" % (stage, corunner, bad, len(got))
