"""Training of the image encoder on the HIP engine (image_encoder.ResNet / SECONDFPN with ``train_enabled``; csrc/img_stem_train.hip)
against float64.

The judge is ``ref_image_encoder.TorchResNet`` / ``TorchSECONDFPN`` in ``.double().train()`` with torch autograd (frozen parts in
``.eval()`` with ``requires_grad_(False)``); the fp32 anchor is the same in float32 on the CPU.  Kernels alone: exact where the
arithmetic is exact (max-pool; the weight gradient on small integers), ``util.assert_precise`` otherwise.

Whole modules: outputs and running statistics against that judge; parameter gradients against the same judge with every ReLU's
derivative taken at the device's own sign pattern (``judge_forward`` says why).  Measured on the MI355X (ratio = error / the
anchor's own error, budget 4 max / 2 rms), worst over frozen_stages -1 / 0 / 2: gradients 1.75 / 1.25, running statistics
1.83 / 1.08, outputs 1.17 / 1.02 -- no tensor needed the ``LOOSE`` fallback below."""
import copy
import ctypes

import pytest
import torch
import torch.nn.functional as F
from torch import nn

import co_occ_amd as pkg
import ref_image_encoder as R
import util
from co_occ_amd import autograd as ag, core, image_encoder as IE, synth
from co_occ_amd._lib import call, ptr
from util import assert_close, assert_precise, precision

pytestmark = pytest.mark.gpu

NECK_KW = dict(in_channels=[256, 512, 1024, 2048], upsample_strides=[0.25, 0.5, 1, 2], out_channels=[128] * 4)
# Tensors of the whole-module cases judged by util.assert_close (the project's 1e-4) instead of assert_precise, by name prefix per
# case: a tensor goes here only after it missed the 4 x / 2 x budget on the device, with its measured ratio in DESIGN.md 11.
LOOSE = {}


def rows_of(x):
    return x.permute(0, 2, 3, 1).reshape(-1, x.shape[1]).contiguous()


def as_bchw(rows, BN, H, W):
    return rows.view(BN, H, W, -1).permute(0, 3, 1, 2)


def bits_equal(a, b):
    return a.shape == b.shape and torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


# ------------------------------------------------------------------ 1. the max-pool kernels alone
POOL_MAPS = [(1, 1, 1), (1, 2, 2), (2, 3, 5), (1, 9, 17), (2, 10, 18), (1, 35, 45)]


def pool_fwd(x, dev, twin=False, stride=None):
    """x [BN,C,Hc,Wc] (CPU) -> (pooled rows on the device, H2 twin or None) through the C entry point."""
    BN, C, Hc, Wc = x.shape
    xs = rows_of(x).to(dev)
    if stride:
        xs = F.pad(xs, (0, stride - C))
    Hp, Wp = (Hc - 1) // 2 + 1, (Wc - 1) // 2 + 1
    out = torch.full((BN * Hp * Wp, C), float("nan"), device=dev)
    tw = torch.zeros(BN * Hp * Wp, C, device=dev) if twin else None
    call("coocc_maxpool2d_rows", ptr(xs), xs.shape[1], BN, Hc, Wc, C, ptr(out), C, ptr(tw))
    torch.cuda.synchronize()
    return out, tw


def pool_bwd(x, dy, dev):
    """x [BN,C,Hc,Wc], dy [BN,C,Hp,Wp] (CPU) -> dx rows [BN*Hc*Wc, C] on the device."""
    BN, C, Hc, Wc = x.shape
    xs, ds = rows_of(x).to(dev), rows_of(dy).to(dev)
    dx = torch.full((BN * Hc * Wc, C), float("nan"), device=dev)
    call("coocc_maxpool2d_rows_bwd", ptr(xs), C, ptr(ds), C, BN, Hc, Wc, C, ptr(dx), C)
    torch.cuda.synchronize()
    return dx


def cpu_pool(x, dy):
    xr = x.clone().requires_grad_(True)
    y = F.max_pool2d(xr, 3, 2, 1)
    y.backward(dy)
    return y.detach(), xr.grad


def int_dy(x, g):
    BN, C, Hc, Wc = x.shape
    return torch.randint(-8, 9, (BN, C, (Hc - 1) // 2 + 1, (Wc - 1) // 2 + 1), generator=g).float()


def check_pool_exact(x, dy, dev, what):
    y, dx = cpu_pool(x, dy)
    out, _ = pool_fwd(x, dev)
    assert bits_equal(out.cpu(), rows_of(y)), "%s: forward bits" % what
    got = pool_bwd(x, dy, dev).cpu()
    assert torch.equal(got, rows_of(dx)), "%s: backward, %d of %d differ" % (what, int((got != rows_of(dx)).sum()), got.numel())
    return out


@pytest.mark.parametrize("C", [4, 64])
@pytest.mark.parametrize("BN,Hc,Wc", POOL_MAPS)
def test_maxpool_distinct_values(dev, BN, Hc, Wc, C):
    g = torch.Generator().manual_seed(7 * Hc + Wc + C)
    n = BN * C * Hc * Wc
    x = ((torch.randperm(n, generator=g) - n // 2).float() * 0.125).view(BN, C, Hc, Wc)
    check_pool_exact(x, int_dy(x, g), dev, "distinct %s x %d" % ((BN, Hc, Wc), C))
    # the same bits from run to run, forward (from strided rows too) and backward
    o1, o2, o3 = pool_fwd(x, dev)[0], pool_fwd(x, dev)[0], pool_fwd(x, dev, stride=C + 8)[0]
    assert bits_equal(o1, o2) and bits_equal(o1, o3)
    dy = int_dy(x, g) * 0.37
    assert bits_equal(pool_bwd(x, dy, dev), pool_bwd(x, dy, dev))


@pytest.mark.parametrize("C", [4, 64])
@pytest.mark.parametrize("BN,Hc,Wc", POOL_MAPS)
def test_maxpool_tie_rule_and_negative_maps(dev, BN, Hc, Wc, C):
    g = torch.Generator().manual_seed(11 * Hc + Wc + C)
    const = torch.full((BN, C, Hc, Wc), 1.5)
    check_pool_exact(const, int_dy(const, g), dev, "constant map")
    ties = torch.randint(0, 3, (BN, C, Hc, Wc), generator=g).float()           # three values: nearly every window has ties
    check_pool_exact(ties, int_dy(ties, g), dev, "planted ties")
    neg = -1.0 - torch.rand(BN, C, Hc, Wc, generator=g)
    out = check_pool_exact(neg, int_dy(neg, g), dev, "negative map")
    assert float(out.max()) < 0, "padding was chosen in an all-negative map"


@pytest.mark.parametrize("H,W", [(70, 90), (64, 96)])
def test_unfused_stem_gives_the_fused_kernels_bits(dev, H, W):
    import test_gpu_image_encoder as TE
    st = TE.Stem(1000 + H)
    x = st.image(H, W)
    pre, _, (BN, Hc, Wc) = st.run(x, dev, True, pool=False)
    want, want_tw, (_, Hp, Wp) = st.run(x, dev, True, pool=True, twin=True)
    out = torch.full((BN * Hp * Wp, 64), float("nan"), device=dev)
    tw = torch.zeros(BN * Hp * Wp, 64, device=dev)
    call("coocc_maxpool2d_rows", ptr(pre), 64, BN, Hc, Wc, 64, ptr(out), 64, ptr(tw))
    torch.cuda.synchronize()
    assert bits_equal(out, want) and bits_equal(tw, want_tw)
    # ... and through the Python layers
    rows = IE.stem_rows(x.to(dev), IE.stem_pack(st.conv, st.bn), relu=True, pool=False)
    pooled, geom = ag.maxpool_rows(rows.t, (rows.B, rows.X, rows.Y, 1))
    assert geom == (BN, Hp, Wp, 1) and bits_equal(pooled, want)
    core.check_h2_overflow()


def test_maxpool_entry_points_validate(dev):
    lib = pkg._lib.load()
    one = ctypes.c_void_p(16)
    assert lib.coocc_maxpool2d_rows(one, 6, 1, 3, 3, 6, one, 8, None, None) == -1 and b"multiple of 4" in lib.coocc_last_error()
    assert lib.coocc_maxpool2d_rows(one, 8, 1, 3, 3, 8, one, 8, one, None) == -1 and b"H2 twin" in lib.coocc_last_error()
    assert lib.coocc_maxpool2d_rows(None, 8, 1, 3, 3, 8, one, 8, None, None) == -1 and b"null" in lib.coocc_last_error()
    assert lib.coocc_maxpool2d_rows(one, 8, 1 << 12, 1 << 10, 1 << 10, 8, one, 8, None, None) == -1 and b"32-bit" in lib.coocc_last_error()
    assert lib.coocc_maxpool2d_rows_bwd(one, 8, ctypes.c_void_p(20), 8, 1, 3, 3, 8, one, 8, None) == -1 and b"aligned" in lib.coocc_last_error()
    assert lib.coocc_img_stem_wgrad(one, 1, 7, 7, one, 64, 32, one, one, 1 << 20, None) == -1 and b"64 stem" in lib.coocc_last_error()
    assert lib.coocc_img_stem_wgrad(one, 1, 7, 7, one, 64, 64, one, one, 16, None) == -1 and b"workspace" in lib.coocc_last_error()


# ------------------------------------------------------------------ 2. the stem weight gradient alone
WGRAD_IMAGES = [(1, 7, 7, 64), (2, 33, 37, 72), (1, 36, 68, 64), (2, 64, 96, 80)]      # (BN, H, W, dy_stride)


def stem_wgrad(x, dy, dev, dy_stride=64):
    """x [BN,3,H,W], dy [BN,64,Hc,Wc] (CPU) -> dW [64,3,7,7] (CPU) through the C entry point."""
    BN, _, H, W = x.shape
    ds = F.pad(rows_of(dy), (0, dy_stride - 64)).to(dev)
    dw = torch.full((147, 64), float("nan"), device=dev)
    nb = int(pkg._lib.load().coocc_img_stem_wgrad_ws(BN, H, W))
    ws = torch.full((nb // 4,), float("nan"), device=dev)
    call("coocc_img_stem_wgrad", ptr(x.to(dev).contiguous()), BN, H, W, ptr(ds), dy_stride, 64, ptr(dw), ptr(ws), nb)
    torch.cuda.synchronize()
    return dw.cpu().view(3, 7, 7, 64).permute(3, 0, 1, 2)


def conv_wgrad(x, dy, dtype):
    w = torch.zeros(64, 3, 7, 7, dtype=dtype, requires_grad=True)
    F.conv2d(x.to(dtype), w, None, stride=2, padding=3).backward(dy.to(dtype))
    return w.grad


@pytest.mark.parametrize("BN,H,W,dy_stride", WGRAD_IMAGES)
def test_stem_weight_gradient_alone(dev, BN, H, W, dy_stride):
    g = torch.Generator().manual_seed(13 * H + W)
    Hc, Wc = (H - 1) // 2 + 1, (W - 1) // 2 + 1
    x = R.fixture_images(BN, H, W, 13 * H + W)
    dy = torch.randn(BN, 64, Hc, Wc, generator=g)
    got = stem_wgrad(x, dy, dev, dy_stride)
    assert_precise(got, conv_wgrad(x, dy, torch.float64), conv_wgrad(x, dy, torch.float32), what="stem wgrad %dx%dx%d" % (BN, H, W))
    assert bits_equal(got, stem_wgrad(x, dy, dev, dy_stride)), "two runs differ"
    # integers small enough that every sum is exact in fp32 (|sum| <= 3 * 2 * BN*Hc*Wc < 2^24): exact equality
    xi = torch.randint(-3, 4, (BN, 3, H, W), generator=g).float()
    di = torch.randint(-2, 3, (BN, 64, Hc, Wc), generator=g).float()
    assert torch.equal(stem_wgrad(xi, di, dev, dy_stride), conv_wgrad(xi, di, torch.float64).float())


# ------------------------------------------------------------------ 3. the stem under train()
def _stem_modules(seed):
    g = torch.Generator().manual_seed(seed)
    conv = torch.nn.Conv2d(3, 64, 7, stride=2, padding=3, bias=False)
    bn = torch.nn.BatchNorm2d(64)
    with torch.no_grad():
        conv.weight.copy_(torch.randn(64, 3, 7, 7, generator=g) * (2.0 / 147) ** 0.5)
        bn.weight.copy_(torch.rand(64, generator=g) + 0.5)
        bn.bias.copy_(0.2 * torch.randn(64, generator=g))
        bn.running_mean.copy_(0.2 * torch.randn(64, generator=g))
        bn.running_var.copy_(torch.rand(64, generator=g) + 0.5)
    return conv, bn


def test_stem_under_train(dev):
    x = R.fixture_images(2, 38, 50, 31)
    g = torch.Generator().manual_seed(32)
    r = torch.randn(2, 64, 10, 13, generator=g)
    refs = {}
    for dt in (torch.float64, torch.float32):
        conv, bn = _stem_modules(30)
        conv, bn = conv.to(dt).train(), bn.to(dt).train()
        y = F.max_pool2d(torch.relu(bn(conv(x.to(dt)))), 3, 2, 1)
        (y * r.to(dt)).sum().backward()
        refs[dt] = dict(y=y.detach(), w=conv.weight.grad, g=bn.weight.grad, b=bn.bias.grad, rm=bn.running_mean, rv=bn.running_var,
                        n=bn.num_batches_tracked)
    conv, bn = _stem_modules(30)
    conv, bn = conv.to(dev).train(), bn.to(dev).train()
    h, geom = ag.stem_conv_bn_rows(x.to(dev), conv, bn, relu=True)
    assert geom == (2, 19, 25, 1)
    h, geom = ag.maxpool_rows(h, geom)
    assert geom == (2, 10, 13, 1)
    (h * rows_of(r).to(dev)).sum().backward()
    r64, r32 = refs[torch.float64], refs[torch.float32]
    got = dict(y=as_bchw(h.detach(), 2, 10, 13), w=conv.weight.grad, g=bn.weight.grad, b=bn.bias.grad, rm=bn.running_mean,
               rv=bn.running_var)
    for k, v in got.items():
        assert_precise(v.cpu(), r64[k], r32[k], what="stem under train: " + k)
    assert int(bn.num_batches_tracked) == int(r64["n"]) == 1
    xg = x.to(dev).requires_grad_(True)
    with pytest.raises(NotImplementedError, match="image"):
        ag.stem_conv_bn_rows(xg, conv, bn)
    bb = IE.ResNet(depth=50).to(dev)
    bb.train_enabled = True
    bb.train()
    with pytest.raises(NotImplementedError, match="image"):
        bb(R.fixture_images(2, 64, 96, 1).to(dev).requires_grad_(True))


def test_stem_with_a_frozen_norm(dev):
    """norm_eval with frozen affine parameters: the BN is folded into k_img_stem's epilogue and the weight gradient passes through
    the epilogue's backward (scale, ReLU mask)."""
    x = R.fixture_images(2, 38, 50, 33)
    r = torch.randn(2, 64, 10, 13, generator=torch.Generator().manual_seed(34))
    refs = {}
    for dt in (torch.float64, torch.float32):
        conv, bn = _stem_modules(35)
        conv, bn = conv.to(dt), bn.to(dt).eval().requires_grad_(False)
        y = F.max_pool2d(torch.relu(bn(conv(x.to(dt)))), 3, 2, 1)
        (y * r.to(dt)).sum().backward()
        refs[dt] = dict(y=y.detach(), w=conv.weight.grad)
    conv, bn = _stem_modules(35)
    conv, bn = conv.to(dev), bn.to(dev).eval().requires_grad_(False)
    stats = [bn.running_mean.clone(), bn.running_var.clone()]
    h, geom = ag.maxpool_rows(*ag.stem_conv_bn_rows(x.to(dev), conv, bn, relu=True))
    (h * rows_of(r).to(dev)).sum().backward()
    r64, r32 = refs[torch.float64], refs[torch.float32]
    assert_precise(as_bchw(h.detach(), 2, 10, 13).cpu(), r64["y"], r32["y"], what="stem, frozen norm: y")
    assert_precise(conv.weight.grad.cpu(), r64["w"], r32["w"], what="stem, frozen norm: w")
    assert torch.equal(stats[0], bn.running_mean) and torch.equal(stats[1], bn.running_var) and int(bn.num_batches_tracked) == 0


# ------------------------------------------------------------------ 4. whole modules against float64
def fixture_sds(seed):
    sdb = R.fixture_state_dict(IE.ResNet(depth=50).state_dict(), seed)
    sdn = R.fixture_state_dict(IE.SECONDFPN(**NECK_KW).state_dict(), seed + 1, R.transposed_keys(NECK_KW["upsample_strides"]))
    return sdb, sdn


def freeze_judge(bb, frozen):
    """mmdet's _freeze_stages on the judge."""
    mods = ([bb.conv1, bb.bn1] + [getattr(bb, "layer%d" % i) for i in range(1, frozen + 1)]) if frozen >= 0 else []
    for m in mods:
        m.eval()
        m.requires_grad_(False)


def judge_forward(bb, nk, x, masks=None):
    """``TorchResNet.forward`` + ``TorchSECONDFPN.forward`` restated over the judge's own modules (bitwise the modules' forward with
    ``masks`` None).  ``masks``: per BN name the sign pattern [B,C,H,W] of the ReLU behind it, taken from the device's forward; that
    ReLU is then ``v * mask``, so the judge's gradient is taken on the same side of every ReLU as the kernel's (``util.train_judge``
    does the same for one layer).  Without it the comparison hangs on the few pre-activations of ~2.3 M that lie within fp32 rounding
    of zero: one of them on the other side moves a gradient by ~1e-3 of its scale, in ANY fp32 evaluation -- on this fixture the CPU
    fp32 anchor itself is 4e-4 from float64 at frozen_stages=-1 for that reason."""
    def relu(v, name):
        m = None if masks is None else masks.get(name)
        return torch.relu(v) if m is None else v * m.to(v.dtype)
    h = F.max_pool2d(relu(bb.bn1(bb.conv1(x)), "img_backbone.bn1"), 3, 2, 1)
    feats = []
    for i in range(4):
        for j, b in enumerate(getattr(bb, "layer%d" % (i + 1))):
            pre = "img_backbone.layer%d.%d." % (i + 1, j)
            y = relu(b.bn1(b.conv1(h)), pre + "bn1")
            y = relu(b.bn2(b.conv2(y)), pre + "bn2")
            y = b.bn3(b.conv3(y))
            h = relu(y + (h if b.downsample is None else b.downsample(h)), pre + "bn3")
        feats.append(h)
    ups = [relu(blk[1](blk[0](f)), "img_neck.deblocks.%d.1" % i) for i, (blk, f) in enumerate(zip(nk.deblocks, feats))]
    return tuple(feats), torch.cat(ups, 1)


def judge_step(sdb, sdn, x, r, frozen, dtype, masks=None):
    bb, nk = R.TorchResNet(50), R.TorchSECONDFPN(NECK_KW["in_channels"], NECK_KW["out_channels"], NECK_KW["upsample_strides"])
    bb.load_state_dict(sdb, strict=True)
    nk.load_state_dict(sdn, strict=True)
    bb, nk = bb.to(dtype).train(), nk.to(dtype).train()
    freeze_judge(bb, frozen)
    feats, out = judge_forward(bb, nk, x.to(dtype), masks)
    (out * r.to(dtype)).sum().backward()
    named = [("img_backbone." + k, p) for k, p in bb.named_parameters()] + [("img_neck." + k, p) for k, p in nk.named_parameters()]
    bufs = [("img_backbone." + k, b) for k, b in bb.named_buffers()] + [("img_neck." + k, b) for k, b in nk.named_buffers()]
    return dict(out=out.detach(), feats=[f.detach() for f in feats], grads={k: p.grad for k, p in named if p.grad is not None},
                stats={k: b.detach().clone() for k, b in bufs})


def test_judge_forward_is_the_modules_forward():
    sdb, sdn = fixture_sds(60)
    bb, nk = R.TorchResNet(50), R.TorchSECONDFPN(NECK_KW["in_channels"], NECK_KW["out_channels"], NECK_KW["upsample_strides"])
    bb.load_state_dict(sdb, strict=True)
    nk.load_state_dict(sdn, strict=True)
    x = R.fixture_images(2, 64, 96, 61)
    with torch.no_grad():
        feats, out = judge_forward(bb.train(), nk.train(), x)
        bb.load_state_dict(sdb, strict=True), nk.load_state_dict(sdn, strict=True)         # the running statistics again
        want = bb(x)
        assert torch.equal(out, nk(list(want))[0]) and all(torch.equal(a, b) for a, b in zip(feats, want))


def tap_relu_masks(monkeypatch, bb, nk):
    """Record, per training-mode BN of the two device modules, the sign pattern of the ReLU output it produces, as [B,C,H,W] CPU
    tensors keyed like the judge's parameters (filled during the next forward)."""
    names = {id(m): "img_backbone." + k for k, m in bb.named_modules()}
    names.update({id(m): "img_neck." + k for k, m in nk.named_modules()})
    strides = {"img_neck.deblocks.%d.1" % i: k for i, (kind, k) in enumerate(nk.levels) if kind == "deconv" and k > 1}
    masks, orig = {}, ag.BatchNormRowsFn.apply

    def apply(x, gamma, beta, res, bn, relu, *rest):
        y = orig(x, gamma, beta, res, bn, relu, *rest)
        if relu:
            masks[names[id(bn)]] = (y.detach() > 0).cpu()
        return y
    monkeypatch.setattr(ag.BatchNormRowsFn, "apply", staticmethod(apply))

    def as_maps(shapes):
        out = {}
        for k, m in masks.items():
            B, C, H, W = shapes[k]
            s = strides.get(k, 1)                  # a deconvolution's rows are (coarse pixel, child (kh, kw)): [B, H/s, W/s, s, s, C]
            out[k] = m.view(B, H // s, W // s, s, s, C).permute(0, 5, 1, 3, 2, 4).reshape(B, C, H, W)
        return out
    return as_maps


def relu_shapes(BN, H, W):
    """[B,C,H,W] of every ReLU of ResNet-50 + the neck at an H x W image, keyed by the BN in front of it."""
    shapes = {"img_backbone.bn1": (BN, 64, H // 2, W // 2)}
    h, w = H // 4, W // 4
    for i, n in enumerate(R.ARCH[50]):
        planes = 64 * 2 ** i
        for j in range(n):
            pre = "img_backbone.layer%d.%d." % (i + 1, j)
            shapes[pre + "bn1"] = (BN, planes, h, w)
            if j == 0 and i > 0:
                h, w = h // 2, w // 2
            shapes[pre + "bn2"] = (BN, planes, h, w)
            shapes[pre + "bn3"] = (BN, planes * 4, h, w)
    for i, c in enumerate(NECK_KW["out_channels"]):
        shapes["img_neck.deblocks.%d.1" % i] = (BN, c, H // 16, W // 16)
    return shapes


_CASES = {}


def module_case(frozen):
    """Weights, images, loss weights and the two plain CPU references of one frozen_stages case, computed once."""
    if frozen not in _CASES:
        sdb, sdn = fixture_sds(60)
        x = R.fixture_images(2, 64, 96, 61)
        r = torch.randn(2, 512, 4, 6, generator=torch.Generator().manual_seed(62))
        _CASES[frozen] = dict(sdb=sdb, sdn=sdn, x=x, r=r, r64=judge_step(sdb, sdn, x, r, frozen, torch.float64),
                              r32=judge_step(sdb, sdn, x, r, frozen, torch.float32))
    return _CASES[frozen]


def build_trainable(dev, sdb, sdn, frozen=0, enable=True, **kw):
    bb = IE.ResNet(depth=50, num_stages=4, out_indices=(0, 1, 2, 3), frozen_stages=frozen, style='pytorch',
                   **dict(dict(norm_cfg=dict(type='BN', requires_grad=True), norm_eval=False), **kw))
    nk = IE.SECONDFPN(**NECK_KW)
    bb.load_state_dict(sdb, strict=True)
    nk.load_state_dict(sdn, strict=True)
    bb, nk = bb.to(dev), nk.to(dev)
    bb.train_enabled = nk.train_enabled = bool(enable)
    return bb.train(), nk.train()


def judged(name, got, r64, r32, case, misses):
    """One tensor of a whole-module case: every figure is printed, the misses are collected and asserted together."""
    if any(name.startswith(p) for p in LOOSE.get(case, ())):
        assert_close(got.cpu(), r64, what=name)
        return
    st = precision(got.cpu(), r64, r32, what="%s %s" % (case, name))
    if not st["ok"]:
        misses.append("%s: ratio %.2f / %.2f (e_max %.2e, anchor %.2e)" % (name, st["ratio_max"], st["ratio_rms"], st["e_max"], st["a_max"]))


@pytest.mark.parametrize("frozen", [-1, 0, 2])
def test_modules_under_train(dev, frozen, monkeypatch):
    """Outputs and running statistics against the plain judge; every parameter gradient against the judge with the device's own
    ReLU masks (``judge_forward``).  Measured on the MI355X: see DESIGN.md 11."""
    c = module_case(frozen)
    r64, r32, case = c["r64"], c["r32"], "frozen_stages=%d" % frozen
    bb, nk = build_trainable(dev, c["sdb"], c["sdn"], frozen)
    as_maps = tap_relu_masks(monkeypatch, bb, nk)
    before = {k: v.detach().clone() for k, v in list(bb.state_dict(prefix="img_backbone.").items())}
    feats = bb(c["x"].to(dev))
    out = nk(feats)[0]
    assert out.is_contiguous(memory_format=torch.channels_last) and all(f.permute(0, 2, 3, 1).is_contiguous() for f in feats)
    (out * c["r"].to(dev)).sum().backward()
    misses = []
    judged("out", out.detach(), r64["out"], r32["out"], case, misses)
    for i, f in enumerate(feats):
        judged("stage %d" % i, f.detach(), r64["feats"][i], r32["feats"][i], case, misses)
        assert f.requires_grad == (i >= frozen), "stage %d output" % i
    named = [("img_backbone." + k, p) for k, p in bb.named_parameters()] + [("img_neck." + k, p) for k, p in nk.named_parameters()]
    with_grad = {k for k, p in named if p.grad is not None}
    assert with_grad == set(r64["grads"]), sorted(with_grad ^ set(r64["grads"]))[:8]
    masks = as_maps(relu_shapes(2, 64, 96))
    trained = [k for k in relu_shapes(2, 64, 96) if not k.startswith(tuple(
        ["img_backbone.bn1"] + ["img_backbone.layer%d." % i for i in range(1, frozen + 1)] if frozen >= 0 else ["\0"]))]
    assert sorted(masks) == sorted(trained)                             # one mask per ReLU behind a training-mode BN
    g64, g32 = (judge_step(c["sdb"], c["sdn"], c["x"], c["r"], frozen, dt, masks)["grads"] for dt in (torch.float64, torch.float32))
    # ResNet-50: 53 convolutions + 53 BNs = 159 parameters; the stem holds 3, layer1 30, layer2 39; the neck 12
    assert len(with_grad) == {-1: 159 + 12, 0: 156 + 12, 2: 156 - 30 - 39 + 12}[frozen]
    for k, p in named:
        if p.grad is not None:
            judged("grad " + k, p.grad, g64[k], g32[k], case, misses)
    stats = dict(bb.state_dict(prefix="img_backbone."), **nk.state_dict(prefix="img_neck."))
    for k, want in r64["stats"].items():
        if k.endswith("num_batches_tracked"):
            assert int(stats[k]) == int(want), k
        else:
            judged("stat " + k, stats[k], want, r32["stats"][k], case, misses)
    # frozen parts: their BN statistics are untouched (bitwise)
    prefixes = (["img_backbone.bn1."] + ["img_backbone.layer%d." % i for i in range(1, frozen + 1)]) if frozen >= 0 else []
    for k, v in before.items():
        if k.startswith(tuple(prefixes)) and prefixes and "running_" in k:
            assert torch.equal(v, stats[k]), k
    assert not misses, "%s: %d tensors over the budget C_MAX = 4, C_RMS = 2:\n%s" % (case, len(misses), "\n".join(misses))
    core.check_h2_overflow()


def test_neck_alone_with_both_deblock_kinds(dev):
    kw = dict(in_channels=[16, 32, 32, 64], out_channels=[16, 16, 32, 16], upsample_strides=[0.5, 1, 1, 2])
    g = torch.Generator().manual_seed(70)
    xs = [torch.randn(2, c, h, w, generator=g) for c, (h, w) in zip(kw["in_channels"], [(12, 20), (6, 10), (6, 10), (3, 5)])]
    r = torch.randn(2, sum(kw["out_channels"]), 6, 10, generator=g)
    for use_conv in (True, False):                    # deconv 2 beside conv / 2 and conv 1; then deconv 1 beside deconv 2
        if not use_conv:
            kw = dict(in_channels=[32, 64], out_channels=[32, 16], upsample_strides=[1, 2])
            xs, r = xs[2:], r[:, :48]
        sd = R.fixture_state_dict(IE.SECONDFPN(use_conv_for_no_stride=use_conv, **kw).state_dict(), 71,
                                  R.transposed_keys(kw["upsample_strides"], use_conv))
        refs = {}
        for dt in (torch.float64, torch.float32):
            nk = R.TorchSECONDFPN(kw["in_channels"], kw["out_channels"], kw["upsample_strides"], use_conv).to(dt).train()
            nk.load_state_dict(R.cast(sd, dt), strict=True)
            leaves = [x.clone().to(dt).requires_grad_(True) for x in xs]
            out = nk(leaves)[0]
            (out * r.to(dt)).sum().backward()
            refs[dt] = dict(out=out.detach(), dx=[l.grad for l in leaves], grads={k: p.grad for k, p in nk.named_parameters()},
                            stats={k: b.clone() for k, b in nk.named_buffers()})
        nk = IE.SECONDFPN(use_conv_for_no_stride=use_conv, **kw)
        kinds = {k for k, _ in nk.levels}
        assert kinds == ({"conv", "deconv"} if use_conv else {"deconv"})
        nk.load_state_dict(sd, strict=True)
        nk = nk.to(dev)
        nk.train_enabled = True
        nk.train()
        # level 0 arrives in NCHW memory (one copy), the others channels-last (read in place)
        leaves = [x.to(dev).requires_grad_(True) if i == 0 else
                  x.to(dev).contiguous(memory_format=torch.channels_last).requires_grad_(True) for i, x in enumerate(xs)]
        out = nk(leaves)[0]
        (out * r.to(dev)).sum().backward()
        r64, r32 = refs[torch.float64], refs[torch.float32]
        what = "neck use_conv=%d " % use_conv
        assert_precise(out.detach().cpu(), r64["out"], r32["out"], what=what + "out")
        for i, l in enumerate(leaves):
            assert_precise(l.grad.cpu(), r64["dx"][i], r32["dx"][i], what=what + "dx %d" % i)
        for k, p in nk.named_parameters():
            assert p.grad is not None and tuple(p.grad.shape) == tuple(p.shape), k
            assert_precise(p.grad.cpu(), r64["grads"][k], r32["grads"][k], what=what + "grad " + k)
        for k, b in nk.named_buffers():
            if k.endswith("num_batches_tracked"):
                assert int(b) == 1
            else:
                assert_precise(b.cpu(), r64["stats"][k], r32["stats"][k], what=what + "stat " + k)
    core.check_h2_overflow()


def _cmp(got, r64, r32, what, tol=util.TOL):
    """``util.TOL`` scale-relative, under the condition that the fp32 torch evaluation is within a quarter of it (the rule of the
    3-D deblock test in test_gpu_trunk_train.py)."""
    e32 = util.rel_err(r32, r64)
    assert e32 <= tol / 4, "%s: the fp32 torch evaluation is %.3e from float64: TOL does not judge this fixture" % (what, e32)
    e = util.rel_err(got, r64)
    print("[image-encoder-train] %-40s scale-relative %.3e (fp32 torch %.3e)" % (what, e, e32))
    assert e <= tol, "%s: %.3e from float64" % (what, e)


@pytest.mark.parametrize("s,train", [(2, True), (4, True), (2, False)])
def test_deblock_2d_through_deconv_bn_rows_against_float64(dev, s, train):
    """ConvTranspose2d(kernel = stride = s) + BatchNorm2d + ReLU through ``autograd.deconv_bn_rows``, the mirror of the 3-D deblock
    test in test_gpu_trunk_train.py: output, dx, dW (and, with batch statistics, dgamma, dbeta) within ``util.TOL`` (scale-relative)
    of float64 torch, where the fp32 torch evaluation is within TOL / 4.  Running statistics under train(): torch's update (momentum
    0.1, unbiased variance) to 1e-5, as derived there for these counts (n = 96 and 384 values per channel); in eval mode (the BN
    folded into the GEMM's epilogue) they are untouched."""
    Cin, Cout, (BN, H, W) = 32, 16, (2, 3, 4)
    gen = torch.Generator().manual_seed(60 + s)
    blk = nn.Sequential(nn.ConvTranspose2d(Cin, Cout, s, stride=s, bias=False), nn.BatchNorm2d(Cout, eps=1e-3, momentum=0.1), nn.ReLU())
    blk.load_state_dict(synth.random_state_dict(blk.state_dict(), seed=60 + s))
    x = torch.randn(BN, Cin, H, W, generator=gen)
    up = torch.randn(BN, Cout, H * s, W * s, generator=gen)
    refs = {}
    for dt in (torch.float64, torch.float32):
        m = copy.deepcopy(blk).to(dt).train(train)
        xa = x.to(dt, copy=True).requires_grad_()       # a copy: x.to(float32) is x itself, and x stays a plain input
        y = m(xa)
        y.backward(up.to(dt))
        refs[dt] = dict(y=y.detach(), dx=xa.grad, dw=m[0].weight.grad, dg=m[1].weight.grad, db=m[1].bias.grad, rm=m[1].running_mean,
                        rv=m[1].running_var, nb=int(m[1].num_batches_tracked))
    m = copy.deepcopy(blk).to(dev).train(train)
    xd = x.to(dev).requires_grad_()
    u = ag.deconv_bn_rows(rows_of(xd), m[0], m[1], s)
    out = ag.fpn_sum_rows([u], [s], Cout, (BN, H * s, W * s, 1))
    out.backward(rows_of(up).to(dev))
    got = dict(y=as_bchw(out.detach(), BN, H * s, W * s), dx=xd.grad, dw=m[0].weight.grad)
    if train:
        got.update(dg=m[1].weight.grad, db=m[1].bias.grad)
    else:
        assert m[1].weight.grad is None and m[1].bias.grad is None          # folded: constants of the epilogue
    assert tuple(m[0].weight.grad.shape) == (Cin, Cout, s, s)
    for k, v in got.items():
        _cmp(v.cpu(), refs[torch.float64][k], refs[torch.float32][k], "deblock 2d s%d train=%d %s" % (s, train, k))
    r = refs[torch.float64]
    assert int(m[1].num_batches_tracked) == r["nb"] == int(train)
    for k, v in (("rm", m[1].running_mean), ("rv", m[1].running_var)):
        if train:
            e = util.rel_err(v.cpu(), r[k])
            assert e <= 1e-5, "running statistic %s: %.3e" % (k, e)
        else:
            assert torch.equal(v.cpu(), blk[1].state_dict()["running_mean" if k == "rm" else "running_var"]), k
    core.check_h2_overflow()


# ------------------------------------------------------------------ 5. modes and options
def _eval_out(bb, nk, x):
    with torch.no_grad():
        return nk(bb(x))[0].clone()


def test_option_off_raises_and_eval_follows_the_trained_weights(dev):
    c = module_case(0)
    x = c["x"].to(dev)
    off_bb, off_nk = build_trainable(dev, c["sdb"], c["sdn"], 0, enable=False)
    assert all(p.requires_grad for p in off_bb.parameters()) and off_bb.bn1.training        # nothing touched with the option off
    with pytest.raises(NotImplementedError) as e:
        off_bb(x)
    assert ".eval()" in str(e.value) and "train_enabled" in str(e.value)
    with pytest.raises(NotImplementedError, match="train_enabled"):
        off_nk([torch.zeros(2, ch, 2, 3, device=dev) for ch in NECK_KW["in_channels"]])
    bb, nk = build_trainable(dev, c["sdb"], c["sdn"], 0)
    before = _eval_out(bb.eval(), nk.eval(), x)                       # the eval packs exist before the weights change
    assert bits_equal(before, _eval_out(off_bb.eval(), off_nk.eval(), x))
    bb.train(), nk.train()
    out = nk(bb(x))[0]
    (out * c["r"].to(dev)).sum().backward()
    params = [p for m in (bb, nk) for p in m.parameters() if p.grad is not None]
    norm = float(torch.sqrt(sum((p.grad.double() ** 2).sum() for p in params)))
    with torch.no_grad():
        for p in params:
            p.add_(p.grad, alpha=-1e-1 / norm)
    after = _eval_out(bb.eval(), nk.eval(), x)
    fresh_bb, fresh_nk = build_trainable(dev, bb.state_dict(), nk.state_dict(), 0, enable=False)
    assert bits_equal(after, _eval_out(fresh_bb.eval(), fresh_nk.eval(), x))
    assert not bits_equal(after, before)
    core.check_h2_overflow()


def test_norm_eval(dev):
    c = module_case(0)
    x = c["x"].to(dev)
    bb, nk = build_trainable(dev, c["sdb"], c["sdn"], 0, norm_eval=True)
    assert not any(m.training for m in IE._bns(bb))
    with pytest.raises(NotImplementedError, match="requires_grad"):
        bb(x)
    bb, nk = build_trainable(dev, c["sdb"], c["sdn"], -1, norm_eval=True, norm_cfg=dict(type='BN', requires_grad=False))
    stats = {k: v.clone() for k, v in bb.state_dict().items() if "running_" in k or "num_batches" in k}
    feats = bb(x)
    sum(f.sum() for f in feats).backward()
    for k, v in bb.state_dict().items():
        if k in stats:
            assert torch.equal(v, stats[k]), k
    got = {k for k, p in bb.named_parameters() if p.grad is not None}
    assert got == {k for k, p in bb.named_parameters() if p.dim() == 4} and "conv1.weight" in got
    # ... and with every statistic frozen the forward is the eval forward
    ev = IE.ResNet(depth=50).to(dev).eval()
    ev.load_state_dict(bb.state_dict())
    with torch.no_grad():
        want = ev(x)
    for f, w in zip(feats, want):
        assert_close(f.detach().cpu(), w.cpu(), what="norm_eval forward")
    core.check_h2_overflow()


# ------------------------------------------------------------------ 6. the detector end to end
def _detector(dev, **kw):
    oc = [32, 32, 32, 32]
    bcfg = dict(type='ResNet', depth=50, stem_channels=64, base_channels=16, num_stages=4, out_indices=(0, 1, 2, 3), frozen_stages=0,
                norm_cfg=dict(type='BN', requires_grad=True), norm_eval=False, style='pytorch', pretrained='ckpts/none.pth')
    ncfg = dict(type='SECONDFPN', in_channels=[64, 128, 256, 512], upsample_strides=[0.25, 0.5, 1, 2], out_channels=oc)
    cfg = synth.model_cfg(C=32, block_inplanes=(32, 64, 128, 256), out_channels=32, rendering=False, input_size=(64, 96), cascade_ratio=1,
                          final_occ_size=(100, 100, 8))       # no fine branch: its MLPs are sized for the full model's 128 channels
    cfg["occ_fuser"] = None                                     # camera-only: the image volume goes straight to the encoder
    cfg["img_view_transformer"].update(numC_input=sum(oc), downsample=16, depth_net='hip', train_depth_net=True)
    torch.manual_seed(90)
    det = pkg.build_detector(cfg, img_backbone=bcfg, img_neck=ncfg, hip_image_encoder=True, external_encoders=True, **kw)
    det.img_backbone.load_state_dict(R.fixture_state_dict(det.img_backbone.state_dict(), 91), strict=True)
    det.img_neck.load_state_dict(R.fixture_state_dict(det.img_neck.state_dict(), 92, R.transposed_keys(ncfg["upsample_strides"])),
                                 strict=True)
    with torch.no_grad():
        det.img_view_transformer.depth_net.depth_conv[4].conv_offset.weight.normal_(0.0, 0.02)
    det.img_view_transformer.depth_net.depth_conv[3].dropout.p = 0.0
    return det.to(dev).train()


def test_detector_trains_its_image_encoder_from_raw_images(dev):
    det = _detector(dev, train_image_encoder=True)
    assert det.img_backbone.train_enabled and det.img_neck.train_enabled and not det.img_backbone.bn1.training
    rig = synth.camera_rig(ncam=2, input_size=(64, 96))
    g = torch.Generator().manual_seed(93)
    img = R.fixture_images(2, 64, 96, 94).view(1, 2, 3, 64, 96)
    depth = (torch.rand(1, 2, 64, 96, generator=g) * 50 + 2) * (torch.rand(1, 2, 64, 96, generator=g) < 0.3)
    gt = torch.randint(1, 17, (1, 100, 100, 8), generator=g).to(torch.uint8)
    gt[torch.rand(gt.shape, generator=g) < 0.8] = 0
    img_inputs = [t.to(dev) for t in [img] + [rig[k] for k in ("rots", "trans", "intrins", "post_rots", "post_trans", "bda")] + [depth]]
    img_inputs.append(rig["input_size"])

    def loss_of(d):
        losses = d.forward_train(img_metas=None, img_inputs=img_inputs, gt_occ=gt.to(dev),
                                 generator=torch.Generator(device=dev).manual_seed(0))
        assert all(bool(torch.isfinite(v).all()) for v in losses.values())
        return sum(v for k, v in losses.items() if k.startswith("loss"))
    loss = loss_of(det)
    loss.backward()
    enc = [(k, p) for k, p in det.named_parameters() if k.startswith(("img_backbone.", "img_neck."))]
    frozen = [k for k, p in enc if not p.requires_grad]
    assert sorted(frozen) == ["img_backbone.bn1.bias", "img_backbone.bn1.weight", "img_backbone.conv1.weight"]
    for k, p in enc:
        if p.requires_grad:
            assert p.grad is not None and bool(torch.isfinite(p.grad).all()) and float(p.grad.abs().sum()) > 0, k
        else:
            assert p.grad is None, k
    params = [p for p in det.parameters() if p.grad is not None]
    norm = float(torch.sqrt(sum((p.grad.double() ** 2).sum() for p in params)))
    with torch.no_grad():
        for p in params:
            p.add_(p.grad, alpha=-1e-2 / norm)
    after = loss_of(det)
    assert float(after.detach()) < float(loss.detach()), "one SGD step lowers the loss: %.6f -> %.6f" % (float(loss.detach()), float(after.detach()))
    with pytest.raises(NotImplementedError, match="train_enabled"):
        loss_of(_detector(dev))
    core.check_h2_overflow()


# ------------------------------------------------------------------ 7. co-runner guard
@pytest.mark.parametrize("corunner", ["h2p", "wino"])
@pytest.mark.parametrize("stage", ["maxpool2d_rows", "maxpool2d_rows_bwd", "img_stem_wgrad"])
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
    BN, H, W = 6, 128, 352
    Hc, Wc = H // 2, W // 2
    Hp, Wp = Hc // 2, Wc // 2
    x = torch.randn(BN * Hc * Wc, 64, generator=gb).to(dev)
    dyp = torch.randn(BN * Hp * Wp, 64, generator=gb).to(dev)
    img = torch.randn(BN, 3, H, W, generator=gb).to(dev)
    nb = int(pkg._lib.load().coocc_img_stem_wgrad_ws(BN, H, W))
    ws = torch.empty(nb // 4, device=dev)
    if stage == "maxpool2d_rows":
        def fn():
            out, tw = torch.empty(BN * Hp * Wp, 64, device=dev), torch.empty(BN * Hp * Wp, 64, device=dev)
            call("coocc_maxpool2d_rows", ptr(x), 64, BN, Hc, Wc, 64, ptr(out), 64, ptr(tw))
            return [out, tw]
    elif stage == "maxpool2d_rows_bwd":
        def fn():
            dx = torch.empty(BN * Hc * Wc, 64, device=dev)
            call("coocc_maxpool2d_rows_bwd", ptr(x), 64, ptr(dyp), 64, BN, Hc, Wc, 64, ptr(dx), 64)
            return [dx]
    else:
        def fn():
            dw = torch.empty(147, 64, device=dev)
            call("coocc_img_stem_wgrad", ptr(img), BN, H, W, ptr(x), 64, 64, ptr(dw), ptr(ws), nb)
            return [dw]
    torch.cuda.synchronize()
    ref, got = CR._run_beside(S, fn, corunner=corunner)
    bad = CR._count_differing(ref, got)
    assert bad == 0, "%s beside %s: %d of %d calls differ from the run alone" % (stage, corunner, bad, len(got))
