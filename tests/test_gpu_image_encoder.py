"""The image encoder on the HIP engine (co_occ_amd/image_encoder.py, csrc/img_stem.hip) against float64.

Single kernels and layers are judged at their own precision (``util.assert_precise``: the fp32 CPU evaluation of the same operation,
and for the GEMM layers the split-f16 emulation, as anchors); module-level outputs by ``util.assert_close`` (TOL), under the condition
that the fp32 restatement (tests/ref_image_encoder.py) is itself within TOL / 4 of float64 on that input."""
import pytest
import torch
import torch.nn.functional as F

import co_occ_amd as pkg
import ref_image_encoder as R
from co_occ_amd import core, image_encoder as IE, synth
from co_occ_amd._lib import call, ptr
from co_occ_amd.core import Rows
from util import TOL, assert_close, assert_precise, gemm_refs, kernels, rel_err

pytestmark = pytest.mark.gpu

STEM_SIZES = [(7, 9), (38, 50), (64, 96), (1, 1)]


def rows_of(x):
    """[BN,C,H,W] -> channels-last rows [BN*H*W, C]."""
    return x.permute(0, 2, 3, 1).reshape(-1, x.shape[1]).contiguous()


def as_rows(x, dev):
    BN, C, H, W = x.shape
    return Rows(rows_of(x).float().to(dev), BN, H, W, 1, C)


def as_bchw(rows, BN, H, W):
    return rows.view(BN, H, W, -1).permute(0, 3, 1, 2)


def bits_equal(a, b):
    return a.shape == b.shape and torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


def bn_of(C, g, eps=1e-5, w_gain=1.0):
    bn = torch.nn.BatchNorm2d(C, eps=eps).eval()
    with torch.no_grad():
        bn.weight.copy_((torch.rand(C, generator=g) + 0.5) * w_gain)
        bn.bias.copy_(0.2 * torch.randn(C, generator=g))
        bn.running_mean.copy_(0.2 * torch.randn(C, generator=g))
        bn.running_var.copy_(torch.rand(C, generator=g) + 0.5)
    return bn


def bn_terms(bn):
    """(scale, bias) of the folded BN in float64."""
    s = bn.weight.double() / torch.sqrt(bn.running_var.double() + bn.eps)
    return s, bn.bias.double() - bn.running_mean.double() * s


# ------------------------------------------------------------------ 1. / 2. the stem kernel
class Stem:
    def __init__(self, seed, corners=False, bias_shift=0.0):
        g = torch.Generator().manual_seed(seed)
        self.conv = torch.nn.Conv2d(3, 64, 7, stride=2, padding=3, bias=False)
        self.bn = bn_of(64, g)
        with torch.no_grad():
            w = torch.randn(64, 3, 7, 7, generator=g) * (2.0 / 147) ** 0.5
            if corners:                   # zero but one tap at each of the four kernel corners, all different
                m = torch.zeros(7, 7)
                m[0, 0], m[0, 6], m[6, 0], m[6, 6] = 1.0, 2.0, 3.0, 4.0
                w = w * m
            self.conv.weight.copy_(w)
            self.bn.bias.add_(bias_shift)
        self.g = g
        self.sd = {"conv1.weight": self.conv.weight.detach().clone()}
        self.sd.update({"bn1." + k: v.detach().clone() for k, v in self.bn.state_dict().items() if v.is_floating_point()})

    def image(self, H, W):
        x = torch.randn(2, 3, H, W, generator=self.g)
        x[1] *= 2.5
        return x

    def ref(self, x, dtype, relu, pool):
        return R.stem(x.to(dtype), R.cast(self.sd, dtype), relu=relu, pool=pool)

    def run(self, x, dev, relu, pool, twin=False):
        """The kernel's rows (and their H2 twin) through the C entry point."""
        w, sc, bi = IE.stem_pack(self.conv.to(dev), self.bn.to(dev))
        BN, _, H, W = x.shape
        Ho, Wo = (H - 1) // 2 + 1, (W - 1) // 2 + 1
        if pool:
            Ho, Wo = (Ho - 1) // 2 + 1, (Wo - 1) // 2 + 1
        out = torch.full((BN * Ho * Wo, 64), float("nan"), device=dev)
        tw = torch.zeros(BN * Ho * Wo, 64, device=dev) if twin else None
        call("coocc_img_stem", ptr(x.to(dev).contiguous()), BN, H, W, ptr(w), ptr(sc), ptr(bi), 64, int(relu), int(pool), ptr(out), 64,
             ptr(tw))
        torch.cuda.synchronize()
        return out, tw, (BN, Ho, Wo)


@pytest.mark.parametrize("relu", [True, False])
@pytest.mark.parametrize("H,W", STEM_SIZES)
def test_stem_convolution_alone(dev, H, W, relu):
    st = Stem(100 * H + W)
    x = st.image(H, W)
    out, _, (BN, Ho, Wo) = st.run(x, dev, relu, pool=False)
    r64, r32 = st.ref(x, torch.float64, relu, False), st.ref(x, torch.float32, relu, False)
    assert tuple(r64.shape) == (BN, 64, Ho, Wo)
    assert_precise(out.cpu(), rows_of(r64), rows_of(r32), what="stem conv %dx%d relu=%d" % (H, W, relu))
    via = IE.stem_rows(x.to(dev), IE.stem_pack(st.conv, st.bn), relu=relu, pool=False)
    assert (via.B, via.X, via.Y, via.Z, via.C) == (BN, Ho, Wo, 1, 64) and bits_equal(via.t, out)
    core.check_h2_overflow()


@pytest.mark.parametrize("H,W", [(7, 9), (38, 50)])
def test_stem_corner_taps(dev, H, W):
    """Only the four kernel corners weigh, each differently: a flipped or transposed tap order, or padding off by one, moves them."""
    st = Stem(7, corners=True)
    x = st.image(H, W)
    out, _, _ = st.run(x, dev, relu=False, pool=False)
    r64, r32 = st.ref(x, torch.float64, False, False), st.ref(x, torch.float32, False, False)
    assert_precise(out.cpu(), rows_of(r64), rows_of(r32), what="stem corner taps %dx%d" % (H, W))


@pytest.mark.parametrize("H,W", STEM_SIZES + [(33, 47)])
def test_stem_fused_with_the_max_pool(dev, H, W):
    st = Stem(200 * H + W)
    x = st.image(H, W)
    out, tw, (BN, Ho, Wo) = st.run(x, dev, relu=True, pool=True, twin=True)
    r64, r32 = st.ref(x, torch.float64, True, True), st.ref(x, torch.float32, True, True)
    assert tuple(r64.shape) == (BN, 64, Ho, Wo)
    assert_precise(out.cpu(), rows_of(r64), rows_of(r32), what="stem fused %dx%d" % (H, W))
    # bit-equal to pooling the kernel's own convolution map on the host
    conv, _, (_, Hc, Wc) = st.run(x, dev, relu=True, pool=False)
    own = F.max_pool2d(as_bchw(conv.cpu(), BN, Hc, Wc), 3, 2, 1)
    assert bits_equal(rows_of(own), out.cpu())
    # the H2 twin is the conversion pass's, bit for bit
    want_tw = core.rows_to_h2(out, name="test_stem_h2")
    torch.cuda.synchronize()
    assert bits_equal(tw, want_tw[:out.numel()].view_as(tw))
    again, tw2, _ = st.run(x, dev, relu=True, pool=True, twin=True)
    assert bits_equal(again, out) and bits_equal(tw2, tw)
    core.check_h2_overflow()


@pytest.mark.parametrize("H,W", [(7, 9), (33, 47), (1, 1)])
def test_padding_is_never_the_maximum(dev, H, W):
    """relu = 0 and a map that is negative everywhere: a padded 0 (or any finite filler) would win the maximum."""
    st = Stem(300 * H + W, bias_shift=-50.0)
    x = st.image(H, W)
    out, _, (BN, Ho, Wo) = st.run(x, dev, relu=False, pool=True)
    conv, _, (_, Hc, Wc) = st.run(x, dev, relu=False, pool=False)
    assert float(conv.max()) < 0
    assert float(out.max()) < 0 and bool(torch.isfinite(out).all())
    assert bits_equal(rows_of(F.max_pool2d(as_bchw(conv.cpu(), BN, Hc, Wc), 3, 2, 1)), out.cpu())
    r64, r32 = st.ref(x, torch.float64, False, True), st.ref(x, torch.float32, False, True)
    assert_precise(out.cpu(), rows_of(r64), rows_of(r32), what="stem fused, negative map %dx%d" % (H, W))


def test_stem_refuses_what_it_cannot_address(dev):
    st = Stem(1)
    w, sc, bi = IE.stem_pack(st.conv.to(dev), st.bn.to(dev))
    x = torch.zeros(1, 3, 8, 8, device=dev)
    out = torch.zeros(4, 64, device=dev)
    with pytest.raises(pkg._lib.CooccArgError):
        call("coocc_img_stem", ptr(x), 1, 8, 8, ptr(w), ptr(sc), ptr(bi), 32, 1, 1, ptr(out), 64, None)
    with pytest.raises(pkg._lib.CooccArgError):                  # BN * Hc * Wc past 2^31: nothing is launched
        call("coocc_img_stem", ptr(x), 40000, 1 << 9, 1 << 9, ptr(w), ptr(sc), ptr(bi), 64, 1, 1, ptr(out), 64, None)
    with pytest.raises(pkg._lib.CooccError):
        IE.stem_rows(torch.zeros(1, 3, 8, 8), (w, sc, bi))


# ------------------------------------------------------------------ 3. layers through the engine
def taps2d(x, w, stride, pad):
    """Taps of a 2-D convolution as GEMM operand pairs: x [B,C,H,W], w [N,C,kh,kw] -> [(rows of tap [B*Ho*Wo, C], W_t [C, N]), ...]."""
    kh, kw = w.shape[2:]
    xp = F.pad(x.double(), (pad, pad, pad, pad))
    Ho, Wo = (x.shape[2] + 2 * pad - kh) // stride + 1, (x.shape[3] + 2 * pad - kw) // stride + 1
    return [(rows_of(xp[:, :, a:a + stride * (Ho - 1) + 1:stride, b:b + stride * (Wo - 1) + 1:stride]), w[:, :, a, b].double().t())
            for a in range(kh) for b in range(kw)], (Ho, Wo)


@pytest.fixture(params=["routed", "split-f16"])
def engine(request, monkeypatch):
    """The layers at the size the issue names are below ``core.H2_DIRECT_MIN_FLOPS`` and route to the fp32-MFMA kernels; the
    product sizes take the split-f16 kernels -- the second pass lowers the threshold so the same layers run there."""
    if request.param == "split-f16":
        monkeypatch.setattr(core, "H2_DIRECT_MIN_FLOPS", 0.0)
    return request.param


def judge_layer(out, pairs, engine, what, **epi):
    r64, r32, rs = gemm_refs(pairs, split=engine == "split-f16", chain=0 if engine == "split-f16" else 2, **epi)
    assert_precise(out.cpu(), r64, r32, rs, what="%s [%s]" % (what, engine))


def layer_inputs(seed, Cin=64, Cout=256, k=1, H=9, W=13):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(2, Cin, H, W, generator=g) * torch.tensor([1.0, 2.5]).view(2, 1, 1, 1)
    w = torch.randn(Cout, Cin, k, k, generator=g) * (2.0 / (Cin * k * k)) ** 0.5
    return g, x, w, bn_of(Cout, g)


def test_pointwise_with_residual_and_relu(dev, engine):
    g, x, w, bn = layer_inputs(11)
    res = torch.randn(2, 256, 9, 13, generator=g)
    pc = IE._pw(w.to(dev), bn.to(dev))
    with kernels() as names:
        out = core.conv_rows(as_rows(x, dev), pc, relu=True, res=as_rows(res, dev))
    assert any(n.startswith("k_gemm_h2") for n in names) == (engine == "split-f16"), names
    sc, bi = bn_terms(bn.cpu())
    judge_layer(out.t, [(rows_of(x), w[:, :, 0, 0].t())], engine, "1x1 + residual + ReLU", scale=sc, bias=bi, res=rows_of(res), relu=True)
    core.check_h2_overflow()


@pytest.mark.parametrize("k,stride,pad,Cout", [(3, 2, 1, 64), (1, 2, 0, 256)])
def test_strided_layers(dev, engine, k, stride, pad, Cout):
    g, x, w, bn = layer_inputs(20 + k, Cout=Cout, k=k)
    pc = (IE._c3 if k == 3 else IE._pw)(w.to(dev), bn.to(dev), stride)
    with kernels() as names:
        out = core.conv_rows(as_rows(x, dev), pc, relu=k == 3)
    assert any(n.startswith("k_gemm_h2") for n in names) == (engine == "split-f16"), names
    pairs, (Ho, Wo) = taps2d(x, w, stride, pad)
    assert (out.X, out.Y, out.C) == (Ho, Wo, Cout) == (5, 7, Cout)
    sc, bi = bn_terms(bn.cpu())
    judge_layer(out.t, pairs, engine, "%dx%d stride %d" % (k, k, stride), scale=sc, bias=bi, relu=k == 3)
    core.check_h2_overflow()


def test_neck_deblocks_write_their_slices(dev, engine):
    """Conv 4x4 / 4, Conv 2x2 / 2 and deconv 1x1 / 1 onto a 9 x 13 map (from 36x52, 18x26, 9x13), deconv 2x2 / 2 onto 8 x 12 (from
    4x6): each writes its slice -- [0,32) [32,96) [96,128) [128,192) -- of a 192-column buffer filled with a sentinel.  Every slice is
    judged alone against float64, the deconvolution child by child; the rest of the buffer keeps the sentinel."""
    oc = [32, 64, 32, 64]
    neck = IE.SECONDFPN(in_channels=[64] * 4, out_channels=oc, upsample_strides=[0.25, 0.5, 1, 2])
    sd = R.fixture_state_dict(neck.state_dict(), 41, R.transposed_keys([0.25, 0.5, 1, 2]))
    neck.load_state_dict(sd)
    neck = neck.to(dev).eval()
    g = torch.Generator().manual_seed(42)
    offs = [0, 32, 96, 128]
    for i, (Hi, Wi, Ho, Wo) in enumerate([(36, 52, 9, 13), (18, 26, 9, 13), (9, 13, 9, 13), (4, 6, 8, 12)]):
        x = torch.randn(2, 64, Hi, Wi, generator=g) * torch.tensor([1.0, 2.5]).view(2, 1, 1, 1)
        buf = torch.full((2 * Ho * Wo, 192), -7.0, device=dev)
        neck.deblock_rows(i, as_rows(x, dev), buf, offs[i])
        torch.cuda.synchronize()
        got = buf.cpu()
        keep = torch.ones(192, dtype=torch.bool)
        keep[offs[i]:offs[i] + oc[i]] = False
        assert bool((got[:, keep] == -7.0).all()), "deblock %d wrote outside its slice" % i
        w = sd["deblocks.%d.0.weight" % i]
        bnm = neck.deblocks[i][1].cpu()
        sc, bi = bn_terms(bnm)
        sl = got[:, offs[i]:offs[i] + oc[i]]
        if i < 2:
            k = 4 if i == 0 else 2
            pairs, size = taps2d(x, w, k, 0)
            assert size == (Ho, Wo)
            judge_layer(sl, pairs, engine, "neck conv %dx%d / %d" % (k, k, k), scale=sc, bias=bi, relu=True)
        else:
            s = 1 if i == 2 else 2
            sl = as_bchw(sl, 2, Ho, Wo)
            for di in range(s):
                for dj in range(s):                       # child (di, dj) of coarse pixel (i, j) lands at (s i + di, s j + dj)
                    child = rows_of(sl[:, :, di::s, dj::s])
                    judge_layer(child, [(rows_of(x), w[:, :, di, dj].double())], engine, "neck deconv %dx%d child (%d,%d)" % (s, s, di, dj),
                                scale=sc, bias=bi, relu=True)
    core.check_h2_overflow()


# ------------------------------------------------------------------ 4. the modules against float64
NECK_KW = dict(in_channels=[256, 512, 1024, 2048], upsample_strides=[0.25, 0.5, 1, 2], out_channels=[128] * 4)


def build_pair(depth, seed, dev):
    bb = IE.ResNet(depth=depth, num_stages=4, out_indices=(0, 1, 2, 3), frozen_stages=0, norm_cfg=dict(type='BN', requires_grad=True),
                   norm_eval=False, style='pytorch')
    nk = IE.SECONDFPN(**NECK_KW)
    sdb = R.fixture_state_dict(bb.state_dict(), seed)
    sdn = R.fixture_state_dict(nk.state_dict(), seed + 1, R.transposed_keys(NECK_KW["upsample_strides"]))
    bb.load_state_dict(sdb, strict=True)
    nk.load_state_dict(sdn, strict=True)
    return bb.to(dev).eval(), nk.to(dev).eval(), sdb, sdn


def refs(x, sdb, sdn, depth):
    out = {}
    for dt in (torch.float64, torch.float32):
        with torch.no_grad():
            feats = R.resnet(x.to(dt), R.cast(sdb, dt), depth)
            out[dt] = (feats, R.second_fpn(feats, R.cast(sdn, dt), NECK_KW["upsample_strides"])[0])
    return out[torch.float64], out[torch.float32]


@pytest.fixture(scope="module")
def r50(dev):
    bb, nk, sdb, sdn = build_pair(50, 50, dev)
    x = R.fixture_images(2, 64, 96, 51)
    r64, r32 = refs(x, sdb, sdn, 50)
    return dict(bb=bb, nk=nk, sdb=sdb, sdn=sdn, x=x, r64=r64, r32=r32)


def check_encoder(dev, bb, nk, x, r64, r32, what):
    for a, b in zip(r32[0] + (r32[1],), r64[0] + (r64[1],)):
        assert rel_err(a, b) <= TOL / 4, "the fp32 restatement itself is %g from float64" % rel_err(a, b)
    with torch.no_grad(), kernels() as names:
        core.TIMER.enabled = 2                                # every C-ABI call is a region: a layout conversion would show
        feats = bb(x.to(dev))
        out = nk(feats)
    assert isinstance(feats, tuple) and isinstance(out, list) and len(out) == 1
    assert names.get("k_img_stem") == 1 and not any("ndhwc" in n or "zyx_to_rows" in n for n in names), names
    for i, (f, want) in enumerate(zip(feats, r64[0])):
        assert tuple(f.shape) == tuple(want.shape)
        r = IE.rows_of_bchw(f)
        assert r is not None and f.data_ptr() == r.t.data_ptr() and IE.bchw_to_rows(f) is r       # a zero-copy view that remembers its Rows
        assert_close(f.cpu(), want, what="%s stage %d" % (what, i))
    assert tuple(out[0].shape) == tuple(r64[1].shape) and IE.rows_of_bchw(out[0]) is not None
    assert_close(out[0].cpu(), r64[1], what=what + " neck")
    core.check_h2_overflow()
    return feats, out[0]


def test_resnet50_and_neck_against_float64(dev, r50):
    check_encoder(dev, r50["bb"], r50["nk"], r50["x"], r50["r64"], r50["r32"], "ResNet-50")
    with torch.no_grad():                                  # Rows end to end (the backbone writes the neck's H2 operands): same function
        fused = IE.run_image_encoder(r50["bb"], r50["nk"], r50["x"].to(dev))
    assert_close(IE.rows_as_bchw(fused).cpu(), r50["r64"][1], what="run_image_encoder")
    core.check_h2_overflow()


def test_resnet101_and_neck_against_float64(dev):
    bb, nk, sdb, sdn = build_pair(101, 101, dev)
    x = R.fixture_images(2, 64, 96, 102)
    r64, r32 = refs(x, sdb, sdn, 101)
    check_encoder(dev, bb, nk, x, r64, r32, "ResNet-101")


def test_sizes_that_are_no_multiple_of_32(dev, r50):
    x = R.fixture_images(2, 70, 90, 70)
    with torch.no_grad():
        want = R.resnet(x.double(), R.cast(r50["sdb"], torch.float64), 50)
        w32 = R.resnet(x, r50["sdb"], 50)
        feats = r50["bb"](x.to(dev))
    assert [tuple(f.shape[2:]) for f in feats] == [(18, 23), (9, 12), (5, 6), (3, 3)]
    for i, (f, a, b) in enumerate(zip(feats, w32, want)):
        assert rel_err(a, b) <= TOL / 4
        assert_close(f.cpu(), b, what="70x90 stage %d" % i)
    with pytest.raises(ValueError) as e:
        r50["nk"](feats)
    assert "(18, 23)" in str(e.value) and "(6, 6)" in str(e.value)
    core.check_h2_overflow()


def test_train_mode_and_cpu_tensors_are_refused(dev, r50):
    bb, nk = r50["bb"], r50["nk"]
    try:
        bb.train(), nk.train()
        with pytest.raises(NotImplementedError) as e:
            bb(r50["x"].to(dev))
        assert ".eval()" in str(e.value)
        with pytest.raises(NotImplementedError):
            nk([torch.zeros(2, c, 2, 3, device=dev) for c in NECK_KW["in_channels"]])
    finally:
        bb.eval(), nk.eval()
    with pytest.raises(pkg._lib.CooccError):
        bb(r50["x"])
    with pytest.raises(pkg._lib.CooccError):
        nk([torch.zeros(2, c, h, w) for c, (h, w) in zip(NECK_KW["in_channels"], [(16, 24), (8, 12), (4, 6), (2, 3)])])


def test_load_state_dict_repacks(dev, r50):
    bb = build_pair(50, 60, dev)[0]
    x = r50["x"].to(dev)
    with torch.no_grad():
        first = bb(x)[3].clone()
        bb.load_state_dict(r50["sdb"])
        second = bb(x)[3]
        want = r50["bb"](x)[3]
    assert bits_equal(second, want) and not bits_equal(first, second)


# ------------------------------------------------------------------ 5. one captured graph
def test_backbone_and_neck_in_one_captured_graph(dev, r50):
    bb, nk = r50["bb"], r50["nk"]
    xa, xb = r50["x"].to(dev), R.fixture_images(2, 64, 96, 77).to(dev)
    with torch.no_grad():
        want_a, want_b = nk(bb(xa))[0].clone(), nk(bb(xb))[0].clone()
        static = xa.clone()
        s = torch.cuda.Stream(device=dev)
        s.wait_stream(torch.cuda.current_stream(dev))
        with torch.cuda.stream(s):
            nk(bb(static))                                    # warm-up on the capture stream: packs, scratch buffers
            torch.cuda.synchronize()
            graph = torch.cuda.CUDAGraph()
            with torch.cuda.graph(graph, stream=s):
                out = nk(bb(static))[0]
        torch.cuda.current_stream(dev).wait_stream(s)
        keep = core.stream_scratch(dev, s)
        graph.replay()
        torch.cuda.synchronize()
        assert bits_equal(out, want_a)
        static.copy_(xb)
        graph.replay()
        torch.cuda.synchronize()
        assert bits_equal(out, want_b) and not bits_equal(want_a, want_b)
    assert keep is not None
    core.check_h2_overflow()


# ------------------------------------------------------------------ 6. the detector from raw images
def test_detector_encodes_raw_images(dev):
    oc = [16, 16, 16, 16]
    bcfg = dict(type='ResNet', depth=50, stem_channels=64, base_channels=16, num_stages=4, out_indices=(0, 1, 2, 3), frozen_stages=0,
                norm_cfg=dict(type='BN', requires_grad=True), norm_eval=False, style='pytorch', pretrained='ckpts/none.pth')
    ncfg = dict(type='SECONDFPN', in_channels=[64, 128, 256, 512], upsample_strides=[0.25, 0.5, 1, 2], out_channels=oc)
    cfg = synth.model_cfg(C=32, block_inplanes=(32, 64, 128, 256), out_channels=32, rendering=False)
    cfg["img_view_transformer"] = dict(
        type='ViewTransformerLiftSplatShootVoxel', numC_input=sum(oc), numC_Trans=16, downsample=16, depth_net='hip',
        grid_config={'xbound': [-8., 8., 2.], 'ybound': [-8., 8., 2.], 'zbound': [-2., 2., 2.], 'dbound': [2.0, 10.0, 1.0]},
        data_config={'input_size': (64, 96)})
    torch.manual_seed(8)
    det = pkg.build_detector(cfg, img_backbone=bcfg, img_neck=ncfg, hip_image_encoder=True, external_encoders=True)
    assert isinstance(det.img_backbone, IE.ResNet) and isinstance(det.img_neck, IE.SECONDFPN)
    sdb = R.fixture_state_dict(det.img_backbone.state_dict(), 80)
    sdn = R.fixture_state_dict(det.img_neck.state_dict(), 81, R.transposed_keys(ncfg["upsample_strides"]))
    det.img_backbone.load_state_dict(sdb, strict=True)
    det.img_neck.load_state_dict(sdn, strict=True)
    det = det.to(dev).eval()
    img = R.fixture_images(2, 64, 96, 82).view(1, 2, 3, 64, 96)
    want = {}
    for dt in (torch.float64, torch.float32):
        with torch.no_grad():
            feats = R.resnet(img.view(2, 3, 64, 96).to(dt), R.cast(sdb, dt), 50)
            want[dt] = R.second_fpn(feats, R.cast(sdn, dt), ncfg["upsample_strides"])[0]
    assert rel_err(want[torch.float32], want[torch.float64]) <= TOL / 4
    with torch.no_grad():
        enc = det.image_encoder(img.to(dev))
    assert tuple(enc["x"].shape) == (1, 2, sum(oc), 4, 6) and tuple(enc["img_feats"][0].shape) == (1, 2, sum(oc), 4, 6)
    assert_close(enc["x"].cpu().view(2, sum(oc), 4, 6), want[torch.float64], what="detector image_encoder")
    assert bits_equal(enc["img_feats"][0], enc["x"])
    rig = synth.camera_rig(ncam=2, input_size=(64, 96))
    cams = [rig[k].to(dev) for k in ("rots", "trans", "intrins", "post_rots", "post_trans", "bda")]
    with torch.no_grad():
        vol, depth, img_feats, geom = det.extract_img_feat([img.to(dev)] + cams, None)
    assert tuple(vol.shape) == (1, 16, 8, 8, 2) and tuple(depth.shape) == (2, 8, 4, 6)
    assert bool(torch.isfinite(vol).all()) and float(vol.abs().sum()) > 0
    assert float((depth.sum(1) - 1).abs().max()) <= 1e-5
    core.check_h2_overflow()
