"""``DepthNet`` -- P/coocc/image2bev/ViewTransformerLSSBEVDepth.py:351-549 on the HIP engine (training is opt-in): image-neck features
[B*N,Cin,H,W] + the camera-parameter vector [B,N,27] -> [B*N, depth_channels + context_channels, H, W] (depth logits first), what
``ViewTransformerLiftSplatShootVoxel`` turns into the (depth_prob, img_feat) pair of ``lift_splat``.  Same constructor arguments
and state_dict keys as the reference's class (107 entries; a released ``img_view_transformer.depth_net.*`` loads strictly).

Inside everything is channels-last rows [B*N*H*W, C] (``core.Rows`` with X = H, Y = W, Z = 1, one camera after the other):
the 3x3 convolutions are 3x3x1 ``PackedConv``s through ``core.conv_rows`` (Winograd / split-f16 like SECOND3D's) with BN folded,
1x1 convolutions and the two MLPs go through ``core.linear_rows``, the dilated ASPP branches are row-table GEMMs over a
[9, B*N*H*W] neighbour table (csrc/depthnet.hip k_nbr_table2d: -1 in the padding and across cameras; taps that are dead on the
whole map are left out), the pooled ASPP branch is a
per-camera bias of ASPP's 1x1, and the deformable convolution is a gather into per-group column matrices (k_dcn_cols) + one GEMM
per group.  mmcv's DCN is restated, not linked: DESIGN.md 10 gives the definition.  The submodules below only hold parameters under
the reference's names; ``DepthNet.forward`` is the one forward.  No CPU or eager-PyTorch fallback.

Training is opt-in (``DepthNet.train_enabled``, default False: ``train()`` then raises).  With it on, the ``train()`` forward is
differentiable in every parameter and in x: batch-statistics BN on rows (``autograd.BatchNormRowsFn``; running statistics updated
as torch does), the 3x3 layers through ``autograd.conv_bn_rows`` as 3x3x1 kernels (``autograd.ConvRowsFn``, the Function of every
dense convolution), the 1x1 layers / MLPs through ``autograd.linear_rows``, the dilated branches through
``lidar_hd.SparseConvV1Fn`` over the live-tap rows of the neighbour table, and the Functions below over the training kernels of
csrc/depthnet.hip: the deformable convolution (``DcnRowsFn``: column matrices recomputed per chunk in the backward, dx by fp32
atomics -- the one place whose bits may differ from run to run), the SE gates, the camera means / camera vector of the pooled
branch (added un-normalised before ``bn1``), dropout with a device-drawn mask.
"""
import math

import torch
from torch import nn

from . import _lib, core
from ._lib import call, ptr
from .core import PackCache, PackedConv, Rows, conv_rows, fold_bn, linear_rows

_F32, _I32 = torch.float32, torch.int32
# rows of the deformable convolution's column matrix that exist at a time: [DCN_CHUNK_ROWS, 9 * C] floats of per-stream scratch
# (the whole matrix of a 6 x 56 x 100 map at 512 channels would be 33 600 x 4 608 floats = 619 MB)
DCN_CHUNK_ROWS = 8192
ASPP_DILATIONS = (6, 12, 18)
DCN_GROUPS = 4


class BasicBlock(nn.Module):
    """mmdet 2.14's ResNet BasicBlock(planes, planes): conv1 3x3 (no bias), bn1, ReLU, conv2 3x3 (no bias), bn2, + identity, ReLU."""

    def __init__(self, inplanes, planes):
        super().__init__()
        self.conv1 = nn.Conv2d(inplanes, planes, 3, padding=1, bias=False)
        self.bn1 = nn.BatchNorm2d(planes)
        self.conv2 = nn.Conv2d(planes, planes, 3, padding=1, bias=False)
        self.bn2 = nn.BatchNorm2d(planes)


class _ASPPModule(nn.Module):
    def __init__(self, inplanes, planes, kernel_size, dilation):
        super().__init__()
        self.atrous_conv = nn.Conv2d(inplanes, planes, kernel_size, padding=0 if kernel_size == 1 else dilation, dilation=dilation,
                                     bias=False)
        self.bn = nn.BatchNorm2d(planes)
        nn.init.kaiming_normal_(self.atrous_conv.weight)


class ASPP(nn.Module):
    """:382-452: 1x1 + three dilated 3x3 branches + the pooled branch, concatenated into a 1x1 (Dropout is the identity in eval)."""

    def __init__(self, inplanes, mid_channels):
        super().__init__()
        self.aspp1 = _ASPPModule(inplanes, mid_channels, 1, 1)
        self.aspp2 = _ASPPModule(inplanes, mid_channels, 3, ASPP_DILATIONS[0])
        self.aspp3 = _ASPPModule(inplanes, mid_channels, 3, ASPP_DILATIONS[1])
        self.aspp4 = _ASPPModule(inplanes, mid_channels, 3, ASPP_DILATIONS[2])
        self.global_avg_pool = nn.Sequential(nn.AdaptiveAvgPool2d((1, 1)), nn.Conv2d(inplanes, mid_channels, 1, bias=False),
                                             nn.BatchNorm2d(mid_channels), nn.ReLU())
        self.conv1 = nn.Conv2d(5 * mid_channels, mid_channels, 1, bias=False)
        self.bn1 = nn.BatchNorm2d(mid_channels)
        self.dropout = nn.Dropout(0.5)                  # :414; parameter-free: the training forward reads its p
        for m in (self.global_avg_pool[1], self.conv1):
            nn.init.kaiming_normal_(m.weight)


class Mlp(nn.Module):
    def __init__(self, in_features, hidden_features, out_features):
        super().__init__()
        self.fc1 = nn.Linear(in_features, hidden_features)
        self.fc2 = nn.Linear(hidden_features, out_features)


class SELayer(nn.Module):
    def __init__(self, channels):
        super().__init__()
        self.conv_reduce = nn.Conv2d(channels, channels, 1, bias=True)
        self.conv_expand = nn.Conv2d(channels, channels, 1, bias=True)


class DeformConv2dPack(nn.Module):
    """Parameters of mmcv 1.4.0's DeformConv2dPack(c, c, 3, padding=1, groups=4, deform_groups=1, bias=False): ``weight``
    [c, c/4, 3, 3] and the zero-initialised ``conv_offset`` = Conv2d(c, 18, 3, padding=1)."""

    def __init__(self, channels, groups=DCN_GROUPS):
        super().__init__()
        if channels % groups or (channels // groups) % 4:
            raise ValueError("DepthNet: the deformable convolution needs mid_channels / %d to be a multiple of 4, got %d"
                             % (groups, channels))
        self.groups = groups
        self.weight = nn.Parameter(torch.empty(channels, channels // groups, 3, 3))
        stdv = 1.0 / math.sqrt(channels // groups * 9)
        nn.init.uniform_(self.weight, -stdv, stdv)
        self.conv_offset = nn.Conv2d(channels, 18, 3, padding=1, bias=True)
        nn.init.zeros_(self.conv_offset.weight)
        nn.init.zeros_(self.conv_offset.bias)


# ------------------------------------------------------------------ launch helpers (rows in, rows out)
def conv3x3_pack(weight, bn=None, bias=None, cout_to=None):
    """A Conv2d 3x3 stride-1 padding-1 weight [N,C,3,3] as the engine's 3x3x1 layer on Rows with X = H, Y = W, Z = 1 (tap 3i + j).
    ``cout_to``: zero-pad the output channels (zero weights, zero bias) so the rows stay 16-byte aligned."""
    w = weight.detach()
    if cout_to and cout_to > w.shape[0]:
        assert bn is None
        extra = cout_to - w.shape[0]
        b = bias.detach() if bias is not None else w.new_zeros(w.shape[0])
        w, bias = torch.cat([w, w.new_zeros(extra, *w.shape[1:])], 0), torch.cat([b, b.new_zeros(extra)])
    return PackedConv(w.unsqueeze(-1), bn=bn, bias=bias, kernel=(3, 3, 1))


ALL_TAPS = tuple(range(9))
_TRAIN_OFF = ("DepthNet: training on the HIP engine is opt-in: set DepthNet.train_enabled = True "
              "(ViewTransformerLiftSplatShootVoxel(depth_net='hip', train_depth_net=True)), or call .eval()")


def live_taps(H, W, dil):
    """The taps 3i + j of a 3x3 convolution with dilation = padding = ``dil`` that reach a real pixel from at least one pixel of an
    H x W map.  The others read nothing but padding (on a 16-row map every vertical tap of dilation 18): leaving them out of the
    table and the pack is exact."""
    return tuple(3 * i + j for i in range(3) for j in range(3) if (i == 1 or dil < H) and (j == 1 or dil < W))


def table_pack(weight, bn=None, taps=ALL_TAPS):
    """A Conv2d 3x3 weight [N,C,3,3] as a row-table layer over ``taps`` (tap 3i + j; default all nine): the dilated convolutions."""
    w = weight.detach()
    w = w.reshape(w.shape[0], w.shape[1], 9)
    if tuple(taps) != ALL_TAPS:
        w = w[:, :, list(taps)]
    return PackedConv(w.contiguous(), bn=bn, taps=len(taps))


def neighbour_table(BN, H, W, dil, device):
    """[9, BN*H*W] int32: the row tap 3i + j of a 3x3 convolution with dilation = padding = ``dil`` reads, -1 where it falls into
    the padding (a camera's taps never reach another camera's rows)."""
    t = torch.empty(9, BN * H * W, device=device, dtype=_I32)
    call("coocc_nbr_table2d", BN, H, W, int(dil), ptr(t))
    return t


def table_conv_rows(x2d, pc, table, relu=True, out=None, out_coff=0, x_h2=None):
    """out[:, out_coff:+Cout] = epi(sum_t W_t . x2d[table[t]]) -- one launch of the row-table GEMM (``lidar.sparse_conv``'s kernel:
    k_gemm_h2w<TABLE> with ``x_h2`` = the H2 rows of x2d, the fp32-MFMA row-table kernel otherwise)."""
    taps, M = table.shape
    dev = x2d.device
    Cin = x2d.shape[1]
    assert Cin == pc.Cin and taps == pc.taps and x2d.shape[0] == M
    if out is None:
        out = torch.empty(M, pc.Cout, device=dev, dtype=_F32)
    d = core.conv_desc(dev, in_=ptr(x2d), w=ptr(pc.w), out=ptr(out, offset=out_coff), scale=ptr(pc.scale), bias=ptr(pc.bias),
                       gather=ptr(table, _I32), M=M, Cin=Cin, Cout=pc.Cout, taps=taps, in_stride=Cin, out_stride=out.shape[1],
                       B=1, Xi=M, Yi=1, Zi=1, Xo=1, Yo=1, Zo=1, ksize=1, stride=1, relu=int(relu), splitk=1,
                       tile_hint=core.TILE_HINT)
    name = "k_conv"
    if x_h2 is not None:
        d.in_, d.w, d.mfma_dtype, d.alpha, name = ptr(x_h2), ptr(pc.h2_pack()), 3, 1.0, "k_gemm_h2w"
    core.launch_conv(d, dev, "%s<dilated table %d->%d>" % (name, Cin, pc.Cout), 2.0 * M * Cin * pc.Cout * taps)
    return out


def _h2_engine(C):
    return core.CONV_ENGINE == "h2" and core.CONV_DTYPE == "f32" and C % 32 == 0


def pixel_linear(x2d, pc, relu=False, out=None, out_coff=0, x_h2=None):
    """``linear_rows`` for the per-pixel 1x1 convolutions.  On the split-f16 engine (Cin % 32 == 0 and at least
    ``core.H2_DIRECT_MIN_FLOPS``, the rule of ``core.route``) the GEMM is ``linear_rows_h2`` over the H2 rows of ``x2d`` -- ``x_h2``
    when the caller has them, else one conversion pass -- otherwise the fp32-MFMA kernel."""
    n, Cin = x2d.shape
    if _h2_engine(Cin) and core.H2_DIRECT and 2.0 * n * Cin * pc.Cout >= core.H2_DIRECT_MIN_FLOPS:
        if x_h2 is None:
            x_h2 = core.rows_to_h2(x2d, name="dn_h2")
        return core.linear_rows_h2(x_h2, n, Cin, pc, relu=relu, out=out, out_coff=out_coff)
    return linear_rows(x2d, pc, relu=relu, out=out, out_coff=out_coff)


def dilated_conv_rows(x, pc, dil, table=None, relu=True, out=None, out_coff=0):
    """Conv2d(3x3, dilation = padding = ``dil``) + folded BN (+ ReLU) on Rows [BN, H, W, 1] -> [BN*H*W, Cout] (or into ``out``)."""
    assert x.Z == 1 and x.coff == 0 and x.stride == x.C
    if table is None:
        table = neighbour_table(x.B, x.X, x.Y, dil, x.t.device)
    return table_conv_rows(x.t, pc, table, relu=relu, out=out, out_coff=out_coff, x_h2=core.h2_rows(x) if _h2_engine(x.C) else None)


def dcn_group_packs(weight, groups=DCN_GROUPS):
    """Per group g the Linear [Cout/G, 9 * Cin/G] (k = tap * Cin/G + channel) that reads group g's column matrix."""
    w = weight.detach()
    co = w.shape[0] // groups
    return [PackedConv(w[g * co:(g + 1) * co].permute(0, 2, 3, 1).reshape(co, -1).contiguous()) for g in range(groups)]


def dcn_columns(x, off, m0, n, groups=DCN_GROUPS, cols=None):
    """The sampled column matrices of rows [m0, m0 + n): [groups, n, 9 * C/groups] (csrc/depthnet.hip k_dcn_cols).  ``x``: Rows
    [BN, H, W, 1]; ``off``: [BN*H*W, >= 18] offset rows ((dy, dx) of tap t at columns 2t, 2t + 1)."""
    assert x.Z == 1 and off.shape[0] == x.B * x.V and off.shape[1] >= 18
    K = 9 * (x.C // groups)
    if cols is None:
        cols = torch.empty(groups * n * K, device=x.t.device, dtype=_F32)
    call("coocc_dcn_cols", x.data(), x.stride, ptr(off), off.shape[1], x.B, x.X, x.Y, x.C, groups, m0, n, ptr(cols))
    return cols[:groups * n * K].view(groups, n, K)


def dcn_rows(x, off, packs, groups=DCN_GROUPS, out=None):
    """Deformable 3x3 convolution (DCNv1, padding 1, ``groups`` weight groups, one offset field) of Rows ``x`` with the offset rows
    ``off``: the sampler fills the column matrices of DCN_CHUNK_ROWS rows at a time, then one GEMM per group writes that group's
    output channels (split-f16 engine when 9 * C/groups is a multiple of 32, the fp32-MFMA kernels otherwise)."""
    M, C = x.B * x.V, x.C
    cg = C // groups
    K = 9 * cg
    dev = x.t.device
    if out is None:
        out = torch.empty(M, C, device=dev, dtype=_F32)
    chunk = max(1, min(int(DCN_CHUNK_ROWS), M))
    cols = core.scratch(dev, "dcn_cols", chunk * 9 * C)
    h2 = _h2_engine(K)
    for m0 in range(0, M, chunk):
        n = min(chunk, M - m0)
        cm = dcn_columns(x, off, m0, n, groups, cols)
        dst = out[m0:m0 + n]
        for g, pc in enumerate(packs):
            if h2:
                core.linear_rows_h2(core.rows_to_h2(cm[g], name="dcn_h2"), n, K, pc, out=dst, out_coff=g * cg)
            else:
                linear_rows(cm[g], pc, out=dst, out_coff=g * cg)
    return out


def se_gate2(x, gate_a, gate_b):
    """(x * sigmoid(gate_a[camera]), x * sigmoid(gate_b[camera])) in one pass: Rows x [BN, H, W, 1], gates [BN, C] logits."""
    M = x.B * x.V
    oa = torch.empty(M, x.C, device=x.t.device, dtype=_F32)
    ob = torch.empty(M, x.C, device=x.t.device, dtype=_F32)
    call("coocc_se_gate2", x.data(), x.stride, x.B, x.V, x.C, ptr(gate_a), ptr(gate_b), ptr(oa), ptr(ob))
    return Rows(oa, x.B, x.X, x.Y, x.Z, x.C), Rows(ob, x.B, x.X, x.Y, x.Z, x.C)


def camera_means(x):
    """[BN, C] channel means of every camera's rows (fp64 sums in a fixed order)."""
    dev = x.t.device
    mean = torch.empty(x.B, x.C, device=dev, dtype=_F32)
    ws = core.stream_buffer(dev, "cam_mean", max(1, int(_lib.load().coocc_cam_mean_ws(x.B, x.V, x.C)) // 8), torch.float64)
    call("coocc_cam_mean", x.data(), x.stride, x.B, x.V, x.C, ptr(mean), ptr(ws), ws.numel() * 8)
    return mean


def aspp_packs(aspp):
    mid = aspp.conv1.weight.shape[0]
    w1 = aspp.conv1.weight.detach().reshape(mid, -1)
    scale, _ = fold_bn(aspp.bn1)
    # the pooled branch is constant over a camera's map, so its slice of the concatenation contributes W[:, 4 mid:] . x5 to every
    # pixel of that camera: a per-camera bias (scaled by bn1 like the rest of the 1x1's sum), never a broadcast map
    w5 = (w1[:, 4 * mid:].double().cpu() * scale.double().cpu()[:, None]).float()
    return dict(a1=PackedConv(aspp.aspp1.atrous_conv.weight.detach().reshape(mid, -1), bn=aspp.aspp1.bn),
                dil={}, dil_src=[(m.atrous_conv.weight, m.bn) for m in (aspp.aspp2, aspp.aspp3, aspp.aspp4)],
                gap=PackedConv(aspp.global_avg_pool[1].weight.detach().reshape(mid, -1), bn=aspp.global_avg_pool[2]),
                cat=PackedConv(w1[:, :4 * mid].contiguous(), bn=aspp.bn1),
                pooled=PackedConv(w5.to(w1.device)))


def _dilated_pack(p, k, taps):
    """Branch k's pack over ``taps``, built on first use and kept with the other packs (so it is dropped with them)."""
    pc = p["dil"].get((k, taps))
    if pc is None:
        w, bn = p["dil_src"][k]
        pc = p["dil"][(k, taps)] = table_pack(w, bn=bn, taps=taps)
    return pc


def aspp_rows(x, p, tables, taps=None):
    """ASPP on Rows [BN, H, W, 1]: four branches straight into the [M, 4 mid] concat buffer, the pooled branch as a per-camera bias.
    ``tables``: per dilated branch the rows [len(taps[k]), M] of its neighbour table; ``taps``: per branch the taps those rows belong
    to (default: all nine)."""
    M, mid, dev = x.B * x.V, x.C, x.t.device
    cat = torch.empty(M, 4 * mid, device=dev, dtype=_F32)
    pixel_linear(x.t, p["a1"], relu=True, out=cat, out_coff=0, x_h2=core.h2_rows(x) if _h2_engine(mid) else None)
    for k, tb in enumerate(tables):
        pc = _dilated_pack(p, k, tuple(taps[k]) if taps is not None else ALL_TAPS)
        dilated_conv_rows(x, pc, ASPP_DILATIONS[k], table=tb, relu=True, out=cat, out_coff=(k + 1) * mid)
    x5 = linear_rows(camera_means(x), p["gap"], relu=True)
    cam_bias = linear_rows(x5, p["pooled"])
    y = pixel_linear(cat, p["cat"], relu=False)
    call("coocc_cam_bias_relu", ptr(y), mid, x.B, x.V, mid, ptr(cam_bias), 1)
    return Rows(y, x.B, x.X, x.Y, x.Z, mid)


# ------------------------------------------------------------------ training (DepthNet.train_enabled): differentiable rows
def _ag():
    from . import autograd
    return autograd


def _gemm_rows(dev, src, src_off, src_stride, n, Cin, w3, out, out_off, Cout, h2=False, alpha_dev=None, tag="dcn"):
    """out[:, out_off:+Cout] = src[:, src_off:+Cin] . w3[:, :, 0]^T over n rows: one launch of the Linear kernels with the weights
    [Cout, Cin, 1] packed on the device.  ``h2``: ``src`` holds dense H2 rows [n, Cin] (split-f16 engine)."""
    ag = _ag()
    wp = (ag.pack_weights_h2_dev if h2 else ag.pack_weights_dev)(w3, Cout, Cin, 1, 0)
    d = core.conv_desc(dev, in_=ptr(src, offset=src_off), w=ptr(wp), out=ptr(out, offset=out_off), M=n, Cin=Cin, Cout=Cout, taps=1,
                       in_stride=src_stride, out_stride=out.shape[-1], B=1, Xi=n, Yi=1, Zi=1, Xo=n, Yo=1, Zo=1, ksize=1, stride=1,
                       tile_hint=core.TILE_HINT)
    if h2:
        d.in_stride, d.mfma_dtype, d.alpha, d.alpha_dev = Cin, 3, 1.0, alpha_dev
    core.launch_conv(d, dev, ("k_gemm_h2 " if h2 else "k_conv ") + tag, 2.0 * n * Cin * Cout)


def _dcn_group_weights(weight, groups):
    """Per group the Linear weights [Cout/G, 9 * Cin/G, 1] (k = tap * Cin/G + channel) of ``dcn_group_packs``, on the device."""
    w = weight.detach().float()
    co = w.shape[0] // groups
    return [w[g * co:(g + 1) * co].permute(0, 2, 3, 1).reshape(co, -1, 1).contiguous() for g in range(groups)]


class DcnRowsFn(torch.autograd.Function):
    """``dcn_rows`` (rows x [M, C], offset rows [M, >= 18], weight [C, C/groups, 3, 3]), differentiable in all three.  The backward
    works through the rows DCN_CHUNK_ROWS at a time and RECOMPUTES each chunk's column matrices (the [M, 9 C] matrix is never
    kept): per group dW_g += cols_g^T dout_g (chunks accumulate in order) and dcols_g = dout_g W_g, then coocc_dcn_cols_bwd turns
    dcols into the offset gradient (deterministic) and adds the corner-weighted dcols into dx (fp32 atomics)."""

    @staticmethod
    def forward(ctx, x2d, off2d, weight, geom, groups):
        ag = _ag()
        BN, H, W = geom
        x2d, off2d = x2d.float().contiguous(), off2d.float().contiguous()
        M, C = x2d.shape
        assert M == BN * H * W and off2d.shape[0] == M and off2d.shape[1] >= 18
        cg = C // groups
        K = 9 * cg
        dev = x2d.device
        xr = Rows(x2d, BN, H, W, 1, C)
        out = torch.empty(M, C, device=dev, dtype=_F32)
        chunk = max(1, min(int(DCN_CHUNK_ROWS), M))
        cols = core.scratch(dev, "dcn_cols", chunk * 9 * C)
        ws = _dcn_group_weights(weight, groups)
        h2 = _h2_engine(K) and ag.TRAIN_H2
        for m0 in range(0, M, chunk):
            n = min(chunk, M - m0)
            cm = dcn_columns(xr, off2d, m0, n, groups, cols)
            for g in range(groups):
                src = ag._rows_h2(cm[g], K) if h2 else cm[g]
                _gemm_rows(dev, src, 0, K, n, K, ws[g], out, m0 * C + g * cg, cg, h2=h2, tag="dcn_fwd")
        ctx.save_for_backward(x2d, off2d, weight)
        ctx.cfg = (BN, H, W, groups)
        return out

    @staticmethod
    def backward(ctx, dout):
        x2d, off2d, weight = ctx.saved_tensors
        BN, H, W, groups = ctx.cfg
        M, C = x2d.shape
        cg = C // groups
        K = 9 * cg
        dev = x2d.device
        dout = dout.float().contiguous()
        xr = Rows(x2d, BN, H, W, 1, C)
        chunk = max(1, min(int(DCN_CHUNK_ROWS), M))
        cols = core.scratch(dev, "dcn_cols", chunk * 9 * C)
        dcols = core.scratch(dev, "dcn_dcols", chunk * 9 * C)
        # dcols_g = dout_g . W_g: the "Linear" [K <- cg] whose weight is W_g transposed
        wt = [w[:, :, 0].t().contiguous().view(K, cg, 1) for w in _dcn_group_weights(weight, groups)]
        need_x, need_off, need_w = ctx.needs_input_grad[:3]
        dw = torch.zeros(groups, cg, K, device=dev, dtype=_F32) if need_w else None
        dx = torch.zeros(M, C, device=dev, dtype=_F32)
        doff = torch.empty(M, off2d.shape[1], device=dev, dtype=_F32)
        wsp = core.workspace(dev)
        for i, m0 in enumerate(range(0, M, chunk)):
            n = min(chunk, M - m0)
            dc = dcols[:groups * n * K].view(groups, n, K)
            if need_w:
                cm = dcn_columns(xr, off2d, m0, n, groups, cols)
            for g in range(groups):
                if need_w:
                    with _lib.TIMER.region("k_wgrad<dcn>", 2.0 * n * K * cg):
                        call("coocc_conv_wgrad", ptr(cm[g]), n, K, ptr(dout, offset=m0 * C + g * cg), C, None, n, K, cg, 1, ptr(dw[g]),
                             int(i > 0), ptr(wsp), wsp.numel())
                if need_x or need_off:
                    _gemm_rows(dev, dout, m0 * C + g * cg, C, n, cg, wt[g], dc[g], 0, K, tag="dcn_dgrad")
            if need_x or need_off:
                with _lib.TIMER.region("k_dcn_cols_bwd", 2.0 * 36 * n * C):
                    call("coocc_dcn_cols_bwd", xr.data(), xr.stride, ptr(off2d), off2d.shape[1], BN, H, W, C, groups, m0, n, ptr(dc),
                         ptr(dx), ptr(doff, offset=m0 * off2d.shape[1]))
        if need_w:       # [g][o][t * cg + c] -> [C, cg, 3, 3]
            dw = dw.view(groups * cg, 3, 3, cg).permute(0, 3, 1, 2).contiguous()
        return (dx if need_x else None), (doff if need_off else None), dw, None, None


class SeGate2Fn(torch.autograd.Function):
    """``se_gate2`` on rows, differentiable in x and both gate logits (coocc_se_gate2_bwd)."""

    @staticmethod
    def forward(ctx, x2d, ga, gb, BN, HW):
        x2d, ga, gb = x2d.float().contiguous(), ga.float().contiguous(), gb.float().contiguous()
        C = x2d.shape[1]
        oa, ob = torch.empty_like(x2d), torch.empty_like(x2d)
        call("coocc_se_gate2", ptr(x2d), C, BN, HW, C, ptr(ga), ptr(gb), ptr(oa), ptr(ob))
        ctx.save_for_backward(x2d, ga, gb)
        ctx.cfg = (BN, HW)
        return oa, ob

    @staticmethod
    def backward(ctx, da, db):
        x2d, ga, gb = ctx.saved_tensors
        BN, HW = ctx.cfg
        C = x2d.shape[1]
        dev = x2d.device
        da = da.float().contiguous() if da is not None else torch.zeros_like(x2d)
        db = db.float().contiguous() if db is not None else torch.zeros_like(x2d)
        dx, dga, dgb = torch.empty_like(x2d), torch.empty_like(ga), torch.empty_like(gb)
        ws = core.stream_buffer(dev, "gate_bwd", max(1, int(_lib.load().coocc_se_gate2_bwd_ws(BN, HW, C)) // 8), torch.float64)
        call("coocc_se_gate2_bwd", ptr(x2d), C, BN, HW, C, ptr(ga), ptr(gb), ptr(da), ptr(db), ptr(dx), ptr(dga), ptr(dgb), ptr(ws),
             ws.numel() * 8)
        return dx, dga, dgb, None, None


def _camera_reduce(entry, x2d, BN, HW):
    C = x2d.shape[1]
    out = torch.empty(BN, C, device=x2d.device, dtype=_F32)
    ws = core.stream_buffer(x2d.device, "cam_mean", max(1, int(_lib.load().coocc_cam_mean_ws(BN, HW, C)) // 8), torch.float64)
    call(entry, ptr(x2d), C, BN, HW, C, ptr(out), ptr(ws), ws.numel() * 8)
    return out


class CamMeanFn(torch.autograd.Function):
    """``camera_means`` on rows [BN*HW, C]; backward: every row of camera b receives dmean[b] / HW."""

    @staticmethod
    def forward(ctx, x2d, BN, HW):
        ctx.cfg = (BN, HW)
        return _camera_reduce("coocc_cam_mean", x2d.float().contiguous(), BN, HW)

    @staticmethod
    def backward(ctx, dmean):
        BN, HW = ctx.cfg
        dmean = dmean.float().contiguous()
        dx = torch.empty(BN * HW, dmean.shape[1], device=dmean.device, dtype=_F32)
        call("coocc_cam_add", None, ptr(dx), BN, HW, dmean.shape[1], ptr(dmean), 1.0 / HW)
        return dx, None, None


class CamAddFn(torch.autograd.Function):
    """y[m] = x[m] + v[camera of m]; backward: dx = dy, dv = the per-camera column sums of dy (fp64, fixed order)."""

    @staticmethod
    def forward(ctx, x2d, v, BN, HW):
        x2d, v = x2d.float().contiguous(), v.float().contiguous()
        y = torch.empty_like(x2d)
        call("coocc_cam_add", ptr(x2d), ptr(y), BN, HW, x2d.shape[1], ptr(v), 1.0)
        ctx.cfg = (BN, HW)
        return y

    @staticmethod
    def backward(ctx, dy):
        BN, HW = ctx.cfg
        dy = dy.float().contiguous()
        return dy, (_camera_reduce("coocc_cam_sum", dy, BN, HW) if ctx.needs_input_grad[1] else None), None, None


class DropoutRowsFn(torch.autograd.Function):
    """y = x * mask / (1 - p) on rows with a given uint8 / bool mask [M, C]; the backward is the same kernel on dy."""

    @staticmethod
    def forward(ctx, x2d, mask, p):
        x2d, mask = x2d.float().contiguous(), mask.contiguous()
        assert mask.shape == x2d.shape and mask.element_size() == 1
        y = torch.empty_like(x2d)
        ctx.save_for_backward(mask)
        ctx.scale = 1.0 / (1.0 - float(p))
        call("coocc_dropout_rows", ptr(x2d), ptr(mask), x2d.shape[0], x2d.shape[1], ctx.scale, ptr(y))
        return y

    @staticmethod
    def backward(ctx, dy):
        (mask,) = ctx.saved_tensors
        dy = dy.float().contiguous()
        dx = torch.empty_like(dy)
        call("coocc_dropout_rows", ptr(dy), ptr(mask), dy.shape[0], dy.shape[1], ctx.scale, ptr(dx))
        return dx, None, None


def dropout_rows(x2d, p, generator=None):
    """nn.Dropout(p) in training mode on rows: the mask is drawn on the device with torch's generator; p == 0 is the identity."""
    if p <= 0.0:
        return x2d
    if p >= 1.0:
        raise ValueError("DepthNet: dropout p must be below 1")
    mask = torch.rand(x2d.shape, device=x2d.device, generator=generator) >= p
    return DropoutRowsFn.apply(x2d, mask, p)


def conv3x3_train(x2d, geom, weight, bn=None, bias=None, relu=True, res=None):
    """Conv2d 3x3 padding 1 (-> batch-statistics BN (+ res)) (-> ReLU) on rows through ``autograd.conv_bn_rows`` with kernel (3, 3, 1)."""
    ag = _ag()
    w5 = weight.unsqueeze(-1)
    if bn is None or res is None:
        return ag.conv_bn_rows(x2d, w5, geom, bn=bn, bias=bias, relu=relu)[0]
    return ag.norm_rows(ag.conv_bn_rows(x2d, w5, geom, bn=None, bias=bias, relu=False)[0], bn, relu=relu, res=res)


def bias_rows(y, bias, geom):
    """y + bias on rows [BN*H*W, C] (C % 4 == 0) with the bias gradient summed in fp64: the bias is handed to ``CamAddFn`` as one
    vector per image row, whose adjoint is ``coocc_cam_sum``'s fixed-order fp64 sum over that row's W pixels; the expand's backward
    adds the BN * H partials.  (The GEMM epilogue's own bias gradient adds 256 rows at a time sequentially in fp32 at widths whose
    quads do not divide a workgroup -- 20, 112 -- which is about twice the error of a pairwise fp32 sum.)"""
    BN, H, W = geom
    return CamAddFn.apply(y, bias.unsqueeze(0).expand(BN * H, -1), BN * H, W)


def dilated_train(x2d, weight, table, taps):
    """Conv2d(3x3, dilation = padding) over the live-tap rows ``table`` [len(taps), M] of the neighbour table, differentiable
    (``lidar_hd.SparseConvV1Fn``).  Stride 1 and dilation = padding: tap 8 - t reads the mirrored pixel, so the transposed book of
    the live taps is the forward table with its rows reversed.  The live taps are a product set (rows i x columns j), so the weight
    handed over is a SLICE of the parameter: the dead taps' gradient is the exact zero of the slice's backward."""
    from .lidar_hd import SparseConvV1Fn
    ii, jj = sorted({t // 3 for t in taps}), sorted({t % 3 for t in taps})
    assert tuple(3 * i + j for i in ii for j in jj) == tuple(taps)
    w = weight[:, :, ii[0]:ii[-1] + 1, jj[0]:jj[-1] + 1].permute(2, 3, 1, 0).unsqueeze(0)          # [1, kh, kw, Cin, Cout]
    return SparseConvV1Fn.apply(x2d, w, table, table.flip(0).contiguous(), None, None, None, None, False)


class _PaddedBN:
    """What ``BatchNormRowsFn`` reads of a norm layer, for BatchNorm1d(cam_channels) on rows padded to a multiple of 4 columns: the
    running statistics it updates are padded copies, and ``commit`` writes the real entries back -- the pad never reaches them."""

    def __init__(self, bn, width):
        self.bn, self.n = bn, bn.num_features
        self.eps, self.momentum, self.track_running_stats = bn.eps, bn.momentum, bn.track_running_stats
        self.num_batches_tracked = bn.num_batches_tracked
        self.running_mean = self.running_var = None
        if bn.running_mean is not None:
            self.running_mean = torch.nn.functional.pad(bn.running_mean.detach().float(), (0, width - self.n))
            self.running_var = torch.nn.functional.pad(bn.running_var.detach().float(), (0, width - self.n), value=1.0)

    def commit(self):
        if self.running_mean is not None and self.track_running_stats:
            with torch.no_grad():
                self.bn.running_mean.copy_(self.running_mean[:self.n])
                self.bn.running_var.copy_(self.running_var[:self.n])


class DepthNet(nn.Module):
    def __init__(self, in_channels, mid_channels, context_channels, depth_channels, cam_channels=27):
        super().__init__()
        if in_channels % 4 or mid_channels % 4:
            raise ValueError("DepthNet: in_channels and mid_channels must be multiples of 4 (16-byte rows)")
        self.in_channels, self.mid_channels = in_channels, mid_channels
        self.context_channels, self.depth_channels, self.cam_channels = context_channels, depth_channels, cam_channels
        self.reduce_conv = nn.Sequential(nn.Conv2d(in_channels, mid_channels, 3, padding=1), nn.BatchNorm2d(mid_channels),
                                         nn.ReLU(inplace=True))
        self.context_conv = nn.Conv2d(mid_channels, context_channels, 1)
        self.bn = nn.BatchNorm1d(cam_channels)
        self.depth_mlp = Mlp(cam_channels, mid_channels, mid_channels)
        self.depth_se = SELayer(mid_channels)
        self.context_mlp = Mlp(cam_channels, mid_channels, mid_channels)
        self.context_se = SELayer(mid_channels)
        self.depth_conv = nn.Sequential(BasicBlock(mid_channels, mid_channels), BasicBlock(mid_channels, mid_channels),
                                        BasicBlock(mid_channels, mid_channels), ASPP(mid_channels, mid_channels),
                                        DeformConv2dPack(mid_channels), nn.Conv2d(mid_channels, depth_channels, 1))
        self._packs = PackCache(self)
        self._tables = {}
        # opt-in: under train() the forward is the differentiable one (batch-statistics BN, dropout, every backward a HIP kernel);
        # off, train() raises as before
        self.train_enabled = False
        # torch.Generator (on the module's device) the dropout mask of the training forward is drawn with; None: the default one
        self.dropout_generator = None

    # ------------------------------------------------------------------ packs
    def _packed(self):
        def build():
            mid, cam = self.mid_channels, self.cam_channels
            cam4 = -(-cam // 4) * 4
            lin = lambda m: PackedConv(m.weight.detach().reshape(m.weight.shape[0], -1), bias=m.bias)
            dev = self.bn.running_mean.device

            def pad(t, fill):
                return torch.cat([t.detach().float(), torch.full((cam4 - cam,), fill, device=dev)]).contiguous()

            def mlp(m, se):
                w1 = m.fc1.weight.detach()
                w1 = torch.cat([w1, w1.new_zeros(w1.shape[0], cam4 - cam)], 1)         # the padded input columns weigh nothing
                return [PackedConv(w1, bias=m.fc1.bias), lin(m.fc2), lin(se.conv_reduce), lin(se.conv_expand)]
            ones, zeros = torch.ones(cam, device=dev), torch.zeros(cam, device=dev)
            dcn = self.depth_conv[4]
            return dict(
                cam4=cam4,
                bn=(pad(self.bn.running_mean, 0.0), pad(self.bn.running_var, 1.0),
                    pad(self.bn.weight if self.bn.weight is not None else ones, 0.0),
                    pad(self.bn.bias if self.bn.bias is not None else zeros, 0.0)),
                reduce=conv3x3_pack(self.reduce_conv[0].weight, bn=self.reduce_conv[1], bias=self.reduce_conv[0].bias),
                context=lin(self.context_conv), context_gate=mlp(self.context_mlp, self.context_se),
                depth_gate=mlp(self.depth_mlp, self.depth_se),
                blocks=[(conv3x3_pack(b.conv1.weight, bn=b.bn1), conv3x3_pack(b.conv2.weight, bn=b.bn2))
                        for b in list(self.depth_conv)[:3]],
                aspp=aspp_packs(self.depth_conv[3]),
                offset=conv3x3_pack(dcn.conv_offset.weight, bias=dcn.conv_offset.bias, cout_to=20),
                dcn=dcn_group_packs(dcn.weight, dcn.groups),
                out=lin(self.depth_conv[5]))
        return self._packs.get_modules((self,), build)

    def _aspp_tables(self, BN, H, W, device):
        """(tables, taps) of the three dilated branches on a [BN, H, W] map: the rows of the neighbour table that belong to the live
        taps, built on the device once per (BN, H, W, dilation)."""
        tables, taps = [], []
        for d in ASPP_DILATIONS:
            key = (BN, H, W, d, device.index)
            t = self._tables.get(key)
            live = live_taps(H, W, d)
            if t is None:
                t = neighbour_table(BN, H, W, d, device)
                if live != ALL_TAPS:
                    t = t[list(live)].contiguous()
                self._tables[key] = t
            tables.append(t)
            taps.append(live)
        return tables, taps

    def _gate(self, cam_rows, packs):
        fc1, fc2, red, exp = packs
        v = linear_rows(linear_rows(cam_rows, fc1, relu=True), fc2)
        return linear_rows(linear_rows(v, red, relu=True), exp)

    def forward_rows(self, x, mlp_input):
        """Rows [BN, H, W, 1] of the image-neck features + [B, N, cam] (or [BN, cam]) camera vectors -> the rows
        [BN*H*W, depth_channels + context_channels] (depth logits first)."""
        if self.training:
            if not self.train_enabled:
                raise NotImplementedError(_TRAIN_OFF)
            assert x.Z == 1 and x.coff == 0 and x.stride == x.C
            return self.forward_rows_train(x.t, (x.B, x.X, x.Y), mlp_input)
        p = self._packed()
        dev = x.t.device
        BN, H, W, mid = x.B, x.X, x.Y, self.mid_channels
        M = BN * H * W
        cam = mlp_input.reshape(-1, mlp_input.shape[-1]).float()
        if cam.shape != (BN, self.cam_channels):
            raise ValueError("DepthNet: mlp_input %s does not hold %d cameras of %d numbers"
                             % (tuple(mlp_input.shape), BN, self.cam_channels))
        cam4 = p["cam4"]
        if cam4 != self.cam_channels:
            cam = torch.nn.functional.pad(cam, (0, cam4 - self.cam_channels))
        cam = cam.contiguous()
        camn = torch.empty_like(cam)
        mean, var, gamma, beta = p["bn"]
        call("coocc_bn_apply", ptr(cam), BN, cam4, ptr(mean), ptr(var), ptr(gamma), ptr(beta), float(self.bn.eps), None, 0, ptr(camn))
        blocks = p["blocks"]
        x = conv_rows(x, p["reduce"], relu=True)
        ctx, dep = se_gate2(x, self._gate(camn, p["context_gate"]), self._gate(camn, p["depth_gate"]))
        D, Cc = self.depth_channels, self.context_channels
        out = torch.empty(M, D + Cc, device=dev, dtype=_F32)
        pixel_linear(ctx.t, p["context"], out=out, out_coff=D)
        h = dep
        for i, (c1, c2) in enumerate(blocks):
            t = conv_rows(h, c1, relu=True, twin_for=(c2,))
            h = conv_rows(t, c2, relu=True, res=h, twin_for=(blocks[i + 1][0],) if i + 1 < len(blocks) else ())
        a = aspp_rows(h, p["aspp"], *self._aspp_tables(BN, H, W, dev))
        off = conv_rows(a, p["offset"], relu=False)
        d = dcn_rows(a, off.t, p["dcn"], self.depth_conv[4].groups)
        pixel_linear(d, p["out"], out=out, out_coff=0)
        return out

    # ------------------------------------------------------------------ training
    def _gate_train(self, camn, m, se, cam4):
        ag = _ag()
        w1 = torch.nn.functional.pad(m.fc1.weight, (0, cam4 - self.cam_channels))       # the padded input columns weigh nothing
        v = ag.linear_rows(ag.linear_rows(camn, w1, m.fc1.bias, relu=True), m.fc2.weight, m.fc2.bias)
        c = se.conv_reduce.weight.shape[0]
        v = ag.linear_rows(v, se.conv_reduce.weight.reshape(c, c), se.conv_reduce.bias, relu=True)
        return ag.linear_rows(v, se.conv_expand.weight.reshape(c, c), se.conv_expand.bias)

    def _aspp_train(self, h, geom):
        ag = _ag()
        aspp = self.depth_conv[3]
        BN, H, W = geom
        mid, dev = self.mid_channels, h.device
        outs = [ag.norm_rows(ag.linear_rows(h, aspp.aspp1.atrous_conv.weight.reshape(mid, mid)), aspp.aspp1.bn, relu=True)]
        tables, taps = self._aspp_tables(BN, H, W, dev)
        for m, tb, tp in zip((aspp.aspp2, aspp.aspp3, aspp.aspp4), tables, taps):
            outs.append(ag.norm_rows(dilated_train(h, m.atrous_conv.weight, tb, tp), m.bn, relu=True))
        w1 = aspp.conv1.weight.reshape(mid, 5 * mid)
        y = ag.linear_rows(torch.cat(outs, 1), w1[:, :4 * mid].contiguous())
        # the pooled branch is constant over a camera's map: its slice of the 1x1 is one vector per camera, added UN-NORMALISED to the
        # four real slices' sum (bn1's batch statistics are those of the whole sum, so nothing can be folded as in eval)
        g = ag.norm_rows(ag.linear_rows(CamMeanFn.apply(h, BN, H * W), aspp.global_avg_pool[1].weight.reshape(mid, mid)),
                         aspp.global_avg_pool[2], relu=True)
        y = CamAddFn.apply(y, ag.linear_rows(g, w1[:, 4 * mid:].contiguous()), BN, H * W)
        y = ag.norm_rows(y, aspp.bn1, relu=True)
        return dropout_rows(y, float(aspp.dropout.p), self.dropout_generator)

    def forward_rows_train(self, x2d, geom, mlp_input):
        """``forward_rows`` under train(): rows [BN*H*W, Cin] (differentiable) of a (BN, H, W) map -> rows [BN*H*W, depth + context].
        Batch-statistics BN everywhere (running statistics updated), dropout after ASPP; ``mlp_input`` takes no gradient."""
        ag = _ag()
        BN, H, W = geom
        g4 = (BN, H, W, 1)
        mid, camc = self.mid_channels, self.cam_channels
        cam = mlp_input.detach().reshape(-1, mlp_input.shape[-1]).float()
        if cam.shape != (BN, camc):
            raise ValueError("DepthNet: mlp_input %s does not hold %d cameras of %d numbers" % (tuple(mlp_input.shape), BN, camc))
        if BN < 2:
            raise ValueError("DepthNet: train() needs more than one camera map per batch (batch statistics of one value per channel "
                             "in the pooled ASPP branch), got %d" % BN)
        if not x2d.is_cuda or not cam.is_cuda:
            raise _lib.CooccError("DepthNet runs on the GPU only (no CPU fallback)")
        cam4 = -(-camc // 4) * 4
        cam = torch.nn.functional.pad(cam, (0, cam4 - camc)).contiguous()
        shim = _PaddedBN(self.bn, cam4)
        ones, zeros = cam.new_ones(camc), cam.new_zeros(camc)
        gamma = torch.nn.functional.pad(self.bn.weight if self.bn.weight is not None else ones, (0, cam4 - camc))
        beta = torch.nn.functional.pad(self.bn.bias if self.bn.bias is not None else zeros, (0, cam4 - camc))
        camn = ag.BatchNormRowsFn.apply(cam, gamma, beta, None, shim, False, None)
        shim.commit()
        x = conv3x3_train(x2d.contiguous(), g4, self.reduce_conv[0].weight, bn=self.reduce_conv[1], bias=self.reduce_conv[0].bias)
        ctx, h = SeGate2Fn.apply(x, self._gate_train(camn, self.context_mlp, self.context_se, cam4),
                                 self._gate_train(camn, self.depth_mlp, self.depth_se, cam4), BN, H * W)
        cc = self.context_conv
        context = ag.linear_rows(ctx, cc.weight.reshape(cc.weight.shape[0], mid), cc.bias)
        for b in list(self.depth_conv)[:3]:
            t = conv3x3_train(h, g4, b.conv1.weight, bn=b.bn1)
            h = conv3x3_train(t, g4, b.conv2.weight, bn=b.bn2, res=h)
        a = self._aspp_train(h, geom)
        dcn = self.depth_conv[4]
        co = dcn.conv_offset
        # 18 offset channels in 20-column rows (16-byte rows): two zero filters, whose gradient the pad's backward drops
        w20 = torch.nn.functional.pad(co.weight, (0, 0, 0, 0, 0, 0, 0, 2))
        b20 = torch.nn.functional.pad(co.bias, (0, 2))
        off = bias_rows(conv3x3_train(a, g4, w20, relu=False), b20, geom)
        d = DcnRowsFn.apply(a, off, dcn.weight, geom, dcn.groups)
        last = self.depth_conv[5]
        depth = ag.linear_rows(d, last.weight.reshape(last.weight.shape[0], mid), None if last.weight.shape[0] % 4 == 0 else last.bias)
        if last.weight.shape[0] % 4 == 0:
            depth = bias_rows(depth, last.bias, geom)
        return torch.cat([depth, context], 1)

    def forward(self, x, mlp_input):
        """x [BN,Cin,H,W], mlp_input [B,N,cam] -> [BN, depth_channels + context_channels, H, W] (a zero-copy view of channels-last
        rows).  Under train() (``train_enabled``) the same shapes from the differentiable forward."""
        if self.training and not self.train_enabled:
            raise NotImplementedError(_TRAIN_OFF)
        if not torch.is_tensor(x) or x.dim() != 4:
            raise ValueError("DepthNet: expected a [B*N,C,H,W] tensor")
        BN, C, H, W = x.shape
        if self.training and BN < 2:
            raise ValueError("DepthNet: train() needs more than one camera map per batch (batch statistics of one value per channel "
                             "in the pooled ASPP branch), got %d" % BN)
        if not x.is_cuda or not mlp_input.is_cuda:
            raise _lib.CooccError("DepthNet runs on the GPU only (no CPU fallback)")
        if C != self.in_channels:
            raise ValueError("DepthNet: %d input channels, built for %d" % (C, self.in_channels))
        if self.training:
            rows = x.float().permute(0, 2, 3, 1).reshape(BN * H * W, C)         # torch plumbing: the gradient of x flows back through it
            out = self.forward_rows_train(rows, (BN, H, W), mlp_input)
        else:
            out = self.forward_rows(core.to_rows(x.unsqueeze(-1)), mlp_input)
        return out.view(BN, H, W, out.shape[1]).permute(0, 3, 1, 2)
