"""``SparseEncoderHD`` -- the sparse middle encoder of ``COOCC_Ray_L`` (projects/configs/coocc_nusc/coocc_lidar.py;
P/coocc/voxel_encoder/sparse_encoder_hd.py, mmdet3d/ops/sparse_block.py, mmdet3d/ops/spconv/{conv,ops,structure}.py) on the HIP
sparse engine: upstream's constructor arguments, defaults, ``forward(voxel_features, coors, batch_size)`` signature, state_dict
keys and spconv **v1** weight shapes ``[kd, kh, kw, Cin, Cout]``, so an upstream checkpoint loads with ``strict=True``.

Upstream runs on the spconv v1 that mmdetection3d vendors; its SubMConv3d / SparseConv3d semantics are restated as in
``lidar.py``: a rule book is a ``[taps, M]`` table of input rows and every convolution + folded eval-mode BN1d + ReLU
(+ residual) is ONE ``lidar.sparse_conv`` launch.  What the 8x / 4x encoders never needed is the per-axis geometry
(``coocc_sparse_conv_table3`` / ``coocc_sparse_down_flags3``: the config's third down-convolution pads ``[0,1,1]``) and the 1x1x1
``conv_out``, which writes straight into the zeroed dense volume through the GEMM's ``out_rows`` scatter.

Batch size 1.  Eval mode by default: ``train()`` runs the differentiable forward (batch-statistics BN1d, gradients through the same
rule books; the section "training" below) only when ``train_enabled`` is set -- what the detectors' ``train_sparse_encoder_hd`` option
does -- and refuses by name otherwise.  The class is NOT in ``lidar.MIDDLE_ENCODERS``: the detectors build it only under
``sparse_encoder_hd=True`` and ``register_into_mmdet(sparse_encoder_hd=True)`` writes it into mmdet3d's registry."""
import os

import torch
from torch import nn

from . import _lib, core, lidar
from ._lib import call, ptr
from .core import PackCache, PackedConv, Rows, fold_bn, stream_buffer
from .registry import Registry

_F32, _I32 = torch.float32, torch.int32
MIDDLE_ENCODERS_HD = Registry("middle_encoder_hd")
# split-f16 engine: feature widths below 32 (the 16-wide first stage) are carried as 32-channel rows whose upper channels are exact
# zeros (zero weight rows / columns, zero folded scale and bias), as ``lidar._SparseEncoderBase._packed`` does, so that stage runs
# the split-f16 rule-book kernel; 0 = it runs the fp32-MFMA kernels on 16-wide rows.  The default of a new module
# (``SparseEncoderHD.wide16``).  It is the 8x encoder's measured choice carried over, not yet a measurement of this module:
# tools/bench_sparse_hd.py times both forms and no run of it is recorded.
WIDE16 = os.environ.get("COOCC_HD_WIDE16", "1") != "0"


def _triple(v, what):
    if isinstance(v, (list, tuple)):
        if len(v) != 3:
            raise ValueError("SparseEncoderHD: %s %r is neither an int nor three per-axis (z, y, x) values" % (what, v))
        return tuple(int(a) for a in v)
    return (int(v),) * 3


def conv_out_size(shape, kernel, stride, pad):
    """ops.py get_conv_output_size per axis (dilation 1)."""
    return tuple((n + 2 * p - k) // s + 1 for n, k, s, p in zip(shape, kernel, stride, pad))


# ----------------------------------------------------------------------------- rule books
# (device, stream) -> generation of the level whose voxels the stream's shared index map holds right now.  Only an integer is kept:
# a finished level (its coordinates, its cached tables) is not held alive by the bookkeeping.
_MAP_GEN = {}
_NEXT_GEN = [0]


class SparseLevel:
    """Active voxels of one resolution: coors [M,3] (z,y,x) int32, spatial shape (D,H,W).  The dense int32 index map (166 MB at
    65 x 800 x 800), the flag volume and the compaction scratch are per-stream buffers (``core.stream_buffer``) shared by every
    level and every sample; the map is cleared by a full memset when a level (re)builds it -- see DESIGN.md section 8."""

    def __init__(self, coors, shape, dense_rows=None):
        self.coors, self.shape = coors, tuple(int(v) for v in shape)
        self.books = {}
        self._dense_rows = dense_rows
        self.cleared_bytes = 0                      # bytes of shared scratch this level cleared (index map, flag volume)
        _NEXT_GEN[0] += 1
        self._gen = _NEXT_GEN[0]

    @property
    def M(self):
        return self.coors.shape[0]

    def index_map(self):
        dev = self.coors.device
        D, H, W = self.shape
        m = stream_buffer(dev, "hd_map", D * H * W, _I32)
        key = (dev.index, _lib.stream(dev).value or 0)
        if _MAP_GEN.get(key) != (self._gen, m.data_ptr()):
            _MAP_GEN[key] = None                    # an error below leaves no owner: the next user clears the buffer again
            if self.M:
                call("coocc_sparse_index_map", ptr(self.coors), self.M, D, H, W, ptr(m))
            else:
                m[:D * H * W].fill_(-1)
            self.cleared_bytes += 4 * D * H * W
            _MAP_GEN[key] = (self._gen, m.data_ptr())
        return m

    def table(self, kernel=(3, 3, 3)):
        """Rule book of SubMConv3d(kernel) -- outputs = inputs, padding k // 2 whatever the layer was given (spconv_ops.h:76-79) --
        or, for (1,1,1), of the 1x1x1 SparseConv3d (conv.py:134-145: the same rows).  One book per resolution and kernel."""
        kernel = tuple(kernel)
        if kernel not in self.books:
            D, H, W = self.shape
            t = torch.empty(kernel[0] * kernel[1] * kernel[2], self.M, device=self.coors.device, dtype=_I32)
            if self.M:
                call("coocc_sparse_conv_table3", ptr(self.coors), self.M, D, H, W, *kernel, 1, 1, 1, *(k // 2 for k in kernel),
                     ptr(self.index_map()), ptr(t))
            self.books[kernel] = t
        return self.books[kernel]

    def downsample(self, kernel, stride, pad):
        """Active set + rule book of SparseConv3d(kernel, stride, pad), each per axis (z,y,x): (SparseLevel of the outputs in ascending
        (z,y,x) order, table [taps, Mo])."""
        kernel, stride, pad = tuple(kernel), tuple(stride), tuple(pad)
        D, H, W = self.shape
        Do, Ho, Wo = conv_out_size(self.shape, kernel, stride, pad)
        if min(Do, Ho, Wo) <= 0:
            raise ValueError("SparseConv3d(kernel %r, stride %r, padding %r) leaves no output on a %r grid" % (kernel, stride, pad, self.shape))
        dev = self.coors.device
        total = Do * Ho * Wo
        flags = stream_buffer(dev, "hd_flags", total, torch.uint8)
        call("coocc_sparse_down_flags3", ptr(self.coors), self.M, D, H, W, *kernel, *stride, *pad, Do, Ho, Wo, ptr(flags))
        self.cleared_bytes += total
        lin = stream_buffer(dev, "hd_lin", total, _I32)
        cnt = stream_buffer(dev, "hd_count", 1, _I32)
        ws = stream_buffer(dev, "hd_compact", total // 1024 + 2, _I32)
        call("coocc_compact_flags", ptr(flags), total, ptr(lin), ptr(cnt), ptr(ws), ws.numel() * 4)
        Mo = int(cnt[:1].item())
        coors = torch.empty(Mo, 3, device=dev, dtype=_I32)
        rows = torch.empty(Mo, device=dev, dtype=_I32)
        table = torch.empty(kernel[0] * kernel[1] * kernel[2], Mo, device=dev, dtype=_I32)
        if Mo:                                      # (an input set none of whose voxels reaches an output leaves Mo = 0)
            call("coocc_sparse_lin_to_coors", ptr(lin), Mo, Do, Ho, Wo, ptr(coors), ptr(rows))
            call("coocc_sparse_conv_table3", ptr(coors), Mo, D, H, W, *kernel, *stride, *pad, ptr(self.index_map()), ptr(table))
        return SparseLevel(coors, (Do, Ho, Wo), dense_rows=rows), table

    def dense_rows(self):
        """Channels-last rows (x*H + y)*D + z of the active voxels in the dense [1,C,Z,Y,X] volume."""
        if self._dense_rows is None:
            D, H, W = self.shape
            c = self.coors.long()
            lin = ((c[:, 0] * H + c[:, 1]) * W + c[:, 2]).int().contiguous()
            rows, tmp = torch.empty(self.M, device=lin.device, dtype=_I32), torch.empty_like(self.coors)
            if self.M:
                call("coocc_sparse_lin_to_coors", ptr(lin), self.M, D, H, W, ptr(tmp), ptr(rows))
            self._dense_rows = rows
        return self._dense_rows


# ----------------------------------------------------------------------------- parameter holders (upstream's keys)
class SparseConvV1(nn.Module):
    """Parameter holder with spconv v1's weight layout [kd, kh, kw, Cin, Cout] (key ``weight``; bias-free as
    ``make_sparse_convmodule`` / mmdet's BasicBlock build it)."""

    def __init__(self, cin, cout, kernel, stride=1, padding=0, subm=False):
        super().__init__()
        self.cin, self.cout, self.subm = cin, cout, subm
        self.kernel, self.stride, self.padding = _triple(kernel, "kernel"), _triple(stride, "stride"), _triple(padding, "padding")
        if subm:
            self.stride, self.padding = (1, 1, 1), tuple(k // 2 for k in self.kernel)         # spconv_ops.h:76-79
        self.weight = nn.Parameter(torch.empty(*self.kernel, cin, cout))
        bound = (cin * self.kernel[0] * self.kernel[1] * self.kernel[2]) ** -0.5              # conv.py:106-107 (kaiming_uniform, a = sqrt 5)
        nn.init.uniform_(self.weight, -bound, bound)

    @property
    def taps(self):
        return self.kernel[0] * self.kernel[1] * self.kernel[2]

    def packed(self, bn, cin_to, cout_to):
        """v1 [kd,kh,kw,Cin,Cout] -> the engine's tap-major [Cout, taps * Cin] (tap t = (kd*ky + kh)*kx + kw), input / output
        channels zero-padded to ``cin_to`` / ``cout_to``; the padded outputs get folded scale 0 and bias 0: exact zeros."""
        w = self.weight.detach().float().permute(4, 0, 1, 2, 3).reshape(self.cout, self.taps, self.cin)
        if cin_to > self.cin:
            w = torch.cat([w, w.new_zeros(self.cout, self.taps, cin_to - self.cin)], 2)
        if cout_to > self.cout:
            w = torch.cat([w, w.new_zeros(cout_to - self.cout, self.taps, cin_to)], 0)
        pc = PackedConv(w.reshape(cout_to, -1).contiguous(), tap_major=True, taps=self.taps)
        s, b = fold_bn(bn)
        z = s.new_zeros(cout_to - self.cout)
        dev = self.weight.device
        pc.scale, pc.bias = torch.cat([s, z]).to(dev).contiguous(), torch.cat([b, z]).to(dev).contiguous()
        return pc


def _norm(norm_cfg, c):
    cfg = dict(norm_cfg)
    t = cfg.pop("type", None)
    cfg.pop("requires_grad", None)
    if t != "BN1d":
        raise NotImplementedError("SparseEncoderHD: norm type %r is not built; only 'BN1d' (folded eval-mode statistics on the active rows)" % (t,))
    return nn.BatchNorm1d(c, **cfg)


class _ConvModule(nn.Sequential):
    """make_sparse_convmodule(order=('conv','norm','act')): conv + BN1d + ReLU (keys 0.weight, 1.*)."""

    def __init__(self, cin, cout, kernel, norm_cfg, stride=1, padding=0, subm=False):
        super().__init__(SparseConvV1(cin, cout, kernel, stride, padding, subm), _norm(norm_cfg, cout), nn.ReLU(inplace=True))


class SparseBasicBlockHD(nn.Module):
    """sparse_block.py:68-121 over mmdet's BasicBlock: conv1 SubM k3 -> bn1 -> ReLU -> conv2 SubM k3 -> bn2 -> + identity -> ReLU
    (keys conv1.weight, bn1.*, conv2.weight, bn2.*)."""

    def __init__(self, planes, norm_cfg):
        super().__init__()
        self.conv1 = SparseConvV1(planes, planes, 3, subm=True)
        self.bn1 = _norm(norm_cfg, planes)
        self.conv2 = SparseConvV1(planes, planes, 3, subm=True)
        self.bn2 = _norm(norm_cfg, planes)
        self.relu = nn.ReLU(inplace=True)


# ----------------------------------------------------------------------------- training (opt-in: SparseEncoderHD.train_enabled)
# Under ``train()`` every SparseConvV1 is an autograd Function over the level's forward book and a transposed one:
#   forward  y[o]  = sum_t W_t^T . x[table[t][o]]                row-table GEMM, as inference (no epilogue: BN1d follows)
#   dgrad    dx[i] = sum_t W_t . dy[bwd[t][i]]                   the same GEMM over the TRANSPOSED book.  SubMConv3d: table.flip(0) (the
#                                                                active set is its own mirror image); SparseConv3d:
#                                                                coocc_sparse_dgrad_table3, made on the device from geometry
#   wgrad    dW_t  = sum_o x[table[t][o]] (x) dy[o]              coocc_conv_wgrad with the forward book (fp32 MFMA), or, opt-in,
#                                                                coocc_conv_wgrad_h2t (split-f16, COOCC_HD_WGRAD_H2 below)
# BN1d = ``autograd.BatchNormRowsFn`` on the active rows (batch statistics, running-statistics updates, residual + ReLU inside); its
# apply pass writes the split-f16 twin the next GEMM reads (coocc_bn_apply_ex).  conv_out's rows reach the dense volume through
# ``autograd.ScatterRowsFn``.  The 16-wide first stage trains on 16-wide rows on the fp32-MFMA kernels (no zero-padded columns in
# training: a padded channel would have to be kept out of every BN statistic), whatever ``wide16`` says for inference.
# COOCC_HD_TRAIN_H2 (default 1): forward GEMMs with Cin % 32 == 0 and dgrad GEMMs with Cout % 32 == 0 on the split-f16 row-table
# kernels when COOCC_CONV_ENGINE=h2, COOCC_LIDAR_H2=1 and COOCC_TRAIN_H2=1 (packs made on the device every step, the gradient operand
# scaled by the device-chosen power of two of autograd.TRAIN_H2_DGRAD); 0 = fp32 MFMA everywhere.  MEASURED at the config's size
# (120 000 voxels on [65,800,800], forward + backward, profiles/sparse_hd_train_bench.json): 57.3 ms against 66.0 ms, the forward
# alone 5.1 against 9.2 ms.  Weight gradients are coocc_conv_wgrad (fp32 MFMA) either way and are most of the rest, unless:
# COOCC_HD_WGRAD_H2 (default 0): under the conditions above, the weight gradient of a layer with pad4(Cin) % 32 == 0 and Cout % 32
# == 0 runs on the split-f16 row-table kernel coocc_conv_wgrad_h2t (csrc/wgrad_h2t.hip: operands gathered and split in registers,
# 32-channel x 32/64-output tiles per wave, the gradient operand scaled by the dgrad's device-chosen power of two) instead of the
# fp32 MFMA's 128 x 128 tiles.  conv_input, the 16-wide stage and COOCC_CONV_ENGINE=f32 keep coocc_conv_wgrad.  MEASURED, same
# size (profiles/sparse_hd_wgrad_bench.json, tools/bench_sparse_hd.py --train; per shape in DESIGN.md 8): 1.05-3.2x per layer
# shape, none slower; forward + backward 36.3 ms with 1 against 58.0 ms with 0.  The default stays 0 until a change of its own.
HD_TRAIN_H2 = os.environ.get("COOCC_HD_TRAIN_H2", "1") != "0"
HD_WGRAD_H2 = os.environ.get("COOCC_HD_WGRAD_H2", "0") != "0"
# 1: the dgrad of a strided SparseConv3d runs as one row-table GEMM per residue class of the input rows over that class's live taps
# (1, 2, 4 or 8 of 27 at stride 2); 0: one launch over all taps of the full transposed book (7/8 of whose entries are -1 at stride
# 2).  Same values up to summation order.  MEASURED, same run: the backward takes 52.2 ms either way -- the row-table kernels skip
# a -1 entry cheaply, so 27 mostly empty taps cost no more than eight launches over 1-8 full ones -- while the class lists (a stable
# sort, one host read, the gathers of the sub-tables: 0.50-0.59 ms per down-convolution against 0.02-0.04 ms for the book alone) add
# 1.7 ms to the forward: 59.0 against 57.3 ms per step.  So the default is 0, not the dense path's choice carried over.
HD_DGRAD_CLASSES = os.environ.get("COOCC_HD_DGRAD_CLASSES", "0") != "0"


def _train_h2():
    from . import autograd as ag
    return HD_TRAIN_H2 and core.CONV_ENGINE == "h2" and lidar.LIDAR_H2 and ag.TRAIN_H2


def class_taps(cls, kernel, stride):
    """Taps t = (kd*ky + kh)*kx + kw that can reach an input row of residue class ``cls`` = (rz*sy + ry)*sx + rx: the output
    coordinate (c + p - k) / s is whole on an axis iff k = (c + p) mod s there."""
    rx, ry, rz = cls % stride[2], (cls // stride[2]) % stride[1], cls // (stride[2] * stride[1])
    return [(kd * kernel[1] + kh) * kernel[2] + kw for kd in range(kernel[0]) for kh in range(kernel[1]) for kw in range(kernel[2])
            if kd % stride[0] == rz and kh % stride[1] == ry and kw % stride[2] == rx]


def dgrad_books(level, out_level, kernel, stride, pad, by_class=None):
    """Transposed rule book of the SparseConv3d(kernel, stride, pad) that made ``out_level`` from ``level``:
    (table [taps, Mi] int32, class ids [Mi] int32, classes).  ``classes``: None, or (``by_class``, default COOCC_HD_DGRAD_CLASSES,
    and a stride above 1) the list of (rows int32 [Mc], taps int64 [Tc], table int32 [Tc, Mc]) over the classes that have rows and
    taps -- rows from a stable device sort of the class ids and ONE host read of the class counts."""
    kernel, stride, pad = tuple(kernel), tuple(stride), tuple(pad)
    dev = level.coors.device
    taps, Mi = kernel[0] * kernel[1] * kernel[2], level.M
    table = torch.empty(taps, Mi, device=dev, dtype=_I32)
    cls = torch.empty(Mi, device=dev, dtype=_I32)
    if Mi:
        call("coocc_sparse_dgrad_table3", ptr(level.coors), Mi, *level.shape, *kernel, *stride, *pad, *out_level.shape,
             ptr(out_level.index_map()), ptr(table), ptr(cls))
    if by_class is None:
        by_class = HD_DGRAD_CLASSES
    if not by_class or stride == (1, 1, 1):
        return table, cls, None
    classes = []
    if Mi and out_level.M:
        ncls = stride[0] * stride[1] * stride[2]
        order = torch.sort(cls, stable=True).indices
        counts = _lib.host_read(torch.bincount(cls, minlength=ncls))
        start = 0
        for c, n in enumerate(counts):
            live = class_taps(c, kernel, stride)
            if n and live:
                rows = order[start:start + n]
                t_idx = torch.tensor(live, device=dev)
                classes.append((rows.int().contiguous(), t_idx, table.index_select(0, t_idx).index_select(1, rows).contiguous()))
            start += n
    return table, cls, classes


class SparseConvV1Fn(torch.autograd.Function):
    """y = relu(scale * sparse_conv(x; W, table) + shift + res): SubMConv3d / SparseConv3d of spconv v1 on rows, differentiable in
    x, W and res.  ``weight``: [kd, kh, kw, Cin, Cout] (upstream's state_dict layout; dW comes back in it); x: [n_in, pad4(Cin)];
    ``bwd``: the transposed book [taps, n_in], or the class list of ``dgrad_books``; ``x_h2``: the split-f16 twin of x when its
    producer wrote one; scale / shift: constants (an eval-mode BN folded into the epilogue) or None."""

    @staticmethod
    def forward(ctx, x, weight, table, bwd, x_h2, scale, shift, res, relu):
        from . import autograd as ag
        taps, Mo = table.shape
        Cin, Cout = weight.shape[3], weight.shape[4]
        n_in, Cp = x.shape
        assert weight.shape[0] * weight.shape[1] * weight.shape[2] == taps and Cp == lidar._pad4(Cin) and Cout % 4 == 0
        w3 = weight.detach().float().reshape(taps, Cin, Cout).permute(2, 1, 0)                 # [Cout, Cin, taps]
        if Cp != Cin:
            w3 = torch.cat([w3, w3.new_zeros(Cout, Cp - Cin, taps)], 1)
        w3 = w3.contiguous()
        out = torch.empty(Mo, Cout, device=x.device, dtype=_F32)
        h2 = _train_h2()
        if Mo:
            epi = dict(scale=scale, shift=shift, res2d=res, relu=relu, tag="sparse_hd_fwd")
            if h2 and Cp % 32 == 0:
                xh = x_h2 if x_h2 is not None else ag._rows_h2(x, Cp)
                ag._table_launch(xh, Cp, ag.pack_weights_h2_dev(w3, Cout, Cp, taps, 0), out, Cout, table, h2_alpha=1.0, **epi)
            else:
                ag._table_launch(x, Cp, ag.pack_weights_dev(w3, Cout, Cp, taps, 0), out, Cout, table, **epi)
        ctx.save_for_backward(x, w3, table, out if relu else None, scale, *([bwd] if torch.is_tensor(bwd) else [t for c in bwd for t in c]))
        ctx.cfg = (Cin, tuple(weight.shape), torch.is_tensor(bwd), h2, bool(relu), res is not None)
        return out

    @staticmethod
    def backward(ctx, dout):
        from . import autograd as ag
        x, w3, table, out, scale = ctx.saved_tensors[:5]
        books = ctx.saved_tensors[5:]
        Cin, wshape, full, h2, relu, has_res = ctx.cfg
        Cout, Cp, taps = w3.shape
        Mo, n_in = table.shape[1], x.shape[0]
        dev = x.device
        dout = dout.float().contiguous()
        need_x, need_w, need_res = ctx.needs_input_grad[0], ctx.needs_input_grad[1], has_res and ctx.needs_input_grad[7]
        h2d = h2 and need_x and Cout % 32 == 0 and Mo > 0
        h2w = HD_WGRAD_H2 and h2 and need_w and Cp % 32 == 0 and Cout % 32 == 0 and Mo > 0
        h2g = h2d or h2w                                            # a split-f16 GEMM reads dacc: it needs the gradient scale
        dacc, gscale, dres = dout, None, None
        if Mo and (h2g or relu or scale is not None or need_res):
            # the epilogue's backward (ReLU mask, folded scale, residual) and, for the split-f16 dgrad / wgrad, max |dacc| -> {2^k, 2^-k}
            dacc, dres, _, gscale = ag.epilogue_bwd(dout, out, scale, relu, want_res=need_res, want_gscale=h2g)
        elif need_res:
            dres = dout
        dx = dw = None
        if need_x:
            dx = torch.zeros(n_in, Cp, device=dev, dtype=_F32)       # rows no output reads, classes without taps: zero gradient
            if Mo and n_in:
                src = ag._rows_h2(dacc, Cout, gscale) if h2d else dacc
                kw = dict(h2_alpha=1.0, alpha_dev=ptr(gscale, offset=1)) if h2d else {}
                pack = ag.pack_weights_h2_dev if h2d else ag.pack_weights_dev
                if full:
                    ag._table_launch(src, Cout, pack(w3, Cout, Cp, taps, 3), dx, Cp, books[0], tag="sparse_hd_dgrad", **kw)
                else:
                    for j in range(0, len(books), 3):
                        rows_c, taps_c, table_c = books[j:j + 3]
                        wsub = w3.index_select(2, taps_c).contiguous()
                        ag._table_launch(src, Cout, pack(wsub, Cout, Cp, taps_c.numel(), 3), dx, Cp, table_c, tag="sparse_hd_dgrad",
                                         out_rows=rows_c, **kw)
        if need_w:
            dw3 = torch.zeros(Cout, Cp, taps, device=dev, dtype=_F32)
            if Mo:
                ws = core.workspace(dev)
                if h2w:
                    with _lib.TIMER.region("k_wgrad_h2t<sparse hd table>", 2.0 * Mo * Cp * Cout * taps):
                        call("coocc_conv_wgrad_h2t", ptr(x), n_in, Cp, ptr(dacc), Cout, ptr(table), Mo, Cp, Cout, taps, ptr(gscale),
                             ptr(dw3), 0, ptr(ws), ws.numel())
                else:
                    with _lib.TIMER.region("k_wgrad<sparse hd table>", 2.0 * Mo * Cp * Cout * taps):
                        call("coocc_conv_wgrad", ptr(x), n_in, Cp, ptr(dacc), Cout, ptr(table), Mo, Cp, Cout, taps, ptr(dw3), 0, ptr(ws),
                             ws.numel())
            dw = dw3[:, :Cin, :].permute(2, 1, 0).reshape(wshape).contiguous()
        return dx, dw, None, None, None, None, None, dres, None


def conv_bn_train(f, fh, conv, bn, table, bwd, res=None, twin=True):
    """SparseConvV1 -> BN1d (+ res) -> ReLU on rows, differentiable: (rows, their split-f16 twin or None).  ``f`` [n_in, pad4(Cin)]
    with its twin ``fh`` (or None), ``table`` / ``bwd`` the forward and transposed books (``SparseConvV1Fn``).  The norm follows its
    own ``training`` flag: batch statistics (``autograd.norm_rows``, whose apply pass writes the twin when the split-f16
    engine will read it), or its folded running statistics in the GEMM's epilogue."""
    from . import autograd as ag
    if not bn.training:
        return SparseConvV1Fn.apply(f, conv.weight, table, bwd, fh, *core.folded_bn(bn, f.device), res, True), None
    y = SparseConvV1Fn.apply(f, conv.weight, table, bwd, fh, None, None, None, False)
    if y.shape[0] == 0:                     # no active row: nothing to normalise, no statistic to update; zero gradients
        return y + (bn.weight.sum() + bn.bias.sum()) * 0, None
    yh = torch.empty_like(y) if (twin and _train_h2() and y.shape[1] % 32 == 0) else None
    return ag.norm_rows(y, bn, res=res, out_h2=yh), yh


@MIDDLE_ENCODERS_HD.register_module()
class SparseEncoderHD(nn.Module):
    def __init__(self, in_channels, sparse_shape, order=('conv', 'norm', 'act'), norm_cfg=dict(type='BN1d', eps=1e-3, momentum=0.01),
                 base_channels=16, output_channels=128, encoder_channels=((16, ), (32, 32, 32), (64, 64, 64), (64, 64, 64)),
                 encoder_paddings=((1, ), (1, 1, 1), (1, 1, 1), ((0, 1, 1), 1, 1)), encoder_strides=(2, 2, 2, 1),
                 block_type='conv_module', keep_depth=True, fp16_enabled=False):
        super().__init__()
        assert block_type in ['conv_module', 'basicblock']
        if tuple(order) != ('conv', 'norm', 'act'):
            raise NotImplementedError("SparseEncoderHD: order %r is not built; only ('conv', 'norm', 'act') (the pre-activation orders "
                                      "cannot fold the norm into the convolution's epilogue)" % (tuple(order),))
        if not keep_depth:
            raise NotImplementedError("SparseEncoderHD: keep_depth=False (the dense volume summed over z) is not built; SECOND3D takes "
                                      "[B,C,Z,Y,X]")
        if fp16_enabled:
            raise NotImplementedError("SparseEncoderHD: fp16_enabled=True (auto_fp16 on the voxel features) is not built; the engine's "
                                      "precision is chosen by COOCC_CONV_ENGINE")
        self.sparse_shape = [int(v) for v in sparse_shape]
        if len(self.sparse_shape) != 3:
            raise ValueError("SparseEncoderHD: sparse_shape %r is not (D, H, W)" % (sparse_shape,))
        self.in_channels, self.order = in_channels, tuple(order)
        self.base_channels, self.output_channels = base_channels, output_channels
        self.encoder_channels, self.encoder_paddings, self.encoder_strides = encoder_channels, encoder_paddings, encoder_strides
        self.stage_num = len(encoder_channels)
        self.keep_depth, self.block_type = keep_depth, block_type
        self.conv_input = _ConvModule(in_channels, base_channels, 3, norm_cfg, subm=True)
        # sparse_encoder_hd.py:136-210
        self.encoder_layers = nn.Sequential()
        cin = base_channels
        for i, blocks in enumerate(encoder_channels):
            mods = []
            for j, cout in enumerate(tuple(blocks)):
                padding = tuple(encoder_paddings[i])[j]
                if i != 0 and j == 0 and block_type == 'conv_module':
                    mods.append(_ConvModule(cin, cout, 3, norm_cfg, stride=encoder_strides[i], padding=padding))
                elif block_type == 'basicblock':
                    if j == len(blocks) - 1 and i != len(encoder_channels) - 1:
                        mods.append(_ConvModule(cin, cout, 3, norm_cfg, stride=encoder_strides[i], padding=padding))
                    else:
                        if cout != cin:
                            raise ValueError("SparseEncoderHD: SparseBasicBlock(%d, %d) after %d channels: the identity add needs equal "
                                             "widths (encoder_channels stage %d)" % (cout, cout, cin, i + 1))
                        mods.append(SparseBasicBlockHD(cout, norm_cfg))
                else:
                    mods.append(_ConvModule(cin, cout, 3, norm_cfg, padding=padding, subm=True))
                cin = cout
            self.encoder_layers.add_module("encoder_layer%d" % (i + 1), nn.Sequential(*mods))
        self.conv_out = _ConvModule(cin, output_channels, (1, 1, 1), norm_cfg, stride=(1, 1, 1), padding=0)
        self._packs = PackCache(self)
        self.wide16 = WIDE16
        # opt-in (the detectors' ``train_sparse_encoder_hd`` option sets it): under ``train()`` the forward runs the differentiable
        # path (``forward_train_rows``); False keeps the refusal below
        self.train_enabled = False
        self.last_active = 0                        # active outputs of the last forward
        self.last_cleared_bytes = 0                 # bytes it cleared: index maps, flag volumes, the dense volume

    def out_shape(self):
        """(D, H, W) of the dense output."""
        shape = tuple(self.sparse_shape)
        for st in self.encoder_layers:
            for m in st:
                if isinstance(m, _ConvModule) and not m[0].subm:
                    shape = conv_out_size(shape, m[0].kernel, m[0].stride, m[0].padding)
        return shape

    def _packed(self):
        def build():
            wide = lidar.LIDAR_H2 and core.CONV_ENGINE == "h2" and self.wide16

            def width(c):
                return 32 if (wide and c < 32) else lidar._pad4(c)
            d = dict(inp=self.conv_input[0].packed(self.conv_input[1], lidar._pad4(self.in_channels), width(self.base_channels)),
                     stages=[], wide=wide)
            for st in self.encoder_layers:
                ps = []
                for m in st:
                    if isinstance(m, SparseBasicBlockHD):
                        w = width(m.conv1.cin)
                        ps.append(("block", m.conv1.packed(m.bn1, w, w), m.conv2.packed(m.bn2, w, w)))
                    else:
                        ps.append(("subm" if m[0].subm else "down", m[0].packed(m[1], width(m[0].cin), width(m[0].cout)), m[0]))
                d["stages"].append(ps)
            co = self.conv_out[0]
            d["out"] = co.packed(self.conv_out[1], width(co.cin), co.cout)
            return d
        engine = (core.CONV_ENGINE, lidar.LIDAR_H2, self.wide16)
        if getattr(self, "_pack_engine", engine) != engine:
            self._packs.invalidate()                # the carried widths depend on the engine
        self._pack_engine = engine
        return self._packs.get_modules((self,), build)

    def forward(self, voxel_features, coors, batch_size):
        """voxel_features [M, in_channels], coors [M,4] (b,z,y,x) or [M,3] (z,y,x) -> the dense [1, C, Z, Y, X] volume
        (``out.dense()``, sparse_encoder_hd.py:128-134): a zero-copy view of channels-last rows that remembers them
        (``lidar_trunk.rows_of_bczyx``), so ``lidar_trunk.run_trunk`` reads it without a transposition."""
        if self.training and not self.train_enabled:
            raise NotImplementedError("SparseEncoderHD: the train() forward (batch-statistics BN1d, gradients through the per-axis rule "
                                      "books) is not built; call .eval()")
        if int(batch_size) != 1:
            raise NotImplementedError("SparseEncoderHD: batch size %d is not built; batch size 1 (one sample per call)" % int(batch_size))
        M, Cin = voxel_features.shape
        if Cin != self.in_channels:
            raise ValueError("SparseEncoderHD: voxel features have %d channels but in_channels = %d (the shipped coocc_lidar.py pairs "
                             "HardSimpleVFE(num_features=5) with in_channels=4: change one of the two)" % (Cin, self.in_channels))
        if not voxel_features.is_cuda:
            raise _lib.CooccError("the sparse LiDAR encoder runs on the GPU only (no CPU fallback)")
        if coors.shape[1] == 4:
            coors = coors[:, 1:]
        coors = coors.int().contiguous()
        if self.training:
            return self.forward_train_rows(voxel_features, self.rule_books(coors, transposed=True))
        levels = self.rule_books(coors)
        f = self.run_layers(voxel_features, levels)
        return self.dense_output(f, levels)

    def rule_books(self, coors, transposed=False):
        """coors [M,3] (z,y,x) int32 -> the levels of the encoder, one per resolution in order, each with its SubM / 1x1x1 books and
        (``.down``) the rule book of the SparseConv3d that made it; ``transposed``: also (``.down_bwd``) that convolution's transposed
        book for the training path (``dgrad_books``).  Coordinates outside ``sparse_shape`` raise ``ValueError`` (a cloud voxelised
        with another range, a mis-sized ``sparse_shape``): the index map is addressed by them."""
        if coors.shape[0]:
            lo, hi = torch.stack([coors.amin(0), coors.amax(0)]).tolist()          # one host read
            if min(lo) < 0 or any(h >= n for h, n in zip(hi, self.sparse_shape)):
                raise ValueError("SparseEncoderHD: voxel coordinates span (z,y,x) %r..%r, outside sparse_shape %r" % (lo, hi, self.sparse_shape))
        cur = SparseLevel(coors, self.sparse_shape)
        cur.down = None
        cur.table()
        levels = [cur]
        for st in self.encoder_layers:
            for m in st:
                if isinstance(m, SparseBasicBlockHD) or m[0].subm:
                    cur.table((3, 3, 3) if isinstance(m, SparseBasicBlockHD) else m[0].kernel)
                else:
                    prev = cur
                    cur, tb = prev.downsample(m[0].kernel, m[0].stride, m[0].padding)
                    cur.down = tb
                    if transposed:
                        _, _, classes = bwd = dgrad_books(prev, cur, m[0].kernel, m[0].stride, m[0].padding)
                        cur.down_bwd = classes if classes is not None else bwd[0]
                    levels.append(cur)
        cur.table((1, 1, 1))
        cur.dense_rows()
        return levels

    def run_layers(self, voxel_features, levels):
        """Every layer up to ``conv_out``: one ``lidar.sparse_conv`` launch each -> rows [M_last, C] of the last level."""
        p = self._packed()
        M, Cin = voxel_features.shape
        cin_p = lidar._pad4(Cin)
        x = voxel_features.float().contiguous()
        if cin_p != Cin:
            x = torch.cat([x, x.new_zeros(M, cin_p - Cin)], 1).contiguous()
        def sc(*args, twin, **kw):                  # always (rows, H2 twin or None)
            r = lidar.sparse_conv(*args, twin=twin, **kw)
            return r if twin else (r, None)
        ops = [item for ps in p["stages"] for item in ps]
        it = iter(levels)
        cur = next(it)
        # ``twin``: the epilogue also writes the H2 operand of the NEXT rule-book GEMM; conv_out scatters through out_rows on the
        # fp32-MFMA kernel and reads fp32 rows, so the last layer writes none
        f, fh = sc(x, cin_p, p["inp"], cur.table(), relu=True, twin=bool(ops))
        for n, item in enumerate(ops):
            twin = n + 1 < len(ops)
            if item[0] == "block":
                tb = cur.table()
                h, hh = sc(f, f.shape[1], item[1], tb, relu=True, feats_h2=fh, twin=True)
                f, fh = sc(h, h.shape[1], item[2], tb, relu=True, res=f, feats_h2=hh, twin=twin)
            elif item[0] == "subm":
                f, fh = sc(f, f.shape[1], item[1], cur.table(item[2].kernel), relu=True, feats_h2=fh, twin=twin)
            else:
                cur = next(it)
                f, fh = sc(f, f.shape[1], item[1], cur.down, relu=True, feats_h2=fh, twin=twin)
        return f

    def dense_output(self, f, levels):
        """conv_out, the 1x1x1 SparseConv3d (conv.py:134-145: a GEMM on the rows of the same active set), writes each row at its
        place in the zeroed dense volume (the GEMM's out_rows scatter): no [M, C] intermediate, no indexed copy."""
        from . import lidar_trunk as lt
        cur = levels[-1]
        D, H, W = cur.shape
        C = self.output_channels
        dense = torch.zeros(W * H * D, C, device=f.device, dtype=_F32)
        lidar.sparse_conv(f, f.shape[1], self._packed()["out"], cur.table((1, 1, 1)), relu=True, out=dense, out_rows=cur.dense_rows())
        # (the split-f16 range guard is sticky: read at the detector's next host read, core.check_h2_overflow)
        self.last_active = cur.M
        self.last_cleared_bytes = sum(lv.cleared_bytes for lv in levels) + dense.numel() * 4
        return lt.rows_as_bczyx(Rows(dense, 1, W, H, D, C))

    def forward_train_rows(self, voxel_features, levels):
        """The differentiable forward (``train()`` with ``train_enabled``) over the levels of ``rule_books(transposed=True)`` ->
        the same [1, C, Z, Y, X] view of channels-last rows as inference, with a ``grad_fn``.  Every BN1d follows its own
        ``training`` flag: batch statistics over the active rows (all ranks' rows for a SyncBatchNorm a user's
        ``convert_sync_batchnorm`` made) and running-statistics updates, or its folded running statistics in the GEMM's epilogue."""
        from . import autograd as ag
        from . import lidar_trunk as lt
        M, Cin = voxel_features.shape
        cin_p = lidar._pad4(Cin)
        x = voxel_features.float()
        if cin_p != Cin:
            x = torch.cat([x, x.new_zeros(M, cin_p - Cin)], 1)
        x = x.contiguous()

        def subm_books(level, kernel):
            tb = level.table(kernel)
            key = ("bwd",) + tuple(kernel)
            if key not in level.books:
                level.books[key] = tb.flip(0).contiguous()            # the voxel at -offset: tap taps - 1 - t of the same book
            return tb, level.books[key]

        it = iter(levels)
        cur = next(it)
        f, fh = conv_bn_train(x, None, self.conv_input[0], self.conv_input[1], *subm_books(cur, self.conv_input[0].kernel))
        for st in self.encoder_layers:
            for m in st:
                if isinstance(m, SparseBasicBlockHD):
                    tb, tbb = subm_books(cur, (3, 3, 3))
                    h, hh = conv_bn_train(f, fh, m.conv1, m.bn1, tb, tbb)
                    f, fh = conv_bn_train(h, hh, m.conv2, m.bn2, tb, tbb, res=f)
                elif m[0].subm:
                    f, fh = conv_bn_train(f, fh, m[0], m[1], *subm_books(cur, m[0].kernel))
                else:
                    cur = next(it)
                    f, fh = conv_bn_train(f, fh, m[0], m[1], cur.down, cur.down_bwd)
        tb = cur.table((1, 1, 1))
        f, _ = conv_bn_train(f, fh, self.conv_out[0], self.conv_out[1], tb, tb, twin=False)       # 1x1x1: one tap, its own transpose
        D, H, W = cur.shape
        if cur.M:
            dense = ag.ScatterRowsFn.apply(f, cur.dense_rows(), W * H * D)
        else:
            dense = torch.zeros(W * H * D, self.output_channels, device=f.device, dtype=_F32) + f.sum() * 0
        self.last_active = cur.M
        self.last_cleared_bytes = sum(lv.cleared_bytes for lv in levels) + dense.numel() * 4
        return lt.rows_as_bczyx(Rows(dense, 1, W, H, D, self.output_channels))
