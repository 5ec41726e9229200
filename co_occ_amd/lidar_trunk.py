"""``SECOND3D`` / ``SECOND3DFPN`` -- the dense LiDAR trunk of ``COOCC_Ray_L`` (projects/configs/coocc_nusc/coocc_lidar.py),
mirrors of P/coocc/backbones/second3d.py and P/coocc/necks/second3d_fpn.py: same ctor kwargs, ``forward`` signatures and
state_dict keys (``blocks.{i}.{3j}.weight`` / ``blocks.{i}.{3j+1}.*``, ``deblocks.{i}.{0,1}.*``, ``extra_blocks.{3j}.weight`` /
``extra_blocks.{3j+1}.*``).

Tensors at the module boundary are the reference's [B,C,Z,Y,X]; inside everything is ``core.Rows`` in (b, x, y, z) order, so
the reference's kernel (1,3,3) is this package's 3x3x1 (Winograd F(m x m,3x3) over (x, y) with ONE z tap on the large
grids, the direct split-f16 kernels below the row threshold and for the (s,s,1)-strided first convs).  The neck's
ConvTranspose3d(kernel = stride = (1,s,s)) layers have no overlap: each is a pointwise GEMM Cin -> s*s*Cout on the coarse
rows, and ``coocc_fpn_sum`` (csrc/second_fpn.hip) gathers the children and adds the levels in the reference's order.
The modules' own ``forward`` is eval mode only (folded BN); ``run_trunk_train`` is the differentiable trunk (batch-statistics BN,
dgrad / wgrad of every layer: ``autograd``).  There is no CPU or eager-PyTorch fallback.
"""
import ctypes

import torch
from torch import nn

from . import _lib, core
from .backbone import build_bn
from .core import PackCache, PackedConv, Rows, conv_rows
from ._lib import call, ptr
from .registry import BACKBONES, NECKS

_F32 = torch.float32


class _Cfg(dict):
    """Config dicts with the attribute access the reference uses on them (``conv_cfg.type``, second3d.py:46)."""
    __getattr__ = dict.get


def rows_as_bczyx(r):
    """Reference-layout view [B,C,Z,Y,X] of Rows (no copy).  Like ``Rows.as_ncdhw`` the view remembers its Rows, so the next
    module of the trunk -- and ``COOCC_Ray_L.extract_pts_feat`` -- find them again without a conversion."""
    v = r.t.view(r.B, r.X, r.Y, r.Z, r.stride)
    if r.coff or r.stride != r.C:
        v = v[..., r.coff:r.coff + r.C]
    v = v.permute(0, 4, 3, 2, 1)
    if not r.persistent:
        v._coocc_rows_zyx = (r, v._version)
    return v


def rows_of_bczyx(x):
    """The Rows behind a [B,C,Z,Y,X] view this module produced and nobody wrote since, or None."""
    back = getattr(x, "_coocc_rows_zyx", None)
    if back is not None:
        r, ver = back
        if ver == x._version and x.dim() == 5 and tuple(x.shape) == (r.B, r.C, r.Z, r.Y, r.X):
            return r
    return None


def bczyx_to_rows(x):
    """[B,C,Z,Y,X] tensor (or Rows, or a view that remembers them) -> Rows in (b, x, y, z) order: at most one conversion
    launch (``coocc_zyx_to_rows``), none for Rows / remembered views / channels-last memory."""
    if isinstance(x, Rows):
        return x
    r = rows_of_bczyx(x)
    if r is not None:
        return r
    if not torch.is_tensor(x) or x.dim() != 5:
        raise ValueError("expected a [B,C,Z,Y,X] tensor")
    if not x.is_cuda:
        raise _lib.CooccError("co_occ_amd modules run on the GPU only (no CPU fallback)")
    B, C, Z, Y, X = x.shape
    x = x.float()
    cl = x.permute(0, 4, 3, 2, 1)
    if cl.is_contiguous():
        return Rows(cl.reshape(B * X * Y * Z, C), B, X, Y, Z, C)
    x = x.contiguous()
    out = torch.empty(B * X * Y * Z, C, device=x.device, dtype=_F32)
    with core.TIMER.region("k_zyx_to_rows", 8.0 * out.numel()):
        call("coocc_zyx_to_rows", ptr(x), ptr(out), B, C, Z, Y, X, C, 0)
    return Rows(out, B, X, Y, Z, C)


def _eval_only(module):
    if module.training:
        raise NotImplementedError("%s: the train() forward (batch statistics, dgrad / wgrad of the anisotropic and transposed "
                                  "convolutions) is not built; call .eval()" % type(module).__name__)


def _kernel_zyx(kernel, what):
    kernel = tuple(int(k) for k in kernel)
    if len(kernel) != 3:
        raise NotImplementedError("%s: kernel %r -- only 3-D kernels (the 'Conv3d' kernel type) run on the HIP engine" % (what, kernel))
    if any(k not in (1, 3) for k in kernel):
        raise NotImplementedError("%s: kernel %r -- extents 1 and 3 only" % (what, kernel))
    return kernel


def _conv_type(cfg, what):
    t = cfg.get("type", "Conv3d")
    if t != "Conv3d":
        raise NotImplementedError("%s: conv type %r (the 'Conv2d' kernel type folds z into the batch) is not built; only "
                                  "'Conv3d'" % (what, t))


def fpn_sum(ups, strides, Cout, twin_for=()):
    """``sum(ups)`` of second3d_fpn.py:119-122 on deblock outputs: ``ups[l]`` = Rows [B*(X/s)*(Y/s)*Z, s*s*Cout] of the pointwise
    deconvolution GEMM of level l (child (kx, ky) of a coarse voxel at columns (kx*s + ky)*Cout ..).  Returns Rows
    [B*X*Y*Z, Cout]; bit-equal to the fp32 sum in the reference's order."""
    u0, s0 = ups[0], strides[0]
    B, X, Y, Z = u0.B, u0.X * s0, u0.Y * s0, u0.Z
    for u, s in zip(ups, strides):
        if (u.B, u.X * s, u.Y * s, u.Z) != (B, X, Y, Z) or u.C != s * s * Cout or u.coff or u.stride != u.C:
            raise ValueError("SECOND3DFPN: level sizes differ after upsampling (%s x stride %d vs %s)"
                             % ((u.X, u.Y, u.Z), s, (X, Y, Z)))
    dev = u0.t.device
    out = Rows(torch.empty(B * X * Y * Z, Cout, device=dev, dtype=_F32), B, X, Y, Z, Cout)
    tw = None
    if core.wants_h2_twin(out, twin_for):
        tw = out.h2 = torch.empty(B * X * Y * Z, Cout, device=dev, dtype=_F32)
    pp = (ctypes.c_void_p * 4)(*[u.t.data_ptr() for u in ups])
    ss = (ctypes.c_int * 4)(*strides)
    with core.TIMER.region("k_fpn_sum", 4.0 * out.t.numel() * (len(ups) + 1 + (1 if tw is not None else 0))):
        call("coocc_fpn_sum", pp, ss, len(ups), B, X, Y, Z, Cout, out.data(), Cout, ptr(tw))
    return out


@BACKBONES.register_module()
class SECOND3D(nn.Module):
    def __init__(self, in_channels=128, out_channels=[128, 128, 256], layer_nums=[3, 5, 5], layer_strides=[2, 2, 2],
                 is_cascade=True, norm_cfg=dict(type='BN3d', eps=1e-3, momentum=0.01), conv_cfg=dict(type='Conv3d', bias=False),
                 init_cfg=None, pretrained=None):
        super().__init__()
        assert len(layer_strides) == len(layer_nums)
        assert len(out_channels) == len(layer_nums)
        assert not (init_cfg and pretrained), 'init_cfg and pretrained cannot be setting at the same time'
        in_filters = list(in_channels) if isinstance(in_channels, (list, tuple)) else [in_channels, *out_channels[:-1]]
        conv_cfg = _Cfg(conv_cfg)                     # a copy: the reference pops "kernel" from the caller's dict
        self.is_cascade = is_cascade
        self.kernel_type = conv_cfg.get("type", "Conv3d")
        _conv_type(conv_cfg, "SECOND3D")
        kernel = _kernel_zyx(conv_cfg.pop("kernel", (1, 3, 3)), "SECOND3D")
        bias = bool(conv_cfg.get("bias", True))                # build_conv_layer passes conv_cfg on: nn.Conv3d's default (second3d.py:54-60)
        padding = tuple((k - 1) // 2 for k in kernel)
        self.kernel, self.layer_strides = kernel, [int(s) for s in layer_strides]
        blocks = []
        for i, n in enumerate(layer_nums):                                      # second3d.py:52-77
            s = self.layer_strides[i]
            block = [nn.Conv3d(in_filters[i], out_channels[i], kernel, stride=(1, s, s), padding=padding, bias=bias),
                     build_bn(norm_cfg, out_channels[i]), nn.ReLU(inplace=True)]
            for _ in range(n):
                block += [nn.Conv3d(out_channels[i], out_channels[i], kernel, padding=padding, bias=bias),
                          build_bn(norm_cfg, out_channels[i]), nn.ReLU(inplace=True)]
            blocks.append(nn.Sequential(*block))
        self.blocks = nn.ModuleList(blocks)
        self.init_cfg = dict(type='Pretrained', checkpoint=pretrained) if isinstance(pretrained, str) else \
            dict(type='Kaiming', layer=self.kernel_type)
        self._packs = PackCache(self)

    def init_weights(self):
        """``init_cfg`` = Kaiming on the conv layers (second3d.py:88; mmcv's kaiming_init: normal, fan_out, relu), applied when
        the caller asks for it as BaseModule does -- the constructor leaves torch's default initialisation and the RNG alone."""
        if self.init_cfg.get("type") == "Pretrained":
            raise NotImplementedError("SECOND3D.init_weights: loading init_cfg checkpoint %r is the caller's (load_state_dict)"
                                      % self.init_cfg.get("checkpoint"))
        for m in self.modules():
            if isinstance(m, nn.Conv3d):
                nn.init.kaiming_normal_(m.weight, mode='fan_out', nonlinearity='relu')
                if m.bias is not None:
                    nn.init.constant_(m.bias, 0)

    def _packed(self):
        kz, ky, kx = self.kernel

        def build():
            out = []
            for i, blk in enumerate(self.blocks):
                s, packs = self.layer_strides[i], []
                for j in range(0, len(blk), 3):
                    st = (s, s, 1) if j == 0 else (1, 1, 1)
                    packs.append(PackedConv(core.zyx_weight(blk[j].weight), bn=blk[j + 1], bias=blk[j].bias, kernel=(kx, ky, kz),
                                            strides=st))
                out.append(packs)
            return out
        return self._packs.get_modules((self,), build)

    def forward_rows(self, x, readers=None):
        """Rows in, one Rows per block out.  ``readers``: per block, the layers outside this module that read its output next
        (the neck's deblocks): a split-f16 layer among them gets its H2 operand from the last conv's epilogue."""
        _eval_only(self)
        p = self._packed()
        outs = []
        for i, packs in enumerate(p):
            h = x
            for j, pc in enumerate(packs):
                if j + 1 < len(packs):
                    nxt = (packs[j + 1],)
                else:
                    nxt = tuple(readers[i]) if readers is not None else ()
                    if self.is_cascade and i + 1 < len(p):
                        nxt += (p[i + 1][0],)
                h = conv_rows(h, pc, relu=True, twin_for=nxt)
            outs.append(h)
            if self.is_cascade:
                x = h
        return outs

    def forward(self, x):
        """[B,C,Z,Y,X] -> tuple of [B,C_i,Z,Y_i,X_i] (second3d.py:91-114), zero-copy views of channels-last rows."""
        _eval_only(self)
        return tuple(rows_as_bczyx(r) for r in self.forward_rows(bczyx_to_rows(x)))


@NECKS.register_module()
class SECOND3DFPN(nn.Module):
    def __init__(self, in_channels=[128, 128, 256], out_channels=[256, 256, 256], upsample_strides=[1, 2, 4],
                 norm_cfg=dict(type='BN3d', eps=1e-3, momentum=0.01), upsample_cfg=dict(type='deconv3d', bias=False),
                 conv_cfg=dict(type='Conv3d', bias=False), extra_conv=None, use_conv_for_no_stride=False, use_for_distill=False,
                 init_cfg=None):
        super().__init__()
        assert len(out_channels) == len(upsample_strides) == len(in_channels)
        if use_for_distill:
            raise NotImplementedError("SECOND3DFPN: use_for_distill (the before-ReLU taps of cross-modality distillation) is not built")
        if upsample_cfg.get("type") != "deconv3d":
            raise NotImplementedError("SECOND3DFPN: upsample type %r is not built; only 'deconv3d'" % upsample_cfg.get("type"))
        _conv_type(conv_cfg, "SECOND3DFPN")
        if not 1 <= len(out_channels) <= 4:
            raise NotImplementedError("SECOND3DFPN: %d levels; the sum kernel takes 1-4" % len(out_channels))
        if len(set(out_channels)) != 1:
            raise ValueError("SECOND3DFPN: sum(ups) needs equal out_channels, got %r" % (out_channels,))
        self.in_channels, self.out_channels = list(in_channels), list(out_channels)
        self.extra_conv = dict(extra_conv) if extra_conv is not None else None
        self.fp16_enabled = False
        self.use_for_distill = False
        self.upsample_strides = []
        deblocks = []
        for i, oc in enumerate(out_channels):                                   # second3d_fpn.py:47-69
            s = upsample_strides[i]
            if s != int(s) or int(s) not in (1, 2, 4, 8):
                raise NotImplementedError("SECOND3DFPN: upsample stride %r; deconvs whose kernel = stride = (1,s,s), s in 1, 2, 4, 8 "
                                          "only (fractional strides are strided convs)" % (s,))
            s = int(s)
            self.upsample_strides.append(s)
            if s > 1 or not use_conv_for_no_stride:
                k = upsample_cfg.get("kernel_size", (1, s, s))
                if tuple(k) != (1, s, s):
                    raise NotImplementedError("SECOND3DFPN: a deconv whose kernel %r differs from its stride (1,%d,%d) overlaps; "
                                              "not built" % (tuple(k), s, s))
                up = nn.ConvTranspose3d(in_channels[i], oc, (1, s, s), stride=(1, s, s), bias=bool(upsample_cfg.get("bias", True)))
            else:
                up = nn.Conv3d(in_channels[i], oc, (1, 1, 1), stride=(1, 1, 1), bias=bool(conv_cfg.get("bias", True)))
            deblocks.append(nn.Sequential(up, build_bn(norm_cfg, oc), nn.ReLU(inplace=True)))
        self.deblocks = nn.ModuleList(deblocks)
        self.extra_kernel = None
        if self.extra_conv is not None:                                         # second3d_fpn.py:72-104
            ec = self.extra_conv
            _conv_type(ec, "SECOND3DFPN extra_conv")
            self.layer_num = ec.pop("num_conv")
            self.extra_kernel = _kernel_zyx(ec.pop("kernel", (3, 3, 3)), "SECOND3DFPN extra_conv")
            if "sep_kernel" in ec:
                raise NotImplementedError("SECOND3DFPN: extra_conv sep_kernel (two convs per norm) is not built")
            pad = tuple((k - 1) // 2 for k in self.extra_kernel)
            extra = []
            for _ in range(self.layer_num):
                extra += [nn.Conv3d(out_channels[-1], out_channels[-1], self.extra_kernel, padding=pad, bias=bool(ec.get("bias", True))),
                          build_bn(norm_cfg, out_channels[-1]), nn.ReLU(inplace=True)]
            self.extra_blocks = nn.Sequential(*extra)
        self.init_cfg = init_cfg
        if init_cfg is None:
            self.init_cfg = [dict(type='Kaiming', layer='ConvTranspose2d'), dict(type='Constant', layer='NaiveSyncBatchNorm2d', val=1.0)]
        self._packs = PackCache(self)

    def _packed(self):
        def build():
            de = []
            for s, blk in zip(self.upsample_strides, self.deblocks):
                up, bn = blk[0], blk[1]
                if isinstance(up, nn.ConvTranspose3d):
                    pc = PackedConv(core.deconv_weight(up.weight, s), ksize=1)
                    # one BN channel serves the s*s children of a coarse voxel
                    pc.scale, pc.bias = core.folded_bn(bn, up.weight.device, up.bias, repeat=s * s)
                else:
                    pc = PackedConv(up.weight, bn=bn, bias=up.bias, ksize=1)
                de.append(pc)
            ex = []
            if self.extra_conv is not None:
                kz, ky, kx = self.extra_kernel
                for j in range(0, len(self.extra_blocks), 3):
                    c, bn = self.extra_blocks[j], self.extra_blocks[j + 1]
                    if (kx, ky, kz) == (3, 3, 3):
                        ex.append(PackedConv(core.zyx_weight(c.weight), bn=bn, bias=c.bias, ksize=3, pad=1))
                    else:
                        ex.append(PackedConv(core.zyx_weight(c.weight), bn=bn, bias=c.bias, kernel=(kx, ky, kz)))
            return dict(de=de, ex=ex)
        return self._packs.get_modules((self,), build)

    def reader_packs(self):
        """Per input level, the layer that reads it (``SECOND3D.forward_rows(readers=...)``)."""
        return [(pc,) for pc in self._packed()["de"]]

    def forward_rows(self, xs):
        _eval_only(self)
        assert len(xs) == len(self.in_channels)
        p = self._packed()
        ups = [conv_rows(x, pc, relu=True) for x, pc in zip(xs, p["de"])]
        ex = p["ex"]
        if len(ups) == 1 and self.upsample_strides[0] == 1:
            out = ups[0]                                                        # second3d_fpn.py:123-124
        else:
            out = fpn_sum(ups, self.upsample_strides, self.out_channels[-1], twin_for=tuple(ex[:1]))
        for j, pc in enumerate(ex):
            out = conv_rows(out, pc, relu=True, twin_for=tuple(ex[j + 1:j + 2]))
        return out

    def forward(self, x):
        """list of [B,C_i,Z,Y_i,X_i] -> [B,C,Z,Y,X] (second3d_fpn.py:108-143), a zero-copy view of channels-last rows."""
        _eval_only(self)
        return rows_as_bczyx(self.forward_rows([bczyx_to_rows(t) for t in x]))


def run_trunk(backbone, neck, x):
    """``neck(backbone(x))`` on Rows end to end: x = [B,C,Z,Y,X] tensor or Rows -> Rows of the neck's output.  The backbone's last
    layers write the H2 operands of the neck's deblocks in their epilogues."""
    feats = backbone.forward_rows(bczyx_to_rows(x), readers=neck.reader_packs())
    return neck.forward_rows(feats)


def run_trunk_train(backbone, neck, x):
    """Differentiable ``neck(backbone(x))``: x = [B,C,Z,Y,X] tensor (or Rows) -> Rows of the neck's output whose ``t`` carries a
    ``grad_fn``.  Every layer is an autograd Function over the HIP kernels (``autograd.second3d_forward_train`` /
    ``second3dfpn_forward_train``); every BN follows its own ``training`` flag -- batch (or SyncBN all-reduced) statistics and
    running-statistics updates under ``train()``, folded running statistics in eval mode.  The modules are the inference modules:
    parameters and state_dict keys are shared, and ``run_trunk`` re-packs from the stepped parameters afterwards (``PackCache``)."""
    from . import autograd as ag
    if isinstance(x, Rows):
        x2d, geom = x.dense2d(), (x.B, x.X, x.Y, x.Z)
    else:
        if not torch.is_tensor(x) or x.dim() != 5:
            raise ValueError("expected a [B,C,Z,Y,X] tensor")
        if not x.is_cuda:
            raise _lib.CooccError("co_occ_amd modules run on the GPU only (no CPU fallback)")
        B, C, Z, Y, X = x.shape
        geom = (B, X, Y, Z)
        if x.requires_grad:
            x2d = ag.ZyxRowsFn.apply(x)
        else:
            x2d = bczyx_to_rows(x).dense2d()
    feats = ag.second3d_forward_train(backbone, x2d, geom)
    out, g = ag.second3dfpn_forward_train(neck, feats)
    return Rows(out, g[0], g[1], g[2], g[3], out.shape[1])
