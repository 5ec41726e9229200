"""``ResNet`` / ``SECONDFPN`` -- the 2-D image encoder of the ``coocc_nusc`` configs (``img_backbone`` / ``img_neck``) on the HIP
engine, opt-in (``COOCC_Ray(hip_image_encoder=True)``); training is a second opt-in (``train_enabled`` on both
modules, ``COOCC_Ray(train_image_encoder=True)``; the section "Training" below).  Mirrors of mmdet 2.14's ``ResNet``
(depth 50 / 101, Bottleneck, ``style='pytorch'``) and mmdet3d's ``SECONDFPN`` (mmdet3d/models/necks/second_fpn.py): same constructor
kwargs, ``forward`` signatures and state_dict keys (``conv1.weight``, ``bn1.*``, ``layer{i}.{j}.conv{1,2,3}.weight``,
``layer{i}.{j}.bn{1,2,3}.*``, ``layer{i}.0.downsample.{0.weight,1.*}``: 318 / 624 entries; ``deblocks.{i}.0.weight``,
``deblocks.{i}.1.*``), so a released ``img_backbone.*`` / ``img_neck.*`` checkpoint loads strictly.

Inside everything is channels-last rows [BN*H*W, C] (``core.Rows`` with X = H, Y = W, Z = 1, one camera after the other, as in
``depth_net``).  The stem -- 7x7 stride-2 convolution over the 3-channel NCHW image + BN + ReLU + 3x3 stride-2 max-pool -- is one
kernel (csrc/img_stem.hip) that reads the image directly and writes the pooled rows (+ their H2 twin).  Every other layer is one the
engine has: 1x1 convolutions through ``core.conv_rows`` (residual + ReLU in ``conv3``'s epilogue, H2 twins written by the
producers), stride-1 3x3 layers as 3x3x1 ``PackedConv``s (``core.route`` picks Winograd or the direct split-f16 kernel), the
stride-2 3x3 ``conv2`` and 1x1 ``downsample`` as (s,s,1)-strided anisotropic ``PackedConv``s, the neck's kernel = stride
convolutions as (k,k,1)/(k,k,1)/pad 0 ``PackedConv``s and its kernel = stride deconvolutions as the pointwise GEMM Cin -> s*s*Cout +
the child scatter of ``coocc_fpn_sum``.  Each deblock writes its slice of ONE [BN*H*W, sum(Cout)] buffer: there is no concat pass.

At the boundary the modules take and return the reference's [BN,C,H,W] tensors: zero-copy channels-last views that remember their
Rows, so ``SECONDFPN.forward`` converts nothing and ``DepthNet.forward`` finds channels-last memory.  The classes live in their own
registries (``IMAGE_BACKBONES`` / ``IMAGE_NECKS``), never in ``registry.BACKBONES`` / ``NECKS``: nothing builds them by default.
CPU tensors are refused; there is no eager-PyTorch fallback.

Training.  ``train_enabled`` is False by default and a ``train()`` forward then raises.  With it on (set it, then call ``train()``),
``ResNet.train(mode)`` follows mmdet 2.14 -- ``frozen_stages >= 0`` puts ``conv1`` / ``bn1`` and stages 1..frozen_stages in eval and
takes their parameters out of the gradient, ``norm_cfg['requires_grad']=False`` freezes the BN affine parameters, ``norm_eval=True``
puts every BN in eval -- and the ``train()`` forward is differentiable in every parameter that requires a gradient: the frozen prefix
runs the inference path above under ``no_grad`` (fused stem kernel, folded BN); every later Bottleneck layer is an
``autograd.conv_bn_rows`` layer (``ConvRowsFn`` + ``BatchNormRowsFn``, each BN in its own mode, residual + ReLU in ``bn3``), the
unfrozen stem is ``StemConvFn`` -> BN -> ``MaxPoolRowsFn`` (csrc/img_stem_train.hip), a deconvolution deblock is the pointwise GEMM on
a differentiable view of its weight + ``FpnSumFn``'s child scatter, and the levels meet in ``torch.cat``.  The modules still return
[BN,C,H,W] views of channels-last rows, now attached to the graph.  An eval-mode BN whose affine parameters require a gradient is
refused (the folded epilogue would give them none); the image gets no gradient; ``with_cp`` stays ignored.
"""
import ctypes

import torch
from torch import nn

from . import _lib, core
from ._lib import call, ptr
from .core import PackCache, PackedConv, Rows, conv_rows
from .depth_net import conv3x3_pack
from .registry import Registry

_F32 = torch.float32
IMAGE_BACKBONES = Registry("image backbone")
IMAGE_NECKS = Registry("image neck")
STEM_CHANNELS = 64              # csrc/img_stem.hip
ARCH = {50: (3, 4, 6, 3), 101: (3, 4, 23, 3)}
EXPANSION = 4


# ------------------------------------------------------------------ [BN,C,H,W] views of Rows
def rows_as_bchw(r):
    """Reference-layout view [BN,C,H,W] of Rows [BN, H, W, 1] (no copy).  The view remembers its Rows (and the tensor version they
    were valid at), so the next module of this file finds them -- H2 twin included -- without a conversion."""
    assert r.Z == 1
    v = r.t.view(r.B, r.X, r.Y, r.stride)
    if r.coff or r.stride != r.C:
        v = v[..., r.coff:r.coff + r.C]
    v = v.permute(0, 3, 1, 2)
    if not r.persistent:
        v._coocc_rows_hw = (r, v._version)
    return v


def rows_of_bchw(x):
    """The Rows behind a [BN,C,H,W] view this file produced and nobody wrote since, or None."""
    back = getattr(x, "_coocc_rows_hw", None)
    if back is not None:
        r, ver = back
        if ver == x._version and x.dim() == 4 and tuple(x.shape) == (r.B, r.C, r.X, r.Y):
            return r
    return None


def bchw_to_rows(x):
    """[BN,C,H,W] tensor (or Rows, or a view that remembers them) -> Rows [BN, H, W, 1]: at most one conversion launch, none for
    Rows / remembered views / channels-last memory."""
    if isinstance(x, Rows):
        return x
    r = rows_of_bchw(x)
    if r is not None:
        return r
    if not torch.is_tensor(x) or x.dim() != 4:
        raise ValueError("expected a [B*N,C,H,W] tensor")
    if not x.is_cuda:
        raise _lib.CooccError("co_occ_amd modules run on the GPU only (no CPU fallback)")
    return core.to_rows(x.unsqueeze(-1))


def _eval_only(module):
    if module.training and not getattr(module, "train_enabled", False):
        raise NotImplementedError("%s: training on the HIP engine is opt-in: set %s.train_enabled = True and call .train() again "
                                  "(COOCC_Ray(hip_image_encoder=True, train_image_encoder=True)), or call .eval()"
                                  % (type(module).__name__, type(module).__name__))


def _ag():
    from . import autograd
    return autograd


def _bns(module):
    return [m for m in module.modules() if isinstance(m, nn.modules.batchnorm._BatchNorm)]


def _check_trainable_norms(module):
    """An eval-mode BN is folded into its convolution's epilogue, which gives gamma / beta no gradient: refuse the combination
    instead of leaving a silent zero."""
    for m in _bns(module):
        if not m.training and any(p is not None and p.requires_grad for p in (m.weight, m.bias)):
            raise NotImplementedError("%s: a BatchNorm in eval mode whose weight / bias require a gradient (norm_eval=True with "
                                      "norm_cfg requires_grad=True) is not built: the folded epilogue gives them none; freeze them "
                                      "(requires_grad=False) or train the norm" % type(module).__name__)


def _freeze(module):
    module.eval()
    for p in module.parameters():
        p.requires_grad = False


def bchw_to_rows2d(x):
    """[BN,C,H,W] tensor (attached to a graph or not) -> (contiguous rows [BN*H*W, C], (BN, H, W, 1)); a view when the memory is
    channels-last (what this file's modules return), one differentiable copy otherwise."""
    if not torch.is_tensor(x) or x.dim() != 4:
        raise ValueError("expected a [B*N,C,H,W] tensor")
    if not x.is_cuda:
        raise _lib.CooccError("co_occ_amd modules run on the GPU only (no CPU fallback)")
    B, C, H, W = x.shape
    return x.float().permute(0, 2, 3, 1).reshape(B * H * W, C), (B, H, W, 1)


def rows2d_as_bchw(t, geom):
    return t.view(geom[0], geom[1], geom[2], t.shape[1]).permute(0, 3, 1, 2)


def _bn2d(norm_cfg, n, what):
    cfg = dict(norm_cfg or dict(type="BN"))
    t = cfg.pop("type", "BN")
    cfg.pop("requires_grad", None)
    if t not in ("BN", "BN2d", "SyncBN"):
        raise NotImplementedError("%s: norm_cfg type %r -- only BN-family norms are folded into the HIP convolutions" % (what, t))
    return nn.BatchNorm2d(n, **cfg)


def stem_pack(conv1, bn1):
    """(w [147, 64] with row (ci*7 + ky)*7 + kx, scale [64], bias [64]) of csrc/img_stem.hip on the weight's device."""
    w = conv1.weight.detach().float()
    return (w.permute(1, 2, 3, 0).reshape(-1, w.shape[0]).contiguous(),) + core.folded_bn(bn1, w.device, conv1.bias)


def stem_rows(img, pack, relu=True, pool=True, twin_for=()):
    """conv 7x7 / 2 / pad 3 + folded BN (+ ReLU) (+ max-pool 3x3 / 2 / pad 1) of img [BN,3,H,W] (fp32 NCHW) -> Rows [BN, Ho, Wo, 1]
    with 64 channels: one launch of k_img_stem.  ``twin_for``: the layers that read the rows next (``core.wants_h2_twin``)."""
    if not torch.is_tensor(img) or img.dim() != 4 or img.shape[1] != 3:
        raise ValueError("image encoder: expected a [B*N,3,H,W] image tensor")
    if not img.is_cuda:
        raise _lib.CooccError("co_occ_amd modules run on the GPU only (no CPU fallback)")
    w, scale, bias = pack
    img = img.float().contiguous()
    BN, _, H, W = img.shape
    Ho, Wo = (H - 1) // 2 + 1, (W - 1) // 2 + 1
    if pool:
        Ho, Wo = (Ho - 1) // 2 + 1, (Wo - 1) // 2 + 1
    C0 = w.shape[1]
    out = Rows(torch.empty(BN * Ho * Wo, C0, device=img.device, dtype=_F32), BN, Ho, Wo, 1, C0)
    tw = None
    if core.wants_h2_twin(out, twin_for):
        tw = out.h2 = torch.empty(BN * Ho * Wo, C0, device=img.device, dtype=_F32)
    Hc, Wc = (H - 1) // 2 + 1, (W - 1) // 2 + 1
    with core.TIMER.region("k_img_stem", 2.0 * BN * Hc * Wc * C0 * 147):
        call("coocc_img_stem", ptr(img), BN, H, W, ptr(w), ptr(scale), ptr(bias), C0, int(relu), int(pool), out.data(), C0, ptr(tw))
    return out


class Bottleneck(nn.Module):
    """mmdet 2.14's Bottleneck (``style='pytorch'``: the stride sits on the 3x3 ``conv2``); parameters only -- ``ResNet`` runs it."""
    expansion = EXPANSION

    def __init__(self, inplanes, planes, stride, downsample, norm_cfg):
        super().__init__()
        self.conv1 = nn.Conv2d(inplanes, planes, 1, bias=False)
        self.bn1 = _bn2d(norm_cfg, planes, "ResNet")
        self.conv2 = nn.Conv2d(planes, planes, 3, stride=stride, padding=1, bias=False)
        self.bn2 = _bn2d(norm_cfg, planes, "ResNet")
        self.conv3 = nn.Conv2d(planes, planes * EXPANSION, 1, bias=False)
        self.bn3 = _bn2d(norm_cfg, planes * EXPANSION, "ResNet")
        self.relu = nn.ReLU(inplace=True)
        self.downsample = downsample
        self.stride = stride


def _pw(weight, bn, stride=1):
    """A Conv2d 1x1 weight [N,C,1,1] (stride s) as the engine's layer on Rows [BN, H, W, 1]."""
    w = weight.detach()
    if stride == 1:
        return PackedConv(w.reshape(w.shape[0], w.shape[1]), bn=bn, ksize=1)
    return PackedConv(w.unsqueeze(-1), bn=bn, kernel=(1, 1, 1), strides=(stride, stride, 1), pads=(0, 0, 0))


def _c3(weight, bn, stride=1):
    if stride == 1:
        return conv3x3_pack(weight, bn=bn)
    return PackedConv(weight.detach().unsqueeze(-1), bn=bn, kernel=(3, 3, 1), strides=(stride, stride, 1), pads=(1, 1, 0))


# accepted and inert; ``frozen_stages``, ``norm_eval`` and ``norm_cfg['requires_grad']`` act under ``train_enabled`` only
_IGNORED = ("pretrained", "init_cfg", "with_cp", "zero_init_residual")


@IMAGE_BACKBONES.register_module()
class ResNet(nn.Module):
    def __init__(self, depth, in_channels=3, stem_channels=None, base_channels=64, num_stages=4, strides=(1, 2, 2, 2),
                 dilations=(1, 1, 1, 1), out_indices=(0, 1, 2, 3), style='pytorch', deep_stem=False, avg_down=False,
                 frozen_stages=-1, conv_cfg=None, norm_cfg=dict(type='BN', requires_grad=True), norm_eval=True, dcn=None,
                 stage_with_dcn=(False, False, False, False), plugins=None, with_cp=False, zero_init_residual=True,
                 pretrained=None, init_cfg=None, **kwargs):
        super().__init__()

        def no(name, value):
            raise NotImplementedError("ResNet on the HIP engine: %s=%r is not built (depth 50 / 101, style='pytorch', plain 7x7 stem, "
                                      "BN, no dilation / DCN / plugins)" % (name, value))
        for k in kwargs:
            no(k, kwargs[k])
        if depth not in ARCH:
            no("depth", depth)
        if in_channels != 3:
            no("in_channels", in_channels)
        if stem_channels not in (None, STEM_CHANNELS) or (stem_channels is None and base_channels != STEM_CHANNELS):
            no("stem_channels", stem_channels if stem_channels is not None else base_channels)
        if style != 'pytorch':
            no("style", style)
        if deep_stem:
            no("deep_stem", deep_stem)
        if avg_down:
            no("avg_down", avg_down)
        if conv_cfg is not None:
            no("conv_cfg", conv_cfg)
        if dcn is not None:
            no("dcn", dcn)
        if plugins is not None:
            no("plugins", plugins)
        if not 1 <= num_stages <= 4:
            no("num_stages", num_stages)
        strides, dilations = tuple(strides)[:num_stages], tuple(dilations)[:num_stages]
        if len(strides) != num_stages or any(s not in (1, 2) for s in strides):
            no("strides", strides)
        if len(dilations) != num_stages or any(d != 1 for d in dilations):
            no("dilations", dilations)
        if (norm_cfg or {}).get("type", "BN") not in ("BN", "BN2d", "SyncBN"):
            no("norm_cfg", norm_cfg)
        if base_channels % 4:
            no("base_channels", base_channels)
        out_indices = tuple(int(i) for i in out_indices)
        assert max(out_indices) < num_stages
        self.depth, self.num_stages, self.strides, self.out_indices = depth, num_stages, strides, out_indices
        self.stem_channels, self.base_channels = STEM_CHANNELS, base_channels
        self.conv1 = nn.Conv2d(3, STEM_CHANNELS, 7, stride=2, padding=3, bias=False)
        self.bn1 = _bn2d(norm_cfg, STEM_CHANNELS, "ResNet")
        self.relu = nn.ReLU(inplace=True)
        self.maxpool = nn.MaxPool2d(kernel_size=3, stride=2, padding=1)
        inplanes = STEM_CHANNELS
        self.res_layers = []
        for i, n in enumerate(ARCH[depth][:num_stages]):
            planes, blocks = base_channels * 2 ** i, []
            for j in range(n):
                s = strides[i] if j == 0 else 1
                down = None
                if j == 0 and (s != 1 or inplanes != planes * EXPANSION):
                    down = nn.Sequential(nn.Conv2d(inplanes, planes * EXPANSION, 1, stride=s, bias=False),
                                         _bn2d(norm_cfg, planes * EXPANSION, "ResNet"))
                blocks.append(Bottleneck(inplanes, planes, s, down, norm_cfg))
                inplanes = planes * EXPANSION
            name = "layer%d" % (i + 1)
            self.add_module(name, nn.Sequential(*blocks))
            self.res_layers.append(name)
        self.feat_dim = inplanes
        # the layers outside this module that read output level i next (a callable returning one tuple of PackedConv per entry of
        # ``out_indices``; the detector points it at the neck's ``reader_packs``): their H2 operands come from the last epilogue
        self.output_readers = None
        self._packs = PackCache(self)
        # training (opt-in).  With ``train_enabled`` on, ``train(mode)`` follows mmdet 2.14 (_freeze_stages + norm_eval) and the
        # train() forward is differentiable in every parameter that requires a gradient; set it, then call ``train()``
        self.train_enabled = False
        self.frozen_stages, self.norm_eval = int(frozen_stages), bool(norm_eval)
        self.norm_requires_grad = bool((norm_cfg or {}).get("requires_grad", True))
        self._prefix_packs = PackCache(self)

    def init_weights(self, pretrained=None):
        """Loading ``pretrained`` / ``init_cfg`` checkpoints is the caller's (``load_state_dict``); torch's default initialisation
        is left alone."""

    def _frozen_modules(self):
        """The frozen prefix of mmdet's ``_freeze_stages``: the stem for ``frozen_stages >= 0``, then stages 1..frozen_stages."""
        if self.frozen_stages < 0:
            return []
        return [self.conv1, self.bn1] + [getattr(self, name) for name in self.res_layers[:self.frozen_stages]]

    def train(self, mode=True):
        super().train(mode)
        if not getattr(self, "train_enabled", False):
            return self
        for m in self._frozen_modules():                      # resnet.py _freeze_stages
            _freeze(m)
        if not self.norm_requires_grad:                       # build_norm_layer(requires_grad=False)
            for m in _bns(self):
                for p in m.parameters():
                    p.requires_grad = False
        if mode and self.norm_eval:
            for m in _bns(self):
                m.eval()
        return self

    def _packed_prefix(self):
        """The inference packs of the frozen prefix alone (the trained layers are packed on the device every step)."""
        n = min(max(self.frozen_stages, 0), len(self.res_layers))

        def build():
            layers = [[self._block_packs(b) for b in getattr(self, name)] for name in self.res_layers[:n]]
            return dict(stem=stem_pack(self.conv1, self.bn1), layers=layers)
        return self._prefix_packs.get_modules(tuple(self._frozen_modules()), build)

    @staticmethod
    def _block_packs(b):
        ds = b.downsample
        return dict(c1=_pw(b.conv1.weight, b.bn1), c2=_c3(b.conv2.weight, b.bn2, b.stride), c3=_pw(b.conv3.weight, b.bn3),
                    ds=_pw(ds[0].weight, ds[1], b.stride) if ds is not None else None)

    @staticmethod
    def _run_block(h, b, nxt):
        t = conv_rows(h, b["c1"], relu=True, twin_for=(b["c2"],))
        t = conv_rows(t, b["c2"], relu=True, twin_for=(b["c3"],))
        idn = conv_rows(h, b["ds"], relu=False) if b["ds"] is not None else h
        return conv_rows(t, b["c3"], relu=True, res=idn, twin_for=nxt)

    def forward_train(self, img):
        """The train() forward: img [BN,3,H,W] -> per entry of ``out_indices`` (rows [BN*H_i*W_i, C_i], (BN, H_i, W_i, 1)), attached to
        the graph.  The frozen prefix (stem + stages 1..frozen_stages, all in eval mode without gradients) runs the inference path
        under no_grad -- fused stem kernel, folded BN --; every later layer is a ``conv_bn_rows`` layer with its BN in its own mode."""
        ag = _ag()
        if torch.is_tensor(img) and img.requires_grad:
            raise NotImplementedError("ResNet: a gradient with respect to the image is not built")
        if not torch.is_tensor(img) or img.dim() != 4 or img.shape[1] != 3:
            raise ValueError("image encoder: expected a [B*N,3,H,W] image tensor")
        if not img.is_cuda:
            raise _lib.CooccError("co_occ_amd modules run on the GPU only (no CPU fallback)")
        _check_trainable_norms(self)
        outs = {}
        nf = min(max(self.frozen_stages, 0), len(self.res_layers))
        if self.frozen_stages >= 0:
            with torch.no_grad():
                p = self._packed_prefix()
                r = stem_rows(img, p["stem"], relu=True, pool=True)
                for i, blocks in enumerate(p["layers"]):
                    for b in blocks:
                        r = self._run_block(r, b, ())
                    outs[i] = (r.t, (r.B, r.X, r.Y, 1))
            h, g = r.t, (r.B, r.X, r.Y, 1)
        else:
            h, g = ag.stem_conv_bn_rows(img, self.conv1, self.bn1, relu=True)
            h, g = ag.maxpool_rows(h, g)
        for i in range(nf, len(self.res_layers)):
            for b in getattr(self, self.res_layers[i]):
                s = (b.stride, b.stride, 1)
                w1, w3 = b.conv1.weight.flatten(1), b.conv3.weight.flatten(1)
                t, _ = ag.conv_bn_rows(h, w1, g, bn=b.bn1, relu=True)
                t, go = ag.conv_bn_rows(t, b.conv2.weight.unsqueeze(-1), g, bn=b.bn2, stride=s, pad=(1, 1, 0), relu=True)
                idn = h
                if b.downsample is not None:
                    wd = b.downsample[0].weight
                    wd = wd.flatten(1) if b.stride == 1 else wd.unsqueeze(-1)
                    idn, _ = ag.conv_bn_rows(h, wd, g, bn=b.downsample[1], stride=s, pad=0, relu=False)
                h, g = ag.conv_bn_rows(t, w3, go, bn=b.bn3, relu=True, res2d=idn)
            outs[i] = (h, g)
        return [outs[i] for i in self.out_indices]

    def _packed(self):
        def build():
            layers = [[self._block_packs(b) for b in getattr(self, name)] for name in self.res_layers]
            return dict(stem=stem_pack(self.conv1, self.bn1), layers=layers)
        return self._packs.get_modules((self,), build)

    @staticmethod
    def _readers_of(block):
        return tuple(pc for pc in (block["c1"], block["ds"]) if pc is not None)

    def forward_rows(self, img, readers=None):
        """img [BN,3,H,W] -> one Rows [BN, H_i, W_i, 1] per entry of ``out_indices``.  ``readers``: per entry, the layers outside this
        module that read it next (default: ``output_readers()``).  The inference path: under train() use ``forward_train``."""
        _eval_only(self)
        if self.training:
            raise NotImplementedError("ResNet.forward_rows is the inference path (folded BN); under train() call forward_train, or .eval()")
        p = self._packed()
        layers = p["layers"]
        if readers is None and self.output_readers is not None:
            readers = self.output_readers()
        if readers is not None and len(readers) != len(self.out_indices):
            readers = None
        h = stem_rows(img, p["stem"], relu=True, pool=True, twin_for=self._readers_of(layers[0][0]))
        outs = []
        for i, blocks in enumerate(layers):
            for j, b in enumerate(blocks):
                if j + 1 < len(blocks):
                    nxt = self._readers_of(blocks[j + 1])
                else:
                    nxt = self._readers_of(layers[i + 1][0]) if i + 1 < len(layers) else ()
                    if readers is not None and i in self.out_indices:
                        nxt += tuple(readers[self.out_indices.index(i)])
                h = self._run_block(h, b, nxt)
            if i in self.out_indices:
                outs.append(h)
        return [outs[sorted(self.out_indices).index(i)] for i in self.out_indices]

    def forward(self, x):
        """[BN,3,H,W] -> tuple of [BN,C_i,H_i,W_i]: zero-copy channels-last views that remember their Rows (eval), or that are
        attached to the graph (train() with ``train_enabled``)."""
        _eval_only(self)
        if self.training:
            return tuple(rows2d_as_bchw(t, g) for t, g in self.forward_train(x))
        return tuple(rows_as_bchw(r) for r in self.forward_rows(x))


@IMAGE_NECKS.register_module()
class SECONDFPN(nn.Module):
    def __init__(self, in_channels=[128, 128, 256], out_channels=[256, 256, 256], upsample_strides=[1, 2, 4],
                 norm_cfg=dict(type='BN', eps=1e-3, momentum=0.01), upsample_cfg=dict(type='deconv', bias=False),
                 conv_cfg=dict(type='Conv2d', bias=False), use_conv_for_no_stride=False, init_cfg=None):
        super().__init__()
        assert len(out_channels) == len(upsample_strides) == len(in_channels)
        if upsample_cfg.get("type") != "deconv":
            raise NotImplementedError("SECONDFPN: upsample_cfg type %r is not built; only 'deconv'" % upsample_cfg.get("type"))
        if conv_cfg.get("type", "Conv2d") != "Conv2d":
            raise NotImplementedError("SECONDFPN: conv_cfg type %r is not built; only 'Conv2d'" % conv_cfg.get("type"))
        if any(c % 4 for c in list(in_channels) + list(out_channels)):
            raise ValueError("SECONDFPN: channel counts must be multiples of 4 (16-byte rows)")
        self.in_channels, self.out_channels = list(in_channels), list(out_channels)
        self.fp16_enabled = False
        self.levels = []                       # ("conv", k) | ("deconv", s)
        deblocks = []
        for i, oc in enumerate(out_channels):                                    # second_fpn.py:44-65
            stride = upsample_strides[i]
            if stride > 1 or (stride == 1 and not use_conv_for_no_stride):
                if stride != int(stride) or int(stride) not in (1, 2, 4, 8):
                    raise NotImplementedError("SECONDFPN: upsample stride %r; deconvolutions with kernel = stride in 1, 2, 4, 8 only"
                                              % (stride,))
                s = int(stride)
                up = nn.ConvTranspose2d(in_channels[i], oc, s, stride=s, bias=bool(upsample_cfg.get("bias", True)))
                self.levels.append(("deconv", s))
            else:
                k = int(round(1.0 / stride))
                up = nn.Conv2d(in_channels[i], oc, k, stride=k, bias=bool(conv_cfg.get("bias", True)))
                self.levels.append(("conv", k))
            deblocks.append(nn.Sequential(up, _bn2d(norm_cfg, oc, "SECONDFPN"), nn.ReLU(inplace=True)))
        self.deblocks = nn.ModuleList(deblocks)
        self.init_cfg = init_cfg
        if init_cfg is None:
            self.init_cfg = [dict(type='Kaiming', layer='ConvTranspose2d'), dict(type='Constant', layer='NaiveSyncBatchNorm2d', val=1.0)]
        self._packs = PackCache(self)
        # training (opt-in, as ``ResNet.train_enabled``): the train() forward is differentiable, every BN in its own mode
        self.train_enabled = False
        self.norm_requires_grad = bool((norm_cfg or {}).get("requires_grad", True))

    def train(self, mode=True):
        super().train(mode)
        if getattr(self, "train_enabled", False) and not self.norm_requires_grad:        # build_norm_layer(requires_grad=False)
            for m in _bns(self):
                for p in m.parameters():
                    p.requires_grad = False
        return self

    def deblock_train(self, i, x2d, geom):
        """Deblock i on differentiable rows -> (rows [BN*H*W, out_channels[i]], (BN, H, W, 1)): a convolution is a ``conv_bn_rows``
        layer, a deconvolution the pointwise GEMM Cin -> s*s*Cout on a view of the module's weight + the child scatter of
        ``FpnSumFn`` (one level)."""
        ag = _ag()
        (kind, k), blk, oc = self.levels[i], self.deblocks[i], self.out_channels[i]
        up, bn = blk[0], blk[1]
        B, H, W, _ = geom
        if kind == "conv":
            if H % k or W % k:
                raise ValueError("SECONDFPN: a %d x %d level is not a multiple of its stride-%d convolution" % (H, W, k))
            w = up.weight.flatten(1) if k == 1 else up.weight.unsqueeze(-1)
            return ag.conv_bn_rows(x2d, w, geom, bn=bn, bias=up.bias, stride=(k, k, 1), pad=0, relu=True)
        if k == 1:
            return ag.conv_bn_rows(x2d, up.weight[:, :, 0, 0].t(), geom, bn=bn, bias=up.bias, relu=True)
        y = ag.deconv_bn_rows(x2d, up, bn, k, relu=True)
        fine = (B, H * k, W * k, 1)
        return ag.fpn_sum_rows([y], [k], oc, fine), fine

    def forward_train(self, xs):
        """[(rows, geom)] per level -> (rows [BN*H*W, sum(out_channels)], geom): the deblocks, then ``torch.cat`` over levels."""
        _check_trainable_norms(self)
        assert len(xs) == len(self.in_channels)
        for (t, g), c in zip(xs, self.in_channels):
            if t.shape[1] != c:
                raise ValueError("SECONDFPN: a level has %d channels, built for %d" % (t.shape[1], c))
        ups = [self.deblock_train(i, t, g) for i, (t, g) in enumerate(xs)]
        if len({g for _, g in ups}) != 1:
            raise ValueError("SECONDFPN: level sizes differ after up/down-sampling: inputs %s give %s (image sides must be multiples "
                             "of 32)" % ([g[1:3] for _, g in xs], [g[1:3] for _, g in ups]))
        return (torch.cat([t for t, _ in ups], 1) if len(ups) > 1 else ups[0][0]), ups[0][1]

    def _packed(self):
        def build():
            de = []
            for (kind, k), blk in zip(self.levels, self.deblocks):
                up, bn = blk[0], blk[1]
                if kind == "deconv":
                    pc = PackedConv(core.deconv_weight(up.weight, k), ksize=1)
                    # one BN channel serves the k*k children of a coarse pixel
                    pc.scale, pc.bias = core.folded_bn(bn, up.weight.device, up.bias, repeat=k * k)
                elif k == 1:
                    pc = PackedConv(up.weight.detach().reshape(up.weight.shape[0], -1), bn=bn, bias=up.bias, ksize=1)
                else:
                    pc = PackedConv(up.weight.detach().unsqueeze(-1), bn=bn, bias=up.bias, kernel=(k, k, 1), strides=(k, k, 1),
                                    pads=(0, 0, 0))
                de.append(pc)
            return de
        return self._packs.get_modules((self,), build)

    def reader_packs(self):
        """Per input level, the layer that reads it (``ResNet.output_readers``)."""
        return [(pc,) for pc in self._packed()]

    def out_size(self, i, H, W):
        kind, k = self.levels[i]
        return (H * k, W * k) if kind == "deconv" else (H // k, W // k)

    def deblock_rows(self, i, x, buf, off):
        """Deblock i (convolution or deconvolution + folded BN + ReLU) of Rows ``x`` into channels [off, off + out_channels[i]) of
        the rows ``buf`` [BN*H*W, stride]; nothing else of ``buf`` is written."""
        pc, (kind, k), oc = self._packed()[i], self.levels[i], self.out_channels[i]
        H, W = self.out_size(i, x.X, x.Y)
        assert buf.shape[0] == x.B * H * W and off % 4 == 0 and off + oc <= buf.shape[1]
        if kind == "conv" or k == 1:
            conv_rows(x, pc, relu=True, out=Rows(buf, x.B, H, W, 1, oc, coff=off, persistent=True))
            return
        u = conv_rows(x, pc, relu=True)                       # [BN*h*w, k*k*oc]: the children of every coarse pixel
        pp = (ctypes.c_void_p * 4)(u.t.data_ptr())
        ss = (ctypes.c_int * 4)(k)
        with core.TIMER.region("k_fpn_sum", 8.0 * x.B * H * W * oc):
            call("coocc_fpn_sum", pp, ss, 1, x.B, H, W, 1, oc, ptr(buf, offset=off), buf.shape[1], None)

    def forward_rows(self, xs):
        """One Rows [BN, H_i, W_i, 1] per level -> Rows [BN, H, W, 1] with sum(out_channels) channels: every deblock writes its
        channel slice of the one buffer."""
        _eval_only(self)
        if self.training:
            raise NotImplementedError("SECONDFPN.forward_rows is the inference path (folded BN); under train() call forward_train, or "
                                      ".eval()")
        assert len(xs) == len(self.in_channels)
        sizes =[self.out_size(i, x.X, x.Y) for i, x in enumerate(xs)]
        if len(set(sizes)) != 1 or min(sizes[0]) < 1 or len({x.B for x in xs}) != 1:
            raise ValueError("SECONDFPN: level sizes differ after up/down-sampling: inputs %s give %s (image sides must be multiples "
                             "of 32)" % ([(x.X, x.Y) for x in xs], sizes))
        for x, c in zip(xs, self.in_channels):
            if x.C != c or x.Z != 1:
                raise ValueError("SECONDFPN: a level has %d channels, built for %d" % (x.C, c))
        (H, W), B, dev = sizes[0], xs[0].B, xs[0].t.device
        Ct = sum(self.out_channels)
        buf = torch.empty(B * H * W, Ct, device=dev, dtype=_F32)
        off = 0
        for i, x in enumerate(xs):
            self.deblock_rows(i, x, buf, off)
            off += self.out_channels[i]
        return Rows(buf, B, H, W, 1, Ct)

    def forward(self, x):
        """list of [BN,C_i,H_i,W_i] -> [cat(ups, 1)] (second_fpn.py:75-91): a zero-copy view of channels-last rows.  Under train()
        (``train_enabled``) the inputs are read without a copy when their memory is channels-last, and the view is attached to the
        graph."""
        _eval_only(self)
        if self.training:
            return [rows2d_as_bchw(*self.forward_train([bchw_to_rows2d(t) for t in x]))]
        return [rows_as_bchw(self.forward_rows([bchw_to_rows(t) for t in x]))]


def _no_neck():
    return None


class NeckReaders:
    """The neck's deblock layers as ``ResNet.output_readers`` (holds the neck weakly, so the backbone's module tree and
    state_dict stay its own)."""

    def __init__(self, neck):
        import weakref
        self._neck = weakref.ref(neck)

    def __getstate__(self):
        return {}                     # the weak reference does not pickle: a restored backbone simply writes no twins for the neck

    def __setstate__(self, state):
        self._neck = _no_neck

    def __call__(self):
        neck = self._neck()
        return neck.reader_packs() if neck is not None and not neck.training else None


def run_image_encoder(backbone, neck, img):
    """``neck(backbone(img))`` on Rows end to end: the backbone's last layers write the H2 operands of the neck's deblocks.  The
    inference path: under train() call the modules (``neck(backbone(img))``)."""
    return neck.forward_rows(backbone.forward_rows(img, readers=neck.reader_packs()))
