"""Backward passes as ``torch.autograd.Function``s over the C-ABI kernels.

Scope: the differentiable ops of the hot path with frozen-statistics BN (eval-mode BN folded into a
per-channel scale/shift, exactly as the forward does): Conv3d / Linear (+BN, ReLU, residual) on
channels-last rows -- one Function, ``ConvRowsFn``, for every dense convolution, keyed by per-axis kernel / stride / padding
triples (a cubic layer is the one whose triples are equal) --, the G1 row gather, voxel pooling / fused lift-splat, the R2 render composite and
the FPN trilinear upsample-add.  Indices (FPS / ball / top-K / assignment, voxel keys) are
non-differentiable, as upstream.  Every backward is a HIP kernel; nothing falls back to torch ops.
"""
import torch

from . import _lib
from ._lib import call, ptr
from .core import TILE_HINT, conv_desc, deconv_weight, folded_bn, launch_conv, lib_pack, out_dim, stream_buffer, workspace, ztrim

_F32 = torch.float32
_tables = {}
# 3x3x3 stride-1 convolutions of the training path (forward and dgrad) through the Winograd kernels when the layer is
# large enough (core.WINO_MIN_ROWS); wgrad stays a direct GEMM.  COOCC_TRAIN_WINO=0: direct convolutions everywhere.
TRAIN_WINO = __import__("os").environ.get("COOCC_TRAIN_WINO", "1") != "0"
# weight gradients of those layers in the Winograd domain too (COOCC_TRAIN_WINO_WGRAD=0: direct k_wgrad)
TRAIN_WINO_WGRAD = TRAIN_WINO and __import__("os").environ.get("COOCC_TRAIN_WINO_WGRAD", "1") != "0"
# Winograd forward / dgrad GEMMs of the training path on the split-f16 engine (weights transformed + split on the device every
# step, coocc_wino_pack_weights_h2_dev); 0: the fp32-MFMA kernels of rounds 1-3
TRAIN_H2 = __import__("os").environ.get("COOCC_TRAIN_H2", "1") != "0"
# ... and the dgrad GEMMs too.  The operand of a dgrad GEMM is a GRADIENT, whose magnitude is set by the loss scale, not by
# BatchNorm, and an f16 is subnormal below 6.1e-5 (with a mean-reduced loss over 640 k voxels |dy| ~ 1e-6: the hi half alone would
# keep a handful of bits).  So the gradient operand gets a per-tensor power-of-two scale chosen ON THE DEVICE: the epilogue-backward
# pass that produces dacc also collects max |dacc| (coocc_conv_epilogue_bwd_ex), a one-thread kernel turns it into {2^k, 2^-k} with
# max |dacc| 2^k in [TARGET, 2 TARGET) (TARGET a power of two: k is the difference of the two frexp exponents), the operand writers
# multiply by the first word and the GEMM's alpha by the second -- exact, no host read, any loss scale.  TARGET = 1024 leaves the
# F(4x4) input transform (x 100 / 8) inside the f16 range: 2048 x 12.5 = 25600 < 65504.
# COOCC_TRAIN_H2_DGRAD=0: dgrad on the fp32-MFMA kernels.
TRAIN_H2_DGRAD = TRAIN_H2 and __import__("os").environ.get("COOCC_TRAIN_H2_DGRAD", "1") != "0"
TRAIN_H2_GRAD_TARGET = 1024.0
# ... and the weight gradients (csrc/wgrad_h2.hip): the Winograd-domain form of the 3x3x3 stride-1 layers (Z in {2, 4, 8}) and the
# 1x1x1 / Linear layers, both operands rewritten voxel-major (KH2), the gradient one with the same device-chosen scale.
# COOCC_TRAIN_H2_WGRAD=0: the fp32-MFMA k_wgrad.
TRAIN_H2_WGRAD = TRAIN_H2 and __import__("os").environ.get("COOCC_TRAIN_H2_WGRAD", "1") != "0"


def _amax_word(dev):
    """The zeroed words (COOCC_AMAX_WORDS) coocc_conv_epilogue_bwd_ex collects max |dacc| in (left zero by its second kernel); one
    set per stream."""
    return stream_buffer(dev, "amax", 2048, torch.int32, zero=True)


def _pad4(n):
    return (n + 3) // 4 * 4


def epilogue_bwd(dout, out, scale, relu, pad_to=None, want_res=False, want_bias=False, want_gscale=False):
    """The backward of a GEMM epilogue y = relu(scale * acc + shift + res) over dout / out [Mo, Cout] (``out`` may be None without
    ReLU, ``scale`` None for 1) -> (dacc [Mo, pad_to or Cout], zero-filled past Cout; dres [Mo, Cout] | None; dbias [Cout] = the
    column sums of dacc | None; gscale | None: the device-side {2^k, 2^-k} of max |dacc|, see TRAIN_H2_DGRAD).  The one
    coocc_conv_epilogue_bwd_ex call; whether the pass is needed at all, and when a gradient scale is wanted, is the caller's."""
    Mo, Cout = dout.shape
    dev, Cp = dout.device, pad_to or Cout
    dacc = torch.zeros(Mo, Cp, device=dev, dtype=_F32) if Cp != Cout else torch.empty(Mo, Cp, device=dev, dtype=_F32)
    dres = torch.empty(Mo, Cout, device=dev, dtype=_F32) if want_res else None
    dbias = torch.empty(Cout, device=dev, dtype=_F32) if want_bias else None
    gscale = torch.empty(2, device=dev, dtype=_F32) if want_gscale else None
    ws = workspace(dev)
    call("coocc_conv_epilogue_bwd_ex", ptr(dout), Cout, ptr(out), Cout, ptr(scale), Mo, Cout, int(relu), ptr(dacc), Cp, ptr(dres), Cout,
         0, ptr(dbias), 0, ptr(ws), ws.numel(), ptr(_amax_word(dev)) if want_gscale else None, ptr(gscale), TRAIN_H2_GRAD_TARGET)
    return dacc, dres, dbias, gscale


def _triple(v):
    """An int, or a per-axis (x, y, z) triple, as a triple of ints."""
    return (int(v),) * 3 if isinstance(v, int) else tuple(int(a) for a in v)


def _out_dims(dims, kernel, strides, pads):
    return tuple(out_dim(n, k, s, p) for n, k, s, p in zip(dims, kernel, strides, pads))


def tap_table(dev, B, Xi, Yi, Zi, kernel, strides, pads, dgrad):
    """[taps, M] int32 row table of a conv geometry given by per-axis kernel / stride / padding triples (cached): forward reads /
    dgrad reads, tap t = (dx*ky + dy)*kz + dz (coocc_conv_tap_table3)."""
    key = (dev.index, B, Xi, Yi, Zi, kernel, strides, pads, bool(dgrad))
    if key not in _tables:
        Xo, Yo, Zo = _out_dims((Xi, Yi, Zi), kernel, strides, pads)
        M = B * Xi * Yi * Zi if dgrad else B * Xo * Yo * Zo
        t = torch.empty(kernel[0] * kernel[1] * kernel[2], M, dtype=torch.int32, device=dev)
        call("coocc_conv_tap_table3", B, Xi, Yi, Zi, Xo, Yo, Zo, *kernel, *strides, *pads, int(bool(dgrad)), ptr(t))
        _tables[key] = t
    return _tables[key]


_live = {}


def live_taps(dev, B, Xi, Yi, Zi, kernel, strides, pads):
    """(indices of the taps that read at least one real voxel, their rows of the forward table), cached per geometry."""
    key = (dev.index, B, Xi, Yi, Zi, kernel, strides, pads)
    if key not in _live:
        tb = tap_table(dev, B, Xi, Yi, Zi, kernel, strides, pads, False)
        idx = torch.nonzero((tb >= 0).any(1)).flatten()
        _live[key] = (idx, tb[idx].contiguous())
    return _live[key]


_classes = {}


def dgrad_classes(dev, B, Xi, Yi, Zi, kernel, strides, pads):
    """Strided dgrad by residue class: input voxels with the same (x mod sx, y mod sy, z mod sz) are reached through the same
    subset of taps (stride 2, k = 3: 1, 2, 4 or 8 of the 27), so each class is its own small row-table GEMM instead
    of 27 taps of which 7/8 of the table entries are empty.  -> list of (rows int32 [Mc], taps int64 [Tc], table
    int32 [Tc, Mc]) over the non-empty classes, cached per geometry.  Stride 4 with a 3-wide kernel: the class x mod 4 == 2
    (pad 1) is reached through no tap -- no output reads those voxels -- and is left out; their gradient is the zero the caller
    initialised."""
    key = (dev.index, B, Xi, Yi, Zi, kernel, strides, pads)
    if key not in _classes:
        tb = tap_table(dev, B, Xi, Yi, Zi, kernel, strides, pads, True)          # [taps, Mi]: output row or -1
        sx, sy, sz = strides
        m = torch.arange(B * Xi * Yi * Zi, device=dev)
        cls = (((m // (Yi * Zi)) % Xi % sx) * sy + (m // Zi) % Yi % sy) * sz + m % Zi % sz
        out = []
        for c in range(sx * sy * sz):
            rows = torch.nonzero(cls == c).flatten()
            if rows.numel() == 0:
                continue
            sub = tb[:, rows]
            taps = torch.nonzero((sub >= 0).any(1)).flatten()
            if taps.numel() == 0:
                continue
            out.append((rows.int().contiguous(), taps, sub[taps].contiguous()))
        _classes[key] = out
    return _classes[key]


def pack_weights_dev(w, Cout, Cin, taps, mode):
    """Device-side fragment-major packing (modes: 0 fwd, 1 fwd tap-major, 2 dgrad flipped, 3 dgrad)."""
    return lib_pack("coocc_conv_pack_weights_dev", w.detach().float().contiguous(), Cout, Cin, taps, mode)


def pack_weights_h2_dev(w, Cout, Cin, taps, mode):
    """``pack_weights_dev`` for the split-f16 engine."""
    return lib_pack("coocc_conv_pack_weights_h2_dev", w, Cout, Cin, taps, mode)


def _z_taps(w, lo, hi):
    """The z taps lo..hi of 3x3x3 weights, [Cout, Cin, 9 * (hi - lo + 1)]."""
    Cout, Cin = w.shape[:2]
    return w.view(Cout, Cin, 3, 3, 3)[..., lo:hi + 1].contiguous().view(Cout, Cin, -1)


def _h2_direct(K, flops):
    """Direct-form GEMMs of the training path on the split-f16 engine: K % 32 == 0 and enough work to pay for the operand pass."""
    from . import core
    return TRAIN_H2 and core.CONV_ENGINE == "h2" and core.H2_DIRECT and K % 32 == 0 and flops >= core.H2_DIRECT_MIN_FLOPS


def _rows_h2(x2d, C, scale_dev=None):
    xh = torch.empty(x2d.shape[0], C, device=x2d.device, dtype=_F32)
    call("coocc_rows_to_h2_ex", ptr(x2d), x2d.shape[1], x2d.shape[0], C, 1.0, ptr(scale_dev), ptr(xh))
    return xh


class _DevWino:
    """What core.conv_rows_wino needs of a PackedConv, with the Winograd packs transformed on the device from the live
    parameter (training re-packs every step): forward packs, or (``dgrad``) the packs of dx = conv(dy, W').  ``h2``: the GEMM runs
    on the split-f16 engine like inference's (core.h2_capable), on packs transformed + split on the device."""

    def __init__(self, w5, dgrad, scale=None, bias=None, h2=False):
        Cout, Cin = w5.shape[:2]
        self.Cin, self.Cout = (Cout, Cin) if dgrad else (Cin, Cout)
        self.scale, self.bias, self.h2 = scale, bias, h2
        self._w_raw, self.wino_tile = True, None
        self.wino_kz, self.aniso = 3, False       # 3x3x3 stride-1 layers only (core.conv_rows_wino)
        self._w5, self._dgrad, self._packs = w5, int(bool(dgrad)), {}
        self.operand_scale_dev = None         # split-f16 engine, dgrad: {scale, 1 / scale} of the gradient rows, chosen on the device

    def _pack(self, entry, tile):
        if (entry, tile) not in self._packs:
            self._packs[entry, tile] = lib_pack(entry, self._w5, *self._w5.shape[:2], tile, self._dgrad).view((tile + 2) ** 2, -1)
        return self._packs[entry, tile]

    def wino_pack(self, tile):
        return self._pack("coocc_wino_pack_weights_dev", tile)

    def wino_h2_pack(self, tile):
        return self._pack("coocc_wino_pack_weights_h2_dev", tile)


def _wino_train(x2d, geom, w5, dgrad, out2d, scale, shift, res2d, relu, grad_scale=None):
    """Winograd path of a 3x3x3 stride-1 pad-1 convolution in training (forward or dgrad); False if not eligible.
    ``grad_scale``: dgrad on the split-f16 engine -- the device-side {scale, 1 / scale} of the gradient rows x2d."""
    from . import core
    if not TRAIN_WINO:
        return False
    B, X, Y, Z = geom
    pk = _DevWino(w5, dgrad, scale, shift, h2=(TRAIN_H2_DGRAD and grad_scale is not None) if dgrad else TRAIN_H2)
    pk.operand_scale_dev = grad_scale if dgrad else None
    xr = core.Rows(x2d, B, X, Y, Z, pk.Cin)
    plan = core.wino_plan(xr, pk, out2d.shape[0], 1 if res2d is not None else 0)
    if plan is None:
        return False
    core.conv_rows_wino(xr, pk, core.Rows(out2d, B, X, Y, Z, pk.Cout), relu,
                        core.Rows(res2d, B, X, Y, Z, pk.Cout) if res2d is not None else None, plan)
    return True


_ztables = {}


def _kh2(x2d, rows, rows_pad, C, scale, scale_dev, out):
    call("coocc_rows_to_kh2", ptr(x2d), C, rows, rows_pad, C, float(scale), ptr(scale_dev), ptr(out))
    return out


def _wino_wgrad(x2d, dacc, geom, Cin, Cout, dw, gscale=None):
    """Weight gradient of a 3x3x3 stride-1 pad-1 layer in the Winograd domain; False if the layer is not eligible.
    ``gscale``: the device-side {scale, 1 / scale} of dacc -> the GEMM runs on the split-f16 engine (csrc/wgrad_h2.hip)."""
    from . import core
    if not TRAIN_WINO_WGRAD:
        return False
    B, X, Y, Z = geom
    dev = x2d.device
    xr = core.Rows(x2d, B, X, Y, Z, Cin)
    pk = _DevWino(torch.empty(Cout, Cin, 0, device=dev), False)      # geometry only: no packs are made (fp32 V / dM rows)
    plan = core.wino_plan(xr, pk, x2d.shape[0], 0)
    if plan is None:
        return False
    tile, pts, Tx, Ty, rows, G, _ = plan
    ws = workspace(dev)
    if ws.numel() < pts * 3 * Cin * Cout or pts * G * max(Cin, Cout) * 4 >= 0xFFFFFF00:
        return False
    if TRAIN_H2_WGRAD and gscale is not None and core.CONV_ENGINE == "h2" and Z in (2, 4, 8) and Cin % 4 == 0 and Cout % 4 == 0:
        # both operands straight into the voxel-major split-f16 form (no fp32 V / dM): V (|V| <= 100 |x|) with the forward path's
        # static scale; dM = A dY A^T amplifies by up to 15^2 on top of the device-chosen gradient scale (max |dacc| -> [1024, 2048)):
        # 1/16 keeps it below the f16 range and the range guard (2048 x 225 / 16 = 28800 < 32768)
        vs, ms = core.H2_WINO_SCALE[tile], 1.0 / 16.0
        Vk = core._wino_buffer(dev, "Vk", pts * G * Cin)
        Mk = core._wino_buffer(dev, "Mk", pts * G * Cout)
        call("coocc_wino_operand_kh2", 0, ptr(x2d), x2d.shape[1], B, X, Y, Z, Cin, tile, ptr(Vk), G, vs, None)
        call("coocc_wino_operand_kh2", 1, ptr(dacc), dacc.shape[1], B, X, Y, Z, Cout, tile, ptr(Mk), G, ms, ptr(gscale))
        with _lib.TIMER.region("k_wgrad_h2 wino%d" % tile, 2.0 * pts * rows * 3 * Cin * Cout):
            call("coocc_wino_wgrad_h2", ptr(Vk), ptr(Mk), G, Z, Cin, Cout, tile, 1.0 / (vs * ms), ptr(gscale, offset=1), ptr(dw), 0,
                 ptr(ws), ws.numel())
        return True
    V = core._wino_buffer(dev, "V", pts * G * Cin)
    dM = core._wino_buffer(dev, "M", pts * G * Cout)
    if G > rows:        # rows past the valid ones (stale from other layers) must not contribute
        V[:pts * G * Cin].view(pts, G, Cin)[:, rows:].zero_()
        dM[:pts * G * Cout].view(pts, G, Cout)[:, rows:].zero_()
    call("coocc_wino_input", ptr(x2d), x2d.shape[1], B, X, Y, Z, Cin, tile, ptr(V), G)
    call("coocc_wino_gradout", ptr(dacc), dacc.shape[1], B, X, Y, Z, Cout, tile, ptr(dM), G)
    key = (dev.index, pts * G, Z)
    if key not in _ztables:
        t = torch.empty(3, pts * G, dtype=torch.int32, device=dev)
        call("coocc_wino_ztap_table", pts * G, Z, ptr(t))
        _ztables[key] = t
    with _lib.TIMER.region("k_wgrad wino%d" % tile, 2.0 * pts * rows * 3 * Cin * Cout):
        call("coocc_wino_wgrad", ptr(V), ptr(dM), G, Z, Cin, Cout, tile, ptr(_ztables[key]), ptr(dw), 0, ptr(ws), ws.numel())
    return True


def _launch(d, x2d, in_C, tag, h2_alpha, alpha_dev):
    """coocc_conv_fwd of ``d`` over the rows x2d.  ``h2_alpha``: x2d holds H2 rows (coocc_rows_to_h2, operand scale 1 / h2_alpha)
    and d.w an H2 pack: split-f16 engine; ``alpha_dev``: device word the accumulators are also multiplied by (the inverse of a
    device-chosen operand scale)."""
    if h2_alpha is not None:
        d.in_stride, d.mfma_dtype, d.alpha, d.alpha_dev, tag = in_C, 3, float(h2_alpha), alpha_dev, "k_gemm_h2 " + tag
    launch_conv(d, x2d.device, tag, 2.0 * d.M * in_C * d.Cout * d.taps)


def _conv_launch(x2d, in_C, w_packed, out2d, Cout, geom_in, geom_out, kernel, strides, pads, scale, shift, res2d, relu,
                 tag="conv_fwd", h2_alpha=None, alpha_dev=None):
    """A convolution over a grid: rows of ``geom_in`` -> rows of ``geom_out`` through the descriptor's per-axis fields."""
    d = conv_desc(x2d.device, in_=ptr(x2d), w=ptr(w_packed), out=ptr(out2d), scale=ptr(scale), bias=ptr(shift), res=ptr(res2d),
                  M=out2d.shape[0], Cin=in_C, Cout=Cout, taps=kernel[0] * kernel[1] * kernel[2], in_stride=x2d.shape[1],
                  out_stride=out2d.shape[1], res_stride=res2d.shape[1] if res2d is not None else 0, B=geom_in[0], Xi=geom_in[1],
                  Yi=geom_in[2], Zi=geom_in[3], Xo=geom_out[1], Yo=geom_out[2], Zo=geom_out[3], ksize=max(kernel), stride=max(strides),
                  pad=max(pads), relu=int(relu), res_mode=1 if res2d is not None else 0, tile_hint=TILE_HINT)
    (d.kx, d.ky, d.kz), (d.px, d.py, d.pz), (d.sx, d.sy, d.sz) = kernel, pads, strides
    _launch(d, x2d, in_C, tag, h2_alpha, alpha_dev)


def _table_launch(x2d, in_C, w_packed, out2d, Cout, table, scale=None, shift=None, res2d=None, relu=False, tag="sparse", out_rows=None,
                  h2_alpha=None, alpha_dev=None):
    """A row-table GEMM: out2d[o] (or out2d[out_rows[o]]) = epi(sum_t W_t . x2d[table[t][o]]) with ``table`` int32 [taps, M], -1 =
    no row.  With a table coocc_conv_fwd reads no geometry but the number of input rows, stated as B * Xi * Yi * Zi."""
    M = out_rows.shape[0] if out_rows is not None else out2d.shape[0]
    d = conv_desc(x2d.device, in_=ptr(x2d), w=ptr(w_packed), out=ptr(out2d), scale=ptr(scale), bias=ptr(shift), res=ptr(res2d),
                  gather=ptr(table, torch.int32), out_rows=ptr(out_rows, torch.int32), M=M, Cin=in_C, Cout=Cout, taps=table.shape[0],
                  in_stride=x2d.shape[1], out_stride=out2d.shape[1], res_stride=res2d.shape[1] if res2d is not None else 0,
                  B=1, Xi=x2d.shape[0], Yi=1, Zi=1, Xo=out2d.shape[0], Yo=1, Zo=1, ksize=1, stride=1, pad=0, relu=int(relu),
                  res_mode=1 if res2d is not None else 0, tile_hint=TILE_HINT)
    _launch(d, x2d, in_C, tag, h2_alpha, alpha_dev)


_UNIT, _NOPAD = (1, 1, 1), (0, 0, 0)


def _wino_layer(kernel, strides, pads):
    """The layers the training Winograd kernels (forward, dgrad, wgrad) cover: 3x3x3, stride 1, pad 1."""
    return kernel == (3, 3, 3) and strides == _UNIT and pads == _UNIT


def _ztrim(Zin, Zout, kernel, strides, pads):
    """``core.ztrim`` of a 3x3x3 layer with equal strides and pads: ((lo, hi), the launch's kernel, its pads) when z taps that
    only read padding can be dropped (exact), else None."""
    if kernel != (3, 3, 3) or len(set(strides)) != 1 or len(set(pads)) != 1:
        return None
    trim, kd = ztrim(Zin, Zout, strides[0], pads[0])
    return None if trim is None else (trim, kd[:3], kd[3:])


class ConvRowsFn(torch.autograd.Function):
    """y = relu(scale * conv(x, W) + shift + res) on channels-last rows for a layer with per-axis ``kernel`` / ``strides`` / ``pads``
    triples (as ``core.PackedConv`` describes them; a cubic layer has equal ones); weight [Cout,Cin,kx,ky,kz] (or [Cout,Cin] for one
    tap); scale/shift are constants (folded eval-mode BN and/or the conv bias).  Differentiable in x, W, conv bias and res.
    Routes by the triple: Winograd forward / dgrad / wgrad for 3x3x3 stride 1 pad 1, the z trim for 3x3x3 with equal strides and
    pads, the split-f16 (KH2) weight gradient for one tap at unit strides, residue-class dgrad wherever a stride exceeds 1; direct
    form otherwise (the one-z-tap Winograd form of inference is not extended to training: the device-side packs are 3x3x3 only)."""

    @staticmethod
    def forward(ctx, x2d, weight, bias, res2d, scale, shift, geom, kernel, strides, pads, relu):
        B, Xi, Yi, Zi = geom
        Cout, Cin = weight.shape[0], weight.shape[1]
        taps = kernel[0] * kernel[1] * kernel[2]
        assert tuple(weight.shape[2:]) in (kernel, ()), "weight %s is not [Cout,Cin,%d,%d,%d]" % ((tuple(weight.shape),) + kernel)
        assert x2d.shape == (B * Xi * Yi * Zi, Cin) and x2d.is_contiguous() and Cin % 4 == 0
        geom_out = (B,) + _out_dims((Xi, Yi, Zi), kernel, strides, pads)
        out = torch.empty(geom_out[0] * geom_out[1] * geom_out[2] * geom_out[3], Cout, device=x2d.device, dtype=_F32)
        eff_shift = shift
        if bias is not None:    # y = scale * (conv + b) + shift
            eff_shift = (bias.detach() * scale if scale is not None else bias.detach()) + (shift if shift is not None else 0)
            eff_shift = eff_shift.float().contiguous()
        w_ = weight.detach().float().contiguous()
        if not (_wino_layer(kernel, strides, pads) and
                _wino_train(x2d, geom, w_.view(Cout, Cin, 3, 3, 3), False, out, scale, eff_shift, res2d, relu)):
            wsub, kd, pd = w_.view(Cout, Cin, taps), kernel, pads
            trim = _ztrim(Zi, geom_out[3], kernel, strides, pads)
            if trim is not None:         # z taps that only read padding are dropped (exact)
                wsub, kd, pd = _z_taps(w_, *trim[0]), trim[1], trim[2]
            nt = kd[0] * kd[1] * kd[2]
            if _h2_direct(Cin, 2.0 * out.shape[0] * Cin * Cout * nt):
                _conv_launch(_rows_h2(x2d, Cin), Cin, pack_weights_h2_dev(wsub, Cout, Cin, nt, 0), out, Cout, geom, geom_out, kd,
                             strides, pd, scale, eff_shift, res2d, relu, h2_alpha=1.0)
            else:
                _conv_launch(x2d, Cin, pack_weights_dev(wsub, Cout, Cin, nt, 0), out, Cout, geom, geom_out, kd, strides, pd, scale,
                             eff_shift, res2d, relu)
        ctx.save_for_backward(x2d, weight, out, scale if scale is not None else torch.empty(0, device=x2d.device))
        ctx.cfg = (geom, geom_out, kernel, strides, pads, relu, bias is not None, res2d is not None, scale is not None)
        return out

    @staticmethod
    def backward(ctx, dout):
        from . import core
        x2d, weight, out, scale = ctx.saved_tensors
        geom, geom_out, kernel, strides, pads, relu, has_bias, has_res, has_scale = ctx.cfg
        scale = scale if has_scale else None
        B, Xi, Yi, Zi = geom
        Cout, Cin = weight.shape[0], weight.shape[1]
        taps = kernel[0] * kernel[1] * kernel[2]
        Mo, Mi = out.shape[0], x2d.shape[0]
        dev = x2d.device
        dout = dout.float().contiguous()
        need_x, need_w, need_b, need_res = ctx.needs_input_grad[:4]
        unit, wino3 = strides == _UNIT, _wino_layer(kernel, strides, pads)
        Cp = _pad4(Cout)
        ws = workspace(dev)
        # split-f16 GEMMs that read dacc: max |dacc| collected by the pass that writes dacc -> {scale, 1 / scale} on the device (see
        # TRAIN_H2_DGRAD).  Asked for by the stride-1 dgrad (its K is Cout) and by the layers whose weight gradient has a split-f16
        # form (Winograd domain, one tap); no other layer collects an amax it would never read
        want_gscale = (core.CONV_ENGINE == "h2" and Cp == Cout and unit and Cin % 4 == 0 and
                       ((TRAIN_H2_DGRAD and need_x and Cout % 32 == 0) or (TRAIN_H2_WGRAD and need_w and (wino3 or taps == 1))))
        dacc, dres, dbias, gscale = epilogue_bwd(dout, out, scale, relu, pad_to=Cp, want_res=has_res and need_res,
                                                 want_bias=has_bias and need_b, want_gscale=want_gscale)
        gscale_d = gscale if (TRAIN_H2_DGRAD and Cout % 32 == 0) else None      # the dgrad GEMM's K is Cout
        if dbias is not None and scale is not None:
            dbias = dbias * scale
        dx = dw = None
        w_ = weight.detach().float().contiguous()
        w3 = w_.view(Cout, Cin, taps)
        if need_x:
            dx = torch.empty(Mi, Cin, device=dev, dtype=_F32)
            if wino3 and Cp == Cout and _wino_train(dacc, geom, w_.view(Cout, Cin, 3, 3, 3), True, dx, None, None, None, False,
                                                    grad_scale=gscale_d):
                pass
            elif unit:
                # dx = conv(dacc, W') with every tap axis flipped (pack mode 2 reverses the mixed-radix tap index = each axis) and
                # pad' = k - 1 - pad per axis
                wsub, kd, pd = w3, kernel, tuple(k - 1 - p for k, p in zip(kernel, pads))
                trim = _ztrim(geom_out[3], Zi, kernel, strides, pd)      # z taps of the flipped kernel that see real dy voxels
                if trim is not None:
                    wsub, kd, pd = _z_taps(w_, 2 - trim[0][1], 2 - trim[0][0]), trim[1], trim[2]
                nt = kd[0] * kd[1] * kd[2]
                if gscale_d is not None and _h2_direct(Cout, 2.0 * Mi * Cin * Cout * nt):
                    # the gradient operand scaled by gscale[0] (chosen on the device), undone by the GEMM through gscale[1]
                    _conv_launch(_rows_h2(dacc, Cout, gscale_d), Cout, pack_weights_h2_dev(wsub, Cout, Cin, nt, 2), dx, Cin, geom_out,
                                 geom, kd, strides, pd, None, None, None, False, tag="conv_dgrad", h2_alpha=1.0,
                                 alpha_dev=ptr(gscale_d, offset=1))
                else:
                    _conv_launch(dacc, Cp, pack_weights_dev(wsub, Cout, Cin, nt, 2), dx, Cin, geom_out, geom, kd, strides, pd, None,
                                 None, None, False, tag="conv_dgrad")
            else:
                dx.zero_()          # voxels no output reads (and classes without taps) get a zero gradient
                for rows_c, taps_c, table_c in dgrad_classes(dev, B, Xi, Yi, Zi, kernel, strides, pads):
                    wp = pack_weights_dev(w3.index_select(2, taps_c), Cout, Cin, taps_c.numel(), 3)
                    _table_launch(dacc, Cp, wp, dx, Cin, table_c, tag="conv_dgrad", out_rows=rows_c)
        if need_w:
            dw = torch.empty(Cout, Cin, taps, device=dev, dtype=_F32)
            if wino3 and Cp == Cout and _wino_wgrad(x2d, dacc, geom, Cin, Cout, dw, gscale if TRAIN_H2_WGRAD else None):
                pass
            elif (TRAIN_H2_WGRAD and gscale is not None and taps == 1 and unit
                  and 2.0 * Mo * Cin * Cout >= core.H2_DIRECT_MIN_FLOPS):
                # 1x1x1 / Linear: both operands voxel-major (KH2), the gradient with its device-chosen scale
                Mp = -(-Mo // 16) * 16
                xk = _kh2(x2d, Mi, Mp, Cin, 1.0, None, torch.empty(Mp * Cin, device=dev, dtype=_F32))
                dk = _kh2(dacc, Mo, Mp, Cout, 1.0, gscale, torch.empty(Mp * Cout, device=dev, dtype=_F32))
                with _lib.TIMER.region("k_wgrad_h2", 2.0 * Mo * Cin * Cout):
                    call("coocc_conv_wgrad_h2", ptr(xk), ptr(dk), Mp, Cin, Cout, 1.0, ptr(gscale, offset=1), ptr(dw), 0, ptr(ws),
                         ws.numel())
            else:
                tb = tap_table(dev, B, Xi, Yi, Zi, kernel, strides, pads, False) if (taps > 1 or not unit) else None
                live = live_taps(dev, B, Xi, Yi, Zi, kernel, strides, pads) if tb is not None else None
                if live is not None and live[0].numel() < taps:
                    # thin grids (Z = 1, 2): taps that only ever read padding have a zero gradient -- skip their GEMMs
                    idx, tb_live = live
                    dw_live = torch.empty(Cout, Cin, idx.numel(), device=dev, dtype=_F32)
                    with _lib.TIMER.region("k_wgrad", 2.0 * Mo * Cin * Cout * idx.numel()):
                        call("coocc_conv_wgrad", ptr(x2d), Mi, Cin, ptr(dacc), Cp, ptr(tb_live), Mo, Cin, Cout, idx.numel(),
                             ptr(dw_live), 0, ptr(ws), ws.numel())
                    dw.zero_()
                    dw.index_copy_(2, idx, dw_live)
                else:
                    with _lib.TIMER.region("k_wgrad", 2.0 * Mo * Cin * Cout * taps):
                        call("coocc_conv_wgrad", ptr(x2d), Mi, Cin, ptr(dacc), Cp, ptr(tb), Mo, Cin, Cout, taps, ptr(dw), 0, ptr(ws),
                             ws.numel())
            dw = dw.view_as(weight)
        return dx, dw, dbias, dres, None, None, None, None, None, None, None


def conv3d_rows(x2d, weight, geom, bias=None, bn=None, stride=1, pad=None, relu=True, res2d=None):
    """Differentiable Conv3d(+eval BN)(+res)(+ReLU) on rows [B*X*Y*Z, Cin] -> ([B*Xo*Yo*Zo, Cout], out geom).
    ``weight`` [Cout,Cin,kx,ky,kz] (any strides: a permuted view of a reference [.,.,kz,ky,kx] parameter keeps its gradient), or
    [Cout,Cin] for a Linear / 1x1; ``stride`` / ``pad``: an int or a per-axis triple (``pad`` None: k // 2 per axis)."""
    kernel = tuple(weight.shape[2:]) if weight.dim() == 5 else _UNIT
    strides = _triple(stride)
    pads = _triple(pad) if pad is not None else tuple(k // 2 for k in kernel)
    scale, shift = folded_bn(bn, x2d.device) if bn is not None else (None, None)
    out = ConvRowsFn.apply(x2d.contiguous(), weight, bias, res2d, scale, shift, tuple(geom), kernel, strides, pads, relu)
    return out, (geom[0],) + _out_dims(tuple(geom[1:]), kernel, strides, pads)


def linear_rows(x2d, weight, bias=None, relu=False):
    """Differentiable nn.Linear (+ReLU) on rows through the same kernels."""
    n = x2d.shape[0]
    return ConvRowsFn.apply(x2d.contiguous(), weight, bias, None, None, None, (1, n, 1, 1), _UNIT, _UNIT, _NOPAD, relu)


# ----------------------------------------------------------------------------- G1 gather
class GatherRowsFn(torch.autograd.Function):
    """out[r] = src[idx[r]] (zeros where idx < 0); backward scatter-adds (bifuser_n.py:138-169 feature grads)."""

    @staticmethod
    def forward(ctx, src, idx):
        assert src.dim() == 2 and src.shape[1] % 4 == 0 and idx.dtype == torch.int32
        out = torch.empty(idx.numel(), src.shape[1], device=src.device, dtype=_F32)
        call("coocc_gather_rows", ptr(src.contiguous()), src.shape[1], ptr(idx.contiguous()), idx.numel(), src.shape[1],
             ptr(out), src.shape[1])
        ctx.save_for_backward(idx)
        ctx.nrows = src.shape[0]
        return out

    @staticmethod
    def backward(ctx, dout):
        (idx,) = ctx.saved_tensors
        C = dout.shape[1]
        dsrc = torch.zeros(ctx.nrows, C, device=dout.device, dtype=_F32)
        call("coocc_scatter_add_rows", ptr(dout.float().contiguous()), C, ptr(idx.contiguous()), idx.numel(), C, ptr(dsrc), C)
        return dsrc, None


def gather_rows(src, idx):
    return GatherRowsFn.apply(src, idx)


class ScatterRowsFn(torch.autograd.Function):
    """out = zeros [nrows, C]; out[idx[r]] = vals[r] (idx unique, negative entries skipped); backward gathers."""

    @staticmethod
    def forward(ctx, vals, idx, nrows):
        assert vals.dim() == 2 and vals.shape[1] % 4 == 0 and idx.dtype == torch.int32
        C = vals.shape[1]
        out = torch.zeros(nrows, C, device=vals.device, dtype=_F32)
        call("coocc_scatter_add_rows", ptr(vals.float().contiguous()), C, ptr(idx.contiguous()), idx.numel(), C, ptr(out), C)
        ctx.save_for_backward(idx)
        return out

    @staticmethod
    def backward(ctx, dout):
        (idx,) = ctx.saved_tensors
        C = dout.shape[1]
        dv = torch.empty(idx.numel(), C, device=dout.device, dtype=_F32)
        call("coocc_gather_rows", ptr(dout.float().contiguous()), C, ptr(idx.contiguous()), idx.numel(), C, ptr(dv), C)
        return dv, None, None


def fuser_fuse_train(fuser, img_rows, pts_rows, sr):
    """Differentiable G1 (bifuser_n.py:138-169) on rows: the neighbour tables of a ``BiFuser_N.search`` result are
    indices (not differentiated, as upstream); gradients reach both feature volumes and ``knn_enc``.
    img_rows / pts_rows: [V, C] channels-last rows of the two inputs -> [V, 4C] = (img | pts | fused_img | fused_pts).
    The gate product and the concat are torch elementwise / copy ops; gather, Linear and scatter are the HIP kernels."""
    V, C = img_rows.shape
    W, b = fuser.knn_enc[0].weight, fuser.knn_enc[0].bias

    def direction(src, rows, out_idx, gate_src):
        if rows is None or rows.shape[1] == 0:
            return torch.zeros(V, C, device=src.device, dtype=_F32)
        g = torch.cat([gather_rows(src, rows[k].contiguous()) for k in range(rows.shape[0])], 1)
        y = linear_rows(g, W, b, relu=True) * gather_rows(gate_src, out_idx)
        return ScatterRowsFn.apply(y, out_idx, V)
    fused_img = direction(img_rows, sr.rows, sr.lin_pts, pts_rows)
    fused_pts = direction(pts_rows, sr.rows_p, sr.lin_img, img_rows)
    return torch.cat([img_rows, pts_rows, fused_img, fused_pts], 1)


# ----------------------------------------------------------------------------- P2 pooling
class LiftSplatFn(torch.autograd.Function):
    """Fused lift (x) splat (view_transformer.lift_splat) with gradients for depth_prob and the context features."""

    @staticmethod
    def forward(ctx, vt, depth_prob, img_feat, geom_feats):
        from ._lib import host_f32
        from .ops import _pool_workspace
        BN, C, H, W = img_feat.shape
        D = depth_prob.shape[1]
        B = geom_feats.shape[0]
        X, Y, Z = (int(v) for v in vt.nx.tolist())
        dev = img_feat.device
        feat = torch.empty(BN * H * W, C, device=dev, dtype=_F32)
        call("coocc_ncdhw_to_ndhwc", ptr(img_feat.float().contiguous()), ptr(feat), BN, C, H * W, C, 0)
        lo = (vt.bx - vt.dx / 2.).tolist() + vt.dx.tolist()
        npts = BN * D * H * W
        out = torch.empty(B * X * Y * Z, C, device=dev, dtype=_F32)
        ws = _pool_workspace(dev, npts, B * X * Y * Z)
        dp = depth_prob.float().contiguous()
        g = geom_feats.reshape(-1, 3).float().contiguous()
        from .ops import pool_ws_clean, pool_ws_done
        call("coocc_lift_splat", ptr(dp), ptr(feat), ptr(g), BN, D, H, W, C, npts // B, host_f32(lo), B, X, Y, Z, ptr(out), C,
             ptr(ws), ws.numel(), pool_ws_clean(ws, npts, B * X * Y * Z))
        pool_ws_done(ws, npts, B * X * Y * Z)
        ctx.save_for_backward(dp, feat, g)
        ctx.cfg = (BN, D, H, W, C, npts // B, lo, B, X, Y, Z)
        return out.view(B, X, Y, Z, C).permute(0, 4, 1, 2, 3)

    @staticmethod
    def backward(ctx, dout):
        from ._lib import host_f32
        dp, feat, g = ctx.saved_tensors
        BN, D, H, W, C, ppb, lo, B, X, Y, Z = ctx.cfg
        dev = dp.device
        drows = dout.permute(0, 2, 3, 4, 1).reshape(-1, C).float().contiguous()
        d_depth = torch.empty_like(dp)
        d_feat = torch.empty_like(feat)
        call("coocc_lift_splat_bwd", ptr(drows), C, ptr(dp), ptr(feat), ptr(g), BN, D, H, W, C, ppb, host_f32(lo), B, X, Y, Z,
             ptr(d_depth), ptr(d_feat))
        d_img = torch.empty(BN, C, H, W, device=dev, dtype=_F32)
        call("coocc_ndhwc_to_ncdhw", ptr(d_feat), ptr(d_img), BN, C, H * W, C, 0)
        return None, d_depth, d_img, None


def lift_splat(vt, depth_prob, img_feat, geom_feats):
    return LiftSplatFn.apply(vt, depth_prob, img_feat, geom_feats)


class VoxelPoolFn(torch.autograd.Function):
    """voxel_pooling (ViewTransformerLSSVoxel.py:100-123) with the gradient of bev_pool_cuda.cu:61-84."""

    @staticmethod
    def forward(ctx, vt, geom_feats, x):
        out = vt.voxel_pooling(geom_feats, x)
        ctx.save_for_backward(geom_feats.reshape(-1, 3).float().contiguous())
        ctx.vt, ctx.shape = vt, tuple(x.shape)
        return out

    @staticmethod
    def backward(ctx, dout):
        from ._lib import host_f32
        (g,) = ctx.saved_tensors
        vt = ctx.vt
        B, N, D, H, W, C = ctx.shape
        X, Y, Z = (int(v) for v in vt.nx.tolist())
        drows = dout.permute(0, 2, 3, 4, 1).reshape(-1, C).float().contiguous()
        npts = B * N * D * H * W
        dx = torch.empty(npts, C, device=dout.device, dtype=_F32)
        lo = (vt.bx - vt.dx / 2.).tolist() + vt.dx.tolist()
        call("coocc_voxel_pool_bwd", ptr(drows), C, ptr(g), npts, npts // B, C, host_f32(lo), B, X, Y, Z, ptr(dx))
        return None, None, dx.view(B, N, D, H, W, C)


def voxel_pooling(vt, geom_feats, x):
    return VoxelPoolFn.apply(vt, geom_feats, x)


# ----------------------------------------------------------------------------- R2 render
class RenderNearestFn(torch.autograd.Function):
    """table [V,4] (sigma, rgb logits per voxel) -> composited maps [N,H,W,4] (coocc_ray.py:574-617)."""

    @staticmethod
    def forward(ctx, table, gemo, grid):
        from ._lib import host_f32
        from .render import RENDER_BOUNDS
        X, Y, Z = grid
        N, D, H, W, _ = gemo.shape
        zvals = torch.linspace(0, D, D, device=table.device)
        maps = torch.empty(N, H, W, 4, device=table.device, dtype=_F32)
        t = table.float().contiguous()
        call("coocc_render_nearest", ptr(t), X, Y, Z, ptr(gemo), ptr(zvals), N, D, H, W, host_f32(RENDER_BOUNDS), 0, ptr(maps))
        ctx.save_for_backward(t, gemo, zvals)
        ctx.grid = grid
        return maps

    @staticmethod
    def backward(ctx, dmaps):
        from ._lib import host_f32
        from .render import RENDER_BOUNDS
        t, gemo, zvals = ctx.saved_tensors
        X, Y, Z = ctx.grid
        N, D, H, W, _ = gemo.shape
        dtable = torch.empty_like(t)
        call("coocc_render_nearest_bwd", ptr(t), X, Y, Z, ptr(gemo), ptr(zvals), N, D, H, W, host_f32(RENDER_BOUNDS),
             ptr(dmaps.float().contiguous()), ptr(dtable))
        return dtable, None, None


class UpsampleMapsFn(torch.autograd.Function):
    """maps [N,H,W,4] -> (rgbs [N,sH,sW,3], depths [N,sH,sW]) (coocc_ray.py:619-625)."""

    @staticmethod
    def forward(ctx, maps, scale):
        N, H, W, _ = maps.shape
        rgbs = torch.empty(N, H * scale, W * scale, 3, device=maps.device, dtype=_F32)
        depths = torch.empty(N, H * scale, W * scale, device=maps.device, dtype=_F32)
        call("coocc_upsample_maps", ptr(maps.contiguous()), N, H, W, scale, ptr(rgbs), ptr(depths))
        ctx.cfg = (N, H, W, scale)
        return rgbs, depths

    @staticmethod
    def backward(ctx, drgbs, ddepths):
        N, H, W, scale = ctx.cfg
        dmaps = torch.empty(N, H, W, 4, device=drgbs.device if drgbs is not None else ddepths.device, dtype=_F32)
        call("coocc_upsample_maps_bwd", ptr(drgbs.float().contiguous()) if drgbs is not None else None,
             ptr(ddepths.float().contiguous()) if ddepths is not None else None, N, H, W, scale, ptr(dmaps))
        return dmaps, None


class RenderLossesFn(torch.autograd.Function):
    """-> tensor [2] = (loss_depth_render, loss_rgb) (coocc_ray.py:423-433)."""

    @staticmethod
    def forward(ctx, rgbs, depths, rgb_gt, depth_gt, D):
        out = torch.empty(3, device=rgbs.device, dtype=_F32)
        r, d = rgbs.contiguous(), depths.contiguous()
        rg, dg = rgb_gt.float().contiguous(), depth_gt.float().contiguous()
        ws = workspace(r.device)
        call("coocc_render_losses", ptr(r), ptr(d), ptr(rg), ptr(dg), d.numel(), int(D), ptr(out), ptr(ws), ws.numel() * 4)
        ctx.save_for_backward(r, d, rg, dg, out)
        ctx.D = int(D)
        return out[:2].clone()

    @staticmethod
    def backward(ctx, gl):
        r, d, rg, dg, out = ctx.saved_tensors
        drgbs, ddepths = torch.empty_like(r), torch.empty_like(d)
        call("coocc_render_losses_bwd", ptr(r), ptr(d), ptr(rg), ptr(dg), d.numel(), ctx.D, ptr(out), ptr(gl.float().contiguous()),
             ptr(drgbs), ptr(ddepths))
        return drgbs, ddepths, None, None, None


class OccLossFn(torch.autograd.Function):
    """-> tensor [4] = the unweighted (ce, sem_scal, geo_scal, lovasz) of OccHead.loss (co_occ_amd/losses.py) for logit rows [P,C]
    (unit column stride, row stride ld >= C, read in place).  ``labels``: uint8 [P], or with ``coords`` ([3,P] int64) the label volume
    [X,Y,Z] read at the coordinates.  The backward is ONE coocc_occ_loss_bwd call on the saved statistics and Lovasz weights."""

    @staticmethod
    def forward(ctx, rows, labels, coords, class_w, empty_idx):
        P, C = rows.shape
        ld = rows.stride(0) if P > 1 else C
        dev = rows.device
        out = torch.empty(4, device=dev, dtype=_F32)
        stats = torch.empty(208, device=dev, dtype=torch.float64)          # COOCC_OCC_LOSS_STATS
        lov_w = torch.empty(P, C, device=dev, dtype=_F32)
        ws = stream_buffer(dev, "s:occ_loss", (int(_lib.load().coocc_occ_loss_ws(P, C)) + 3) // 4)
        if coords is not None:
            row_labels, (VX, VY, VZ) = torch.empty(P, device=dev, dtype=torch.uint8), labels.shape
        else:
            row_labels, VX, VY, VZ = None, 0, 0, 0
        call("coocc_occ_loss_fwd", ptr(rows, _F32, strided=True), P, C, ld, ptr(labels, torch.uint8), ptr(coords, torch.int64), VX, VY, VZ,
             ptr(row_labels), ptr(class_w, _F32), int(empty_idx), ptr(out), ptr(stats), ptr(lov_w), ptr(ws), ws.numel() * 4)
        ctx.save_for_backward(rows, labels if row_labels is None else row_labels, class_w, stats, lov_w)
        ctx.cfg = (P, C, ld, int(empty_idx))
        return out

    @staticmethod
    def backward(ctx, gl):
        rows, row_labels, class_w, stats, lov_w = ctx.saved_tensors
        P, C, ld, empty_idx = ctx.cfg
        drows = torch.empty(P, C, device=rows.device, dtype=_F32)
        call("coocc_occ_loss_bwd", ptr(rows, _F32, strided=True), P, C, ld, ptr(row_labels), ptr(class_w), empty_idx, ptr(stats),
             ptr(lov_w), ptr(gl.float().contiguous()), ptr(drows), C)
        return drows, None, None, None, None


class DepthLossFn(torch.autograd.Function):
    """-> 0-dim tensor = ``weight * sum / max(1, n_fg)`` of ``ViewTransformerLiftSplatShootVoxel.get_depth_loss`` ('bce') for depth
    probabilities [B*N,D,h,w] (any strides / dtype: read as contiguous float32) against int32 ``labels`` [B*N,h,w] (0 = no
    foreground, 1..D = bin 0..D-1; ``losses.depth_labels_device``).  Two launches forward, ONE coocc_depth_bce_bwd call backward on the
    saved (sum, n_fg) pair; the gradient comes back in the input's shape and dtype."""

    @staticmethod
    def forward(ctx, preds, labels, weight):
        BN, D, h, w = preds.shape
        dev = preds.device
        p = preds.detach().float().contiguous()
        loss = torch.empty((), device=dev, dtype=_F32)
        stats = torch.empty(2, device=dev, dtype=torch.float64)             # COOCC_DEPTH_BCE_STATS
        ws = stream_buffer(dev, "s:depth_loss", (int(_lib.load().coocc_depth_bce_ws(BN * h * w, D)) + 3) // 4)
        call("coocc_depth_bce", ptr(p, _F32), ptr(labels, torch.int32), BN, D, h, w, float(weight), ptr(loss), ptr(stats), ptr(ws),
             ws.numel() * 4)
        ctx.save_for_backward(p, labels, stats)
        ctx.cfg = (BN, D, h, w, float(weight), preds.dtype)
        return loss

    @staticmethod
    def backward(ctx, gl):
        p, labels, stats = ctx.saved_tensors
        BN, D, h, w, weight, dtype = ctx.cfg
        dp = torch.empty(BN, D, h, w, device=p.device, dtype=_F32)
        call("coocc_depth_bce_bwd", ptr(p), ptr(labels), BN, D, h, w, weight, ptr(stats), ptr(gl.float().reshape(1).contiguous()), ptr(dp))
        return (dp if dtype == _F32 else dp.to(dtype)), None, None


def render_block_train(sigma_head, rgb_head, feats2d, grid, gemo, scale=16):
    """Differentiable render block: feats2d [X*Y*Z, C] rows -> (rgbs, depths).  The per-voxel heads run through
    ConvRowsFn (Linear+ReLU layers), so gradients reach the voxel features and both MLPs.  ``rgb_head=None``: the
    depth-only branch (coocc_ray.py:436-484) -- the colour columns of the table are zero and ``rgbs`` is meaningless."""
    def mlp(m, x):
        for l in m.hidden_layers:
            x = linear_rows(x, l.weight, l.bias, relu=True)
        return linear_rows(x, m.output_layer.weight, m.output_layer.bias, relu=False)
    sig = mlp(sigma_head, feats2d)                       # [V,1]
    rgb = mlp(rgb_head, feats2d) if rgb_head is not None else torch.zeros(sig.shape[0], 3, device=sig.device)   # [V,3]
    table = torch.cat([sig, rgb], 1)                     # plumbing: 16 B per voxel
    N, D, H, W = gemo.shape[-5:-1]
    maps = RenderNearestFn.apply(table, gemo.reshape(N, D, H, W, 3).float().contiguous(), tuple(grid))
    return UpsampleMapsFn.apply(maps, scale)


def render_losses(rgbs, depths, rgb_gt, depth_gt, D):
    out = RenderLossesFn.apply(rgbs, depths, rgb_gt, depth_gt, D)
    return dict(loss_depth_render=out[0], loss_rgb=out[1])


# ----------------------------------------------------------------------------- FPN top-down step
class UpsampleAddFn(torch.autograd.Function):
    """fine + trilinear(coarse -> fine size) on rows (fpn3d.py:88-92)."""

    @staticmethod
    def forward(ctx, coarse2d, fine2d, gc, gf):
        B, Xc, Yc, Zc = gc
        _, Xf, Yf, Zf = gf
        C = fine2d.shape[1]
        out = fine2d.clone()
        call("coocc_upsample_add_trilinear", ptr(coarse2d.contiguous()), ptr(out), B, C, Xc, Yc, Zc, Xf, Yf, Zf)
        ctx.cfg = (B, C, Xc, Yc, Zc, Xf, Yf, Zf)
        return out

    @staticmethod
    def backward(ctx, dout):
        B, C, Xc, Yc, Zc, Xf, Yf, Zf = ctx.cfg
        dout = dout.float().contiguous()
        dc = torch.empty(B * Xc * Yc * Zc, C, device=dout.device, dtype=_F32)
        call("coocc_upsample_trilinear_bwd", ptr(dout), ptr(dc), B, C, Xc, Yc, Zc, Xf, Yf, Zf, 0)
        return dc, dout, None, None


def upsample_add(coarse2d, fine2d, gc, gf):
    return UpsampleAddFn.apply(coarse2d, fine2d, tuple(gc), tuple(gf))


# ----------------------------------------------------------------------------- decoder trunk (C0 + C1 + C2)
def rows_from_ncdhw(x):
    """[B,C,X,Y,Z] -> ([B*X*Y*Z, C] contiguous rows, (B,X,Y,Z)); differentiable (torch permute / copy)."""
    B, C, X, Y, Z = x.shape
    return x.float().permute(0, 2, 3, 4, 1).reshape(B * X * Y * Z, C).contiguous(), (B, X, Y, Z)


def ncdhw_from_rows(rows, geom):
    B, X, Y, Z = geom
    return rows.view(B, X, Y, Z, rows.shape[1]).permute(0, 4, 1, 2, 3)


def conv_bn_rows(x2d, weight, geom, bn=None, bias=None, stride=1, pad=None, relu=True, res2d=None, sync=None, force_train=False):
    """Conv3d -> BatchNorm (+res) -> ReLU on rows with the norm layer's OWN mode: a BN in training mode (or any BN with
    ``force_train``) gets the convolution without epilogue and then ``norm_rows`` -- batch (or SyncBN all-reduced) statistics,
    running stats updated, as nn.BatchNorm3d / nn.SyncBatchNorm do under model.train() upstream; a BN in eval mode is folded into
    the GEMM epilogue (frozen statistics).  The kernel is ``weight.shape[2:]``; ``stride`` / ``pad`` as ``conv3d_rows`` takes them."""
    if bn is not None and (bn.training or force_train):
        y, g = conv3d_rows(x2d, weight, geom, bias=bias, bn=None, stride=stride, pad=pad, relu=False)
        return norm_rows(y, bn, relu=relu, res=res2d, sync=sync), g
    return conv3d_rows(x2d, weight, geom, bias=bias, bn=bn, stride=stride, pad=pad, relu=relu, res2d=res2d)


def _cm(x, geom, m, relu=True):
    """mmcv-style ConvModule (conv, bn) on rows."""
    return conv_bn_rows(x, m.conv.weight, geom, bias=m.conv.bias, bn=m.bn, relu=relu)


def con_enc_train(con_enc, x2d, geom):
    """bifuser_n.py:23-30: Sequential(Conv3d, BN, ReLU, Conv3d, BN, ReLU) on rows."""
    x2d, geom = conv_bn_rows(x2d, con_enc[0].weight, geom, bias=con_enc[0].bias, bn=con_enc[1], relu=True)
    return conv_bn_rows(x2d, con_enc[3].weight, geom, bias=con_enc[3].bias, bn=con_enc[4], relu=True)


def backbone_forward_train(backbone, x2d, geom):
    """CustomResNet3D (resnet3d.py:196-205) on rows -> [(rows, geom)] per out index."""
    x, g = conv_bn_rows(x2d, backbone.input_proj[0].weight, geom, bn=backbone.input_proj[1], relu=True)
    feats = []
    for i, layer in enumerate(backbone.layers):
        for blk in layer:
            out, go = conv_bn_rows(x, blk.conv1.weight, g, bn=blk.bn1, stride=blk.stride, relu=True)
            if blk.downsample is not None:
                res, _ = conv_bn_rows(x, blk.downsample[0].weight, g, bn=blk.downsample[1], stride=blk.stride, pad=0, relu=False)
            else:
                res = x
            x, g = conv_bn_rows(out, blk.conv2.weight, go, bn=blk.bn2, relu=True, res2d=res)
        if i in backbone.out_indices:
            feats.append((x, g))
    return feats


def neck_forward_train(neck, feats):
    """FPN3D (fpn3d.py:70-108) on [(rows, geom)]."""
    lat = [_cm(x, g, neck.lateral_convs[i][0]) for i, (x, g) in enumerate(feats)]
    for i in range(len(lat) - 1, 0, -1):
        (c, gc), (f, gf) = lat[i], lat[i - 1]
        lat[i - 1] = (upsample_add(c, f, gc, gf), gf)
    return [_cm(x, g, neck.fpn_convs[i][0]) for i, (x, g) in enumerate(lat)]


def trunk_forward_train(con_enc, backbone, neck, x2d, geom):
    """Differentiable con_enc -> CustomResNet3D -> FPN3D on rows (bifuser_n.py:23-30, resnet3d.py:196-205,
    fpn3d.py:70-108); every BN follows its own training flag (conv_bn_rows).  x2d: [B*X*Y*Z, 4C] fused rows.  Returns
    [(rows, geom)] per level.  The modules are the inference modules: parameters (and state_dict keys) are shared."""
    if con_enc is not None:
        x2d, geom = con_enc_train(con_enc, x2d, geom)
    feats = backbone_forward_train(backbone, x2d, geom)
    return feats if neck is None else neck_forward_train(neck, feats)


# ----------------------------------------------------------------------------- OccHead coarse mix (C3)
class OccHeadMixFn(torch.autograd.Function):
    """out[v] = sum_l softmax(wlogit[v])_l * trilinear(level_l -> level-0 size)[v]   (occ_head.py:155-166)."""

    @staticmethod
    def forward(ctx, wlogit, geoms, *levels):
        from ._lib import host_i32
        L = len(levels)
        B, X0, Y0, Z0 = geoms[0]
        C = levels[0].shape[1]
        lv = [t.contiguous() for t in levels]
        arr = (_lib.c_void_p * L)(*[t.data_ptr() for t in lv])
        dims = host_i32([v for g in geoms for v in g[1:]])
        out = torch.empty(B * X0 * Y0 * Z0, C, device=lv[0].device, dtype=_F32)
        wl = wlogit.contiguous() if wlogit is not None else None
        call("coocc_occhead_mix", arr, dims, L, ptr(wl), ptr(out), B, C)
        ctx.save_for_backward(*( [wl] if wl is not None else [] ), *lv)
        ctx.cfg = (geoms, wl is not None)
        return out

    @staticmethod
    def backward(ctx, dout):
        from ._lib import host_i32
        geoms, has_w = ctx.cfg
        saved = ctx.saved_tensors
        wl = saved[0] if has_w else None
        lv = saved[1:] if has_w else saved
        L = len(lv)
        B, X0, Y0, Z0 = geoms[0]
        C = lv[0].shape[1]
        dev = dout.device
        dout = dout.float().contiguous()
        V0 = B * X0 * Y0 * Z0
        g = [torch.empty(V0, C, device=dev, dtype=_F32) for _ in range(L)]
        dwl = torch.empty(V0, L, device=dev, dtype=_F32) if has_w else None
        arr = (_lib.c_void_p * L)(*[t.data_ptr() for t in lv])
        garr = (_lib.c_void_p * L)(*[t.data_ptr() for t in g])
        dims = host_i32([v for gg in geoms for v in gg[1:]])
        call("coocc_occhead_mix_bwd", arr, dims, L, ptr(wl), ptr(dout), garr, ptr(dwl), B, C)
        grads = [g[0]]
        for l in range(1, L):
            _, Xl, Yl, Zl = geoms[l]
            if (Xl, Yl, Zl) == (X0, Y0, Z0):
                grads.append(g[l])
                continue
            dl = torch.empty(B * Xl * Yl * Zl, C, device=dev, dtype=_F32)
            call("coocc_upsample_trilinear_bwd", ptr(g[l]), ptr(dl), B, C, Xl, Yl, Zl, X0, Y0, Z0, 0)
            grads.append(dl)
        return (dwl, None) + tuple(grads)


def occhead_coarse_train(head, feats):
    """Differentiable OccHead.forward_coarse_voxel on rows: feats = [(rows, geom)] per level (from
    trunk_forward_train) -> (out_voxel_feats rows, occupancy logits rows [V0, num_cls])."""
    occs = []
    for i, (x, g) in enumerate(feats):
        m = head.occ_convs[i]
        o, go = conv_bn_rows(x, m[0].weight, g, bias=m[0].bias, bn=m[1], relu=True)
        occs.append((o, go))
    wlogit = None
    g0 = occs[0][1]
    if head.soft_weights:
        sw = head.voxel_soft_weights
        h, _ = conv_bn_rows(occs[0][0], sw[0].weight, g0, bias=sw[0].bias, bn=sw[1], relu=True)
        wlogit, _ = conv_bn_rows(h, sw[3].weight, g0, bias=sw[3].bias, relu=False)
    out = OccHeadMixFn.apply(wlogit, tuple(g for _, g in occs), *[o for o, _ in occs])
    pc = head.occ_pred_conv
    h, _ = conv_bn_rows(out, pc[0].weight, g0, bias=pc[0].bias, bn=pc[1], relu=True)
    occ, _ = conv_bn_rows(h, pc[3].weight, g0, bias=pc[3].bias, relu=False)
    return out, occ


# ----------------------------------------------------------------------------- fine branch (C4)
class FineSampleVoxelFn(torch.autograd.Function):
    """Trilinear grid_sample of out_voxel_feats at the fine children of the selected coarse voxels (occ_head.py:205-214).
    vol2d [X*Y*Z, C] rows, coarse_lin int32 [n] -> (feat [r^3*n, C], fine_xyz int64 [3, r^3*n])."""

    @staticmethod
    def forward(ctx, vol2d, coarse_lin, geom, ratio, final_size):
        from ._lib import host_i32
        _, X, Y, Z = geom
        C = vol2d.shape[1]
        n = coarse_lin.numel()
        nf = n * ratio ** 3
        fine_xyz = torch.empty(3, nf, device=vol2d.device, dtype=torch.int64)
        feat = torch.empty(nf, C, device=vol2d.device, dtype=_F32)
        call("coocc_fine_sample_voxel", ptr(vol2d.contiguous()), C, X, Y, Z, ptr(coarse_lin), n, ratio, host_i32(final_size),
             ptr(fine_xyz), ptr(feat), C)
        ctx.save_for_backward(fine_xyz)
        ctx.cfg = (X, Y, Z, C, tuple(final_size))
        ctx.mark_non_differentiable(fine_xyz)
        return feat, fine_xyz

    @staticmethod
    def backward(ctx, dfeat, _):
        from ._lib import host_i32
        (fine_xyz,) = ctx.saved_tensors
        X, Y, Z, C, final_size = ctx.cfg
        dvol = torch.empty(X * Y * Z, C, device=dfeat.device, dtype=_F32)
        call("coocc_fine_sample_voxel_bwd", ptr(dfeat.float().contiguous()), C, C, X, Y, Z, ptr(fine_xyz), fine_xyz.shape[1],
             host_i32(final_size), ptr(dvol))
        return dvol, None, None, None, None


class GroupNormRowsFn(torch.autograd.Function):
    """nn.GroupNorm followed by ReLU, differentiable in x, gamma, beta: on rows [n, C], every row its own sample
    (occ_head.py:70-83), or with ``maps`` = (N, HW) over the N images of [N*HW, C] image rows (occ_head.py:64-68)."""

    @staticmethod
    def forward(ctx, x, gamma, beta, groups, eps, relu, maps=None):
        y = x.float().contiguous().clone()
        # the leading extents of the two entry points: (n, row stride C) | (N, HW)
        entry, lead = ("coocc_groupnorm_rows", (y.shape[0], y.shape[1])) if maps is None else ("coocc_groupnorm_nhwc", tuple(maps))
        call(entry, ptr(y), *lead, y.shape[1], groups, ptr(gamma.detach().float().contiguous()),
             ptr(beta.detach().float().contiguous()), float(eps), int(relu))
        ctx.save_for_backward(x.float().contiguous(), y, gamma.detach().float().contiguous())
        ctx.cfg = (entry + "_bwd", lead, groups, float(eps), int(relu))
        return y

    @staticmethod
    def backward(ctx, dy):
        x, y, gamma = ctx.saved_tensors
        entry, lead, groups, eps, relu = ctx.cfg
        C = x.shape[1]
        dx = torch.empty_like(x)
        dgamma = torch.empty(C, device=x.device, dtype=_F32)
        dbeta = torch.empty(C, device=x.device, dtype=_F32)
        call(entry, ptr(x), ptr(y), ptr(dy.float().contiguous()), *lead, C, groups, ptr(gamma), eps, relu, ptr(dx), ptr(dgamma),
             ptr(dbeta))
        return dx, dgamma, dbeta, None, None, None, None


class FineSampleImgFn(torch.autograd.Function):
    """Camera branch of C4: project fine points into the cameras and sum the bilinear samples of img rows
    [ncam*Hf*Wf, Ci] (occ_head.py:217-234); gradient w.r.t. the image features."""

    @staticmethod
    def forward(ctx, img_rows, params, fine_xyz, ncam, Hf, Wf, ratio):
        Ci = img_rows.shape[1]
        nf = fine_xyz.shape[1]
        samp = torch.empty(nf, Ci, device=img_rows.device, dtype=_F32)
        call("coocc_fine_sample_img", ptr(img_rows.contiguous()), ncam, Ci, Hf, Wf, ptr(params), ptr(fine_xyz), nf, ptr(samp), Ci,
             ratio if ratio in (2, 4) else 0)
        ctx.save_for_backward(params, fine_xyz)
        ctx.cfg = (ncam, Ci, Hf, Wf)
        return samp

    @staticmethod
    def backward(ctx, dsamp):
        params, fine_xyz = ctx.saved_tensors
        ncam, Ci, Hf, Wf = ctx.cfg
        dimg = torch.empty(ncam * Hf * Wf, Ci, device=dsamp.device, dtype=_F32)
        call("coocc_fine_sample_img_bwd", ptr(dsamp.float().contiguous()), Ci, ncam, Ci, Hf, Wf, ptr(params), ptr(fine_xyz),
             fine_xyz.shape[1], ptr(dimg))
        return dimg, None, None, None, None, None, None


def fine_branch_train(head, out_voxel_rows, geom, coarse_lin, img_feats=None, transform=None):
    """Differentiable fine branch (occ_head.py:180-237): the selected coarse voxels' children sample out_voxel_feats
    trilinearly and, with sample_from_img, the image features through the cameras; fine_mlp = Linear -> GroupNorm ->
    ReLU -> Linear.  The selection itself (argmax != empty, or the training-time random top-k) is an index and not
    differentiated.  img_feats: [[1,N,Cimg,Hf,Wf]] (a leaf may require grad); transform: img_inputs[1:]."""
    r = head.cascade_ratio
    feat, fine_xyz = FineSampleVoxelFn.apply(out_voxel_rows, coarse_lin, tuple(geom), r,
                                             tuple(int(v) for v in head.final_occ_size))
    parts = [feat] if head.sample_from_voxel else []
    if head.sample_from_img and img_feats is not None:
        f = img_feats[0]
        _, N_i, C_i, Hf, Wf = f.shape
        rows = f[0].permute(0, 2, 3, 1).reshape(N_i * Hf * Wf, C_i)            # NHWC rows (a view + copy: plumbing)
        m0 = head.img_mlp_0
        g = linear_rows(rows, m0[0].weight.flatten(1), m0[0].bias, relu=False)
        g = GroupNormRowsFn.apply(g, m0[1].weight, m0[1].bias, m0[1].num_groups, m0[1].eps, True, (N_i, Hf * Wf))

        class _G:       # geometry holder for the parameter block
            X, Y, Z = geom[1], geom[2], geom[3]
        params = head._projection_params(transform, _G, out_voxel_rows.device)
        samp = FineSampleImgFn.apply(g, params, fine_xyz, N_i, Hf, Wf, r)
        m1 = head.img_mlp
        s_ = linear_rows(samp, m1[0].weight, m1[0].bias, relu=False)
        parts.append(GroupNormRowsFn.apply(s_, m1[1].weight, m1[1].bias, m1[1].num_groups, m1[1].eps, True))
    x = parts[0] if len(parts) == 1 else torch.cat(parts, 1)
    h = linear_rows(x, head.fine_mlp[0].weight, head.fine_mlp[0].bias, relu=False)
    gn = head.fine_mlp[1]
    h = GroupNormRowsFn.apply(h, gn.weight, gn.bias, gn.num_groups, gn.eps, True)
    return linear_rows(h, head.fine_mlp[3].weight, head.fine_mlp[3].bias, relu=False), fine_xyz


# ----------------------------------------------------------------------------- BatchNorm with batch statistics
def _sync_group(bn, sync):
    """The process group a training-mode BN synchronises over, or None.  sync=None: follow the module type
    (nn.SyncBatchNorm, what norm_cfg type='SyncBN' builds upstream) whenever torch.distributed is initialised."""
    import torch.distributed as dist
    if sync is None:
        sync = isinstance(bn, torch.nn.SyncBatchNorm)
    if not sync or not (dist.is_available() and dist.is_initialized()) or dist.get_world_size() == 1:
        return None
    return getattr(bn, "process_group", None) or dist.group.WORLD


class BatchNormRowsFn(torch.autograd.Function):
    """Training-mode BatchNorm3d / SyncBN on rows [M, C] (+ residual, ReLU): batch mean / biased variance, running
    statistics updated in place like torch (momentum, unbiased variance).  With a process group the statistics are
    those of all ranks' rows (one all-reduce of 2C+1 floats in the forward, one of 2C in the backward, as
    torch.nn.SyncBatchNorm does); the returned dgamma / dbeta are this rank's share, which DDP then reduces.
    ``out_h2``: optional [M, C] fp32-sized buffer (C % 32 == 0) the apply pass fills with the split-f16 twin of y
    (coocc_bn_apply_ex: the operand of a following split-f16 GEMM, no coocc_rows_to_h2 launch)."""

    @staticmethod
    def forward(ctx, x, gamma, beta, res, bn, relu, group=None, out_h2=None):
        x = x.float().contiguous()
        M, C = x.shape
        dev = x.device
        mean = torch.empty(C, device=dev, dtype=_F32)
        var = torch.empty(C, device=dev, dtype=_F32)
        ws = workspace(dev)
        call("coocc_bn_stats", ptr(x), C, M, C, ptr(mean), ptr(var), ptr(ws), ws.numel() * 4)
        count = float(M)
        if group is not None:
            import torch.distributed as dist
            m64 = mean.double()
            pack = torch.cat([m64 * M, (var.double() + m64 * m64) * M, torch.tensor([float(M)], device=dev, dtype=torch.float64)])
            dist.all_reduce(pack, group=group)
            count = float(pack[-1].item())
            gm = pack[:C] / count
            mean = gm.float()
            var = (pack[C:2 * C] / count - gm * gm).clamp_(min=0).float()
        y = torch.empty_like(x)
        g, b = gamma.detach().float().contiguous(), beta.detach().float().contiguous()
        if out_h2 is not None:
            call("coocc_bn_apply_ex", ptr(x), M, C, ptr(mean), ptr(var), ptr(g), ptr(b), float(bn.eps),
                 ptr(res.float().contiguous()) if res is not None else None, int(relu), ptr(y), ptr(out_h2))
        else:
            call("coocc_bn_apply", ptr(x), M, C, ptr(mean), ptr(var), ptr(g), ptr(b), float(bn.eps),
                 ptr(res.float().contiguous()) if res is not None else None, int(relu), ptr(y))
        if bn.track_running_stats and bn.running_mean is not None:
            with torch.no_grad():
                bn.num_batches_tracked += 1          # torch increments first; momentum=None = cumulative moving average
                mom = bn.momentum if bn.momentum is not None else 1.0 / float(bn.num_batches_tracked)
                bn.running_mean.mul_(1 - mom).add_(mean, alpha=mom)
                bn.running_var.mul_(1 - mom).add_(var * (count / max(count - 1, 1)), alpha=mom)
        ctx.save_for_backward(x, y, mean, var, g)
        ctx.cfg = (float(bn.eps), int(relu), res is not None, group, count)
        return y

    @staticmethod
    def backward(ctx, dy):
        x, y, mean, var, g = ctx.saved_tensors
        eps, relu, has_res, group, count = ctx.cfg
        M, C = x.shape
        dev = x.device
        dy = dy.float().contiguous()
        dx = torch.empty_like(x)
        dres = torch.empty_like(x) if has_res else None
        sums = torch.empty(2, C, device=dev, dtype=_F32)        # [dgamma | dbeta] of this rank's rows
        ws = workspace(dev)
        call("coocc_bn_backward_sums", ptr(x), ptr(y), ptr(dy), M, C, ptr(mean), ptr(var), eps, relu, ptr(sums[0]), ptr(sums[1]),
             ptr(ws), ws.numel() * 4)
        tot = sums
        if group is not None:
            import torch.distributed as dist
            tot = sums.clone()
            dist.all_reduce(tot, group=group)
        call("coocc_bn_backward_dx", ptr(x), ptr(y), ptr(dy), M, C, ptr(mean), ptr(var), ptr(g), eps, relu, ptr(tot[0]), ptr(tot[1]),
             float(count), ptr(dx), ptr(dres))
        return dx, sums[0], sums[1], dres, None, None, None, None


def norm_rows(y, bn, relu=True, res=None, sync=None, out_h2=None):
    """``bn`` in training mode on rows (+ res) (+ ReLU): ``BatchNormRowsFn`` with the layer's own parameters and the process group
    ``_sync_group`` finds for it; ``out_h2`` as the Function takes it."""
    return BatchNormRowsFn.apply(y, bn.weight, bn.bias, res, bn, relu, _sync_group(bn, sync), out_h2)


def conv3d_bn_train_rows(x2d, weight, geom, bn, **kw):
    """``conv_bn_rows`` with batch statistics whatever the norm layer's mode.  Use conv3d_rows(bn=...) for frozen statistics."""
    return conv_bn_rows(x2d, weight, geom, bn=bn, force_train=True, **kw)


# ----------------------------------------------------------------------------- LiDAR-only trunk (SECOND3D + SECOND3DFPN)
# Training of lidar_trunk's modules.  The anisotropic layers (3x3x1 kernels, strides (s, s, 1), pads (1, 1, 0)) are ConvRowsFn
# layers like any other: coocc_conv_fwd through the descriptor's per-axis fields, the same launch with flipped weights for the
# stride-1 dgrad, row-table launches per residue class for the strided one, coocc_conv_wgrad over the live taps.
class FpnSumFn(torch.autograd.Function):
    """``lidar_trunk.fpn_sum`` on 2-D tensors: ups[l] [B*(X/s)*(Y/s)*Z, s*s*C] (child-major deblock outputs) -> [B*X*Y*Z, C].  The
    backward re-lays dout into every level's own layout (coocc_fpn_sum_bwd); a stride-1 level's gradient is dout itself."""

    @staticmethod
    def forward(ctx, geom, strides, C, *ups):
        import ctypes
        B, X, Y, Z = geom
        ups = [u.float().contiguous() for u in ups]
        for u, s in zip(ups, strides):
            assert u.shape == (B * (X // s) * (Y // s) * Z, s * s * C) and X % s == 0 and Y % s == 0, "level sizes differ after upsampling"
        out = torch.empty(B * X * Y * Z, C, device=ups[0].device, dtype=_F32)
        pp = (ctypes.c_void_p * 4)(*[u.data_ptr() for u in ups])
        ss = (ctypes.c_int * 4)(*strides)
        with _lib.TIMER.region("k_fpn_sum", 4.0 * out.numel() * (len(ups) + 1)):
            call("coocc_fpn_sum", pp, ss, len(ups), B, X, Y, Z, C, ptr(out), C, None)
        ctx.cfg = (geom, tuple(strides), C)
        return out

    @staticmethod
    def backward(ctx, dout):
        import ctypes
        (B, X, Y, Z), strides, C = ctx.cfg
        dout = dout.float().contiguous()
        need = ctx.needs_input_grad[3:]
        grads = [None if (s == 1 or not n) else torch.empty(B * (X // s) * (Y // s) * Z, s * s * C, device=dout.device, dtype=_F32)
                 for s, n in zip(strides, need)]
        if any(g is not None for g in grads):
            pp = (ctypes.c_void_p * 4)(*[g.data_ptr() if g is not None else None for g in grads])
            ss = (ctypes.c_int * 4)(*strides)
            with _lib.TIMER.region("k_fpn_sum_bwd", 4.0 * dout.numel() * (1 + sum(g is not None for g in grads))):
                call("coocc_fpn_sum_bwd", ptr(dout), C, pp, ss, len(strides), B, X, Y, Z, C)
        return (None, None, None) + tuple(dout if (s == 1 and n) else g for s, n, g in zip(strides, need, grads))


def fpn_sum_rows(ups, strides, C, geom):
    return FpnSumFn.apply(tuple(geom), tuple(int(s) for s in strides), int(C), *ups)


def deconv_bn_rows(x2d, up, bn, s, relu=True, sync=None):
    """A deconvolution deblock with kernel = stride -- nn.ConvTranspose3d((1,s,s)) -> BN3d -> ReLU of SECOND3DFPN
    (second3d_fpn.py:47-69), or nn.ConvTranspose2d(s) -> BN2d -> ReLU of SECONDFPN (second_fpn.py:44-65) -- on the COARSE rows
    [M, Cin] -> [M, s*s*Cout] (child (kx, ky) of a coarse voxel, (kh, kw) of a coarse pixel, at columns (kx*s + ky)*Cout ..): the
    pointwise GEMM with ``core.deconv_weight``'s layout taken as a differentiable view of the parameter (so the weight gradient
    lands in the module's own tensor), then the norm layer in its own mode.  One BN channel serves the s*s children, so batch
    statistics over the [M*s*s, Cout] view of the GEMM's output are those of the upsampled volume; a BN in eval mode is folded into
    the GEMM's epilogue with its scale / shift repeated s*s times."""
    w = deconv_weight(up.weight, s, detach=False)
    cout = up.weight.shape[1]
    b = up.bias.repeat(s * s) if up.bias is not None else None
    n = x2d.shape[0]
    if bn is not None and bn.training:
        y = linear_rows(x2d, w, b, relu=False)
        return norm_rows(y.view(n * s * s, cout), bn, relu=relu, sync=sync).view(n, s * s * cout)
    scale, shift = folded_bn(bn, x2d.device, repeat=s * s) if bn is not None else (None, None)
    return ConvRowsFn.apply(x2d.contiguous(), w, b, None, scale, shift, (1, n, 1, 1), _UNIT, _UNIT, _NOPAD, relu)


class ZyxRowsFn(torch.autograd.Function):
    """The trunk's entry transposition [B,C,Z,Y,X] -> rows in (b, x, y, z) order (coocc_zyx_to_rows) with its gradient: the
    permuted view of the row gradient, no kernel."""

    @staticmethod
    def forward(ctx, x):
        from .lidar_trunk import bczyx_to_rows
        r = bczyx_to_rows(x.detach())
        ctx.cfg = (r.B, r.X, r.Y, r.Z, r.C)
        t = r.dense2d()
        return t.clone() if t.data_ptr() == x.data_ptr() else t      # channels-last memory: a view of the input itself

    @staticmethod
    def backward(ctx, drows):
        B, X, Y, Z, C = ctx.cfg
        return drows.view(B, X, Y, Z, C).permute(0, 4, 3, 2, 1)


def _zyx(w):
    """A reference conv weight [N,C,kz,ky,kx] in the [N,C,kx,ky,kz] order this package's taps read (``core.zyx_weight`` without the
    detach: the gradient flows back to the parameter)."""
    return w.permute(0, 1, 4, 3, 2).contiguous()


def second3d_forward_train(backbone, x2d, geom):
    """SECOND3D (second3d.py:91-114) on rows -> [(rows, geom)] per block; the inference module's own parameters."""
    outs = []
    for i, blk in enumerate(backbone.blocks):
        s = backbone.layer_strides[i]
        h, g = x2d, geom
        for j in range(0, len(blk), 3):
            st = (s, s, 1) if j == 0 else (1, 1, 1)
            h, g = conv_bn_rows(h, _zyx(blk[j].weight), g, bn=blk[j + 1], bias=blk[j].bias, stride=st, pad=blk[j].padding[::-1], relu=True)
        outs.append((h, g))
        if backbone.is_cascade:
            x2d, geom = h, g
    return outs


def second3dfpn_forward_train(neck, feats):
    """SECOND3DFPN (second3d_fpn.py:108-143) on [(rows, geom)] -> (rows, geom)."""
    from torch import nn
    assert len(feats) == len(neck.in_channels)
    C = neck.out_channels[-1]
    ups, fine = [], None
    for (x, g), s, blk in zip(feats, neck.upsample_strides, neck.deblocks):
        up, bn = blk[0], blk[1]
        if isinstance(up, nn.ConvTranspose3d):
            ups.append(deconv_bn_rows(x, up, bn, s))
        else:
            ups.append(conv_bn_rows(x, up.weight, g, bn=bn, bias=up.bias, relu=True)[0])
        gf = (g[0], g[1] * s, g[2] * s, g[3])
        if fine is not None and gf != fine:
            raise ValueError("SECOND3DFPN: level sizes differ after upsampling (%s vs %s)" % (gf[1:], fine[1:]))
        fine = gf
    if len(ups) == 1 and neck.upsample_strides[0] == 1:
        out = ups[0]                                                            # second3d_fpn.py:123-124
    else:
        out = fpn_sum_rows(ups, neck.upsample_strides, C, fine)
    if neck.extra_conv is not None:
        for j in range(0, len(neck.extra_blocks), 3):
            c, bn = neck.extra_blocks[j], neck.extra_blocks[j + 1]
            out, fine = conv_bn_rows(out, _zyx(c.weight), fine, bn=bn, bias=c.bias, pad=c.padding[::-1], relu=True)
    return out, fine


# ----------------------------------------------------------------------------- image encoder (ResNet stem, SECONDFPN deblocks)
# Training of image_encoder's modules.  Every Bottleneck layer and the neck's convolutions are ConvRowsFn layers on rows
# [BN*H*W, C] (X = H, Y = W, Z = 1); what the engine lacked is the stem (csrc/img_stem_train.hip).
class StemConvFn(torch.autograd.Function):
    """y = relu(scale * conv7x7/2(img, W) + shift) of the fp32 NCHW image [BN,3,H,W] -> rows [BN*Hc*Wc, 64] (k_img_stem without the
    pool); weight [64,3,7,7]; scale / shift constants (a folded eval-mode BN) or None.  Differentiable in W (coocc_img_stem_wgrad);
    the image gets no gradient."""

    @staticmethod
    def forward(ctx, img, weight, scale, shift, relu):
        if ctx.needs_input_grad[0] or img.requires_grad:
            raise NotImplementedError("StemConvFn: a gradient with respect to the image is not built")
        img = img.detach().float().contiguous()
        BN, _, H, W = img.shape
        C0 = weight.shape[0]
        assert tuple(weight.shape[1:]) == (3, 7, 7)
        dev = img.device
        w = weight.detach().float().permute(1, 2, 3, 0).reshape(147, C0).contiguous()
        sc = scale if scale is not None else torch.ones(C0, device=dev, dtype=_F32)
        sh = shift if shift is not None else torch.zeros(C0, device=dev, dtype=_F32)
        Hc, Wc = (H - 1) // 2 + 1, (W - 1) // 2 + 1
        out = torch.empty(BN * Hc * Wc, C0, device=dev, dtype=_F32)
        with _lib.TIMER.region("k_img_stem", 2.0 * out.shape[0] * C0 * 147):
            call("coocc_img_stem", ptr(img), BN, H, W, ptr(w), ptr(sc), ptr(sh), C0, int(relu), 0, ptr(out), C0, None)
        ctx.save_for_backward(img, out, scale if scale is not None else torch.empty(0, device=dev))
        ctx.cfg = (scale is not None, bool(relu), tuple(weight.shape))
        return out

    @staticmethod
    def backward(ctx, dout):
        img, out, scale = ctx.saved_tensors
        has_scale, relu, wshape = ctx.cfg
        if not ctx.needs_input_grad[1]:
            return None, None, None, None, None
        BN, _, H, W = img.shape
        C0 = wshape[0]
        dev = img.device
        dacc = dout.float().contiguous()
        if has_scale or relu:
            dacc = epilogue_bwd(dacc, out, scale if has_scale else None, relu)[0]
        dw = torch.empty(147, C0, device=dev, dtype=_F32)
        nb = int(_lib.load().coocc_img_stem_wgrad_ws(BN, H, W))
        part = stream_buffer(dev, "s:stem_wgrad", (nb + 3) // 4)
        with _lib.TIMER.region("k_img_stem_wgrad", 2.0 * out.shape[0] * C0 * 147):
            call("coocc_img_stem_wgrad", ptr(img), BN, H, W, ptr(dacc), C0, C0, ptr(dw), ptr(part), part.numel() * 4)
        return None, dw.view(3, 7, 7, C0).permute(3, 0, 1, 2), None, None, None


def stem_conv_bn_rows(img, conv, bn, relu=True, sync=None):
    """The ResNet stem's Conv2d(3, 64, 7, 2, 3) -> BN -> ReLU on rows with the norm layer's own mode (as ``conv_bn_rows``) ->
    (rows [BN*Hc*Wc, 64], (BN, Hc, Wc, 1))."""
    BN, _, H, W = img.shape
    geom = (BN, (H - 1) // 2 + 1, (W - 1) // 2 + 1, 1)
    if bn.training:
        return norm_rows(StemConvFn.apply(img, conv.weight, None, None, False), bn, relu=relu, sync=sync), geom
    return StemConvFn.apply(img, conv.weight, *folded_bn(bn, img.device, conv.bias), relu), geom


class MaxPoolRowsFn(torch.autograd.Function):
    """MaxPool2d(3, 2, 1) on rows [BN*Hc*Wc, C] -> [BN*Hp*Wp, C] (coocc_maxpool2d_rows).  No index tensor is kept: the backward
    recomputes every window's first maximum from the pre-pool rows, which their producer (the BN / ReLU pass) saves anyway."""

    @staticmethod
    def forward(ctx, x2d, geom):
        BN, Hc, Wc = geom
        x2d = x2d.float().contiguous()
        C = x2d.shape[1]
        assert x2d.shape[0] == BN * Hc * Wc and C % 4 == 0
        Hp, Wp = (Hc - 1) // 2 + 1, (Wc - 1) // 2 + 1
        out = torch.empty(BN * Hp * Wp, C, device=x2d.device, dtype=_F32)
        with _lib.TIMER.region("k_maxpool2d_rows", 9.0 * out.numel()):
            call("coocc_maxpool2d_rows", ptr(x2d), C, BN, Hc, Wc, C, ptr(out), C, None)
        ctx.save_for_backward(x2d)
        ctx.cfg = (BN, Hc, Wc)
        return out

    @staticmethod
    def backward(ctx, dout):
        (x2d,) = ctx.saved_tensors
        BN, Hc, Wc = ctx.cfg
        C = x2d.shape[1]
        dout = dout.float().contiguous()
        dx = torch.empty_like(x2d)
        with _lib.TIMER.region("k_maxpool2d_rows_bwd", 36.0 * dx.numel()):
            call("coocc_maxpool2d_rows_bwd", ptr(x2d), C, ptr(dout), C, BN, Hc, Wc, C, ptr(dx), C)
        return dx, None


def maxpool_rows(x2d, geom):
    """-> (pooled rows, (BN, Hp, Wp, 1)) of rows with geom (BN, Hc, Wc, 1)."""
    BN, Hc, Wc = geom[:3]
    return MaxPoolRowsFn.apply(x2d, (BN, Hc, Wc)), (BN, (Hc - 1) // 2 + 1, (Wc - 1) // 2 + 1, 1)
