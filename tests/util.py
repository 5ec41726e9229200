"""Shared tolerance rule for float parity: BASELINE.json asks for "within 1e-4 fp32".  With
seeded random weights the decoder's activations reach |x| ~ 1e2, where one fp32 ulp is already
8e-6 and two CPU runs of the same torch graph with different thread counts differ by 5e-4
(measured), so the bound is applied relative to the tensor's scale:
    max|a - b| <= tol * max(1, max|b|),   tol = 1e-4.
Integer / index outputs are always compared bit-exactly."""
import contextlib
import os

import numpy as np
import torch

TOL = 1e-4


def to_np(a):
    if torch.is_tensor(a):
        return a.detach().float().cpu().numpy()
    return np.asarray(a)


def rel_err(a, b):
    a, b = to_np(a).astype(np.float64), to_np(b).astype(np.float64)
    assert a.shape == b.shape, "shape %s vs %s" % (a.shape, b.shape)
    if a.size == 0:
        return 0.0
    return float(np.abs(a - b).max() / max(1.0, np.abs(b).max()))


def assert_close(a, b, tol=TOL, what=""):
    e = rel_err(a, b)
    if os.environ.get("COOCC_PRINT_ERR"):
        print("[err] %-28s %.3e" % (what, e))
    assert e <= tol, "%s scale-relative error %.3e > %.1e" % (what, e, tol)
    return e


# ------------------------------------------------------------------ the high-precision judge
# ``assert_close`` bounds the error by 1e-4 of max(1, scale): 100-1000x looser than the split-f16 engine's precision, and an
# absolute 1e-4 for small outputs.  ``assert_precise`` judges a kernel against float64 at the kernel's OWN precision:
#     e_max = max|out - ref64| / max|ref64|          e_rms = rms(out - ref64) / rms(ref64)      (no floor at 1)
#     e_max <= C_MAX * max(e32_max, esplit_max, 2^-24)          e_rms <= C_RMS * max(e32_rms, esplit_rms, 2^-24)
# e32: the plain fp32 CPU evaluation of the same operation (the fp32 noise floor); esplit: the same operation with its operands
# split the engine's way (csrc/gemm_h2.hip: hi = f16(a), lo = f16((a - hi) 2^11), the three kept terms, fp64 products and sums,
# the result rounded to fp32) -- the anchor at short K, where the dropped lo*lo term (2^-22 per product) is not below the fp32
# accumulation error.  An all-zero reference demands exact zeros.
C_MAX, C_RMS = 4.0, 2.0
FLOOR = 2.0 ** -24
H2_LO = 2048.0


def _f64(a):
    if torch.is_tensor(a):
        return a.detach().to("cpu", torch.float64)
    return torch.as_tensor(np.asarray(a), dtype=torch.float64)


def errors(out, ref64):
    """(e_max, e_rms) of ``out`` against ``ref64``, each relative to the reference's own scale."""
    o, r = _f64(out), _f64(ref64)
    assert o.shape == r.shape, "shape %s vs %s" % (tuple(o.shape), tuple(r.shape))
    scale = float(r.abs().max()) if r.numel() else 0.0
    if scale == 0.0:
        return (0.0, 0.0) if not r.numel() or float(o.abs().max()) == 0.0 else (float("inf"), float("inf"))
    d = o - r
    return float(d.abs().max()) / scale, float(d.pow(2).mean().sqrt() / r.pow(2).mean().sqrt())


def precision(out, ref64, ref32=None, refsplit=None, anchor=None, out_ulp=0.0, c_max=C_MAX, c_rms=C_RMS, what=""):
    """The judge's numbers for one output (no assertion): dict(e_max, e_rms, a_max, a_rms, ratio_max, ratio_rms, ok).
    ``anchor``: (e_max, e_rms) to use instead of ref32's (the Winograd fp32 emulation); ``out_ulp``: the relative rounding of
    a narrower output type, added to the budget outside the constants."""
    e_max, e_rms = errors(out, ref64)
    e32 = anchor if anchor is not None else (errors(ref32, ref64) if ref32 is not None else (0.0, 0.0))
    es = errors(refsplit, ref64) if refsplit is not None else (0.0, 0.0)
    a_max, a_rms = max(e32[0], es[0], FLOOR), max(e32[1], es[1], FLOOR)
    b_max, b_rms = c_max * a_max + out_ulp, c_rms * a_rms + out_ulp
    st = dict(what=what, e_max=e_max, e_rms=e_rms, e32_max=e32[0], e32_rms=e32[1], es_max=es[0], es_rms=es[1], a_max=a_max,
              a_rms=a_rms, ratio_max=e_max / b_max * c_max, ratio_rms=e_rms / b_rms * c_rms,
              ok=bool(e_max <= b_max and e_rms <= b_rms))
    line = ("[prec] %-44s e_max %.2e e_rms %.2e | e32 %.2e/%.2e esplit %.2e/%.2e | ratio %.2f/%.2f (<= %g/%g)%s" % (
        what, e_max, e_rms, e32[0], e32[1], es[0], es[1], st["ratio_max"], st["ratio_rms"], c_max, c_rms, "" if st["ok"] else "  MISS"))
    print(line)
    log = os.environ.get("COOCC_PREC_LOG")
    if log:
        import json
        with open(log, "a") as f:
            f.write(json.dumps(st) + "\n")
    return st


def assert_precise(out, ref64, ref32=None, refsplit=None, **kw):
    st = precision(out, ref64, ref32, refsplit, **kw)
    assert st["ok"], ("%s: e_max %.3e (%.2f x anchor %.2e), e_rms %.3e (%.2f x anchor %.2e) against float64 -- over the budget "
                      "C_MAX = %g, C_RMS = %g" % (st["what"], st["e_max"], st["ratio_max"], st["a_max"], st["e_rms"], st["ratio_rms"],
                                                  st["a_rms"], kw.get("c_max", C_MAX), kw.get("c_rms", C_RMS)))
    return st


def h2_split(a):
    """The engine's operand split of fp32 values (csrc/h2_rows.h split_h2): float64 (hi, lo), a = hi + lo 2^-11 + O(2^-22 a)."""
    a = _f64(a)
    hi = a.to(torch.float16).double()
    return hi, ((a - hi) * H2_LO).to(torch.float16).double()


def split_mm(a, b):
    """a @ b with both operands split and the three leading terms kept, in float64 (ah bh + 2^-11 (ah bl + al bh))."""
    ah, al = h2_split(a)
    bh, bl = h2_split(b)
    return ah @ bh + (ah @ bl + al @ bh) / H2_LO


def epilogue(acc, scale=None, bias=None, res=None, relu=False, gate=None):
    """The conv epilogue in acc's precision: acc * scale + bias (+ residual), ReLU, * gate (csrc/gemm_h2.hip h2_epilogue_vec)."""
    dt = acc.dtype
    if scale is not None:
        acc = acc * _f64(scale).to(dt)
    if bias is not None:
        acc = acc + _f64(bias).to(dt)
    if res is not None:
        acc = acc + _f64(res).to(dt)
    if relu:
        acc = torch.relu(acc)
    if gate is not None:
        acc = acc * _f64(gate).to(dt)
    return acc


def gemm_refs(pairs, round_to=None, split=True, chain=0, **epi):
    """float64 / fp32 / split-f16 evaluations of  epi(sum_t A_t @ W_t)  for [(A_t [M, K], W_t [K, N]), ...] (the taps of a
    convolution, the slots of a gather GEMM).  ``round_to``: operands first rounded to that type (f16 / bf16 layers), exactly as
    the kernel sees them.  ``chain``: the fp32 evaluation is a sequential chain of K steps of ``chain`` products each (the
    accumulation order of the exact-fp32 MFMA kernels, v_mfma_f32_32x32x2_f32: chain = 2) instead of one blocked CPU GEMM per
    pair, whose error is below such a chain's.  Returns (ref64, ref32, refsplit or None), [M, N]."""
    acc64 = acc32 = accs = None
    for a, w in pairs:
        a, w = _f64(a), _f64(w)
        if round_to is not None:
            a, w = a.to(round_to).double(), w.to(round_to).double()
        p64 = a @ w
        acc64 = p64 if acc64 is None else acc64 + p64
        if chain:
            a32, w32 = a.float(), w.float()
            if acc32 is None:
                acc32 = torch.zeros(p64.shape, dtype=torch.float32)
            for k in range(0, a.shape[1], chain):
                acc32 = acc32 + a32[:, k:k + chain] @ w32[k:k + chain]
        else:
            p32 = a.float() @ w.float()
            acc32 = p32 if acc32 is None else acc32 + p32
        if split:
            ps = split_mm(a, w)
            accs = ps if accs is None else accs + ps
    e32 = {k: (_f64(v).float() if torch.is_tensor(v) else v) for k, v in epi.items()}
    refsplit = epilogue(accs.float().double(), **epi).float() if split else None
    return epilogue(acc64, **epi), epilogue(acc32, **e32), refsplit


def conv_taps(x, w, stride=1, pad=None, z_taps=None):
    """Taps of a 3-D convolution as GEMM operand pairs: x [B, C, X, Y, Z], w [N, C, kx, ky, kz] ->
    [(rows of tap t [B*Xo*Yo*Zo, C] in (b, x, y, z) order, W_t [C, N]), ...]."""
    kx, ky, kz = w.shape[2:]
    pad = (kx // 2) if pad is None else pad
    xp = torch.nn.functional.pad(_f64(x), (pad,) * 6)
    B, C = x.shape[:2]
    Xo, Yo, Zo = ((n + 2 * pad - k) // stride + 1 for n, k in zip(x.shape[2:], (kx, ky, kz)))
    out = []
    for a in range(kx):
        for b in range(ky):
            for c in range(kz):
                s = xp[:, :, a:a + stride * (Xo - 1) + 1:stride, b:b + stride * (Yo - 1) + 1:stride, c:c + stride * (Zo - 1) + 1:stride]
                out.append((s.permute(0, 2, 3, 4, 1).reshape(-1, C), _f64(w[:, :, a, b, c]).t()))
    return out


def ncdhw_rows(t):
    """[B, C, X, Y, Z] -> channels-last rows [B*X*Y*Z, C] (the kernels' output layout)."""
    return t.permute(0, 2, 3, 4, 1).reshape(-1, t.shape[1])


# Winograd F(m x m, 3x3) over (x, y), direct z taps (csrc/winograd.hip Wino<m + 2>): the transform matrices of the kernels
WINO_BT = {
    2: [[1, 0, -1, 0], [0, 1, 1, 0], [0, -1, 1, 0], [0, 1, 0, -1]],
    3: [[1, -1.5, -1.5, 1, 0], [0, 1, -2.5, 1, 0], [0, -0.5, 0.5, 1, 0], [0, -2, -1, 1, 0], [0, 1, -1.5, -1.5, 1]],
    4: [[1, -1.5, -2, 1.5, 1, 0], [0, -1, 0.5, 2.5, 1, 0], [0, 1, -2.5, 0.5, 1, 0], [0, -2, -1, 2, 1, 0], [0, 0.5, -1, -0.5, 1, 0],
        [0, 1, -1.5, -2, 1.5, 1]],
}
WINO_AT = {
    2: [[1, 1, 1, 0], [0, 1, -1, -1]],
    3: [[1, 1, 1, 1, 0], [0, -1, 2, 0.5, 0], [0, 1, 4, 0.25, 1]],
    4: [[1, 1, 1, 1, 1, 0], [0, 1, -1, 0.5, -2, 0], [0, 1, 1, 0.25, 4, 0], [0, 1, -1, 0.125, -8, 1]],
}


def wino_G(m):
    from co_occ_amd.core import PackedConv
    return PackedConv._wino_G(m)


def wino_conv(x, w, m, dtype=torch.float32, vscale=1.0):
    """3x3x3 stride-1 pad-1 convolution (no epilogue) by F(m x m, 3x3) over (x, y) with direct z taps, in ``dtype``:
    V = B^T d B * vscale, U = G g G^T (fp64, rounded to dtype), M[p] = sum_{dz, c} V[p] U[p] (one GEMM per transform point),
    Y = A^T M A / vscale.  Returns rows [B*X*Y*Z, N].  In fp32 this is the algorithm's own noise floor (the transforms
    amplify rounding): the anchor of the Winograd GPU cases."""
    B, C, X, Y, Z = x.shape
    N = w.shape[0]
    n = m + 2
    Tx, Ty = -(-X // m), -(-Y // m)
    BT, AT = torch.tensor(WINO_BT[m], dtype=dtype), torch.tensor(WINO_AT[m], dtype=dtype)
    U = torch.einsum("pa,qb,ncabz->pqzcn", wino_G(m), wino_G(m), _f64(w)).to(dtype)               # [n, n, 3, C, N]
    xp = torch.zeros(B, C, Tx * m + 2, Ty * m + 2, Z + 2, dtype=dtype)
    xp[:, :, 1:X + 1, 1:Y + 1, 1:Z + 1] = _f64(x).to(dtype)
    d = xp.unfold(2, n, m).unfold(3, n, m)                               # [B, C, Tx, Ty, Z+2, n, n]
    V = torch.einsum("pa,kctuzae,qe->kctuzpq", BT, d, BT) * vscale     # [B, C, Tx, Ty, Z+2, n, n]
    V = V.permute(5, 6, 0, 2, 3, 4, 1)                                   # [n, n, B, Tx, Ty, Z+2, C]
    M = torch.zeros(n, n, B, Tx, Ty, Z, N, dtype=dtype)
    for dz in range(3):
        M = M + torch.matmul(V[:, :, :, :, :, dz:dz + Z, :], U[:, :, dz][:, :, None, None, None])
    Yt = torch.einsum("ip,pqktuzn,jq->ktiujzn", AT, M, AT) / vscale     # [B, Tx, m, Ty, m, Z, N]
    Yt = Yt.reshape(B, Tx * m, Ty * m, Z, N)[:, :X, :Y]
    return Yt.reshape(-1, N)


def _wino_V(x, m, dtype):
    B, C, X, Y, Z = x.shape
    n, Tx, Ty = m + 2, -(-X // m), -(-Y // m)
    BT = torch.tensor(WINO_BT[m], dtype=dtype)
    xp = torch.zeros(B, C, Tx * m + 2, Ty * m + 2, Z + 2, dtype=dtype)
    xp[:, :, 1:X + 1, 1:Y + 1, 1:Z + 1] = _f64(x).to(dtype)
    d = xp.unfold(2, n, m).unfold(3, n, m)                               # [B, C, Tx, Ty, Z+2, n, n]
    return torch.einsum("pa,kctuzae,qe->pqktuzc", BT, d, BT)           # [n, n, B, Tx, Ty, Z+2, C]


def wino_wgrad(x, dy, m, dtype=torch.float32):
    """Weight gradient of the 3x3x3 stride-1 pad-1 convolution in the Winograd domain (the algorithm of csrc/wgrad_h2.hip and
    coocc_wino_wgrad), in ``dtype``: V = B^T d B, dM = A dY A^T, dU[p][dz] = sum V[p]^T dM[p] (rows shifted by dz),
    dW = G^T dU G.  x [B, C, X, Y, Z], dy [B, N, X, Y, Z] -> [N, C, 3, 3, 3]."""
    B, C, X, Y, Z = x.shape
    N = dy.shape[1]
    n, Tx, Ty = m + 2, -(-X // m), -(-Y // m)
    V = _wino_V(x, m, dtype)
    AT = torch.tensor(WINO_AT[m], dtype=dtype)
    dyp = torch.zeros(B, N, Tx * m, Ty * m, Z, dtype=dtype)
    dyp[:, :, :X, :Y] = _f64(dy).to(dtype)
    dM = torch.einsum("ip,kntiujz,jq->pqktuzn", AT, dyp.view(B, N, Tx, m, Ty, m, Z), AT).reshape(n, n, -1, N)
    dU = torch.stack([V[:, :, :, :, :, dz:dz + Z].reshape(n, n, -1, C).transpose(2, 3) @ dM for dz in range(3)], 2)
    G = wino_G(m).to(dtype)
    return torch.einsum("pa,qb,pqzcn->ncabz", G, G, dU)


# ------------------------------------------------------------------ which kernels ran (core.TIMER region names)
def kernels_start():
    from co_occ_amd import core
    core.TIMER.enabled, core.TIMER.only = 1, None
    core.TIMER.reset()


def kernels_stop():
    """{region name: launches} of everything launched since ``kernels_start``."""
    from co_occ_amd import core
    torch.cuda.synchronize()
    names = {k: v["launches"] for k, v in core.TIMER.summary().items()}
    core.TIMER.enabled = False
    core.TIMER.reset()
    return names


@contextlib.contextmanager
def kernels():
    """The TIMER region names of the launches inside the block (a dict name -> launches, filled when the block ends)."""
    names = {}
    kernels_start()
    try:
        yield names
    finally:
        names.update(kernels_stop())


# ------------------------------------------------------------------ the OccHead fine-branch chain (Linear-first form)
def fine_chain(samp, vq, prm, dtype=torch.float64, split=False):
    """logits = W3 h + b3,  h = ReLU(GN16(vq + W0[:, 128:] y1 + b0)),  y1 = ReLU(GN16(samp + b_img))   (occ_head.py:70-83 with
    both Linear(128 -> 64) layers applied before the resampling: samp / vq are the resampled P = W_img g and Q = W0[:, :128] x;
    csrc/fine_mlp.hip k_fine_mlp<pre>, csrc/fine2_h2.hip).  GroupNorm(16, 64) over groups of 4 channels of one point.
    ``split``: the two GEMMs with fp32-valued operands split the engine's way (fp64 otherwise), result rounded to fp32."""
    t = lambda k: _f64(prm[k]).to(dtype)

    def gn(h, w, b, eps):
        v = h.reshape(h.shape[0], 16, -1)
        m = v.mean(-1, keepdim=True)
        var = (v - m).pow(2).mean(-1, keepdim=True)
        return ((v - m) / torch.sqrt(var + eps)).reshape(h.shape) * w + b
    mm = (lambda a, b: split_mm(a.float(), b.float())) if split else (lambda a, b: a @ b)
    y1 = torch.relu(gn(_f64(samp).to(dtype) + t("b_img"), t("g_img"), t("be_img"), prm["eps_img"]))
    h = torch.relu(gn(_f64(vq).to(dtype) + mm(y1, t("w_f0")[:, 128:].t()) + t("b_f0"), t("g_f0"), t("be_f0"), prm["eps_f0"]))
    out = mm(h, t("w_f3").t()) + t("b_f3")
    return out.float() if split else out


# ------------------------------------------------------------------ training: the own-scale judge of forward / dgrad / wgrad
def train_judge(x, w, up, yd, dx, dw, k, stride, wino, what, names):
    """Judge a ConvRowsFn forward (yd rows), dgrad (dx rows) and wgrad (dw) on float64 autograd of conv3d + ReLU with the
    ReLU mask of the kernel's own forward, after checking which kernels ran (``names``: region -> launches).  Anchors: the
    split emulation (the gradient operand scaled like the device does it: max |dy| into [512, 1024)) on the split-f16 GEMMs,
    the Winograd fp32 emulations at the tile the launch used on the Winograd ones, fp32 elsewhere."""
    import re
    import torch.nn.functional as F
    from co_occ_amd import core
    tiles = {int(m.group(1)) for n in names for m in [re.fullmatch(r"k_gemm_h2z wino(\d)", n)] if m}
    wtiles = {int(m.group(1)) for n in names for m in [re.fullmatch(r"k_wgrad_h2 wino(\d)", n)] if m}
    if wino:
        assert len(tiles) == 1 and names["k_gemm_h2z wino%d" % min(tiles)] >= 2, "forward + dgrad on the Winograd split-f16 GEMM: %s" % names
    else:
        assert not tiles and any(n.startswith("k_gemm_h2") and "dgrad" not in n for n in names), "forward: %s" % names
        assert ("k_gemm_h2 conv_dgrad" if stride == 1 else "conv_dgrad") in names, "dgrad: %s" % names
    if k == 3 and stride == 1:
        assert len(wtiles) == 1, "wgrad in the Winograd domain on the split-f16 engine: %s" % names
    else:
        assert ("k_wgrad_h2" if k == 1 else "k_wgrad") in names, "wgrad: %s" % names
    pad = k // 2
    B, Cout = up.shape[:2]
    yd = yd.detach().cpu()
    r64, r32, rs = gemm_refs(conv_taps(x, w, stride, pad), split=not wino, relu=True)
    if wino:
        rs = None
        tile = min(tiles)
        r32 = torch.relu(wino_conv(x, w, tile, vscale=core.H2_WINO_SCALE[tile]))
    assert_precise(yd, r64, r32, rs, what="train fwd " + what)
    mask = (yd > 0).view(B, *up.shape[2:], Cout).permute(0, 4, 1, 2, 3)
    dy = up * mask
    grads = {}
    for dt in (torch.float64, torch.float32):
        xa, wa = x.to(dt).requires_grad_(True), w.to(dt).requires_grad_(True)
        F.conv3d(xa, wa, stride=stride, padding=pad).backward(dy.to(dt))
        grads[dt] = (ncdhw_rows(xa.grad), wa.grad)
    (dx64, dw64), (dx32, dw32) = grads[torch.float64], grads[torch.float32]
    amax = float(dy.abs().max())
    s = 2.0 ** (9 - torch.floor(torch.log2(torch.tensor(amax))).item()) if amax > 0 else 1.0
    dxs = dws = None
    wt = w.transpose(0, 1).flip(2, 3, 4)
    if stride == 1 and not wino:
        _, _, dxs = gemm_refs([(a * s, b) for a, b in conv_taps(dy, wt, 1, pad)])
        dxs = (dxs.double() / s).float()
    if stride == 1 and k == 1:
        _, _, dws = gemm_refs([(ncdhw_rows(dy).t() * s, ncdhw_rows(x))])
        dws = (dws.double() / s).float().view_as(dw64)
    if stride == 1 and k == 3:
        dw32 = wino_wgrad(x, dy, min(wtiles))          # the weight gradient runs in the Winograd domain
        if wino:
            dx32 = wino_conv(dy, wt, min(tiles))         # ... and so does the stride-1 dgrad
    assert_precise(dx.cpu(), dx64, dx32, dxs, what="train dgrad " + what)
    assert_precise(dw.cpu(), dw64, dw32, dws, what="train wgrad " + what)
