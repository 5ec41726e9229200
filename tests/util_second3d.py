"""Helpers of the LiDAR-trunk tests beyond tests/util.py: per-axis-stride taps for ``util.gemm_refs`` and the one-z-tap form of
``util.wino_conv`` (the Winograd fp32 emulation of a 3x3x1 layer)."""
import torch

from util import WINO_AT, WINO_BT, _f64, wino_G


def conv_taps_axes(x, w, strides=(1, 1, 1), pads=None):
    """Taps of a convolution with per-axis kernel / stride / padding as GEMM operand pairs: x [B, C, X, Y, Z], w [N, C, kx, ky, kz] ->
    [(rows of tap t = (dx*ky + dy)*kz + dz [B*Xo*Yo*Zo, C] in (b, x, y, z) order, W_t [C, N]), ...]."""
    k = tuple(w.shape[2:])
    pads = tuple((n - 1) // 2 for n in k) if pads is None else tuple(pads)
    xp = torch.nn.functional.pad(_f64(x), (pads[2], pads[2], pads[1], pads[1], pads[0], pads[0]))
    C = x.shape[1]
    o = [(n + 2 * p - kk) // s + 1 for n, kk, s, p in zip(x.shape[2:], k, strides, pads)]
    out = []
    for a in range(k[0]):
        for b in range(k[1]):
            for c in range(k[2]):
                s = xp[:, :, a:a + strides[0] * (o[0] - 1) + 1:strides[0], b:b + strides[1] * (o[1] - 1) + 1:strides[1],
                       c:c + strides[2] * (o[2] - 1) + 1:strides[2]]
                out.append((s.permute(0, 2, 3, 4, 1).reshape(-1, C), _f64(w[:, :, a, b, c]).t()))
    return out


def wino_conv_1z(x, w, m, dtype=torch.float32, vscale=1.0):
    """3x3x1 stride-1 pad-(1,1,0) convolution (no epilogue) by F(m x m, 3x3) over (x, y) with its single z tap, in ``dtype``
    (``util.wino_conv`` restricted to one z tap): x [B, C, X, Y, Z], w [N, C, 3, 3, 1] -> rows [B*X*Y*Z, N]."""
    B, C, X, Y, Z = x.shape
    N = w.shape[0]
    n = m + 2
    Tx, Ty = -(-X // m), -(-Y // m)
    BT, AT = torch.tensor(WINO_BT[m], dtype=dtype), torch.tensor(WINO_AT[m], dtype=dtype)
    U = torch.einsum("pa,qb,ncab->pqcn", wino_G(m), wino_G(m), _f64(w)[..., 0]).to(dtype)          # [n, n, C, N]
    xp = torch.zeros(B, C, Tx * m + 2, Ty * m + 2, Z, dtype=dtype)
    xp[:, :, 1:X + 1, 1:Y + 1] = _f64(x).to(dtype)
    d = xp.unfold(2, n, m).unfold(3, n, m)                               # [B, C, Tx, Ty, Z, n, n]
    V = torch.einsum("pa,kctuzae,qe->kctuzpq", BT, d, BT) * vscale
    V = V.permute(5, 6, 0, 2, 3, 4, 1)                                   # [n, n, B, Tx, Ty, Z, C]
    M = torch.matmul(V, U[:, :, None, None, None])                      # [n, n, B, Tx, Ty, Z, N]
    Yt = torch.einsum("ip,pqktuzn,jq->ktiujzn", AT, M, AT) / vscale     # [B, Tx, m, Ty, m, Z, N]
    return Yt.reshape(B, Tx * m, Ty * m, Z, N)[:, :X, :Y].reshape(-1, N)


def bits_equal(a, b):
    if a.shape != b.shape or a.dtype != b.dtype:
        return False
    it = {4: torch.int32, 2: torch.int16, 8: torch.int64}[a.element_size()]
    return torch.equal(a.contiguous().view(it), b.contiguous().view(it))
