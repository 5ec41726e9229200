"""Plain-torch references, input generators and the three judging rules for the normalisation and column-sum kernels: training-mode
BatchNorm (csrc/backward.hip ``coocc_bn_*``, csrc/sparse_train.hip ``coocc_bn_apply_ex``), the two GroupNorms (csrc/fine.hip, their
backward in csrc/backward.hip) and ``coocc_conv_epilogue_bwd[_ex]`` (csrc/conv_bwd.hip).  Used by tests/test_norm_host.py (no GPU) and
tests/test_gpu_norm.py.

Every operation is written once as a function of a dtype: float64 is the reference, float32 the anchor of ``util.assert_precise``.
The formulas are those of the kernels' own comments; a reference takes exactly what the entry takes (``mean`` / ``var`` are inputs of
the apply and backward passes, ``y`` is an input of every backward pass and the ReLU mask is ``y > 0`` of that ``y`` alone).

The rules:
  1. exact -- ``assert_exact``: bit equality (and integer-valued sums: exact integers);
  2. elementwise outputs -- ``util.assert_precise(out, ref64, ref32)`` with the project's C_MAX = 4, C_RMS = 2;
  3. per-channel sums -- ``assert_sum``: a derived bound per channel.  With t_i the float64 terms of a channel, S = sum |t_i|, n terms:
       fp64-accumulated, terms exact floats (mean, dbeta, fast dbias)  |out - ref| <= 2^-24 |ref| + n 2^-53 S
       fp64-accumulated dgamma                                         |out - ref| <= 2^-24 |ref| + 8 2^-24 S
       fp32-accumulated (atomics, generic dbias)                       |out - ref| <= (depth + 8) 2^-24 S
     (2^-24 |ref|: the one rounding of the fp64 total to float; n 2^-53 S: n sequential fp64 additions; 8 2^-24 S: the fp32
     roundings of xhat and rstd inside each term; depth: the longest chain of fp32 additions a term passes through.)
     A sum accumulated onto a start value s (``dbias_accumulate``) is out = fl32(s + d) with |d - ref_d| <= b0, hence
     |out - (s + ref_d)| <= b0 (1 + 2^-24) + 2^-24 |s + ref_d| for the fp64 forms; for the fp32 form s is one more term and one more
     addition: (depth + 9) 2^-24 (S + |s|)."""
import json
import math
import os

import torch

import util

F32, F64 = torch.float32, torch.float64
U24, U53 = 2.0 ** -24, 2.0 ** -53
TINY = 2.0 ** -126               # the smallest normal float
BN_EPS, GN_EPS = 1e-3, 1e-5
NAN = float("nan")


def eps32(eps):
    """``eps`` as the kernels see it: a float argument."""
    return float(torch.tensor(eps, dtype=F32))


def col_fast(C):
    """csrc/colreduce.h col_fast: the widths that take the float4 / fp64 fast column reductions."""
    return C % 4 == 0 and C // 4 <= 256 and 256 % (C // 4) == 0


def cdiv(a, b):
    return -(-a // b)


# ----------------------------------------------------------------------------- input generators
def gen(seed):
    return torch.Generator().manual_seed(seed)


def no_subnormals(t):
    return torch.where(t.abs() < TINY, torch.zeros_like(t), t)


def clipped(pre):
    """A post-ReLU output as a backward entry gets it: exact zeros where the ReLU clipped, every 5th of them -0.0, no subnormals."""
    y = torch.relu(no_subnormals(pre.to(F32))).contiguous().clone()
    flat = y.view(-1)
    if not bool((flat == 0).any()):
        flat[0] = 0.0
    idx = (flat == 0).nonzero().flatten()
    flat[idx] = 0.0
    flat[idx[::5]] = -0.0
    return y


def bn_rows(M, C, kind, g):
    """"normal": N(0, 1).  "offset": per-channel std log-uniform over [0.01, 10] (shuffled), mean up to +-100 std."""
    x = torch.randn(M, C, generator=g)
    if kind == "offset":
        std = torch.logspace(-2, 1, C)[torch.randperm(C, generator=g)]
        x = x * std + std * torch.linspace(-100, 100, C)
    else:
        assert kind == "normal"
    return no_subnormals(x)


def gn_rows(N, HW, C, kind, g):
    """"normal": N(0, 1).  "offset": 0.5 N(0, 1) + linspace(-4, 4, C)."""
    x = torch.randn(N, HW, C, generator=g)
    if kind == "offset":
        x = 0.5 * x + torch.linspace(-4, 4, C)
    else:
        assert kind == "normal"
    return no_subnormals(x)


def affine(C, g):
    return torch.rand(C, generator=g) + 0.5, torch.randn(C, generator=g) * 0.2


def int_grad(shape, g):
    """A gradient drawn from {-3 .. 3}: every masked sum of it is an exact integer in fp32 and in fp64."""
    return torch.randint(-3, 4, shape, generator=g).to(F32)


def bn_case(M, C, kind, seed=None):
    """Everything the BatchNorm entries take at one shape: x, the float-rounded float64 statistics, gamma / beta, a residual, dy
    (normal and integer-valued), and per relu the y a backward pass is handed (relu 1: clipped; relu 0: the unclipped output, whose
    negatives the kernel must ignore)."""
    g = gen(1000 * M + C if seed is None else seed)
    x = bn_rows(M, C, kind, g)
    m64, v64 = bn_stats(x, F64)
    c = dict(M=M, C=C, kind=kind, x=x, mean=m64.to(F32), var=v64.to(F32), eps=BN_EPS)
    c["gamma"], c["beta"] = affine(C, g)
    c["res"] = torch.randn(M, C, generator=g)
    c["dy"] = no_subnormals(torch.randn(M, C, generator=g))
    c["dy_int"] = int_grad((M, C), g)
    pre = bn_apply(x, c["mean"], c["var"], c["gamma"], c["beta"], BN_EPS, c["res"], 0, F32)
    c["y"] = {0: no_subnormals(pre), 1: clipped(pre)}
    return c


def gn_case(N, HW, C, groups, kind, seed=None):
    g = gen(100 * HW + C + 7 * N + groups if seed is None else seed)
    x = gn_rows(N, HW, C, kind, g)
    c = dict(N=N, HW=HW, C=C, groups=groups, kind=kind, x=x, eps=GN_EPS)
    c["gamma"], c["beta"] = affine(C, g)
    c["dy"] = no_subnormals(torch.randn(N, HW, C, generator=g))
    c["dy_int"] = int_grad((N, HW, C), g)
    pre = gn_forward(x, groups, c["gamma"], c["beta"], GN_EPS, 0, F32)
    c["y"] = {0: no_subnormals(pre), 1: clipped(pre)}
    return c


# ----------------------------------------------------------------------------- BatchNorm with batch statistics
def bn_stats(x, dt):
    """Two-pass mean and biased variance per channel of rows [M, C]."""
    x = x.to(dt)
    mean = x.mean(0)
    return mean, (x - mean).pow(2).mean(0)


def bn_apply(x, mean, var, gamma, beta, eps, res, relu, dt):
    """y = relu((x - mean) * rstd * gamma + beta (+ res)),  rstd = 1 / sqrt(var + eps)."""
    x, mean, var, gamma, beta = (t.to(dt) for t in (x, mean, var, gamma, beta))
    v = (x - mean) * (1 / torch.sqrt(var + eps32(eps))) * gamma + beta
    if res is not None:
        v = v + res.to(dt)
    return torch.relu(v) if relu else v


def masked(y, dy, relu, dt=F32):
    """dpre = dy * [y > 0] (relu) -- exact in every dtype; -0.0, 0.0 and NaN of y all clip."""
    dy = dy.to(dt)
    return torch.where(y > 0, dy, torch.zeros((), dtype=dt)) if relu else dy


def bn_backward_terms(x, y, dy, mean, var, eps, relu, dt):
    """The terms [M, C] whose column sums are dgamma (dpre * xhat) and dbeta (dpre)."""
    x, mean, var = (t.to(dt) for t in (x, mean, var))
    dpre = masked(y, dy, relu, dt)
    return dpre * ((x - mean) * (1 / torch.sqrt(var + eps32(eps)))), dpre


def bn_backward_dx(x, y, dy, mean, var, gamma, eps, relu, dgamma, dbeta, count, dt):
    """dx = gamma * rstd * (dpre - dbeta / count - xhat * dgamma / count) from GIVEN sums and count (those of the whole cross-rank
    batch under SyncBN); dres = dpre."""
    x, mean, var, gamma, dgamma, dbeta = (t.to(dt) for t in (x, mean, var, gamma, dgamma, dbeta))
    rstd = 1 / torch.sqrt(var + eps32(eps))
    dpre = masked(y, dy, relu, dt)
    xhat = (x - mean) * rstd
    return gamma * rstd * (dpre - dbeta / count - xhat * dgamma / count), dpre


# ----------------------------------------------------------------------------- GroupNorm ([N, HW, C]; rows [n, C] are HW = 1)
def _gn_xhat(x, groups, eps, dt):
    N, HW, C = x.shape
    xs = x.to(dt).view(N, HW, groups, C // groups)
    mean = xs.mean((1, 3), keepdim=True)
    var = (xs - mean).pow(2).mean((1, 3), keepdim=True)
    rstd = 1 / torch.sqrt(var + eps32(eps))
    return (xs - mean) * rstd, rstd


def gn_forward(x, groups, gamma, beta, eps, relu, dt):
    """y = relu(xhat * gamma + beta), statistics per (image, group) over HW * C / groups values."""
    xhat, _ = _gn_xhat(x, groups, eps, dt)
    v = xhat.reshape(x.shape) * gamma.to(dt) + beta.to(dt)
    return torch.relu(v) if relu else v


def gn_backward(x, y, dy, groups, gamma, eps, relu, dt, drop_m2=False):
    """dxhat = dy * [y > 0] * gamma;  dx = rstd * (dxhat - m1 - xhat * m2), m1 = mean(dxhat), m2 = mean(dxhat * xhat) per (image,
    group).  Returns dx and the terms [N * HW, C] of dgamma (dpre * xhat) and dbeta (dpre).  ``drop_m2``: the wrong variant of the
    host test."""
    N, HW, C = x.shape
    xhat, rstd = _gn_xhat(x, groups, eps, dt)
    dpre = masked(y, dy, relu, dt)
    dxh = (dpre * gamma.to(dt)).view(xhat.shape)
    m1 = dxh.mean((1, 3), keepdim=True)
    m2 = (dxh * xhat).mean((1, 3), keepdim=True)
    if drop_m2:
        m2 = torch.zeros_like(m2)
    dx = (rstd * (dxh - m1 - xhat * m2)).reshape(N, HW, C)
    return dx, (dpre.view(xhat.shape) * xhat).reshape(N * HW, C), dpre.reshape(N * HW, C)


# ----------------------------------------------------------------------------- the gradient scale of coocc_conv_epilogue_bwd_ex
def amax_k(amax, target):
    """k_amax_scale's rule on the host: k = e_target - e_amax of frexp (x = m 2^e, m in [0.5, 1)), clamped to +-100; 0 for an amax
    that is zero, infinite or NaN.  amax 2^k then lies in [2^(e_t - 1), 2^e_t) with 2^(e_t - 1) <= target < 2^e_t."""
    a = float(torch.tensor(amax, dtype=F32))
    if not (a > 0.0 and a < 3.0e38):
        return 0
    return min(max(math.frexp(target)[1] - math.frexp(a)[1], -100), 100)


def amax_interval(target):
    e = math.frexp(target)[1]
    return 2.0 ** (e - 1), 2.0 ** e


# ----------------------------------------------------------------------------- rule 1
def bits_equal(a, b):
    a, b = a.detach().cpu().contiguous(), b.detach().cpu().contiguous()
    return a.shape == b.shape and a.dtype == b.dtype == F32 and bool(torch.equal(a.view(torch.int32), b.view(torch.int32)))


def assert_exact(out, ref, what=""):
    """Bit equality of two fp32 tensors, NaN-free."""
    assert not bool(torch.isnan(out).any()), what + ": NaN in the result"
    if not bits_equal(out, ref):
        o, r = out.detach().cpu(), ref.detach().cpu()
        assert o.shape == r.shape, "%s: shape %s vs %s" % (what, tuple(o.shape), tuple(r.shape))
        bad = (o.contiguous().view(torch.int32) != r.contiguous().view(torch.int32))
        i = bad.nonzero()[0].tolist()
        raise AssertionError("%s: %d of %d values differ in their bits, first at %s: %r vs %r" % (
            what, int(bad.sum()), o.numel(), i, float(o[tuple(i)]), float(r[tuple(i)])))


# ----------------------------------------------------------------------------- rule 3
def _log(st):
    log = os.environ.get("COOCC_PREC_LOG")
    if log:
        with open(log, "a") as f:
            f.write(json.dumps(st) + "\n")


def sum_bound(terms, form, depth=None, start=None):
    """(ref, bound) per channel for the column sum of float64 ``terms`` [n, C] under one of the forms of the module docstring:
    "f64" (terms exact floats), "f64_dgamma", "f32" (``depth`` required).  ``start``: the value accumulated onto."""
    t = terms.to(F64)
    n = t.shape[0]
    ref, S = t.sum(0), t.abs().sum(0)
    if form == "f32":
        assert depth is not None
        if start is not None:
            s = start.to(F64)
            return ref + s, (depth + 9) * U24 * (S + s.abs())
        return ref, (depth + 8) * U24 * S
    b = U24 * ref.abs() + (n * U53 * S if form == "f64" else 8 * U24 * S)
    assert form in ("f64", "f64_dgamma")
    if start is not None:
        ref = ref + start.to(F64)
        b = b * (1 + U24) + U24 * ref.abs()
    return ref, b


def sum_ratio(out, terms, form, depth=None, start=None, what=""):
    """max over channels of |out - ref| / bound (0 where both vanish); no assertion."""
    ref, b = sum_bound(terms, form, depth, start)
    o = out.detach().to("cpu", F64)
    assert o.shape == ref.shape, "%s: shape %s vs %s" % (what, tuple(o.shape), tuple(ref.shape))
    if bool(torch.isnan(o).any()):
        return float("inf")
    d = (o - ref).abs()
    r = torch.where(d == 0, torch.zeros_like(d), d / b.clamp(min=1e-300))
    ratio = float(r.max()) if r.numel() else 0.0
    print("[bound] %-44s %-10s max |out - ref| / bound %.3f (<= 1)%s" % (what, form, ratio, "" if ratio <= 1 else "  MISS"))
    _log(dict(what=what, form=form, ratio_bound=ratio, ok=ratio <= 1))
    return ratio


def assert_sum(out, terms, form, depth=None, start=None, what=""):
    ratio = sum_ratio(out, terms, form, depth, start, what)
    assert ratio <= 1.0, "%s: a per-channel sum is %.3f of its bound from float64 (form %s%s)" % (
        what, ratio, form, "" if depth is None else ", depth %d" % depth)
    return ratio


def assert_int_sum(out, terms, start=None, what=""):
    """The exact-integer form of rule 1 for a sum of integer-valued terms (a dropped or doubled contribution shows as +-1 .. 3)."""
    ref = terms.to(F64).sum(0)
    if start is not None:
        ref = ref + start.to(F64)
    assert float(ref.abs().max()) < 2.0 ** 24
    assert_exact(out, ref.to(F32) + 0.0, what)        # (+ 0.0: an empty or cancelling sum is +0.0 on both sides)


def var_ratio(var, x, what=""):
    """coocc_bn_stats' variance against the two-pass float64 one: |var - var64| <= 2^-24 var64 + 4 M 2^-53 mean(x^2) (the fp64
    one-pass form E[x^2] - mean^2: M additions for each moment and the product), never negative, exactly 0 for M = 1."""
    xd = x.to(F64)
    M = xd.shape[0]
    _, v64 = bn_stats(xd, F64)
    b = U24 * v64 + 4 * M * U53 * xd.pow(2).mean(0)
    v = var.detach().to("cpu", F64)
    if bool(torch.isnan(v).any()) or bool((v < 0).any()) or (M == 1 and float(v.abs().max()) != 0.0):
        ratio = float("inf")
    else:
        d = (v - v64).abs()
        ratio = float(torch.where(d == 0, torch.zeros_like(d), d / b.clamp(min=1e-300)).max())
    print("[bound] %-44s %-10s max |out - ref| / bound %.3f (<= 1)%s" % (what, "var", ratio, "" if ratio <= 1 else "  MISS"))
    _log(dict(what=what, form="var", ratio_bound=ratio, ok=ratio <= 1))
    return ratio


def assert_var(var, x, what=""):
    ratio = var_ratio(var, x, what)
    assert ratio <= 1.0, "%s: the variance is %.3f of its bound from float64 (or negative, or not 0 at M = 1)" % (what, ratio)
    return ratio


def assert_precise(out, ref64, ref32, what=""):
    """Rule 2, and no NaN in the result."""
    assert not bool(torch.isnan(out).any()), what + ": NaN in the result"
    return util.assert_precise(out, ref64, ref32, what=what)
