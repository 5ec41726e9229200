"""The normalisation and column-sum entries without a GPU: (a) each refuses bad arguments with COOCC_EINVAL and a message naming it,
before any launch; (b) the float64 references of tests/norm_refs.py agree with ``torch.nn`` modules in float64, forward and
autograd; (c) each judging rule of norm_refs rejects wrong results made on the CPU and passes a correct fp32 one; (d) the input
generators have the properties tests/test_gpu_norm.py relies on."""
import ctypes

import pytest
import torch

from co_occ_amd import _lib

import norm_refs as R
import util

F32, F64 = torch.float32, torch.float64
ONE = ctypes.c_void_p(16)       # a non-null, 16-byte aligned dummy address: validation never dereferences device pointers
ODD = ctypes.c_void_p(20)       # ... and one that is 4- but not 16-byte aligned


# ----------------------------------------------------------------------------- a. argument validation
def _refused(lib, rc, name, what):
    assert rc == -1, "%s: %s returned %d, not COOCC_EINVAL" % (name, what, rc)
    assert name.encode() in lib.coocc_last_error(), "%s: %s: the message %r does not name the entry" % (name, what, lib.coocc_last_error())


def test_bn_entries_validate_before_launching():
    lib = _lib.load()
    dbl = 8

    def stats(x=ONE, stride=64, M=130, C=64, mean=ONE, var=ONE, ws=ONE, ws_bytes=1 << 30):
        return lib.coocc_bn_stats(x, stride, M, C, mean, var, ws, ws_bytes, None)

    def sums(M=130, C=64, ws=ONE, ws_bytes=1 << 30, dgamma=ONE):
        return lib.coocc_bn_backward_sums(ONE, ONE, ONE, M, C, ONE, ONE, 1e-3, 1, dgamma, ONE, ws, ws_bytes, None)
    # the fast form (C = 64) keeps 2 doubles per channel and 64-row block, the generic one (C = 24) per 256-row block
    fast, generic = dbl * 2 * R.cdiv(130, 64) * 64, dbl * 2 * R.cdiv(300, 256) * 24
    for what, kw in [("stride < C", dict(stride=63)), ("M = 0", dict(M=0)), ("a null x", dict(x=None)), ("a null mean", dict(mean=None)),
                     ("a null var", dict(var=None)), ("a null workspace", dict(ws=None)),
                     ("a workspace one double short of the fast form", dict(ws_bytes=fast - dbl)),
                     ("a workspace one double short of the generic form", dict(M=300, C=24, stride=24, ws_bytes=generic - dbl))]:
        _refused(lib, stats(**kw), "bn_stats", what)
    for what, kw in [("M = 0", dict(M=0)), ("a null dgamma", dict(dgamma=None)), ("a null workspace", dict(ws=None)),
                     ("a workspace one double short of the fast form", dict(ws_bytes=fast - dbl)),
                     ("a workspace one double short of the generic form", dict(M=300, C=24, ws_bytes=generic - dbl))]:
        _refused(lib, sums(**kw), "bn_backward_sums", what)
    for count in (0.0, 0.5):
        rc = lib.coocc_bn_backward_dx(ONE, ONE, ONE, 130, 64, ONE, ONE, ONE, 1e-3, 1, ONE, ONE, count, ONE, None, None)
        _refused(lib, rc, "bn_backward_dx", "count = %g" % count)

    def apply_ex(x=ONE, C=64, y=ONE, res=None, mean=ONE, twin=None):
        return lib.coocc_bn_apply_ex(x, 130, C, mean, ONE, ONE, ONE, 1e-3, res, 1, y, twin, None)
    for what, kw in [("C % 4 != 0", dict(C=6)), ("a misaligned x", dict(x=ODD)), ("a misaligned y", dict(y=ODD)),
                     ("a misaligned residual", dict(res=ODD)), ("a misaligned mean", dict(mean=ODD)),
                     ("a twin with C % 32 != 0", dict(C=48, twin=ONE)), ("a misaligned twin", dict(twin=ODD)), ("a null x", dict(x=None))]:
        _refused(lib, apply_ex(**kw), "bn_apply_ex", what)


def test_groupnorm_entries_validate_before_launching():
    """(C <= 4096 is a limit of the backward alone: its per-block column sums live in 2 C floats of LDS; the forward keeps none.)"""
    lib = _lib.load()

    def fwd(n=10, C=64, stride=64, groups=16):
        return lib.coocc_groupnorm_rows(ONE, n, C, stride, groups, ONE, ONE, 1e-5, 1, None)

    def bwd(n=10, C=64, stride=64, groups=16, dx=ONE):
        return lib.coocc_groupnorm_rows_bwd(ONE, ONE, ONE, n, C, stride, groups, ONE, 1e-5, 1, dx, ONE, ONE, None)
    for what, kw in [("C % groups != 0", dict(groups=5)), ("stride < C", dict(stride=63)), ("groups = 0", dict(groups=0))]:
        _refused(lib, fwd(**kw), "groupnorm_rows", what)
        _refused(lib, bwd(**kw), "groupnorm_rows_bwd", what)
    _refused(lib, bwd(C=4100, stride=4100, groups=2), "groupnorm_rows_bwd", "C > 4096")
    _refused(lib, bwd(dx=None), "groupnorm_rows_bwd", "a null dx")
    rc = lib.coocc_groupnorm_nhwc_bwd(ONE, ONE, ONE, 2, 9, 130, 2, ONE, 1e-5, 1, ONE, ONE, ONE, None)
    _refused(lib, rc, "groupnorm_nhwc_bwd", "65 channels per group")
    rc = lib.coocc_groupnorm_nhwc_bwd(ONE, ONE, ONE, 2, 9, 64, 5, ONE, 1e-5, 1, ONE, ONE, ONE, None)
    _refused(lib, rc, "groupnorm_nhwc_bwd", "C % groups != 0")
    rc = lib.coocc_groupnorm_nhwc(ONE, 2, 0, 64, 16, ONE, ONE, 1e-5, 1, None)
    _refused(lib, rc, "groupnorm_nhwc", "HW = 0")


def test_conv_epilogue_bwd_validates_before_launching():
    """dacc and dres both null wherever the case allows it, so that no pass is launched in front of the refusal."""
    lib = _lib.load()

    def ex(M=300, C=64, dacc=None, dbias=None, ws=ONE, ws_floats=1 << 30, amax=None, scale2=None, target=1024.0, relu=0, out=None):
        return lib.coocc_conv_epilogue_bwd_ex(ONE, C, out, C, None, M, C, relu, dacc, C, None, C, 0, dbias, 0, ws, ws_floats, amax, scale2,
                                              target, None)
    generic = R.cdiv(300, 256)
    for what, kw in [("amax_word without scale2", dict(amax=ONE)), ("scale2 without amax_word", dict(scale2=ONE)),
                     ("an operand scale without dacc", dict(amax=ONE, scale2=ONE)),
                     ("an operand scale with C % 4 != 0", dict(C=6, dacc=ONE, amax=ONE, scale2=ONE)),
                     ("an operand scale with target 0", dict(dacc=ONE, amax=ONE, scale2=ONE, target=0.0)),
                     ("relu without out", dict(relu=1)), ("M = 0", dict(M=0)),
                     ("a dbias workspace one float short of the generic form (C = 24)", dict(C=24, dbias=ONE, ws_floats=generic * 24 - 1)),
                     ("a dbias workspace one float short of the generic form (C = 64)", dict(dbias=ONE, ws_floats=generic * 64 - 1)),
                     ("a null dbias workspace", dict(dbias=ONE, ws=None))]:
        _refused(lib, ex(**kw), "conv_epilogue_bwd", what)


# ----------------------------------------------------------------------------- b. the references against torch.nn in float64
def _close(a, b, what):
    scale = max(1.0, float(b.abs().max()))
    err = float((a - b).abs().max()) / scale
    assert err <= 1e-12, "%s: %.2e of scale" % (what, err)


@pytest.mark.parametrize("M,C", [(65, 64), (300, 24), (7, 3)])
@pytest.mark.parametrize("kind", ["normal", "offset"])
def test_bn_references_agree_with_torch_in_float64(M, C, kind):
    c = R.bn_case(M, C, kind)
    x, dy, gamma, beta, res = (c[k].to(F64) for k in ("x", "dy", "gamma", "beta", "res"))
    eps = R.eps32(c["eps"])
    bn = torch.nn.BatchNorm1d(C, eps=eps).double().train()
    bn.weight.data.copy_(gamma)
    bn.bias.data.copy_(beta)
    xa, ra = x.clone().requires_grad_(), res.clone().requires_grad_()
    y = torch.relu(bn(xa) + ra)
    y.backward(dy)
    mean, var = R.bn_stats(x, F64)
    _close(mean, xa.detach().mean(0), "mean")
    _close(var, xa.detach().var(0, unbiased=False), "var")
    _close(bn.running_mean, 0.1 * mean, "the module saw the same mean")
    yr = R.bn_apply(x, mean, var, gamma, beta, eps, res, 1, F64)
    _close(yr, y.detach(), "bn_apply")
    tg, tb = R.bn_backward_terms(x, yr, dy, mean, var, eps, 1, F64)
    _close(tg.sum(0), bn.weight.grad, "dgamma")
    _close(tb.sum(0), bn.bias.grad, "dbeta")
    dx, dres = R.bn_backward_dx(x, yr, dy, mean, var, gamma, eps, 1, tg.sum(0), tb.sum(0), float(M), F64)
    _close(dx, xa.grad, "dx")
    _close(dres, ra.grad, "dres")


@pytest.mark.parametrize("N,HW,C,groups", [(33, 1, 64, 16), (2, 37, 64, 16), (3, 20, 32, 32)])
@pytest.mark.parametrize("kind", ["normal", "offset"])
def test_gn_references_agree_with_torch_in_float64(N, HW, C, groups, kind):
    c = R.gn_case(N, HW, C, groups, kind)
    x, dy, gamma, beta = (c[k].to(F64) for k in ("x", "dy", "gamma", "beta"))
    eps = R.eps32(c["eps"])
    gn = torch.nn.GroupNorm(groups, C, eps=eps).double()
    gn.weight.data.copy_(gamma)
    gn.bias.data.copy_(beta)
    rows = HW == 1
    xa = (x.view(N, C) if rows else x.transpose(1, 2)).clone().requires_grad_()        # [n, C] | [N, C, HW]
    y = torch.relu(gn(xa))
    y.backward(dy.view(N, C) if rows else dy.transpose(1, 2))
    back = (lambda t: t.view(N, 1, C)) if rows else (lambda t: t.transpose(1, 2))
    yr = R.gn_forward(x, groups, gamma, beta, eps, 1, F64)
    _close(yr, back(y.detach()), "gn forward")
    dx, tg, tb = R.gn_backward(x, yr, dy, groups, gamma, eps, 1, F64)
    _close(dx, back(xa.grad), "gn dx")
    _close(tg.sum(0), gn.weight.grad, "gn dgamma")
    _close(tb.sum(0), gn.bias.grad, "gn dbeta")


# ----------------------------------------------------------------------------- c. each rule rejects a wrong result
def _seq32(t):
    """A column sum by sequential fp32 additions, row after row (torch's own CPU reductions accumulate floats more precisely)."""
    acc = torch.zeros(t.shape[1:], dtype=F32)
    for row in t.to(F32):
        acc = acc + row
    return acc


def _rejects(fn, *a, **kw):
    try:
        fn(*a, **kw)
    except AssertionError:
        return True
    return False


def test_rule_1_rejects_wrong_results():
    c = R.bn_case(130, 64, "normal")
    y, dy, dyi = c["y"][1], c["dy"], c["dy_int"]
    scale = torch.linspace(-2, 2, 64)
    dres = R.masked(y, dy, 1)
    assert bool((y == 0).any()) and bool(((y == 0) & (dy != 0)).any())
    R.assert_exact(dres.clone(), dres, "masked dy")
    R.assert_exact(R.masked(y, dy, 1) * scale, dres * scale, "dacc")
    assert _rejects(R.assert_exact, torch.where(y >= 0, dy, torch.zeros(())), dres), "the mask taken as y >= 0"
    assert _rejects(R.assert_exact, (dres.double() * scale.double() * (1 + 2.0 ** -23)).float(), dres * scale), "dacc one ulp off"
    nan = dres.clone()
    nan[5, 5] = R.NAN
    assert _rejects(R.assert_exact, nan, nan), "a NaN in the result"
    # integer-valued sums: exact
    terms = R.masked(y, dyi, 1, F64)
    good = _seq32(terms)                 # a sequential fp32 sum of integers is exact
    R.assert_int_sum(good, terms, what="integer dbeta")
    assert _rejects(R.assert_int_sum, terms[:-1].sum(0).float(), terms), "one row dropped"
    lane = torch.ones(130, dtype=torch.bool)
    lane[3::64] = False
    assert _rejects(R.assert_int_sum, terms[lane].sum(0).float(), terms), "one row lane of 64 dropped"
    assert _rejects(R.assert_int_sum, (terms.sum(0) + terms[7]).float(), terms), "one row counted twice"


def test_rule_2_rejects_wrong_results():
    # BatchNorm apply: a differently associated fp32 evaluation passes; statistics from a one-pass fp32 variance do not
    c = R.bn_case(300, 64, "offset")
    x, mean, var, gamma, beta, res = (c[k] for k in ("x", "mean", "var", "gamma", "beta", "res"))
    args = (gamma, beta, c["eps"], res, 1)
    y64, y32 = R.bn_apply(x, mean, var, *args, F64), R.bn_apply(x, mean, var, *args, F32)
    other = torch.relu((x - mean) * ((1 / torch.sqrt(var + R.eps32(c["eps"]))) * gamma) + (beta + res))
    R.assert_precise(other, y64, y32, "bn_apply, another fp32 association")
    m32 = _seq32(x) / 300
    v1 = (_seq32(x * x) / 300 - m32 * m32).clamp(min=0)
    assert _rejects(R.assert_precise, R.bn_apply(x, mean, v1, *args, F32), y64, y32), "a fp32 one-pass variance"
    assert _rejects(R.assert_precise, R.bn_apply(x, mean, var, gamma, beta, c["eps"], res, 0, F32), y64, y32), "no ReLU"
    # GroupNorm dx: pairwise fp32 passes, m2 left out does not, the mask as y >= 0 does not
    g = R.gn_case(2, 37, 64, 16, "offset")
    a = (g["x"], g["y"][1], g["dy"], 16, g["gamma"], g["eps"], 1)
    dx64, dx32 = R.gn_backward(*a, F64)[0], R.gn_backward(*a, F32)[0]
    R.assert_precise(dx32.clone(), dx64, dx32, "gn dx in fp32")
    assert _rejects(R.assert_precise, R.gn_backward(*a, F32, drop_m2=True)[0], dx64, dx32), "m2 left out of dx"
    ywrong = torch.where(g["y"][1] == 0, torch.ones(()), g["y"][1])                       # y >= 0 as the mask
    assert _rejects(R.assert_precise, R.gn_backward(g["x"], ywrong, *a[2:], F32)[0], dx64, dx32), "the mask taken as y >= 0"


def test_rule_3_rejects_wrong_results():
    M, C = 4161, 128
    c = R.bn_case(M, C, "offset")
    x, y, dy, mean, var = c["x"], c["y"][1], c["dy"], c["mean"], c["var"]
    tg, tb = R.bn_backward_terms(x, y, dy, mean, var, c["eps"], 1, F64)
    tg32, _ = R.bn_backward_terms(x, y, dy, mean, var, c["eps"], 1, F32)
    # correct stand-ins: fp64 sums of fp32-made terms rounded to float (the fp64 forms); pairwise and sequential fp32 sums (the fp32 form)
    R.assert_sum(tg32.double().sum(0).float(), tg, "f64_dgamma", what="dgamma")
    R.assert_sum(tb.sum(0).float(), tb, "f64", what="dbeta")
    R.assert_sum((x.double().sum(0) / M).float(), x.double() / M, "f64", what="mean")
    R.assert_var(R.bn_stats(x, F64)[1].float(), x, "var")
    xd = x.double()
    mu = xd.sum(0) / M
    R.assert_var(((xd * xd).sum(0) / M - mu * mu).clamp(min=0).float(), x, "var, one pass in fp64")
    # wrong ones
    assert _rejects(R.assert_sum, tg32[:-1].double().sum(0).float(), tg, "f64_dgamma"), "one row dropped from dgamma"
    assert _rejects(R.assert_sum, tb[:-1].sum(0).float(), tb, "f64"), "one row dropped from dbeta"
    lane = torch.ones(M, dtype=torch.bool)
    lane[5::64] = False
    assert _rejects(R.assert_sum, tb[lane].sum(0).float(), tb, "f64"), "one row lane of 64 dropped"
    assert _rejects(R.assert_sum, tb[:64 * 64].sum(0).float(), tb, "f64"), "partials 65.. ignored"
    assert _rejects(R.assert_sum, _seq32(tb), tb, "f64"), "a sequential fp32 sum in place of the fp64 one"
    m32 = _seq32(x) / M
    v1 = (_seq32(x * x) / M - m32 * m32).clamp(min=0)
    assert _rejects(R.assert_var, v1, x), "a fp32 one-pass variance on the offset inputs"
    assert _rejects(R.assert_var, R.bn_stats(x, F64)[1].float() * -1, x), "a negative variance"
    assert _rejects(R.assert_var, torch.full((4,), 1e-12), torch.randn(1, 4)), "a non-zero variance at M = 1"
    # the fp32 form, at most 1024 contributions per channel
    g = R.gn_case(333, 1, 128, 32, "normal")
    _, gg, gb = R.gn_backward(g["x"], g["y"][1], g["dy"], 32, g["gamma"], g["eps"], 1, F64)
    _, gg32, gb32 = R.gn_backward(g["x"], g["y"][1], g["dy"], 32, g["gamma"], g["eps"], 1, F32)
    for form_sum in (lambda t: t.sum(0), _seq32):
        R.assert_sum(form_sum(gg32), gg, "f32", depth=333, what="gn dgamma")
        R.assert_sum(form_sum(gb32), gb, "f32", depth=333, what="gn dbeta")
    assert _rejects(R.assert_sum, gg32[1:].sum(0), gg, "f32", depth=333), "one row dropped from gn dgamma"
    assert _rejects(R.assert_sum, (gb32.sum(0) + gb32[100]), gb, "f32", depth=333), "one row counted twice in gn dbeta"
    # accumulation onto a start value
    start = torch.randn(C)
    R.assert_sum(start + tb.sum(0).float(), tb, "f64", start=start, what="dbias accumulate")
    R.assert_sum(start[:128] + gb32.sum(0), gb, "f32", depth=258, start=start[:128], what="generic dbias accumulate")
    assert _rejects(R.assert_sum, tb.sum(0).float(), tb, "f64", start=start), "the start value dropped"


# ----------------------------------------------------------------------------- d. the generators
@pytest.mark.parametrize("kind", ["normal", "offset"])
def test_generators_have_the_properties_the_gpu_tests_rely_on(kind):
    for make, args in [(R.bn_case, (1, 3)), (R.bn_case, (1, 4)), (R.bn_case, (130, 64)), (R.bn_case, (257, 260)),
                       (R.gn_case, (1, 1, 8, 2)), (R.gn_case, (100, 1, 64, 64)), (R.gn_case, (2, 37, 64, 16))]:
        a, b = make(*args, kind), make(*args, kind)
        for k, v in a.items():
            if torch.is_tensor(v):
                assert R.bits_equal(v, b[k]), "seeded: " + k
                assert not bool(((v != 0) & (v.abs() < R.TINY)).any()), "no subnormals: " + k
                assert bool(torch.isfinite(v).all()), k
        y1, y0 = a["y"][1], a["y"][0]
        zero = y1 == 0
        neg = torch.signbit(y1) & zero
        assert bool(zero.any()) and bool(neg.any()), "exact zeros, some of them -0.0"
        assert int(zero.sum()) < 2 or bool((zero & ~neg).any()), "... and some of them +0.0"
        assert bool((y1 >= 0).all()) and not bool(((y1 != 0) & (y1.abs() < R.TINY)).any())
        assert R.bits_equal(y1[~zero], y0[~zero]), "y is the unclipped output where it is positive"
        assert set(a["dy_int"].unique().tolist()) <= {-3.0, -2.0, -1.0, 0.0, 1.0, 2.0, 3.0} and float(a["dy_int"].abs().max()) > 0
        if a["x"].numel() > 100:
            assert bool((y0 < 0).any()), "the unclipped y of relu = 0 has negatives the kernel must ignore"
    if kind == "offset":
        c = R.bn_case(4161, 128, "offset")
        std, mean = c["x"].double().std(0), c["x"].double().mean(0)
        assert 0.008 < float(std.min()) < 0.012 and 8 < float(std.max()) < 12, "std spread over [0.01, 10]"
        assert 90 < float((mean / std).abs().max()) < 110, "means up to +-100 std"
        g = R.gn_case(2, 37, 64, 16, "offset")
        assert abs(float(g["x"][..., 0].mean()) + 4) < 0.3 and abs(float(g["x"][..., -1].mean()) - 4) < 0.3


def test_amax_rule_on_the_host():
    lo, hi = R.amax_interval(1024.0)
    assert (lo, hi) == (1024.0, 2048.0) and R.amax_interval(1000.0) == (512.0, 1024.0)
    for a in (6e-8, 1 - 2.0 ** -24, 1.0, 1 + 2.0 ** -23, 1023.9, 1024.0, 3e3, 1e30):
        k = R.amax_k(a, 1024.0)
        assert lo <= float(torch.tensor(a, dtype=F32)) * 2.0 ** k < hi, a
    assert R.amax_k(1e-30, 1024.0) == 100 and R.amax_k(1e-38, 1024.0) == 100 and R.amax_k(1e35, 1024.0) == -100
    assert R.amax_k(0.0, 1024.0) == 0 and R.amax_k(float("inf"), 1024.0) == 0 and R.amax_k(R.NAN, 1024.0) == 0
    assert util.C_MAX == 4.0 and util.C_RMS == 2.0
