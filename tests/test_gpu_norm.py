"""The normalisation and column-sum kernels on the GPU, each entry alone through the C ABI against float64 (tests/norm_refs.py: the
references, the input kinds and the three judging rules): training-mode BatchNorm (``coocc_bn_stats / _apply / _apply_ex /
_backward_sums / _backward_dx / _backward``, both forms of csrc/colreduce.h), ``coocc_groupnorm_rows`` / ``_nhwc`` and their backward,
and ``coocc_conv_epilogue_bwd[_ex]`` with its bias-gradient sums and the device-made gradient scale.

Every buffer a kernel writes starts as NaN, the padding columns of strided buffers (inputs too) hold NaN: padding must still be NaN
afterwards and no NaN may reach a result.  Which of the two column-sum forms an entry took is observed, not assumed: the BatchNorm
entries refuse a workspace that is too small for the form they select (the fast form needs 4 x the blocks of the generic one), and
for the bias gradient a column [2^24, 1, 1, ..., -2^24] sums to the count of ones in fp64 and to 0 in sequential fp32."""
import functools

import pytest
import torch

from co_occ_amd import autograd as ag, core
from co_occ_amd._lib import CooccArgError, call, ptr

import norm_refs as R

pytestmark = pytest.mark.gpu

F32, F64 = torch.float32, torch.float64
KINDS = ["normal", "offset"]
_bn_case = functools.lru_cache(maxsize=None)(R.bn_case)
_gn_case = functools.lru_cache(maxsize=None)(R.gn_case)


def nans(dev, *shape):
    return torch.full(shape, R.NAN, device=dev, dtype=F32)


def D(dev, t):
    t = t.to(dev).contiguous()
    assert t.data_ptr() % 16 == 0
    return t


def padded(dev, t, stride, coff=0):
    """[rows, stride] of NaN with ``t`` [rows, C] in the columns from ``coff``."""
    buf = nans(dev, t.shape[0], stride)
    buf[:, coff:coff + t.shape[1]] = t.to(dev)
    return buf


def shifted(dev, t):
    """A copy of ``t`` that starts one float past a 16-byte aligned address: (buffer, 1) for ``ptr(buffer, offset=1)``."""
    buf = nans(dev, t.numel() + 1)
    assert buf.data_ptr() % 16 == 0
    buf[1:] = t.to(dev).flatten()
    return buf


def only_padding_is_nan(buf, C, coff=0, what=""):
    """The [rows, stride] output ``buf``: its C columns from ``coff`` NaN-free, every other column still NaN.  Returns the columns."""
    keep = torch.ones(buf.shape[1], dtype=torch.bool, device=buf.device)
    keep[coff:coff + C] = False
    assert bool(torch.isnan(buf[:, keep]).all()), what + ": a padding column was written"
    out = buf[:, coff:coff + C]
    assert not bool(torch.isnan(out).any()), what + ": NaN in the result"
    return out.contiguous()


_WS = {}


def ws64(dev):
    """A workspace of 2^18 doubles (the largest case, 4161 x 128 in the fast form, takes 2 * 66 * 128 of them)."""
    if dev not in _WS:
        _WS[dev] = torch.empty(1 << 18, dtype=F64, device=dev)
    return _WS[dev]


def parts_bytes(M, C, fast):
    """Bytes of the fp64 partials of a BatchNorm column reduction: 2 per channel and block of 64 (fast) or 256 (generic) rows."""
    return 8 * 2 * R.cdiv(M, 64 if fast else 256) * C


# ============================================================================= BatchNorm with batch statistics
BN_FAST = [(1, 4), (63, 64), (64, 64), (65, 64), (200, 8), (130, 1024), (4161, 128)]
BN_GENERIC = [(1, 3), (513, 6), (300, 24), (257, 260)]
BN_SHAPES = BN_FAST + BN_GENERIC


def test_shape_lists_select_the_forms_they_claim():
    assert all(R.col_fast(C) for _, C in BN_FAST) and not any(R.col_fast(C) for _, C in BN_GENERIC)
    assert R.cdiv(4161, 64) == 66          # more than 64 partial blocks: col_final's second lap


def stats(dev, xbuf, stride, M, C, offset=0, ws_bytes=None):
    mean, var = nans(dev, C), nans(dev, C)
    ws = ws64(dev)
    call("coocc_bn_stats", ptr(xbuf, offset=offset), stride, M, C, ptr(mean), ptr(var), ptr(ws), ws.numel() * 8 if ws_bytes is None else ws_bytes)
    return mean, var


def judge_stats(mean, var, x, what):
    M = x.shape[0]
    R.assert_sum(mean, x.to(F64) / M, "f64", what=what + " mean")
    R.assert_var(var, x, what + " var")


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("M,C", BN_SHAPES)
def test_bn_stats(dev, M, C, kind):
    c = _bn_case(M, C, kind)
    what = "bn_stats %s %dx%d" % (kind, M, C)
    xd = D(dev, c["x"])
    mean, var = stats(dev, xd, C, M, C)
    mean2, var2 = stats(dev, xd, C, M, C)
    judge_stats(mean.cpu(), var.cpu(), c["x"], what)
    assert R.bits_equal(mean, mean2) and R.bits_equal(var, var2), what + ": two calls on the same inputs differ"
    if R.col_fast(C) and M > 64:            # the fast form was selected: a workspace that holds only the generic form's partials is refused
        with pytest.raises(CooccArgError):
            stats(dev, xd, C, M, C, ws_bytes=parts_bytes(M, C, False))


@pytest.mark.parametrize("kind", KINDS)
def test_bn_stats_strided_and_misaligned(dev, kind):
    M, C = 130, 64
    c = _bn_case(M, C, kind)
    x = c["x"]
    small = parts_bytes(M, C, False)
    # stride 68, NaN padding: the fast form (it refuses the generic form's workspace)
    xb = padded(dev, x, 68)
    with pytest.raises(CooccArgError):
        stats(dev, xb, 68, M, C, ws_bytes=small)
    judge_stats(*(t.cpu() for t in stats(dev, xb, 68, M, C)), x, "bn_stats %s stride 68" % kind)
    # stride 65 and a base pointer one float off: the generic form (its workspace suffices)
    judge_stats(*(t.cpu() for t in stats(dev, padded(dev, x, 65), 65, M, C, ws_bytes=small)), x, "bn_stats %s stride 65" % kind)
    judge_stats(*(t.cpu() for t in stats(dev, shifted(dev, x), C, M, C, offset=1, ws_bytes=small)), x, "bn_stats %s base + 1" % kind)


def bn_apply(dev, c, relu, res, ex=False, twin=None):
    M, C = c["M"], c["C"]
    y = nans(dev, M, C)
    a = [ptr(D(dev, c["x"])), M, C] + [ptr(D(dev, c[k])) for k in ("mean", "var", "gamma", "beta")] + [c["eps"], ptr(D(dev, res)) if res is not None else None,
                                                                                                      relu, ptr(y)]
    if ex:
        call("coocc_bn_apply_ex", *a, ptr(twin))
    else:
        call("coocc_bn_apply", *a)
    return y


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("M,C", BN_SHAPES)
def test_bn_apply_and_its_twin_writing_form(dev, M, C, kind):
    c = _bn_case(M, C, kind)
    for relu in (0, 1):
        for res in (None, c["res"]):
            what = "bn_apply %s %dx%d relu %d res %d" % (kind, M, C, relu, res is not None)
            y = bn_apply(dev, c, relu, res)
            args = (c["x"], c["mean"], c["var"], c["gamma"], c["beta"], c["eps"], res, relu)
            R.assert_precise(y.cpu(), R.bn_apply(*args, F64), R.bn_apply(*args, F32), what)
            assert R.bits_equal(y, bn_apply(dev, c, relu, res)), what + ": two calls on the same inputs differ"
            if C % 4 == 0:
                twin = nans(dev, M, C) if C % 32 == 0 else None
                R.assert_exact(bn_apply(dev, c, relu, res, ex=True, twin=twin), y, what + ": bn_apply_ex y")
                if twin is not None:
                    want = nans(dev, M, C)
                    call("coocc_rows_to_h2", ptr(y), C, M, C, 1.0, ptr(want))
                    assert R.bits_equal(twin, want), what + ": bn_apply_ex's twin is not rows_to_h2(y)"
    torch.cuda.synchronize()
    core.check_h2_overflow()


def bn_sums(dev, c, y, dy, relu, shift=None, ws_bytes=None):
    """coocc_bn_backward_sums; ``shift``: the one input handed over one float past an aligned address."""
    M, C = c["M"], c["C"]
    t = dict(x=c["x"], y=y, dy=dy, mean=c["mean"], var=c["var"])
    p = {k: (ptr(shifted(dev, v), offset=1) if k == shift else ptr(D(dev, v))) for k, v in t.items()}
    dgamma, dbeta = nans(dev, C), nans(dev, C)
    ws = ws64(dev)
    call("coocc_bn_backward_sums", p["x"], p["y"], p["dy"], M, C, p["mean"], p["var"], c["eps"], relu, ptr(dgamma), ptr(dbeta), ptr(ws),
         ws.numel() * 8 if ws_bytes is None else ws_bytes)
    return dgamma, dbeta


def bn_dx(dev, c, y, dy, relu, dgamma, dbeta, count):
    M, C = c["M"], c["C"]
    dx, dres = nans(dev, M, C), nans(dev, M, C)
    call("coocc_bn_backward_dx", *(ptr(D(dev, t)) for t in (c["x"], y, dy)), M, C, *(ptr(D(dev, c[k])) for k in ("mean", "var", "gamma")),
         c["eps"], relu, ptr(D(dev, dgamma)), ptr(D(dev, dbeta)), float(count), ptr(dx), ptr(dres))
    return dx, dres


def judge_sums(c, y, dy, relu, dgamma, dbeta, what):
    tg, tb = R.bn_backward_terms(c["x"], y, dy, c["mean"], c["var"], c["eps"], relu, F64)
    R.assert_sum(dgamma.cpu(), tg, "f64_dgamma", what=what + " dgamma")
    R.assert_sum(dbeta.cpu(), tb, "f64", what=what + " dbeta")
    return tg, tb


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("M,C", BN_SHAPES)
def test_bn_backward(dev, M, C, kind):
    c = _bn_case(M, C, kind)
    for relu in (0, 1):
        what = "bn_backward %s %dx%d relu %d" % (kind, M, C, relu)
        y, dy = c["y"][relu], c["dy"]
        dgamma, dbeta = bn_sums(dev, c, y, dy, relu)
        tg, tb = judge_sums(c, y, dy, relu, dgamma, dbeta, what)
        dg2, db2 = bn_sums(dev, c, y, dy, relu)
        assert R.bits_equal(dgamma, dg2) and R.bits_equal(dbeta, db2), what + ": two calls on the same inputs differ"
        # integer-valued dy: dbeta is an exact integer
        _, dbi = bn_sums(dev, c, y, c["dy_int"], relu)
        R.assert_int_sum(dbi.cpu(), R.masked(y, c["dy_int"], relu, F64), what=what + " integer dbeta")
        # dx from GIVEN sums (the float-rounded float64 ones, handed to the device and to the references alike): this batch's with
        # count = M, then those of a batch twice as large
        otg, otb = R.bn_backward_terms(c["x"], y, c["res"], c["mean"], c["var"], c["eps"], relu, F64)      # (a second rank's terms)
        for sg, sb, count in ((tg.sum(0).to(F32), tb.sum(0).to(F32), M), ((tg.sum(0) + otg.sum(0)).to(F32), (tb.sum(0) + otb.sum(0)).to(F32), 2 * M)):
            dx, dres = bn_dx(dev, c, y, dy, relu, sg, sb, count)
            a = (c["x"], y, dy, c["mean"], c["var"], c["gamma"], c["eps"], relu, sg, sb, float(count))
            R.assert_precise(dx.cpu(), R.bn_backward_dx(*a, F64)[0], R.bn_backward_dx(*a, F32)[0], what + " dx count %d" % count)
            R.assert_exact(dres.cpu(), R.masked(y, dy, relu), what + " dres")
            dxb, dresb = bn_dx(dev, c, y, dy, relu, sg, sb, count)
            assert R.bits_equal(dx, dxb) and R.bits_equal(dres, dresb), what + ": two calls on the same inputs differ"
        # the one-call form is the two halves, bit for bit
        dx, dres = bn_dx(dev, c, y, dy, relu, dgamma, dbeta, M)
        dx1, dres1, dg1, db1 = nans(dev, M, C), nans(dev, M, C), nans(dev, C), nans(dev, C)
        ws = ws64(dev)
        call("coocc_bn_backward", *(ptr(D(dev, t)) for t in (c["x"], y, dy)), M, C, *(ptr(D(dev, c[k])) for k in ("mean", "var", "gamma")),
             c["eps"], relu, ptr(dx1), ptr(dres1), ptr(dg1), ptr(db1), ptr(ws), ws.numel() * 8)
        for got, want, name in ((dx1, dx, "dx"), (dres1, dres, "dres"), (dg1, dgamma, "dgamma"), (db1, dbeta, "dbeta")):
            R.assert_exact(got, want, what + ": coocc_bn_backward's %s against sums + dx" % name)


@pytest.mark.parametrize("kind", KINDS)
def test_bn_backward_sums_falls_back_on_a_misaligned_input(dev, kind):
    M, C = 130, 64
    c = _bn_case(M, C, kind)
    y, dy, small = c["y"][1], c["dy"], parts_bytes(M, C, False)
    with pytest.raises(CooccArgError):          # aligned: the fast form, which this workspace is too small for
        bn_sums(dev, c, y, dy, 1, ws_bytes=small)
    fast = bn_sums(dev, c, y, dy, 1)
    for shift in ("x", "y", "dy", "mean", "var"):
        what = "bn_backward_sums %s, %s one float off" % (kind, shift)
        dgamma, dbeta = bn_sums(dev, c, y, dy, 1, shift=shift, ws_bytes=small)      # ... the generic form, for which it suffices
        judge_sums(c, y, dy, 1, dgamma, dbeta, what)
        # (the two forms add the same fp64 terms in different orders: equal within the bounds, not promised to be equal in their bits)
        print("[forms] %s: %d of %d dgamma and %d of %d dbeta words equal to the fast form's" % (
            what, int((dgamma == fast[0]).sum()), C, int((dbeta == fast[1]).sum()), C))
        _, dbi = bn_sums(dev, c, y, c["dy_int"], 1, shift=shift, ws_bytes=small)
        R.assert_int_sum(dbi.cpu(), R.masked(y, c["dy_int"], 1, F64), what=what + " integer dbeta")


# ============================================================================= GroupNorm
def gn_depth_rows(n, groups):
    """k_groupnorm_rows_bwd: thread i is the pair (row i / groups, group i % groups); a block's 256 pairs add into one LDS word per
    channel (at most ceil(256 / groups) + 1 rows of a channel), then every block adds its word to the global one."""
    return min(n, R.cdiv(256, groups) + 1) + R.cdiv(n * groups, 256)


def gn_depth_nhwc(N, HW):
    """k_groupnorm_nhwc_bwd: a block (one image, one group) adds its HW rows into one LDS word per channel, then the N images' blocks
    add theirs to the global one."""
    return HW + N


def gn_check(dev, c, relu, fwd, bwd, depth, what):
    """Forward (in place) and backward of one GroupNorm entry pair on case ``c``; ``fwd(xbuf)`` / ``bwd(x, y, dy, dx, dgamma, dbeta)``
    launch on contiguous [N, HW, C] device tensors."""
    N, HW, C, groups = c["N"], c["HW"], c["C"], c["groups"]
    x, gamma, beta, eps = c["x"], c["gamma"], c["beta"], c["eps"]
    yd = D(dev, x).clone()
    fwd(yd)
    a = (x, groups, gamma, beta, eps, relu)
    R.assert_precise(yd.cpu(), R.gn_forward(*a, F64), R.gn_forward(*a, F32), what + " y")
    if C == groups and HW == 1:             # one value per group: xhat = 0, y = beta (or relu(beta)) exactly
        want = (torch.relu(beta) if relu else beta).expand(N, 1, C)
        assert bool((yd.cpu() == want).all()), what + ": y is not beta at one channel per group"
    y = c["y"][relu]
    for dy, integer in ((c["dy"], False), (c["dy_int"], True)):
        dx, dgamma, dbeta = nans(dev, N, HW, C), nans(dev, C), nans(dev, C)
        bwd(D(dev, x), D(dev, y), D(dev, dy), dx, dgamma, dbeta)
        b = (x, y, dy, groups, gamma, eps, relu)
        dx64, tg, tb = R.gn_backward(*b, F64)
        w = what + (" integer dy" if integer else "")
        R.assert_precise(dx.cpu(), dx64, R.gn_backward(*b, F32)[0], w + " dx")
        R.assert_sum(dgamma.cpu(), tg, "f32", depth=depth, what=w + " dgamma")
        R.assert_sum(dbeta.cpu(), tb, "f32", depth=depth, what=w + " dbeta")
        if integer:
            R.assert_int_sum(dbeta.cpu(), tb, what=w + " dbeta")
        if C == groups and HW == 1:
            assert float(dx.abs().max()) == 0.0, what + ": dx is not zero at one channel per group"


GN_ROWS = [(1, 8, 2), (255, 64, 16), (256, 64, 16), (257, 64, 16), (333, 128, 32), (100, 64, 64), (77, 48, 1), (40, 4096, 2)]


def rows_fwd(c, relu, stride=None, coff=0):
    n, C = c["N"], c["C"]
    return lambda xb: call("coocc_groupnorm_rows", ptr(xb, offset=coff), n, C, stride or C, c["groups"], ptr(D(xb.device, c["gamma"])),
                           ptr(D(xb.device, c["beta"])), c["eps"], relu)


def rows_bwd(c, relu, stride=None, coff=0):
    n, C = c["N"], c["C"]
    return lambda x, y, dy, dx, dgamma, dbeta: call(
        "coocc_groupnorm_rows_bwd", ptr(x, offset=coff), ptr(y, offset=coff), ptr(dy, offset=coff), n, C, stride or C, c["groups"],
        ptr(D(x.device, c["gamma"])), c["eps"], relu, ptr(dx, offset=coff), ptr(dgamma), ptr(dbeta))


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("n,C,groups", GN_ROWS)
def test_groupnorm_rows(dev, n, C, groups, kind):
    """(40, 4096, 2) is the backward's C limit: 2 * 4096 floats = 32 KB of dynamic LDS, within the 64 KB a workgroup may ask for
    without an attribute."""
    assert 2 * C * 4 <= 64 * 1024 and n <= 1024
    c = _gn_case(n, 1, C, groups, kind)
    for relu in (0, 1):
        gn_check(dev, c, relu, rows_fwd(c, relu), rows_bwd(c, relu), gn_depth_rows(n, groups), "groupnorm_rows %s %s relu %d" % (kind, (n, C, groups), relu))


@pytest.mark.parametrize("kind", KINDS)
def test_groupnorm_rows_on_a_column_range_of_wider_rows(dev, kind):
    """The head's form: 64 columns at column 128 of 192-wide rows; x, y, dy and dx all use that stride, every other column holds NaN
    and keeps it."""
    n, C, groups, stride, coff = 257, 64, 16, 192, 128
    c = _gn_case(n, 1, C, groups, kind)
    x, gamma, beta, eps = c["x"].view(n, C), c["gamma"], c["beta"], c["eps"]
    for relu in (0, 1):
        what = "groupnorm_rows %s strided relu %d" % (kind, relu)
        xb = padded(dev, x, stride, coff)
        rows_fwd(c, relu, stride, coff)(xb)
        a = (c["x"], groups, gamma, beta, eps, relu)
        yd = only_padding_is_nan(xb, C, coff, what + " y")
        R.assert_precise(yd.cpu().view(n, 1, C), R.gn_forward(*a, F64), R.gn_forward(*a, F32), what + " y")
        y, dy = c["y"][relu], c["dy"]
        dxb, dgamma, dbeta = nans(dev, n, stride), nans(dev, C), nans(dev, C)
        rows_bwd(c, relu, stride, coff)(padded(dev, x, stride, coff), padded(dev, y.view(n, C), stride, coff), padded(dev, dy.view(n, C), stride, coff),
                                        dxb, dgamma, dbeta)
        b = (c["x"], y, dy, groups, gamma, eps, relu)
        dx64, tg, tb = R.gn_backward(*b, F64)
        dx = only_padding_is_nan(dxb, C, coff, what + " dx")
        R.assert_precise(dx.cpu().view(n, 1, C), dx64, R.gn_backward(*b, F32)[0], what + " dx")
        R.assert_sum(dgamma.cpu(), tg, "f32", depth=gn_depth_rows(n, groups), what=what + " dgamma")
        R.assert_sum(dbeta.cpu(), tb, "f32", depth=gn_depth_rows(n, groups), what=what + " dbeta")


def test_groupnorm_rows_without_rows(dev):
    C = 64
    x, gamma, beta = nans(dev, C), torch.ones(C, device=dev), torch.zeros(C, device=dev)
    call("coocc_groupnorm_rows", ptr(x), 0, C, C, 16, ptr(gamma), ptr(beta), 1e-5, 1)
    dx, dgamma, dbeta = nans(dev, C), nans(dev, C), nans(dev, C)
    call("coocc_groupnorm_rows_bwd", ptr(x), ptr(x), ptr(x), 0, C, C, 16, ptr(gamma), 1e-5, 1, ptr(dx), ptr(dgamma), ptr(dbeta))
    torch.cuda.synchronize()
    assert bool(torch.isnan(x).all()) and bool(torch.isnan(dx).all()), "n = 0 wrote rows"
    assert float(dgamma.abs().max()) == 0.0 and float(dbeta.abs().max()) == 0.0, "n = 0: dgamma / dbeta are not zeroed"


GN_NHWC = [(1, 1, 8, 2), (2, 37, 64, 16), (3, 300, 128, 2), (2, 257, 32, 32), (40, 1, 64, 16)]


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("N,HW,C,groups", GN_NHWC)
def test_groupnorm_nhwc(dev, N, HW, C, groups, kind):
    assert C // groups <= 64 and N * HW <= 1024
    c = _gn_case(N, HW, C, groups, kind)
    for relu in (0, 1):
        fwd = lambda xb: call("coocc_groupnorm_nhwc", ptr(xb), N, HW, C, groups, ptr(D(dev, c["gamma"])), ptr(D(dev, c["beta"])), c["eps"], relu)
        bwd = lambda x, y, dy, dx, dgamma, dbeta: call("coocc_groupnorm_nhwc_bwd", ptr(x), ptr(y), ptr(dy), N, HW, C, groups, ptr(D(dev, c["gamma"])),
                                                       c["eps"], relu, ptr(dx), ptr(dgamma), ptr(dbeta))
        gn_check(dev, c, relu, fwd, bwd, gn_depth_nhwc(N, HW), "groupnorm_nhwc %s %s relu %d" % (kind, (N, HW, C, groups), relu))


# ============================================================================= coocc_conv_epilogue_bwd[_ex]
def epilogue(dev, dout, M, C, relu=0, out=None, scale=None, dacc=None, dres=None, dres_acc=0, dbias=None, dbias_acc=0, ws=None, ws_floats=None,
             amax=None, scale2=None, target=0.0, strides=None):
    """coocc_conv_epilogue_bwd_ex on device buffers; ``strides``: (dout, out, dacc, dres), C each by default."""
    sd, so, sa, sr = strides or (C, C, C, C)
    for t in (dout, out, dacc, dres, ws, scale):
        assert t is None or t.data_ptr() % 16 == 0
    call("coocc_conv_epilogue_bwd_ex", ptr(dout), sd, ptr(out), so, ptr(scale), M, C, relu, ptr(dacc), sa, ptr(dres), sr, dres_acc, ptr(dbias), dbias_acc,
         ptr(ws), (ws.numel() if ws is not None else 0) if ws_floats is None else ws_floats, ptr(amax), ptr(scale2), target)


def epi_inputs(M, C, seed):
    g = R.gen(seed)
    dy = R.no_subnormals(torch.randn(M, C, generator=g))
    return dict(dy=dy, dy_int=R.int_grad((M, C), g), y=R.clipped(torch.randn(M, C, generator=g)), start=torch.randn(M, C, generator=g),
                scale=torch.linspace(-2, 2, C) if C > 1 else torch.tensor([-1.5]))


# (C, (dout, out, dacc, dres) strides): whole dwordx4 rows, the same with padded strides, the scalar path, that with a padded dacc, C = 1
EPI_FORMS = [(64, (64, 64, 64, 64)), (64, (68, 72, 68, 76)), (6, (6, 6, 6, 6)), (6, (6, 6, 8, 6)), (1, (1, 1, 1, 1))]


@pytest.mark.parametrize("full", [True, False])
@pytest.mark.parametrize("C,strides", EPI_FORMS)
def test_epilogue_bwd_dacc_and_dres_are_exact(dev, C, strides, full):
    """M with M * ceil(C / 4) a multiple of the 256-thread block, and 37 rows; relu x scale x dres_accumulate."""
    c4 = R.cdiv(C, 4)
    M = 256 // c4 if full else 37
    assert (M * c4 % 256 == 0) == full
    c = epi_inputs(M, C, 31 * C + M)
    sd, so, sa, sr = strides
    dyb, yb = padded(dev, c["dy"], sd), padded(dev, c["y"], so)
    for relu in (0, 1):
        for scale in (None, c["scale"]):
            for acc in (0, 1):
                what = "epilogue_bwd C %d strides %s M %d relu %d scale %d accumulate %d" % (C, strides, M, relu, scale is not None, acc)
                dacc = nans(dev, M, sa)
                dres = padded(dev, c["start"], sr) if acc else nans(dev, M, sr)
                epilogue(dev, dyb, M, C, relu, yb, D(dev, scale) if scale is not None else None, dacc, dres, acc, strides=strides)
                dpre = R.masked(c["y"], c["dy"], relu)
                R.assert_exact(only_padding_is_nan(dres, C, what=what + " dres").cpu(), c["start"] + dpre if acc else dpre, what + " dres")
                R.assert_exact(only_padding_is_nan(dacc, C, what=what + " dacc").cpu(), dpre * scale if scale is not None else dpre, what + " dacc")
    # dacc alone and dres alone
    dacc, dres = nans(dev, M, sa), nans(dev, M, sr)
    epilogue(dev, dyb, M, C, 1, yb, None, dacc, None, strides=strides)
    epilogue(dev, dyb, M, C, 1, yb, None, None, dres, strides=strides)
    R.assert_exact(only_padding_is_nan(dacc, C).cpu(), R.masked(c["y"], c["dy"], 1), "dacc alone")
    R.assert_exact(only_padding_is_nan(dres, C).cpu(), R.masked(c["y"], c["dy"], 1), "dres alone")


def dbias(dev, c, M, C, relu, dy, fast, start=None, stride=None):
    """The bias gradient alone (dacc and dres null).  ``fast``: a workspace of 2^16 floats; else one that suffices for the generic
    form only, (M + 255) / 256 * C floats."""
    ws = torch.empty(1 << 16, device=dev)
    out = D(dev, start).clone() if start is not None else nans(dev, C)
    s = stride or C
    epilogue(dev, padded(dev, dy, s), M, C, relu, padded(dev, c["y"], s), dbias=out, dbias_acc=int(start is not None), ws=ws,
             ws_floats=None if fast else R.cdiv(M, 256) * C, strides=(s, s, C, C))
    return out


DBIAS = [("fast", 1100, 64, True), ("fast, 66 blocks", 4161, 128, True), ("generic by C", 1000, 24, True),
         ("generic by the workspace", 1000, 64, False), ("fast, one lane", 130, 1024, True), ("generic, two channel blocks", 257, 260, True)]


@pytest.mark.parametrize("name,M,C,roomy", DBIAS)
def test_epilogue_bwd_bias_gradient(dev, name, M, C, roomy):
    """k_colsum_part / k_colsum_final (generic): 256 sequential fp32 additions within a part, then one per part: depth 256 + nparts;
    those cases keep at most 1024 rows."""
    fast = R.col_fast(C) and roomy
    assert fast == name.startswith("fast")
    c = epi_inputs(M, C, 17 * C + M)
    start = c["start"][0]
    assert fast or M <= 1024
    form = dict(form="f64") if fast else dict(form="f32", depth=min(M, 256) + R.cdiv(M, 256))
    for relu in (0, 1):
        for stride in (C, C + 4):
            what = "dbias %s %dx%d relu %d stride %d" % (name, M, C, relu, stride)
            terms = R.masked(c["y"], c["dy"], relu, F64)
            d0 = dbias(dev, c, M, C, relu, c["dy"], roomy, stride=stride)
            R.assert_sum(d0.cpu(), terms, what=what, **form)
            assert R.bits_equal(d0, dbias(dev, c, M, C, relu, c["dy"], roomy, stride=stride)), what + ": two calls on the same inputs differ"
            d1 = dbias(dev, c, M, C, relu, c["dy"], roomy, start=start, stride=stride)
            R.assert_sum(d1.cpu(), terms, start=start, what=what + " accumulate", **form)
            R.assert_exact(d1.cpu(), start + d0.cpu(), what + ": accumulate = 1 is not dbias + the accumulate = 0 result")
            di = dbias(dev, c, M, C, relu, c["dy_int"], roomy, stride=stride)
            R.assert_int_sum(di.cpu(), R.masked(c["y"], c["dy_int"], relu, F64), what=what + " integer")
            istart = torch.arange(C, dtype=F32) - 7
            di = dbias(dev, c, M, C, relu, c["dy_int"], roomy, start=istart, stride=stride)
            R.assert_int_sum(di.cpu(), R.masked(c["y"], c["dy_int"], relu, F64), start=istart, what=what + " integer accumulate")


def test_epilogue_bwd_bias_gradient_takes_the_form_its_workspace_allows(dev):
    """The column [2^24, 1 x 200, -2^24] within one 256-row part sums to 200 in fp64 (the fast form) and to 0 by sequential fp32
    additions (2^24 + 1 rounds back to 2^24: the generic form) -- both within their bounds, so only this probe tells which ran."""
    M, C = 300, 64
    dy = torch.zeros(M, C)
    dy[0], dy[1:201], dy[201] = 2.0 ** 24, 1.0, -2.0 ** 24
    c = dict(y=torch.ones(M, C))
    for relu in (0, 1):
        got = dbias(dev, c, M, C, relu, dy, True).cpu()
        assert bool((got == 200.0).all()), "a roomy workspace: the fast (fp64) form, got %r" % got[:4].tolist()
        got = dbias(dev, c, M, C, relu, dy, False).cpu()
        assert bool((got == 0.0).all()), "a workspace for the generic form only: the fp32 form, got %r" % got[:4].tolist()
    got = dbias(dev, dict(y=torch.ones(M, 24)), M, 24, 0, dy[:, :24].contiguous(), True).cpu()
    assert bool((got == 0.0).all()), "C = 24: the generic form, got %r" % got[:4].tolist()


# ----------------------------------------------------------------------------- the device-made gradient scale
TARGET = ag.TRAIN_H2_GRAD_TARGET
AMAXES = [1e-30, 6e-8, 1 - 2.0 ** -24, 1.0, 1 + 2.0 ** -23, 1023.9, 1024.0, 3e3, 1e30]


def scaled(dev, dy, y=None, relu=0, scale=None):
    """(dacc, scale2 on the host, the amax words) of one coocc_conv_epilogue_bwd_ex pass with the operand scale asked for."""
    M, C = dy.shape
    words = torch.zeros(2048, dtype=torch.int32, device=dev)          # COOCC_AMAX_WORDS
    dacc, scale2 = nans(dev, M, C), nans(dev, 2)
    epilogue(dev, D(dev, dy), M, C, relu, D(dev, y) if y is not None else None, D(dev, scale) if scale is not None else None, dacc,
             amax=words, scale2=scale2, target=TARGET)
    return dacc, scale2.cpu(), words


def check_scale(scale2, words, amax, what):
    k = R.amax_k(amax, TARGET)
    assert scale2.tolist() == [2.0 ** k, 2.0 ** -k], "%s: scale2 %r, k = %d by the kernel's rule" % (what, scale2.tolist(), k)
    assert int(words.abs().max()) == 0, what + ": the amax words are not left zero"
    return k


@pytest.mark.parametrize("where", ["row 0", "the last row", "block 66", "the tail block"])
def test_gradient_scale_follows_the_kernels_rule(dev, where):
    """M = 1100, C = 64: 69 workgroups of 16 rows, so workgroups 64 .. 68 share the slots of 0 .. 4 and the last one has dead threads."""
    M, C = 1100, 64
    row, col = {"row 0": (0, 0), "the last row": (M - 1, C - 1), "block 66": (66 * 16 + 3, 17), "the tail block": (68 * 16 + 5, 40)}[where]
    assert R.cdiv(M * C // 4, 256) == 69 and M * C // 4 % 256 != 0
    lo, hi = R.amax_interval(TARGET)
    assert (lo, hi) == (1024.0, 2048.0)
    g = R.gen(5)
    shape = (torch.rand(M, C, generator=g) * 0.5 + 0.25) * (torch.randint(0, 2, (M, C), generator=g) * 2 - 1).float()      # 0.25 <= |.| < 0.75
    for amax in AMAXES:
        a32 = float(torch.tensor(amax, dtype=F32))
        dy = shape * a32
        dy[row, col] = -a32
        assert float(dy.abs().max()) == a32 and not bool(((dy != 0) & (dy.abs() < R.TINY)).any())
        dacc, scale2, words = scaled(dev, dy)
        k = check_scale(scale2, words, a32, "amax %g in %s" % (amax, where))
        assert abs(k) == 100 or lo <= a32 * 2.0 ** k < hi, (amax, k)
        R.assert_exact(dacc.cpu(), dy, "dacc beside the scale")


def test_gradient_scale_edges(dev):
    M, C = 37, 64
    g = R.gen(6)
    zero = torch.zeros(M, C)
    # an all-zero gradient and an infinite one: {1, 1}
    for name, v in (("zero", 0.0), ("infinite", float("inf")), ("minus infinite", float("-inf"))):
        dy = zero.clone()
        dy[20, 33] = v
        _, scale2, words = scaled(dev, dy)
        assert scale2.tolist() == [1.0, 1.0] and int(words.abs().max()) == 0, (name, scale2.tolist())
    # the clamp of k at +-100 (1e-38 lies below the smallest normal float: nothing else in that gradient, which is zero elsewhere)
    for v, k in ((1e-38, 100), (1e-30, 100), (1e35, -100)):
        dy = zero.clone()
        dy[36, 63] = v
        _, scale2, words = scaled(dev, dy)
        assert R.amax_k(v, TARGET) == k
        check_scale(scale2, words, v, "amax %g" % v)
    # the amax is that of dacc = dpre * scale, after the mask: row 0 holds the largest |dy| but is clipped by its ReLU, so neither its
    # own threads nor the dead threads of the tail block (which re-read row 0) may contribute it
    dy = R.no_subnormals(torch.randn(M, C, generator=g))
    y = R.clipped(torch.randn(M, C, generator=g))
    dy[0], y[0] = 1e6, 0.0
    y[0, ::2] = -0.0
    scale = torch.linspace(0.5, 3, C)
    dacc, scale2, words = scaled(dev, dy, y, 1, scale)
    want = R.masked(y, dy, 1) * scale
    R.assert_exact(dacc.cpu(), want, "dacc with mask and scale")
    assert float(want.abs().max()) < 100
    check_scale(scale2, words, float(want.abs().max()), "amax of the masked, scaled gradient")
    # ... and unmasked, row 0 decides
    _, scale2, words = scaled(dev, dy, y, 0, scale)
    check_scale(scale2, words, float((dy * scale).abs().max()), "amax with row 0 live")
