"""The split-f16 weight gradient over a row table (``coocc_conv_wgrad_h2t``, csrc/wgrad_h2t.hip) on the GPU: the kernel through the
C ABI against float64 at its own precision (``util.assert_precise`` per tap: anchors fp32 and the engine's split restatement), the
device-chosen gradient scale and the range guard, one layer and the whole ``SparseEncoderHD`` under ``train()`` with
``lidar_hd.HD_WGRAD_H2`` set (weight gradients within ``util.TOL`` of float64, everything else bit-equal to the knob-off run), and
the co-runner guard beside split-f16 GEMMs of a second stream."""
import contextlib
import math

import numpy as np
import pytest
import torch

from co_occ_amd import autograd as ag, core, lidar, lidar_hd
from co_occ_amd._lib import CooccRangeError, call, ptr
from co_occ_amd.lidar_hd import SparseEncoderHD

import test_gpu_sparse_hd as T
import test_gpu_sparse_hd_train as TT
import util
import wgrad_h2t_cases as W

pytestmark = pytest.mark.gpu

bits_equal = TT.bits_equal


@contextlib.contextmanager
def knob(on, engine="h2"):
    """``lidar_hd.HD_WGRAD_H2`` and ``core.CONV_ENGINE`` for the block, restored after."""
    old = lidar_hd.HD_WGRAD_H2, core.CONV_ENGINE
    lidar_hd.HD_WGRAD_H2, core.CONV_ENGINE = bool(on), engine
    try:
        yield
    finally:
        lidar_hd.HD_WGRAD_H2, core.CONV_ENGINE = old


def wgrad_h2t(x, dy, tb, scale2=None, dw=None, accumulate=0):
    (in_rows, Cin), (M, Cout), taps = x.shape, dy.shape, tb.shape[0]
    if dw is None:
        dw = torch.full((Cout, Cin, taps), float("nan"), device=x.device)
    ws = core.workspace(x.device)
    call("coocc_conv_wgrad_h2t", ptr(x), in_rows, Cin, ptr(dy), Cout, ptr(tb), M, Cin, Cout, taps, ptr(scale2), ptr(dw), accumulate,
         ptr(ws), ws.numel())
    return dw


def judge(dw, x, dy, tb, what, s=1.0, start=None):
    """``dw`` [Cout, Cin, taps] per tap against float64 (+ ``start``, the dw accumulated onto, rounded into the anchors); the split
    restatement is taken on dy * s, as the kernel takes it."""
    dw = dw.cpu()
    for t in range(tb.shape[0]):
        xg = W.gathered(x, tb[t]).t()
        r64, r32, _ = util.gemm_refs([(xg, dy)], split=False)
        rs = (util.split_mm(xg, dy.double() * s) / s).float()
        if start is not None:
            st = start[:, :, t].t()
            r64, r32, rs = r64 + st.double(), r32 + st, (rs.double() + st.double()).float()
        util.assert_precise(dw[:, :, t].t(), r64, r32, rs, what="%s tap %d" % (what, t))


# ----------------------------------------------------------------------------- a. the kernel against float64
@pytest.mark.parametrize("M", [1, 15, 16, 17, 33, 4099])
@pytest.mark.parametrize("taps", [1, 27])
@pytest.mark.parametrize("Cin,Cout", [(32, 32), (32, 64), (64, 64), (64, 128), (128, 128)])
def test_kernel_matches_float64_at_its_own_precision(dev, Cin, Cout, taps, M):
    """Step edges (M around 16 and 32), several slices (4099 rows at a 256-row minimum), every tile form; in_rows != M; about 30 %
    live entries, one all-dead tap (exact zeros), one dead 16-row run; accumulate 0 and 1; two calls bit-equal."""
    in_rows = M + 37
    g = torch.Generator().manual_seed(1000 * Cin + 10 * Cout + taps + M)
    x, dy = torch.randn(in_rows, Cin, generator=g), torch.randn(M, Cout, generator=g)
    tb = W.book(taps, M, in_rows, seed=M + taps)
    xd, dyd, tbd = x.to(dev), dy.to(dev), torch.from_numpy(tb).to(dev)
    what = "wgrad_h2t %d->%d taps %d M %d" % (Cin, Cout, taps, M)
    dw0 = wgrad_h2t(xd, dyd, tbd)
    dw0b = wgrad_h2t(xd, dyd, tbd)
    start = torch.randn(Cout, Cin, taps, generator=g)
    dw1 = wgrad_h2t(xd, dyd, tbd, dw=start.to(dev), accumulate=1)
    torch.cuda.synchronize()
    core.check_h2_overflow()
    assert bits_equal(dw0, dw0b), what + ": two calls on the same inputs differ"
    judge(dw0, x, dy, tb, what)
    if W.dead_tap(taps) is not None:
        assert float(dw0[:, :, W.dead_tap(taps)].abs().max()) == 0.0, what + ": the all-dead tap"
    judge(dw1, x, dy, tb, what + " accumulate", start=start)
    assert bits_equal(dw1, start.to(dev) + dw0), what + ": accumulate = 1 is not dw + the accumulate = 0 result"


# ----------------------------------------------------------------------------- b. the gradient scale and the range guard
def _scaled(dev, dy):
    """dacc (a copy of dy) and the device pair {s, 1/s} of ``coocc_conv_epilogue_bwd_ex``."""
    M, C = dy.shape
    dacc, scale2 = torch.empty_like(dy), torch.empty(2, device=dev)
    ws = core.workspace(dev)
    call("coocc_conv_epilogue_bwd_ex", ptr(dy), C, None, C, None, M, C, 0, ptr(dacc), C, None, C, 0, None, 0, ptr(ws), ws.numel(),
         ptr(ag._amax_word(dev)), ptr(scale2), ag.TRAIN_H2_GRAD_TARGET)
    return dacc, scale2


@pytest.mark.parametrize("mag", [1e-7, 1e3])
def test_gradient_scale_keeps_the_precision_and_the_guard_fires(dev, mag):
    Cin = Cout = 64
    taps, M, in_rows = 27, 300, 337
    g = torch.Generator().manual_seed(77)
    x, dy = torch.randn(in_rows, Cin, generator=g), torch.randn(M, Cout, generator=g) * mag
    tb = W.book(taps, M, in_rows, seed=9)
    xd, tbd = x.to(dev), torch.from_numpy(tb).to(dev)
    dacc, scale2 = _scaled(dev, dy.to(dev))
    dw = wgrad_h2t(xd, dacc, tbd, scale2=scale2)
    torch.cuda.synchronize()
    core.check_h2_overflow()
    s, inv = (float(v) for v in scale2.cpu())
    amax = float(dy.abs().max())
    # a power of two and its inverse, that bring max |dacc| into [target, 2 target): far above f16's subnormals, under the guard
    assert s * inv == 1.0 and math.frexp(s)[0] == 0.5 and ag.TRAIN_H2_GRAD_TARGET <= amax * s < 2 * ag.TRAIN_H2_GRAD_TARGET, (s, inv, amax)
    assert bits_equal(dacc, dy.to(dev))
    judge(dw, x, dy, tb, "wgrad_h2t scaled |dacc| %g" % mag, s=s)
    # one value of `in` beyond the 16-bit operand range, in a row the book reads
    row = int(tb[0][tb[0] >= 0][0])
    xd[row, 3] = 4e4
    wgrad_h2t(xd, dacc, tbd, scale2=scale2)
    torch.cuda.synchronize()
    with pytest.raises(CooccRangeError):
        core.check_h2_overflow()
    core.check_h2_overflow()                  # ... and the flag was reset


# ----------------------------------------------------------------------------- c. one layer
REGION, REGION_F32 = "k_wgrad_h2t<sparse hd table>", "k_wgrad<sparse hd table>"


def _layer(kind):
    if kind not in TT._LAYER:
        TT._LAYER[kind] = TT._layer_case(kind)
    return TT._LAYER[kind]


def test_down_layer_takes_the_new_wgrad_and_nothing_else_changes(dev):
    c = _layer("down")
    r64, r32 = c["refs"][torch.float64], c["refs"][torch.float32]
    with knob(False):
        off, names_off = TT._run_layer(dev, c, False)
        off = {k: (v.clone() if torch.is_tensor(v) else v) for k, v in off.items()}
    with knob(True):
        on, names_on = TT._run_layer(dev, c, False)
    assert names_off.get(REGION_F32) == 1 and REGION not in names_off, names_off
    assert names_on.get(REGION) == 1 and REGION_F32 not in names_on, names_on
    assert tuple(on["dw"].shape) == tuple(c["w"].shape), "dW comes back in the v1 layout"
    TT._cmp(on["dw"].cpu(), r64["dw"], r32["dw"], "down h2 wgrad_h2=1 dw")
    for key in ("y", "dx", "dgamma", "dbeta"):
        assert bits_equal(on[key], off[key]), key + " changed with the knob"


def test_subm16_layer_and_the_fp32_engine_keep_the_fp32_wgrad(dev):
    c = _layer("subm16")
    with knob(True):
        g, names = TT._run_layer(dev, c, False)
    assert names.get(REGION_F32) == 1 and REGION not in names, names
    r64, r32 = c["refs"][torch.float64], c["refs"][torch.float32]
    TT._cmp(g["dw"].cpu(), r64["dw"], r32["dw"], "subm16 h2 wgrad_h2=1 dw")
    c = _layer("down")
    with knob(False, "f32"):
        off, names_off = TT._run_layer(dev, c, False)
        off = {k: (v.clone() if torch.is_tensor(v) else v) for k, v in off.items()}
    with knob(True, "f32"):
        on, names_on = TT._run_layer(dev, c, False)
    assert names_on == names_off and REGION not in names_on and names_on.get(REGION_F32) == 1, (names_on, names_off)
    for key in ("y", "dx", "dw", "dgamma", "dbeta"):
        assert bits_equal(on[key], off[key]), "engine f32: %s changed with the knob" % key


# ----------------------------------------------------------------------------- d. the whole module
def _module_run(dev, c, on):
    m = SparseEncoderHD(**c["cfg"])
    m.load_state_dict(c["sd"], strict=True)
    m = m.to(dev).train()
    m.train_enabled = True
    m.wide16 = True
    f = c["feats"].to(dev).requires_grad_()
    with knob(on):
        with util.kernels() as names:
            y = m(f, c["coors"].to(dev), 1)
            (y * c["gout"].to(dev)).sum().backward()
    core.check_h2_overflow()
    return m, y.detach(), f.grad, names


@pytest.mark.parametrize("kind", list(T.MODULE_CFGS))
def test_module_under_train_with_the_new_wgrad(dev, kind):
    c = TT._module_case(kind)
    r64, r32 = c["refs"][torch.float64], c["refs"][torch.float32]
    _, y_off, df_off, names_off = _module_run(dev, c, False)
    m, y_on, df_on, names_on = _module_run(dev, c, True)
    assert REGION not in names_off
    assert bits_equal(y_on, y_off) and bits_equal(df_on, df_off), "y / dfeats changed with the knob"
    want = sum(1 for mod in m.modules() if isinstance(mod, lidar_hd.SparseConvV1) and lidar._pad4(mod.cin) % 32 == 0 and mod.cout % 32 == 0)
    total = sum(1 for mod in m.modules() if isinstance(mod, lidar_hd.SparseConvV1))
    assert 0 < want < total
    assert names_on.get(REGION, 0) == want and names_on.get(REGION_F32, 0) == total - want, (names_on, want, total)
    for k, p in m.named_parameters():
        assert p.grad is not None and tuple(p.grad.shape) == tuple(p.shape), k
        TT._cmp(p.grad.cpu(), r64[k + ".grad"], r32[k + ".grad"], "%s h2 wgrad_h2=1 %s.grad" % (kind, k))


def test_module_under_train_on_an_empty_cloud_with_the_new_wgrad(dev):
    m = SparseEncoderHD(**T.MODULE_CFGS["basicblock"]).to(dev).train()
    m.train_enabled = True
    f = torch.zeros(0, 4, device=dev, requires_grad=True)
    with knob(True):
        y = m(f, torch.zeros(0, 3, dtype=torch.int32, device=dev), 1)
        y.sum().backward()
    assert float(y.detach().abs().max()) == 0.0 and tuple(f.grad.shape) == (0, 4)
    for k, p in m.named_parameters():
        assert p.grad is not None and float(p.grad.abs().max()) == 0.0, k


# ----------------------------------------------------------------------------- e. co-runner guard
N_CALLS = 20


def test_kernel_is_bit_stable_beside_split_f16_gemms(dev):
    """In the manner of tests/test_gpu_sparse_hd_train.py: 20 calls at M = 60 000, 64 -> 64, 27 taps on one stream beside split-f16
    pointwise layers of a second stream give the bits of the run alone."""
    g = torch.Generator().manual_seed(11)
    xb = core.to_rows(torch.randn(1, 128, 100, 100, 8, generator=g).to(dev))
    pc = core.PackedConv((torch.randn(128, 128, 1, 1, 1, generator=g) * 0.05).to(dev), ksize=1, pad=0)
    M, in_rows, C, taps = 60000, 61000, 64, 27
    x, dy = torch.randn(in_rows, C, generator=g).to(dev), torch.randn(M, C, generator=g).to(dev)
    tb = torch.from_numpy(W.book(taps, M, in_rows, seed=4)).to(dev)
    s0, s1 = torch.cuda.Stream(device=dev), torch.cuda.Stream(device=dev)
    with torch.no_grad():
        core.conv_rows(xb, pc, relu=False)
        torch.cuda.synchronize()
        with torch.cuda.stream(s0):
            ref = wgrad_h2t(x, dy, tb)
        torch.cuda.synchronize()
        assert bool(torch.isfinite(ref).all()) and float(ref.abs().max()) > 0.0
        got = []
        for _ in range(N_CALLS):
            with torch.cuda.stream(s1):
                for _ in range(4):
                    core.conv_rows(xb, pc, relu=False)
            with torch.cuda.stream(s0):
                got.append(wgrad_h2t(x, dy, tb))
        torch.cuda.synchronize()
    core.check_h2_overflow()
    bad = sum(int(not bits_equal(ref, t)) for t in got)
    assert bad == 0, "coocc_conv_wgrad_h2t beside split-f16 GEMMs: %d of %d calls differ from the run alone" % (bad, N_CALLS)
