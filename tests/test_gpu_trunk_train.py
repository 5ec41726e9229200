"""Training of the LiDAR-only trunk on the GPU (``lidar_trunk.run_trunk_train``, co_occ_amd/autograd.py, csrc/conv_bwd.hip's row
tables, csrc/trunk_train.hip): the per-axis row tables against a numpy brute-force book, the backward of the sum kernel bit for bit, one anisotropic layer and one
deblock against float64 torch autograd, a small whole trunk against the plain-torch restatement (tests/ref_second3d.py) under
``train()``, the detector's ``train_lidar_trunk`` option end to end, and the co-runner guard of the new re-layout kernel."""
import copy
import ctypes

import numpy as np
import pytest
import torch
import torch.nn.functional as F
from torch import nn

import co_occ_amd as pkg
import co_occ_amd.synth as synth
from co_occ_amd import autograd as ag, core, lidar_trunk as lt
from co_occ_amd._lib import call, ptr

import ref_second3d
import util
from util_second3d import bits_equal, conv_taps_axes

pytestmark = pytest.mark.gpu


# ------------------------------------------------------------------ a. the per-axis row tables
def book(B, dims, kernel, strides, pads):
    """Brute force over every (output voxel, tap): (forward table [taps, Mo], dgrad table [taps, Mi]) of int32, -1 where empty."""
    (Xi, Yi, Zi), (kx, ky, kz), (sx, sy, sz), (px, py, pz) = dims, kernel, strides, pads
    Xo, Yo, Zo = (Xi + 2 * px - kx) // sx + 1, (Yi + 2 * py - ky) // sy + 1, (Zi + 2 * pz - kz) // sz + 1
    fwd = -np.ones((kx * ky * kz, B * Xo * Yo * Zo), np.int32)
    dg = -np.ones((kx * ky * kz, B * Xi * Yi * Zi), np.int32)
    for b in range(B):
        for ox in range(Xo):
            for oy in range(Yo):
                for oz in range(Zo):
                    o = ((b * Xo + ox) * Yo + oy) * Zo + oz
                    for dx in range(kx):
                        for dy in range(ky):
                            for dz in range(kz):
                                ix, iy, iz = ox * sx - px + dx, oy * sy - py + dy, oz * sz - pz + dz
                                if 0 <= ix < Xi and 0 <= iy < Yi and 0 <= iz < Zi:
                                    i, t = ((b * Xi + ix) * Yi + iy) * Zi + iz, (dx * ky + dy) * kz + dz
                                    fwd[t, o], dg[t, i] = i, o
    return fwd, dg, (Xo, Yo, Zo)


def _table3(dev, B, dims, kernel, strides, pads, dgrad):
    return ag.tap_table(dev, B, *dims, tuple(kernel), tuple(strides), tuple(pads), dgrad).cpu().numpy()


# 3x3x1 kernels at strides (s, s, 1) on every grid, and the cubic geometries of the decoder trunk on (6, 5, 3)
_GRIDS = [(9, 7, 2), (8, 8, 1), (6, 5, 3)]
_BOOKS = [pytest.param(g, (3, 3, 1), (s, s, 1), (1, 1, 0), id="grid%d-%d" % (i, s)) for s in (1, 2, 4) for i, g in enumerate(_GRIDS)] + \
         [pytest.param((6, 5, 3), (k,) * 3, (s,) * 3, (k // 2,) * 3, id="cubic-k%d-s%d" % (k, s)) for k, s in ((3, 1), (3, 2), (1, 2))]


@pytest.mark.parametrize("grid, kernel, strides, pads", _BOOKS)
def test_tap_table3_equals_the_brute_force_book(dev, grid, kernel, strides, pads):
    B, s = 2, strides[0]
    fwd, dg, _ = book(B, grid, kernel, strides, pads)
    assert np.array_equal(_table3(dev, B, grid, kernel, strides, pads, False), fwd)
    got = _table3(dev, B, grid, kernel, strides, pads, True)
    assert np.array_equal(got, dg)
    if grid[0] == 9 and s == 4:
        X, Y, Z = grid
        x = (np.arange(B * X * Y * Z) // (Y * Z)) % X
        dead = (x == 2) | (x == 6)                     # o*4 - 1 + d = 2 or 6 has no solution with d in 0..2
        assert dead.sum() == 2 * B * Y * Z and (got[:, dead] == -1).all(), "input columns 2 and 6 are read by no output"
        assert (got[:, (x == 3)] >= 0).any()


@pytest.mark.parametrize("stride", [1, 2])
@pytest.mark.parametrize("k", [3, 1])
def test_tap_table3_with_cubic_arguments_is_the_scalar_table(dev, k, stride):
    """The two C entries on the same grid, bit for bit: ``coocc_conv_tap_table`` is ``coocc_conv_tap_table3`` with equal triples,
    its extent check included."""
    B, (X, Y, Z), pad = 2, (6, 5, 3), k // 2
    Xo, Yo, Zo = (core.out_dim(n, k, stride, pad) for n in (X, Y, Z))
    for dgrad in (False, True):
        M = B * X * Y * Z if dgrad else B * Xo * Yo * Zo
        want = torch.full((k ** 3, M), -7, dtype=torch.int32, device=dev)
        got = torch.full((k ** 3, M), -9, dtype=torch.int32, device=dev)
        call("coocc_conv_tap_table", B, X, Y, Z, Xo, Yo, Zo, k, stride, pad, int(dgrad), ptr(want))
        call("coocc_conv_tap_table3", B, X, Y, Z, Xo, Yo, Zo, k, k, k, stride, stride, stride, pad, pad, pad, int(dgrad), ptr(got))
        assert torch.equal(got, want) and int(got.min()) >= -1 and int(got.max()) >= 0
    t = torch.empty(27, 100, dtype=torch.int32, device=dev)
    with pytest.raises(pkg._lib.CooccArgError, match="extents"):
        call("coocc_conv_tap_table3", 1, 9, 7, 2, 2, 2, 2, 3, 3, 1, 4, 4, 1, 1, 1, 0, 0, ptr(t))
    with pytest.raises(pkg._lib.CooccArgError, match="extents"):           # (6 + 2 - 3) // 2 + 1 = 3 outputs along x, not 2
        call("coocc_conv_tap_table", 1, 6, 5, 3, 2, 3, 2, 3, 2, 1, 0, ptr(t))


# ------------------------------------------------------------------ b. backward of the sum kernel
def _relayout(dout, B, X, Y, Z, C, s):
    """Index restatement: fine row (b, x, y, z) -> row ((b, x // s, y // s, z), child (x % s) * s + y % s) of the level's layout."""
    r = torch.arange(B * X * Y * Z)
    z, y, x, b = r % Z, (r // Z) % Y, (r // (Z * Y)) % X, r // (Z * Y * X)
    crow = ((b * (X // s) + x // s) * (Y // s) + y // s) * Z + z
    out = torch.full((B * (X // s) * (Y // s) * Z * s * s, C), float("nan"))
    out[crow * s * s + (x % s) * s + y % s] = dout
    return out.view(-1, s * s * C)


@pytest.mark.parametrize("C", [4, 12])
@pytest.mark.parametrize("grid, strides", [((8, 8, 3), (1, 2, 4)), ((8, 8, 3), (2,)), ((8, 8, 3), (1, 2, 4, 8)), ((6, 10, 1), (1, 2))])
def test_fpn_sum_bwd_is_the_exact_relayout_and_the_adjoint_of_the_sum(dev, grid, strides, C):
    B, (X, Y, Z) = 2, grid
    g = torch.Generator().manual_seed(7 * C + len(strides))
    ups = [torch.randn(B * (X // s) * (Y // s) * Z, s * s * C, generator=g).to(dev).requires_grad_() for s in strides]
    dout = torch.randn(B * X * Y * Z, C, generator=g)
    with util.kernels() as names:
        out = ag.fpn_sum_rows(ups, strides, C, (B, X, Y, Z))
        out.backward(dout.to(dev))
    assert names.get("k_fpn_sum") == 1 and names.get("k_fpn_sum_bwd", 0) == (1 if any(s > 1 for s in strides) else 0), names
    for u, s in zip(ups, strides):
        want = _relayout(dout, B, X, Y, Z, C, s)
        assert not torch.isnan(want).any() and bits_equal(u.grad.cpu(), want), "level stride %d" % s
    # <dups, ups> == <dout, sum(ups)>: the sum is linear, its backward the adjoint; the kernel's sum is the fp32 chain of
    # len(strides) additions, each within 2^-24 of its partial sum, itself bounded by the sum of the |levels|
    lhs = sum(float((u.grad.double() * u.detach().double()).sum()) for u in ups)
    rhs = float((dout.double() * out.detach().cpu().double()).sum())
    with torch.no_grad():
        mag = ag.fpn_sum_rows([u.detach().abs() for u in ups], strides, C, (B, X, Y, Z)).cpu().double()
    bound = len(strides) * 2.0 ** -24 * float((dout.abs().double() * mag).sum())
    assert abs(lhs - rhs) <= bound, (lhs, rhs, bound)


# ------------------------------------------------------------------ c. one anisotropic layer
def _gather(rows, idx):
    """rows[idx] with zeros where idx < 0."""
    out = rows[torch.as_tensor(idx).clamp(min=0).long()].clone()
    out[torch.as_tensor(idx) < 0] = 0
    return out


@pytest.mark.parametrize("Cin, Cout", [(32, 64), (8, 12)])
@pytest.mark.parametrize("s", [1, 2, 4])
@pytest.mark.parametrize("grid, res", [pytest.param((9, 7, 2), False, id="grid0"), pytest.param((8, 8, 1), False, id="grid1"),
                                       pytest.param((8, 8, 1), True, id="grid1-res")])
def test_anisotropic_layer_forward_dgrad_wgrad_against_float64(dev, monkeypatch, grid, res, s, Cin, Cout):
    """3x3x1 kernel, strides (s, s, 1), pads (1, 1, 0), conv + ReLU: forward, dx and dW against float64 autograd of F.conv3d with
    the ReLU mask of the kernel's own forward (as ``util.train_judge``), judged by ``util.assert_precise``.  Anchors: the fp32
    evaluation in the MFMA's accumulation order (chain = 2) and, on the split-f16 routes, the split emulation with the gradient
    operand scaled as the device scales it.  (32, 64) takes the split-f16 GEMMs (with the flop floor lifted, as the precision tests
    do), (8, 12) the fp32-MFMA ones; the strided dgrad and the weight gradient are fp32-MFMA launches on either.  ``res``: a random
    [Mo, Cout] residual added before the ReLU -- the float64 reference adds it too, and its gradient is dy under the ReLU mask,
    bit for bit (the epilogue's backward copies it)."""
    monkeypatch.setattr(core, "H2_DIRECT_MIN_FLOPS", 0.0)
    h2 = Cin % 32 == 0
    kernel, strides, pads = (3, 3, 1), (s, s, 1), (1, 1, 0)
    X, Y, Z = grid
    gen = torch.Generator().manual_seed(100 * s + Cin + X)
    x = torch.randn(1, Cin, X, Y, Z, generator=gen)
    w = torch.randn(Cout, Cin, 3, 3, 1, generator=gen) * (2.0 / (9 * Cin)) ** 0.5
    fwd, dg, (Xo, Yo, Zo) = book(1, grid, kernel, strides, pads)
    up = torch.randn(1, Cout, Xo, Yo, Zo, generator=gen)
    r2 = torch.randn(Xo * Yo * Zo, Cout, generator=gen) if res else None
    xd = util.ncdhw_rows(x).contiguous().to(dev).requires_grad_()
    wd = w.to(dev).requires_grad_()
    rd = r2.to(dev).requires_grad_() if res else None
    with util.kernels() as names:
        yd, go = ag.conv_bn_rows(xd, wd, (1, X, Y, Z), stride=strides, relu=True, res2d=rd)
        yd.backward(util.ncdhw_rows(up).contiguous().to(dev))
    core.check_h2_overflow()
    assert go == (1, Xo, Yo, Zo)
    if h2:
        assert names.get("k_gemm_h2 conv_fwd") == 1, names
        assert (names.get("k_gemm_h2 conv_dgrad") == 1 and "conv_dgrad" not in names) if s == 1 else \
            (names.get("conv_dgrad", 0) >= 1 and "k_gemm_h2 conv_dgrad" not in names), names
    else:
        assert names.get("conv_fwd") == 1 and names.get("conv_dgrad", 0) >= 1 and not any(n.startswith("k_gemm_h2") for n in names), names
    assert names.get("k_wgrad") == 1, names
    if s == 4:                  # classes (x mod 4, y mod 4) with a 2 are reached through no tap: 3 x 3 classes at most
        assert names["conv_dgrad"] <= 9, names
    # forward
    r64, r32, rs = util.gemm_refs(conv_taps_axes(x, w, strides), chain=2, split=h2, res=r2, relu=True)
    yk = yd.detach().cpu()
    util.assert_precise(yk, r64, r32, rs, what="aniso fwd s%d %s %d->%d res=%s" % (s, grid, Cin, Cout, res))
    # backward, ReLU mask of the kernel's own forward
    dy_rows = util.ncdhw_rows(up) * (yk > 0)
    if res:                     # the masked entries are +0 (a select; the product dy * 0 would carry dy's sign into the zero)
        assert bits_equal(rd.grad.cpu(), torch.where(yk > 0, util.ncdhw_rows(up), torch.zeros(()))) and torch.equal(rd.grad.cpu(), dy_rows), \
            "the residual's gradient is dy under the ReLU mask, bit for bit"
    dy = dy_rows.view(1, Xo, Yo, Zo, Cout).permute(0, 4, 1, 2, 3)
    xa, wa = x.double().requires_grad_(), w.double().requires_grad_()
    F.conv3d(xa, wa, stride=strides, padding=pads).backward(dy.double())
    dx64, dw64 = util.ncdhw_rows(xa.grad), wa.grad
    amax = float(dy.abs().max())
    sc = 2.0 ** (9 - np.floor(np.log2(amax))) if amax > 0 else 1.0        # max |dy| into [512, 1024), as the device chooses it
    w3 = w.reshape(Cout, Cin, 9)
    pairs = [(_gather(dy_rows, dg[t]), w3[:, :, t]) for t in range(9)]        # dx[i] = sum_t dy[o(i, t)] W_t
    d64, d32, _ = util.gemm_refs(pairs, chain=2, split=False)
    assert torch.allclose(d64, dx64, atol=1e-12), "the dgrad book agrees with autograd"
    dxs = None
    if h2 and s == 1:
        dxs = (util.gemm_refs([(a * sc, b) for a, b in pairs])[2].double() / sc).float()
    dxk = xd.grad.cpu()
    util.assert_precise(dxk, dx64, d32, dxs, what="aniso dgrad s%d %s %d->%d" % (s, grid, Cin, Cout))
    if s == 4:
        xs = (torch.arange(X * Y * Z) // (Y * Z)) % X
        ys = (torch.arange(X * Y * Z) // Z) % Y
        unread = (xs % 4 == 2) | (ys % 4 == 2)
        assert unread.any() and float(dxk[unread].abs().max()) == 0.0, "voxels no output reads have an exactly zero gradient"
    xrows = util.ncdhw_rows(x)
    per_tap = [util.gemm_refs([(dy_rows.t(), _gather(xrows, fwd[t]))], chain=2, split=False) for t in range(9)]      # dW_t = dy^T x(t)
    w64 = torch.stack([p[0] for p in per_tap], 2).view_as(dw64)
    w32 = torch.stack([p[1] for p in per_tap], 2).view_as(dw64)
    assert torch.allclose(w64, dw64, atol=1e-10), "the wgrad book agrees with autograd"
    util.assert_precise(wd.grad.cpu(), dw64, w32, None, what="aniso wgrad s%d %s %d->%d" % (s, grid, Cin, Cout))


# ------------------------------------------------------------------ d. one deblock
def _cmp(got, r64, r32, what, tol=util.TOL):
    """``util.TOL`` scale-relative, under the condition that the fp32 torch evaluation is within a quarter of it."""
    e32 = util.rel_err(r32, r64)
    assert e32 <= tol / 4, "%s: the fp32 torch evaluation is %.3e from float64: TOL does not judge this fixture" % (what, e32)
    e = util.rel_err(got, r64)
    print("[trunk-train] %-40s scale-relative %.3e (fp32 torch %.3e)" % (what, e, e32))
    assert e <= tol, "%s: %.3e from float64" % (what, e)


@pytest.mark.parametrize("s", [2, 4])
def test_deblock_with_batch_statistics_against_float64(dev, s):
    """ConvTranspose3d(kernel = stride = (1,s,s)) + BatchNorm3d (training mode) + ReLU: output, dx, dW, dgamma, dbeta within
    ``util.TOL`` (scale-relative) of float64 torch, where the fp32 torch evaluation is within TOL / 4.  Running statistics: torch's
    update (momentum 0.1 here, unbiased variance) to 1e-5 -- the fp32 batch statistics round at ~1e-6 and the update scales that by
    the momentum; a biased variance would be off by momentum / (n - 1) >= 2.6e-4 (n = 96 and 384 values per channel)."""
    Cin, Cout, (Z, Y, X) = 32, 16, (2, 3, 4)
    gen = torch.Generator().manual_seed(40 + s)
    blk = nn.Sequential(nn.ConvTranspose3d(Cin, Cout, (1, s, s), stride=(1, s, s), bias=False), nn.BatchNorm3d(Cout, eps=1e-3, momentum=0.1),
                        nn.ReLU())
    blk.load_state_dict(synth.random_state_dict(blk.state_dict(), seed=40 + s))
    x = torch.randn(1, Cin, Z, Y, X, generator=gen)
    up = torch.randn(1, Cout, Z, Y * s, X * s, generator=gen)
    refs = {}
    for dt in (torch.float64, torch.float32):
        m = copy.deepcopy(blk).to(dt).train()
        xa = x.to(dt, copy=True).requires_grad_()       # a copy: x.to(float32) is x itself, and x stays a plain input
        y = m(xa)
        y.backward(up.to(dt))
        refs[dt] = dict(y=y.detach(), dx=xa.grad, dw=m[0].weight.grad, dg=m[1].weight.grad, db=m[1].bias.grad, rm=m[1].running_mean,
                        rv=m[1].running_var, nb=int(m[1].num_batches_tracked))
    m = copy.deepcopy(blk).to(dev).train()
    xd = x.to(dev).requires_grad_()
    rows = ag.ZyxRowsFn.apply(xd)
    with util.kernels() as names:
        u = ag.deconv_bn_rows(rows, m[0], m[1], s)
        out = ag.fpn_sum_rows([u], [s], Cout, (1, X * s, Y * s, Z))
        out.backward(up.permute(0, 4, 3, 2, 1).reshape(-1, Cout).contiguous().to(dev))
    assert names.get("k_fpn_sum_bwd") == 1 and names.get("k_fpn_sum") == 1, names
    got = dict(y=out.detach().view(1, X * s, Y * s, Z, Cout).permute(0, 4, 3, 2, 1), dx=xd.grad, dw=m[0].weight.grad, dg=m[1].weight.grad,
               db=m[1].bias.grad)
    assert tuple(m[0].weight.grad.shape) == (Cin, Cout, 1, s, s)
    for k, v in got.items():
        _cmp(v.cpu(), refs[torch.float64][k], refs[torch.float32][k], "deblock s%d %s" % (s, k))
    r = refs[torch.float64]
    assert int(m[1].num_batches_tracked) == r["nb"] == 1
    for k, v in (("rm", m[1].running_mean), ("rv", m[1].running_var)):
        e = util.rel_err(v, r[k])
        assert e <= 1e-5, "running statistic %s: %.3e" % (k, e)


# ------------------------------------------------------------------ e. a small whole trunk
_TRUNK = {}
GAIN, SEED = 1.0, 71


def _trunk_cfgs(cascade):
    norm = dict(type='BN3d', eps=1e-3, momentum=0.01)
    b = dict(in_channels=[32, 32, 32], out_channels=[32, 32, 64], layer_nums=[1, 2, 1], layer_strides=[1, 2, 4], is_cascade=cascade,
             norm_cfg=dict(norm), conv_cfg=dict(type='Conv3d', kernel=(1, 3, 3), bias=False))
    # a cascade multiplies the strides (1, 2, 8): the neck's upsampling must undo that for sum(ups) to have levels of one size
    n = dict(in_channels=[32, 32, 64], out_channels=[32, 32, 32], upsample_strides=[1, 2, 8 if cascade else 4], norm_cfg=dict(norm),
             upsample_cfg=dict(type='deconv3d', bias=False), extra_conv=dict(type='Conv3d', num_conv=1, bias=False),
             use_conv_for_no_stride=True)
    return b, n


def _trunk_case(cascade):
    """The float64 and fp32 CPU evaluations of the restatement under train(), computed once per variant."""
    if cascade not in _TRUNK:
        bcfg, ncfg = _trunk_cfgs(cascade)
        rb, rn = ref_second3d.RefSECOND3D(**bcfg), ref_second3d.RefSECOND3DFPN(**ncfg)
        sdb = synth.random_state_dict(rb.state_dict(), seed=SEED, gain=GAIN)
        sdn = synth.random_state_dict(rn.state_dict(), seed=SEED + 1, gain=GAIN)
        x = synth.second3d_input((2, 16, 16), C=32, seed=SEED)
        gout = torch.randn(1, 32, 2, 16, 16, generator=torch.Generator().manual_seed(SEED))
        refs = {}
        for dt in (torch.float64, torch.float32):
            b, n = copy.deepcopy(rb), copy.deepcopy(rn)
            b.load_state_dict(sdb), n.load_state_dict(sdn)
            b, n = b.to(dt).train(), n.to(dt).train()
            xa = x.to(dt, copy=True).requires_grad_()       # a copy: x.to(float32) is x itself, and x stays a plain input
            y = n(list(b(xa)))
            (y * gout.to(dt)).sum().backward()
            r = dict(y=y.detach(), dx=xa.grad)
            for tag, mod in (("backbone.", b), ("neck.", n)):
                r.update({tag + k + ".grad": p.grad for k, p in mod.named_parameters()})
                r.update({tag + k: v.detach().clone() for k, v in mod.named_buffers() if "running" in k})
            refs[dt] = r
        _TRUNK[cascade] = dict(cfg=(bcfg, ncfg), sd=(sdb, sdn), x=x, gout=gout, refs=refs)
    return _TRUNK[cascade]


@pytest.mark.parametrize("cascade", [False, True])
def test_small_trunk_under_train_matches_the_float64_restatement(dev, cascade):
    """SECOND3D(layer_nums [1,2,1], strides [1,2,4]) + SECOND3DFPN(use_conv_for_no_stride, one extra conv) on [1,32,2,16,16] under
    train(): output, every parameter's gradient, the input gradient and every running statistic within ``util.TOL`` (scale-relative,
    per tensor) of the plain-torch restatement in float64.  Condition, asserted per tensor: the fp32 torch evaluation of the same
    restatement is within TOL / 4 of the float64 one -- the seed / weight gain above were picked on the CPU so that it holds (the
    cascade's last block normalises over 8 voxels, where batch statistics are touchy)."""
    S = _trunk_case(cascade)
    bcfg, ncfg = S["cfg"]
    b, n = lt.SECOND3D(**bcfg), lt.SECOND3DFPN(**ncfg)
    assert list(b.state_dict()) == list(S["sd"][0]) and list(n.state_dict()) == list(S["sd"][1])
    b.load_state_dict(S["sd"][0]), n.load_state_dict(S["sd"][1])
    b, n = b.to(dev).train(), n.to(dev).train()
    xd = S["x"].to(dev).requires_grad_()
    out = lt.run_trunk_train(b, n, xd)
    assert isinstance(out, core.Rows) and out.t.grad_fn is not None and (out.X, out.Y, out.Z, out.C) == (16, 16, 2, 32)
    y = lt.rows_as_bczyx(out)
    (y * S["gout"].to(dev)).sum().backward()
    core.check_h2_overflow()
    r64, r32 = S["refs"][torch.float64], S["refs"][torch.float32]
    got = dict(y=y.detach(), dx=xd.grad)
    for tag, mod in (("backbone.", b), ("neck.", n)):
        for k, p in mod.named_parameters():
            assert p.grad is not None and tuple(p.grad.shape) == tuple(p.shape), tag + k
            got[tag + k + ".grad"] = p.grad
        got.update({tag + k: v for k, v in mod.named_buffers() if "running" in k})
    assert set(got) == set(r64)
    for k in sorted(got):
        _cmp(got[k].cpu(), r64[k], r32[k], "trunk cascade=%s %s" % (cascade, k))
    with pytest.raises(NotImplementedError, match="train"):
        b(xd.detach())


# ------------------------------------------------------------------ f. the detector
def test_detector_trains_its_lidar_trunk_and_evaluates_on_the_stepped_weights(dev):
    cfg = synth.model_cfg_lidar()
    det = pkg.build_detector(cfg, external_encoders=True, train_lidar_trunk=True)
    det.load_state_dict(synth.random_state_dict(det.state_dict(), seed=5, gain=0.5))
    sdb, sdn = synth.second3d_weights(det.pts_backbone, det.pts_neck, 63)
    det.pts_backbone.load_state_dict(sdb), det.pts_neck.load_state_dict(sdn)
    det = det.to(dev).train()
    x = synth.second3d_input((8, 100, 100), seed=63).to(dev)
    gt = torch.randint(0, 17, (1, 200, 200, 16), generator=torch.Generator().manual_seed(3)).to(dev)
    with torch.no_grad():
        det.eval()
        pv = det.trunk_from_middle(x)[0].clone()
        det.train()
    want = det.forward_train(gt_occ=gt, precomputed=dict(pts_voxel_feats=pv), generator=torch.Generator(device=dev).manual_seed(0))
    det.zero_grad()
    rm0 = det.pts_backbone.blocks[0][1].running_mean.clone()
    losses = det.forward_train(gt_occ=gt, precomputed=dict(pts_middle_feats=x), generator=torch.Generator(device=dev).manual_seed(0))
    assert set(losses) == set(want) and all(v.requires_grad for k, v in losses.items() if k.startswith("loss"))
    sum(v for k, v in losses.items() if k.startswith("loss")).backward()
    core.check_h2_overflow()
    trunk = [(k, p) for k, p in det.named_parameters() if k.startswith(("pts_backbone.", "pts_neck."))]
    assert len(trunk) == len(list(det.pts_backbone.parameters())) + len(list(det.pts_neck.parameters())) > 60
    for k, p in trunk:
        assert p.grad is not None and bool(torch.isfinite(p.grad).all()) and float(p.grad.abs().max()) > 0.0, k
    assert not torch.equal(det.pts_backbone.blocks[0][1].running_mean, rm0), "a training-mode BN updates its running mean"
    opt = torch.optim.SGD([p for _, p in trunk], lr=1e-3)
    opt.step()
    det.eval()
    with torch.no_grad():
        got = lt.run_trunk(det.pts_backbone, det.pts_neck, x)
        b2, n2 = lt.SECOND3D(**{k: v for k, v in cfg["pts_backbone"].items() if k != "type"}), \
            lt.SECOND3DFPN(**{k: v for k, v in cfg["pts_neck"].items() if k != "type"})
        b2.load_state_dict(det.pts_backbone.state_dict()), n2.load_state_dict(det.pts_neck.state_dict())
        fresh = lt.run_trunk(b2.to(dev).eval(), n2.to(dev).eval(), x)
    core.check_h2_overflow()
    assert bits_equal(got.t, fresh.t), "eval() after the step runs on the stepped weights (PackCache)"
    assert not bits_equal(got.t, core.to_rows(pv).t), "... which differ from the ones before it"


# ------------------------------------------------------------------ g. co-runner guard
N_CALLS = 20


@pytest.mark.parametrize("corunner", ["h2p", "wino"])
def test_fpn_sum_bwd_is_bit_stable_beside_matrix_core_work(dev, corunner):
    """In the manner of tests/test_gpu_second3d_corunner.py: 20 calls on fixed inputs beside split-f16 layers of a second stream
    give the bits they give alone."""
    g = torch.Generator().manual_seed(11)
    xb = core.to_rows(torch.randn(1, 128, 100, 100, 8, generator=g).to(dev))
    pc = (core.PackedConv((torch.randn(128, 128, 1, 1, 1, generator=g) * 0.05).to(dev), ksize=1, pad=0) if corunner == "h2p" else
          core.PackedConv((torch.randn(128, 128, 3, 3, 3, generator=g) * 0.02).to(dev), ksize=3, pad=1))
    B, X, Y, Z, C = 1, 100, 100, 8, 128
    dout = torch.randn(B * X * Y * Z, C, generator=g).to(dev)
    strides = (1, 2, 4)

    def fn():
        grads = [None] + [torch.empty(B * (X // s) * (Y // s) * Z, s * s * C, device=dev) for s in strides[1:]]
        pp = (ctypes.c_void_p * 4)(*[t.data_ptr() if t is not None else None for t in grads])
        call("coocc_fpn_sum_bwd", ptr(dout), C, pp, (ctypes.c_int * 4)(*strides), 3, B, X, Y, Z, C)
        return grads[1:]
    s0, s1 = torch.cuda.Stream(device=dev), torch.cuda.Stream(device=dev)
    with torch.no_grad():
        core.conv_rows(xb, pc, relu=False)
        torch.cuda.synchronize()
        with torch.cuda.stream(s0):
            ref = fn()
        torch.cuda.synchronize()
        for t, s in zip(ref, strides[1:]):
            assert bits_equal(t.cpu(), _relayout(dout.cpu(), B, X, Y, Z, C, s))
        got = []
        for _ in range(N_CALLS):
            with torch.cuda.stream(s1):
                for _ in range(4):
                    core.conv_rows(xb, pc, relu=False)
            with torch.cuda.stream(s0):
                got.append(fn())
        torch.cuda.synchronize()
    core.check_h2_overflow()
    bad = sum(int(not all(bits_equal(a, b) for a, b in zip(ref, t))) for t in got)
    assert bad == 0, "fpn_sum_bwd beside %s: %d of %d calls differ from the run alone" % (corunner, bad, N_CALLS)
