"""The high-precision judge of tests/util.py checked on the CPU: it accepts an fp32 evaluation and a correct emulation of the
split-f16 engine (csrc/gemm_h2.hip), and rejects the emulated engine with subtly lost terms that ``assert_close`` lets through
(tests/test_gpu_precision.py shows the same on the GPU kernels).  The fp32 Winograd emulation that anchors the Winograd GPU cases
computes the convolution, at fp32-level error, for all three tiles."""
import pytest
import torch

from util import (FLOOR, assert_precise, conv_taps, errors, gemm_refs, h2_split, ncdhw_rows, precision, rel_err,
                  split_mm, wino_conv)


def engine(a, b, drop_lo=None, lo_scale=2048.0, drop_chunk=None):
    """The split-f16 engine emulated with fp32 accumulation (f16 x f16 products are exact in fp32): ah bh + (ah bl + al bh) / 2^11.
    drop_lo: "a" | "b" -- one operand's lo half lost; lo_scale: the power of two lo is decoded with; drop_chunk: the lo halves of
    both operands lost on K entries [32 c, 32 c + 32) only."""
    ah, al = h2_split(a)
    bh, bl = h2_split(b)
    if drop_lo == "a":
        al = torch.zeros_like(al)
    if drop_lo == "b":
        bl = torch.zeros_like(bl)
    if drop_chunk is not None:
        al, bl = al.clone(), bl.clone()
        al[:, 32 * drop_chunk:32 * drop_chunk + 32] = 0
        bl[32 * drop_chunk:32 * drop_chunk + 32] = 0
    ah, al, bh, bl = ah.float(), al.float(), bh.float(), bl.float()
    return ah @ bh + (ah @ bl + al @ bh) / lo_scale


# conv-sized GEMMs (M x K x N): a 3x3x3 layer's K = 27 Cin, and a pointwise layer whose K is too short for the fp32 anchor alone
GEMMS = [(4000, 1728, 128), (2000, 3456, 128), (20000, 64, 64)]


@pytest.mark.parametrize("M,K,N", GEMMS)
def test_judge_accepts_fp32_and_the_split_engine_and_rejects_lost_terms(M, K, N):
    g = torch.Generator().manual_seed(M + K)
    a = torch.randn(M, K, generator=g)
    b = torch.randn(K, N, generator=g) * K ** -0.5
    ref64, ref32, refs = gemm_refs([(a, b)])
    what = "%dx%dx%d" % (M, K, N)
    assert_precise(ref32, ref64, ref32, refs, what="fp32 " + what)
    assert_precise(engine(a, b), ref64, ref32, refs, what="split-f16 engine " + what)
    bad = {"lo of A dropped": engine(a, b, drop_lo="a"), "lo of B dropped": engine(a, b, drop_lo="b"),
           "lo decoded with 2^-10": engine(a, b, lo_scale=1024.0), "lo dropped on one K chunk": engine(a, b, drop_chunk=K // 64)}
    for name, out in bad.items():
        st = precision(out, ref64, ref32, refs, what=name + " " + what)
        assert not st["ok"], "the judge accepted the engine with %s (%s)" % (name, what)
        if K >= 768 and name != "lo dropped on one K chunk":
            assert rel_err(out, ref64) < 1e-3            # all of these are close to assert_close's 1e-4 ...
    # ... and the chunk-dropped engine passes it outright at the long K: the gap this judge closes
    if K >= 768:
        assert rel_err(bad["lo dropped on one K chunk"], ref64) <= 1e-4


def test_judge_has_no_floor_at_one_and_demands_exact_zeros():
    g = torch.Generator().manual_seed(3)
    a, b = torch.randn(500, 256, generator=g) * 1e-3, torch.randn(256, 32, generator=g) * 1e-3
    ref64, ref32, refs = gemm_refs([(a, b)])
    assert float(ref64.abs().max()) < 1e-4
    assert rel_err(torch.zeros_like(ref32), ref64) <= 1e-4            # the old rule accepts zeros here
    assert not precision(torch.zeros_like(ref32), ref64, ref32, refs, what="zeros for a 1e-5 output")["ok"]
    assert_precise(engine(a, b), ref64, ref32, refs, what="split-f16 engine, 1e-5 output")
    z = torch.zeros(7, 5, dtype=torch.float64)
    assert errors(z.float(), z) == (0.0, 0.0)
    assert_precise(z.float(), z, z.float(), what="all-zero reference")
    bump = z.clone()
    bump[3, 2] = 1e-30
    assert not precision(bump, z, z.float(), what="nonzero against an all-zero reference")["ok"]


def test_split_emulation_keeps_three_terms():
    """h2_split is the engine's split (hi + lo 2^-11 carries 22 significand bits) and split_mm keeps ah bh + 2^-11 (ah bl + al bh)."""
    g = torch.Generator().manual_seed(4)
    a = torch.randn(64, 96, generator=g)
    hi, lo = h2_split(a)
    assert float(((hi + lo / 2048.0) - a.double()).abs().max() / a.abs().max()) < 2 ** -21
    assert torch.equal(hi, a.half().double())
    b = torch.randn(96, 16, generator=g)
    bh, bl = h2_split(b)
    assert torch.allclose(split_mm(a, b), hi @ bh + (hi @ bl + lo @ bh) / 2048.0, rtol=0, atol=1e-12)


@pytest.mark.parametrize("m", [2, 3, 4])
@pytest.mark.parametrize("B,Cin,Cout,grid", [(1, 64, 96, (13, 11, 4)), (2, 32, 17, (9, 10, 1)), (1, 96, 32, (8, 7, 2))])
def test_winograd_emulation_matches_fp64_direct_convolution(m, B, Cin, Cout, grid):
    """The fp32 emulation (same transform matrices, z taps, operand scale as csrc/winograd.hip and core.H2_WINO_SCALE) computes
    the convolution: exactly in fp64 (the algorithm), and within fp32-level error in fp32 -- above direct fp32 by the transforms'
    amplification (F(2): ~1.5x, F(4): ~10x measured), far below anything a wrong transform point would give."""
    from co_occ_amd import core
    g = torch.Generator().manual_seed(m * 100 + Cin)
    x = torch.randn(B, Cin, *grid, generator=g)
    w = torch.randn(Cout, Cin, 3, 3, 3, generator=g) * (2.0 / (Cin * 27)) ** 0.5
    ref64, ref32, _ = gemm_refs(conv_taps(x, w), split=False)
    assert float((ref64 - ncdhw_rows(torch.nn.functional.conv3d(x.double(), w.double(), padding=1))).abs().max()) < 1e-12
    e64 = errors(wino_conv(x, w, m, torch.float64), ref64)
    assert e64[0] < 1e-13, "the fp64 Winograd emulation is not the convolution: %s" % (e64,)
    e32 = errors(ref32, ref64)
    ew = errors(wino_conv(x, w, m, vscale=core.H2_WINO_SCALE[m]), ref64)
    print("[wino-emul] F(%d) B%d %d->%d %s: e %.2e/%.2e, direct fp32 %.2e/%.2e" % (m, B, Cin, Cout, grid, *ew, *e32))
    assert ew[0] <= 32 * max(e32[0], FLOOR) and ew[1] <= 16 * max(e32[1], FLOOR)
    assert ew[0] < 1e-5
