"""The linear adjoint kernels of csrc/backward.hip on the GPU, each entry alone through the C ABI against float64 (tests/adjoint_refs.py:
the restatements, the cases and the judging rules): ``coocc_upsample_trilinear_bwd``, ``coocc_occhead_mix_bwd``,
``coocc_upsample_maps_bwd``, ``coocc_fine_sample_voxel_bwd`` / ``_img_bwd`` (with their forwards, which share the normalisation and
the projection), ``coocc_lift_splat_bwd``, ``coocc_voxel_pool_bwd`` and ``coocc_scatter_add_rows``.

Every buffer a kernel writes starts as NaN and is followed by guard elements that must keep their sentinel; the padding columns of
strided buffers (inputs too) hold NaN and must still hold it afterwards.  Three rules judge the results: exact (integer data,
power-of-two weights: the float64 value, whatever the order of the sums; the sign of a zero is not part of the value), precise
(``util.assert_precise`` on N(0, 1) data, the fp32 restatement as the anchor; for the two sampler adjoints, whose atomics add in an
order that changes from run to run, the worst of three seeded orders of it) and two calls (the same launch twice gives the same
bits, for every kernel without atomics).  No verdict compares a kernel with itself."""
import ctypes
import functools

import pytest
import torch

from co_occ_amd import _lib
from co_occ_amd._lib import call, host_f32, host_i32, ptr

import adjoint_refs as R
import util

pytestmark = pytest.mark.gpu

F32, F64 = torch.float32, torch.float64
GUARD, SENT = 64, 12345.0


def D(dev, t):
    t = t.to(dev).contiguous()
    assert t.data_ptr() % 16 == 0
    return t


def guarded(dev, numel, dtype=F32, fill=R.NAN):
    """A flat buffer of ``numel`` elements of ``fill`` followed by GUARD sentinels."""
    buf = torch.full((numel + GUARD,), fill, device=dev, dtype=dtype)
    buf[numel:] = SENT
    return buf


def finish(buf, numel, what):
    assert bool((buf[numel:] == SENT).all()), what + ": wrote behind its output"
    return buf[:numel].clone()


def padded(dev, t, stride):
    """[rows, stride] of NaN with ``t`` [rows, C] in its first columns."""
    buf = torch.full((t.shape[0], stride), R.NAN, device=dev, dtype=F32)
    buf[:, :t.shape[1]] = t.to(dev)
    return buf


def same(out, ref, what):
    """Rule 1 / bit equality up to the sign of a zero (an empty sum is +0.0, a sum of products with zeros may be -0.0)."""
    R.assert_exact(out.cpu() + 0.0, ref.cpu() + 0.0, what)


def exact(out, ref64, ref32, what):
    same(out, R.exact_ref(ref64, ref32), what)


def precise(out, ref64, ref32, what, anchor=None):
    assert not bool(torch.isnan(out).any()), what + ": NaN in the result"
    return util.assert_precise(out.cpu(), ref64, ref32, anchor=anchor, what=what)


def precise_atomics(out, adj, what):
    """Rule 2 for a kernel that adds with fp32 atomics: ``adj(dtype, order=None)`` is its restatement; float64 is the reference, the
    worst of three seeded orders of the fp32 contributions the anchor (adjoint_refs.atomics_anchor)."""
    ref64 = adj(F64)
    return precise(out, ref64, None, what, anchor=R.atomics_anchor(lambda order: adj(F32, order), ref64))


def prod(t):
    n = 1
    for v in t:
        n *= v
    return n


# ============================================================================= coocc_upsample_trilinear_bwd
def tri_bwd(dev, dfine, coarse, accumulate=0, prior=None, what="upsample_trilinear_bwd"):
    B, Xf, Yf, Zf, C = dfine.shape
    n = B * prod(coarse) * C
    buf = guarded(dev, n)
    if prior is not None:
        buf[:n] = prior.to(dev).flatten()
    call("coocc_upsample_trilinear_bwd", ptr(D(dev, dfine)), ptr(buf), B, C, *coarse, Xf, Yf, Zf, accumulate)
    return finish(buf, n, what).view(B, *coarse, C).cpu()


@pytest.mark.parametrize("B,C,coarse,fine", R.TRI_EXACT)
def test_upsample_trilinear_bwd_exact(dev, B, C, coarse, fine):
    c = R.tri_case(B, C, coarse, fine, exact=True)
    what = "upsample_trilinear_bwd exact %s -> %s" % (coarse, fine)
    out = tri_bwd(dev, c["dfine"], coarse, what=what)
    exact(out, R.trilinear_adj(c["dfine"], coarse, F64), R.trilinear_adj(c["dfine"], coarse, F32), what)
    R.assert_exact(tri_bwd(dev, c["dfine"], coarse), out, what + ", second call")


@pytest.mark.parametrize("B,C,coarse,fine", R.TRI_PRECISE)
def test_upsample_trilinear_bwd_precise(dev, B, C, coarse, fine):
    c = R.tri_case(B, C, coarse, fine, exact=False)
    what = "upsample_trilinear_bwd %s -> %s" % (coarse, fine)
    out = tri_bwd(dev, c["dfine"], coarse, what=what)
    precise(out, R.trilinear_adj(c["dfine"], coarse, F64), R.trilinear_adj(c["dfine"], coarse, F32), what)
    R.assert_exact(tri_bwd(dev, c["dfine"], coarse), out, what + ", second call")


def test_upsample_trilinear_bwd_equal_grids_copy_bits(dev):
    B, C, coarse, fine = R.TRI_COPY
    c = R.tri_case(B, C, coarse, fine, exact=False)
    R.assert_exact(tri_bwd(dev, c["dfine"], coarse), c["dfine"], "upsample_trilinear_bwd 5x5x5 -> 5x5x5")


@pytest.mark.parametrize("case,is_exact", [(R.TRI_EXACT[1], True), (R.TRI_PRECISE[1], False)])
def test_upsample_trilinear_bwd_accumulate(dev, case, is_exact):
    """accumulate = 1: the prior contents plus the accumulate = 0 result, one fp32 addition per element."""
    B, C, coarse, fine = case
    c = R.tri_case(B, C, coarse, fine, exact=is_exact)
    what = "upsample_trilinear_bwd accumulate %s -> %s" % (coarse, fine)
    plain = tri_bwd(dev, c["dfine"], coarse)
    acc = tri_bwd(dev, c["dfine"], coarse, accumulate=1, prior=c["prior"], what=what)
    R.assert_exact(acc, c["prior"] + plain, what)
    ref64 = c["prior"].to(F64) + R.trilinear_adj(c["dfine"], coarse, F64)
    if is_exact:
        exact(acc, ref64, None, what)
    else:
        precise(acc, ref64, c["prior"] + R.trilinear_adj(c["dfine"], coarse, F32), what)


# ============================================================================= coocc_occhead_mix_bwd
def mix_bwd(dev, c, what):
    """-> (g [L] of [V0, C] on the device, dwlogit [V0, L] or None)."""
    B, C, dims = c["B"], c["C"], c["dims"]
    L, V0 = len(dims), B * prod(dims[0])
    lv = [D(dev, p) for p in c["levels"]]
    gb = [guarded(dev, V0 * C) for _ in range(L)]
    wl = None if c["wlogit"] is None else D(dev, c["wlogit"])
    dwl = None if wl is None else guarded(dev, V0 * L)
    arr = (ctypes.c_void_p * L)(*[t.data_ptr() for t in lv])
    garr = (ctypes.c_void_p * L)(*[t.data_ptr() for t in gb])
    call("coocc_occhead_mix_bwd", arr, host_i32([v for d in dims for v in d]), L, ptr(wl), ptr(D(dev, c["dout"])), garr, ptr(dwl), B, C)
    g = [finish(b, V0 * C, what + " g[%d]" % l).view(V0, C) for l, b in enumerate(gb)]
    return g, None if dwl is None else finish(dwl, V0 * L, what + " dwlogit").view(V0, L)


def mix_chain(dev, c, g):
    """The per-level gradients pulled down by coocc_upsample_trilinear_bwd, as OccHeadMixFn.backward does (a level on the level-0
    grid takes its scaled gradient as it is)."""
    B, C, dims = c["B"], c["C"], c["dims"]
    out = []
    for l, d in enumerate(dims):
        gl = g[l].view(B, *dims[0], C)
        out.append(gl.cpu() if d == dims[0] else tri_bwd(dev, gl, d))
    return out


@pytest.mark.parametrize("name", [n for n in R.MIX if n != "L1"])
def test_occhead_mix_bwd_precise(dev, name):
    c = R.mix_case(name)
    what = "occhead_mix_bwd " + name
    g, dwl = mix_bwd(dev, c, what)
    g64, d64 = R.mix_adj(c["levels"], c["wlogit"], c["dout"], F64)
    g32, d32 = R.mix_adj(c["levels"], c["wlogit"], c["dout"], F32)
    for l in range(len(g)):
        precise(g[l], g64[l], g32[l], what + " g[%d]" % l)
    if c["wlogit"] is None:
        assert dwl is None
    else:
        precise(dwl, d64, d32, what + " dwlogit")
    lv64, lv32 = R.mix_level_grads(c["levels"], g64, F64), R.mix_level_grads(c["levels"], g32, F32)
    for l, d in enumerate(mix_chain(dev, c, g)):
        precise(d, lv64[l], lv32[l], what + " gradient of level %d" % l)
    g2, dwl2 = mix_bwd(dev, c, what)
    for a, b in zip(g + ([dwl] if dwl is not None else []), g2 + ([dwl2] if dwl is not None else [])):
        R.assert_exact(b.cpu(), a.cpu(), what + ", second call")


@pytest.mark.parametrize("name", R.MIX_EXACT)
def test_occhead_mix_bwd_exact(dev, name):
    """L = 1: g[0] is dout's bits and dwlogit exactly 0.  wlogit = NULL (dwlogit = NULL), L = 2: weights 1/2, factor 2."""
    c = R.mix_case(name, exact=True)
    what = "occhead_mix_bwd exact " + name
    g, dwl = mix_bwd(dev, c, what)
    g64, d64 = R.mix_adj(c["levels"], c["wlogit"], c["dout"], F64)
    g32, d32 = R.mix_adj(c["levels"], c["wlogit"], c["dout"], F32)
    for l in range(len(g)):
        exact(g[l], g64[l], g32[l], what + " g[%d]" % l)
    lv64 = R.mix_level_grads(c["levels"], g64, F64)
    for l, d in enumerate(mix_chain(dev, c, g)):
        exact(d, lv64[l], None, what + " gradient of level %d" % l)
    if name == "L1":
        R.assert_exact(g[0].cpu(), c["dout"], what + ": g[0] is dout")
        same(dwl, torch.zeros_like(d64, dtype=F32), what + " dwlogit")
    else:
        assert c["wlogit"] is None and dwl is None


# ============================================================================= coocc_upsample_maps_bwd
def maps_bwd(dev, dr, dd, N, H, W, scale, what="upsample_maps_bwd"):
    buf = guarded(dev, N * H * W * 4)
    call("coocc_upsample_maps_bwd", ptr(None if dr is None else D(dev, dr)), ptr(None if dd is None else D(dev, dd)), N, H, W, scale, ptr(buf))
    return finish(buf, N * H * W * 4, what).view(N, H, W, 4).cpu()


def maps_grads(N, H, W, scale, is_exact):
    g = R.gen(N + 10 * H + 100 * W + scale)
    draw = (lambda s: R.ints(s, g, -4, 4)) if is_exact else (lambda s: R.normal(s, g))
    return draw((N, H * scale, W * scale, 3)), draw((N, H * scale, W * scale))


@pytest.mark.parametrize("N,H,W,scale", R.MAPS_EXACT)
def test_upsample_maps_bwd_exact(dev, N, H, W, scale):
    dr, dd = maps_grads(N, H, W, scale, True)
    what = "upsample_maps_bwd exact %dx%dx%d x%d" % (N, H, W, scale)
    out = maps_bwd(dev, dr, dd, N, H, W, scale, what)
    exact(out, R.maps_adj(dr, dd, N, H, W, scale, F64), R.maps_adj(dr, dd, N, H, W, scale, F32), what)
    R.assert_exact(maps_bwd(dev, dr, dd, N, H, W, scale), out, what + ", second call")


@pytest.mark.parametrize("N,H,W,scale", R.MAPS_PRECISE)
def test_upsample_maps_bwd_precise(dev, N, H, W, scale):
    dr, dd = maps_grads(N, H, W, scale, False)
    what = "upsample_maps_bwd %dx%dx%d x%d" % (N, H, W, scale)
    out = maps_bwd(dev, dr, dd, N, H, W, scale, what)
    precise(out, R.maps_adj(dr, dd, N, H, W, scale, F64), R.maps_adj(dr, dd, N, H, W, scale, F32), what)
    R.assert_exact(maps_bwd(dev, dr, dd, N, H, W, scale), out, what + ", second call")


def test_upsample_maps_bwd_scale_1_copies_bits(dev):
    N, H, W, scale = R.MAPS_COPY
    dr, dd = maps_grads(N, H, W, scale, False)
    R.assert_exact(maps_bwd(dev, dr, dd, N, H, W, scale), torch.cat([dr, dd[..., None]], 3), "upsample_maps_bwd x1")


@pytest.mark.parametrize("which", ["drgbs", "ddepths"])
def test_upsample_maps_bwd_one_gradient_alone(dev, which):
    """drgbs alone leaves channel 3 exactly 0, ddepths alone channels 0 - 2."""
    N, H, W, scale = R.MAPS_EXACT[1]
    dr, dd = maps_grads(N, H, W, scale, True)
    dr, dd = (dr, None) if which == "drgbs" else (None, dd)
    what = "upsample_maps_bwd with %s alone" % which
    out = maps_bwd(dev, dr, dd, N, H, W, scale, what)
    exact(out, R.maps_adj(dr, dd, N, H, W, scale, F64), R.maps_adj(dr, dd, N, H, W, scale, F32), what)
    zero = out[..., 3:] if which == "drgbs" else out[..., :3]
    assert bool((zero == 0).all()) and bool((out != 0).any())


# ============================================================================= the voxel sampler and its adjoint
def sample_voxel(dev, vol, coarse, pointwise, what):
    """coocc_fine_sample_voxel at ratio 2 -> (fine_xyz [3, nf] on the device, feat [nf, C])."""
    X, Y, Z, C = vol.shape
    n, stride = coarse.numel(), C + 2
    nf = 8 * n
    xyz = guarded(dev, 3 * nf, torch.int64, fill=-7)
    feat = guarded(dev, nf * stride)
    lib = _lib.load()
    lib.coocc_fine_set_pointwise(1 if pointwise else 0)
    try:
        call("coocc_fine_sample_voxel", ptr(D(dev, vol)), C, X, Y, Z, ptr(D(dev, coarse)), n, 2, host_i32(R.VOX_FINAL), ptr(xyz), ptr(feat), stride)
    finally:
        lib.coocc_fine_set_pointwise(0)
    rows = finish(feat, nf * stride, what).view(nf, stride)
    assert bool(torch.isnan(rows[:, C:]).all()), what + ": a padding column was written"
    return finish(xyz, 3 * nf, what + " fine_xyz").view(3, nf), rows[:, :C].contiguous()


def voxel_bwd(dev, dfeat, xyz_dev, C, what):
    X, Y, Z = R.VOX_DIMS
    nf = xyz_dev.shape[1]
    buf = guarded(dev, X * Y * Z * C)
    src = padded(dev, dfeat, C + 3) if nf else torch.full((1, C + 3), R.NAN, device=dev)
    idx = xyz_dev if nf else torch.zeros(3, 1, dtype=torch.int64, device=dev)
    call("coocc_fine_sample_voxel_bwd", ptr(src), C + 3, C, X, Y, Z, ptr(idx), nf, host_i32(R.VOX_FINAL), ptr(buf))
    return finish(buf, X * Y * Z * C, what).view(X, Y, Z, C).cpu()


@pytest.mark.parametrize("C", R.VOX_C)
def test_fine_sample_voxel_and_its_adjoint(dev, C):
    g = R.gen(40 + C)
    vol = R.normal(R.VOX_DIMS + (C,), g)
    coarse = R.vox_coarse_list()
    want_xyz = R.fine_children(coarse.long(), R.VOX_DIMS)
    r64, r32 = R.sample_voxel_fwd(vol, want_xyz, R.VOX_FINAL, F64), R.sample_voxel_fwd(vol, want_xyz, R.VOX_FINAL, F32)
    for pointwise in (False, True):
        what = "fine_sample_voxel C=%d %s" % (C, "point by point" if pointwise else "grouped")
        xyz, feat = sample_voxel(dev, vol, coarse, pointwise, what)
        assert torch.equal(xyz.cpu(), want_xyz), what + ": fine_xyz"
        precise(feat, r64, r32, what)
    what = "fine_sample_voxel_bwd C=%d" % C
    rep = R.vox_repeat_list()                                  # the forward's list, then one point 50 times over
    dfeat = R.normal((rep.shape[1], C), g)
    for name, lst, dlst in [("the forward's list", want_xyz, xyz), ("one point x50", rep, D(dev, rep)), ("nfine=1", want_xyz[:, 77:78].contiguous(), None)]:
        df = dfeat[:lst.shape[1]]
        out = voxel_bwd(dev, df, D(dev, lst) if dlst is None else dlst, C, "%s %s" % (what, name))
        precise_atomics(out, lambda dt, order=None: R.sample_voxel_adj(df, lst, R.VOX_FINAL, R.VOX_DIMS, dt, order), "%s %s" % (what, name))


@pytest.mark.parametrize("C", R.VOX_C)
def test_fine_sample_voxel_bwd_exact_corners_and_empty_list(dev, C):
    """The corners of the final grid (seven of eight taps outside, weights 1/8), one of them 50 times over; nfine = 0 zeroes dvol."""
    xyz = R.vox_corner_list()
    dfeat = R.ints((xyz.shape[1], C), R.gen(50 + C), -4, 4)
    what = "fine_sample_voxel_bwd exact C=%d" % C
    out = voxel_bwd(dev, dfeat, D(dev, xyz), C, what)
    exact(out, R.sample_voxel_adj(dfeat, xyz, R.VOX_FINAL, R.VOX_DIMS, F64), R.sample_voxel_adj(dfeat, xyz, R.VOX_FINAL, R.VOX_DIMS, F32), what)
    assert int((out != 0).any(-1).sum()) == 8
    out = voxel_bwd(dev, dfeat[:0], D(dev, xyz[:, :0]), C, what + " nfine=0")
    same(out, torch.zeros_like(out), what + " nfine=0")


# ============================================================================= the image sampler and its adjoint
def img_bwd(dev, dfeat, prm, xyz, Hf, Wf, what):
    Ci, nf = dfeat.shape[1], xyz.shape[1]
    buf = guarded(dev, 2 * Hf * Wf * Ci)
    src = padded(dev, dfeat, Ci + 3) if nf else torch.full((1, Ci + 3), R.NAN, device=dev)
    idx = D(dev, xyz) if nf else torch.zeros(3, 1, dtype=torch.int64, device=dev)
    call("coocc_fine_sample_img_bwd", ptr(src), Ci + 3, 2, Ci, Hf, Wf, ptr(D(dev, prm)), ptr(idx), nf, ptr(buf))
    return finish(buf, 2 * Hf * Wf * Ci, what).view(2, Hf, Wf, Ci).cpu()


@pytest.mark.parametrize("post_rot", [False, True])
@pytest.mark.parametrize("Hf,Wf", R.IMG_MAPS)
@pytest.mark.parametrize("Ci", R.IMG_C)
def test_fine_sample_img_and_its_adjoint(dev, Ci, Hf, Wf, post_rot):
    prm, xyz = R.camera_rig(post_rot)
    nf = xyz.shape[1]
    g = R.gen(60 + Ci + Hf)
    img, dfeat = R.normal((2, Hf, Wf, Ci), g), R.normal((nf, Ci), g)
    what = "fine_sample_img Ci=%d %dx%d%s" % (Ci, Hf, Wf, " post-rotated" if post_rot else "")
    stride = Ci + 2
    feat = guarded(dev, nf * stride)
    call("coocc_fine_sample_img", ptr(D(dev, img)), 2, Ci, Hf, Wf, ptr(D(dev, prm)), ptr(D(dev, xyz)), nf, ptr(feat), stride, 0)
    rows = finish(feat, nf * stride, what).view(nf, stride)
    assert bool(torch.isnan(rows[:, Ci:]).all()), what + ": a padding column was written"
    precise(rows[:, :Ci].contiguous(), R.sample_img_fwd(img, prm, xyz, F64), R.sample_img_fwd(img, prm, xyz, F32), what)
    what = what.replace("fine_sample_img", "fine_sample_img_bwd")
    out = img_bwd(dev, dfeat, prm, xyz, Hf, Wf, what)
    if (Hf, Wf) == (1, 1):
        # every weight is exactly 1: each of the 2 Ci outputs is ONE sum of up to 720 gradients in an order that changes from run to
        # run -- no fixed set of orders anchors a max / rms over so few values (40 runs of Ci = 4 spread over 2.4e-7 ... 1.1e-6 rms),
        # so the sums are held to rule 3's worst-case bound per element; the integer case below judges the same path exactly
        masks = [m for _, _, _, m, _ in R.project(prm, xyz, 2, F64)]
        idx = torch.cat([torch.where(m, cam, -1) for cam, m in enumerate(masks)]).to(torch.int32)
        R.assert_scatter(out.view(2, Ci), torch.zeros(2, Ci), torch.cat([dfeat, dfeat]), idx, what)
    else:
        precise_atomics(out, lambda dt, order=None: R.sample_img_adj(dfeat, prm, xyz, 2, Hf, Wf, dt, order=order), what)


@pytest.mark.parametrize("Ci", R.IMG_C)
def test_fine_sample_img_bwd_exact_on_a_1x1_map(dev, Ci):
    """A 1 x 1 map takes every visible point with weight 1: integer gradients sum to exact integers per camera.  nfine = 0 zeroes dimg."""
    prm, xyz = R.camera_rig()
    dfeat = R.ints((xyz.shape[1], Ci), R.gen(70 + Ci), -4, 4)
    what = "fine_sample_img_bwd exact Ci=%d" % Ci
    out = img_bwd(dev, dfeat, prm, xyz, 1, 1, what)
    exact(out, R.sample_img_adj(dfeat, prm, xyz, 2, 1, 1, F64), R.sample_img_adj(dfeat, prm, xyz, 2, 1, 1, F32), what)
    out = img_bwd(dev, dfeat[:0], prm, xyz[:, :0], 6, 8, what + " nfine=0")
    same(out, torch.zeros_like(out), what + " nfine=0")


# ============================================================================= coocc_lift_splat_bwd and coocc_voxel_pool_bwd
_pool_case = functools.lru_cache(maxsize=None)(R.pool_case)
POOL_IDS = ["%dx%dx%dx%d_c%d_b%d" % s[:6] for s in R.POOL]


def lift_splat_bwd(dev, c, shape, what):
    N, D_, H, W, C, B, grid = shape
    stride = C + 4
    dd, df = guarded(dev, N * D_ * H * W), guarded(dev, N * H * W * C)
    dout = padded(dev, c["dout"], stride)
    call("coocc_lift_splat_bwd", ptr(dout), stride, ptr(D(dev, c["depth"])), ptr(D(dev, c["feat"])), ptr(D(dev, c["geom"])), N, D_, H, W, C,
         c["ppb"], host_f32(c["lo_dx"]), B, *grid, ptr(dd), ptr(df))
    return finish(dd, N * D_ * H * W, what + " d_depth").view(N, D_, H, W).cpu(), finish(df, N * H * W * C, what + " d_feat").view(N * H * W, C).cpu()


def voxel_pool_bwd(dev, c, shape, what):
    N, D_, H, W, C, B, grid = shape
    npts, stride = N * D_ * H * W, C + 4
    dx = guarded(dev, npts * C)
    call("coocc_voxel_pool_bwd", ptr(padded(dev, c["dout"], stride)), stride, ptr(D(dev, c["geom"])), npts, c["ppb"], C, host_f32(c["lo_dx"]), B,
         *grid, ptr(dx))
    return finish(dx, npts * C, what).view(npts, C).cpu()


def check_outside_pixel(dd, df, shape, what):
    N, D_, H, W = shape[:4]
    if N * H * W > 1:
        assert bool((dd[N - 1, :, H - 1, W - 1] == 0).all()) and bool((df[-1] == 0).all()), what + ": a ray outside the grid has a gradient"


@pytest.mark.parametrize("gname", list(R.POOL_GRIDS))
@pytest.mark.parametrize("shape", R.POOL, ids=POOL_IDS)
def test_pooling_adjoints_exact_and_the_adjoint_identity(dev, monkeypatch, shape, gname):
    """Integer data: both adjoints equal float64, and <dout, lift_splat(depth, feat)> = <d_depth, depth> = <d_feat, feat> as exact
    integers for both COOCC_POOL_SEG forms of the forward -- which ties the adjoint's (-1, 0) truncation band to the forward's."""
    from co_occ_amd.ops import _pool_workspace
    N, D_, H, W, C, B, grid = shape
    c = _pool_case(*shape, gname, True)
    what = "lift_splat_bwd exact %s %s" % (shape[:6], gname)
    dd, df = lift_splat_bwd(dev, c, shape, what)
    r64, r32 = R.lift_splat_adj(c["dout"], c["depth"], c["feat"], c["keys"], F64), R.lift_splat_adj(c["dout"], c["depth"], c["feat"], c["keys"], F32)
    exact(dd, r64[0], r32[0], what + " d_depth")
    exact(df, r64[1], r32[1], what + " d_feat")
    check_outside_pixel(dd, df, shape, what)
    dd2, df2 = lift_splat_bwd(dev, c, shape, what)
    R.assert_exact(dd2, dd, what + " d_depth, second call")
    R.assert_exact(df2, df, what + " d_feat, second call")
    dx = voxel_pool_bwd(dev, c, shape, what.replace("lift_splat", "voxel_pool"))
    same(dx, R.voxel_pool_adj(c["dout"], c["keys"], F64).to(F32), "voxel_pool_bwd exact %s %s" % (shape[:6], gname))
    npts, nvox = N * D_ * H * W, c["nvox"]
    lhs_d, lhs_f = float((dd.to(F64) * c["depth"].to(F64)).sum()), float((df.to(F64) * c["feat"].to(F64)).sum())
    depth, feat, geom = D(dev, c["depth"]), D(dev, c["feat"]), D(dev, c["geom"])
    for mode in ("0", "1"):
        monkeypatch.setenv("COOCC_POOL_SEG", mode)
        out = torch.full((nvox, C), 7.0, device=dev)
        ws = _pool_workspace(dev, npts, nvox)
        call("coocc_lift_splat", ptr(depth), ptr(feat), ptr(geom), N, D_, H, W, C, c["ppb"], host_f32(c["lo_dx"]), B, *grid, ptr(out), C,
             ptr(ws), ws.numel(), 0)
        exact(out, R.lift_splat_fwd(c["depth"], c["feat"], c["keys"], nvox, F64), None, "lift_splat forward, COOCC_POOL_SEG=" + mode)
        rhs = float((out.cpu().to(F64) * c["dout"].to(F64)).sum())
        assert rhs == lhs_d == lhs_f, "%s: <dout, fwd> = %r, <d_depth, depth> = %r, <d_feat, feat> = %r (COOCC_POOL_SEG=%s)" % (
            what, rhs, lhs_d, lhs_f, mode)


@pytest.mark.parametrize("gname", list(R.POOL_GRIDS))
@pytest.mark.parametrize("shape", R.POOL, ids=POOL_IDS)
def test_pooling_adjoints_precise(dev, shape, gname):
    c = _pool_case(*shape, gname, False)
    what = "lift_splat_bwd %s %s" % (shape[:6], gname)
    dd, df = lift_splat_bwd(dev, c, shape, what)
    r64, r32 = R.lift_splat_adj(c["dout"], c["depth"], c["feat"], c["keys"], F64), R.lift_splat_adj(c["dout"], c["depth"], c["feat"], c["keys"], F32)
    precise(dd, r64[0], r32[0], what + " d_depth")
    precise(df, r64[1], r32[1], what + " d_feat")
    check_outside_pixel(dd, df, shape, what)
    dx = voxel_pool_bwd(dev, c, shape, what.replace("lift_splat", "voxel_pool"))
    same(dx, R.voxel_pool_adj(c["dout"], c["keys"], F64).to(F32), "voxel_pool_bwd %s %s" % (shape[:6], gname))      # a gather: dout's bits


# ============================================================================= coocc_scatter_add_rows
def scatter(dev, c, n, C, rows, ss, ds, what):
    dst = torch.full((rows + 2, ds), R.NAN, device=dev)
    dst[:rows, :C] = c["dst"].to(dev)
    dst[rows:] = SENT
    before = dst.clone()
    src = padded(dev, c["src"], ss) if n else torch.full((1, ss), R.NAN, device=dev)
    idx = D(dev, c["idx"][:n]) if n else torch.zeros(1, dtype=torch.int32, device=dev)
    call("coocc_scatter_add_rows", ptr(src), ss, ptr(idx), n, C, ptr(dst), ds)
    assert bool((dst[rows:] == SENT).all()) and bool(torch.isnan(dst[:rows, C:]).all()), what + ": wrote outside its rows"
    return dst[:rows, :C].cpu(), before, dst


@pytest.mark.parametrize("n,C,rows,ss,ds", R.SCATTER)
def test_scatter_add_rows(dev, n, C, rows, ss, ds):
    what = "scatter_add_rows %dx%d -> %d rows" % (n, C, rows)
    c = R.scatter_case(n, C, rows, exact=True)
    out, _, _ = scatter(dev, c, n, C, rows, ss, ds, what + " exact")
    exact(out, R.scatter_add(c["dst"], c["src"], c["idx"], F64), R.scatter_add(c["dst"], c["src"], c["idx"], F32), what + " exact")
    c = R.scatter_case(n, C, rows, exact=False)
    out, _, _ = scatter(dev, c, n, C, rows, ss, ds, what)
    assert not bool(torch.isnan(out).any())
    R.assert_scatter(out, c["dst"], c["src"], c["idx"], what)
    _, before, after = scatter(dev, c, 0, C, rows, ss, ds, what + " n=0")
    assert torch.equal(before.view(torch.int32), after.view(torch.int32)), what + ": n = 0 touched dst"
