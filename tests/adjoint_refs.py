"""Plain-torch restatements, input generators and the judging rules for the linear adjoint kernels of csrc/backward.hip:
``coocc_upsample_trilinear_bwd``, ``coocc_occhead_mix_bwd``, ``coocc_upsample_maps_bwd``, ``coocc_fine_sample_voxel_bwd``,
``coocc_fine_sample_img_bwd``, ``coocc_lift_splat_bwd``, ``coocc_voxel_pool_bwd`` and ``coocc_scatter_add_rows`` (and the forward
samplers of csrc/fine.hip, which share the projection and the normalisation).  Used by tests/test_adjoints_host.py (no GPU) and
tests/test_gpu_adjoints.py.

Every operation is written once as a function of a dtype, from the formulas in the kernels' comments: float64 is the reference,
float32 the anchor of ``util.assert_precise``.  A forward is a sum of weight x value over explicit taps; its adjoint is the explicit
transpose (``index_add`` of weight x gradient, or the transposed axis matrix) -- never torch autograd, so the float32 form is an
honest evaluation of the same sums.  tests/test_adjoints_host.py ties each restatement to torch (``F.interpolate``,
``F.grid_sample``, softmax, ``index_add``) in float64.

The rules:
  1. exact   -- ``assert_exact``: small-integer data and weights that are powers of two: every product and every partial sum is
                representable, so the fp32 result is the float64 one bit for bit in any order.  Pure gathers are exact too.
  2. precise -- ``util.assert_precise(out, ref64, ref32)`` with the project's C_MAX = 4, C_RMS = 2, on N(0, 1) data.
  3. scatter -- ``assert_scatter``: per element |out - ref| <= 2^-24 |ref| + (k - 1) 2^-24 sum |terms| with k contributions: k - 1
                fp32 additions in any order, each rounding a partial sum that is at most sum |terms| (first order in 2^-24; the
                2^-24 |ref| term takes the second order up), for the atomics of ``coocc_scatter_add_rows``."""
import math

import torch

import util
from norm_refs import assert_exact, bits_equal, gen, no_subnormals     # noqa: F401  (assert_exact: used through this module)

F32, F64 = torch.float32, torch.float64
U24 = 2.0 ** -24
NAN = float("nan")


def ints(shape, g, lo=-3, hi=3):
    """Integer-valued floats of [lo, hi]."""
    return torch.randint(lo, hi + 1, tuple(shape), generator=g).to(F32)


def normal(shape, g):
    return no_subnormals(torch.randn(tuple(shape), generator=g))


# ----------------------------------------------------------------------------- resampling (align_corners=False)
def lin_src(n_in, n_out, dtype, align_corners=False):
    """ATen's source-index rule for linear resampling of ``n_in`` -> ``n_out`` samples: (i0, i1, w0, w1) per output index.
    align_corners=False: s = max(0, (in / out) (d + 0.5) - 0.5), i0 = int(s), i1 = i0 + [i0 < in - 1], w1 = s - i0, w0 = 1 - w1;
    in == out is the identity.  (align_corners=True exists only as a wrong answer for the host test.)"""
    d = torch.arange(n_out, dtype=dtype)
    if n_in == n_out:
        i = torch.arange(n_out)
        return i, i.clone(), torch.ones(n_out, dtype=dtype), torch.zeros(n_out, dtype=dtype)
    if align_corners:
        s = d * (torch.tensor(n_in - 1, dtype=dtype) / torch.tensor(max(n_out - 1, 1), dtype=dtype))
    else:
        scale = torch.tensor(n_in, dtype=dtype) / torch.tensor(n_out, dtype=dtype)
        s = torch.clamp(scale * (d + 0.5) - 0.5, min=0)
    i0 = s.to(torch.int64)
    i1 = i0 + (i0 < n_in - 1).to(torch.int64)
    w1 = s - i0.to(dtype)
    return i0, i1, 1 - w1, w1


def axis_matrix(n_in, n_out, dtype, mutate=None):
    """[n_out, n_in]: row d holds the two tap weights of fine index d.  ``mutate`` makes the wrong matrices of the host test:
    "drop_last" loses the upper tap wherever it lands on the last coarse index, "shift" moves the window by one fine index,
    "align_corners" takes the other convention's weights."""
    i0, i1, w0, w1 = lin_src(n_in, n_out, dtype, align_corners=mutate == "align_corners")
    if mutate == "drop_last":
        w1 = torch.where((i1 == n_in - 1) & (i1 != i0), torch.zeros_like(w1), w1)
    m = torch.zeros(n_out, n_in, dtype=dtype)
    r = torch.arange(n_out)
    m.index_put_((r, i0), w0, accumulate=True)
    m.index_put_((r, i1), w1, accumulate=True)
    if mutate == "shift":
        m = torch.roll(m, 1, 0)
    return m


def _axes(coarse, fine, dtype, mutate):
    mutate = mutate if isinstance(mutate, (tuple, list)) else (mutate,) * len(coarse)
    return [axis_matrix(c, f, dtype, m) for c, f, m in zip(coarse, fine, mutate)]


def trilinear_fwd(coarse, fine_dims, dtype, mutate=None):
    """F.interpolate(mode="trilinear", align_corners=False) of channels-last ``coarse`` [B, Xc, Yc, Zc, C] to ``fine_dims``."""
    ax, ay, az = _axes(coarse.shape[1:4], fine_dims, dtype, mutate)
    v = torch.einsum("xa,bayzc->bxyzc", ax, coarse.to(dtype))
    v = torch.einsum("yb,nxbzc->nxyzc", ay, v)
    return torch.einsum("zd,nxydc->nxyzc", az, v)


def trilinear_adj(dfine, coarse_dims, dtype, mutate=None):
    """The transpose of ``trilinear_fwd``: dcoarse[b, a, ...] = sum_x w[x, a] ... dfine[b, x, ...]   (k_upsample_trilinear_bwd)."""
    ax, ay, az = _axes(coarse_dims, dfine.shape[1:4], dtype, mutate)
    v = torch.einsum("zd,nxyzc->nxydc", az, dfine.to(dtype))
    v = torch.einsum("yb,nxyzc->nxbzc", ay, v)
    return torch.einsum("xa,nxyzc->nayzc", ax, v)


def trilinear_adj_fused(dfine, coarse_dims, dtype):
    """The same adjoint with the three weights multiplied first (wx wy) wz and one sum over all fine voxels: another fp32 order."""
    ax, ay, az = _axes(coarse_dims, dfine.shape[1:4], dtype, None)
    w = (ax[:, None, None, :, None, None] * ay[None, :, None, None, :, None]) * az[None, None, :, None, None, :]
    return torch.einsum("xyzabd,nxyzc->nabdc", w, dfine.to(dtype))


def maps_fwd(maps, scale, dtype):
    """x``scale`` bilinear upsampling of the render maps [N, H, W, 4] -> (rgbs [N, sH, sW, 3], depths [N, sH, sW])."""
    N, H, W, _ = maps.shape
    ay, ax = axis_matrix(H, H * scale, dtype), axis_matrix(W, W * scale, dtype)
    up = torch.einsum("yh,nhwc->nywc", ay, maps.to(dtype))
    up = torch.einsum("xw,nywc->nyxc", ax, up)
    return up[..., :3], up[..., 3]


def maps_adj(drgbs, ddepths, N, H, W, scale, dtype, mutate=None):
    """dmaps [N, H, W, 4] of ``maps_fwd``; a gradient that is None contributes zeros (k_upsample_maps_bwd)."""
    ay, ax = axis_matrix(H, H * scale, dtype, mutate), axis_matrix(W, W * scale, dtype, mutate)
    d = torch.zeros(N, H * scale, W * scale, 4, dtype=dtype)
    if drgbs is not None:
        d[..., :3] = drgbs.to(dtype)
    if ddepths is not None:
        d[..., 3] = ddepths.to(dtype)
    v = torch.einsum("xw,nyxc->nywc", ax, d)
    return torch.einsum("yh,nywc->nhwc", ay, v)


# ----------------------------------------------------------------------------- OccHead mix
def mix_weights(wlogit, V0, L, dtype):
    """softmax over the L levels per level-0 voxel; a missing ``wlogit`` is all zeros (uniform weights)."""
    wl = torch.zeros(V0, L, dtype=dtype) if wlogit is None else wlogit.to(dtype).reshape(V0, L)
    e = torch.exp(wl - wl.max(1, keepdim=True).values)
    return e / e.sum(1, keepdim=True)


def mix_fwd(levels, wlogit, dtype):
    """out[v] = sum_l softmax(wlogit[v])_l up_l(level_l)[v]; levels: channels-last [B, Xl, Yl, Zl, C], level 0 sets the grid."""
    B, X0, Y0, Z0, C = levels[0].shape
    w = mix_weights(wlogit, B * X0 * Y0 * Z0, len(levels), dtype)
    ups = [trilinear_fwd(p, (X0, Y0, Z0), dtype).reshape(-1, C) for p in levels]
    return sum(w[:, l:l + 1] * ups[l] for l in range(len(levels)))


def mix_adj(levels, wlogit, dout, dtype, perm=None):
    """(g [L] of [V0, C], dwlogit [V0, L]) as k_occhead_mix_bwd writes them: g_l = w_l dout, dwlogit_l = w_l (dot_l - sum_k w_k dot_k)
    with dot_l = <dout, up_l>.  ``perm``: the softmax weights permuted over the levels (a wrong answer for the host test)."""
    B, X0, Y0, Z0, C = levels[0].shape
    L = len(levels)
    w = mix_weights(wlogit, B * X0 * Y0 * Z0, L, dtype)
    if perm is not None:
        w = w[:, perm]
    g = dout.to(dtype).reshape(-1, C)
    dots = torch.stack([(g * trilinear_fwd(p, (X0, Y0, Z0), dtype).reshape(-1, C)).sum(1) for p in levels], 1)
    mean = (w * dots).sum(1, keepdim=True)
    return [w[:, l:l + 1] * g for l in range(L)], w * (dots - mean)


def mix_level_grads(levels, gl, dtype):
    """The per-level scaled gradients pulled down to their own grids (what OccHeadMixFn.backward returns for the levels)."""
    B, X0, Y0, Z0, C = levels[0].shape
    return [trilinear_adj(g.reshape(B, X0, Y0, Z0, C), p.shape[1:4], dtype) for g, p in zip(gl, levels)]


# ----------------------------------------------------------------------------- voxel sampler
def voxel_taps(fine_xyz, final_size, dims, dtype):
    """The 8 taps of grid_sample(bilinear, zeros, align_corners=False) per fine point: (rows [nf, 8] into the X Y Z volume, weights
    [nf, 8], valid [nf, 8]).  g = (q / (final - 1) - 0.5) 2,  p = ((g + 1) size - 1) / 2."""
    base, frac = [], []
    for a in range(3):
        q = fine_xyz[a].to(dtype)
        g = (q / torch.tensor(final_size[a] - 1, dtype=dtype) - 0.5) * 2
        p = ((g + 1) * dims[a] - 1) / 2
        fl = torch.floor(p)
        base.append(fl.to(torch.int64))
        frac.append(p - fl)
    rows, wts, ok = [], [], []
    X, Y, Z = dims
    for a in range(2):
        for b in range(2):
            for d in range(2):
                x, y, z = base[0] + a, base[1] + b, base[2] + d
                wx = frac[0] if a else 1 - frac[0]
                wy = frac[1] if b else 1 - frac[1]
                wz = frac[2] if d else 1 - frac[2]
                v = (x >= 0) & (x < X) & (y >= 0) & (y < Y) & (z >= 0) & (z < Z)
                rows.append(torch.where(v, (x * Y + y) * Z + z, torch.zeros_like(x)))
                wts.append(wx * wy * wz)
                ok.append(v)
    return torch.stack(rows, 1), torch.stack(wts, 1), torch.stack(ok, 1)


def _gather_taps(src_rows, rows, wts, ok, dtype):
    w = torch.where(ok, wts, torch.zeros_like(wts))
    return (src_rows.to(dtype)[rows] * w[..., None]).sum(1)


def _scatter_taps(grad, rows, wts, ok, nrows, dtype, order=None):
    """index_add of weight x gradient, one contribution after the other: point by point, or (``order``: a seed) in a seeded
    permutation of the contributions -- the atomics kernels add theirs in an order that changes from run to run."""
    w = torch.where(ok, wts, torch.zeros_like(wts))
    contrib = (grad.to(dtype)[:, None, :] * w[..., None]).reshape(-1, grad.shape[1])
    rows = rows.reshape(-1)
    if order is not None:
        perm = torch.randperm(rows.numel(), generator=gen(order))
        rows, contrib = rows[perm], contrib[perm]
    return torch.zeros(nrows, grad.shape[1], dtype=dtype).index_add_(0, rows, contrib)


def sample_voxel_fwd(vol, fine_xyz, final_size, dtype):
    """feat [nf, C] of ``vol`` [X, Y, Z, C] at the fine points ``fine_xyz`` [3, nf]."""
    X, Y, Z, C = vol.shape
    return _gather_taps(vol.reshape(-1, C), *voxel_taps(fine_xyz, final_size, (X, Y, Z), dtype), dtype)


def sample_voxel_adj(dfeat, fine_xyz, final_size, dims, dtype, order=None):
    """dvol [X, Y, Z, C]: every tap row receives weight x dfeat[f]   (k_fine_sample_voxel_bwd)."""
    X, Y, Z = dims
    return _scatter_taps(dfeat, *voxel_taps(fine_xyz, final_size, dims, dtype), X * Y * Z, dtype, order).reshape(X, Y, Z, -1)


def fine_children(coarse_lin, dims, ratio=2):
    """The fine list of ``coarse_lin`` as the forward writes it: point f = o n + i, o = (a r + b) r + c, q = coarse r + (a, b, c)."""
    X, Y, Z = dims
    cz, cy, cx = coarse_lin % Z, coarse_lin // Z % Y, coarse_lin // (Z * Y)
    out = []
    for a in range(ratio):
        for b in range(ratio):
            for c in range(ratio):
                out.append(torch.stack([cx * ratio + a, cy * ratio + b, cz * ratio + c]))
    return torch.cat(out, 1).to(torch.int64)


# ----------------------------------------------------------------------------- image sampler
HDR, CAM = 17, 27          # csrc/fine.hip k_projection_params: 17 header floats, 27 per camera


def camera_rig(post_rot=False):
    """The two-camera rig of the image-sampler tests as a parameter block (float32 [17 + 27 ncam]) and its fine grid.
    Fine grid 12 x 10 x 6, voxel size 1, origin (-5.5, -4.5, -2.5), image 32 x 24 (wimg1 = 31, himg1 = 23), focal 14, centre
    (15.5, 11.5).  Camera 0: identity rotation at (0.3, 0.2, -9), sees every point.  Camera 1: at (-3.2, 0.1, 0.4) inside the grid,
    looking along +x (camera x = world y, camera y = world z, depth = world x): a quarter of the points are behind it.
    ``post_rot``: camera 1 with a post-rotation (a small rotation and scale about the image centre) and post-translation."""
    prm = torch.zeros(HDR + 2 * CAM, dtype=F64)
    prm[0:9] = torch.eye(3, dtype=F64).flatten()
    prm[9:12] = 1.0
    prm[12:15] = torch.tensor([-5.5, -4.5, -2.5], dtype=F64)
    prm[15], prm[16] = 31.0, 23.0
    K = torch.tensor([[14.0, 0, 15.5], [0, 14.0, 11.5], [0, 0, 1]], dtype=F64)
    inv_rot = [torch.eye(3, dtype=F64), torch.tensor([[0.0, 1, 0], [0, 0, 1], [1, 0, 0]], dtype=F64)]
    trans = [torch.tensor([0.3, 0.2, -9.0], dtype=F64), torch.tensor([-3.2, 0.1, 0.4], dtype=F64)]
    for cam in range(2):
        q = prm[HDR + cam * CAM:HDR + (cam + 1) * CAM]
        q[0:9], q[9:12], q[12:21] = inv_rot[cam].flatten(), trans[cam], K.flatten()
        q[21:25] = torch.tensor([1.0, 0, 0, 1], dtype=F64)
        if post_rot and cam == 1:
            c, s = 0.96 * math.cos(0.05), 0.96 * math.sin(0.05)
            q[21:25] = torch.tensor([c, -s, s, c], dtype=F64)
            q[25], q[26] = 15.5 - (c * 15.5 - s * 11.5) + 0.37, 11.5 - (s * 15.5 + c * 11.5) - 0.21
    grid = torch.stack(torch.meshgrid(torch.arange(12), torch.arange(10), torch.arange(6), indexing="ij")).reshape(3, -1)
    return prm.to(F32), grid.to(torch.int64)


def project(prm, fine_xyz, ncam, dtype):
    """The projection chain of k_fine_sample_img per (camera, point): (u2, v2 normalised to [-1, 1], depth d, mask, margin).
    ``margin``: the distance to the nearest branch of the mask d > 1e-5 && -1 < u2 < 1 && -1 < v2 < 1 (for a point behind the
    camera only the depth branch decides)."""
    p = prm.to(dtype)
    q3 = fine_xyz.to(dtype)
    pt = [q3[a] * p[9 + a] + p[12 + a] for a in range(3)]
    b = [p[3 * r] * pt[0] + p[3 * r + 1] * pt[1] + p[3 * r + 2] * pt[2] for r in range(3)]
    eps = torch.tensor(1e-5, dtype=F32).to(dtype)          # the kernel's float literal
    out = []
    for cam in range(ncam):
        q = p[HDR + cam * CAM:HDR + (cam + 1) * CAM]
        t = [b[a] - q[9 + a] for a in range(3)]
        c = [q[3 * r] * t[0] + q[3 * r + 1] * t[1] + q[3 * r + 2] * t[2] for r in range(3)]
        ix, iy, d = [q[12 + 3 * r] * c[0] + q[13 + 3 * r] * c[1] + q[14 + 3 * r] * c[2] for r in range(3)]
        u, v = ix / (d + eps), iy / (d + eps)
        u2 = q[21] * u + q[22] * v + q[25]
        v2 = q[23] * u + q[24] * v + q[26]
        u2 = (u2 / p[15] - 0.5) * 2
        v2 = (v2 / p[16] - 0.5) * 2
        front = d > eps
        m = front & (u2 > -1) & (u2 < 1) & (v2 > -1) & (v2 < 1)
        edge = torch.minimum(torch.minimum((u2 + 1).abs(), (1 - u2).abs()), torch.minimum((v2 + 1).abs(), (1 - v2).abs()))
        margin = torch.where(front, torch.minimum((d - eps).abs(), edge), (d - eps).abs())
        out.append((u2, v2, d, m, margin))
    return out


def img_taps(prm, fine_xyz, ncam, Hf, Wf, dtype, ignore_mask=None):
    """The taps of grid_sample(bilinear, zeros, align_corners=True) x mask over all cameras: (rows [nf, 4 ncam] into the
    [ncam, Hf, Wf] maps, weights, valid).  ``ignore_mask``: a camera whose mask is taken as true (a wrong answer for the host test)."""
    rows, wts, ok = [], [], []
    for cam, (u2, v2, _, m, _) in enumerate(project(prm, fine_xyz, ncam, dtype)):
        if cam == ignore_mask:
            m = torch.isfinite(u2) & torch.isfinite(v2) & (u2.abs() < 1e6) & (v2.abs() < 1e6)
        px, py = (u2 + 1) / 2 * (Wf - 1), (v2 + 1) / 2 * (Hf - 1)
        px, py = torch.where(m, px, torch.zeros_like(px)), torch.where(m, py, torch.zeros_like(py))
        flx, fly = torch.floor(px), torch.floor(py)
        x0, y0, ax, ay = flx.to(torch.int64), fly.to(torch.int64), px - flx, py - fly
        for yy in range(2):
            for xx in range(2):
                x, y = x0 + xx, y0 + yy
                v = m & (x >= 0) & (x < Wf) & (y >= 0) & (y < Hf)
                rows.append(torch.where(v, (cam * Hf + y) * Wf + x, torch.zeros_like(x)))
                wts.append((ax if xx else 1 - ax) * (ay if yy else 1 - ay))
                ok.append(v)
    return torch.stack(rows, 1), torch.stack(wts, 1), torch.stack(ok, 1)


def sample_img_fwd(img, prm, fine_xyz, dtype):
    """feat [nf, Ci] of the maps ``img`` [ncam, Hf, Wf, Ci], summed over the cameras that see the point."""
    ncam, Hf, Wf, Ci = img.shape
    return _gather_taps(img.reshape(-1, Ci), *img_taps(prm, fine_xyz, ncam, Hf, Wf, dtype), dtype)


def sample_img_adj(dfeat, prm, fine_xyz, ncam, Hf, Wf, dtype, ignore_mask=None, order=None):
    """dimg [ncam, Hf, Wf, Ci]   (k_fine_sample_img_bwd)."""
    taps = img_taps(prm, fine_xyz, ncam, Hf, Wf, dtype, ignore_mask)
    return _scatter_taps(dfeat, *taps, ncam * Hf * Wf, dtype, order).reshape(ncam, Hf, Wf, -1)


# ----------------------------------------------------------------------------- pooling
def voxel_keys(geom, lo_dx, pts_per_batch, grid, batch_zero=False, floor=False):
    """The voxel row of every point, or -1, with the fp32 arithmetic of ``voxel_of``: (x - lo) / dx in float (IEEE subtraction and
    division), truncated toward zero, then filtered; row = ((b X + ix) Y + iy) Z + iz with b = p / pts_per_batch.  The float64
    references take these keys as an input.  ``batch_zero`` / ``floor``: the wrong keys of the host test."""
    X, Y, Z = grid
    l = torch.tensor(lo_dx, dtype=F32)
    gq = (geom.to(F32) - l[:3]) / l[3:]
    idx = (torch.floor(gq) if floor else torch.trunc(gq)).to(torch.int64)
    kept = ((idx >= 0) & (idx < torch.tensor([X, Y, Z]))).all(1)
    b = torch.arange(geom.shape[0]) // pts_per_batch
    if batch_zero:
        b = torch.zeros_like(b)
    key = ((b * X + idx[:, 0]) * Y + idx[:, 1]) * Z + idx[:, 2]
    return torch.where(kept, key, torch.full_like(key, -1))


def pool_geometry(npts, lo_dx, grid, g):
    """Points spread over the grid and a margin around it (0.8 voxels below, 0.3 above), a sixth of them inside the grid but for one
    axis, which lies in the band (-1, 0) that truncation keeps in voxel 0 and a floor would drop."""
    l = torch.tensor(lo_dx, dtype=F64)
    size = torch.tensor(grid, dtype=F64)
    u = torch.rand(npts, 3, generator=g, dtype=F64) * (size + 1.1) - 0.8
    band = torch.arange(npts) % 6 == 0
    ax = torch.randint(0, 3, (npts,), generator=g)
    val = -(torch.rand(npts, generator=g, dtype=F64) * 0.9 + 0.05)
    inside = torch.rand(npts, 3, generator=g, dtype=F64) * (size - 0.2) + 0.1
    u = torch.where(band[:, None], inside, u)
    u[band, ax[band]] = val[band]
    return (u * l[3:] + l[:3]).to(F32)


def _pix(N, D, HW):
    p = torch.arange(N * D * HW)
    return p // (D * HW) * HW + p % HW


def lift_splat_fwd(depth, feat, keys, nvox, dtype):
    """out [nvox, C] = sum over the kept points of depth[p] feat[pixel(p)];  depth [N, D, H, W], feat [N H W, C]."""
    N, D, H, W = depth.shape
    prod = depth.to(dtype).reshape(-1, 1) * feat.to(dtype)[_pix(N, D, H * W)]
    kept = keys >= 0
    return torch.zeros(nvox, feat.shape[1], dtype=dtype).index_add_(0, keys[kept], prod[kept])


def lift_splat_adj(dout, depth, feat, keys, dtype):
    """(d_depth [N, D, H, W], d_feat [N H W, C]): d_depth[p] = <dout[key p], feat[pixel p]>, d_feat[pixel] = sum_d depth[p] dout[key p]."""
    N, D, H, W = depth.shape
    g = voxel_pool_adj(dout, keys, dtype)
    pix = _pix(N, D, H * W)
    d_depth = (g * feat.to(dtype)[pix]).sum(1).reshape(N, D, H, W)
    d_feat = torch.zeros(N * H * W, feat.shape[1], dtype=dtype).index_add_(0, pix, depth.to(dtype).reshape(-1, 1) * g)
    return d_depth, d_feat


def voxel_pool_adj(dout, keys, dtype):
    """dx[p] = dout[key p], zeros for a dropped point (a gather: exact in any type)."""
    g = dout.to(dtype)[keys.clamp(min=0)]
    return torch.where((keys >= 0)[:, None], g, torch.zeros_like(g))


# ----------------------------------------------------------------------------- scatter_add_rows
def scatter_add(dst, src, idx, dtype):
    """dst[idx[r]] += src[r] for idx[r] >= 0."""
    keep = idx >= 0
    return dst.to(dtype).clone().index_add_(0, idx[keep].to(torch.int64), src.to(dtype)[keep])


def scatter_bound(dst, src, idx):
    """(ref64, bound) per element of rule 3; the start value of ``dst`` is one of the k terms."""
    keep = idx >= 0
    i = idx[keep].to(torch.int64)
    ref = scatter_add(dst, src, idx, F64)
    mag = dst.to(F64).abs().index_add_(0, i, src.to(F64)[keep].abs())
    k = torch.ones(dst.shape[0], dtype=F64).index_add_(0, i, torch.ones(i.numel(), dtype=F64))
    return ref, U24 * ref.abs() + (k - 1)[:, None] * U24 * mag


def scatter_ratio(out, dst, src, idx, what=""):
    ref, bound = scatter_bound(dst, src, idx)
    err = (out.to(F64) - ref).abs()
    ratio = float(torch.where(bound > 0, err / bound.clamp(min=1e-300), torch.where(err > 0, torch.full_like(err, math.inf),
                                                                                  torch.zeros_like(err))).max())
    print("[scatter] %-40s worst share of the derived bound %.3f" % (what, ratio))
    util_log(dict(what=what, bound_share=ratio))
    return ratio


def assert_scatter(out, dst, src, idx, what=""):
    ratio = scatter_ratio(out, dst, src, idx, what)
    assert ratio <= 1.0, "%s: an element is %.3f of its bound from float64" % (what, ratio)
    return ratio


def util_log(st):
    import json
    import os
    log = os.environ.get("COOCC_PREC_LOG")
    if log:
        with open(log, "a") as f:
            f.write(json.dumps(st) + "\n")


# ----------------------------------------------------------------------------- rule 1 and the anchors of rule 2
def exact_ref(ref64, ref32=None):
    """The fp32 image of an exact case's float64 reference (+ 0.0: an empty or cancelling sum is +0.0), after checking that nothing
    was rounded -- and, when given, that the float32 restatement has the same bits."""
    r = ref64.to(F32) + 0.0
    assert bool((r.to(F64) == ref64).all()), "an exact case whose float64 reference is not representable in fp32"
    if ref32 is not None:
        assert bits_equal(ref32 + 0.0, r), "an exact case whose float32 and float64 restatements differ"
    return r


def atomics_anchor(adj32, ref64, seeds=(1, 2, 3)):
    """The anchor of rule 2 for the two sampler adjoints, whose fp32 atomics add a row's contributions in an order that changes
    from run to run: the worst (e_max, e_rms) of the fp32 restatement ``adj32(order=seed)`` under three seeded permutations of
    the contribution order.  One fixed order flatters: with a row of 410 contributions in a tensor of 480 values (a coarse voxel
    listed 50 times, C = 4) the point-by-point fp32 sum was 4.0e-7 / 3.2e-7 from float64, 300 seeded orders of the same sum
    reached 2.0e-6 / 7.1e-7 and 40 runs of the kernel 3.0e-7 ... 2.2e-6 / 2.3e-7 ... 7.5e-7."""
    errs = [util.errors(adj32(order=s), ref64) for s in seeds]
    return max(e[0] for e in errs), max(e[1] for e in errs)


def rejects(out, ref64, ref32):
    """True when rule 2 turns ``out`` down."""
    return not util.precision(out, ref64, ref32, what="(host) a wrong result")["ok"]


# ----------------------------------------------------------------------------- the cases (shared by the host and the GPU tests)
# coocc_upsample_trilinear_bwd: (B, C, coarse, fine)
TRI_EXACT = [(1, 4, (1, 1, 1), (8, 8, 8)), (2, 8, (3, 2, 4), (6, 4, 8)), (1, 4, (2, 3, 1), (16, 3, 8)), (1, 12, (5, 4, 2), (20, 16, 8))]
TRI_PRECISE = [(1, 4, (3, 5, 2), (20, 8, 3)), (2, 8, (7, 3, 4), (9, 24, 5)), (1, 68, (2, 2, 2), (3, 3, 3))]
TRI_COPY = (1, 4, (5, 5, 5), (5, 5, 5))
# coocc_occhead_mix_bwd: name -> (B, C, levels, logits): "none" = wlogit NULL, "normal" = 3 N(0, 1), "peak" = one level 40 above
MIX = {
    "L1": (1, 8, [(3, 2, 2)], "normal"),
    "L4": (2, 64, [(8, 6, 4), (4, 3, 2), (2, 2, 1), (8, 6, 4)], "normal"),
    "L3_c260": (1, 260, [(5, 3, 2), (3, 2, 2), (1, 1, 1)], "normal"),
    "null_logits": (1, 8, [(4, 4, 2), (2, 2, 1)], "none"),
    "peak": (2, 64, [(8, 6, 4), (4, 3, 2), (2, 2, 1), (8, 6, 4)], "peak"),
}
MIX_EXACT = ["L1", "null_logits"]          # uniform weights 1 and 1/2, factors 1 and 2: exact with integer data
# coocc_upsample_maps_bwd: (N, H, W, scale)
MAPS_EXACT = [(1, 1, 1, 16), (2, 3, 5, 2), (1, 1, 7, 16), (1, 4, 1, 4)]
MAPS_PRECISE = [(2, 3, 5, 16), (1, 2, 2, 3)]
MAPS_COPY = (3, 2, 3, 1)
# the voxel sampler: the volume, the final grid, the widths; the image sampler: the maps and the widths
VOX_DIMS, VOX_FINAL, VOX_C = (6, 5, 4), (12, 10, 8), [4, 64, 130]
IMG_MAPS, IMG_C = [(6, 8), (1, 1)], [4, 64, 100]
# the pooling adjoints: (N, D, H, W, C, B, grid) and the two voxel grids (lo, dx)
POOL = [(1, 1, 1, 1, 4, 1, (1, 1, 1)), (2, 9, 3, 5, 12, 2, (4, 3, 2)), (3, 5, 2, 3, 260, 1, (3, 3, 2)), (1, 70, 2, 2, 128, 1, (2, 2, 1))]
POOL_GRIDS = {"unit": [0.0, 0.0, 0.0, 1.0, 1.0, 1.0], "offset": [-1.3, 0.7, -0.4, 0.4, 0.8, 1.6]}
# coocc_scatter_add_rows: (n, C, rows, source stride, destination stride)
SCATTER = [(200, 16, 50, 16, 16), (1000, 3, 1, 5, 7)]


def tri_case(B, C, coarse, fine, exact, seed=0):
    g = gen(1000 * sum(fine) + 10 * C + B + seed)
    shape = (B,) + tuple(fine) + (C,)
    return dict(dfine=ints(shape, g, -4, 4) if exact else normal(shape, g),
                prior=ints((B,) + tuple(coarse) + (C,), g, -4, 4) if exact else normal((B,) + tuple(coarse) + (C,), g))


def mix_case(name, exact=False):
    B, C, dims, logits = MIX[name]
    g = gen(sum(map(ord, name)))
    draw = (lambda s: ints(s, g)) if exact else (lambda s: normal(s, g))
    levels = [draw((B,) + d + (C,)) for d in dims]
    V0, L = B * dims[0][0] * dims[0][1] * dims[0][2], len(dims)
    dout = ints((V0, C), g, -4, 4) if exact else normal((V0, C), g)
    wl = None
    if logits != "none":
        wl = no_subnormals(3 * torch.randn(V0, L, generator=g))
        if logits == "peak":                  # every second voxel: one level 40 above the others
            v = torch.arange(0, V0, 2)
            wl[v, (v // 2) % L] += 40.0
    return dict(B=B, C=C, dims=dims, levels=levels, wlogit=wl, dout=dout)


def vox_coarse_list():
    """The coarse voxels of the voxel-sampler cases: the 8 corners of the volume (their children hold every corner of the final
    grid, where half of the taps fall outside) and 12 others."""
    X, Y, Z = VOX_DIMS
    corners = [(x * Y + y) * Z + z for x in (0, X - 1) for y in (0, Y - 1) for z in (0, Z - 1)]
    others = torch.randperm(X * Y * Z, generator=gen(5))[:12].tolist()
    return torch.tensor(corners + others, dtype=torch.int32)


def vox_repeat_list():
    """The children of ``vox_coarse_list`` followed by one interior fine point 50 times over (eight rows of 50 contributions)."""
    return torch.cat([fine_children(vox_coarse_list().long(), VOX_DIMS), torch.tensor([[5], [7], [3]]).repeat(1, 50)], 1).contiguous()


def vox_corner_list():
    """The exact list: the 8 corners of the final grid (weights 1/2 per axis, p = -1/2 and size - 1/2), one of them 50 times over."""
    fx, fy, fz = (f - 1 for f in VOX_FINAL)
    pts = [(x, y, z) for x in (0, fx) for y in (0, fy) for z in (0, fz)] + [(fx, 0, fz)] * 50
    return torch.tensor(pts, dtype=torch.int64).t().contiguous()


def pool_case(N, D, H, W, C, B, grid, gname, exact):
    g = gen(N * 1000 + D * 100 + C + len(gname) + (7 if exact else 0))
    npts = N * D * H * W
    lo_dx = POOL_GRIDS[gname]
    geom = pool_geometry(npts, lo_dx, grid, g).reshape(N, D, H * W, 3)
    if N * H * W > 1:                          # the last pixel's whole ray leaves the grid
        l = torch.tensor(lo_dx, dtype=F32)
        geom[N - 1, :, H * W - 1] = l[:3] - 5 * l[3:]
    geom = geom.reshape(npts, 3).contiguous()
    nvox = B * grid[0] * grid[1] * grid[2]
    draw = (lambda s, a=3: ints(s, g, -a, a)) if exact else (lambda s, a=3: normal(s, g))
    return dict(geom=geom, lo_dx=lo_dx, ppb=npts // B, nvox=nvox, keys=voxel_keys(geom, lo_dx, npts // B, grid),
                depth=draw((N, D, H, W)), feat=draw((N * H * W, C)), dout=draw((nvox, C), 4))


def scatter_case(n, C, rows, exact):
    g = gen(n + C + rows)
    idx = torch.randint(0, rows, (n,), generator=g).to(torch.int32)
    idx[torch.arange(n) % 7 == 3] = -1
    draw = (lambda s: ints(s, g)) if exact else (lambda s: normal(s, g))
    return dict(idx=idx, src=draw((n, C)), dst=draw((rows, C)))
