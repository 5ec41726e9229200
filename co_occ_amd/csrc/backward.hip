// Backward kernels of the HBM-bound ops: G1 row gather, P2 voxel pooling / fused
// lift-splat, R2 render composite + x16 map upsample + render losses.  The reference gets these from
// torch autograd over its eager ops (index_put / cumprod / interpolate backward); here each is one kernel.
// Index-producing steps (FPS, ball query, top-K, assignment, voxel keys) are non-differentiable.
#include "common.h"
#include "colreduce.h"

typedef float f32x4 __attribute__((ext_vector_type(4)));

// ------------------------------------------------------------------ G1: rows gather / scatter-add
__global__ __launch_bounds__(256) void k_gather_rows(const float* __restrict__ src, int src_stride,
                                                      const int32_t* __restrict__ idx, int n, int C,
                                                      float* __restrict__ dst, int dst_stride) {
  const int c4 = C >> 2;
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  if (i >= (long long)n * c4) return;
  const int r = (int)(i / c4), c = (int)(i % c4) * 4;
  const int s = idx[r];
  f32x4 v = {0.f, 0.f, 0.f, 0.f};
  if (s >= 0) v = *(const f32x4*)(src + (size_t)s * src_stride + c);
  *(f32x4*)(dst + (size_t)r * dst_stride + c) = v;
}

extern "C" int coocc_gather_rows(const float* src, int src_stride, const int32_t* idx, int n, int C, float* dst,
                                 int dst_stride, void* stream) {
  COOCC_CHECK_ARG(src && idx && dst && n >= 0 && C > 0 && C % 4 == 0 && src_stride % 4 == 0 && dst_stride % 4 == 0,
                  "gather_rows: bad args (C, strides % 4 == 0)");
  if (n == 0) return COOCC_OK;
  hipLaunchKernelGGL(k_gather_rows, dim3(cdiv((long long)n * (C / 4), 256)), dim3(256), 0, as_stream(stream), src, src_stride,
                     idx, n, C, dst, dst_stride);
  COOCC_LAUNCH_CHECK("k_gather_rows");
  return COOCC_OK;
}

// dst[idx[r]] += src[r]   (several r may share a row: hardware fp32 atomics, order not fixed)
__global__ __launch_bounds__(256) void k_scatter_add_rows(const float* __restrict__ src, int src_stride,
                                                           const int32_t* __restrict__ idx, int n, int C,
                                                           float* __restrict__ dst, int dst_stride) {
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  if (i >= (long long)n * C) return;
  const int r = (int)(i / C), c = (int)(i % C);
  const int d = idx[r];
  if (d >= 0) unsafeAtomicAdd(dst + (size_t)d * dst_stride + c, src[(size_t)r * src_stride + c]);
}

extern "C" int coocc_scatter_add_rows(const float* src, int src_stride, const int32_t* idx, int n, int C, float* dst,
                                      int dst_stride, void* stream) {
  COOCC_CHECK_ARG(src && idx && dst && n >= 0 && C > 0, "scatter_add_rows: bad args");
  COOCC_CHECK_ARG(src_stride >= C && dst_stride >= C, "scatter_add_rows: row strides below C");
  if (n == 0) return COOCC_OK;
  hipLaunchKernelGGL(k_scatter_add_rows, dim3(cdiv((long long)n * C, 256)), dim3(256), 0, as_stream(stream), src, src_stride,
                     idx, n, C, dst, dst_stride);
  COOCC_LAUNCH_CHECK("k_scatter_add_rows");
  return COOCC_OK;
}

// ------------------------------------------------------------------ P2 backward
// same quantisation as pool.hip (truncate toward zero, then filter)
__device__ __forceinline__ int voxel_of(float x, float y, float z, int b, float lox, float loy, float loz, float dx, float dy,
                                        float dz, int X, int Y, int Z) {
  float gx = __fdiv_rn(x - lox, dx), gy = __fdiv_rn(y - loy, dy), gz = __fdiv_rn(z - loz, dz);
  long long ix = (long long)gx, iy = (long long)gy, iz = (long long)gz;
  bool kept = ix >= 0 && ix < X && iy >= 0 && iy < Y && iz >= 0 && iz < Z;
  return kept ? (int)((((size_t)b * X + ix) * Y + iy) * Z + iz) : -1;
}

// voxel_pooling backward (= bev_pool_grad_kernel, bev_pool_cuda.cu:61-84, without the sort): dx[p] = dout[voxel(p)]
__global__ __launch_bounds__(256) void k_voxel_pool_bwd(const float* __restrict__ dout, int dout_stride,
                                                         const float* __restrict__ geom, int npts, int pts_per_batch, int C,
                                                         float lox, float loy, float loz, float dx, float dy, float dz,
                                                         int X, int Y, int Z, float* __restrict__ dxr) {
  const int c4 = C >> 2;
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  if (i >= (long long)npts * c4) return;
  const int p = (int)(i / c4), c = (int)(i % c4) * 4;
  const int v = voxel_of(geom[(size_t)p * 3], geom[(size_t)p * 3 + 1], geom[(size_t)p * 3 + 2], p / pts_per_batch, lox, loy, loz,
                         dx, dy, dz, X, Y, Z);
  f32x4 g = {0.f, 0.f, 0.f, 0.f};
  if (v >= 0) g = *(const f32x4*)(dout + (size_t)v * dout_stride + c);
  *(f32x4*)(dxr + (size_t)p * C + c) = g;
}

extern "C" int coocc_voxel_pool_bwd(const float* dout, int dout_stride, const float* geom, int npts, int pts_per_batch,
                                    int C, const float* lo_dx_host, int B, int X, int Y, int Z, float* dx, void* stream) {
  COOCC_CHECK_ARG(dout && geom && dx && lo_dx_host && npts > 0 && pts_per_batch > 0 && C > 0 && C % 4 == 0 && dout_stride % 4 == 0,
                  "voxel_pool_bwd: bad args");
  COOCC_CHECK_ARG(dout_stride >= C && B > 0 && X > 0 && Y > 0 && Z > 0, "voxel_pool_bwd: dout_stride < C or an empty grid");
  // the batch index p / pts_per_batch of the last point must stay inside the B gradient volumes
  COOCC_CHECK_ARG((long long)npts <= (long long)B * pts_per_batch, "voxel_pool_bwd: more points than B * pts_per_batch");
  const float* l = lo_dx_host;
  hipLaunchKernelGGL(k_voxel_pool_bwd, dim3(cdiv((long long)npts * (C / 4), 256)), dim3(256), 0, as_stream(stream), dout,
                     dout_stride, geom, npts, pts_per_batch, C, l[0], l[1], l[2], l[3], l[4], l[5], X, Y, Z, dx);
  COOCC_LAUNCH_CHECK("k_voxel_pool_bwd");
  return COOCC_OK;
}

// fused lift-splat backward: one wave per pixel (n,h,w), lanes along channels, loop over the D depth bins:
//   d_depth[n,d,h,w] = <dout[voxel(p)], feat[n,h,w,:]>      d_feat[n,h,w,:] = sum_d depth[p] * dout[voxel(p)]
// No atomics, fixed order: deterministic.
__global__ __launch_bounds__(256) void k_lift_splat_bwd(const float* __restrict__ dout, int dout_stride,
                                                         const float* __restrict__ depth, const float* __restrict__ feat,
                                                         const float* __restrict__ geom, int N, int D, int HW, int C,
                                                         int pts_per_batch, float lox, float loy, float loz, float dx,
                                                         float dy, float dz, int X, int Y, int Z,
                                                         float* __restrict__ d_depth, float* __restrict__ d_feat) {
  const int pix = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (pix >= N * HW) return;
  const int n = pix / HW, hw = pix % HW;
  for (int c0 = 0; c0 < C; c0 += 256) {
    const int c = c0 + lane * 4;
    const bool on = c < C;
    f32x4 f = {0.f, 0.f, 0.f, 0.f}, acc = {0.f, 0.f, 0.f, 0.f};
    if (on) f = *(const f32x4*)(feat + (size_t)pix * C + c);
    for (int d = 0; d < D; ++d) {
      const int p = (n * D + d) * HW + hw;
      const int v = voxel_of(geom[(size_t)p * 3], geom[(size_t)p * 3 + 1], geom[(size_t)p * 3 + 2], p / pts_per_batch, lox, loy,
                             loz, dx, dy, dz, X, Y, Z);
      f32x4 g = {0.f, 0.f, 0.f, 0.f};
      if (v >= 0 && on) g = *(const f32x4*)(dout + (size_t)v * dout_stride + c);
      float dot = g[0] * f[0] + g[1] * f[1] + g[2] * f[2] + g[3] * f[3];
      for (int m = 32; m > 0; m >>= 1) dot += __shfl_xor(dot, m);
      if (lane == 0) {
        if (c0 == 0) d_depth[p] = dot; else d_depth[p] += dot;
      }
      acc = acc + depth[p] * g;
    }
    if (on) *(f32x4*)(d_feat + (size_t)pix * C + c) = acc;
  }
}

extern "C" int coocc_lift_splat_bwd(const float* dout, int dout_stride, const float* depth, const float* feat_nhwc,
                                    const float* geom, int N, int D, int H, int W, int C, int pts_per_batch,
                                    const float* lo_dx_host, int B, int X, int Y, int Z, float* d_depth,
                                    float* d_feat_nhwc, void* stream) {
  COOCC_CHECK_ARG(dout && depth && feat_nhwc && geom && lo_dx_host && d_depth && d_feat_nhwc && N > 0 && D > 0 && H > 0 && W > 0,
                  "lift_splat_bwd: bad args");
  COOCC_CHECK_ARG(C > 0 && C % 4 == 0 && dout_stride % 4 == 0 && pts_per_batch > 0, "lift_splat_bwd: C, stride % 4 == 0");
  COOCC_CHECK_ARG(dout_stride >= C && B > 0 && X > 0 && Y > 0 && Z > 0, "lift_splat_bwd: dout_stride < C or an empty grid");
  // the batch index p / pts_per_batch of the last point must stay inside the B gradient volumes
  COOCC_CHECK_ARG((long long)N * D * H * W <= (long long)B * pts_per_batch, "lift_splat_bwd: more points than B * pts_per_batch");
  const float* l = lo_dx_host;
  hipLaunchKernelGGL(k_lift_splat_bwd, dim3(cdiv((long long)N * H * W, 4)), dim3(256), 0, as_stream(stream), dout, dout_stride,
                     depth, feat_nhwc, geom, N, D, H * W, C, pts_per_batch, l[0], l[1], l[2], l[3], l[4], l[5], X, Y, Z, d_depth,
                     d_feat_nhwc);
  COOCC_LAUNCH_CHECK("k_lift_splat_bwd");
  return COOCC_OK;
}

// ------------------------------------------------------------------ R2 backward
// Forward (render.hip k_render_nearest; coocc_ray.py:574-625): per ray, samples k = 0..D-1 at voxel v_k:
//   sigma_k = relu(t[v_k].s), a_k = 1 - exp(-relu(sigma_k * dist_k)), c_k = in_k ? sigmoid(t[v_k].rgb) : 0.5,
//   T_k = prod_{j<k} (1 - a_j + 1e-10), w_k = a_k T_k, rgb = sum w_k c_k, depth = sum w_k z_k.
// Backward, with q_k = <g_rgb, c_k> + g_depth z_k and S_k = sum_{j>k} q_j w_j:
//   dL/dc_k = w_k g_rgb;  dL/da_k = q_k T_k - S_k / (1 - a_k + 1e-10);  da_k/ds_k = exp(-sigma_k dist_k) dist_k [s_k > 0]
// One wave per ray, lanes along depth (CH consecutive samples per lane), prefix product by an up-scan,
// suffix sum by a down-scan; gradients are added to dtable[v_k] with hardware fp32 atomics.
__global__ __launch_bounds__(256) void k_render_nearest_bwd(const float* __restrict__ table, int Y, int Z,
                                                             const float* __restrict__ geom,
                                                             const float* __restrict__ zvals, int N, int D, int H, int W,
                                                             float lox, float loy, float loz, float dx, float dy, float dz,
                                                             float nx, float ny, float nz, const float* __restrict__ dmaps,
                                                             float* __restrict__ dtable) {
  const int ray = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (ray >= N * H * W) return;
  const int w = ray % W, h = (ray / W) % H, n = ray / (W * H);
  const f32x4 gm = *(const f32x4*)(dmaps + (size_t)ray * 4);     // d rgb (3), d depth
  const int CH = (D + 63) / 64;                                   // <= 4 (D <= 256)
  const int d0 = lane * CH;
  int vox[4], inb[4];
  float al[4], cr[4], cg[4], cb[4], dist[4], sg[4], zv[4];
  auto pos = [&](int d, int& ix, int& iy, int& iz) -> bool {
    const float* g = geom + ((((size_t)n * D + d) * H + h) * W + w) * 3;
    float gx = __fdiv_rn(g[0] - lox, dx), gy = __fdiv_rn(g[1] - loy, dy), gz = __fdiv_rn(g[2] - loz, dz);
    bool in = gx >= 0.f && gx < nx && gy >= 0.f && gy < ny && gz >= 0.f && gz < nz;
    ix = in ? (int)gx : 0; iy = in ? (int)gy : 0; iz = in ? (int)gz : 0;
    return in;
  };
  float prod = 1.f;
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    al[j] = 0.f; cr[j] = cg[j] = cb[j] = 0.f; vox[j] = -1; inb[j] = 0; dist[j] = 0.f; sg[j] = 0.f; zv[j] = 0.f;
    const int d = d0 + j;
    if (j < CH && d < D) {
      int x0, y0, z0, x1, y1, z1;
      inb[j] = pos(d, x0, y0, z0);
      vox[j] = (x0 * Y + y0) * Z + z0;
      dist[j] = 1e10f;
      if (d + 1 < D) {
        pos(d + 1, x1, y1, z1);
        float ex = (float)(x1 - x0), ey = (float)(y1 - y0), ez = (float)(z1 - z0);
        dist[j] = __fsqrt_rn(ex * ex + ey * ey + ez * ez);
      }
      const f32x4 t = *(const f32x4*)(table + (size_t)vox[j] * 4);
      sg[j] = t[0];
      zv[j] = zvals[d];
      al[j] = 1.f - expf(-fmaxf(fmaxf(t[0], 0.f) * dist[j], 0.f));
      cr[j] = inb[j] ? 1.f / (1.f + expf(-t[1])) : 0.5f;
      cg[j] = inb[j] ? 1.f / (1.f + expf(-t[2])) : 0.5f;
      cb[j] = inb[j] ? 1.f / (1.f + expf(-t[3])) : 0.5f;
      prod *= 1.f - al[j] + 1e-10f;
    }
  }
  float inc = prod;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    float v = __shfl_up(inc, o);
    if (lane >= o) inc *= v;
  }
  float T = __shfl_up(inc, 1);
  if (lane == 0) T = 1.f;
  float Tk[4], wk[4], qw = 0.f;
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    Tk[j] = T; wk[j] = al[j] * T;
    qw += (gm[0] * cr[j] + gm[1] * cg[j] + gm[2] * cb[j] + gm[3] * zv[j]) * wk[j];
    T *= 1.f - al[j] + 1e-10f;
  }
  // exclusive suffix sum of q*w across lanes
  float suf = qw;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    float v = __shfl_down(suf, o);
    if (lane + o < 64) suf += v;
  }
  float S = __shfl_down(suf, 1);
  if (lane == 63) S = 0.f;
#pragma unroll
  for (int j = 3; j >= 0; --j) {
    const int d = d0 + j;
    if (j < CH && d < D) {
      const float q = gm[0] * cr[j] + gm[1] * cg[j] + gm[2] * cb[j] + gm[3] * zv[j];
      const float da = q * Tk[j] - S / (1.f - al[j] + 1e-10f);
      const float sig = fmaxf(sg[j], 0.f);
      const float ds = (sg[j] > 0.f && sig * dist[j] > 0.f) ? da * expf(-sig * dist[j]) * dist[j] : 0.f;
      float* o = dtable + (size_t)vox[j] * 4;
      if (ds != 0.f) unsafeAtomicAdd(o, ds);
      if (inb[j] && wk[j] != 0.f) {
        unsafeAtomicAdd(o + 1, wk[j] * gm[0] * cr[j] * (1.f - cr[j]));
        unsafeAtomicAdd(o + 2, wk[j] * gm[1] * cg[j] * (1.f - cg[j]));
        unsafeAtomicAdd(o + 3, wk[j] * gm[2] * cb[j] * (1.f - cb[j]));
      }
      S += q * wk[j];
    }
  }
}

extern "C" int coocc_render_nearest_bwd(const float* table, int X, int Y, int Z, const float* geom, const float* zvals,
                                        int N, int D, int H, int W, const float* bounds_host, const float* dmaps,
                                        float* dtable, void* stream) {
  COOCC_CHECK_ARG(table && geom && zvals && bounds_host && dmaps && dtable, "render_nearest_bwd: null pointer");
  COOCC_CHECK_ARG(N > 0 && D > 0 && D <= 256 && H > 0 && W > 0, "render_nearest_bwd: bad sizes (D <= 256)");
  const float* bd = bounds_host;
  float dx = bd[2], dy = bd[5], dz = bd[8];
  float bx = bd[0] + bd[2] / 2.0f, by = bd[3] + bd[5] / 2.0f, bz = bd[6] + bd[8] / 2.0f;
  float lox = bx - dx / 2.f, loy = by - dy / 2.f, loz = bz - dz / 2.f;
  float nx = (bd[1] - bd[0]) / bd[2], ny = (bd[4] - bd[3]) / bd[5], nz = (bd[7] - bd[6]) / bd[8];
  COOCC_CHECK_ARG(nx <= (float)X && ny <= (float)Y && nz <= (float)Z, "render_nearest_bwd: render bounds exceed the voxel volume");
  hipStream_t s = as_stream(stream);
  COOCC_HIP(hipMemsetAsync(dtable, 0, sizeof(float) * 4 * (size_t)X * Y * Z, s));
  hipLaunchKernelGGL(k_render_nearest_bwd, dim3(cdiv((long long)N * H * W, 4)), dim3(256), 0, s, table, Y, Z, geom, zvals, N, D,
                     H, W, lox, loy, loz, dx, dy, dz, nx, ny, nz, dmaps, dtable);
  COOCC_LAUNCH_CHECK("k_render_nearest_bwd");
  return COOCC_OK;
}

// x`scale` bilinear upsample (align_corners=False) adjoint: one wave per coarse pixel gathers from the fine
// pixels whose two source taps include it (deterministic, no atomics).
struct LinB { int i0, i1; float w0, w1; };
__device__ __forceinline__ LinB lin_srcb(int dst, int in, int out) {
  LinB r;
  if (in == out) { r.i0 = r.i1 = dst; r.w0 = 1.f; r.w1 = 0.f; return r; }
  float scale = (float)in / (float)out;
  float s = scale * ((float)dst + 0.5f) - 0.5f;
  s = s < 0.f ? 0.f : s;
  r.i0 = (int)s;
  r.i1 = r.i0 + (r.i0 < in - 1 ? 1 : 0);
  r.w1 = s - (float)r.i0;
  r.w0 = 1.f - r.w1;
  return r;
}

__global__ COOCC_SCALAR_FP32 __launch_bounds__(256) void k_upsample_maps_bwd(const float* __restrict__ drgbs, const float* __restrict__ ddepths,
                                                            int N, int H, int W, int scale, float* __restrict__ dmaps) {
  const int pix = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (pix >= N * H * W) return;
  const int w = pix % W, h = (pix / W) % H, n = pix / (W * H);
  const int oH = H * scale, oW = W * scale;
  const int ylo = h == 0 ? 0 : max(0, (h - 1) * scale), yhi = h == H - 1 ? oH - 1 : min(oH - 1, (h + 2) * scale);
  const int xlo = w == 0 ? 0 : max(0, (w - 1) * scale), xhi = w == W - 1 ? oW - 1 : min(oW - 1, (w + 2) * scale);
  const int nxr = xhi - xlo + 1, tot = (yhi - ylo + 1) * nxr;
  float a0 = 0.f, a1 = 0.f, a2 = 0.f, a3 = 0.f;
  for (int i = lane; i < tot; i += 64) {
    const int oy = ylo + i / nxr, ox = xlo + i % nxr;
    const LinB ly = lin_srcb(oy, H, oH), lx = lin_srcb(ox, W, oW);
    const float wy = (ly.i0 == h ? ly.w0 : 0.f) + (ly.i1 == h ? ly.w1 : 0.f);
    const float wx = (lx.i0 == w ? lx.w0 : 0.f) + (lx.i1 == w ? lx.w1 : 0.f);
    const float wt = wy * wx;
    if (wt != 0.f) {
      const size_t p = ((size_t)n * oH + oy) * oW + ox;
      if (drgbs) { a0 += wt * drgbs[p * 3]; a1 += wt * drgbs[p * 3 + 1]; a2 += wt * drgbs[p * 3 + 2]; }
      if (ddepths) a3 += wt * ddepths[p];
    }
  }
  for (int m = 32; m > 0; m >>= 1) {
    a0 += __shfl_xor(a0, m); a1 += __shfl_xor(a1, m); a2 += __shfl_xor(a2, m); a3 += __shfl_xor(a3, m);
  }
  if (lane == 0) *(f32x4*)(dmaps + (size_t)pix * 4) = f32x4{a0, a1, a2, a3};
}

extern "C" int coocc_upsample_maps_bwd(const float* drgbs, const float* ddepths, int N, int H, int W, int scale,
                                       float* dmaps, void* stream) {
  COOCC_CHECK_ARG(dmaps && (drgbs || ddepths) && N > 0 && H > 0 && W > 0 && scale >= 1, "upsample_maps_bwd: bad args");
  hipLaunchKernelGGL(k_upsample_maps_bwd, dim3(cdiv((long long)N * H * W, 4)), dim3(256), 0, as_stream(stream), drgbs, ddepths, N,
                     H, W, scale, dmaps);
  COOCC_LAUNCH_CHECK("k_upsample_maps_bwd");
  return COOCC_OK;
}

// render losses backward (coocc_ray.py:423-433): gl[0] = dL/d loss_depth_render, gl[1] = dL/d loss_rgb;
// nfg = number of foreground pixels (out[2] of coocc_render_losses).
__global__ __launch_bounds__(256) void k_render_losses_bwd(const float* __restrict__ rgbs, const float* __restrict__ depths,
                                                            const float* __restrict__ rgb_gt,
                                                            const float* __restrict__ depth_gt, size_t npix, float D,
                                                            const float* __restrict__ losses_out,
                                                            const float* __restrict__ gl, float* __restrict__ drgbs,
                                                            float* __restrict__ ddepths) {
  const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= npix) return;
  const float nfg = losses_out[2];
  float g = (depth_gt[i] - (2.f - 0.5f / 2.f)) / 0.5f;
  g = fminf(fmaxf(g, 0.f), D);
  ddepths[i] = g > 0.f ? gl[0] * 2.f * (depths[i] / D - g / D) / (D * nfg) : 0.f;
  const float k = gl[1] * 2.f / (3.f * (float)npix);
  for (int c = 0; c < 3; ++c) drgbs[i * 3 + c] = k * (rgbs[i * 3 + c] - rgb_gt[i * 3 + c]);
}

extern "C" int coocc_render_losses_bwd(const float* rgbs, const float* depths, const float* rgb_gt, const float* depth_gt,
                                       int64_t npix, int D, const float* losses_out, const float* gl, float* drgbs,
                                       float* ddepths, void* stream) {
  COOCC_CHECK_ARG(rgbs && depths && rgb_gt && depth_gt && losses_out && gl && drgbs && ddepths && npix > 0 && D > 0,
                  "render_losses_bwd: bad args");
  hipLaunchKernelGGL(k_render_losses_bwd, dim3(cdiv(npix, 256)), dim3(256), 0, as_stream(stream), rgbs, depths, rgb_gt, depth_gt,
                     (size_t)npix, (float)D, losses_out, gl, drgbs, ddepths);
  COOCC_LAUNCH_CHECK("k_render_losses_bwd");
  return COOCC_OK;
}

// ------------------------------------------------------------------ FPN trilinear upsample-add backward
// forward (interp.hip k_upsample_add, fpn3d.py:88-92): fine += trilinear(coarse -> fine size).  The fine
// gradient passes through unchanged; the coarse gradient is the adjoint of the interpolation, gathered per
// coarse voxel from the <= MAXC^3 fine voxels whose two taps per axis include it (deterministic).
constexpr int MAXC = 20;   // fine taps per coarse index and axis: up to ~2x the upsampling factor + 2 (factor <= 8)

__device__ __forceinline__ int axis_weights(int c, int in, int out, int& lo, float* w) {
  // fine indices d in [lo, lo+n) with weight w[d-lo] onto coarse index c
  const float inv = (float)out / (float)in;
  int dlo = in == out ? c : max(0, (int)floorf(((float)c - 0.5f) * inv - 0.5f) - 1);
  int dhi = in == out ? c : min(out - 1, (int)ceilf(((float)c + 1.5f) * inv - 0.5f) + 1);
  if (c == 0) dlo = 0;
  if (c == in - 1) dhi = out - 1;
  int first = -1, n = 0;
  for (int d = dlo; d <= dhi; ++d) {
    const LinB l = lin_srcb(d, in, out);
    const float wt = (l.i0 == c ? l.w0 : 0.f) + (l.i1 == c ? l.w1 : 0.f);
    if (wt != 0.f || first >= 0) {
      if (first < 0) first = d;
      if (d - first < MAXC) { w[d - first] = wt; n = d - first + 1; }
    }
  }
  lo = first < 0 ? 0 : first;
  return n;
}

__global__ __launch_bounds__(256) void k_upsample_trilinear_bwd(const float* __restrict__ dfine, float* __restrict__ dcoarse,
                                                                 int B, int C, int Xc, int Yc, int Zc, int Xf, int Yf,
                                                                 int Zf, int accumulate) {
  const int c4 = C >> 2;
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  if (i >= (long long)B * Xc * Yc * Zc * c4) return;
  const int c = (int)(i % c4) * 4;
  long long v = i / c4;
  const int z = (int)(v % Zc); v /= Zc;
  const int y = (int)(v % Yc); v /= Yc;
  const int x = (int)(v % Xc); const int b = (int)(v / Xc);
  float wx[MAXC], wy[MAXC], wz[MAXC];
  int x0, y0, z0;
  const int nx = axis_weights(x, Xc, Xf, x0, wx), ny = axis_weights(y, Yc, Yf, y0, wy), nz = axis_weights(z, Zc, Zf, z0, wz);
  f32x4 acc = {0.f, 0.f, 0.f, 0.f};
  for (int a = 0; a < nx; ++a)
    for (int bb = 0; bb < ny; ++bb) {
      const float wxy = wx[a] * wy[bb];
      if (wxy == 0.f) continue;
      for (int cc = 0; cc < nz; ++cc) {
        const float wt = wxy * wz[cc];
        if (wt != 0.f)
          acc = acc + wt * *(const f32x4*)(dfine + ((((size_t)b * Xf + x0 + a) * Yf + y0 + bb) * Zf + z0 + cc) * C + c);
      }
    }
  f32x4* o = (f32x4*)(dcoarse + ((((size_t)b * Xc + x) * Yc + y) * Zc + z) * C + c);
  *o = accumulate ? *o + acc : acc;
}

extern "C" int coocc_upsample_trilinear_bwd(const float* dfine, float* dcoarse, int B, int C, int Xc, int Yc, int Zc, int Xf,
                                            int Yf, int Zf, int accumulate, void* stream) {
  COOCC_CHECK_ARG(dfine && dcoarse && B > 0 && C > 0 && C % 4 == 0, "upsample_trilinear_bwd: bad args (C % 4 == 0)");
  COOCC_CHECK_ARG(Xc > 0 && Yc > 0 && Zc > 0, "upsample_trilinear_bwd: empty coarse grid");
  COOCC_CHECK_ARG(Xf <= 8 * Xc && Yf <= 8 * Yc && Zf <= 8 * Zc && Xf >= Xc && Yf >= Yc && Zf >= Zc,
                  "upsample_trilinear_bwd: supports upsampling factors up to 8");
  hipLaunchKernelGGL(k_upsample_trilinear_bwd, dim3(cdiv((long long)B * Xc * Yc * Zc * (C / 4), 256)), dim3(256), 0,
                     as_stream(stream), dfine, dcoarse, B, C, Xc, Yc, Zc, Xf, Yf, Zf, accumulate);
  COOCC_LAUNCH_CHECK("k_upsample_trilinear_bwd");
  return COOCC_OK;
}

// ------------------------------------------------------------------ OccHead multi-level mix backward
// forward (interp.hip k_occhead_mix, occ_head.py:155-166): out[v] = sum_l softmax(wlogit[v])_l * up_l(level_l)[v].
// One wave per level-0 voxel, lanes along channels: dot_l = <dout[v], up_l[v]> (wave reduction), softmax backward
//   dwlogit_l = w_l (dot_l - sum_k w_k dot_k),
// and the per-level scaled gradients g_l[v] = w_l * dout[v] (level 0 is written straight into dlevel0; the others
// go to scratch rows and are pulled down by coocc_upsample_trilinear_bwd, the adjoint gather).
struct MixLevelsB { const float* p[4]; float* g[4]; int X[4], Y[4], Z[4]; int L; };

__global__ __launch_bounds__(256) void k_occhead_mix_bwd(MixLevelsB lv, const float* __restrict__ wlogit,
                                                          const float* __restrict__ dout, float* __restrict__ dwlogit,
                                                          int B, int C) {
  const int X0 = lv.X[0], Y0 = lv.Y[0], Z0 = lv.Z[0];
  const long long V0 = (long long)B * X0 * Y0 * Z0;
  const long long v = ((long long)blockIdx.x * blockDim.x + threadIdx.x) >> 6;
  const int lane = threadIdx.x & 63;
  if (v >= V0) return;
  long long r = v;
  const int z = (int)(r % Z0); r /= Z0;
  const int y = (int)(r % Y0); r /= Y0;
  const int x = (int)(r % X0); const int b = (int)(r / X0);
  float w[4], dot[4] = {0.f, 0.f, 0.f, 0.f};
  float mx = -INFINITY;
  for (int l = 0; l < lv.L; ++l) { w[l] = wlogit ? wlogit[v * lv.L + l] : 0.f; mx = fmaxf(mx, w[l]); }
  float sum = 0.f;
  for (int l = 0; l < lv.L; ++l) { w[l] = expf(w[l] - mx); sum += w[l]; }
  for (int l = 0; l < lv.L; ++l) w[l] /= sum;
  for (int c = lane * 4; c < C; c += 256) {
    const f32x4 g = *(const f32x4*)(dout + v * C + c);
    for (int l = 0; l < lv.L; ++l) {
      const LinB lx = lin_srcb(x, lv.X[l], X0), ly = lin_srcb(y, lv.Y[l], Y0), lz = lin_srcb(z, lv.Z[l], Z0);
      const float* vol = lv.p[l];
      const int Xl = lv.X[l], Yl = lv.Y[l], Zl = lv.Z[l];
      auto at = [&](int xx, int yy, int zz) { return *(const f32x4*)(vol + ((((size_t)b * Xl + xx) * Yl + yy) * Zl + zz) * C + c); };
      const f32x4 s = lx.w0 * (ly.w0 * (lz.w0 * at(lx.i0, ly.i0, lz.i0) + lz.w1 * at(lx.i0, ly.i0, lz.i1)) +
                                ly.w1 * (lz.w0 * at(lx.i0, ly.i1, lz.i0) + lz.w1 * at(lx.i0, ly.i1, lz.i1))) +
                      lx.w1 * (ly.w0 * (lz.w0 * at(lx.i1, ly.i0, lz.i0) + lz.w1 * at(lx.i1, ly.i0, lz.i1)) +
                                ly.w1 * (lz.w0 * at(lx.i1, ly.i1, lz.i0) + lz.w1 * at(lx.i1, ly.i1, lz.i1)));
      dot[l] += g[0] * s[0] + g[1] * s[1] + g[2] * s[2] + g[3] * s[3];
      *(f32x4*)(lv.g[l] + v * C + c) = w[l] * g;
    }
  }
  for (int l = 0; l < lv.L; ++l)
    for (int m = 32; m > 0; m >>= 1) dot[l] += __shfl_xor(dot[l], m);
  if (lane == 0 && dwlogit) {
    float mean = 0.f;
    for (int l = 0; l < lv.L; ++l) mean += w[l] * dot[l];
    for (int l = 0; l < lv.L; ++l) dwlogit[v * lv.L + l] = w[l] * (dot[l] - mean);
  }
}

extern "C" int coocc_occhead_mix_bwd(const float* const* levels_host, const int* dims_host, int L, const float* wlogit,
                                     const float* dout, float* const* glevels_host, float* dwlogit, int B, int C,
                                     void* stream) {
  COOCC_CHECK_ARG(levels_host && dims_host && dout && glevels_host && L >= 1 && L <= 4 && C % 4 == 0, "occhead_mix_bwd: bad args");
  COOCC_CHECK_ARG(B > 0 && C > 0, "occhead_mix_bwd: B, C > 0");
  for (int l = 0; l < L; ++l) {
    COOCC_CHECK_ARG(levels_host[l] && glevels_host[l], "occhead_mix_bwd: null level or gradient pointer");
    COOCC_CHECK_ARG(dims_host[l * 3] > 0 && dims_host[l * 3 + 1] > 0 && dims_host[l * 3 + 2] > 0, "occhead_mix_bwd: empty level");
  }
  MixLevelsB lv;
  lv.L = L;
  for (int l = 0; l < 4; ++l) {
    lv.p[l] = l < L ? levels_host[l] : nullptr;
    lv.g[l] = l < L ? glevels_host[l] : nullptr;
    lv.X[l] = l < L ? dims_host[l * 3 + 0] : 1;
    lv.Y[l] = l < L ? dims_host[l * 3 + 1] : 1;
    lv.Z[l] = l < L ? dims_host[l * 3 + 2] : 1;
  }
  const long long V0 = (long long)B * lv.X[0] * lv.Y[0] * lv.Z[0];
  hipLaunchKernelGGL(k_occhead_mix_bwd, dim3(cdiv(V0 * 64, 256)), dim3(256), 0, as_stream(stream), lv, wlogit, dout, dwlogit, B, C);
  COOCC_LAUNCH_CHECK("k_occhead_mix_bwd");
  return COOCC_OK;
}

// ------------------------------------------------------------------ fine branch backward (C4)
// coocc_fine_sample_voxel backward: trilinear grid_sample(align_corners=False, zeros) adjoint.  One wave per fine
// point, lanes along channels; the 8 corner rows of dvol receive w * dfeat[f] with hardware fp32 atomics.
__global__ __launch_bounds__(256) void k_fine_sample_voxel_bwd(const float* __restrict__ dfeat, int dfeat_stride, int C, int X,
                                                                int Y, int Z, const int64_t* __restrict__ fine_xyz,
                                                                long long nf, float fx1, float fy1, float fz1,
                                                                float* __restrict__ dvol) {
  const long long f = ((long long)blockIdx.x * blockDim.x + threadIdx.x) >> 6;
  const int lane = threadIdx.x & 63;
  if (f >= nf) return;
  const int qx = (int)fine_xyz[f], qy = (int)fine_xyz[nf + f], qz = (int)fine_xyz[2 * nf + f];
  float gx = ((float)qx / fx1 - 0.5f) * 2.f, gy = ((float)qy / fy1 - 0.5f) * 2.f, gz = ((float)qz / fz1 - 0.5f) * 2.f;
  float px = ((gx + 1.f) * (float)X - 1.f) / 2.f, py = ((gy + 1.f) * (float)Y - 1.f) / 2.f, pz = ((gz + 1.f) * (float)Z - 1.f) / 2.f;
  float flx = floorf(px), fly = floorf(py), flz = floorf(pz);
  int x0 = (int)flx, y0 = (int)fly, z0 = (int)flz;
  float tx = px - flx, ty = py - fly, tz = pz - flz;
  float wx[2] = {1.f - tx, tx}, wy[2] = {1.f - ty, ty}, wz[2] = {1.f - tz, tz};
  for (int c = lane; c < C; c += 64) {
    const float g = dfeat[(size_t)f * dfeat_stride + c];
#pragma unroll
    for (int a = 0; a < 2; ++a)
#pragma unroll
      for (int b = 0; b < 2; ++b)
#pragma unroll
        for (int d = 0; d < 2; ++d) {
          int x = x0 + a, y = y0 + b, z = z0 + d;
          if ((unsigned)x < (unsigned)X && (unsigned)y < (unsigned)Y && (unsigned)z < (unsigned)Z)
            unsafeAtomicAdd(dvol + (((size_t)x * Y + y) * Z + z) * C + c, g * (wx[a] * wy[b] * wz[d]));
        }
  }
}

extern "C" int coocc_fine_sample_voxel_bwd(const float* dfeat, int dfeat_stride, int C, int X, int Y, int Z,
                                           const int64_t* fine_xyz, int64_t nfine, const int* final_size_host, float* dvol,
                                           void* stream) {
  COOCC_CHECK_ARG(dfeat && fine_xyz && final_size_host && dvol && C > 0 && nfine >= 0, "fine_sample_voxel_bwd: bad args");
  COOCC_CHECK_ARG(dfeat_stride >= C && X > 0 && Y > 0 && Z > 0, "fine_sample_voxel_bwd: dfeat_stride < C or an empty volume");
  // q / (final - 1) normalises the fine coordinate
  COOCC_CHECK_ARG(final_size_host[0] >= 2 && final_size_host[1] >= 2 && final_size_host[2] >= 2,
                  "fine_sample_voxel_bwd: final_size below 2");
  hipStream_t s = as_stream(stream);
  COOCC_HIP(hipMemsetAsync(dvol, 0, sizeof(float) * (size_t)X * Y * Z * C, s));
  if (nfine == 0) return COOCC_OK;
  hipLaunchKernelGGL(k_fine_sample_voxel_bwd, dim3(cdiv(nfine * 64, 256)), dim3(256), 0, s, dfeat, dfeat_stride, C, X, Y, Z, fine_xyz,
                     (long long)nfine, (float)(final_size_host[0] - 1), (float)(final_size_host[1] - 1),
                     (float)(final_size_host[2] - 1), dvol);
  COOCC_LAUNCH_CHECK("k_fine_sample_voxel_bwd");
  return COOCC_OK;
}

// nn.GroupNorm over rows [n, C] (+ReLU) backward.  y = relu(xhat * gamma + beta), xhat = (x - mean) * rstd per (row, group).
//   dxhat = dy * [y > 0] * gamma;   dx = rstd * (dxhat - mean(dxhat) - xhat * mean(dxhat * xhat))
//   dgamma = sum_rows dy' * xhat,   dbeta = sum_rows dy'     (column sums: per-block partials in LDS, then fp32 atomics)
// x is the PRE-norm input (the forward kernel works in place, so the caller keeps a copy), y the post-ReLU output.
// Statistics as the forward takes them (gn_group_stats: Acc = double for wide groups, whose two group means are summed in it as
// well).  dxhat is ONE rounded product in both loops (mul_unfused: never fused into the subtraction of its mean), so a group of one
// channel gives dx = 0 exactly.
template <typename Acc>
__device__ __forceinline__ void groupnorm_rows_bwd_group(const float* __restrict__ px, const float* __restrict__ py,
                                                         const float* __restrict__ pdy, int cpg, const float* __restrict__ gamma,
                                                         float eps, int relu, float* __restrict__ pdx, float* s_dgamma,
                                                         float* s_dbeta) {
  Acc mean;
  float rstd;
  gn_group_stats<Acc>(px, cpg, eps, mean, rstd);
  Acc m1 = 0, m2 = 0;
  for (int c = 0; c < cpg; ++c) {
    const float xh = (float)(px[c] - mean) * rstd;
    float g_ = pdy[c];
    if (relu && !(py[c] > 0.f)) g_ = 0.f;
    atomicAdd(&s_dgamma[c], g_ * xh);
    atomicAdd(&s_dbeta[c], g_);
    const float dxh = mul_unfused(g_, gamma[c]);
    m1 += dxh; m2 += (Acc)dxh * xh;
  }
  m1 /= (Acc)cpg; m2 /= (Acc)cpg;
  for (int c = 0; c < cpg; ++c) {
    const float xh = (float)(px[c] - mean) * rstd;
    float g_ = pdy[c];
    if (relu && !(py[c] > 0.f)) g_ = 0.f;
    pdx[c] = rstd * (mul_unfused(g_, gamma[c]) - (float)m1 - xh * (float)m2);
  }
}

__global__ __launch_bounds__(256) void k_groupnorm_rows_bwd(const float* __restrict__ x, const float* __restrict__ y,
                                                             const float* __restrict__ dy, long long n, int C, int stride,
                                                             int groups, const float* __restrict__ gamma, float eps, int relu,
                                                             float* __restrict__ dx, float* __restrict__ dgamma,
                                                             float* __restrict__ dbeta) {
  extern __shared__ float s_part[];   // [2][C]
  for (int i = threadIdx.x; i < 2 * C; i += 256) s_part[i] = 0.f;
  __syncthreads();
  const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n * groups) {
    const long long row = i / groups;
    const int g = (int)(i - row * groups);
    const int cpg = C / groups;
    const float* px = x + row * stride + g * cpg;
    const float* pdy = dy + row * stride + g * cpg;
    const float* py = y + row * stride + g * cpg;
    float* pdx = dx + row * stride + g * cpg;
    if (cpg > GN_WIDE_GROUP)
      groupnorm_rows_bwd_group<double>(px, py, pdy, cpg, gamma + g * cpg, eps, relu, pdx, s_part + g * cpg, s_part + C + g * cpg);
    else
      groupnorm_rows_bwd_group<float>(px, py, pdy, cpg, gamma + g * cpg, eps, relu, pdx, s_part + g * cpg, s_part + C + g * cpg);
  }
  __syncthreads();
  for (int c = threadIdx.x; c < C; c += 256) {
    if (dgamma) unsafeAtomicAdd(dgamma + c, s_part[c]);
    if (dbeta) unsafeAtomicAdd(dbeta + c, s_part[C + c]);
  }
}

extern "C" int coocc_groupnorm_rows_bwd(const float* x, const float* y, const float* dy, int64_t n, int C, int stride, int groups,
                                        const float* gamma, float eps, int relu, float* dx, float* dgamma, float* dbeta,
                                        void* stream) {
  COOCC_CHECK_ARG(x && y && dy && gamma && dx && C > 0 && groups > 0 && C % groups == 0 && stride >= C && C <= 4096,
                  "groupnorm_rows_bwd: bad args");
  hipStream_t s = as_stream(stream);
  if (dgamma) COOCC_HIP(hipMemsetAsync(dgamma, 0, sizeof(float) * C, s));
  if (dbeta) COOCC_HIP(hipMemsetAsync(dbeta, 0, sizeof(float) * C, s));
  if (n == 0) return COOCC_OK;
  hipLaunchKernelGGL(k_groupnorm_rows_bwd, dim3(cdiv(n * groups, 256)), dim3(256), 2 * C * sizeof(float), s, x, y, dy, (long long)n, C,
                     stride, groups, gamma, eps, relu, dx, dgamma, dbeta);
  COOCC_LAUNCH_CHECK("k_groupnorm_rows_bwd");
  return COOCC_OK;
}

// coocc_fine_sample_img backward: adjoint of the per-camera bilinear grid_sample(align_corners=True, zeros) * mask summed
// over cameras.  Same projection as the forward (fine.hip), one wave per fine point, lanes along channels, fp32 atomics
// into dimg:[ncam,Hf,Wf,Ci].  params: the block built by coocc_projection_params.
__global__ COOCC_SCALAR_FP32 __launch_bounds__(256) void k_fine_sample_img_bwd(const float* __restrict__ dfeat, int dfeat_stride, int ncam, int Ci,
                                                              int Hf, int Wf, const float* __restrict__ prm,
                                                              const int64_t* __restrict__ fine_xyz, long long nf,
                                                              float* __restrict__ dimg) {
  const long long f = ((long long)blockIdx.x * blockDim.x + threadIdx.x) >> 6;
  const int lane = threadIdx.x & 63;
  if (f >= nf) return;
  float p0 = (float)fine_xyz[f] * prm[9] + prm[12];
  float p1 = (float)fine_xyz[nf + f] * prm[10] + prm[13];
  float p2 = (float)fine_xyz[2 * nf + f] * prm[11] + prm[14];
  float bx = prm[0] * p0 + prm[1] * p1 + prm[2] * p2;
  float by = prm[3] * p0 + prm[4] * p1 + prm[5] * p2;
  float bz = prm[6] * p0 + prm[7] * p1 + prm[8] * p2;
  const float wimg1 = prm[15], himg1 = prm[16];
  for (int cam = 0; cam < ncam; ++cam) {
    const float* q = prm + 17 + cam * 27;
    float tx = bx - q[9], ty = by - q[10], tz = bz - q[11];
    float cx = q[0] * tx + q[1] * ty + q[2] * tz;
    float cy = q[3] * tx + q[4] * ty + q[5] * tz;
    float cz = q[6] * tx + q[7] * ty + q[8] * tz;
    float ix = q[12] * cx + q[13] * cy + q[14] * cz;
    float iy = q[15] * cx + q[16] * cy + q[17] * cz;
    float d = q[18] * cx + q[19] * cy + q[20] * cz;
    float u = ix / (d + 1e-5f), v = iy / (d + 1e-5f);
    float u2 = q[21] * u + q[22] * v + q[25];
    float v2 = q[23] * u + q[24] * v + q[26];
    u2 = (u2 / wimg1 - 0.5f) * 2.f;
    v2 = (v2 / himg1 - 0.5f) * 2.f;
    bool m = d > 1e-5f && u2 > -1.f && u2 < 1.f && v2 > -1.f && v2 < 1.f;
    if (!m) continue;
    float px = (u2 + 1.f) / 2.f * (float)(Wf - 1), py = (v2 + 1.f) / 2.f * (float)(Hf - 1);
    float flx = floorf(px), fly = floorf(py);
    int x0 = (int)flx, y0 = (int)fly;
    float ax = px - flx, ay = py - fly;
    float* base = dimg + (size_t)cam * Hf * Wf * Ci;
    for (int c = lane; c < Ci; c += 64) {
      const float g = dfeat[(size_t)f * dfeat_stride + c];
#pragma unroll
      for (int yy = 0; yy < 2; ++yy)
#pragma unroll
        for (int xx = 0; xx < 2; ++xx) {
          int x = x0 + xx, y = y0 + yy;
          if ((unsigned)x < (unsigned)Wf && (unsigned)y < (unsigned)Hf)
            unsafeAtomicAdd(base + ((size_t)y * Wf + x) * Ci + c, g * ((xx ? ax : 1.f - ax) * (yy ? ay : 1.f - ay)));
        }
    }
  }
}

extern "C" int coocc_fine_sample_img_bwd(const float* dfeat, int dfeat_stride, int ncam, int Ci, int Hf, int Wf,
                                         const float* params, const int64_t* fine_xyz, int64_t nfine, float* dimg,
                                         void* stream) {
  COOCC_CHECK_ARG(dfeat && params && fine_xyz && dimg && ncam > 0 && Ci > 0 && nfine >= 0, "fine_sample_img_bwd: bad args");
  COOCC_CHECK_ARG(dfeat_stride >= Ci && Hf > 0 && Wf > 0, "fine_sample_img_bwd: dfeat_stride < Ci or an empty feature map");
  hipStream_t s = as_stream(stream);
  COOCC_HIP(hipMemsetAsync(dimg, 0, sizeof(float) * (size_t)ncam * Hf * Wf * Ci, s));
  if (nfine == 0) return COOCC_OK;
  hipLaunchKernelGGL(k_fine_sample_img_bwd, dim3(cdiv(nfine * 64, 256)), dim3(256), 0, s, dfeat, dfeat_stride, ncam, Ci, Hf, Wf, params,
                     fine_xyz, (long long)nfine, dimg);
  COOCC_LAUNCH_CHECK("k_fine_sample_img_bwd");
  return COOCC_OK;
}

// nn.GroupNorm over an NHWC image batch (+ReLU) backward: statistics per (image, group) over HW * C/groups values.
// One block per (group, image), like the forward.  x = input before the in-place forward, y = output after it.
__global__ __launch_bounds__(256) void k_groupnorm_nhwc_bwd(const float* __restrict__ x, const float* __restrict__ y,
                                                             const float* __restrict__ dy, int HW, int C, int groups,
                                                             const float* __restrict__ gamma, float eps, int relu,
                                                             float* __restrict__ dx, float* __restrict__ dgamma,
                                                             float* __restrict__ dbeta) {
  __shared__ double s_r[4][4];
  __shared__ float s_stat[4];      // mean, rstd, m1, m2
  __shared__ float s_g[64], s_b[64];
  const int n = blockIdx.y, g = blockIdx.x, cpg = C / groups;
  const size_t off = (size_t)n * HW * C + g * cpg;
  const int total = HW * cpg;
  auto block_sum2 = [&](double a, double b, double& ra, double& rb) {
    for (int m = 32; m > 0; m >>= 1) { a += __shfl_xor(a, m); b += __shfl_xor(b, m); }
    __syncthreads();
    if ((threadIdx.x & 63) == 0) { s_r[threadIdx.x >> 6][0] = a; s_r[threadIdx.x >> 6][1] = b; }
    __syncthreads();
    ra = s_r[0][0] + s_r[1][0] + s_r[2][0] + s_r[3][0];
    rb = s_r[0][1] + s_r[1][1] + s_r[2][1] + s_r[3][1];
  };
  if (threadIdx.x < 64) { s_g[threadIdx.x] = 0.f; s_b[threadIdx.x] = 0.f; }
  double sum = 0, sq = 0;
  for (int i = threadIdx.x; i < total; i += 256) {
    float v = x[off + (size_t)(i / cpg) * C + (i % cpg)];
    sum += v; sq += (double)v * v;
  }
  double a, b;
  block_sum2(sum, sq, a, b);
  const double meand = a / total, vard = b / total - meand * meand;
  const float mean = (float)meand, rstd = (float)(1.0 / sqrt((vard > 0 ? vard : 0) + (double)eps));
  double m1 = 0, m2 = 0;
  for (int i = threadIdx.x; i < total; i += 256) {
    const int c = i % cpg;
    const size_t idx = off + (size_t)(i / cpg) * C + c;
    const float xh = (x[idx] - mean) * rstd;
    float g_ = dy[idx];
    if (relu && !(y[idx] > 0.f)) g_ = 0.f;
    atomicAdd(&s_g[c], g_ * xh);
    atomicAdd(&s_b[c], g_);
    const float dxh = g_ * gamma[g * cpg + c];
    m1 += dxh; m2 += (double)dxh * xh;
  }
  block_sum2(m1, m2, a, b);
  const float fm1 = (float)(a / total), fm2 = (float)(b / total);
  for (int i = threadIdx.x; i < total; i += 256) {
    const int c = i % cpg;
    const size_t idx = off + (size_t)(i / cpg) * C + c;
    const float xh = (x[idx] - mean) * rstd;
    float g_ = dy[idx];
    if (relu && !(y[idx] > 0.f)) g_ = 0.f;
    dx[idx] = rstd * (g_ * gamma[g * cpg + c] - fm1 - xh * fm2);
  }
  __syncthreads();
  if (threadIdx.x < cpg) {
    if (dgamma) unsafeAtomicAdd(dgamma + g * cpg + threadIdx.x, s_g[threadIdx.x]);
    if (dbeta) unsafeAtomicAdd(dbeta + g * cpg + threadIdx.x, s_b[threadIdx.x]);
  }
}

extern "C" int coocc_groupnorm_nhwc_bwd(const float* x, const float* y, const float* dy, int N, int HW, int C, int groups,
                                        const float* gamma, float eps, int relu, float* dx, float* dgamma, float* dbeta,
                                        void* stream) {
  COOCC_CHECK_ARG(x && y && dy && gamma && dx && N > 0 && HW > 0 && C > 0 && groups > 0 && C % groups == 0 && C / groups <= 64,
                  "groupnorm_nhwc_bwd: bad args (channels per group <= 64)");
  hipStream_t s = as_stream(stream);
  if (dgamma) COOCC_HIP(hipMemsetAsync(dgamma, 0, sizeof(float) * C, s));
  if (dbeta) COOCC_HIP(hipMemsetAsync(dbeta, 0, sizeof(float) * C, s));
  hipLaunchKernelGGL(k_groupnorm_nhwc_bwd, dim3(groups, N), dim3(256), 0, s, x, y, dy, HW, C, groups, gamma, eps, relu, dx, dgamma,
                     dbeta);
  COOCC_LAUNCH_CHECK("k_groupnorm_nhwc_bwd");
  return COOCC_OK;
}

// ------------------------------------------------------------------ BatchNorm with batch statistics (training mode)
// Rows [M, C] (channels-last voxels): per-channel mean / biased variance over the M rows, deterministic two-pass column
// reductions (256-row partials, then one pass over the partials in fp64).
__global__ __launch_bounds__(256) void k_bn_part4(const float* __restrict__ x, int stride, int M, int C, double* __restrict__ part) {
  const int q = C >> 2, cq = threadIdx.x % q, r = threadIdx.x / q, R = 256 / q;
  const int m0 = blockIdx.x * COL_ROWS, m1 = min(M, m0 + COL_ROWS);
  double acc[2][4] = {};
  for (int m = m0 + r; m < m1; m += R) {
    const bn_f4 v = *(const bn_f4*)(x + (size_t)m * stride + 4 * cq);
#pragma unroll
    for (int e = 0; e < 4; ++e) { acc[0][e] += v[e]; acc[1][e] += (double)v[e] * v[e]; }
  }
  col_block_reduce<2>(acc, q, r, cq, C, part);
}

__global__ __launch_bounds__(256) void k_bn_final4(const double* __restrict__ part, int nparts, int M, int C, float* __restrict__ mean,
                                                    float* __restrict__ var) {
  double t[2];
  col_final<2>(part, nparts, C, t);
  const int c = blockIdx.x * 4 + (threadIdx.x & 3);
  if ((threadIdx.x >> 2) == 0 && c < C) {
    const double mu = t[0] / M, v = t[1] / M - mu * mu;
    mean[c] = (float)mu;
    var[c] = (float)(v > 0 ? v : 0);
  }
}

__global__ __launch_bounds__(256) void k_bn_part(const float* __restrict__ x, int stride, int M, int C, double* __restrict__ part) {
  const int c = blockIdx.y * 256 + threadIdx.x;
  if (c >= C) return;
  const int m0 = blockIdx.x * 256, m1 = min(M, m0 + 256);
  double s = 0, q = 0;
  for (int m = m0; m < m1; ++m) { const float v = x[(size_t)m * stride + c]; s += v; q += (double)v * v; }
  part[((size_t)blockIdx.x * C + c) * 2] = s;
  part[((size_t)blockIdx.x * C + c) * 2 + 1] = q;
}

__global__ __launch_bounds__(256) void k_bn_final(const double* __restrict__ part, int nparts, int M, int C, float* __restrict__ mean,
                                                   float* __restrict__ var) {
  const int c = blockIdx.x * 256 + threadIdx.x;
  if (c >= C) return;
  double s = 0, q = 0;
  for (int p = 0; p < nparts; ++p) { s += part[((size_t)p * C + c) * 2]; q += part[((size_t)p * C + c) * 2 + 1]; }
  const double mu = s / M, v = q / M - mu * mu;
  mean[c] = (float)mu;
  var[c] = (float)(v > 0 ? v : 0);
}

extern "C" int coocc_bn_stats(const float* x, int stride, int M, int C, float* mean, float* var, void* ws, size_t ws_bytes,
                              void* stream) {
  COOCC_CHECK_ARG(x && mean && var && M > 0 && C > 0 && stride >= C, "bn_stats: bad args");
  const bool fast = col_fast(C) && stride % 4 == 0 && ((uintptr_t)x & 15) == 0;
  const int nparts = fast ? cdiv(M, COL_ROWS) : (M + 255) / 256;
  COOCC_CHECK_ARG(ws && ws_bytes >= sizeof(double) * 2 * (size_t)nparts * C, "bn_stats: workspace too small");
  hipStream_t s = as_stream(stream);
  if (fast) {
    hipLaunchKernelGGL(k_bn_part4, dim3(nparts), dim3(256), 0, s, x, stride, M, C, (double*)ws);
    hipLaunchKernelGGL(k_bn_final4, dim3(cdiv(C, 4)), dim3(256), 0, s, (const double*)ws, nparts, M, C, mean, var);
  } else {
    hipLaunchKernelGGL(k_bn_part, dim3(nparts, cdiv(C, 256)), dim3(256), 0, s, x, stride, M, C, (double*)ws);
    hipLaunchKernelGGL(k_bn_final, dim3(cdiv(C, 256)), dim3(256), 0, s, (const double*)ws, nparts, M, C, mean, var);
  }
  COOCC_LAUNCH_CHECK("bn_stats");
  return COOCC_OK;
}

// y = relu((x - mean) * rstd * gamma + beta (+ res))
__global__ __launch_bounds__(256) void k_bn_apply(const float* __restrict__ x, int M, int C, const float* __restrict__ mean,
                                                   const float* __restrict__ var, const float* __restrict__ gamma,
                                                   const float* __restrict__ beta, float eps, const float* __restrict__ res,
                                                   int relu, float* __restrict__ y) {
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  if (i >= (long long)M * C) return;
  const int c = (int)(i % C);
  float v = (x[i] - mean[c]) * (1.f / sqrtf(var[c] + eps)) * gamma[c] + beta[c];
  if (res) v += res[i];
  y[i] = relu ? fmaxf(v, 0.f) : v;
}

extern "C" int coocc_bn_apply(const float* x, int M, int C, const float* mean, const float* var, const float* gamma,
                              const float* beta, float eps, const float* res, int relu, float* y, void* stream) {
  COOCC_CHECK_ARG(x && mean && var && gamma && beta && y && M > 0 && C > 0, "bn_apply: bad args");
  hipLaunchKernelGGL(k_bn_apply, dim3(cdiv((long long)M * C, 256)), dim3(256), 0, as_stream(stream), x, M, C, mean, var, gamma, beta, eps,
                     res, relu, y);
  COOCC_LAUNCH_CHECK("k_bn_apply");
  return COOCC_OK;
}

// backward: dpre = dy * [y > 0];  dres = dpre;  dgamma = sum dpre * xhat;  dbeta = sum dpre;
//           dx = gamma * rstd * (dpre - dbeta / M - xhat * dgamma / M)
__global__ __launch_bounds__(256) void k_bn_bwd_part(const float* __restrict__ x, const float* __restrict__ y,
                                                      const float* __restrict__ dy, int M, int C, const float* __restrict__ mean,
                                                      const float* __restrict__ var, float eps, int relu, double* __restrict__ part) {
  const int c = blockIdx.y * 256 + threadIdx.x;
  if (c >= C) return;
  const int m0 = blockIdx.x * 256, m1 = min(M, m0 + 256);
  const float mu = mean[c], rstd = 1.f / sqrtf(var[c] + eps);
  double a = 0, b = 0;
  for (int m = m0; m < m1; ++m) {
    const size_t i = (size_t)m * C + c;
    float g = dy[i];
    if (relu && !(y[i] > 0.f)) g = 0.f;
    a += (double)g * ((x[i] - mu) * rstd);
    b += g;
  }
  part[((size_t)blockIdx.x * C + c) * 2] = a;
  part[((size_t)blockIdx.x * C + c) * 2 + 1] = b;
}

__global__ __launch_bounds__(256) void k_bn_bwd_part4(const float* __restrict__ x, const float* __restrict__ y,
                                                       const float* __restrict__ dy, int M, int C, const float* __restrict__ mean,
                                                       const float* __restrict__ var, float eps, int relu, double* __restrict__ part) {
  const int q = C >> 2, cq = threadIdx.x % q, r = threadIdx.x / q, R = 256 / q;
  const int m0 = blockIdx.x * COL_ROWS, m1 = min(M, m0 + COL_ROWS);
  const bn_f4 mu = *(const bn_f4*)(mean + 4 * cq), vr = *(const bn_f4*)(var + 4 * cq);
  float rstd[4];
#pragma unroll
  for (int e = 0; e < 4; ++e) rstd[e] = 1.f / sqrtf(vr[e] + eps);
  double acc[2][4] = {};
  for (int m = m0 + r; m < m1; m += R) {
    const size_t i = (size_t)m * C + 4 * cq;
    const bn_f4 g4 = *(const bn_f4*)(dy + i), x4 = *(const bn_f4*)(x + i);
    bn_f4 y4 = {1.f, 1.f, 1.f, 1.f};
    if (relu) y4 = *(const bn_f4*)(y + i);
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const float g = (relu && !(y4[e] > 0.f)) ? 0.f : g4[e];
      acc[0][e] += (double)g * ((x4[e] - mu[e]) * rstd[e]);
      acc[1][e] += g;
    }
  }
  col_block_reduce<2>(acc, q, r, cq, C, part);
}

__global__ __launch_bounds__(256) void k_bn_bwd_final4(const double* __restrict__ part, int nparts, int C, float* __restrict__ dgamma,
                                                        float* __restrict__ dbeta) {
  double t[2];
  col_final<2>(part, nparts, C, t);
  const int c = blockIdx.x * 4 + (threadIdx.x & 3);
  if ((threadIdx.x >> 2) == 0 && c < C) { dgamma[c] = (float)t[0]; dbeta[c] = (float)t[1]; }
}

__global__ __launch_bounds__(256) void k_bn_bwd_final(const double* __restrict__ part, int nparts, int C, float* __restrict__ dgamma,
                                                       float* __restrict__ dbeta) {
  const int c = blockIdx.x * 256 + threadIdx.x;
  if (c >= C) return;
  double a = 0, b = 0;
  for (int p = 0; p < nparts; ++p) { a += part[((size_t)p * C + c) * 2]; b += part[((size_t)p * C + c) * 2 + 1]; }
  dgamma[c] = (float)a;
  dbeta[c] = (float)b;
}

__global__ __launch_bounds__(256) void k_bn_bwd_dx(const float* __restrict__ x, const float* __restrict__ y, const float* __restrict__ dy,
                                                    int M, int C, const float* __restrict__ mean, const float* __restrict__ var,
                                                    const float* __restrict__ gamma, float eps, int relu,
                                                    const float* __restrict__ dgamma, const float* __restrict__ dbeta,
                                                    float count, float* __restrict__ dx, float* __restrict__ dres) {
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  if (i >= (long long)M * C) return;
  const int c = (int)(i % C);
  const float rstd = 1.f / sqrtf(var[c] + eps);
  float g = dy[i];
  if (relu && !(y[i] > 0.f)) g = 0.f;
  if (dres) dres[i] = g;
  const float xh = (x[i] - mean[c]) * rstd;
  dx[i] = gamma[c] * rstd * (g - dbeta[c] / count - xh * dgamma[c] / count);
}

// The backward in two halves, so that SyncBN can all-reduce the two per-channel sums between them:
// sums: dgamma = sum dy' * xhat, dbeta = sum dy' over THIS rank's rows (dy' = dy * [y > 0] with ReLU);
// dx  : from sums and a row count that may be those of the whole (cross-rank) batch.
extern "C" int coocc_bn_backward_sums(const float* x, const float* y, const float* dy, int M, int C, const float* mean,
                                      const float* var, float eps, int relu, float* dgamma, float* dbeta, void* ws,
                                      size_t ws_bytes, void* stream) {
  COOCC_CHECK_ARG(x && y && dy && mean && var && dgamma && dbeta && M > 0 && C > 0, "bn_backward_sums: bad args");
  const bool fast = col_fast(C) && (((uintptr_t)x | (uintptr_t)y | (uintptr_t)dy | (uintptr_t)mean | (uintptr_t)var) & 15) == 0;
  const int nparts = fast ? cdiv(M, COL_ROWS) : (M + 255) / 256;
  COOCC_CHECK_ARG(ws && ws_bytes >= sizeof(double) * 2 * (size_t)nparts * C, "bn_backward_sums: workspace too small");
  hipStream_t s = as_stream(stream);
  if (fast) {
    hipLaunchKernelGGL(k_bn_bwd_part4, dim3(nparts), dim3(256), 0, s, x, y, dy, M, C, mean, var, eps, relu, (double*)ws);
    hipLaunchKernelGGL(k_bn_bwd_final4, dim3(cdiv(C, 4)), dim3(256), 0, s, (const double*)ws, nparts, C, dgamma, dbeta);
  } else {
    hipLaunchKernelGGL(k_bn_bwd_part, dim3(nparts, cdiv(C, 256)), dim3(256), 0, s, x, y, dy, M, C, mean, var, eps, relu, (double*)ws);
    hipLaunchKernelGGL(k_bn_bwd_final, dim3(cdiv(C, 256)), dim3(256), 0, s, (const double*)ws, nparts, C, dgamma, dbeta);
  }
  COOCC_LAUNCH_CHECK("bn_backward_sums");
  return COOCC_OK;
}

extern "C" int coocc_bn_backward_dx(const float* x, const float* y, const float* dy, int M, int C, const float* mean,
                                    const float* var, const float* gamma, float eps, int relu, const float* sum_dgamma,
                                    const float* sum_dbeta, double count, float* dx, float* dres, void* stream) {
  COOCC_CHECK_ARG(x && y && dy && mean && var && gamma && sum_dgamma && sum_dbeta && dx && M > 0 && C > 0 && count >= 1.0,
                  "bn_backward_dx: bad args");
  hipLaunchKernelGGL(k_bn_bwd_dx, dim3(cdiv((long long)M * C, 256)), dim3(256), 0, as_stream(stream), x, y, dy, M, C, mean, var,
                     gamma, eps, relu, sum_dgamma, sum_dbeta, (float)count, dx, dres);
  COOCC_LAUNCH_CHECK("bn_backward_dx");
  return COOCC_OK;
}

extern "C" int coocc_bn_backward(const float* x, const float* y, const float* dy, int M, int C, const float* mean, const float* var,
                                 const float* gamma, float eps, int relu, float* dx, float* dres, float* dgamma, float* dbeta,
                                 void* ws, size_t ws_bytes, void* stream) {
  COOCC_CHECK_ARG(gamma && dx, "bn_backward: bad args");
  int rc = coocc_bn_backward_sums(x, y, dy, M, C, mean, var, eps, relu, dgamma, dbeta, ws, ws_bytes, stream);
  if (rc != COOCC_OK) return rc;
  return coocc_bn_backward_dx(x, y, dy, M, C, mean, var, gamma, eps, relu, dgamma, dbeta, (double)M, dx, dres, stream);
}
