// SSIM of the rendered colour maps on the device: the second member of the triple save_rendered_img returns
// (P/utils/save_rendered_img.py:22-37, 39-79), skimage.metrics.structural_similarity(pred, target, channel_axis=-1) of scikit-image
// 0.19.3 with no other argument, without copying the [N,H,W,3] maps to the host (103 MB per sample at 6 x 896 x 1600).
//
//   rgbs [N,H,W,3]     what k_upsample_maps writes (interleaved)        x = rgbs[v,:,:,c]
//   gt_img [N,3,H,W]   the reference's img[0][0], NCHW, as it is        y = gt_img[v,c]
//
// Per view and channel: 7 x 7 uniform window, NP = 49; ux, uy, uxx, uyy, uxy the box means of x, y, x^2, y^2, xy; sample covariance
// vx = NP/(NP-1) (uxx - ux^2), vy, vxy likewise; R = data_range (skimage takes 2.0 for a float image), C1 = (0.01 R)^2,
// C2 = (0.03 R)^2; S = (2 ux uy + C1)(2 vxy + C2) / ((ux^2 + uy^2 + C1)(vx + vy + C2)); the channel's value is the mean of S over
// the (H-6)(W-6) pixels whose whole window lies inside the image (skimage crops 3 per side: the filter's boundary mode never
// matters), the view's value the mean of its three channels.  Per view the block holds 8 doubles:
//   [0..2] channel means   [3] (c0 + c1 + c2) / 3 rounded once to fp32   [4] the mean of [3] over the views as save_rendered_img
//   accumulates it (sequential fp32 sum / N; the same value in every row)   [5] (H-6)(W-6)   [6] data_range   [7] 0
//
// k_render_ssim_part: a workgroup of three waves owns a 16 x 64 tile of windows of one view; wave c takes channel c, lane j the
// tile's column j.  The 22 x 72 pixels under the tile (6-pixel halo, rounded up to whole 16-byte groups) are staged in LDS as six
// fp32 planes -- the interleaved rgb is split on the way in -- with 16-byte loads when W % 4 == 0 and the addresses allow, one
// element at a time otherwise.  A lane then walks down its column: per input row the 7-tap row sums of x, y, x^2, y^2, xy in fp64
// (the product of two fp32 values is exact in fp64), kept in a ring of 7 rows in registers; per window row the 7-tap column sum of
// the ring in row order, then S in fp64.  All lanes of a wave read consecutive LDS words of one row: no bank conflicts.  The wave
// adds its lanes' sums with the fixed shuffle tree and writes ONE fp64 partial per (tile, channel); k_render_ssim_final (one wave)
// adds a view's partials in a fixed order (lane l takes partials l, l + 64, ..., then the tree): no floating-point atomics,
// run-to-run bit-equal.
//
// Resources (hipcc 6.x, gfx950): k_render_ssim_part<4> and <1> 118 VGPRs each, k_render_ssim_final 28, no scratch; 38,016 B of LDS per workgroup of 192
// threads -> 4 workgroups (12 waves) per CU.  About 125 fp64 instructions per window and channel (19 of them conversions): the
// pass is bound by the fp64 pipe, not by HBM -- 182 us at 6 x 896 x 1600, 14 % of the 8 TB/s peak at 24 B per pixel
// (profiles/render_ssim_kernels.txt).
#include <math.h>

#include <cmath>

#include "common.h"

constexpr int RS_SLOTS = 8;                       // doubles per view in the block
constexpr int RS_TH = 16, RS_TW = 64;             // windows per tile: rows, columns (one lane per column)
constexpr int RS_WIN = 7;
constexpr int RS_ROWS = RS_TH + RS_WIN - 1;       // staged rows: 22
constexpr int RS_COLS = RS_TW + 8;                // staged columns: the 6-pixel halo rounded up to whole groups of 4 (72)
constexpr int RS_PLANE = RS_ROWS * RS_COLS;
enum { RS_C0 = 0, RS_SSIM = 3, RS_SSIM_MEAN = 4, RS_COUNT = 5, RS_RANGE = 6 };

template <int V>
__device__ __forceinline__ void rs_load(const float* __restrict__ p, float (&v)[V]) {
  if constexpr (V == 4) {
    const float4 t = *reinterpret_cast<const float4*>(p);
    v[0] = t.x; v[1] = t.y; v[2] = t.z; v[3] = t.w;
  } else {
    v[0] = p[0];
  }
}

// V = 4 only when W % 4 == 0 and both maps are 16-byte aligned: every group of 4 floats then lies inside one row and is aligned
template <int V>
__global__ __launch_bounds__(192) COOCC_SCALAR_FP32 void k_render_ssim_part(const float* __restrict__ rgbs,
                                                                            const float* __restrict__ gt_img, int H, int W,
                                                                            double c1, double c2, double* __restrict__ part) {
  __shared__ __attribute__((aligned(16))) float s_x[3 * RS_PLANE];
  __shared__ __attribute__((aligned(16))) float s_y[3 * RS_PLANE];
  const int v = blockIdx.z, x0 = blockIdx.x * RS_TW, y0 = blockIdx.y * RS_TH;
  const size_t HW = (size_t)H * W;
  const float* rgb = rgbs + (size_t)v * HW * 3;
  const float* gt = gt_img + (size_t)v * HW * 3;
  const int cols = min(RS_COLS, W - x0);            // staged columns that exist; x0 < W - 6, so at least 7

  // rgb: per staged row 3 * RS_COLS consecutive floats, element e = pixel e / 3, channel e % 3
  constexpr int XG = 3 * RS_COLS / V;
  for (int i = threadIdx.x; i < RS_ROWS * XG; i += 192) {
    const int r = i / XG, e0 = (i - r * XG) * V, gy = y0 + r;
    float t[V];
#pragma unroll
    for (int k = 0; k < V; ++k) t[k] = 0.f;
    if (gy < H && e0 < 3 * cols) rs_load<V>(rgb + ((size_t)gy * W + x0) * 3 + e0, t);
#pragma unroll
    for (int k = 0; k < V; ++k) {
      const int e = e0 + k, px = e / 3;
      s_x[(e - 3 * px) * RS_PLANE + r * RS_COLS + px] = t[k];
    }
  }
  // gt: per channel and staged row RS_COLS consecutive floats
  constexpr int YG = RS_COLS / V;
  for (int i = threadIdx.x; i < 3 * RS_ROWS * YG; i += 192) {
    const int cr = i / YG, q0 = (i - cr * YG) * V, c = cr / RS_ROWS, r = cr - c * RS_ROWS, gy = y0 + r;
    float t[V];
#pragma unroll
    for (int k = 0; k < V; ++k) t[k] = 0.f;
    if (gy < H && q0 < cols) rs_load<V>(gt + ((size_t)c * H + gy) * W + x0 + q0, t);
#pragma unroll
    for (int k = 0; k < V; ++k) s_y[c * RS_PLANE + r * RS_COLS + q0 + k] = t[k];
  }
  __syncthreads();

  const int c = threadIdx.x >> 6, j = threadIdx.x & 63;
  const float* px = s_x + c * RS_PLANE + j;
  const float* py = s_y + c * RS_PLANE + j;
  const bool col_ok = x0 + j < W - (RS_WIN - 1);
  const int rows_ok = H - (RS_WIN - 1) - y0;         // window rows of this tile that exist (may exceed RS_TH)
  constexpr double INV_NP = 1.0 / 49.0, COV = 49.0 / 48.0;
  double ring[RS_WIN][5];
  double acc = 0.0;
#pragma unroll
  for (int r = 0; r < RS_ROWS; ++r) {
    double s0 = 0, s1 = 0, s2 = 0, s3 = 0, s4 = 0;
#pragma unroll
    for (int t = 0; t < RS_WIN; ++t) {
      const double a = (double)px[r * RS_COLS + t], b = (double)py[r * RS_COLS + t];
      s0 += a; s1 += b;
      s2 = fma(a, a, s2); s3 = fma(b, b, s3); s4 = fma(a, b, s4);   // exact products: the fused form rounds as the separate one
    }
    double* slot = ring[r % RS_WIN];
    slot[0] = s0; slot[1] = s1; slot[2] = s2; slot[3] = s3; slot[4] = s4;
    if (r >= RS_WIN - 1) {
      const int o = r - (RS_WIN - 1);                // window row o covers staged rows o .. o + 6, added in that order
      double u[5];
#pragma unroll
      for (int q = 0; q < 5; ++q) {
        double t = ring[o % RS_WIN][q];
#pragma unroll
        for (int k = 1; k < RS_WIN; ++k) t += ring[(o + k) % RS_WIN][q];
        u[q] = t * INV_NP;
      }
      const double ux = u[0], uy = u[1];
      const double vx = COV * (u[2] - ux * ux), vy = COV * (u[3] - uy * uy), vxy = COV * (u[4] - ux * uy);
      const double num = (2.0 * ux * uy + c1) * (2.0 * vxy + c2);
      const double den = (ux * ux + uy * uy + c1) * (vx + vy + c2);
      const double S = num / den;
      acc += (col_ok && o < rows_ok) ? S : 0.0;
    }
  }
  for (int m = 32; m > 0; m >>= 1) acc += __shfl_xor(acc, m);
  if (j == 0) part[(((size_t)v * gridDim.y + blockIdx.y) * gridDim.x + blockIdx.x) * 3 + c] = acc;
}

// one wave: the views in turn, the partials of a view and channel in a fixed order
__global__ __launch_bounds__(64) void k_render_ssim_final(const double* __restrict__ part, int N, int tiles, double count,
                                                          double data_range, double* __restrict__ block) {
  const int lane = threadIdx.x;
  float total = 0.f;
  for (int v = 0; v < N; ++v) {
    double s[3] = {0, 0, 0};
#pragma unroll 4                                   // the loads of four steps in flight; the additions keep their order
    for (int b = lane; b < tiles; b += 64) {
      const double* p = part + ((size_t)v * tiles + b) * 3;
      s[0] += p[0]; s[1] += p[1]; s[2] += p[2];
    }
    for (int m = 32; m > 0; m >>= 1) {
      s[0] += __shfl_xor(s[0], m); s[1] += __shfl_xor(s[1], m); s[2] += __shfl_xor(s[2], m);
    }
    if (lane == 0) {
      const double m0 = s[0] / count, m1 = s[1] / count, m2 = s[2] / count;
      const float ssim = (float)((m0 + m1 + m2) / 3.0);          // the channel mean, rounded to fp32 once
      total = total + ssim;                                      // ssim_total += ssim (save_rendered_img.py:73)
      double* o = block + (size_t)v * RS_SLOTS;
      o[RS_C0] = m0; o[RS_C0 + 1] = m1; o[RS_C0 + 2] = m2;
      o[RS_SSIM] = (double)ssim;
      o[RS_COUNT] = count; o[RS_RANGE] = data_range;
      o[7] = 0.0;
    }
  }
  if (lane == 0) {
    const double mean = (double)__fdiv_rn(total, (float)N);      // ssim_total / N (:79)
    for (int v = 0; v < N; ++v) block[(size_t)v * RS_SLOTS + RS_SSIM_MEAN] = mean;
  }
}

extern "C" int64_t coocc_render_eval_ssim(const float* rgbs, const float* gt_img, int N, int H, int W, double data_range,
                                          double* block, void* ws, size_t ws_bytes, void* stream) {
  COOCC_CHECK_ARG(N >= 1 && N <= 65535, "render_eval_ssim: 1 <= N <= 65535 views");
  COOCC_CHECK_ARG(H >= RS_WIN && W >= RS_WIN, "render_eval_ssim: H and W must be at least the 7 x 7 window (H = %d, W = %d)", H, W);
  COOCC_CHECK_ARG(std::isfinite(data_range) && data_range > 0.0, "render_eval_ssim: data_range must be positive and finite");
  const long long tx = ((long long)W - (RS_WIN - 1) + RS_TW - 1) / RS_TW, ty = ((long long)H - (RS_WIN - 1) + RS_TH - 1) / RS_TH;
  COOCC_CHECK_ARG(ty <= 65535 && tx * ty <= (1LL << 30), "render_eval_ssim: maps too large (H = %d, W = %d)", H, W);
  const size_t need = sizeof(double) * 3 * (size_t)N * (size_t)(tx * ty);    // does not depend on the addresses
  if (!ws) return (int64_t)need;
  COOCC_CHECK_ARG(rgbs && gt_img && block, "render_eval_ssim: null rgbs, gt_img or block");
  if (ws_bytes < need) return coocc_set_error(COOCC_ENOMEM, "render_eval_ssim: workspace too small (%zu < %zu bytes)", ws_bytes, need);
  const bool vec = W % 4 == 0 && ((uintptr_t)rgbs & 15) == 0 && ((uintptr_t)gt_img & 15) == 0;
  const double c1 = (0.01 * data_range) * (0.01 * data_range), c2 = (0.03 * data_range) * (0.03 * data_range);
  hipStream_t s = as_stream(stream);
  const dim3 grid((unsigned)tx, (unsigned)ty, (unsigned)N);
  if (vec)
    hipLaunchKernelGGL(k_render_ssim_part<4>, grid, dim3(192), 0, s, rgbs, gt_img, H, W, c1, c2, (double*)ws);
  else
    hipLaunchKernelGGL(k_render_ssim_part<1>, grid, dim3(192), 0, s, rgbs, gt_img, H, W, c1, c2, (double*)ws);
  COOCC_LAUNCH_CHECK("k_render_ssim_part");
  hipLaunchKernelGGL(k_render_ssim_final, dim3(1), dim3(64), 0, s, (const double*)ws, N, (int)(tx * ty),
                     (double)(((long long)H - 6) * ((long long)W - 6)), data_range, block);
  COOCC_LAUNCH_CHECK("k_render_ssim_final");
  return COOCC_OK;
}
