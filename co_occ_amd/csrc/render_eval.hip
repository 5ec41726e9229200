// On-device evaluation of the rendered maps: the test_rendering tail of COOCC_Ray.simple_test (P/coocc/detectors/coocc_ray.py:626-637),
// compute_psnr (P/utils/save_rendered_img.py:10-20) and the depth error of save_rendered_img (:39-79), without copying the
// [N,H,W,4] maps to the host (138 MB per sample at 6 x 896 x 1600).
//
//   rgbs [N,H,W,3], depths [N,H,W]    what k_upsample_maps writes
//   gt_img [N,3,H,W]                  the reference's img[0][0], NCHW, as it is (upstream does not denormalise it either)
//   gt_depth [N,H,W]                  optional
//
// coocc_render_eval_stats: one pass over the maps.  Every workgroup writes fp64 partial sums (and the depth extrema) of its pixel
// slice of ONE view into the workspace; the last step adds the partials of a view in a fixed order (lane l takes partials l, l + 64,
// ..., then a fixed shuffle tree): no floating-point atomics, run-to-run bit-equal.  The squared differences are formed in fp64 from
// the fp32 inputs, so the PSNR is the float64 value rounded once to fp32.  Per view the stats block holds 8 doubles:
//   [0] sq_rgb = sum (rgb - gt)^2 over H*W*3      [1] dmin   [2] dmax  (of the depth map; exact fp32 values)
//   [3] sq_depth = sum (depth - gt_depth)^2 and [4] n_valid, over the pixels with gt_depth > 0
//   [5] psnr = -10 ln(sq_rgb / (3HW)) / ln 10, rounded to fp32 (+inf for a zero error, as upstream; NaN without rgbs)
//   [6] mean of [5] over the views as upstream accumulates it (sequential fp32 sum / N; the same value in every row)   [7] 0
// coocc_render_panels: the [rgb | gt | depth_] uint8 panel of coocc_ray.py:629-633 per view; dmin / dmax come from the stats block on
// the device.  The fp32 operations are spelled in upstream's order with IEEE division and no contraction (build.py FILE_FLAGS:
// -ffp-contract=off), so the bytes are the CPU's.
//
// Both kernels are HBM-bound (28 B read per pixel; the panels write 9 B more): a thread takes 4 consecutive pixels -- three 16-byte
// reads of the interleaved rgb, one per gt plane, one per depth map -- when the sizes and addresses allow, one pixel otherwise.
#include <math.h>

#include "common.h"

constexpr int RE_SLOTS = 8;          // doubles per view in the stats block
constexpr int RE_PART = 5;           // doubles per workgroup partial: sq_rgb, sq_depth, n_valid, dmin, dmax
constexpr int RE_MAX_BPV = 256;      // workgroups per view at most (6 views: 1536 workgroups, 6 per CU)
enum { RE_SQ_RGB = 0, RE_DMIN = 1, RE_DMAX = 2, RE_SQ_DEPTH = 3, RE_NVALID = 4, RE_PSNR = 5, RE_PSNR_MEAN = 6 };

template <int V>
__device__ __forceinline__ void re_load(const float* __restrict__ p, float (&v)[V]) {
  if constexpr (V == 4) {
    const float4 t = *reinterpret_cast<const float4*>(p);
    v[0] = t.x; v[1] = t.y; v[2] = t.z; v[3] = t.w;
  } else {
#pragma unroll
    for (int i = 0; i < V; ++i) v[i] = p[i];
  }
}

static int re_blocks_per_view(long long groups) { return (int)std::max<long long>(1, std::min<long long>(RE_MAX_BPV, (groups + 1023) / 1024)); }

template <int V>
__global__ __launch_bounds__(256) COOCC_SCALAR_FP32 void k_render_eval_part(const float* __restrict__ rgbs,
                                                                            const float* __restrict__ depths,
                                                                            const float* __restrict__ gt_img,
                                                                            const float* __restrict__ gt_depth, long long HW,
                                                                            double* __restrict__ part) {
  __shared__ double s_p[4][RE_PART];
  const int v = blockIdx.y;
  const float* dp = depths + (size_t)v * HW;
  const float* gd = gt_depth ? gt_depth + (size_t)v * HW : nullptr;
  const float* rgb = rgbs ? rgbs + (size_t)v * HW * 3 : nullptr;
  const float* gt = rgbs ? gt_img + (size_t)v * HW * 3 : nullptr;
  double sc = 0, sd = 0, sn = 0;
  float mn = INFINITY, mx = -INFINITY;
  const long long groups = HW / V;                   // the launcher picks V = 4 only when HW % 4 == 0
  for (long long g = (long long)blockIdx.x * 256 + threadIdx.x; g < groups; g += (long long)gridDim.x * 256) {
    const long long p = g * V;
    float d[V];
    re_load<V>(dp + p, d);
#pragma unroll
    for (int i = 0; i < V; ++i) { mn = fminf(mn, d[i]); mx = fmaxf(mx, d[i]); }
    if (gd) {
      float t[V];
      re_load<V>(gd + p, t);
#pragma unroll
      for (int i = 0; i < V; ++i)
        if (t[i] > 0.f) {
          const double e = (double)d[i] - (double)t[i];
          sd += e * e;
          sn += 1.0;
        }
    }
    if (rgb) {
      float r[3][V], q[3][V];                        // r: 3V interleaved floats (pixel-major); q[c]: plane c
#pragma unroll
      for (int k = 0; k < 3; ++k) {
        re_load<V>(rgb + p * 3 + k * V, r[k]);
        re_load<V>(gt + (size_t)k * HW + p, q[k]);
      }
#pragma unroll
      for (int j = 0; j < 3 * V; ++j) {              // element j of the group = pixel j / 3, channel j % 3
        const double e = (double)r[j / V][j % V] - (double)q[j % 3][j / 3];
        sc += e * e;
      }
    }
  }
  for (int m = 32; m > 0; m >>= 1) {
    sc += __shfl_xor(sc, m); sd += __shfl_xor(sd, m); sn += __shfl_xor(sn, m);
    mn = fminf(mn, __shfl_xor(mn, m)); mx = fmaxf(mx, __shfl_xor(mx, m));
  }
  if ((threadIdx.x & 63) == 0) {
    double* s = s_p[threadIdx.x >> 6];
    s[0] = sc; s[1] = sd; s[2] = sn; s[3] = (double)mn; s[4] = (double)mx;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    double* o = part + ((size_t)v * gridDim.x + blockIdx.x) * RE_PART;
    o[0] = s_p[0][0] + s_p[1][0] + s_p[2][0] + s_p[3][0];
    o[1] = s_p[0][1] + s_p[1][1] + s_p[2][1] + s_p[3][1];
    o[2] = s_p[0][2] + s_p[1][2] + s_p[2][2] + s_p[3][2];
    o[3] = fmin(fmin(s_p[0][3], s_p[1][3]), fmin(s_p[2][3], s_p[3][3]));
    o[4] = fmax(fmax(s_p[0][4], s_p[1][4]), fmax(s_p[2][4], s_p[3][4]));
  }
}

// one wave: the views in turn, the partials of a view in a fixed order
__global__ __launch_bounds__(64) void k_render_eval_final(const double* __restrict__ part, int N, int bpv, long long HW, int has_rgb,
                                                          double* __restrict__ block) {
  const int lane = threadIdx.x;
  float psum = 0.f;
  for (int v = 0; v < N; ++v) {
    double sc = 0, sd = 0, sn = 0, mn = INFINITY, mx = -INFINITY;
    for (int b = lane; b < bpv; b += 64) {
      const double* p = part + ((size_t)v * bpv + b) * RE_PART;
      sc += p[0]; sd += p[1]; sn += p[2];
      mn = fmin(mn, p[3]); mx = fmax(mx, p[4]);
    }
    for (int m = 32; m > 0; m >>= 1) {
      sc += __shfl_xor(sc, m); sd += __shfl_xor(sd, m); sn += __shfl_xor(sn, m);
      mn = fmin(mn, __shfl_xor(mn, m)); mx = fmax(mx, __shfl_xor(mx, m));
    }
    if (lane == 0) {
      // compute_psnr_from_mse (save_rendered_img.py:10-11) on the fp64 mean, rounded to fp32 once
      const float psnr = has_rgb ? (float)(-10.0 * log(sc / (3.0 * (double)HW)) / log(10.0)) : NAN;
      psum = psum + psnr;                            // psnr_total += psnr (coocc_ray.py:635)
      double* o = block + (size_t)v * RE_SLOTS;
      o[RE_SQ_RGB] = sc; o[RE_DMIN] = mn; o[RE_DMAX] = mx; o[RE_SQ_DEPTH] = sd; o[RE_NVALID] = sn;
      o[RE_PSNR] = (double)psnr;
      o[7] = 0.0;
    }
  }
  if (lane == 0) {
    const double mean = (double)__fdiv_rn(psum, (float)N);   // psnr_total / rgbs.shape[0] (:637)
    for (int v = 0; v < N; ++v) block[(size_t)v * RE_SLOTS + RE_PSNR_MEAN] = mean;
  }
}

// np.uint8(x.clip(0, 1) * 255.0) (coocc_ray.py:632-633): clip, one fp32 multiply, truncation
__device__ __forceinline__ unsigned re_u8(float x) { return (unsigned)(fminf(fmaxf(x, 0.f), 1.f) * 255.0f); }

template <int V>
__device__ __forceinline__ void re_store(uint8_t* __restrict__ o, const unsigned (&b)[3 * V]) {
  if constexpr (V == 4) {                            // 12 bytes at a 4-byte aligned address
    uint32_t* w = reinterpret_cast<uint32_t*>(o);
#pragma unroll
    for (int k = 0; k < 3; ++k) w[k] = b[4 * k] | (b[4 * k + 1] << 8) | (b[4 * k + 2] << 16) | (b[4 * k + 3] << 24);
  } else {
#pragma unroll
    for (int j = 0; j < 3 * V; ++j) o[j] = (uint8_t)b[j];
  }
}

template <int V>
__global__ __launch_bounds__(256) COOCC_SCALAR_FP32 void k_render_panels(const float* __restrict__ rgbs,
                                                                         const float* __restrict__ depths,
                                                                         const float* __restrict__ gt_img,
                                                                         const double* __restrict__ block, int H, int W,
                                                                         uint8_t* __restrict__ panels) {
  const int v = blockIdx.y;
  const long long HW = (long long)H * W;
  const float* dp = depths + (size_t)v * HW;
  const float* rgb = rgbs + (size_t)v * HW * 3;
  const float* gt = gt_img + (size_t)v * HW * 3;
  uint8_t* out = panels + (size_t)v * HW * 9;
  const float dmin = (float)block[(size_t)v * RE_SLOTS + RE_DMIN], dmax = (float)block[(size_t)v * RE_SLOTS + RE_DMAX];
  const float den = (dmax - dmin) + 1e-8f;           // depths[v].max() - depths[v].min() + 1e-8 (:631)
  const long long groups = HW / V;                   // V = 4 only when W % 4 == 0: a group stays inside one row
  for (long long g = (long long)blockIdx.x * 256 + threadIdx.x; g < groups; g += (long long)gridDim.x * 256) {
    const long long p = g * V;
    const long long y = p / W, x = p - y * W;
    float d[V], r[3][V], q[3][V];
    re_load<V>(dp + p, d);
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      re_load<V>(rgb + p * 3 + k * V, r[k]);
      re_load<V>(gt + (size_t)k * HW + p, q[k]);
    }
    unsigned b0[3 * V], b1[3 * V], b2[3 * V];
#pragma unroll
    for (int j = 0; j < 3 * V; ++j) {
      b0[j] = re_u8(r[j / V][j % V]);
      b1[j] = re_u8(q[j % 3][j / 3]);                // gt_img[v].permute(1, 2, 0)
    }
#pragma unroll
    for (int i = 0; i < V; ++i) {
      const unsigned u = re_u8(__fdiv_rn(d[i] - dmin, den));
      b2[3 * i] = b2[3 * i + 1] = b2[3 * i + 2] = u; // .unsqueeze(-1).repeat(1, 1, 3)
    }
    uint8_t* row = out + (size_t)y * W * 9 + (size_t)x * 3;   // torch.cat([rgb, gt, depth_], dim=1): [H, 3W, 3]
    re_store<V>(row, b0);
    re_store<V>(row + (size_t)W * 3, b1);
    re_store<V>(row + (size_t)W * 6, b2);
  }
}

static inline bool re_aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }

extern "C" int64_t coocc_render_eval_stats(const float* rgbs, const float* depths, const float* gt_img, const float* gt_depth, int N,
                                           int H, int W, double* block, void* ws, size_t ws_bytes, void* stream) {
  COOCC_CHECK_ARG(N >= 1 && N <= 65535, "render_eval_stats: 1 <= N <= 65535 views");
  COOCC_CHECK_ARG(H > 0 && W > 0, "render_eval_stats: empty maps (H * W == 0)");
  const long long HW = (long long)H * W;
  const bool vec = HW % 4 == 0 && re_aligned16(rgbs) && re_aligned16(depths) && re_aligned16(gt_img) && re_aligned16(gt_depth);
  // the workspace size does not depend on the addresses: sized for the one-pixel form, which has the most groups
  const int bpv_max = re_blocks_per_view(HW);
  const size_t need = sizeof(double) * RE_PART * (size_t)N * bpv_max;
  if (!ws) return (int64_t)need;
  COOCC_CHECK_ARG(depths && block, "render_eval_stats: null depths or stats block");
  COOCC_CHECK_ARG((rgbs != nullptr) == (gt_img != nullptr), "render_eval_stats: rgbs and gt_img come together (both or neither)");
  if (ws_bytes < need) return coocc_set_error(COOCC_ENOMEM, "render_eval_stats: workspace too small (%zu < %zu bytes)", ws_bytes, need);
  hipStream_t s = as_stream(stream);
  const int bpv = re_blocks_per_view(vec ? HW / 4 : HW);
  if (vec)
    hipLaunchKernelGGL(k_render_eval_part<4>, dim3(bpv, N), dim3(256), 0, s, rgbs, depths, gt_img, gt_depth, HW, (double*)ws);
  else
    hipLaunchKernelGGL(k_render_eval_part<1>, dim3(bpv, N), dim3(256), 0, s, rgbs, depths, gt_img, gt_depth, HW, (double*)ws);
  COOCC_LAUNCH_CHECK("k_render_eval_part");
  hipLaunchKernelGGL(k_render_eval_final, dim3(1), dim3(64), 0, s, (const double*)ws, N, bpv, HW, rgbs ? 1 : 0, block);
  COOCC_LAUNCH_CHECK("k_render_eval_final");
  return COOCC_OK;
}

extern "C" int coocc_render_panels(const float* rgbs, const float* depths, const float* gt_img, const double* block, int N, int H,
                                   int W, uint8_t* panels, void* stream) {
  COOCC_CHECK_ARG(N >= 1 && N <= 65535, "render_panels: 1 <= N <= 65535 views");
  COOCC_CHECK_ARG(H > 0 && W > 0, "render_panels: empty maps (H * W == 0)");
  COOCC_CHECK_ARG(block, "render_panels: the stats block of coocc_render_eval_stats is required (depth_ needs dmin / dmax)");
  COOCC_CHECK_ARG(rgbs && depths && gt_img && panels, "render_panels: null rgbs, depths, gt_img or panels");
  const long long HW = (long long)H * W;
  const bool vec = W % 4 == 0 && re_aligned16(rgbs) && re_aligned16(depths) && re_aligned16(gt_img) && ((uintptr_t)panels & 3) == 0;
  const int bpv = re_blocks_per_view(vec ? HW / 4 : HW);
  hipStream_t s = as_stream(stream);
  if (vec)
    hipLaunchKernelGGL(k_render_panels<4>, dim3(bpv, N), dim3(256), 0, s, rgbs, depths, gt_img, block, H, W, panels);
  else
    hipLaunchKernelGGL(k_render_panels<1>, dim3(bpv, N), dim3(256), 0, s, rgbs, depths, gt_img, block, H, W, panels);
  COOCC_LAUNCH_CHECK("k_render_panels");
  return COOCC_OK;
}
