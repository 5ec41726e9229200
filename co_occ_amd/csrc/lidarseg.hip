// LiDAR-segmentation point predictions (points_occ): OccHead.forward_lidarseg (P/coocc/dense_heads/occ_head.py:339-383),
// the label step of COOCC_Ray.simple_test (P/coocc/detectors/coocc_ray.py:556-560) and simple_evaluation_semantic (:693-700,
// fast_hist_crop of P/utils/metric_util.py:8-23) in one pass over the points, without the host round trip.
//
// Per point, one thread:
//   grid coordinate  ((p - min) / (max - min)) * 2 - 1                                  fp32, the reference's order
//   trilinear sample F.grid_sample(mode='bilinear', align_corners=True, padding border | zeros) of the logits [C,X,Y,Z]
//                    at (x, y, z) -> (X, Y, Z): the reference permutes the point to (z, y, x) = grid (W, H, D) order, and
//                    this file restates ATen's CPU grid_sampler_3d (corner order tnw..bse, weights as products of distances
//                    (W)*(H)*(D), out-of-bounds corners skipped) with no FMA contraction (build.py FILE_FLAGS: -ffp-contract=off)
//                    so the sampled logits are the CPU's bits.  Out-of-range points are kept (the reference computes
//                    out_of_range_mask and never uses it).
//   mode 0 (eval)    softmax over C; label = first maximum of the probabilities over classes 1..C-1, + 1   (coocc_ray.py:557)
//   mode 1 (train)   label = first maximum of the raw sampled logits over classes 1..C-1, + 1              (occ_head.py:366)
//   histogram        fast_hist_crop(pred, trunc(target), arange(16)): [label-1][pred-1] over labels 1..16 (C == 17), counts in
//                    LDS per workgroup, flushed with 64-bit atomics as k_eval_semantic does.
#include "common.h"

constexpr int LSEG_MAX_C = 32;
constexpr int LSEG_NB = 16;          // fast_hist_crop(..., unique_label = arange(16)): classes 1..16

// grid_sampler_compute_source_index, align_corners=True: ((g + 1) / 2) * (size - 1), clipped to [0, size-1] for border
__device__ __forceinline__ float lseg_source_index(float g, int size, int border) {
  float c = ((g + 1.f) / 2.f) * (float)(size - 1);
  if (border) c = fminf((float)(size - 1), fmaxf(c, 0.f));
  return c;
}

template <int CM>
__global__ __launch_bounds__(256) void k_lidarseg_points(const float* __restrict__ logits, long long sc, long long sx, long long sy,
                                                         long long sz, int C, int X, int Y, int Z, const float* __restrict__ points,
                                                         int n, long long pstride, int label_col, float mn0, float mn1, float mn2,
                                                         float rg0, float rg1, float rg2, int border, int train,
                                                         float* __restrict__ probs, int64_t* __restrict__ labels,
                                                         unsigned long long* __restrict__ hist) {
  __shared__ unsigned int s_hist[LSEG_NB * LSEG_NB];
  if (hist) {
    for (int b = threadIdx.x; b < LSEG_NB * LSEG_NB; b += 256) s_hist[b] = 0;
    __syncthreads();
  }
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i < n) {
    const float* pt = points + (long long)i * pstride;
    // normalise in the reference's order, then grid_sample's (W, H, D) = point (z, y, x)
    const float gx = __fdiv_rn(pt[0] - mn0, rg0) * 2.f - 1.f;
    const float gy = __fdiv_rn(pt[1] - mn1, rg1) * 2.f - 1.f;
    const float gz = __fdiv_rn(pt[2] - mn2, rg2) * 2.f - 1.f;
    const float iw = lseg_source_index(gz, Z, border);      // ix of ATen (innermost dim W = Z)
    const float ih = lseg_source_index(gy, Y, border);      // iy (H = Y)
    const float id = lseg_source_index(gx, X, border);      // iz (D = X)
    const float fw = floorf(iw), fh = floorf(ih), fd = floorf(id);
    // distances to the floor / ceil corners (ATen: (ix_bse - ix), (ix - ix_bsw), ... as int64 -> float); all are finite here
    // whenever any corner is in bounds, which is the only case their products are used
    const float w1 = iw - fw, w0 = (fw + 1.f) - iw;
    const float h1 = ih - fh, h0 = (fh + 1.f) - ih;
    const float d1 = id - fd, d0 = (fd + 1.f) - id;
    // in-bounds test per axis and corner in float (no float -> int conversion of a far-out coordinate)
    const bool vw0 = fw >= 0.f && fw <= (float)(Z - 1), vw1 = fw + 1.f >= 0.f && fw + 1.f <= (float)(Z - 1);
    const bool vh0 = fh >= 0.f && fh <= (float)(Y - 1), vh1 = fh + 1.f >= 0.f && fh + 1.f <= (float)(Y - 1);
    const bool vd0 = fd >= 0.f && fd <= (float)(X - 1), vd1 = fd + 1.f >= 0.f && fd + 1.f <= (float)(X - 1);
    const int cw = vw0 ? (int)fw : 0, ch = vh0 ? (int)fh : 0, cd = vd0 ? (int)fd : 0;
    const int cw1 = vw1 ? (int)fw + 1 : 0, ch1 = vh1 ? (int)fh + 1 : 0, cd1 = vd1 ? (int)fd + 1 : 0;
    // ATen's eight corners: t/b = D (x) floor/ceil, n/s = H (y), w/e = W (z)
    const float wt[8] = {w0 * h0 * d0, w1 * h0 * d0, w0 * h1 * d0, w1 * h1 * d0,   // tnw tne tsw tse
                         w0 * h0 * d1, w1 * h0 * d1, w0 * h1 * d1, w1 * h1 * d1};  // bnw bne bsw bse
    const bool ok[8] = {vd0 && vh0 && vw0, vd0 && vh0 && vw1, vd0 && vh1 && vw0, vd0 && vh1 && vw1,
                        vd1 && vh0 && vw0, vd1 && vh0 && vw1, vd1 && vh1 && vw0, vd1 && vh1 && vw1};
    const long long off[8] = {cd * sx + ch * sy + cw * sz,  cd * sx + ch * sy + cw1 * sz,  cd * sx + ch1 * sy + cw * sz,
                              cd * sx + ch1 * sy + cw1 * sz, cd1 * sx + ch * sy + cw * sz, cd1 * sx + ch * sy + cw1 * sz,
                              cd1 * sx + ch1 * sy + cw * sz, cd1 * sx + ch1 * sy + cw1 * sz};
    float v[CM];
#pragma unroll
    for (int c = 0; c < CM; ++c) {
      if (c < C) {
        const float* p = logits + c * sc;
        float acc = 0.f;
#pragma unroll
        for (int k = 0; k < 8; ++k)
          if (ok[k]) acc = acc + p[off[k]] * wt[k];
        v[c] = acc;
      }
    }
    int arg = 1;
    if (!train) {
      // torch.softmax (lastdim): exp(x - max), sum, times 1 / sum
      float mx = v[0];
#pragma unroll
      for (int c = 1; c < CM; ++c)
        if (c < C) mx = fmaxf(mx, v[c]);
      float sum = 0.f;
#pragma unroll
      for (int c = 0; c < CM; ++c)
        if (c < C) {
          v[c] = expf(v[c] - mx);
          sum = sum + v[c];
        }
      const float inv = __fdiv_rn(1.f, sum);
#pragma unroll
      for (int c = 0; c < CM; ++c)
        if (c < C) v[c] = v[c] * inv;
      if (probs) {
        float* po = probs + (long long)i * C;
#pragma unroll
        for (int c = 0; c < CM; ++c)
          if (c < C) po[c] = v[c];
      }
    }
    float best = v[1];
#pragma unroll
    for (int c = 2; c < CM; ++c)
      if (c < C && v[c] > best) { best = v[c]; arg = c; }
    if (labels) labels[i] = arg;
    if (hist && arg <= LSEG_NB) {
      // int(trunc(t)) in 1..16  <=>  1 <= t < 17 (NaN fails both)
      const float t = pt[label_col];
      if (t >= 1.f && t < (float)(LSEG_NB + 1)) atomicAdd(&s_hist[((int)t - 1) * LSEG_NB + arg - 1], 1u);
    }
  }
  if (hist) {
    __syncthreads();
    for (int b = threadIdx.x; b < LSEG_NB * LSEG_NB; b += 256) {
      const unsigned int c = s_hist[b];
      if (c) atomicAdd(&hist[b], (unsigned long long)c);
    }
  }
}

extern "C" int coocc_lidarseg_points(const float* logits, int64_t stride_c, int64_t stride_x, int64_t stride_y, int64_t stride_z,
                                     int C, int X, int Y, int Z, const float* points, int64_t n, int64_t point_stride,
                                     int point_cols, int label_col, const float* range_host, int padding_mode, int mode,
                                     float* probs, int64_t* labels, int accumulate, int64_t* hist, void* stream) {
  COOCC_CHECK_ARG(logits && range_host && C >= 2 && C <= LSEG_MAX_C && X > 0 && Y > 0 && Z > 0,
                  "lidarseg_points: bad args (logits, range, 2 <= C <= 32, grid)");
  COOCC_CHECK_ARG(n >= 0 && n < (1ll << 31) && (n == 0 || points) && point_cols >= 3 && point_stride >= point_cols,
                  "lidarseg_points: bad point table (n, points, point_cols >= 3, point_stride >= point_cols)");
  COOCC_CHECK_ARG(stride_c >= 0 && stride_x >= 0 && stride_y >= 0 && stride_z >= 0, "lidarseg_points: negative logits stride");
  COOCC_CHECK_ARG(padding_mode == 0 || padding_mode == 1, "lidarseg_points: padding_mode 0 (zeros) or 1 (border)");
  COOCC_CHECK_ARG(mode == 0 || mode == 1, "lidarseg_points: mode 0 (eval) or 1 (train)");
  COOCC_CHECK_ARG(!probs || mode == 0, "lidarseg_points: probabilities are an eval-mode output");
  COOCC_CHECK_ARG(!hist || (C == LSEG_NB + 1 && label_col >= 0 && label_col < point_cols),
                  "lidarseg_points: the 16x16 histogram needs C == 17 and 0 <= label_col < point_cols");
  const float mn0 = range_host[0], mn1 = range_host[1], mn2 = range_host[2];
  const float rg0 = range_host[3] - mn0, rg1 = range_host[4] - mn1, rg2 = range_host[5] - mn2;
  hipStream_t s = as_stream(stream);
  if (hist && !accumulate) COOCC_HIP(hipMemsetAsync(hist, 0, sizeof(int64_t) * LSEG_NB * LSEG_NB, s));
  if (n == 0) return COOCC_OK;
#define LSEG_LAUNCH(CM)                                                                                                        \
  hipLaunchKernelGGL(k_lidarseg_points<CM>, dim3(cdiv(n, 256)), dim3(256), 0, s, logits, stride_c, stride_x, stride_y, stride_z, \
                     C, X, Y, Z, points, (int)n, point_stride, label_col, mn0, mn1, mn2, rg0, rg1, rg2, padding_mode, mode,  \
                     probs, labels, (unsigned long long*)hist)
  if (C <= LSEG_NB + 1)
    LSEG_LAUNCH(LSEG_NB + 1);
  else
    LSEG_LAUNCH(LSEG_MAX_C);
#undef LSEG_LAUNCH
  COOCC_LAUNCH_CHECK("k_lidarseg_points");
  return COOCC_OK;
}
