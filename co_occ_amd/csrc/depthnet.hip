// The kernels DepthNet (co_occ_amd/depth_net.py; ViewTransformerLSSBEVDepth.py:351-549) adds to the engine.  Everything else of
// the module is a convolution or a Linear the GEMMs of conv3d.hip / gemm_h2.hip already run.  Feature maps are channels-last rows
// [BN*H*W][C], row (b*H + y)*W + x, one camera after the other.
//
//   k_nbr_table2d     the [9][BN*H*W] row table of a DILATED 3x3 convolution (ASPP's branches): tap t = 3i + j reads row
//                     (y + (i-1) d, x + (j-1) d) of the SAME camera, -1 in the padding.  The row-table GEMM does the rest.
//   k_dcn_cols        the deformable sampler of DCNv1 (mmcv 1.4.0 DeformConv2dPack, 3x3, padding 1, deform_groups 1): one wave per
//                     pixel, the nine sample positions / corner weights / validity are wave-uniform, lanes run across channel quads so
//                     each of the four corner rows is one coalesced read.  Writes group g's column matrix [rows][9 * C/G] (k = tap *
//                     C/G + channel) contiguously: the K-slab of that group's GEMM.
//   k_se_gate2        both SE-gated copies of x in one pass: out_a = x * sigmoid(ga[camera]), out_b = x * sigmoid(gb[camera]).
//   k_cam_part4 / k_cam_final4   per-camera channel means (colreduce.h: fp64, fixed order) -- ASPP's pooled branch.
//   k_cam_bias_relu   y = relu(y + bias[camera]) in place: the pooled branch's contribution to ASPP's 1x1 is a per-camera bias.
//
// Every kernel here multiplies a vector by a scalar or by another vector's element, the source form of the packed-fp32 op_sel
// hazard (common.h): all of them are COOCC_SCALAR_FP32.  They are HBM-bound.
#include "colreduce.h"

typedef float f32x4 __attribute__((ext_vector_type(4)));

// ------------------------------------------------------------------ dilated 3x3 row table
__global__ __launch_bounds__(256) void k_nbr_table2d(int BN, int H, int W, int dil, int32_t* __restrict__ table) {
  const long long M = (long long)BN * H * W;
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  if (i >= 9 * M) return;
  const int t = (int)(i / M);
  const int m = (int)(i % M);
  const int x = m % W, y = (m / W) % H, b = m / (W * H);
  const int yy = y + (t / 3 - 1) * dil, xx = x + (t % 3 - 1) * dil;
  const bool in = (unsigned)yy < (unsigned)H && (unsigned)xx < (unsigned)W;
  table[i] = in ? (b * H + yy) * W + xx : -1;
}

extern "C" int coocc_nbr_table2d(int BN, int H, int W, int dil, int32_t* table, void* stream) {
  COOCC_CHECK_ARG(table && BN > 0 && H > 0 && W > 0 && dil > 0, "nbr_table2d: bad args");
  const long long M = (long long)BN * H * W;
  COOCC_CHECK_ARG(9 * M < (1ll << 31), "nbr_table2d: map too large (row indices are 32-bit)");
  hipLaunchKernelGGL(k_nbr_table2d, dim3(cdiv(9 * M, 256)), dim3(256), 0, as_stream(stream), BN, H, W, dil, table);
  COOCC_LAUNCH_CHECK("k_nbr_table2d");
  return COOCC_OK;
}

// ------------------------------------------------------------------ deformable sampler
// Sample position of tap (i, j) at pixel (y, x): (y - 1 + i + off[2t], x - 1 + j + off[2t + 1]); bilinear, zeros outside: the value is
// 0 when the position is <= -1 or >= H (W), and a corner outside the image contributes 0 (mmcv's deformable_im2col_bilinear).  A NaN
// offset fails every comparison and gives 0 as well; no index is formed before the position has passed the range test.
COOCC_SCALAR_FP32 __global__ __launch_bounds__(256) void k_dcn_cols(const float* __restrict__ x, int x_stride,
                                                                     const float* __restrict__ off, int off_stride, int H, int W, int C,
                                                                     int Cg, int m0, int n, float* __restrict__ cols) {
  const int r = __builtin_amdgcn_readfirstlane(blockIdx.x * 4 + (threadIdx.x >> 6)), lane = threadIdx.x & 63;
  if (r >= n) return;
  const int m = m0 + r;
  const int px = m % W, py = (m / W) % H, b = m / (W * H);
  const float* o = off + (size_t)m * off_stride;
  const int K = 9 * Cg;
  const size_t gstride = (size_t)n * K;
  const int quads = C >> 2;
  for (int t = 0; t < 9; ++t) {
    const float sy = (float)(py - 1 + t / 3) + o[2 * t], sx = (float)(px - 1 + t % 3) + o[2 * t + 1];
    const bool inside = sy > -1.f && sy < (float)H && sx > -1.f && sx < (float)W;
    float w00 = 0.f, w01 = 0.f, w10 = 0.f, w11 = 0.f;
    const float *p00 = x, *p01 = x, *p10 = x, *p11 = x;
    bool v00 = false, v01 = false, v10 = false, v11 = false;
    if (inside) {
      const float fy = floorf(sy), fx = floorf(sx);
      const int y0 = (int)fy, x0 = (int)fx;              // y0 in [-1, H-1], x0 in [-1, W-1]
      const float ly = sy - fy, lx = sx - fx, hy = 1.f - ly, hx = 1.f - lx;
      const bool ylo = y0 >= 0, yhi = y0 + 1 <= H - 1, xlo = x0 >= 0, xhi = x0 + 1 <= W - 1;
      v00 = ylo && xlo; v01 = ylo && xhi; v10 = yhi && xlo; v11 = yhi && xhi;
      w00 = hy * hx; w01 = hy * lx; w10 = ly * hx; w11 = ly * lx;
      const size_t base = (size_t)b * H * W;
      if (v00) p00 = x + (base + (size_t)y0 * W + x0) * x_stride;
      if (v01) p01 = x + (base + (size_t)y0 * W + x0 + 1) * x_stride;
      if (v10) p10 = x + (base + (size_t)(y0 + 1) * W + x0) * x_stride;
      if (v11) p11 = x + (base + (size_t)(y0 + 1) * W + x0 + 1) * x_stride;
    }
    for (int q = lane; q < quads; q += 64) {
      const int c = q << 2;
      f32x4 acc = {0.f, 0.f, 0.f, 0.f};
      if (v00) acc = acc + *(const f32x4*)(p00 + c) * w00;
      if (v01) acc = acc + *(const f32x4*)(p01 + c) * w01;
      if (v10) acc = acc + *(const f32x4*)(p10 + c) * w10;
      if (v11) acc = acc + *(const f32x4*)(p11 + c) * w11;
      const int g = c / Cg, cg = c - g * Cg;
      *(f32x4*)(cols + (size_t)g * gstride + (size_t)r * K + t * Cg + cg) = acc;
    }
  }
}

extern "C" int coocc_dcn_cols(const float* x, int x_stride, const float* off, int off_stride, int BN, int H, int W, int C, int groups,
                              int m0, int n, float* cols, void* stream) {
  COOCC_CHECK_ARG(x && off && cols && BN > 0 && H > 0 && W > 0 && C > 0 && groups > 0 && C % groups == 0 && (C / groups) % 4 == 0,
                  "dcn_cols: bad args (channels per group must be a multiple of 4)");
  COOCC_CHECK_ARG(x_stride >= C && x_stride % 4 == 0 && off_stride >= 18, "dcn_cols: row strides");
  COOCC_CHECK_ARG(((uintptr_t)x & 15) == 0 && ((uintptr_t)cols & 15) == 0, "dcn_cols: x / cols must be 16-byte aligned");
  const long long M = (long long)BN * H * W;
  COOCC_CHECK_ARG(M < (1ll << 31) && m0 >= 0 && n >= 0 && (long long)m0 + n <= M, "dcn_cols: rows [m0, m0 + n) outside the map");
  if (n == 0) return COOCC_OK;
  hipLaunchKernelGGL(k_dcn_cols, dim3(cdiv(n, 4)), dim3(256), 0, as_stream(stream), x, x_stride, off, off_stride, H, W, C, C / groups, m0,
                     n, cols);
  COOCC_LAUNCH_CHECK("k_dcn_cols");
  return COOCC_OK;
}

// ------------------------------------------------------------------ SE gates
__device__ __forceinline__ float sigmoid_f(float g) { return (float)(1.0 / (1.0 + exp(-(double)g))); }

COOCC_SCALAR_FP32 __global__ __launch_bounds__(256) void k_se_gate2(const float* __restrict__ x, int x_stride, long long M, int C,
                                                                     int rows_per_cam, const float* __restrict__ ga,
                                                                     const float* __restrict__ gb, float* __restrict__ oa,
                                                                     float* __restrict__ ob) {
  const int quads = C >> 2;
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  if (i >= M * quads) return;
  const long long m = i / quads;
  const int c = (int)(i % quads) << 2;
  const int cam = (int)(m / rows_per_cam);
  const f32x4 v = *(const f32x4*)(x + (size_t)m * x_stride + c);
  const f32x4 a = *(const f32x4*)(ga + (size_t)cam * C + c), bq = *(const f32x4*)(gb + (size_t)cam * C + c);
  f32x4 ra, rb;
#pragma unroll
  for (int e = 0; e < 4; ++e) { ra[e] = v[e] * sigmoid_f(a[e]); rb[e] = v[e] * sigmoid_f(bq[e]); }
  *(f32x4*)(oa + (size_t)m * C + c) = ra;
  *(f32x4*)(ob + (size_t)m * C + c) = rb;
}

extern "C" int coocc_se_gate2(const float* x, int x_stride, int BN, int rows_per_cam, int C, const float* gate_a, const float* gate_b,
                              float* out_a, float* out_b, void* stream) {
  COOCC_CHECK_ARG(x && gate_a && gate_b && out_a && out_b && BN > 0 && rows_per_cam > 0 && C > 0 && C % 4 == 0 && x_stride >= C &&
                      x_stride % 4 == 0, "se_gate2: bad args (C and the row stride must be multiples of 4)");
  COOCC_CHECK_ARG((((uintptr_t)x | (uintptr_t)gate_a | (uintptr_t)gate_b | (uintptr_t)out_a | (uintptr_t)out_b) & 15) == 0,
                  "se_gate2: pointers must be 16-byte aligned");
  const long long M = (long long)BN * rows_per_cam;
  hipLaunchKernelGGL(k_se_gate2, dim3(cdiv(M * (C / 4), 256)), dim3(256), 0, as_stream(stream), x, x_stride, M, C, rows_per_cam, gate_a,
                     gate_b, out_a, out_b);
  COOCC_LAUNCH_CHECK("k_se_gate2");
  return COOCC_OK;
}

// ------------------------------------------------------------------ per-camera channel means
// grid (row blocks of one camera, camera): a block never straddles two cameras.
__global__ __launch_bounds__(256) void k_cam_part4(const float* __restrict__ x, int stride, int HW, int C, double* __restrict__ part) {
  const int q = C >> 2, cq = threadIdx.x % q, r = threadIdx.x / q, R = 256 / q;
  const int m0 = blockIdx.x * COL_ROWS, m1 = min(HW, m0 + COL_ROWS);
  const float* xc = x + (size_t)blockIdx.y * HW * stride;
  double acc[1][4] = {};
  for (int m = m0 + r; m < m1; m += R) {
    const bn_f4 v = *(const bn_f4*)(xc + (size_t)m * stride + 4 * cq);
#pragma unroll
    for (int e = 0; e < 4; ++e) acc[0][e] += v[e];
  }
  col_block_reduce<1>(acc, q, r, cq, C, part + (size_t)blockIdx.y * gridDim.x * C);
}

__global__ __launch_bounds__(256) void k_cam_final4(const double* __restrict__ part, int nparts, int HW, int C, float* __restrict__ mean) {
  double t[1];
  col_final<1>(part + (size_t)blockIdx.y * nparts * C, nparts, C, t);
  const int c = blockIdx.x * 4 + (threadIdx.x & 3);
  if ((threadIdx.x >> 2) == 0 && c < C) mean[(size_t)blockIdx.y * C + c] = (float)(t[0] / HW);
}

// any C / stride: one thread per (camera, channel), rows in order
__global__ __launch_bounds__(256) void k_cam_mean(const float* __restrict__ x, int stride, int HW, int div, int C,
                                                  float* __restrict__ mean) {
  const int c = blockIdx.x * 256 + threadIdx.x;
  if (c >= C) return;
  const float* xc = x + (size_t)blockIdx.y * HW * stride + c;
  double s = 0;
  for (int m = 0; m < HW; ++m) s += xc[(size_t)m * stride];
  mean[(size_t)blockIdx.y * C + c] = (float)(s / div);
}

extern "C" size_t coocc_cam_mean_ws(int BN, int HW, int C) {
  if (BN <= 0 || HW <= 0 || C <= 0) return 0;
  return sizeof(double) * (size_t)BN * cdiv(HW, COL_ROWS) * C;
}

// out[b][c] = (sum over camera b's rows) / div: the means (div = HW) and, for the training path, the plain sums (div = 1)
static int cam_reduce(const float* x, int stride, int BN, int HW, int C, int div, float* out, void* ws, size_t ws_bytes, void* stream,
                      const char* what) {
  hipStream_t s = as_stream(stream);
  const bool fast = col_fast(C) && stride % 4 == 0 && ((uintptr_t)x & 15) == 0;
  if (fast) {
    const int nparts = cdiv(HW, COL_ROWS);
    COOCC_CHECK_ARG(ws && ((uintptr_t)ws & 7) == 0 && ws_bytes >= coocc_cam_mean_ws(BN, HW, C), "cam_mean / cam_sum: workspace too small");
    hipLaunchKernelGGL(k_cam_part4, dim3(nparts, BN), dim3(256), 0, s, x, stride, HW, C, (double*)ws);
    hipLaunchKernelGGL(k_cam_final4, dim3(cdiv(C, 4), BN), dim3(256), 0, s, (const double*)ws, nparts, div, C, out);
  } else {
    hipLaunchKernelGGL(k_cam_mean, dim3(cdiv(C, 256), BN), dim3(256), 0, s, x, stride, HW, div, C, out);
  }
  COOCC_LAUNCH_CHECK(what);
  return COOCC_OK;
}

extern "C" int coocc_cam_mean(const float* x, int stride, int BN, int HW, int C, float* mean, void* ws, size_t ws_bytes, void* stream) {
  COOCC_CHECK_ARG(x && mean && BN > 0 && BN < 65536 && HW > 0 && C > 0 && stride >= C, "cam_mean: bad args");
  return cam_reduce(x, stride, BN, HW, C, HW, mean, ws, ws_bytes, stream, "cam_mean");
}

// ------------------------------------------------------------------ per-camera bias + ReLU, in place
COOCC_SCALAR_FP32 __global__ __launch_bounds__(256) void k_cam_bias_relu(float* __restrict__ y, int y_stride, long long M, int C,
                                                                          int rows_per_cam, const float* __restrict__ bias, int relu) {
  const int quads = C >> 2;
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  if (i >= M * quads) return;
  const long long m = i / quads;
  const int c = (int)(i % quads) << 2;
  const int cam = (int)(m / rows_per_cam);
  float* p = y + (size_t)m * y_stride + c;
  f32x4 v = *(const f32x4*)p;
  const f32x4 bq = *(const f32x4*)(bias + (size_t)cam * C + c);
#pragma unroll
  for (int e = 0; e < 4; ++e) { v[e] += bq[e]; if (relu) v[e] = fmaxf(v[e], 0.f); }
  *(f32x4*)p = v;
}

extern "C" int coocc_cam_bias_relu(float* y, int y_stride, int BN, int rows_per_cam, int C, const float* bias, int relu, void* stream) {
  COOCC_CHECK_ARG(y && bias && BN > 0 && rows_per_cam > 0 && C > 0 && C % 4 == 0 && y_stride >= C && y_stride % 4 == 0,
                  "cam_bias_relu: bad args (C and the row stride must be multiples of 4)");
  COOCC_CHECK_ARG((((uintptr_t)y | (uintptr_t)bias) & 15) == 0, "cam_bias_relu: pointers must be 16-byte aligned");
  const long long M = (long long)BN * rows_per_cam;
  hipLaunchKernelGGL(k_cam_bias_relu, dim3(cdiv(M * (C / 4), 256)), dim3(256), 0, as_stream(stream), y, y_stride, M, C, rows_per_cam, bias,
                     relu);
  COOCC_LAUNCH_CHECK("k_cam_bias_relu");
  return COOCC_OK;
}

// ================================================================== training (DepthNet.train_enabled)
//   k_dcn_cols_bwd    the adjoint of k_dcn_cols, same geometry (one wave per pixel, wave-uniform positions / weights / validity).
//                     doff: lanes run over channel quads, a per-lane fp32 partial and a fixed-order wave reduction -- deterministic.
//                     dx:   fp32 atomic adds of w_corner * dcol, lanes over single channels so that each wave instruction covers one
//                     contiguous row segment.  The only place of the training path whose bits may differ from run to run.
//   k_gate2_bwd*      dx = d_oa sigmoid(ga) + d_ob sigmoid(gb) in one pass; dga / dgb per camera in fp64, fixed order (colreduce.h).
//   coocc_cam_sum     per-camera column sums (k_cam_part4 / k_cam_final4 with divisor 1): the adjoint of adding a camera's vector.
//   k_cam_add         y = x + v[camera] * scale: the pooled branch's vector onto ASPP's 1x1 (scale 1) and the adjoint of the camera
//                     means (x = NULL, scale 1 / HW).
//   k_dropout_rows    y = x * mask * scale.

// ------------------------------------------------------------------ adjoint of the deformable sampler
COOCC_SCALAR_FP32 __global__ __launch_bounds__(256) void k_dcn_cols_bwd(const float* __restrict__ x, int x_stride,
                                                                         const float* __restrict__ off, int off_stride, int H, int W,
                                                                         int C, int Cg, int m0, int n, const float* __restrict__ dcols,
                                                                         float* __restrict__ dx, float* __restrict__ doff) {
  const int r = __builtin_amdgcn_readfirstlane(blockIdx.x * 4 + (threadIdx.x >> 6)), lane = threadIdx.x & 63;
  if (r >= n) return;
  const int m = m0 + r;
  const int px = m % W, py = (m / W) % H, b = m / (W * H);
  const float* o = off + (size_t)m * off_stride;
  float* dor = doff + (size_t)r * off_stride;
  for (int j = 18 + lane; j < off_stride; j += 64) dor[j] = 0.f;
  const int K = 9 * Cg;
  const size_t gstride = (size_t)n * K;
  const int quads = C >> 2;
  for (int t = 0; t < 9; ++t) {
    const float sy = (float)(py - 1 + t / 3) + o[2 * t], sx = (float)(px - 1 + t % 3) + o[2 * t + 1];
    const bool inside = sy > -1.f && sy < (float)H && sx > -1.f && sx < (float)W;
    float gy = 0.f, gx = 0.f;
    if (inside) {
      const float fy = floorf(sy), fx = floorf(sx);
      const int y0 = (int)fy, x0 = (int)fx;              // y0 in [-1, H-1], x0 in [-1, W-1]
      const float ly = sy - fy, lx = sx - fx, hy = 1.f - ly, hx = 1.f - lx;
      const bool ylo = y0 >= 0, yhi = y0 + 1 <= H - 1, xlo = x0 >= 0, xhi = x0 + 1 <= W - 1;
      const bool v00 = ylo && xlo, v01 = ylo && xhi, v10 = yhi && xlo, v11 = yhi && xhi;
      const float w00 = hy * hx, w01 = hy * lx, w10 = ly * hx, w11 = ly * lx;
      const size_t base = (size_t)b * H * W;
      size_t r00 = 0, r01 = 0, r10 = 0, r11 = 0;         // rows of the valid corners; formed only after the range tests
      if (v00) r00 = base + (size_t)y0 * W + x0;
      if (v01) r01 = base + (size_t)y0 * W + x0 + 1;
      if (v10) r10 = base + (size_t)(y0 + 1) * W + x0;
      if (v11) r11 = base + (size_t)(y0 + 1) * W + x0 + 1;
      const float* drow = dcols + (size_t)r * K + t * Cg;
      for (int q = lane; q < quads; q += 64) {
        const int c = q << 2;
        const int g = c / Cg, cg = c - g * Cg;
        const f32x4 d = *(const f32x4*)(drow + (size_t)g * gstride + cg);
        f32x4 a00 = {0.f, 0.f, 0.f, 0.f}, a01 = a00, a10 = a00, a11 = a00;
        if (v00) a00 = *(const f32x4*)(x + r00 * x_stride + c);
        if (v01) a01 = *(const f32x4*)(x + r01 * x_stride + c);
        if (v10) a10 = *(const f32x4*)(x + r10 * x_stride + c);
        if (v11) a11 = *(const f32x4*)(x + r11 * x_stride + c);
        const f32x4 ty = (a10 - a00) * hx + (a11 - a01) * lx, tx = (a01 - a00) * hy + (a11 - a10) * ly;
#pragma unroll
        for (int e = 0; e < 4; ++e) { gy += d[e] * ty[e]; gx += d[e] * tx[e]; }
      }
      for (int c = lane; c < C; c += 64) {
        const int g = c / Cg;
        const float d = drow[(size_t)g * gstride + (c - g * Cg)];
        if (v00) unsafeAtomicAdd(dx + r00 * C + c, w00 * d);
        if (v01) unsafeAtomicAdd(dx + r01 * C + c, w01 * d);
        if (v10) unsafeAtomicAdd(dx + r10 * C + c, w10 * d);
        if (v11) unsafeAtomicAdd(dx + r11 * C + c, w11 * d);
      }
    }
    for (int s = 32; s >= 1; s >>= 1) { gy += __shfl_xor(gy, s); gx += __shfl_xor(gx, s); }
    if (lane == 0) { dor[2 * t] = gy; dor[2 * t + 1] = gx; }
  }
}

extern "C" int coocc_dcn_cols_bwd(const float* x, int x_stride, const float* off, int off_stride, int BN, int H, int W, int C,
                                  int groups, int m0, int n, const float* dcols, float* dx, float* doff, void* stream) {
  COOCC_CHECK_ARG(x && off && dcols && dx && doff && BN > 0 && H > 0 && W > 0 && C > 0 && groups > 0 && C % groups == 0 &&
                      (C / groups) % 4 == 0, "dcn_cols_bwd: bad args (channels per group must be a multiple of 4)");
  COOCC_CHECK_ARG(x_stride >= C && x_stride % 4 == 0 && off_stride >= 18, "dcn_cols_bwd: row strides");
  COOCC_CHECK_ARG(((uintptr_t)x & 15) == 0 && ((uintptr_t)dcols & 15) == 0, "dcn_cols_bwd: x / dcols must be 16-byte aligned");
  const long long M = (long long)BN * H * W;
  COOCC_CHECK_ARG(M < (1ll << 31) && m0 >= 0 && n >= 0 && (long long)m0 + n <= M, "dcn_cols_bwd: rows [m0, m0 + n) outside the map");
  if (n == 0) return COOCC_OK;
  hipLaunchKernelGGL(k_dcn_cols_bwd, dim3(cdiv(n, 4)), dim3(256), 0, as_stream(stream), x, x_stride, off, off_stride, H, W, C,
                     C / groups, m0, n, dcols, dx, doff);
  COOCC_LAUNCH_CHECK("k_dcn_cols_bwd");
  return COOCC_OK;
}

// ------------------------------------------------------------------ SE gates, backward
__device__ __forceinline__ double dsigmoid_d(float g) { const double s = 1.0 / (1.0 + exp(-(double)g)); return s * (1.0 - s); }

// grid (row blocks of one camera, camera): dx of the block's rows and its fp64 partials of sum x d_oa | sum x d_ob
COOCC_SCALAR_FP32 __global__ __launch_bounds__(256) void k_gate2_bwd_part4(const float* __restrict__ x, int x_stride, int HW, int C,
                                                                            const float* __restrict__ ga, const float* __restrict__ gb,
                                                                            const float* __restrict__ da, const float* __restrict__ db,
                                                                            float* __restrict__ dx, double* __restrict__ part) {
  const int q = C >> 2, cq = threadIdx.x % q, r = threadIdx.x / q, R = 256 / q;
  const int m0 = blockIdx.x * COL_ROWS, m1 = min(HW, m0 + COL_ROWS);
  const size_t row0 = (size_t)blockIdx.y * HW;
  const f32x4 a = *(const f32x4*)(ga + (size_t)blockIdx.y * C + 4 * cq), bq = *(const f32x4*)(gb + (size_t)blockIdx.y * C + 4 * cq);
  f32x4 sa, sb;
#pragma unroll
  for (int e = 0; e < 4; ++e) { sa[e] = sigmoid_f(a[e]); sb[e] = sigmoid_f(bq[e]); }
  double acc[2][4] = {};
  for (int m = m0 + r; m < m1; m += R) {
    const f32x4 v = *(const f32x4*)(x + (row0 + m) * x_stride + 4 * cq);
    const f32x4 ua = *(const f32x4*)(da + (row0 + m) * C + 4 * cq), ub = *(const f32x4*)(db + (row0 + m) * C + 4 * cq);
    f32x4 o;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      o[e] = ua[e] * sa[e] + ub[e] * sb[e];
      acc[0][e] += (double)v[e] * (double)ua[e];
      acc[1][e] += (double)v[e] * (double)ub[e];
    }
    *(f32x4*)(dx + (row0 + m) * C + 4 * cq) = o;
  }
  col_block_reduce<2>(acc, q, r, cq, C, part + (size_t)blockIdx.y * gridDim.x * C * 2);
}

__global__ __launch_bounds__(256) void k_gate2_bwd_final4(const double* __restrict__ part, int nparts, int C,
                                                          const float* __restrict__ ga, const float* __restrict__ gb,
                                                          float* __restrict__ dga, float* __restrict__ dgb) {
  double t[2];
  col_final<2>(part + (size_t)blockIdx.y * nparts * C * 2, nparts, C, t);
  const int c = blockIdx.x * 4 + (threadIdx.x & 3);
  if ((threadIdx.x >> 2) == 0 && c < C) {
    const size_t i = (size_t)blockIdx.y * C + c;
    dga[i] = (float)(dsigmoid_d(ga[i]) * t[0]);
    dgb[i] = (float)(dsigmoid_d(gb[i]) * t[1]);
  }
}

// any C % 4 == 0: the elementwise pass, then one thread per (camera, channel) with the rows in order
COOCC_SCALAR_FP32 __global__ __launch_bounds__(256) void k_gate2_bwd_dx(long long M, int C, int rows_per_cam,
                                                                         const float* __restrict__ ga, const float* __restrict__ gb,
                                                                         const float* __restrict__ da, const float* __restrict__ db,
                                                                         float* __restrict__ dx) {
  const int quads = C >> 2;
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  if (i >= M * quads) return;
  const long long m = i / quads;
  const int c = (int)(i % quads) << 2;
  const int cam = (int)(m / rows_per_cam);
  const f32x4 a = *(const f32x4*)(ga + (size_t)cam * C + c), bq = *(const f32x4*)(gb + (size_t)cam * C + c);
  const f32x4 ua = *(const f32x4*)(da + (size_t)m * C + c), ub = *(const f32x4*)(db + (size_t)m * C + c);
  f32x4 o;
#pragma unroll
  for (int e = 0; e < 4; ++e) o[e] = ua[e] * sigmoid_f(a[e]) + ub[e] * sigmoid_f(bq[e]);
  *(f32x4*)(dx + (size_t)m * C + c) = o;
}

__global__ __launch_bounds__(256) void k_gate2_bwd_cols(const float* __restrict__ x, int x_stride, int HW, int C,
                                                        const float* __restrict__ ga, const float* __restrict__ gb,
                                                        const float* __restrict__ da, const float* __restrict__ db,
                                                        float* __restrict__ dga, float* __restrict__ dgb) {
  const int c = blockIdx.x * 256 + threadIdx.x;
  if (c >= C) return;
  const size_t row0 = (size_t)blockIdx.y * HW;
  double s0 = 0, s1 = 0;
  for (int m = 0; m < HW; ++m) {
    const double v = x[(row0 + m) * x_stride + c];
    s0 += v * (double)da[(row0 + m) * C + c];
    s1 += v * (double)db[(row0 + m) * C + c];
  }
  const size_t i = (size_t)blockIdx.y * C + c;
  dga[i] = (float)(dsigmoid_d(ga[i]) * s0);
  dgb[i] = (float)(dsigmoid_d(gb[i]) * s1);
}

extern "C" size_t coocc_se_gate2_bwd_ws(int BN, int HW, int C) {
  if (BN <= 0 || HW <= 0 || C <= 0) return 0;
  return sizeof(double) * 2 * (size_t)BN * cdiv(HW, COL_ROWS) * C;
}

extern "C" int coocc_se_gate2_bwd(const float* x, int x_stride, int BN, int rows_per_cam, int C, const float* gate_a,
                                  const float* gate_b, const float* d_out_a, const float* d_out_b, float* dx, float* dgate_a,
                                  float* dgate_b, void* ws, size_t ws_bytes, void* stream) {
  COOCC_CHECK_ARG(x && gate_a && gate_b && d_out_a && d_out_b && dx && dgate_a && dgate_b && BN > 0 && BN < 65536 && rows_per_cam > 0 &&
                      C > 0 && C % 4 == 0 && x_stride >= C && x_stride % 4 == 0,
                  "se_gate2_bwd: bad args (C and the row stride must be multiples of 4)");
  COOCC_CHECK_ARG((((uintptr_t)x | (uintptr_t)gate_a | (uintptr_t)gate_b | (uintptr_t)d_out_a | (uintptr_t)d_out_b | (uintptr_t)dx) & 15) == 0,
                  "se_gate2_bwd: pointers must be 16-byte aligned");
  hipStream_t s = as_stream(stream);
  const int HW = rows_per_cam;
  if (col_fast(C)) {
    const int nparts = cdiv(HW, COL_ROWS);
    COOCC_CHECK_ARG(ws && ((uintptr_t)ws & 7) == 0 && ws_bytes >= coocc_se_gate2_bwd_ws(BN, HW, C), "se_gate2_bwd: workspace too small");
    hipLaunchKernelGGL(k_gate2_bwd_part4, dim3(nparts, BN), dim3(256), 0, s, x, x_stride, HW, C, gate_a, gate_b, d_out_a, d_out_b, dx,
                       (double*)ws);
    hipLaunchKernelGGL(k_gate2_bwd_final4, dim3(cdiv(C, 4), BN), dim3(256), 0, s, (const double*)ws, nparts, C, gate_a, gate_b, dgate_a,
                       dgate_b);
  } else {
    const long long M = (long long)BN * HW;
    hipLaunchKernelGGL(k_gate2_bwd_dx, dim3(cdiv(M * (C / 4), 256)), dim3(256), 0, s, M, C, HW, gate_a, gate_b, d_out_a, d_out_b, dx);
    hipLaunchKernelGGL(k_gate2_bwd_cols, dim3(cdiv(C, 256), BN), dim3(256), 0, s, x, x_stride, HW, C, gate_a, gate_b, d_out_a, d_out_b,
                       dgate_a, dgate_b);
  }
  COOCC_LAUNCH_CHECK("se_gate2_bwd");
  return COOCC_OK;
}

// ------------------------------------------------------------------ per-camera column sums, camera vector onto rows, dropout
extern "C" int coocc_cam_sum(const float* x, int stride, int BN, int HW, int C, float* sum, void* ws, size_t ws_bytes, void* stream) {
  COOCC_CHECK_ARG(x && sum && BN > 0 && BN < 65536 && HW > 0 && C > 0 && stride >= C, "cam_sum: bad args");
  return cam_reduce(x, stride, BN, HW, C, 1, sum, ws, ws_bytes, stream, "cam_sum");
}

COOCC_SCALAR_FP32 __global__ __launch_bounds__(256) void k_cam_add(const float* __restrict__ x, float* __restrict__ y, long long M, int C,
                                                                    int rows_per_cam, const float* __restrict__ v, float scale) {
  const int quads = C >> 2;
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  if (i >= M * quads) return;
  const long long m = i / quads;
  const int c = (int)(i % quads) << 2;
  const int cam = (int)(m / rows_per_cam);
  const f32x4 vq = *(const f32x4*)(v + (size_t)cam * C + c);
  f32x4 o = {0.f, 0.f, 0.f, 0.f};
  if (x) o = *(const f32x4*)(x + (size_t)m * C + c);
#pragma unroll
  for (int e = 0; e < 4; ++e) o[e] += vq[e] * scale;
  *(f32x4*)(y + (size_t)m * C + c) = o;
}

extern "C" int coocc_cam_add(const float* x, float* y, int BN, int rows_per_cam, int C, const float* v, float scale, void* stream) {
  COOCC_CHECK_ARG(y && v && BN > 0 && rows_per_cam > 0 && C > 0 && C % 4 == 0, "cam_add: bad args (C must be a multiple of 4)");
  COOCC_CHECK_ARG((((uintptr_t)x | (uintptr_t)y | (uintptr_t)v) & 15) == 0, "cam_add: pointers must be 16-byte aligned");
  const long long M = (long long)BN * rows_per_cam;
  hipLaunchKernelGGL(k_cam_add, dim3(cdiv(M * (C / 4), 256)), dim3(256), 0, as_stream(stream), x, y, M, C, rows_per_cam, v, scale);
  COOCC_LAUNCH_CHECK("k_cam_add");
  return COOCC_OK;
}

COOCC_SCALAR_FP32 __global__ __launch_bounds__(256) void k_dropout_rows(const float* __restrict__ x, const uint8_t* __restrict__ mask,
                                                                         long long quads, float scale, float* __restrict__ y) {
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  if (i >= quads) return;
  const f32x4 v = *(const f32x4*)(x + 4 * i);
  const uchar4 k = *(const uchar4*)(mask + 4 * i);
  f32x4 o;
  o[0] = v[0] * (float)k.x * scale; o[1] = v[1] * (float)k.y * scale; o[2] = v[2] * (float)k.z * scale; o[3] = v[3] * (float)k.w * scale;
  *(f32x4*)(y + 4 * i) = o;
}

extern "C" int coocc_dropout_rows(const float* x, const uint8_t* mask, int64_t M, int C, float scale, float* y, void* stream) {
  COOCC_CHECK_ARG(x && mask && y && M > 0 && C > 0 && C % 4 == 0, "dropout_rows: bad args (C must be a multiple of 4)");
  COOCC_CHECK_ARG((((uintptr_t)x | (uintptr_t)y) & 15) == 0 && ((uintptr_t)mask & 3) == 0, "dropout_rows: alignment (x, y 16 bytes; mask 4)");
  const long long quads = (long long)M * (C / 4);
  hipLaunchKernelGGL(k_dropout_rows, dim3(cdiv(quads, 256)), dim3(256), 0, as_stream(stream), x, mask, quads, scale, y);
  COOCC_LAUNCH_CHECK("k_dropout_rows");
  return COOCC_OK;
}
