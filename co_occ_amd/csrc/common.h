// Shared helpers for libcoocc_hip.so (gfx950 only; wave = 64 lanes).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>

#include "../../include/coocc_hip.h"

#define COOCC_WAVE 64

int coocc_set_error(int code, const char* fmt, ...);

#define COOCC_CHECK_ARG(cond, ...)                                  \
  do {                                                              \
    if (!(cond)) return coocc_set_error(COOCC_EINVAL, __VA_ARGS__); \
  } while (0)

#define COOCC_HIP(call)                                                                   \
  do {                                                                                    \
    hipError_t e__ = (call);                                                              \
    if (e__ != hipSuccess)                                                                \
      return coocc_set_error(COOCC_EHIP, "%s failed: %s (%s:%d)", #call,                  \
                             hipGetErrorString(e__), __FILE__, __LINE__);                 \
  } while (0)

#define COOCC_LAUNCH_CHECK(name)                                                          \
  do {                                                                                    \
    hipError_t e__ = hipGetLastError();                                                   \
    if (e__ != hipSuccess)                                                                \
      return coocc_set_error(COOCC_EHIP, "launch of %s failed: %s", name,                 \
                             hipGetErrorString(e__));                                     \
  } while (0)

// Kernel attribute: no packed-fp32 VALU instructions (v_pk_fma_f32 / v_pk_mul_f32 / v_pk_add_f32 / v_pk_mov_b32) in this kernel.
// gfx950 hazard found in round 6 (profiles/r6_pk_opsel_probe.txt, tools/proto/pk_opsel_probe.hip): a packed-fp32 instruction whose op_sel
// routes the HIGH dword of src1 into the LOW result (what hipcc emits for `vec * other[1]`) reads that operand as 0.0 in lanes 48-63
// now and then WHILE a wave of another kernel on the same SIMD runs a 128-bit-operand MFMA (v_mfma_f32_32x32x16_f16 ...): bit-exact
// alone, wrong next to this package's own split-f16 GEMMs.  Every kernel whose ISA held that form carries this attribute, and
// tools/isa_lint.py (tests/test_isa_lint.py) checks the built library for it.
#define COOCC_SCALAR_FP32 __attribute__((target("no-packed-fp32-ops")))

static inline hipStream_t as_stream(void* s) { return (hipStream_t)s; }
static inline unsigned cdiv(long long a, long long b) { return (unsigned)((a + b - 1) / b); }
// Workspace carving (host): every array of a workspace starts on a 256-byte boundary, counted from the aligned base.
static inline size_t al256(size_t n) { return (n + 255) & ~(size_t)255; }
static inline char* ws_base256(void* ws) { return (char*)al256((uintptr_t)ws); }

// Mean and rstd (two-pass, biased variance) of the cpg channels one thread of the row-wise GroupNorm kernels walks (k_groupnorm_rows,
// k_groupnorm_rows_bwd).  Acc = float: the sequential fp32 sums of the 4-channel groups of the fine branch.  Groups wider than
// GN_WIDE_GROUP take Acc = double, and keep the mean in it for x - mean: a sequential fp32 sum over thousands of channels put y at
// 5-11 x the fp32 noise floor from float64, and the fp32 rounding of the mean is an ABSOLUTE error of xhat that dgamma's terms near
// xhat = 0 do not forgive (tests/test_gpu_norm.py, C / groups = 2048).
constexpr int GN_WIDE_GROUP = 64;
template <typename Acc>
__device__ __forceinline__ void gn_group_stats(const float* __restrict__ p, int cpg, float eps, Acc& mean, float& rstd) {
  mean = 0;
  for (int c = 0; c < cpg; ++c) mean += p[c];
  mean /= (Acc)cpg;
  Acc var = 0;
  for (int c = 0; c < cpg; ++c) { Acc d = p[c] - mean; var += d * d; }
  var /= (Acc)cpg;
  rstd = 1.f / sqrtf((float)var + eps);
}

// a * b rounded to fp32 and never fused into an addition that consumes it
__device__ __forceinline__ float mul_unfused(float a, float b) {
#pragma clang fp contract(off)
  return a * b;
}

// squared distance with the contraction nvcc applies to the reference expression
// (furthest_point_sample_cuda.cu:65-66, ball_query_cuda.cu:41-42); see oracle/c/coocc_oracle.c.
__device__ __forceinline__ float sqdist3(float x1, float y1, float z1, float x2, float y2,
                                         float z2) {
  float dx = x2 - x1, dy = y2 - y1, dz = z2 - z1;
  return __fmaf_rn(dz, dz, __fmaf_rn(dy, dy, __fmul_rn(dx, dx)));
}
