// Training of the LiDAR-only trunk (SECOND3D + SECOND3DFPN, co_occ_amd/lidar_trunk.py run_trunk_train): the one kernel the
// table-driven backward of the conv family (csrc/conv_bwd.hip, whose row tables take per-axis kernel / stride / padding) lacks.
//  * k_fpn_sum_bwd: backward of k_fpn_sum (csrc/second_fpn.hip).  d sum / d level = 1, so every level's gradient is dout itself,
//    re-laid into that deblock's child-major rows [B*(X/s)*(Y/s)*Z][s*s][C]: a pure gather-free scatter of whole rows, every fine
//    voxel owning exactly one child slot per level.  dout is read once for all levels.  HBM-bound: (1 + levels written) * rows * C * 4 bytes.
#include <string.h>

#include "common.h"

typedef float f32x4 __attribute__((ext_vector_type(4)));

struct FpnSumBwdK {
  const float* dout;     // [B*X*Y*Z][dout_stride], C channels
  float* du[4];          // level l: [B*(X/s)*(Y/s)*Z][s*s][C], or NULL (not wanted: a stride-1 level's gradient is dout itself)
  int s[4];
  int levels, X, Y, Z, C, dout_stride;
  long long rows;
};

// The forward's shape: 32 lanes per fine row (one dwordx4 per lane and 128 channels), 8 rows per workgroup; the row is loaded once
// and stored to its child slot on every level.  No arithmetic: bit-exact.
__global__ __launch_bounds__(256) COOCC_SCALAR_FP32 void k_fpn_sum_bwd(FpnSumBwdK p) {
  const long long row = (long long)blockIdx.x * 8 + (threadIdx.x >> 5);
  if (row >= p.rows) return;
  const int lane = threadIdx.x & 31;
  const int z = (int)(row % p.Z);
  long long q = row / p.Z;
  const int y = (int)(q % p.Y); q /= p.Y;
  const int x = (int)(q % p.X);
  const long long b = q / p.X;
  float* dst[4];
#pragma unroll
  for (int l = 0; l < 4; ++l) {
    dst[l] = nullptr;
    if (l < p.levels && p.du[l]) {
      const int s = p.s[l];
      const long long crow = ((b * (p.X / s) + x / s) * (p.Y / s) + y / s) * p.Z + z;
      dst[l] = p.du[l] + (crow * (s * s) + (x % s) * s + (y % s)) * p.C;
    }
  }
  const float* src = p.dout + row * p.dout_stride;
  for (int n = lane * 4; n < p.C; n += 128) {
    const f32x4 v = *(const f32x4*)(src + n);
#pragma unroll
    for (int l = 0; l < 4; ++l)
      if (dst[l]) *(f32x4*)(dst[l] + n) = v;
  }
}

extern "C" int coocc_fpn_sum_bwd(const float* dout, int dout_stride, float* const* dups, const int* strides, int levels, int B, int X,
                                 int Y, int Z, int C, void* stream) {
  COOCC_CHECK_ARG(dout && dups && strides && levels >= 1 && levels <= 4, "fpn_sum_bwd: 1-4 levels");
  COOCC_CHECK_ARG(B > 0 && X > 0 && Y > 0 && Z > 0 && C > 0 && C % 4 == 0 && dout_stride >= C && dout_stride % 4 == 0 && ((uintptr_t)dout & 15) == 0,
                  "fpn_sum_bwd: bad sizes (C, dout_stride %% 4 == 0, 16-byte aligned rows)");
  FpnSumBwdK k;
  memset(&k, 0, sizeof(k));
  int wanted = 0;
  for (int l = 0; l < levels; ++l) {
    const int s = strides[l];
    COOCC_CHECK_ARG(s == 1 || s == 2 || s == 4 || s == 8, "fpn_sum_bwd: upsample strides are 1, 2, 4 or 8");
    COOCC_CHECK_ARG(X % s == 0 && Y % s == 0, "fpn_sum_bwd: the grid is not a multiple of a level's stride");
    COOCC_CHECK_ARG(((uintptr_t)dups[l] & 15) == 0, "fpn_sum_bwd: misaligned level");
    COOCC_CHECK_ARG(dups[l] != dout, "fpn_sum_bwd: a level's gradient aliases dout (pass NULL for a stride-1 level)");
    k.du[l] = dups[l];
    k.s[l] = s;
    wanted += dups[l] != nullptr;
  }
  if (!wanted) return COOCC_OK;          // every level skipped (stride 1 everywhere): nothing to write
  k.dout = dout; k.dout_stride = dout_stride;
  k.levels = levels; k.X = X; k.Y = Y; k.Z = Z; k.C = C;
  k.rows = (long long)B * X * Y * Z;
  COOCC_CHECK_ARG(k.rows < (1ll << 31) * 8, "fpn_sum_bwd: too many rows");
  hipLaunchKernelGGL(k_fpn_sum_bwd, dim3(cdiv(k.rows, 8)), dim3(256), 0, as_stream(stream), k);
  COOCC_LAUNCH_CHECK("k_fpn_sum_bwd");
  return COOCC_OK;
}
