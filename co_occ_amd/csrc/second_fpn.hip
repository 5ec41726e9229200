// The LiDAR-only trunk's own kernels (SECOND3D + SECOND3DFPN, co_occ_amd/lidar_trunk.py):
//  * k_fpn_sum: the neck's  sum(ups)  (second3d_fpn.py:119-122) over the outputs of its deblocks.  A ConvTranspose3d with
//    kernel = stride = (1, s, s) has no overlap -- every coarse voxel produces its s*s children -- so each deblock is a pointwise
//    GEMM Cin -> s*s*Cout on the COARSE rows (BN + ReLU in its epilogue) and this kernel gathers, for every fine voxel, the child
//    slot of its parent on each level and adds them in the reference's order ((0 + u0) + u1) + u2.
//  * k_zyx_to_rows: the trunk's entry transposition, the reference's [B,C,Z,Y,X] volume -> channels-last rows in this library's
//    (b, x, y, z) order, in one pass (coocc_ncdhw_to_ndhwc keeps the voxel order of its source).
// Both are pure data movement: HBM-bound, judged as a share of the 8 TB/s peak.
#include <string.h>

#include "common.h"
#include "h2_rows.h"

int coocc_h2_flag_ptr(int** out);

struct FpnSumK {
  const float* u[4];     // level l: [B * (X/s) * (Y/s) * Z][s*s][C] rows (coarse voxel, child = (x % s) * s + (y % s), channel)
  int s[4];
  int levels, X, Y, Z, C, out_stride;
  long long rows;
  float* out;
  void* out_h2t;         // H2 twin [rows][C] of the sum (C % 32 == 0), or NULL
  int* h2_flag;
};

// 32 lanes per output row (128 channels = one dwordx4 per lane and level), 8 rows per workgroup; the child offset comes from the
// output coordinate, no index table.  COOCC_SCALAR_FP32: plain v_add_f32, none of the packed-fp32 forms of DESIGN.md 3.9.
__global__ __launch_bounds__(256) COOCC_SCALAR_FP32 void k_fpn_sum(FpnSumK p) {
  const long long row = (long long)blockIdx.x * 8 + (threadIdx.x >> 5);
  if (row >= p.rows) return;
  const int lane = threadIdx.x & 31;
  const int z = (int)(row % p.Z);
  long long q = row / p.Z;
  const int y = (int)(q % p.Y); q /= p.Y;
  const int x = (int)(q % p.X);
  const long long b = q / p.X;
  const float* src[4];
#pragma unroll
  for (int l = 0; l < 4; ++l) {
    if (l < p.levels) {
      const int s = p.s[l];
      const long long crow = ((b * (p.X / s) + x / s) * (p.Y / s) + y / s) * p.Z + z;
      src[l] = p.u[l] + (crow * (s * s) + (x % s) * s + (y % s)) * p.C;
    } else src[l] = nullptr;
  }
  for (int n = lane * 4; n < p.C; n += 128) {
    f32x4 v[4];
#pragma unroll
    for (int l = 0; l < 4; ++l)
      if (l < p.levels) v[l] = *(const f32x4*)(src[l] + n);
    f32x4 acc = f32x4{0.f, 0.f, 0.f, 0.f} + v[0];          // sum() starts from int 0: 0 + u0 (turns a -0.0 into +0.0, as torch does)
#pragma unroll
    for (int l = 1; l < 4; ++l)
      if (l < p.levels) acc = acc + v[l];
    *(f32x4*)(p.out + row * p.out_stride + n) = acc;
    if (p.out_h2t) { store_h2(p.out_h2t, (size_t)row, p.C, n, acc); h2_guard(p.h2_flag, acc); }
  }
}

extern "C" int coocc_fpn_sum(const float* const* ups, const int* strides, int levels, int B, int X, int Y, int Z, int C, float* out,
                             int out_stride, void* out_h2_twin, void* stream) {
  COOCC_CHECK_ARG(ups && strides && out && levels >= 1 && levels <= 4, "fpn_sum: 1-4 levels");
  COOCC_CHECK_ARG(B > 0 && X > 0 && Y > 0 && Z > 0 && C > 0 && C % 4 == 0 && out_stride >= C && out_stride % 4 == 0 && ((uintptr_t)out & 15) == 0,
                  "fpn_sum: bad sizes (C, out_stride %% 4 == 0, 16-byte aligned rows)");
  COOCC_CHECK_ARG(!out_h2_twin || (C % 32 == 0 && ((uintptr_t)out_h2_twin & 15) == 0), "fpn_sum: the H2 twin needs C %% 32 == 0");
  FpnSumK k;
  memset(&k, 0, sizeof(k));
  for (int l = 0; l < levels; ++l) {
    const int s = strides[l];
    COOCC_CHECK_ARG(s == 1 || s == 2 || s == 4 || s == 8, "fpn_sum: upsample strides are 1, 2, 4 or 8");
    COOCC_CHECK_ARG(X % s == 0 && Y % s == 0, "fpn_sum: the grid is not a multiple of a level's stride (levels of different sizes)");
    COOCC_CHECK_ARG(ups[l] && ((uintptr_t)ups[l] & 15) == 0, "fpn_sum: null / misaligned level");
    k.u[l] = ups[l];
    k.s[l] = s;
  }
  k.levels = levels; k.X = X; k.Y = Y; k.Z = Z; k.C = C; k.out_stride = out_stride;
  k.rows = (long long)B * X * Y * Z;
  COOCC_CHECK_ARG(k.rows < (1ll << 31) * 8, "fpn_sum: too many rows");
  k.out = out;
  k.out_h2t = out_h2_twin;
  if (out_h2_twin) {
    const int rc = coocc_h2_flag_ptr(&k.h2_flag);
    if (rc != COOCC_OK) return rc;
  }
  hipLaunchKernelGGL(k_fpn_sum, dim3(cdiv(k.rows, 8)), dim3(256), 0, as_stream(stream), k);
  COOCC_LAUNCH_CHECK("k_fpn_sum");
  return COOCC_OK;
}

// One workgroup: 64 consecutive elements of the flattened (y, x) plane of one (b, z) -- the source's contiguous axis, so every
// tile but the plane's last is full whatever X is -- x one 128-channel slab, staged through LDS.  Reads: dwordx4 along (y, x), 16 lanes
// = 256 contiguous bytes per channel (VEC: Y*X % 4 == 0 and a 16-byte aligned source; else 4-byte loads, 64 lanes along the
// plane).  LDS rows are 129 floats: the staging writes and the row reads below are both 2-way at worst over 64 lanes.  Writes: 32
// lanes along the channels of one row, 128 contiguous bytes per instruction and row, two rows per wave instruction.
#define ZT_X 64
#define ZT_C 128
template <bool VEC>
__global__ __launch_bounds__(256) void k_zyx_to_rows(const float* __restrict__ src, float* __restrict__ dst, int C, int Z, int Y, int X,
                                                      int dst_stride, int dst_coff) {
  __shared__ float tile[ZT_X][ZT_C + 1];
  const int t = threadIdx.x;
  const int YX = Y * X;
  const int p0 = blockIdx.x * ZT_X;
  const int z = blockIdx.y;
  const int cslabs = (C + ZT_C - 1) / ZT_C;
  const int b = blockIdx.z / cslabs, c0 = (blockIdx.z % cslabs) * ZT_C;
  const int cn = min(ZT_C, C - c0);
  const size_t plane = (size_t)Z * YX;
  const float* base = src + ((size_t)b * C + c0) * plane + (size_t)z * YX;
  if (VEC) {
    const int q = t & 15, p = p0 + 4 * q;                 // p % 4 == 0 and YX % 4 == 0: p < YX covers p .. p + 3
    for (int c = t >> 4; c < cn; c += 16) {
      const f32x4 v = p < YX ? *(const f32x4*)(base + (size_t)c * plane + p) : f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int e = 0; e < 4; ++e) tile[4 * q + e][c] = v[e];
    }
  } else {
    const int p = p0 + (t & 63);
    for (int c = t >> 6; c < cn; c += 4) tile[t & 63][c] = p < YX ? base[(size_t)c * plane + p] : 0.f;
  }
  __syncthreads();
  const int j = t & 31;
  for (int r = t >> 5; r < ZT_X; r += 8) {
    const int p = p0 + r;
    if (p >= YX) break;
    const int y = p / X, x = p - y * X;
    float* o = dst + ((((size_t)b * X + x) * Y + y) * Z + z) * dst_stride + dst_coff + c0;
#pragma unroll
    for (int e = 0; e < 4; ++e)
      if (j + 32 * e < cn) o[j + 32 * e] = tile[r][j + 32 * e];
  }
}

extern "C" int coocc_zyx_to_rows(const float* src, float* dst, int B, int C, int Z, int Y, int X, int dst_stride, int dst_coff,
                                 void* stream) {
  COOCC_CHECK_ARG(src && dst && B > 0 && C > 0 && Z > 0 && Y > 0 && X > 0 && dst_stride >= dst_coff + C, "zyx_to_rows: bad args");
  COOCC_CHECK_ARG(C % 4 == 0 && dst_stride % 4 == 0 && dst_coff % 4 == 0 && ((uintptr_t)dst & 15) == 0, "zyx_to_rows: 16-byte aligned rows (C, stride, offset %% 4 == 0)");
  const long long gz = (long long)B * ((C + ZT_C - 1) / ZT_C);
  COOCC_CHECK_ARG((long long)Y * X < (1ll << 30) && Z <= 65535 && gz <= 65535, "zyx_to_rows: Z and B*ceil(C/128) must fit a grid dimension (65535)");
  dim3 grid(cdiv((long long)Y * X, ZT_X), (unsigned)Z, (unsigned)gz);
  if (((long long)Y * X) % 4 == 0 && ((uintptr_t)src & 15) == 0)
    hipLaunchKernelGGL(k_zyx_to_rows<true>, grid, dim3(256), 0, as_stream(stream), src, dst, C, Z, Y, X, dst_stride, dst_coff);
  else
    hipLaunchKernelGGL(k_zyx_to_rows<false>, grid, dim3(256), 0, as_stream(stream), src, dst, C, Z, Y, X, dst_stride, dst_coff);
  COOCC_LAUNCH_CHECK("k_zyx_to_rows");
  return COOCC_OK;
}
