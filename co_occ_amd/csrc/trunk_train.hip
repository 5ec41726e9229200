// Training of the LiDAR-only trunk (SECOND3D + SECOND3DFPN, co_occ_amd/lidar_trunk.py run_trunk_train): what the table-driven
// backward of the conv family (csrc/conv_bwd.hip) did not have yet.
//  * k_tap_table3: the row tables of a convolution with per-axis kernel / stride / padding -- the backbone's 3x3x1 layers with
//    strides (s, s, 1), s up to 4.  Same conventions as k_tap_table (tap t = (dx*ky + dy)*kz + dz, rows in (b, x, y, z) order, -1
//    for padding / "no output reads this voxel through this tap"); for cubic arguments the same table.
//  * k_fpn_sum_bwd: backward of k_fpn_sum (csrc/second_fpn.hip).  d sum / d level = 1, so every level's gradient is dout itself,
//    re-laid into that deblock's child-major rows [B*(X/s)*(Y/s)*Z][s*s][C]: a pure gather-free scatter of whole rows, every fine
//    voxel owning exactly one child slot per level.  dout is read once for all levels.  HBM-bound: (1 + levels written) * rows * C * 4 bytes.
#include <string.h>

#include "common.h"

typedef float f32x4 __attribute__((ext_vector_type(4)));

struct Tap3K {
  int B, Xi, Yi, Zi, Xo, Yo, Zo;
  int kx, ky, kz, sx, sy, sz, px, py, pz;
  int dgrad;
  long long M;
  int32_t* table;
};

__global__ __launch_bounds__(256) void k_tap_table3(Tap3K p) {
  const long long taps = (long long)p.kx * p.ky * p.kz;
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  if (i >= p.M * taps) return;
  const int t = (int)(i / p.M);
  const long long m = i % p.M;
  const int dz = t % p.kz, dy = (t / p.kz) % p.ky, dx = t / (p.kz * p.ky);
  long long r = -1;
  if (!p.dgrad) {
    const int z = (int)(m % p.Zo), y = (int)((m / p.Zo) % p.Yo), x = (int)((m / ((long long)p.Zo * p.Yo)) % p.Xo);
    const long long b = m / ((long long)p.Zo * p.Yo * p.Xo);
    const int ix = x * p.sx - p.px + dx, iy = y * p.sy - p.py + dy, iz = z * p.sz - p.pz + dz;
    if ((unsigned)ix < (unsigned)p.Xi && (unsigned)iy < (unsigned)p.Yi && (unsigned)iz < (unsigned)p.Zi)
      r = ((b * p.Xi + ix) * p.Yi + iy) * p.Zi + iz;
  } else {
    const int z = (int)(m % p.Zi), y = (int)((m / p.Zi) % p.Yi), x = (int)((m / ((long long)p.Zi * p.Yi)) % p.Xi);
    const long long b = m / ((long long)p.Zi * p.Yi * p.Xi);
    const int ox = x + p.px - dx, oy = y + p.py - dy, oz = z + p.pz - dz;
    if (ox >= 0 && oy >= 0 && oz >= 0 && ox % p.sx == 0 && oy % p.sy == 0 && oz % p.sz == 0 && ox / p.sx < p.Xo && oy / p.sy < p.Yo &&
        oz / p.sz < p.Zo)
      r = ((b * p.Xo + ox / p.sx) * p.Yo + oy / p.sy) * p.Zo + oz / p.sz;
  }
  p.table[i] = (int32_t)r;
}

extern "C" int coocc_conv_tap_table3(int B, int Xi, int Yi, int Zi, int Xo, int Yo, int Zo, int kx, int ky, int kz, int sx, int sy, int sz,
                                     int px, int py, int pz, int dgrad, int32_t* table, void* stream) {
  COOCC_CHECK_ARG(table && B > 0 && Xi > 0 && Yi > 0 && Zi > 0 && Xo > 0 && Yo > 0 && Zo > 0, "conv_tap_table3: null table or empty grid");
  COOCC_CHECK_ARG(kx > 0 && ky > 0 && kz > 0 && sx > 0 && sy > 0 && sz > 0 && px >= 0 && py >= 0 && pz >= 0 && kx <= 64 && ky <= 64 && kz <= 64,
                  "conv_tap_table3: kernel extents 1..64, strides >= 1, paddings >= 0 per axis");
  COOCC_CHECK_ARG(Xi + 2 * px >= kx && Yi + 2 * py >= ky && Zi + 2 * pz >= kz && Xo == (Xi + 2 * px - kx) / sx + 1 &&
                      Yo == (Yi + 2 * py - ky) / sy + 1 && Zo == (Zi + 2 * pz - kz) / sz + 1,
                  "conv_tap_table3: output extents (%d,%d,%d) are not (n + 2p - k) / s + 1 of input (%d,%d,%d)", Xo, Yo, Zo, Xi, Yi, Zi);
  Tap3K p;
  memset(&p, 0, sizeof(p));
  p.B = B; p.Xi = Xi; p.Yi = Yi; p.Zi = Zi; p.Xo = Xo; p.Yo = Yo; p.Zo = Zo;
  p.kx = kx; p.ky = ky; p.kz = kz; p.sx = sx; p.sy = sy; p.sz = sz; p.px = px; p.py = py; p.pz = pz;
  p.dgrad = dgrad ? 1 : 0;
  const long long Mi = (long long)B * Xi * Yi * Zi, Mo = (long long)B * Xo * Yo * Zo;
  p.M = dgrad ? Mi : Mo;
  const long long taps = (long long)kx * ky * kz;
  COOCC_CHECK_ARG(p.M * taps < (1ll << 31) && Mi < (1ll << 31) && Mo < (1ll << 31), "conv_tap_table3: too large (32-bit rows)");
  p.table = table;
  hipLaunchKernelGGL(k_tap_table3, dim3(cdiv(p.M * taps, 256)), dim3(256), 0, as_stream(stream), p);
  COOCC_LAUNCH_CHECK("k_tap_table3");
  return COOCC_OK;
}

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
