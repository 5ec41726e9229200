// Training of SparseEncoderHD (co_occ_amd/lidar_hd.py, the train() forward): what the inference rule books (csrc/lidar.hip) and the
// batch-statistics BatchNorm of the dense training path (csrc/backward.hip) did not have yet.
//  * k_sp_dgrad_table3: the TRANSPOSED rule book of a per-axis SparseConv3d(kernel, stride, pad), straight from geometry: for input
//    row i at (z, y, x) and tap t = (kd*ky + kh)*kx + kw the output coordinate is (c + p - k) / s per axis (divisible, in range),
//    looked up in the OUTPUT level's index map.  One thread per (tap, input row), rows fastest: coalesced 4-byte stores, every entry
//    written exactly once (no atomic, no fill pass).  The thread of tap 0 also writes the row's residue class
//    ((z+pz) % sz * sy + (y+py) % sy) * sx + (x+px) % sx -- the taps that can reach a row depend on its class alone (k = class mod s
//    per axis), so a strided dgrad can run as one small row-table GEMM per class (COOCC_HD_DGRAD_CLASSES=1; autograd.dgrad_classes does
//    the same on dense grids).
//    HBM-bound: Mi * 12 bytes of coordinates (re-read per tap from cache), taps * Mi index-map words read (4 bytes each, scattered:
//    up to a 64-byte sector apiece), taps * Mi * 4 + Mi * 4 bytes written.
//  * k_bn_apply_ex: coocc_bn_apply (y = relu((x - mean) * rstd * gamma + beta (+ res)), the same expression, the same bits) whose
//    pass also writes the split-f16 twin of y through store_h2 / h2_guard (csrc/h2_rows.h), so a BN output feeds the next rule-book
//    GEMM without a coocc_rows_to_h2 launch.  One thread per 4 channels, 16-byte accesses.  HBM-bound: M * C * 4 bytes read
//    (+ M * C * 4 with a residual), M * C * 4 written (+ M * C * 4 with the twin; a separate conversion pass reads and writes
//    another M * C * 4 each).
// Both are COOCC_SCALAR_FP32: they run next to the split-f16 GEMMs of the same training step.
#include "common.h"
#include "h2_rows.h"

int coocc_h2_flag_ptr(int** out);      // gemm_h2.hip: the host-mapped range-guard flag of the 16-bit operand writers

struct SpDgradK {
  const int32_t* coors;    // [Mi][3] (z, y, x) of the input level
  const int32_t* out_map;  // [Do*Ho*Wo] index map of the output level (-1 = inactive)
  int32_t* table;          // [taps][Mi]
  int32_t* classes;        // [Mi] or NULL
  long long Mi;
  int Di, Hi, Wi, Do, Ho, Wo;
  int kz, ky, kx, sz, sy, sx, pz, py, px;
};

__global__ __launch_bounds__(256) COOCC_SCALAR_FP32 void k_sp_dgrad_table3(SpDgradK p) {
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  const int taps = p.kz * p.ky * p.kx;
  if (i >= p.Mi * taps) return;
  const int t = (int)(i / p.Mi);
  const size_t m = (size_t)(i % p.Mi);
  const int kw = t % p.kx, kh = (t / p.kx) % p.ky, kd = t / (p.kx * p.ky);
  const int cz = p.coors[m * 3], cy = p.coors[m * 3 + 1], cx = p.coors[m * 3 + 2];
  const bool inside = (unsigned)cz < (unsigned)p.Di && (unsigned)cy < (unsigned)p.Hi && (unsigned)cx < (unsigned)p.Wi;
  int r = -1;
  if (inside) {       // (a row that is no voxel of this grid reaches nothing)
    const int z = cz + p.pz - kd, y = cy + p.py - kh, x = cx + p.px - kw;
    if (z >= 0 && y >= 0 && x >= 0 && z % p.sz == 0 && y % p.sy == 0 && x % p.sx == 0) {
      const int oz = z / p.sz, oy = y / p.sy, ox = x / p.sx;
      if (oz < p.Do && oy < p.Ho && ox < p.Wo) r = p.out_map[((size_t)oz * p.Ho + oy) * p.Wo + ox];
    }
  }
  p.table[i] = r;
  if (t == 0 && p.classes)
    p.classes[m] = inside ? (((cz + p.pz) % p.sz) * p.sy + (cy + p.py) % p.sy) * p.sx + (cx + p.px) % p.sx : 0;
}

extern "C" int coocc_sparse_dgrad_table3(const int32_t* in_coors, int Mi, int Di, int Hi, int Wi, int kz, int ky, int kx, int sz, int sy,
                                         int sx, int pz, int py, int px, int Do, int Ho, int Wo, const int32_t* out_map, int32_t* table,
                                         int32_t* classes, void* stream) {
  COOCC_CHECK_ARG(Mi >= 0 && out_map && ((in_coors && table) || Mi == 0), "sparse_dgrad_table3: bad args (null pointer or negative row count)");
  COOCC_CHECK_ARG(kz > 0 && ky > 0 && kx > 0 && kz <= 7 && ky <= 7 && kx <= 7 && sz > 0 && sy > 0 && sx > 0 && sz <= 64 && sy <= 64 &&
                      sx <= 64 && pz >= 0 && py >= 0 && px >= 0 && pz <= 64 && py <= 64 && px <= 64,
                  "sparse_dgrad_table3: kernel (%d,%d,%d) / stride (%d,%d,%d) / padding (%d,%d,%d): extents 1..7, strides 1..64, "
                  "paddings 0..64 per axis", kz, ky, kx, sz, sy, sx, pz, py, px);
  COOCC_CHECK_ARG(Di > 0 && Hi > 0 && Wi > 0 && (long long)Di * Hi * Wi <= 0x7FFFFFFFll,
                  "sparse_dgrad_table3: input grid %d x %d x %d: extents must be positive and the grid at most 2^31 - 1 cells", Di, Hi, Wi);
  // the index map is addressed with these extents, so they are checked against ops.py get_conv_output_size, not trusted
  COOCC_CHECK_ARG(Di + 2 * pz >= kz && Hi + 2 * py >= ky && Wi + 2 * px >= kx && Do == (Di + 2 * pz - kz) / sz + 1 &&
                      Ho == (Hi + 2 * py - ky) / sy + 1 && Wo == (Wi + 2 * px - kx) / sx + 1,
                  "sparse_dgrad_table3: output grid %d x %d x %d is not (in + 2 p - k) / s + 1 per axis of %d x %d x %d", Do, Ho, Wo, Di, Hi,
                  Wi);
  COOCC_CHECK_ARG((long long)Do * Ho * Wo <= 0x7FFFFFFFll, "sparse_dgrad_table3: output grid %d x %d x %d exceeds 2^31 - 1 cells", Do, Ho, Wo);
  const long long n = (long long)Mi * kz * ky * kx;
  COOCC_CHECK_ARG((n + 255) / 256 <= 0x7FFFFFFFll, "sparse_dgrad_table3: %lld table entries exceed one launch (2^31 - 1 blocks of 256)", n);
  if (Mi == 0) return COOCC_OK;
  SpDgradK p;
  p.coors = in_coors; p.out_map = out_map; p.table = table; p.classes = classes; p.Mi = Mi;
  p.Di = Di; p.Hi = Hi; p.Wi = Wi; p.Do = Do; p.Ho = Ho; p.Wo = Wo;
  p.kz = kz; p.ky = ky; p.kx = kx; p.sz = sz; p.sy = sy; p.sx = sx; p.pz = pz; p.py = py; p.px = px;
  hipLaunchKernelGGL(k_sp_dgrad_table3, dim3((unsigned)cdiv(n, 256)), dim3(256), 0, as_stream(stream), p);
  COOCC_LAUNCH_CHECK("k_sp_dgrad_table3");
  return COOCC_OK;
}

// the expression of k_bn_apply (csrc/backward.hip), operation for operation
__device__ __forceinline__ float bn_apply1(float x, float mean, float var, float gamma, float beta, float eps) {
  return (x - mean) * (1.f / sqrtf(var + eps)) * gamma + beta;
}

__global__ __launch_bounds__(256) COOCC_SCALAR_FP32 void k_bn_apply_ex(const float* __restrict__ x, long long M, int C,
                                                                        const float* __restrict__ mean, const float* __restrict__ var,
                                                                        const float* __restrict__ gamma, const float* __restrict__ beta,
                                                                        float eps, const float* __restrict__ res, int relu,
                                                                        float* __restrict__ y, void* __restrict__ out_h2,
                                                                        int* __restrict__ flag) {
  const int c4 = C >> 2;
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  if (i >= M * c4) return;
  const long long m = i / c4;
  const int c = (int)(i - m * c4) * 4;
  const f32x4 xv = *(const f32x4*)(x + m * C + c);
  const f32x4 mu = *(const f32x4*)(mean + c), va = *(const f32x4*)(var + c), g = *(const f32x4*)(gamma + c), b = *(const f32x4*)(beta + c);
  f32x4 v;
#pragma unroll
  for (int e = 0; e < 4; ++e) v[e] = bn_apply1(xv[e], mu[e], va[e], g[e], b[e], eps);
  if (res) {
    const f32x4 rv = *(const f32x4*)(res + m * C + c);
#pragma unroll
    for (int e = 0; e < 4; ++e) v[e] += rv[e];
  }
  if (relu) {
#pragma unroll
    for (int e = 0; e < 4; ++e) v[e] = fmaxf(v[e], 0.f);
  }
  *(f32x4*)(y + m * C + c) = v;
  if (out_h2) {
    store_h2(out_h2, (size_t)m, C, c, v);
    h2_guard(flag, v);
  }
}

extern "C" int coocc_bn_apply_ex(const float* x, int M, int C, const float* mean, const float* var, const float* gamma, const float* beta,
                                 float eps, const float* res, int relu, float* y, void* out_h2, void* stream) {
  COOCC_CHECK_ARG(x && mean && var && gamma && beta && y && M > 0 && C > 0, "bn_apply_ex: bad args");
  COOCC_CHECK_ARG(C % 4 == 0 && (((uintptr_t)x | (uintptr_t)y | (uintptr_t)res | (uintptr_t)mean | (uintptr_t)var | (uintptr_t)gamma |
                                  (uintptr_t)beta) & 15) == 0,
                  "bn_apply_ex: C %% 4 == 0 and 16-byte aligned pointers (rows of whole dwordx4)");
  COOCC_CHECK_ARG(!out_h2 || (C % 32 == 0 && ((uintptr_t)out_h2 & 15) == 0), "bn_apply_ex: the split-f16 twin needs C %% 32 == 0 and a 16-byte "
                  "aligned pointer");
  int* flag = nullptr;
  if (out_h2 && coocc_h2_flag_ptr(&flag) != COOCC_OK) return COOCC_EHIP;
  const long long n = (long long)M * (C / 4);
  hipLaunchKernelGGL(k_bn_apply_ex, dim3(cdiv(n, 256)), dim3(256), 0, as_stream(stream), x, (long long)M, C, mean, var, gamma, beta, eps, res,
                     relu, y, out_h2, flag);
  COOCC_LAUNCH_CHECK("k_bn_apply_ex");
  return COOCC_OK;
}
