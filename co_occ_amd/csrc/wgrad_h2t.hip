// Weight gradient of a rule-book (row-table) convolution on the split-f16 engine:
//   dW[n][c][t] = sum_m in[table[t][m]][c] * dacc[m][n]        (table entry -1: the row contributes nothing)
// with both fp32 operands split IN REGISTERS (hi = f16(v), lo = f16((v - hi) 2^11)) and three v_mfma_f32_32x32x16_f16 per product
// (hi hi, hi lo, lo hi), fp32 accumulate -- the arithmetic of csrc/wgrad_h2.hip, whose KH2 operand (8 consecutive rows per 16-byte
// fragment) a gather cannot feed.  The reference trains these layers through spconv v1's fp32 backward (sparse_encoder_hd.py:66-212:
// SubMConv3d / SparseConv3d); csrc/conv_bwd.hip's k_wgrad<true> is the fp32-MFMA form, on 128 x 128 tiles these 32..128-wide layers
// fill to 1/16 .. 1/4.
//
// The reduction index of the MFMA is the output row m.  Lane (r = lane & 31, h = lane >> 5) of a 32x32x16 operand holds 8
// consecutive k of row r: in[table[t][m + 8h + j]][c0 + r] and dacc[m + 8h + j][n0 + r], j = 0..7 -- eight dword buffer loads per
// lane, each two whole 128-byte row segments across the wave (k_wgrad's addressing, 8 voxels deep per lane instead of 1): no LDS, no
// transposition pass.  A row id of -1 (and a row past the slice) is OR-ed into the offset and reads zeros through the descriptor's
// range check.  The row ids of a step are read once per tap and wave, two steps ahead of their MFMAs; the operands one step ahead.
//
// A wave owns 32 input channels x 32 NB outputs for TPW taps: it loads, scales and splits its dacc fragments once per 16-row step
// and reuses them for every tap it owns.  (tap group, channel block, output group) are dealt over the waves of the workgroups of
// grid.x; grid.y cuts the row axis into slices of >= 256 rows.  A tap whose 16 row ids of a step are all -1 (wave-uniform: the ids
// depend on h only) skips its loads, splits and MFMAs.  Partial sums go to slabs [slice][t][Cin][Cout]; conv_bwd.hip's reduce sums
// them in slice order into dw[Cout][Cin][taps].
#include "common.h"
#include "conv_k.h"
#include "h2_rows.h"
#include <algorithm>

typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));
typedef float f32x16 __attribute__((ext_vector_type(16)));

struct WgradH2T {
  const float* in; const float* dacc; const int32_t* table; const float* scale2; float* slabs; int* flag;
  unsigned in_bytes, dacc_bytes, table_bytes;
  int in_stride, dacc_stride, M, Cin, Cout, taps;
  int tgroups, cblocks, items;      // items = tgroups * cblocks * (Cout / (32 NB)): one per wave
  int mslice;                       // rows per slice (a multiple of 16)
};

__device__ __forceinline__ float h2t_load(__amdgpu_buffer_rsrc_t r, unsigned off) {
  return __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(r, (int)off, 0, 0));
}

// the split of 8 values into the hi / lo fragments; amax: running max of |bits| (NaN and inf order above every finite value)
__device__ __forceinline__ void h2t_split8(const float (&v)[8], f16x8& hi, f16x8& lo, unsigned& amax) {
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    _Float16 a, b;
    split_h2(v[j], a, b);
    hi[j] = a; lo[j] = b;
    amax = max(amax, __float_as_uint(v[j]) & 0x7FFFFFFFu);
  }
}

template <int NB, int TPW>
__global__ __launch_bounds__(256, 2) void k_wgrad_h2t(WgradH2T p) {
  const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int r = lane & 31, h = lane >> 5;
  int item = blockIdx.x * 4 + wave;
  if (item >= p.items) return;                              // (no barrier in this kernel)
  const int tg = item % p.tgroups; item /= p.tgroups;
  const int cb = item % p.cblocks; const int ng = item / p.cblocks;
  const int t0 = tg * TPW, c0 = cb * 32, n0 = ng * 32 * NB;
  const int mbeg = blockIdx.y * p.mslice, mend = min(p.M, mbeg + p.mslice);
  __amdgpu_buffer_rsrc_t rs_in = __builtin_amdgcn_make_buffer_rsrc((void*)p.in, 0, p.in_bytes, 0x00020000);
  __amdgpu_buffer_rsrc_t rs_da = __builtin_amdgcn_make_buffer_rsrc((void*)p.dacc, 0, p.dacc_bytes, 0x00020000);
  __amdgpu_buffer_rsrc_t rs_tb = __builtin_amdgcn_make_buffer_rsrc((void*)p.table, 0, p.table_bytes, 0x00020000);
  const float s = p.scale2 ? p.scale2[0] : 1.f, inv = p.scale2 ? p.scale2[1] : 1.f;
  const unsigned ca = (unsigned)(c0 + r) * 4u, nb0 = (unsigned)(n0 + r) * 4u;

  f32x16 hh[TPW][NB], xx[TPW][NB];
#pragma unroll
  for (int u = 0; u < TPW; ++u)
#pragma unroll
    for (int b = 0; b < NB; ++b)
#pragma unroll
      for (int e = 0; e < 16; ++e) { hh[u][b][e] = 0.f; xx[u][b][e] = 0.f; }
  unsigned amax = 0u;

  // three stages: row ids two steps ahead, operands one step ahead of their MFMAs; two statically named operand sets
  int ids[TPW][8];
  float a0[TPW][8], b0[NB][8], a1[TPW][8], b1[NB][8];
  bool live0[TPW], live1[TPW];
  auto load_ids = [&](int m) {
#pragma unroll
    for (int u = 0; u < TPW; ++u) {
      const int t = t0 + u;
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        const int mm = m + 8 * h + j;
        int id = -1;
        if (t < p.taps)                                      // wave-uniform
          id = __builtin_amdgcn_raw_buffer_load_b32(rs_tb, (int)(((unsigned)t * (unsigned)p.M + (unsigned)min(mm, p.M - 1)) * 4u), 0, 0);
        ids[u][j] = id | ((mend - 1 - mm) >> 31);            // -1 past the slice
      }
    }
  };
  auto load_ops = [&](int m, float (&a)[TPW][8], float (&b)[NB][8], bool (&live)[TPW]) {
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const int mm = m + 8 * h + j;
      const unsigned mmask = (unsigned)((mend - 1 - mm) >> 31), rb = (unsigned)mm * (unsigned)p.dacc_stride * 4u;
#pragma unroll
      for (int q = 0; q < NB; ++q) b[q][j] = h2t_load(rs_da, (rb + nb0 + 128u * q) | mmask);
    }
#pragma unroll
    for (int u = 0; u < TPW; ++u) {
      int all = -1;
#pragma unroll
      for (int j = 0; j < 8; ++j) all &= ids[u][j];          // negative iff all eight ids are negative
      live[u] = __builtin_amdgcn_ballot_w64(all >= 0) != 0;  // some lane of the wave holds a live row
      if (live[u]) {
#pragma unroll
        for (int j = 0; j < 8; ++j)
          a[u][j] = h2t_load(rs_in, ((unsigned)ids[u][j] * (unsigned)p.in_stride * 4u + ca) | (unsigned)(ids[u][j] >> 31));
      }
    }
  };
  auto mfmas = [&](const float (&a)[TPW][8], const float (&b)[NB][8], const bool (&live)[TPW]) {
    f16x8 bh[NB], bl[NB];
#pragma unroll
    for (int q = 0; q < NB; ++q) {
      float v[8];
#pragma unroll
      for (int j = 0; j < 8; ++j) v[j] = b[q][j] * s;
      h2t_split8(v, bh[q], bl[q], amax);
    }
#pragma unroll
    for (int u = 0; u < TPW; ++u) {
      if (!live[u]) continue;
      f16x8 ah, al;
      h2t_split8(a[u], ah, al, amax);
#pragma unroll
      for (int q = 0; q < NB; ++q) {
        hh[u][q] = __builtin_amdgcn_mfma_f32_32x32x16_f16(ah, bh[q], hh[u][q], 0, 0, 0);
        xx[u][q] = __builtin_amdgcn_mfma_f32_32x32x16_f16(ah, bl[q], xx[u][q], 0, 0, 0);
        xx[u][q] = __builtin_amdgcn_mfma_f32_32x32x16_f16(al, bh[q], xx[u][q], 0, 0, 0);
      }
    }
  };
  load_ids(mbeg);
  load_ops(mbeg, a0, b0, live0);
  load_ids(mbeg + 16);
  for (int m = mbeg; m < mend; m += 32) {
    load_ops(m + 16, a1, b1, live1);       // uses the row ids fetched one step ago
    load_ids(m + 32);
    mfmas(a0, b0, live0);
    load_ops(m + 32, a0, b0, live0);
    load_ids(m + 48);
    mfmas(a1, b1, live1);                  // past mend: every tap dead, dacc all zeros
  }
  if (p.flag && amax >= __float_as_uint(H2_GUARD)) *(volatile int*)p.flag = 1;      // |v| >= H2_GUARD, inf or NaN
  const float lo = inv * (1.f / H2_LO_SCALE);
#pragma unroll
  for (int u = 0; u < TPW; ++u) {
    const int t = t0 + u;
    if (t >= p.taps) break;
    float* sl = p.slabs + ((size_t)blockIdx.y * p.taps + t) * (size_t)p.Cin * p.Cout;
#pragma unroll
    for (int q = 0; q < NB; ++q)
#pragma unroll
      for (int e = 0; e < 16; ++e) {
        const int c = c0 + (e & 3) + 8 * (e >> 2) + 4 * h, n = n0 + q * 32 + r;
        sl[(size_t)c * p.Cout + n] = hh[u][q][e] * inv + xx[u][q][e] * lo;
      }
  }
}

// reduce kernels of conv_bwd.hip (same slab layout)
int coocc_wgrad_reduce_launch(const float* slabs, int nslices, int Cin, int Cout, int taps, float* dw, int accumulate, hipStream_t s);

template <int NB, int TPW>
static void launch_h2t(WgradH2T& p, int nslices, hipStream_t s) {
  p.tgroups = (p.taps + TPW - 1) / TPW;
  p.cblocks = p.Cin / 32;
  p.items = p.tgroups * p.cblocks * (p.Cout / (32 * NB));
  hipLaunchKernelGGL((k_wgrad_h2t<NB, TPW>), dim3(cdiv(p.items, 4), (unsigned)nslices), dim3(256), 0, s, p);
}

// waves per slice of the form the widths select: Cout % 64 == 0 -> 64 outputs x 2 taps per wave, else 32 outputs x 3 taps
static long long h2t_items(int Cin, int Cout, int taps) {
  return Cout % 64 == 0 ? (long long)((taps + 1) / 2) * (Cin / 32) * (Cout / 64) : (long long)((taps + 2) / 3) * (Cin / 32) * (Cout / 32);
}

extern "C" int coocc_conv_wgrad_h2t(const float* in, int in_rows, int in_stride, const float* dacc, int dacc_stride,
                                    const int32_t* table, int M, int Cin, int Cout, int taps, const float* scale2, float* dw,
                                    int accumulate, float* ws, int64_t ws_floats, void* stream) {
  COOCC_CHECK_ARG(in && dacc && dw && ws, "conv_wgrad_h2t: null pointer");
  COOCC_CHECK_ARG(table, "conv_wgrad_h2t: the row table is required (identity rows: coocc_conv_wgrad_h2)");
  COOCC_CHECK_ARG(M > 0 && in_rows > 0 && taps > 0, "conv_wgrad_h2t: M, in_rows and taps must be positive");
  COOCC_CHECK_ARG(Cin > 0 && Cout > 0 && Cin % 32 == 0 && Cout % 32 == 0, "conv_wgrad_h2t: Cin and Cout must be multiples of 32");
  COOCC_CHECK_ARG(in_stride >= Cin && dacc_stride >= Cout, "conv_wgrad_h2t: row strides below the channel counts");
  const int64_t per = (int64_t)taps * Cin * Cout;
  COOCC_CHECK_ARG(ws_floats >= per, "conv_wgrad_h2t: workspace smaller than one weight slab set (taps * Cin * Cout floats)");
  const unsigned long long in_bytes = (unsigned long long)in_rows * in_stride * 4ull, da_bytes = (unsigned long long)M * dacc_stride * 4ull,
                           tb_bytes = (unsigned long long)taps * M * 4ull;
  COOCC_CHECK_ARG(in_bytes < 0xFFFFFF00ull && da_bytes < 0xFFFFFF00ull && tb_bytes < 0xFFFFFF00ull,
                  "conv_wgrad_h2t: operand larger than 4 GB");
  int* flag = nullptr;
  if (coocc_h2_flag_ptr(&flag) != COOCC_OK) return COOCC_EHIP;
  // slices of the row axis: ~2 workgroups per CU over the chip, >= 256 rows each, within the workspace
  const long long wgs = (h2t_items(Cin, Cout, taps) + 3) / 4;
  long long nslices = (512 + wgs - 1) / wgs;
  nslices = std::min<long long>(nslices, (M + 255) / 256);
  nslices = std::min<long long>(nslices, ws_floats / per);
  nslices = std::min<long long>(nslices, 4096);
  int mslice = (int)((M + nslices - 1) / nslices);
  mslice = (mslice + 15) / 16 * 16;
  nslices = (M + mslice - 1) / mslice;
  WgradH2T p;
  p.in = in; p.dacc = dacc; p.table = table; p.scale2 = scale2; p.slabs = ws; p.flag = flag;
  p.in_bytes = (unsigned)in_bytes; p.dacc_bytes = (unsigned)da_bytes; p.table_bytes = (unsigned)tb_bytes;
  p.in_stride = in_stride; p.dacc_stride = dacc_stride; p.M = M; p.Cin = Cin; p.Cout = Cout; p.taps = taps; p.mslice = mslice;
  hipStream_t s = as_stream(stream);
  if (Cout % 64 == 0) launch_h2t<2, 2>(p, (int)nslices, s);
  else launch_h2t<1, 3>(p, (int)nslices, s);
  COOCC_LAUNCH_CHECK("k_wgrad_h2t");
  return coocc_wgrad_reduce_launch(ws, (int)nslices, Cin, Cout, taps, dw, accumulate, s);
}
