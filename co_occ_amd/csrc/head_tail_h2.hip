// The two two-layer pointwise chains at the end of OccHead.forward_coarse_rows (occ_head.py:149-171, :182), ONE launch each, on
// the split-f16 engine of gemm_h2.hip.
//
// k_head_pred_h2:
//   hq     = [ relu(bn(W_p0 x)) | Q = W_f0[:, :128] x ]        128 -> 128 (the merged occ_pred_conv[0] + fine_mlp[0] pack)
//   logits = W_p1 hq[:, :64] + b                                64 -> ncls (occ_pred_conv[3])
//   flag   = argmax(logits) != empty_idx                        (the fine branch's foreground test)
// Layer by layer this was four launches (k_gemm_h2p<4>, k_rows_to_h2, k_gemm_h2w, k_argmax_flags; 76 us at 80 000 rows): the 64
// hidden channels went to HBM as fp32, came back, went out again as H2 rows and came back again, the 17-column second layer ran
// on a 128-column tile, and the logits were read once more for one byte per voxel.  Here a workgroup owns 128 rows from the H2
// rows of x to the finished logits:
//   * the A tile (4 chunks x 128 rows x 128 B = 64 KB) is staged once by global_load_lds with k_gemm_h2p's source-side swizzle,
//     the weights of all chunks are loaded once, and layer 1 runs k_gemm_h2p<4>'s MFMA sequence (chunk order, P0 / P1 / P2 order,
//     alpha / lo combination, scale / bias / ReLU expressions): every value is the one that kernel produces;
//   * Q (columns 64-127) goes to HBM as fp32 in the [V, 128] layout k_fine2_h2 reads; the hidden columns 0-63 go to HBM only
//     when the caller asks, and always into LDS as H2 rows (split_h2: what k_rows_to_h2 writes), over chunks 0-1 of the tile;
//   * layer 2 is ONE 32-column tile: wave w takes rows 32 w .. 32 w + 31, the two chunks and their k16 steps in k_gemm_h2w's order,
//     so a logit sees the MFMA sequence it sees there;
//   * the logits pass through 17 KB of LDS: written to HBM as whole contiguous runs instead of 4-byte pieces, and scanned per
//     row in k_argmax_flags's comparison order for the flag.
//
// k_head_soft_h2:
//   wlogit = W_s1 relu(bn(W_s0 x)) + b                          128 -> 64 -> L (voxel_soft_weights)
// Two launches before (k_gemm_h2p<4>, then the fp32-MFMA k_conv<128,32,32,32> on the fp32 hidden rows; 46 us).  Layer 1 as above
// with two row blocks per wave (the 64 real columns only); the hidden activation stays in LDS as FP32 rows and layer 2 runs
// k_conv's v_mfma_f32_32x32x2_f32 sequence on it (k = 32 chunk + 8 q + 4 h + s, chunks, q and s ascending), weights straight from
// the fp32 fragment-major pack.
//
// 64 KB of LDS and <= 256 registers each: two workgroups per CU.
#include <string.h>

#include "conv_k.h"
#include "h2_rows.h"

typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));

#define HT_BM 128
#define HT_STAGE (HT_BM * 128)
#define HT_LST 33              // floats per row of the output tile in LDS (odd: the per-row scan is conflict-free)
#define HT_HST 68              // floats per row of the fp32 hidden activation in LDS (272 B: 16-byte aligned, rows 4 banks apart)
#define HT_SOFT_OUT 36864      // byte offset of k_head_soft_h2's output tile: behind the 128 x 68 floats of the hidden activation

struct HeadTailK {
  const char* x; long long rowbytes;                 // H2 rows [M][in_stride]
  int M; const int32_t* M_dev;
  const char* w1; const float* scale1; const float* bias1;      // layer 1: H2 pack (columns padded to 128), folded BN
  float* hq; int hq_stride; int write_hidden;        // pred: [M][>= 128] = hidden | Q; soft: [M][>= 64] hidden, on request
  const char* w2; const float* bias2; int nout;      // layer 2: pred H2 pack / soft fp32 pack, bias or NULL, ncls / L
  float* out; int out_stride;                        // logits / wlogit
  int empty_idx; uint8_t* flags;
  float alpha;
  int* h2_flag;
  const char* zrow;
};

__device__ __forceinline__ void ht_glds16(const void* g, void* l) {
  __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)g, (__attribute__((address_space(3))) void*)l, 16, 0, 0);
}

// the whole A tile: chunk c of row r = (4 j + wave) 8 + srow -> stage c, lane-linear (the swizzle sits on the source address)
__device__ __forceinline__ void ht_stage_tile(const HeadTailK& p, char* As, int m0, int wave, int lane) {
  const int srow = lane >> 3, slot = lane & 7;
  const unsigned aq = (unsigned)((slot ^ ((4 * (wave & 1) + (srow >> 1)) & 7)) * 16);
#pragma unroll
  for (int c = 0; c < 4; ++c)
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int m = m0 + (j * 4 + wave) * 8 + srow;
      const char* src = m < p.M ? p.x + ((long long)m * p.rowbytes + c * 128 + aq) : p.zrow;
      ht_glds16(src, &As[c * HT_STAGE + (j * 4 + wave) * 8 * 128]);
    }
}

// layer 1 on column tile `ctile` and the TM row blocks rb0 .. rb0 + TM - 1: k_gemm_h2p<4>'s sequence per accumulator
template <int TM>
__device__ __forceinline__ void ht_layer1(const HeadTailK& p, const char* As, int ctile, int rb0, int lane, const unsigned (&fragoff)[4],
                                          f32x16 (&hh)[TM], f32x16 (&xx)[TM]) {
  f16x8 breg[4][2][2];                   // [chunk][k16 step][plane]
  const char* wcur = p.w1 + (long long)ctile * 4096 + lane * 16;
#pragma unroll
  for (int c = 0; c < 4; ++c)
#pragma unroll
    for (int s2 = 0; s2 < 2; ++s2)
#pragma unroll
      for (int pl = 0; pl < 2; ++pl) breg[c][s2][pl] = *(const f16x8*)(wcur + c * 16384 + (s2 * 2 + pl) * 1024);
#pragma unroll
  for (int i = 0; i < TM; ++i)
#pragma unroll
    for (int r = 0; r < 16; ++r) { hh[i][r] = 0.f; xx[i][r] = 0.f; }
  __syncthreads();                       // (carries vmcnt(0): the tile has landed)
#pragma unroll
  for (int c = 0; c < 4; ++c) {
#pragma unroll
    for (int s2 = 0; s2 < 2; ++s2) {
      f16x8 fhi[TM], flo[TM];
#pragma unroll
      for (int i = 0; i < TM; ++i) {
        fhi[i] = *(const f16x8*)&As[fragoff[2 * s2 + 0] + (c * HT_STAGE + (rb0 + i) * 4096)];
        flo[i] = *(const f16x8*)&As[fragoff[2 * s2 + 1] + (c * HT_STAGE + (rb0 + i) * 4096)];
      }
#pragma unroll
      for (int i = 0; i < TM; ++i) hh[i] = __builtin_amdgcn_mfma_f32_32x32x16_f16(breg[c][s2][0], fhi[i], hh[i], 0, 0, 0);
#pragma unroll
      for (int i = 0; i < TM; ++i) xx[i] = __builtin_amdgcn_mfma_f32_32x32x16_f16(breg[c][s2][1], fhi[i], xx[i], 0, 0, 0);
#pragma unroll
      for (int i = 0; i < TM; ++i) xx[i] = __builtin_amdgcn_mfma_f32_32x32x16_f16(breg[c][s2][0], flo[i], xx[i], 0, 0, 0);
      __builtin_amdgcn_sched_barrier(0);
    }
  }
  __syncthreads();                       // every wave has read the tile for the last time: its LDS is free
}

// the GEMM epilogue of gemm_h2.hip up to the ReLU: channels n .. n + 3 of accumulator quad j
__device__ __forceinline__ f32x4 ht_epi1(const HeadTailK& p, const f32x16& hh, const f32x16& xx, int j, int n, float alpha, float lo, bool relu) {
  f32x4 v;
#pragma unroll
  for (int e = 0; e < 4; ++e) v[e] = hh[4 * j + e] * alpha + xx[4 * j + e] * lo;
  if (p.scale1) v = v * *(const f32x4*)(p.scale1 + n);
  if (p.bias1) v = v + *(const f32x4*)(p.bias1 + n);
  if (relu) { v[0] = fmaxf(v[0], 0.f); v[1] = fmaxf(v[1], 0.f); v[2] = fmaxf(v[2], 0.f); v[3] = fmaxf(v[3], 0.f); }
  return v;
}

// the finished [rows][nout] tile in LDS (row stride HT_LST) -> HBM, whole runs per wave instruction
__device__ __forceinline__ void ht_store_tile(const HeadTailK& p, const float* Ls, int m0, int nrows, int tid) {
  const int nout = p.nout;
  for (int idx = tid; idx < nrows * nout; idx += 256) {
    const int r = idx / nout, c = idx - r * nout;
    p.out[(size_t)(m0 + r) * p.out_stride + c] = Ls[r * HT_LST + c];
  }
}

__global__ __launch_bounds__(256, 2) void k_head_pred_h2(HeadTailK p) {
  constexpr int TM = 4;
  __shared__ __attribute__((aligned(16))) char As[4 * HT_STAGE];
  const int m0 = blockIdx.x * HT_BM;
  if (p.M_dev) {                         // row count on the device (grid sized for the capacity p.M): whole tiles past it leave
    p.M = min(p.M, *p.M_dev);
    if (m0 >= p.M) return;
  }
  const int tid = threadIdx.x;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6), lane = tid & 63;
  const int li = lane & 31, h = lane >> 5;
  ht_stage_tile(p, As, m0, wave, lane);
  unsigned fragoff[4];
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    const int sl = (q & 1) * 4 + 2 * (q >> 1) + h;                                     // q = 2 s + plane
    fragoff[q] = li * 128 + ((sl ^ ((li >> 1) & 7)) << 4);
  }
  const float alpha = p.alpha, lo = alpha * (1.f / H2_LO_SCALE);
  const unsigned swz = (unsigned)((li >> 1) & 7);
  {
    f32x16 hh[TM], xx[TM];
    ht_layer1<TM>(p, As, wave, 0, lane, fragoff, hh, xx);
    // lane (li, h) holds, for row m0 + 32 i + li, the columns 32 wave + 8 j + 4 h + 0..3 (j = 0..3)
    const int nb = wave * 32 + 4 * h;
    const bool hidden = wave < 2;          // columns 0-63: relu(bn(.)), the operand of layer 2; 64-127: Q
#pragma unroll
    for (int i = 0; i < TM; ++i) {
      const int m = m0 + i * 32 + li;
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const int n = nb + 8 * j;
        const f32x4 v = ht_epi1(p, hh[i], xx[i], j, n, alpha, lo, hidden);
        if (hidden) {
          f16x4 vh, vl;
#pragma unroll
          for (int e = 0; e < 4; ++e) {
            _Float16 a, b;
            split_h2(v[e], a, b);
            vh[e] = a; vl[e] = b;
          }
          // H2 row in LDS: chunk = wave, row 32 i + li, channel 8 j + 4 h + e -> hi at slot j, lo at slot 4 + j, 8 h bytes in
          const unsigned base = (unsigned)wave * HT_STAGE + (unsigned)(i * 32 + li) * 128 + 8 * h;
          *(f16x4*)&As[base + (((unsigned)j ^ swz) << 4)] = vh;
          *(f16x4*)&As[base + (((unsigned)(4 + j) ^ swz) << 4)] = vl;
          if (m < p.M) h2_guard(p.h2_flag, v);
        }
        if (m < p.M && (!hidden || p.write_hidden)) *(f32x4*)(p.hq + (size_t)m * p.hq_stride + n) = v;
      }
    }
  }
  // ---- layer 2: rows 32 wave .. 32 wave + 31 x 32 columns, K = 64
  f16x8 b2[2][2][2];
  {
    const char* wcur = p.w2 + lane * 16;   // column tile 0 of a pack padded to 128 columns: 16 KB per chunk
#pragma unroll
    for (int c = 0; c < 2; ++c)
#pragma unroll
      for (int s2 = 0; s2 < 2; ++s2)
#pragma unroll
        for (int pl = 0; pl < 2; ++pl) b2[c][s2][pl] = *(const f16x8*)(wcur + c * 16384 + (s2 * 2 + pl) * 1024);
  }
  f32x16 hh2, xx2;
#pragma unroll
  for (int r = 0; r < 16; ++r) { hh2[r] = 0.f; xx2[r] = 0.f; }
  __syncthreads();                         // the hidden activation is in LDS
#pragma unroll
  for (int c = 0; c < 2; ++c)
#pragma unroll
    for (int s2 = 0; s2 < 2; ++s2) {
      const f16x8 fhi = *(const f16x8*)&As[fragoff[2 * s2 + 0] + (c * HT_STAGE + wave * 4096)];
      const f16x8 flo = *(const f16x8*)&As[fragoff[2 * s2 + 1] + (c * HT_STAGE + wave * 4096)];
      hh2 = __builtin_amdgcn_mfma_f32_32x32x16_f16(b2[c][s2][0], fhi, hh2, 0, 0, 0);
      xx2 = __builtin_amdgcn_mfma_f32_32x32x16_f16(b2[c][s2][1], fhi, xx2, 0, 0, 0);
      xx2 = __builtin_amdgcn_mfma_f32_32x32x16_f16(b2[c][s2][0], flo, xx2, 0, 0, 0);
    }
  // logits of row 32 wave + li, columns 8 j + 4 h + e -> the LDS tile (over chunk 2: nobody reads it any more)
  float* Ls = (float*)&As[2 * HT_STAGE];
#pragma unroll
  for (int j = 0; j < 4; ++j)
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const int n = 8 * j + 4 * h + e;
      float v = hh2[4 * j + e] * alpha + xx2[4 * j + e] * lo;
      if (n < p.nout) {
        if (p.bias2) v += p.bias2[n];
        Ls[(wave * 32 + li) * HT_LST + n] = v;
      }
    }
  __syncthreads();
  const int nrows = min(HT_BM, p.M - m0);
  ht_store_tile(p, Ls, m0, nrows, tid);
  if (p.flags && tid < nrows) {            // k_argmax_flags: the first maximum wins, comparisons in class order
    const float* r = Ls + tid * HT_LST;
    float best = r[0];
    int bi = 0;
    for (int c = 1; c < p.nout; ++c)
      if (r[c] > best) { best = r[c]; bi = c; }
    p.flags[m0 + tid] = bi != p.empty_idx;
  }
}

__global__ __launch_bounds__(256, 2) void k_head_soft_h2(HeadTailK p) {
  constexpr int TM = 2;
  __shared__ __attribute__((aligned(16))) char As[4 * HT_STAGE];
  const int m0 = blockIdx.x * HT_BM;
  if (p.M_dev) {
    p.M = min(p.M, *p.M_dev);
    if (m0 >= p.M) return;
  }
  const int tid = threadIdx.x;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6), lane = tid & 63;
  const int li = lane & 31, h = lane >> 5;
  ht_stage_tile(p, As, m0, wave, lane);
  unsigned fragoff[4];
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    const int sl = (q & 1) * 4 + 2 * (q >> 1) + h;
    fragoff[q] = li * 128 + ((sl ^ ((li >> 1) & 7)) << 4);
  }
  float* Hs = (float*)As;
  {
    // wave w: column tile w & 1 (the 64 real columns), row blocks 2 (w >> 1), 2 (w >> 1) + 1
    const int ctile = wave & 1, rb0 = 2 * (wave >> 1);
    const float alpha = p.alpha, lo = alpha * (1.f / H2_LO_SCALE);
    f32x16 hh[TM], xx[TM];
    ht_layer1<TM>(p, As, ctile, rb0, lane, fragoff, hh, xx);
    const int nb = ctile * 32 + 4 * h;
#pragma unroll
    for (int i = 0; i < TM; ++i) {
      const int row = (rb0 + i) * 32 + li, m = m0 + row;
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const int n = nb + 8 * j;
        const f32x4 v = ht_epi1(p, hh[i], xx[i], j, n, alpha, lo, true);
        *(f32x4*)&Hs[row * HT_HST + n] = v;
        if (p.write_hidden && m < p.M) *(f32x4*)(p.hq + (size_t)m * p.hq_stride + n) = v;
      }
    }
  }
  // ---- layer 2 (fp32 MFMA, k_conv<128,32,32,32>): wave w on rows 32 w .. 32 w + 31, 32 columns, K = 64
  // weights: fragment-major fp32 pack, column group 0 / wave slot 0 of chunk c: [q][lane][4] = W[n = li][32 c + 8 q + 4 h + 0..3]
  f32x4 wb[2][4];
#pragma unroll
  for (int c = 0; c < 2; ++c)
#pragma unroll
    for (int q = 0; q < 4; ++q) wb[c][q] = *(const f32x4*)((const float*)p.w2 + c * 4096 + q * 256 + lane * 4);
  f32x16 acc;
#pragma unroll
  for (int r = 0; r < 16; ++r) acc[r] = 0.f;
  __syncthreads();                         // the hidden activation is in LDS
#pragma unroll
  for (int c = 0; c < 2; ++c)
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const f32x4 a = *(const f32x4*)&Hs[(wave * 32 + li) * HT_HST + c * 32 + q * 8 + h * 4];
#pragma unroll
      for (int s = 0; s < 4; ++s) acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a[s], wb[c][q][s], acc, 0, 0, 0);
    }
  // D: row = (r & 3) + 8 (r >> 2) + 4 h of this wave's block, column li
  float* Ls = (float*)&As[HT_SOFT_OUT];
  if (li < p.nout) {
    const float b = p.bias2 ? p.bias2[li] : 0.f;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      float v = acc[r];
      if (p.bias2) v += b;
      Ls[(wave * 32 + (r & 3) + 8 * (r >> 2) + 4 * h) * HT_LST + li] = v;
    }
  }
  __syncthreads();
  ht_store_tile(p, Ls, m0, min(HT_BM, p.M - m0), tid);
}

static int ht_fill(HeadTailK& k, const char* who, const void* x_h2, int in_stride, int rows, const int32_t* rows_dev, const void* w1_pack,
                   const float* scale1, const float* bias1, float* hidden, int hidden_stride, int hidden_min, const void* w2_pack,
                   const float* bias2, int nout, float* out, int out_stride) {
  COOCC_CHECK_ARG(x_h2 && w1_pack && w2_pack && out, "%s: null pointer", who);
  COOCC_CHECK_ARG(rows >= 0 && in_stride >= 128 && in_stride % 32 == 0, "%s: 128-channel H2 rows (in_stride >= 128, a multiple of 32)", who);
  COOCC_CHECK_ARG(nout >= 1 && nout <= 32 && out_stride >= nout, "%s: 1 .. 32 output columns, out_stride >= columns", who);
  COOCC_CHECK_ARG(!hidden || (hidden_stride >= hidden_min && hidden_stride % 4 == 0), "%s: hidden row stride (>= %d floats, a multiple of 4)", who, hidden_min);
  COOCC_CHECK_ARG(((uintptr_t)x_h2 & 15) == 0 && ((uintptr_t)hidden & 15) == 0 && ((uintptr_t)w1_pack & 15) == 0 && ((uintptr_t)w2_pack & 15) == 0 &&
                      ((uintptr_t)scale1 & 15) == 0 && ((uintptr_t)bias1 & 15) == 0 && ((uintptr_t)out & 3) == 0,
                  "%s: pointers must be 16-byte aligned", who);
  memset(&k, 0, sizeof(k));
  k.x = (const char*)x_h2; k.rowbytes = (long long)in_stride * 4;
  k.M = rows; k.M_dev = rows_dev;
  k.w1 = (const char*)w1_pack; k.scale1 = scale1; k.bias1 = bias1;
  k.hq = hidden; k.hq_stride = hidden_stride;
  k.w2 = (const char*)w2_pack; k.bias2 = bias2; k.nout = nout;
  k.out = out; k.out_stride = out_stride;
  k.alpha = 1.f;
  const void* z = nullptr;
  int rc = coocc_zero_row(&z);
  if (rc != COOCC_OK) return rc;
  k.zrow = (const char*)z;
  return coocc_h2_flag_ptr(&k.h2_flag);
}

extern "C" int coocc_head_pred_h2(const void* x_h2, int in_stride, int rows, const int32_t* rows_dev, const void* w1_pack,
                                  const float* scale1, const float* bias1, float* hq, int hq_stride, int write_hidden,
                                  const void* w2_pack, const float* bias2, int ncls, float* logits, int logit_stride,
                                  int empty_idx, uint8_t* flags, void* stream) {
  COOCC_CHECK_ARG(hq, "head_pred_h2: null pointer");
  HeadTailK k;
  const int rc = ht_fill(k, "head_pred_h2", x_h2, in_stride, rows, rows_dev, w1_pack, scale1, bias1, hq, hq_stride, 128, w2_pack, bias2, ncls,
                         logits, logit_stride);
  if (rc != COOCC_OK) return rc;
  if (rows == 0) return COOCC_OK;
  k.write_hidden = write_hidden;
  k.empty_idx = empty_idx; k.flags = flags;
  hipLaunchKernelGGL(k_head_pred_h2, dim3(cdiv(rows, HT_BM)), dim3(256), 0, as_stream(stream), k);
  COOCC_LAUNCH_CHECK("k_head_pred_h2");
  return COOCC_OK;
}

extern "C" int coocc_head_soft_h2(const void* x_h2, int in_stride, int rows, const int32_t* rows_dev, const void* w1_pack,
                                  const float* scale1, const float* bias1, float* hidden, int hidden_stride, const void* w2_pack,
                                  const float* bias2, int L, float* wlogit, int wlogit_stride, void* stream) {
  HeadTailK k;
  const int rc = ht_fill(k, "head_soft_h2", x_h2, in_stride, rows, rows_dev, w1_pack, scale1, bias1, hidden, hidden_stride, 64, w2_pack, bias2, L,
                         wlogit, wlogit_stride);
  if (rc != COOCC_OK) return rc;
  if (rows == 0) return COOCC_OK;
  k.write_hidden = hidden != nullptr;
  hipLaunchKernelGGL(k_head_soft_h2, dim3(cdiv(rows, HT_BM)), dim3(256), 0, as_stream(stream), k);
  COOCC_LAUNCH_CHECK("k_head_soft_h2");
  return COOCC_OK;
}
