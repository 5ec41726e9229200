// The four occupancy losses of OccHead.loss (co_occ_amd/losses.py: class-weighted cross-entropy, sem_scal, geo_scal, Lovasz-softmax)
// and their analytic gradient with respect to the logits, plus the majority-vote label pooling of loss_voxel -- on the device,
// without a host read, bitwise reproducible from run to run (DESIGN.md "OccHead losses on the device").
//
// Forward:  k_occ_pass1 (softmax per row, fp64 statistics per block, Lovasz sort keys) -> k_occ_stats (block partials added in block
// order, the three closed-form terms and the backward's coefficients) -> one stable radix sort of (class, error descending) ->
// k_lov_count / k_lov_scan / k_lov_apply (foreground prefix count along the sorted order, Lovasz gradient, sum(e * jac) per tile in
// fp64, signed weight scattered back to [P][C]) -> k_lov_final.  Backward: k_occ_bwd, one pass over the rows.
// Every floating-point reduction is "per-thread / per-block partial in a fixed order, then one block in a fixed order"; the only
// integer prefix sums are exact.  No float atomics anywhere.
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <rocprim/rocprim.hpp>

#include "common.h"

namespace {

constexpr int OL_TILE = 256;                 // rows per pass-1 tile (one row per lane), sorted elements per pass-2 tile
constexpr int OL_MAXC = 32;
constexpr int OL_NPART = 8 + 4 * OL_MAXC;    // doubles per block partial = the raw part of the statistics block
constexpr int OL_MAXBLK = 256;               // pass-1 blocks (grid-stride over the tiles)
// statistics block (COOCC_OCC_LOSS_STATS doubles):
//   [0] sum w[t]*nll  [1] sum w[t]  [2] sum tgt*(1-p_e)  [3] sum (1-p_e)  [4] sum tgt  [5] sum (1-tgt)*p_e  [6] sum (1-tgt)  [7] valid rows
//   [8 + 4c + 0..3]   n_t, nom, sum_p, spec_num of class c
//   [D + 0] number of present classes  [D + 1] dL_geo/dp_e of an occupied row  [D + 2] ... of an empty row      (D = 136)
//   [D + 8 + c] dL_sem/dp_c of a row of class c, [D + 40 + c] ... of any other row (both already / present classes; 0 when c is absent)
constexpr int OL_D = OL_NPART;
static_assert(OL_D + 8 + 2 * OL_MAXC == COOCC_OCC_LOSS_STATS, "statistics block layout");


// -log(x) clamped at 100 as losses._bce_to_one: value 100 and ZERO gradient at or below 1e-43
__device__ __forceinline__ double bce1(double x) { return x > 1e-43 ? -log(x) : 100.0; }
__device__ __forceinline__ double dbce1(double x) { return x > 1e-43 ? -1.0 / x : 0.0; }

__device__ __forceinline__ int row_label(const uint8_t* __restrict__ labels, const int64_t* __restrict__ coords, long long i,
                                         long long P, int VX, int VY, int VZ, int C) {
  int lab;
  if (coords) {                                        // loss_point's gather: labels is the volume [VX][VY][VZ], coords [3][P]
    long long x = coords[i], y = coords[P + i], z = coords[2 * P + i];
    bool in = x >= 0 && x < VX && y >= 0 && y < VY && z >= 0 && z < VZ;
    lab = in ? labels[((size_t)x * VY + y) * VZ + z] : 255;
  } else {
    lab = labels[i];
  }
  return lab < C ? lab : 255;                          // 255 = ignore; anything else outside [0, C) is undefined input: ignored too
}

template <int CT>
__device__ __forceinline__ float softmax_row(const float* __restrict__ x, int C, float (&p)[CT], float& lse) {
  float m = -INFINITY;
#pragma unroll
  for (int c = 0; c < CT; ++c) {
    p[c] = c < C ? x[c] : -INFINITY;
    m = fmaxf(m, p[c]);
  }
  float s = 0.f;
#pragma unroll
  for (int c = 0; c < CT; ++c) {
    p[c] = c < C ? expf(p[c] - m) : 0.f;
    s += p[c];
  }
  float inv = 1.f / s;
#pragma unroll
  for (int c = 0; c < CT; ++c) p[c] *= inv;
  lse = m + logf(s);
  return m;
}

// ------------------------------------------------------------------ pass 1
template <int CT>
__global__ __launch_bounds__(256) void k_occ_pass1(const float* __restrict__ logits, long long P, int C, int ld,
                                                    const uint8_t* __restrict__ labels, const int64_t* __restrict__ coords, int VX,
                                                    int VY, int VZ, uint8_t* __restrict__ rowlab, const float* __restrict__ cw,
                                                    int empty_idx, unsigned long long* __restrict__ keys,
                                                    unsigned* __restrict__ vals, double* __restrict__ part) {
  __shared__ float s_p[OL_TILE][CT + 1];
  __shared__ unsigned char s_lab[OL_TILE];
  __shared__ double s_cls[8][CT][4];
  __shared__ double s_sc[4][8];
  const int tid = threadIdx.x;
  const int cc = tid % CT, cpart = tid / CT;           // per-class task: class cc, rows [32 * cpart, 32 * cpart + 32) of the tile
  const bool ctask = cpart < 8 && cc < C;
  double a_nt = 0, a_nom = 0, a_sp = 0, a_spec = 0;    // per-class sums of this thread's task, carried across tiles
  double st[7] = {0, 0, 0, 0, 0, 0, 0};
  const long long tiles = (P + OL_TILE - 1) / OL_TILE;
  for (long long tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
    const long long i = tile * OL_TILE + tid;
    int lab = 255;
    if (i < P) {
      lab = row_label(labels, coords, i, P, VX, VY, VZ, C);
      if (rowlab) rowlab[i] = (uint8_t)lab;
      float p[CT], lse;
      const float* x = logits + (size_t)i * ld;
      softmax_row<CT>(x, C, p, lse);
      if (lab != 255) {
        float xt = 0.f, pe = 0.f;
#pragma unroll
        for (int c = 0; c < CT; ++c) {
          if (c == lab) xt = x[c];
          if (c == empty_idx) pe = p[c];
        }
        float w = cw ? cw[lab] : 1.f;
        st[0] += (double)w * (double)(lse - xt);
        st[1] += (double)w;
        float ne = 1.f - pe;
        if (lab != empty_idx) { st[2] += (double)ne; st[4] += 1.0; } else { st[5] += (double)pe; st[6] += 1.0; }
        st[3] += (double)ne;
      }
#pragma unroll
      for (int c = 0; c < CT; ++c) {
        if (c < C) {
          s_p[tid][c] = p[c];
          unsigned fg = c == lab;
          float e = fabsf((fg ? 1.f : 0.f) - p[c]);
          // ascending radix order = class ascending, error descending; ignored rows go behind every class
          unsigned long long key = lab != 255 ? ((unsigned long long)c << 32) | (unsigned)~__float_as_uint(e)
                                              : (unsigned long long)C << 32;
          keys[(size_t)i * C + c] = key;
          vals[(size_t)i * C + c] = lab != 255 ? ((unsigned)i << 1) | fg : 0u;
        }
      }
    }
    s_lab[tid] = (unsigned char)lab;
    __syncthreads();
    if (ctask) {
      for (int r = cpart * 32; r < cpart * 32 + 32; ++r) {
        int l = s_lab[r];
        if (l == 255) continue;
        double pr = (double)s_p[r][cc];
        a_sp += pr;
        if (l == cc) { a_nt += 1.0; a_nom += pr; } else { a_spec += 1.0 - pr; }
      }
    }
    __syncthreads();
  }
#pragma unroll
  for (int k = 0; k < 7; ++k)
    for (int m = 32; m > 0; m >>= 1) st[k] += __shfl_xor(st[k], m);
  if ((tid & 63) == 0)
    for (int k = 0; k < 7; ++k) s_sc[tid >> 6][k] = st[k];
  if (ctask) { s_cls[cpart][cc][0] = a_nt; s_cls[cpart][cc][1] = a_nom; s_cls[cpart][cc][2] = a_sp; s_cls[cpart][cc][3] = a_spec; }
  __syncthreads();
  double* out = part + (size_t)blockIdx.x * OL_NPART;
  if (tid < 7) out[tid] = s_sc[0][tid] + s_sc[1][tid] + s_sc[2][tid] + s_sc[3][tid];
  if (tid == 7) out[7] = 0.0;
  if (tid < 4 * C) {
    int c = tid >> 2, k = tid & 3;
    double s = 0;
    for (int q = 0; q < 8; ++q) s += s_cls[q][c][k];
    out[8 + tid] = s;
  }
}

// block partials -> statistics, the three closed-form terms, the backward's coefficients.  One block.
__global__ __launch_bounds__(256) void k_occ_stats(const double* __restrict__ part, int nblocks, int C, float* __restrict__ out,
                                                    double* __restrict__ stats) {
  __shared__ double s[OL_NPART];
  const int tid = threadIdx.x;
  if (tid < OL_NPART) {
    double a = 0;
    if (tid < 8 + 4 * C)
      for (int b = 0; b < nblocks; ++b) a += part[(size_t)b * OL_NPART + tid];
    s[tid] = a;
  }
  __syncthreads();
  if (tid == 0) s[7] = s[4] + s[6];
  __syncthreads();
  if (tid < OL_NPART) stats[tid] = s[tid];
  if (tid != 0) return;
  const double eps = 1e-5, nvalid = s[7];
  out[0] = (float)(s[0] / s[1]);                                   // NaN when every row is ignored, like F.cross_entropy
  // geo_scal
  double inter = s[2], sne = s[3] + eps, ntg = s[4] + eps, nng = s[6] + eps;
  double prec = inter / sne, rec = inter / ntg, spec = s[5] / nng;
  out[2] = (float)(bce1(prec) + bce1(rec) + bce1(spec));
  double dprec_common = -inter / (sne * sne);
  stats[OL_D + 1] = -(dbce1(prec) * (1.0 / sne + dprec_common) + dbce1(rec) / ntg);
  stats[OL_D + 2] = -(dbce1(prec) * dprec_common) + dbce1(spec) / nng;
  // sem_scal
  double npres = 0, per = 0;
  for (int c = 0; c < C; ++c) npres += s[8 + 4 * c] > 0 ? 1.0 : 0.0;
  for (int c = 0; c < OL_MAXC; ++c) {
    double s1 = 0, s0 = 0;
    if (c < C && s[8 + 4 * c] > 0) {
      double nt = s[8 + 4 * c], nom = s[9 + 4 * c], sp = s[10 + 4 * c], sn = s[11 + 4 * c], neg = nvalid - nt;
      double spc = sp > 1e-38 ? sp : 1e-38, dsp = sp >= 1e-38 ? 1.0 : 0.0;          // clamp(min=1e-38) and its gradient
      double rp = nom / spc, rr = nom / nt, rs = sn / (neg > 1 ? neg : 1.0);
      bool hp = sp > 0, hs = neg > 0;
      per += (hp ? bce1(rp) : 0.0) + bce1(rr) + (hs ? bce1(rs) : 0.0);
      double fp = hp ? dbce1(rp) : 0.0, fr = dbce1(rr), fs = hs ? dbce1(rs) : 0.0;
      s1 = (fp * (1.0 / spc - dsp * nom / (spc * spc)) + fr / nt) / npres;
      s0 = (fp * (-dsp * nom / (spc * spc)) - fs / (neg > 1 ? neg : 1.0)) / npres;
    }
    stats[OL_D + 8 + c] = s1;
    stats[OL_D + 8 + OL_MAXC + c] = s0;
  }
  out[1] = (float)(per / npres);                                   // NaN without a present class, like losses.sem_scal_loss
  stats[OL_D] = npres;
  for (int k = 3; k < 8; ++k) stats[OL_D + k] = 0.0;
}

// ------------------------------------------------------------------ pass 2 (sorted order: class c = [c * nvalid, (c + 1) * nvalid))
__device__ __forceinline__ int block_prefix(unsigned fg, int tid, int* s_w, int& total) {   // inclusive prefix count of fg in a 256 block
  unsigned long long b = __ballot(fg);
  int lane = tid & 63, wv = tid >> 6;
  int incl = __popcll(b & ((2ull << lane) - 1ull));
  if (lane == 0) s_w[wv] = __popcll(b);
  __syncthreads();
  int off = 0;
  for (int q = 0; q < 4; ++q) off += q < wv ? s_w[q] : 0;
  total = s_w[0] + s_w[1] + s_w[2] + s_w[3];
  return off + incl;
}

__global__ __launch_bounds__(256) void k_lov_count(const unsigned* __restrict__ vals, const double* __restrict__ stats, int ntiles,
                                                    int* __restrict__ tilecnt) {
  __shared__ int s_w[4];
  const int c = blockIdx.y, tile = blockIdx.x;
  const long long nv = (long long)stats[7], k = (long long)tile * OL_TILE + threadIdx.x;
  const bool present = stats[8 + 4 * c] > 0;
  unsigned fg = (present && k < nv) ? vals[(size_t)c * nv + k] & 1u : 0u;
  int total;
  block_prefix(fg, threadIdx.x, s_w, total);
  if (threadIdx.x == 0) tilecnt[(size_t)c * ntiles + tile] = total;
}

__global__ __launch_bounds__(64) void k_lov_scan(int* __restrict__ tilecnt, int ntiles) {      // exclusive, in place, one wave per class
  int* t = tilecnt + (size_t)blockIdx.x * ntiles;
  int carry = 0;
  for (int base = 0; base < ntiles; base += 64) {
    int j = base + threadIdx.x, v = j < ntiles ? t[j] : 0, incl = v;
    for (int d = 1; d < 64; d <<= 1) {
      int u = __shfl_up(incl, d);
      if ((int)threadIdx.x >= d) incl += u;
    }
    if (j < ntiles) t[j] = carry + incl - v;
    carry += __shfl(incl, 63);
  }
}

__global__ __launch_bounds__(256) void k_lov_apply(const unsigned long long* __restrict__ keys, const unsigned* __restrict__ vals,
                                                    const double* __restrict__ stats, const int* __restrict__ tileoff, int ntiles,
                                                    long long P, int C, float* __restrict__ lov_w, double* __restrict__ lpart) {
  __shared__ int s_w[4];
  __shared__ double s_e[4];
  const int c = blockIdx.y, tile = blockIdx.x, tid = threadIdx.x;
  const long long nv = (long long)stats[7], k = (long long)tile * OL_TILE + tid;
  const bool in = stats[8 + 4 * c] > 0 && k < nv;
  unsigned v = in ? vals[(size_t)c * nv + k] : 0u;
  unsigned fg = v & 1u;
  int total;
  int incl = block_prefix(fg, tid, s_w, total);
  double contrib = 0;
  if (in) {
    float e = __uint_as_float(~(unsigned)keys[(size_t)c * nv + k]);
    double gts = stats[8 + 4 * c], cum = (double)(tileoff[(size_t)c * ntiles + tile] + incl), pos = (double)(k + 1);
    double jac = 1.0 - (gts - cum) / (gts + pos - cum);                      // lovasz_grad (lovasz_softmax.py:21-33)
    double cump = cum - (double)fg;
    double jprev = k > 0 ? 1.0 - (gts - cump) / (gts + (pos - 1.0) - cump) : 0.0;
    double g = jac - jprev;
    contrib = (double)e * g;
    double w = e == 0.f ? 0.0 : (fg ? -g : g) / stats[OL_D];                 // d|fg - p|/dp = -1 (fg) / +1, 0 at an error of exactly 0
    if ((long long)(v >> 1) < P) lov_w[(size_t)(v >> 1) * C + c] = (float)w;      // always true; keeps a store inside lov_w whatever the sort returned
  }
  for (int m = 32; m > 0; m >>= 1) contrib += __shfl_xor(contrib, m);
  if ((tid & 63) == 0) s_e[tid >> 6] = contrib;
  __syncthreads();
  if (tid == 0) lpart[(size_t)c * ntiles + tile] = s_e[0] + s_e[1] + s_e[2] + s_e[3];
}

__global__ __launch_bounds__(64) void k_lov_final(const double* __restrict__ lpart, const double* __restrict__ stats, int ntiles, int C,
                                                   float* __restrict__ out) {
  __shared__ double s[OL_MAXC];
  const int c = threadIdx.x;
  if (c < OL_MAXC) {
    double a = 0;
    if (c < C)
      for (int t = 0; t < ntiles; ++t) a += lpart[(size_t)c * ntiles + t];
    s[c] = a;
  }
  __syncthreads();
  if (c != 0) return;
  double a = 0;
  for (int q = 0; q < C; ++q) a += s[q];
  out[3] = stats[7] > 0 ? (float)(a / stats[OL_D]) : 0.f;                    // no valid row: 0, like losses.lovasz_softmax
}

// ------------------------------------------------------------------ backward
template <int CT>
__global__ __launch_bounds__(256) void k_occ_bwd(const float* __restrict__ logits, long long P, int C, int ld,
                                                  const uint8_t* __restrict__ labels, const float* __restrict__ cw, int empty_idx,
                                                  const double* __restrict__ stats, const float* __restrict__ lov_w,
                                                  const float* __restrict__ gout, float* __restrict__ dlogits, int ldg) {
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  if (i >= P) return;
  float* d = dlogits + (size_t)i * ldg;
  int lab = labels[i];
  if (lab >= C) {                                      // ignored rows: exactly 0
#pragma unroll
    for (int c = 0; c < CT; ++c)
      if (c < C) d[c] = 0.f;
    return;
  }
  float p[CT], lse;
  softmax_row<CT>(logits + (size_t)i * ld, C, p, lse);
  const double g_ce = gout[0], g_sem = gout[1], g_geo = gout[2], g_lov = gout[3];
  double g[CT], dot = 0;
#pragma unroll
  for (int c = 0; c < CT; ++c) {
    g[c] = 0;
    if (c < C) {
      double v = g_sem * (c == lab ? stats[OL_D + 8 + c] : stats[OL_D + 8 + OL_MAXC + c]);
      if (c == empty_idx) v += g_geo * (lab != empty_idx ? stats[OL_D + 1] : stats[OL_D + 2]);
      if (stats[8 + 4 * c] > 0) v += g_lov * (double)lov_w[(size_t)i * C + c];
      g[c] = v;
      dot += v * (double)p[c];
    }
  }
  const double wce = g_ce * (double)(cw ? cw[lab] : 1.f) / stats[1];
#pragma unroll
  for (int c = 0; c < CT; ++c)
    if (c < C) d[c] = (float)((double)p[c] * (g[c] - dot) + wce * ((double)p[c] - (c == lab ? 1.0 : 0.0)));
}

// ------------------------------------------------------------------ label pooling (occ_head.py:269-281, losses.pool_labels)
template <int R>
__global__ __launch_bounds__(256) void k_pool_labels(const uint8_t* __restrict__ vol, long long cells, int H, int W, int D,
                                                      int empty_idx, int num_cls, uint8_t* __restrict__ out) {
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  if (i >= cells) return;
  int d = (int)(i % D), w = (int)(i / D % W), h = (int)(i / ((long long)D * W) % H);
  long long b = i / ((long long)D * W * H);
  int bin[R * R * R], sum = 0;
#pragma unroll
  for (int a = 0; a < R; ++a)
#pragma unroll
    for (int e = 0; e < R; ++e)
#pragma unroll
      for (int f = 0; f < R; ++f) {
        int t = vol[(((size_t)b * H * R + h * R + a) * ((size_t)W * R) + w * R + e) * ((size_t)D * R) + d * R + f];
        sum += t;
        bin[(a * R + e) * R + f] = t == 255 ? num_cls : (t < num_cls - 1 ? t : num_cls - 1);
      }
  int n_empty = 0, m = -1, arg = 0;
  for (int l = 0; l <= num_cls; ++l) {                 // first (= smallest label) maximum of the histogram with the empty bin zeroed
    int n = 0;
#pragma unroll
    for (int q = 0; q < R * R * R; ++q) n += bin[q] == l;
    if (l == empty_idx) { n_empty = n; n = 0; }
    if (n > m) { m = n; arg = l; }
  }
  if (arg == num_cls) arg = 255;
  int o = (m == 1 && n_empty > 0) ? 255 : arg;
  out[i] = (uint8_t)(sum == empty_idx ? empty_idx : o);
}

struct OlLayout {
  size_t part, keys_in, keys_out, vals_in, vals_out, tilecnt, lpart, tmp, tmp_bytes, total;
  int ntiles;
};

static OlLayout ol_layout(int64_t P, int C) {
  OlLayout L;
  size_t n = (size_t)P * C, o = 0;
  L.ntiles = (int)((P + OL_TILE - 1) / OL_TILE);
  L.part = o; o += al256(sizeof(double) * OL_MAXBLK * OL_NPART);
  L.keys_in = o; o += al256(8 * n);
  L.keys_out = o; o += al256(8 * n);
  L.vals_in = o; o += al256(4 * n);
  L.vals_out = o; o += al256(4 * n);
  L.tilecnt = o; o += al256(sizeof(int) * (size_t)C * L.ntiles);
  L.lpart = o; o += al256(sizeof(double) * (size_t)C * L.ntiles);
  size_t tmp = 0;
  (void)rocprim::radix_sort_pairs(nullptr, tmp, (unsigned long long*)nullptr, (unsigned long long*)nullptr, (unsigned*)nullptr,
                                  (unsigned*)nullptr, n, 0, 38, (hipStream_t)0);
  L.tmp = o; L.tmp_bytes = al256(tmp); o += L.tmp_bytes;
  L.total = o + 256;
  return L;
}

static bool ol_shape_ok(int64_t P, int C, int ld) { return P > 0 && P < ((int64_t)1 << 31) && C >= 1 && C <= OL_MAXC && ld >= C; }

}  // namespace

extern "C" size_t coocc_occ_loss_ws(int64_t P, int C) {
  if (P <= 0 || P >= ((int64_t)1 << 31) || C < 1 || C > OL_MAXC) return 256;
  return ol_layout(P, C).total;
}

extern "C" int coocc_pool_labels(const uint8_t* vol, int B, int H, int W, int D, int ratio, int empty_idx, int num_cls, uint8_t* out,
                                 void* stream) {
  COOCC_CHECK_ARG(vol && out, "pool_labels: null pointer");
  COOCC_CHECK_ARG(ratio == 1 || ratio == 2 || ratio == 4, "pool_labels: ratio %d (1, 2 and 4 are implemented)", ratio);
  COOCC_CHECK_ARG(B > 0 && H > 0 && W > 0 && D > 0 && num_cls >= 1 && num_cls <= 254 && empty_idx >= 0 && empty_idx < num_cls,
                  "pool_labels: bad shape B=%d H=%d W=%d D=%d num_cls=%d empty_idx=%d", B, H, W, D, num_cls, empty_idx);
  long long cells = (long long)B * H * W * D;
  hipStream_t s = as_stream(stream);
  if (ratio == 1) {
    COOCC_HIP(hipMemcpyAsync(out, vol, (size_t)cells, hipMemcpyDeviceToDevice, s));
    return COOCC_OK;
  }
  if (ratio == 2)
    hipLaunchKernelGGL(k_pool_labels<2>, dim3(cdiv(cells, 256)), dim3(256), 0, s, vol, cells, H, W, D, empty_idx, num_cls, out);
  else
    hipLaunchKernelGGL(k_pool_labels<4>, dim3(cdiv(cells, 256)), dim3(256), 0, s, vol, cells, H, W, D, empty_idx, num_cls, out);
  COOCC_LAUNCH_CHECK("k_pool_labels");
  return COOCC_OK;
}

#define OL_DISPATCH(C, CALL) \
  do {                       \
    if ((C) <= 8) { CALL(8); } else if ((C) <= 16) { CALL(16); } else if ((C) <= 24) { CALL(24); } else { CALL(32); } \
  } while (0)

extern "C" int coocc_occ_loss_fwd(const float* logits, int64_t P, int C, int ld, const uint8_t* labels, const int64_t* coords, int VX,
                                  int VY, int VZ, uint8_t* row_labels, const float* class_w, int empty_idx, float* out, double* stats,
                                  float* lov_w, void* ws, size_t ws_bytes, void* stream) {
  COOCC_CHECK_ARG(C <= OL_MAXC, "occ_loss_fwd: C = %d (at most %d classes)", C, OL_MAXC);
  COOCC_CHECK_ARG(logits && labels && out && stats && lov_w && ws, "occ_loss_fwd: null pointer");
  COOCC_CHECK_ARG(ol_shape_ok(P, C, ld) && empty_idx >= 0 && empty_idx < C, "occ_loss_fwd: bad shape P=%lld C=%d ld=%d empty_idx=%d",
                  (long long)P, C, ld, empty_idx);
  COOCC_CHECK_ARG(!coords || (row_labels && VX > 0 && VY > 0 && VZ > 0),
                  "occ_loss_fwd: the coordinate form needs row_labels and the volume's extents");
  OlLayout L = ol_layout(P, C);
  if (ws_bytes < L.total) return coocc_set_error(COOCC_ENOMEM, "occ_loss_fwd: workspace too small (%zu < %zu bytes)", ws_bytes, L.total);
  char* b = ws_base256(ws);
  double* part = (double*)(b + L.part);
  unsigned long long *k_in = (unsigned long long*)(b + L.keys_in), *k_out = (unsigned long long*)(b + L.keys_out);
  unsigned *v_in = (unsigned*)(b + L.vals_in), *v_out = (unsigned*)(b + L.vals_out);
  int* tilecnt = (int*)(b + L.tilecnt);
  double* lpart = (double*)(b + L.lpart);
  hipStream_t s = as_stream(stream);
  int nblocks = std::min(L.ntiles, OL_MAXBLK);
#define OL_PASS1(CT)                                                                                                              \
  hipLaunchKernelGGL(k_occ_pass1<CT>, dim3(nblocks), dim3(256), 0, s, logits, (long long)P, C, ld, labels, coords, VX, VY, VZ,      \
                     row_labels, class_w, empty_idx, k_in, v_in, part)
  OL_DISPATCH(C, OL_PASS1);
#undef OL_PASS1
  hipLaunchKernelGGL(k_occ_stats, dim3(1), dim3(256), 0, s, (const double*)part, nblocks, C, out, stats);
  COOCC_LAUNCH_CHECK("k_occ_pass1");
  COOCC_HIP(rocprim::radix_sort_pairs(b + L.tmp, L.tmp_bytes, k_in, k_out, v_in, v_out, (size_t)P * C, 0, 38, s));
  hipLaunchKernelGGL(k_lov_count, dim3(L.ntiles, C), dim3(256), 0, s, (const unsigned*)v_out, (const double*)stats, L.ntiles, tilecnt);
  hipLaunchKernelGGL(k_lov_scan, dim3(C), dim3(64), 0, s, tilecnt, L.ntiles);
  hipLaunchKernelGGL(k_lov_apply, dim3(L.ntiles, C), dim3(256), 0, s, (const unsigned long long*)k_out, (const unsigned*)v_out,
                     (const double*)stats, (const int*)tilecnt, L.ntiles, (long long)P, C, lov_w, lpart);
  hipLaunchKernelGGL(k_lov_final, dim3(1), dim3(64), 0, s, (const double*)lpart, (const double*)stats, L.ntiles, C, out);
  COOCC_LAUNCH_CHECK("k_lov");
  return COOCC_OK;
}

extern "C" int coocc_occ_loss_bwd(const float* logits, int64_t P, int C, int ld, const uint8_t* row_labels, const float* class_w,
                                  int empty_idx, const double* stats, const float* lov_w, const float* gout, float* dlogits, int ldg,
                                  void* stream) {
  COOCC_CHECK_ARG(C <= OL_MAXC, "occ_loss_bwd: C = %d (at most %d classes)", C, OL_MAXC);
  COOCC_CHECK_ARG(logits && row_labels && stats && lov_w && gout && dlogits, "occ_loss_bwd: null pointer");
  COOCC_CHECK_ARG(ol_shape_ok(P, C, ld) && ldg >= C && empty_idx >= 0 && empty_idx < C,
                  "occ_loss_bwd: bad shape P=%lld C=%d ld=%d ldg=%d empty_idx=%d", (long long)P, C, ld, ldg, empty_idx);
  hipStream_t s = as_stream(stream);
#define OL_BWD(CT)                                                                                                                 \
  hipLaunchKernelGGL(k_occ_bwd<CT>, dim3(cdiv(P, 256)), dim3(256), 0, s, logits, (long long)P, C, ld, row_labels, class_w, empty_idx, \
                     stats, lov_w, gout, dlogits, ldg)
  OL_DISPATCH(C, OL_BWD);
#undef OL_BWD
  COOCC_LAUNCH_CHECK("k_occ_bwd");
  return COOCC_OK;
}
