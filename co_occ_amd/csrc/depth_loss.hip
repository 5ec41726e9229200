// The DepthNet depth loss of ViewTransformerLiftSplatShootVoxel (co_occ_amd/view_transformer.py get_downsampled_gt_depth +
// get_depth_loss, 'bce') and its gradient with respect to the depth probabilities -- on the device, without a host read, bitwise
// reproducible from run to run (DESIGN.md "DepthNet depth loss on the device").
//
// Forward:  k_depth_labels (nearest non-zero depth of every ds x ds patch -> bin value and label) -> k_depth_bce (fp32 terms of the
// foreground pixels, one fp64 partial per (pixel block, bin slice) workgroup) -> k_depth_bce_final (partials added in a fixed order,
// the loss and the (sum, n_fg) pair the backward reads).  Backward: k_depth_bce_bwd, one pass that writes every element.
// Every floating-point reduction is "per-thread partial, butterfly inside the wave, waves in wave order, workgroups in index order".
// No float atomics anywhere.
#include "common.h"

namespace {

typedef float dl_f4 __attribute__((ext_vector_type(4)));

constexpr int DB_BINS = 8;                   // bins per slice: r50 (4224 pixels, D = 112) runs 17 x 14 workgroups instead of 17

__device__ __forceinline__ float zero_is_far(float x) { return x == 0.f ? 1e5f : x; }
__device__ __forceinline__ float min2(float a, float b) { return b < a ? b : a; }

__device__ __forceinline__ void write_label(float m, float c0, float step, int D, float* __restrict__ vals, int* __restrict__ labels,
                                            size_t o) {
  float v = __fdiv_rn(m - c0, step);                   // two fp32 operations, as the eager expression; never a reciprocal
  vals[o] = v;
  labels[o] = (v >= 0.f && v < (float)(D + 1)) ? (int)v : 0;
}

// ------------------------------------------------------------------ labels, ds >= 4: a lane owns 4 columns of a patch (one 16-byte
// load per patch row), the DS / 4 lanes of a patch sit next to each other in the wave and meet in a shuffle butterfly
template <int DS>
__global__ __launch_bounds__(256) void k_depth_labels_v(const float* __restrict__ gt, long long nchunks, int W, float c0, float step,
                                                         int D, float* __restrict__ vals, int* __restrict__ labels) {
  constexpr int L = DS / 4;
  const long long t = (long long)blockIdx.x * 256 + threadIdx.x;
  const int wq = W >> 2;                               // chunks per image row = (W / DS) * L
  const bool in = t < nchunks;                         // nchunks is a multiple of L: the lanes of a patch are in or out together
  long long row = 0;                                   // bn * h + i
  int c = 0;
  float m = INFINITY;
  if (in) {
    row = t / wq;
    c = (int)(t - row * wq);
    const float* p = gt + (size_t)row * DS * W + 4 * c;          // H = h * DS: row * DS is the patch's first image row
#pragma unroll
    for (int r = 0; r < DS; ++r) {
      dl_f4 v = *(const dl_f4*)(p + (size_t)r * W);
      m = min2(m, min2(min2(zero_is_far(v[0]), zero_is_far(v[1])), min2(zero_is_far(v[2]), zero_is_far(v[3]))));
    }
  }
#pragma unroll
  for (int s = L / 2; s > 0; s >>= 1) m = min2(m, __shfl_xor(m, s));
  if (in && (c & (L - 1)) == 0) write_label(m, c0, step, D, vals, labels, (size_t)row * (W / DS) + c / L);
}

// any ds (1 and 2; also the larger ones when gt is not 16-byte aligned): one thread per output pixel
__global__ __launch_bounds__(256) void k_depth_labels_s(const float* __restrict__ gt, long long npix, int W, int ds, float c0,
                                                         float step, int D, float* __restrict__ vals, int* __restrict__ labels) {
  const long long t = (long long)blockIdx.x * 256 + threadIdx.x;
  if (t >= npix) return;
  const int w = W / ds;
  const long long row = t / w;
  const int j = (int)(t - row * w);
  const float* p = gt + (size_t)row * ds * W + (size_t)j * ds;
  float m = INFINITY;
  for (int r = 0; r < ds; ++r)
    for (int e = 0; e < ds; ++e) m = min2(m, zero_is_far(p[(size_t)r * W + e]));
  write_label(m, c0, step, D, vals, labels, (size_t)t);
}

// ------------------------------------------------------------------ BCE forward: workgroup (x, y) = pixels [256 x, 256 x + 256) x
// bins [DB_BINS y, DB_BINS y + DB_BINS); lanes run along the pixels (the fastest index of a bin plane)
__device__ __forceinline__ float bce_term(float p, bool y) {
  return y ? -fmaxf(logf(p), -100.f) : -fmaxf(log1pf(-p), -100.f);         // the -100 clamp of F.binary_cross_entropy
}

// COOCC_SCALAR_FP32: the log1pf expansion compiled to v_pk_add_f32 with op_sel[src1] = 1
__global__ __launch_bounds__(256) COOCC_SCALAR_FP32 void k_depth_bce(const float* __restrict__ prob, const int* __restrict__ labels, long long P, int D,
                                                    int hw, double* __restrict__ part, double* __restrict__ cnt) {
  __shared__ double s_a[4];
  __shared__ int s_n[4];
  const int tid = threadIdx.x;
  const long long p = (long long)blockIdx.x * 256 + tid;
  const int d0 = blockIdx.y * DB_BINS;
  double acc = 0;
  bool fg = false;
  if (p < P) {
    const int lab = labels[p];
    fg = lab > 0;
    if (fg) {
      const long long bn = p / hw;
      const float* x = prob + ((size_t)bn * D + d0) * hw + (p - bn * hw);
      float v[DB_BINS];
#pragma unroll
      for (int k = 0; k < DB_BINS; ++k) v[k] = d0 + k < D ? x[(size_t)k * hw] : 0.f;
#pragma unroll
      for (int k = 0; k < DB_BINS; ++k)
        if (d0 + k < D) acc += (double)bce_term(v[k], d0 + k + 1 == lab);
    }
  }
  for (int m = 32; m > 0; m >>= 1) acc += __shfl_xor(acc, m);
  const unsigned long long b = __ballot(fg);
  if ((tid & 63) == 0) { s_a[tid >> 6] = acc; s_n[tid >> 6] = __popcll(b); }
  __syncthreads();
  if (tid == 0) {
    part[(size_t)blockIdx.y * gridDim.x + blockIdx.x] = ((s_a[0] + s_a[1]) + s_a[2]) + s_a[3];
    if (blockIdx.y == 0) cnt[blockIdx.x] = (double)(s_n[0] + s_n[1] + s_n[2] + s_n[3]);
  }
}

// one workgroup: thread t adds partials t, t + 256, ... in that order, then the butterfly and the four waves in wave order
__global__ __launch_bounds__(256) void k_depth_bce_final(const double* __restrict__ part, int nparts, const double* __restrict__ cnt,
                                                          int nblk, float weight, float* __restrict__ loss, double* __restrict__ stats) {
  __shared__ double s_a[4], s_n[4];
  const int tid = threadIdx.x;
  double a = 0, n = 0;
  for (int k = tid; k < nparts; k += 256) a += part[k];
  for (int k = tid; k < nblk; k += 256) n += cnt[k];                 // integers below 2^53: exact in any order
  for (int m = 32; m > 0; m >>= 1) { a += __shfl_xor(a, m); n += __shfl_xor(n, m); }
  if ((tid & 63) == 0) { s_a[tid >> 6] = a; s_n[tid >> 6] = n; }
  __syncthreads();
  if (tid != 0) return;
  a = ((s_a[0] + s_a[1]) + s_a[2]) + s_a[3];
  n = s_n[0] + s_n[1] + s_n[2] + s_n[3];
  stats[0] = a;
  stats[1] = n;
  loss[0] = (float)((double)weight * a / (n > 1.0 ? n : 1.0));       // no foreground: a = 0 and the loss is exactly 0
}

// ------------------------------------------------------------------ BCE backward, the forward's grid; every element is written
__global__ __launch_bounds__(256) void k_depth_bce_bwd(const float* __restrict__ prob, const int* __restrict__ labels, long long P,
                                                        int D, int hw, float weight, const double* __restrict__ stats,
                                                        const float* __restrict__ gout, float* __restrict__ dprob) {
  const long long p = (long long)blockIdx.x * 256 + threadIdx.x;
  if (p >= P) return;
  const int d0 = blockIdx.y * DB_BINS;
  const int lab = labels[p];
  const long long bn = p / hw;
  const size_t o = ((size_t)bn * D + d0) * hw + (p - bn * hw);
  if (lab <= 0) {
#pragma unroll
    for (int k = 0; k < DB_BINS; ++k)
      if (d0 + k < D) dprob[o + (size_t)k * hw] = 0.f;
    return;
  }
  const double n = stats[1];
  const float s = (float)((double)gout[0] * (double)weight / (n > 1.0 ? n : 1.0));
  float v[DB_BINS];
#pragma unroll
  for (int k = 0; k < DB_BINS; ++k) v[k] = d0 + k < D ? prob[o + (size_t)k * hw] : 0.f;
#pragma unroll
  for (int k = 0; k < DB_BINS; ++k)
    if (d0 + k < D) {
      const float y = d0 + k + 1 == lab ? 1.f : 0.f;
      dprob[o + (size_t)k * hw] = s * (v[k] - y) / fmaxf((1.f - v[k]) * v[k], 1e-12f);
    }
}

static inline int db_blocks(int64_t P) { return (int)((P + 255) / 256); }
static inline int db_slices(int D) { return (D + DB_BINS - 1) / DB_BINS; }
static bool db_shape_ok(int BN, int D, int h, int w) {
  if (!(BN > 0 && h > 0 && w > 0 && D >= 1 && D <= (1 << 16) && (int64_t)BN * h * w < ((int64_t)1 << 31))) return false;
  return (int64_t)db_blocks((int64_t)BN * h * w) * db_slices(D) < ((int64_t)1 << 30);        // the partial count is an int
}

}  // namespace

extern "C" int coocc_depth_labels(const float* gt, int BN, int H, int W, int ds, float c0, float step, int D, float* vals,
                                  int32_t* labels, void* stream) {
  COOCC_CHECK_ARG(gt && vals && labels, "depth_labels: null pointer");
  COOCC_CHECK_ARG(ds >= 1 && ds <= 32 && (ds & (ds - 1)) == 0, "depth_labels: ds = %d (a power of two from 1 to 32)", ds);
  COOCC_CHECK_ARG(D >= 1, "depth_labels: D = %d (at least one bin)", D);
  COOCC_CHECK_ARG(BN > 0 && H > 0 && W > 0 && H % ds == 0 && W % ds == 0 && (int64_t)BN * H * W < ((int64_t)1 << 40),
                  "depth_labels: bad shape BN=%d H=%d W=%d for ds=%d (H and W are multiples of ds)", BN, H, W, ds);
  hipStream_t s = as_stream(stream);
  const long long npix = (long long)BN * (H / ds) * (W / ds);
  if (ds >= 4 && ((uintptr_t)gt & 15) == 0) {
    const long long nchunks = (long long)BN * (H / ds) * (W / 4);
#define DL_LAUNCH(DS) \
  hipLaunchKernelGGL(k_depth_labels_v<DS>, dim3(cdiv(nchunks, 256)), dim3(256), 0, s, gt, nchunks, W, c0, step, D, vals, labels)
    if (ds == 4) DL_LAUNCH(4); else if (ds == 8) DL_LAUNCH(8); else if (ds == 16) DL_LAUNCH(16); else DL_LAUNCH(32);
#undef DL_LAUNCH
  } else {
    hipLaunchKernelGGL(k_depth_labels_s, dim3(cdiv(npix, 256)), dim3(256), 0, s, gt, npix, W, ds, c0, step, D, vals, labels);
  }
  COOCC_LAUNCH_CHECK("k_depth_labels");
  return COOCC_OK;
}

extern "C" size_t coocc_depth_bce_ws(int64_t P, int D) {
  if (P <= 0 || P >= ((int64_t)1 << 31) || D < 1 || D > (1 << 16)) return 256;
  return sizeof(double) * (size_t)db_blocks(P) * (db_slices(D) + 1) + 256;
}

extern "C" int coocc_depth_bce(const float* prob, const int32_t* labels, int BN, int D, int h, int w, float weight, float* loss,
                               double* stats, void* ws, size_t ws_bytes, void* stream) {
  COOCC_CHECK_ARG(prob && labels && loss && stats && ws, "depth_bce: null pointer");
  COOCC_CHECK_ARG(D >= 1, "depth_bce: D = %d (at least one bin)", D);
  COOCC_CHECK_ARG(db_shape_ok(BN, D, h, w), "depth_bce: bad shape BN=%d D=%d h=%d w=%d", BN, D, h, w);
  const int64_t P = (int64_t)BN * h * w;
  const size_t need = coocc_depth_bce_ws(P, D);
  COOCC_CHECK_ARG(ws_bytes >= need, "depth_bce: workspace too small (%zu < %zu bytes)", ws_bytes, need);
  const int nblk = db_blocks(P), nsl = db_slices(D);
  double* part = (double*)ws_base256(ws);
  double* cnt = part + (size_t)nblk * nsl;
  hipStream_t s = as_stream(stream);
  hipLaunchKernelGGL(k_depth_bce, dim3(nblk, nsl), dim3(256), 0, s, prob, labels, (long long)P, D, h * w, part, cnt);
  hipLaunchKernelGGL(k_depth_bce_final, dim3(1), dim3(256), 0, s, (const double*)part, nblk * nsl, (const double*)cnt, nblk, weight, loss,
                     stats);
  COOCC_LAUNCH_CHECK("k_depth_bce");
  return COOCC_OK;
}

extern "C" int coocc_depth_bce_bwd(const float* prob, const int32_t* labels, int BN, int D, int h, int w, float weight,
                                   const double* stats, const float* gout, float* dprob, void* stream) {
  COOCC_CHECK_ARG(prob && labels && stats && gout && dprob, "depth_bce_bwd: null pointer");
  COOCC_CHECK_ARG(D >= 1, "depth_bce_bwd: D = %d (at least one bin)", D);
  COOCC_CHECK_ARG(db_shape_ok(BN, D, h, w), "depth_bce_bwd: bad shape BN=%d D=%d h=%d w=%d", BN, D, h, w);
  const int64_t P = (int64_t)BN * h * w;
  hipLaunchKernelGGL(k_depth_bce_bwd, dim3(db_blocks(P), db_slices(D)), dim3(256), 0, as_stream(stream), prob, labels, (long long)P, D,
                     h * w, weight, stats, gout, dprob);
  COOCC_LAUNCH_CHECK("k_depth_bce_bwd");
  return COOCC_OK;
}
