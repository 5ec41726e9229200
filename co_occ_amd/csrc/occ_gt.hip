// Occupancy ground truth from the annotation rows (co_occ_amd/occ_gt.py): what the reference's LoadOccupancy,
// LoadOccupancy2 (P/datasets/pipelines/loading.py:59-134, 217-353) and LoadNuscOccupancyAnnotations (loading_nusc_occ.py:61-137)
// put into results -- gt_occ, the visibility masks, points_occ and aabb -- without the dense volume ever being made on the host.
// Integers are the reference's integers; this file is compiled with -ffp-contract=off (build.FILE_FLAGS) because every float
// that decides an integer (a voxel index, a pixel, d*10) is rounded where numpy / ATen's CPU code rounds it.
//
//   form A  k_scatter_win + k_scatter_final: an indexed assignment where THE LAST ROW WINS.  atomicMax of ((row + 1) << 8 | label)
//           per voxel, then the low byte: the maximum is the highest row, whatever the thread order.
//   form B  k_rows_to_voxels: centre = (idx[[2,1,0]] + 0.5) * voxel_size + lo in float64, rounded to fp32, bda_rot @ centre in fp32
//           (ATen's CPU bmm: products rounded, sums left to right), back to float64, (x - lo) / voxel_size, clip, truncate.
//   form C  k_points_to_voxels: points @ bda_rot^T in fp32, the learning_map table, floor((clip(p, lo, hi - 1e-5) - lo) / voxel_size)
//           in float64; the same kernel makes points_occ and the LiDAR visibility voxels of form B.
//   vote    k_vote_keys + rocprim::radix_sort_keys + k_vote_runs: keys voxel * 256 + label sorted, then the thread on a voxel's first
//           key walks its label runs in ascending label: count modulo 65 536 (the reference's uint16 counter), strictly greater
//           replaces -- np.argmax, the lowest label among the maxima.  No atomics on the volume; independent of the row order.
//   masks   k_visible_min + k_visible_flag: lidar_project (csrc/lidar_project.h), the chain depth_maps.hip calls; a pixel keeps the lexicographic
//           minimum of (d*10 truncated, row) below 2048 with a 64-bit atomicMin -- the reference's sequential z-buffer, whose strict `<` lets the
//           lowest row win among equals -- and a row is visible if it is the pixel's winner in any camera.
//   aabb    k_cloud_aabb + k_aabb_final: the two rigid float64 transforms left to right, min / max on order-preserving 64-bit keys,
//           one rounding to fp32 at the end; a NaN takes the all-ones key in both slots and comes out as NaN, as numpy's min / max.
// Every kernel checks its indices against the volume: rows outside it are skipped, whatever they contain.
#include <stdlib.h>
#include <string.h>

#include <rocprim/rocprim.hpp>

#include "common.h"
#include "lidar_project.h"

namespace {

constexpr unsigned OG_DROPPED = 0xFFFFFFFFu;

struct OgGrid { double lo[3], hi[3], vs[3]; int g[3]; };
struct OgMat { float m[9]; int on; };
struct OgXf { double r1[9], t1[3], r2[9], t2[3]; };

// ---------------------------------------------------------------- form A
__global__ __launch_bounds__(256) void k_scatter_win(const uint16_t* __restrict__ rows, long long N, int G0, int G1, int G2, int use_semantic,
                                                     unsigned int* __restrict__ win) {
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  if (i >= N) return;
  const uint16_t* r = rows + i * 4;
  const int a = r[0], b = r[1], c = r[2];
  unsigned lab = r[3] & 255u;
  if (use_semantic) { if (lab == 0u) lab = 255u; }
  else { if (lab == 0u) return; lab = 1u; }
  if (a >= G0 || b >= G1 || c >= G2) return;
  atomicMax(win + ((size_t)a * G1 + b) * G2 + c, ((unsigned)(i + 1) << 8) | lab);
}

__global__ __launch_bounds__(256) void k_scatter_final(const unsigned int* __restrict__ win, long long V, uint8_t* __restrict__ vol) {
  const long long v = (long long)blockIdx.x * 256 + threadIdx.x;
  if (v < V) vol[v] = (uint8_t)(win[v] & 255u);
}

// ---------------------------------------------------------------- form B
__global__ __launch_bounds__(256) COOCC_SCALAR_FP32 void k_rows_to_voxels(const uint16_t* __restrict__ rows, long long N, OgGrid G, OgMat B,
                                                                          int* __restrict__ vox, uint8_t* __restrict__ labels,
                                                                          float* __restrict__ centres) {
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  if (i >= N) return;
  const uint16_t* r = rows + i * 4;
  const float cx = (float)(((double)r[2] + 0.5) * G.vs[0] + G.lo[0]);
  const float cy = (float)(((double)r[1] + 0.5) * G.vs[1] + G.lo[1]);
  const float cz = (float)(((double)r[0] + 0.5) * G.vs[2] + G.lo[2]);
  if (centres) { centres[i * 3] = cx; centres[i * 3 + 1] = cy; centres[i * 3 + 2] = cz; }
  const float t[3] = {(B.m[0] * cx + B.m[1] * cy) + B.m[2] * cz, (B.m[3] * cx + B.m[4] * cy) + B.m[5] * cz,
                      (B.m[6] * cx + B.m[7] * cy) + B.m[8] * cz};
  int idx[3];
#pragma unroll
  for (int a = 0; a < 3; ++a) {
    double w = ((double)t[a] - G.lo[a]) / G.vs[a];
    w = fmin(fmax(w, 0.0), (double)(G.g[a] - 1));          // np.clip
    idx[a] = (w >= 0.0) ? (int)w : -1;                     // a NaN stays out
  }
  const bool ok = idx[0] >= 0 && idx[1] >= 0 && idx[2] >= 0;
  vox[i] = ok ? (idx[0] * G.g[1] + idx[1]) * G.g[2] + idx[2] : -1;
  const unsigned lab = r[3] & 255u;
  labels[i] = (uint8_t)(lab == 0u ? 255u : lab);
}

// ---------------------------------------------------------------- form C, points_occ, the LiDAR visibility voxels
// mode 0: points_occ only; 1: form C (clip, floor; non-finite points dropped); 2: LiDAR mask (in-range test on the points as given,
// truncation, label 1)
__global__ __launch_bounds__(256) COOCC_SCALAR_FP32 void k_points_to_voxels(const float* __restrict__ points, long long P, int stride,
                                                                            const uint8_t* __restrict__ seg, const uint8_t* __restrict__ table,
                                                                            OgMat B, OgGrid G, int mode, int* __restrict__ vox,
                                                                            uint8_t* __restrict__ labels, float* __restrict__ points_occ) {
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  if (i >= P) return;
  const float* p = points + (size_t)i * stride;
  const float x = p[0], y = p[1], z = p[2];
  float t[3] = {x, y, z};
  if (B.on) {          // points @ bda_rot^T
    t[0] = (x * B.m[0] + y * B.m[1]) + z * B.m[2];
    t[1] = (x * B.m[3] + y * B.m[4]) + z * B.m[5];
    t[2] = (x * B.m[6] + y * B.m[7]) + z * B.m[8];
  }
  const unsigned lab = seg ? table[seg[i]] : 0u;
  if (points_occ) {
    float* o = points_occ + i * 4;
    o[0] = t[0]; o[1] = t[1]; o[2] = t[2]; o[3] = (float)lab;
  }
  if (mode == 0) return;
  int idx[3];
  bool ok = true;
  if (mode == 1) {
#pragma unroll
    for (int a = 0; a < 3; ++a) {
      ok = ok && isfinite(t[a]);
      const double c = fmin(fmax((double)t[a], G.lo[a]), G.hi[a]);          // hi: the host's hi - 1e-5
      const double w = floor((c - G.lo[a]) / G.vs[a]);
      idx[a] = (w >= 0.0) ? (int)fmin(w, (double)(G.g[a] - 1)) : 0;
    }
    labels[i] = (uint8_t)lab;
  } else {
    const float q[3] = {x, y, z};
#pragma unroll
    for (int a = 0; a < 3; ++a) {
      const double c = (double)q[a];
      ok = ok && c >= G.lo[a] && c < G.hi[a];
      const double w = (c - G.lo[a]) / G.vs[a];
      idx[a] = (w >= 0.0 && w < (double)G.g[a]) ? (int)w : -1;
      ok = ok && idx[a] >= 0;
    }
    labels[i] = 1;
  }
  vox[i] = ok ? (idx[0] * G.g[1] + idx[1]) * G.g[2] + idx[2] : -1;
}

// ---------------------------------------------------------------- the vote
__global__ __launch_bounds__(256) void k_vote_keys(const int* __restrict__ vox, const uint8_t* __restrict__ labels, long long N, long long V,
                                                   unsigned int* __restrict__ keys, unsigned int* __restrict__ dropped) {
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  if (i >= N) return;
  const long long v = vox[i];
  if (v < 0 || v >= V) {
    keys[i] = OG_DROPPED;
    atomicAdd(dropped, 1u);
  } else {
    keys[i] = ((unsigned)v << 8) | labels[i];
  }
}

// first index in (pos, n] whose key differs from keys[pos]: gallop, then bisect
__device__ __forceinline__ long long og_run_end(const unsigned int* __restrict__ keys, long long pos, long long n, unsigned key) {
  long long step = 1;
  while (pos + step < n && keys[pos + step] == key) step <<= 1;
  long long lo = pos + (step >> 1), hi = pos + step < n ? pos + step : n;          // keys[lo] == key; keys[hi] != key or hi == n
  while (hi - lo > 1) {
    const long long mid = lo + ((hi - lo) >> 1);
    if (keys[mid] == key) lo = mid; else hi = mid;
  }
  return hi;
}

__global__ __launch_bounds__(256) void k_vote_runs(const unsigned int* __restrict__ keys, long long N, const unsigned int* __restrict__ dropped,
                                                   long long V, int post_empty, uint8_t* __restrict__ vol) {
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  const long long n = N - (long long)*dropped;          // the dropped keys sort to the end
  if (i >= n) return;
  const unsigned voxel = keys[i] >> 8;
  if (i > 0 && (keys[i - 1] >> 8) == voxel) return;
  if ((long long)voxel >= V) return;
  unsigned best = 0u, best_count = 0u;          // np.argmax of a zeroed counter is 0
  long long pos = i;
  while (pos < n) {
    const unsigned key = keys[pos];
    if ((key >> 8) != voxel) break;
    const long long end = og_run_end(keys, pos, n, key);
    const unsigned count = (unsigned)(end - pos) & 0xFFFFu;          // the reference's counter is uint16
    if (count > best_count) { best_count = count; best = key & 255u; }
    pos = end;
  }
  if (post_empty >= 0) {          // form C: a vote of 0 becomes 255, then the unoccupied id becomes 0
    if (best == 0u) best = 255u;
    if (best == (unsigned)post_empty) best = 0u;
  }
  vol[voxel] = (uint8_t)best;
}

// ---------------------------------------------------------------- the camera visibility of the centres
__device__ __forceinline__ bool og_project(const float* __restrict__ C, float x, float y, float z, int H, int W, int& px, int& py,
                                           int& d10) {
  float u, v, d;
  lidar_project(C, x, y, z, u, v, d);
  if (!(u >= 0.f && u < (float)W && v >= 0.f && v < (float)H && d >= 0.f)) return false;
  const float t = d * 10.f;
  if (!(t < 2048.f)) return false;          // never below the canvas's 2048; covers d*10 >= 32 768, where the int16 cast is undefined
  px = (int)u; py = (int)v; d10 = (int)t;
  return px >= 0 && px < W && py >= 0 && py < H;
}

__global__ __launch_bounds__(256) COOCC_SCALAR_FP32 void k_visible_min(const float* __restrict__ centres, long long N,
                                                                       const float* __restrict__ cams, int ncam, int H, int W,
                                                                       unsigned long long* __restrict__ canvas) {
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  if (i >= N) return;
  const float x = centres[i * 3], y = centres[i * 3 + 1], z = centres[i * 3 + 2];
  for (int cam = 0; cam < ncam; ++cam) {
    int px, py, d10;
    if (!og_project(cams + (size_t)cam * LIDAR_CAM_FLOATS, x, y, z, H, W, px, py, d10)) continue;
    atomicMin(canvas + ((size_t)cam * H + py) * W + px, ((unsigned long long)d10 << 32) | (unsigned long long)i);
  }
}

__global__ __launch_bounds__(256) COOCC_SCALAR_FP32 void k_visible_flag(const float* __restrict__ centres, long long N,
                                                                        const float* __restrict__ cams, int ncam, int H, int W,
                                                                        const unsigned long long* __restrict__ canvas,
                                                                        uint8_t* __restrict__ flags) {
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  if (i >= N) return;
  const float x = centres[i * 3], y = centres[i * 3 + 1], z = centres[i * 3 + 2];
  uint8_t seen = 0;
  for (int cam = 0; cam < ncam; ++cam) {
    int px, py, d10;
    if (!og_project(cams + (size_t)cam * LIDAR_CAM_FLOATS, x, y, z, H, W, px, py, d10)) continue;
    if (canvas[((size_t)cam * H + py) * W + px] == (((unsigned long long)d10 << 32) | (unsigned long long)i)) seen = 1;
  }
  flags[i] = seen;
}

// ---------------------------------------------------------------- aabb
__device__ __forceinline__ unsigned long long og_order_key(double d) {          // increasing with d
  const unsigned long long b = (unsigned long long)__double_as_longlong(d);
  return (b >> 63) ? ~b : (b | (1ull << 63));
}

__device__ __forceinline__ double og_key_value(unsigned long long k) {
  return __longlong_as_double((long long)((k >> 63) ? (k & ~(1ull << 63)) : ~k));
}

__global__ __launch_bounds__(256) void k_cloud_aabb(const float* __restrict__ points, long long P, int stride, OgXf X,
                                                    unsigned long long* __restrict__ slots) {
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  unsigned long long k[6] = {0ull, 0ull, 0ull, 0ull, 0ull, 0ull};          // 0 is below every key and every complement in use
  if (i < P) {
    const float* p = points + (size_t)i * stride;
    const double x = p[0], y = p[1], z = p[2];
    const double e0 = ((X.r1[0] * x + X.r1[1] * y) + X.r1[2] * z) + X.t1[0];
    const double e1 = ((X.r1[3] * x + X.r1[4] * y) + X.r1[5] * z) + X.t1[1];
    const double e2 = ((X.r1[6] * x + X.r1[7] * y) + X.r1[8] * z) + X.t1[2];
    const double g[3] = {((X.r2[0] * e0 + X.r2[1] * e1) + X.r2[2] * e2) + X.t2[0], ((X.r2[3] * e0 + X.r2[4] * e1) + X.r2[5] * e2) + X.t2[1],
                         ((X.r2[6] * e0 + X.r2[7] * e1) + X.r2[8] * e2) + X.t2[2]};
#pragma unroll
    for (int a = 0; a < 3; ++a) {
      const unsigned long long key = og_order_key(g[a]);
      const bool nan = g[a] != g[a];          // numpy's min / max give NaN where a value is NaN: all ones, above every key in use
      k[a] = nan ? ~0ull : ~key;              // the minimum, as a maximum of complements
      k[3 + a] = nan ? ~0ull : key;
    }
  }
#pragma unroll
  for (int a = 0; a < 6; ++a) {
    unsigned long long m = k[a];
    for (int off = COOCC_WAVE / 2; off > 0; off >>= 1) {
      const unsigned long long o = __shfl_xor(m, off, COOCC_WAVE);
      m = o > m ? o : m;
    }
    if ((threadIdx.x & (COOCC_WAVE - 1)) == 0 && m != 0ull) atomicMax(slots + a, m);
  }
}

__global__ void k_aabb_final(const unsigned long long* __restrict__ slots, float* __restrict__ aabb) {
  const int a = threadIdx.x;
  if (a >= 6) return;
  const unsigned long long s = slots[a];
  aabb[a] = s == ~0ull ? __uint_as_float(0x7FC00000u) : (float)og_key_value(a < 3 ? ~s : s);          // the one rounding to fp32
}

static bool og_grid_ok(int G0, int G1, int G2) {
  return G0 >= 1 && G1 >= 1 && G2 >= 1 && G0 <= 65535 && G1 <= 65535 && G2 <= 65535 && (long long)G0 * G1 * G2 <= (1LL << 24);
}

static OgMat og_mat(const float* m) {
  OgMat B;
  for (int i = 0; i < 9; ++i) B.m[i] = m ? m[i] : (i % 4 == 0 ? 1.f : 0.f);
  B.on = m != nullptr;
  return B;
}

}  // namespace

extern "C" int coocc_occ_scatter_labels(const uint16_t* rows, int64_t N, int G0, int G1, int G2, int use_semantic, uint32_t* win,
                                        uint8_t* vol, void* stream) {
  COOCC_CHECK_ARG((rows || N == 0) && win && vol, "occ_scatter_labels: null rows / win / vol");
  COOCC_CHECK_ARG(og_grid_ok(G0, G1, G2), "occ_scatter_labels: grid %d x %d x %d (1 .. 65535 per side, 2^24 voxels at most)", G0, G1, G2);
  COOCC_CHECK_ARG(N >= 0 && N < (1LL << 24) - 1, "occ_scatter_labels: N = %lld rows (below 2^24 - 1)", (long long)N);
  const long long V = (long long)G0 * G1 * G2;
  hipStream_t s = as_stream(stream);
  COOCC_HIP(hipMemsetAsync(win, 0, (size_t)V * sizeof(uint32_t), s));
  if (N > 0) hipLaunchKernelGGL(k_scatter_win, dim3(cdiv(N, 256)), dim3(256), 0, s, rows, (long long)N, G0, G1, G2, use_semantic, win);
  hipLaunchKernelGGL(k_scatter_final, dim3(cdiv(V, 256)), dim3(256), 0, s, (const unsigned int*)win, V, vol);
  COOCC_LAUNCH_CHECK("k_scatter_labels");
  return COOCC_OK;
}

extern "C" int coocc_occ_rows_to_voxels(const uint16_t* rows, int64_t N, const double* grid, const float* bda, int G0, int G1, int G2,
                                        int32_t* vox, uint8_t* labels, float* centres, void* stream) {
  COOCC_CHECK_ARG((rows && vox && labels) || N == 0, "occ_rows_to_voxels: null rows / vox / labels");
  COOCC_CHECK_ARG(grid, "occ_rows_to_voxels: null grid (host doubles lo[3] voxel_size[3])");
  COOCC_CHECK_ARG(og_grid_ok(G0, G1, G2), "occ_rows_to_voxels: grid %d x %d x %d (1 .. 65535 per side, 2^24 voxels at most)", G0, G1, G2);
  COOCC_CHECK_ARG(N >= 0 && N < (1LL << 31), "occ_rows_to_voxels: N = %lld rows", (long long)N);
  if (N == 0) return COOCC_OK;
  OgGrid G;
  for (int a = 0; a < 3; ++a) { G.lo[a] = grid[a]; G.vs[a] = grid[3 + a]; G.hi[a] = 0.0; }
  G.g[0] = G0; G.g[1] = G1; G.g[2] = G2;
  hipLaunchKernelGGL(k_rows_to_voxels, dim3(cdiv(N, 256)), dim3(256), 0, as_stream(stream), rows, (long long)N, G, og_mat(bda), vox, labels,
                     centres);
  COOCC_LAUNCH_CHECK("k_rows_to_voxels");
  return COOCC_OK;
}

extern "C" int coocc_occ_points_to_voxels(const float* points, int64_t P, int point_stride, const uint8_t* seg, const uint8_t* table,
                                          const float* bda, const double* grid, int G0, int G1, int G2, int mode, int32_t* vox,
                                          uint8_t* labels, float* points_occ, void* stream) {
  COOCC_CHECK_ARG(points || P == 0, "occ_points_to_voxels: null points");
  COOCC_CHECK_ARG(mode >= 0 && mode <= 2, "occ_points_to_voxels: mode %d (0 points_occ only, 1 annotation voxels, 2 LiDAR mask voxels)", mode);
  COOCC_CHECK_ARG(P >= 0 && P < (1LL << 31) && point_stride >= 3, "occ_points_to_voxels: P = %lld points of %d floats", (long long)P, point_stride);
  COOCC_CHECK_ARG(!seg || table, "occ_points_to_voxels: lidarseg bytes without the 256-entry table");
  COOCC_CHECK_ARG(mode == 0 || P == 0 || (vox && labels && grid), "occ_points_to_voxels: mode %d needs vox, labels and the grid", mode);
  COOCC_CHECK_ARG(mode == 0 || og_grid_ok(G0, G1, G2), "occ_points_to_voxels: grid %d x %d x %d (1 .. 65535 per side, 2^24 voxels at most)", G0,
                  G1, G2);
  COOCC_CHECK_ARG(mode != 0 || points_occ || P == 0, "occ_points_to_voxels: mode 0 writes points_occ only and it is null");
  if (P == 0) return COOCC_OK;
  OgGrid G;
  for (int a = 0; a < 3; ++a) { G.lo[a] = grid ? grid[a] : 0.0; G.hi[a] = grid ? grid[3 + a] : 0.0; G.vs[a] = grid ? grid[6 + a] : 1.0; }
  G.g[0] = G0; G.g[1] = G1; G.g[2] = G2;
  hipLaunchKernelGGL(k_points_to_voxels, dim3(cdiv(P, 256)), dim3(256), 0, as_stream(stream), points, (long long)P, point_stride, seg, table,
                     og_mat(bda), G, mode, vox, labels, points_occ);
  COOCC_LAUNCH_CHECK("k_points_to_voxels");
  return COOCC_OK;
}

extern "C" size_t coocc_occ_vote_ws(int64_t N) {
  if (N <= 0 || N >= ((int64_t)1 << 31)) return 256;
  size_t tmp = 0;
  (void)rocprim::radix_sort_keys(nullptr, tmp, (unsigned int*)nullptr, (unsigned int*)nullptr, (size_t)N, 0, 32, (hipStream_t)0);
  return 256 + 2 * al256(4 * (size_t)N) + al256(tmp) + 256;
}

extern "C" int coocc_occ_vote_labels(const int32_t* vox, const uint8_t* labels, int64_t N, int64_t V, int fill, int post_empty, uint8_t* vol,
                                     void* ws, size_t ws_bytes, void* stream) {
  COOCC_CHECK_ARG(vol && ((vox && labels && ws) || N == 0), "occ_vote_labels: null pointer");
  COOCC_CHECK_ARG(V >= 1 && V <= (1LL << 24), "occ_vote_labels: V = %lld voxels (2^24 at most: the keys are voxel * 256 + label in 32 bits)",
                  (long long)V);
  COOCC_CHECK_ARG(N >= 0 && N < (1LL << 31), "occ_vote_labels: N = %lld rows", (long long)N);
  COOCC_CHECK_ARG(fill >= 0 && fill <= 255 && post_empty >= -1 && post_empty <= 255, "occ_vote_labels: fill %d, post_empty %d", fill, post_empty);
  hipStream_t s = as_stream(stream);
  COOCC_HIP(hipMemsetAsync(vol, fill, (size_t)V, s));
  if (N == 0) return COOCC_OK;
  const size_t need = coocc_occ_vote_ws(N);
  if (ws_bytes < need) return coocc_set_error(COOCC_ENOMEM, "occ_vote_labels: workspace too small (%zu < %zu bytes)", ws_bytes, need);
  char* b = ws_base256(ws);
  unsigned int* dropped = (unsigned int*)b;
  unsigned int* k_in = (unsigned int*)(b + 256);
  unsigned int* k_out = (unsigned int*)(b + 256 + al256(4 * (size_t)N));
  char* tmp = b + 256 + 2 * al256(4 * (size_t)N);
  size_t tmp_bytes = 0;
  (void)rocprim::radix_sort_keys(nullptr, tmp_bytes, (unsigned int*)nullptr, (unsigned int*)nullptr, (size_t)N, 0, 32, (hipStream_t)0);
  COOCC_HIP(hipMemsetAsync(dropped, 0, 256, s));
  hipLaunchKernelGGL(k_vote_keys, dim3(cdiv(N, 256)), dim3(256), 0, s, vox, labels, (long long)N, (long long)V, k_in, dropped);
  COOCC_LAUNCH_CHECK("k_vote_keys");
  COOCC_HIP(rocprim::radix_sort_keys(tmp, tmp_bytes, k_in, k_out, (size_t)N, 0, 32, s));
  hipLaunchKernelGGL(k_vote_runs, dim3(cdiv(N, 256)), dim3(256), 0, s, (const unsigned int*)k_out, (long long)N, (const unsigned int*)dropped,
                     (long long)V, post_empty, vol);
  COOCC_LAUNCH_CHECK("k_vote_runs");
  return COOCC_OK;
}

extern "C" int coocc_occ_visible_rows(const float* centres, int64_t N, const float* cams, int ncam, int H, int W, uint64_t* canvas,
                                      uint8_t* flags, void* stream) {
  COOCC_CHECK_ARG(((centres && flags) || N == 0) && cams && canvas, "occ_visible_rows: null pointer");
  COOCC_CHECK_ARG(ncam >= 1 && ncam <= 65535, "occ_visible_rows: %d cameras (1 .. 65535)", ncam);
  COOCC_CHECK_ARG(H >= 1 && W >= 1 && H <= 32767 && W <= 32767, "occ_visible_rows: image %d x %d (the reference's pixels are int16)", H, W);
  COOCC_CHECK_ARG(N >= 0 && N < (1LL << 32), "occ_visible_rows: N = %lld rows (the row index is the key's low 32 bits)", (long long)N);
  if (N == 0) return COOCC_OK;
  hipStream_t s = as_stream(stream);
  COOCC_HIP(hipMemsetAsync(canvas, 0xFF, (size_t)ncam * H * W * sizeof(uint64_t), s));
  hipLaunchKernelGGL(k_visible_min, dim3(cdiv(N, 256)), dim3(256), 0, s, centres, (long long)N, cams, ncam, H, W,
                     reinterpret_cast<unsigned long long*>(canvas));
  hipLaunchKernelGGL(k_visible_flag, dim3(cdiv(N, 256)), dim3(256), 0, s, centres, (long long)N, cams, ncam, H, W,
                     reinterpret_cast<const unsigned long long*>(canvas), flags);
  COOCC_LAUNCH_CHECK("k_visible_rows");
  return COOCC_OK;
}

extern "C" int coocc_occ_cloud_aabb(const float* points, int64_t P, int point_stride, const double* transforms, uint64_t* slots, float* aabb,
                                    void* stream) {
  COOCC_CHECK_ARG(points && transforms && slots && aabb, "occ_cloud_aabb: null pointer");
  COOCC_CHECK_ARG(P >= 1 && P < (1LL << 38) && point_stride >= 3, "occ_cloud_aabb: P = %lld points of %d floats (an empty cloud has no box)",
                  (long long)P, point_stride);
  OgXf X;
  for (int i = 0; i < 9; ++i) { X.r1[i] = transforms[i]; X.r2[i] = transforms[12 + i]; }
  for (int i = 0; i < 3; ++i) { X.t1[i] = transforms[9 + i]; X.t2[i] = transforms[21 + i]; }
  hipStream_t s = as_stream(stream);
  COOCC_HIP(hipMemsetAsync(slots, 0, 6 * sizeof(uint64_t), s));
  hipLaunchKernelGGL(k_cloud_aabb, dim3(cdiv(P, 256)), dim3(256), 0, s, points, (long long)P, point_stride, X,
                     reinterpret_cast<unsigned long long*>(slots));
  hipLaunchKernelGGL(k_aabb_final, dim3(1), dim3(64), 0, s, reinterpret_cast<const unsigned long long*>(slots), aabb);
  COOCC_LAUNCH_CHECK("k_cloud_aabb");
  return COOCC_OK;
}
