// The multi-sweep LiDAR cloud from the raw sweeps (co_occ_amd/sweeps.py): mmdet3d 0.17's LoadPointsFromMultiSweeps
// (with LoadPointsFromFile in front of it) -- the key frame with column 4 zeroed, then every chosen sweep filtered by _remove_close,
// rotated and shifted into the key frame's LiDAR frame with numpy's float64 arithmetic and its two roundings to fp32, column 4 the
// time lag, all concatenated in order -- without the merged cloud ever being made on the host.
//
// The input is ONE buffer of raw rows (load_dim floats each) and a table of at most 65 segments (coocc_sweep_seg).  A segment names
// n_rows input rows from in_row0 and the first output row out_row0 they would take if nothing were dropped; segments may name the
// same input rows (pad_empty_sweeps: sweeps_num records on the key frame).  Per row of a segment:
//   filter     dropped where |x| < r and |y| < r in fp32 on the untransformed coordinates (strict; a NaN is never close)
//   transform  xyz = float(double(xyz) @ R^T), every product rounded in fp64, (x0 r0 + x1 r1) + x2 r2; then xyz = float(double(xyz) + t):
//              two roundings to fp32, nearest even, denormal results kept.  Compiled with -ffp-contract=off (build.FILE_FLAGS)
//   column 4   dt (0 for the key frame).  The other columns are copied bit for bit; use_dim picks and orders the output columns
//
// No segment filters: k_sweeps_merge, one launch, a thread an output row; a thread finds its segment by a search over the segment
// starts held in LDS.  Some segment filters: three launches, no atomics, the same bytes from run to run --
//   k_sweeps_count   keep count per tile of 256 rows (ballot + popcount per wave, the four waves summed through LDS)
//   k_sweeps_scan    one workgroup: exclusive scan of the tile counts, the total into *count
//   k_sweeps_merge   the write pass: tile offset + the offsets of the waves before it (LDS) + the rank in the ballot
// so kept rows keep their order (hard voxelisation reads the cloud in row order).  Rows past *count are not written.
//
// The kernels trust nothing in the device table for addressing: an input row outside [0, in_rows) is treated as dropped (filtering)
// or written as zeros (not filtering), an output row is the thread's own index or a scanned rank below it.  The entry checks the host
// copy of the table before it launches.  ~10 MB moved at 11 x 34 720 rows: launch- and latency-bound, 20-byte rows read as dwords.
#include "common.h"

constexpr int SW_TILE = 256;
constexpr int SW_MAX_SEGS = COOCC_SWEEPS_MAX_SEGS;
constexpr int SW_MAX_USE = COOCC_SWEEPS_MAX_USE;

struct sw_cols { int n; int col[SW_MAX_USE]; };

// the segment of output row i: the last s with start[s] <= i (starts ascend, start[0] == 0, empty segments repeat a start)
__device__ __forceinline__ int sw_find(const long long* start, int nseg, long long i) {
  int lo = 0, hi = nseg - 1;
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if (start[mid] <= i) lo = mid; else hi = mid - 1;
  }
  return lo;
}

__device__ __forceinline__ void sw_load_starts(const coocc_sweep_seg* __restrict__ segs, int nseg, long long* start) {
  for (int s = threadIdx.x; s < nseg; s += SW_TILE) start[s] = segs[s].out_row0;
  __syncthreads();
}

// the input row of padded output row i, or -1 where the table does not hold one inside the raw buffer
__device__ __forceinline__ long long sw_in_row(const coocc_sweep_seg& g, long long i, long long in_rows) {
  const long long k = i - g.out_row0;
  if (k < 0 || k >= g.n_rows) return -1;
  const long long r = g.in_row0 + k;
  return (r >= 0 && r < in_rows) ? r : -1;
}

__device__ __forceinline__ bool sw_keep(const coocc_sweep_seg& g, const uint32_t* __restrict__ row, float radius) {
  if (!(g.flags & COOCC_SWEEP_FILTER)) return true;
  const float x = __uint_as_float(row[0]), y = __uint_as_float(row[1]);
  return !(fabsf(x) < radius && fabsf(y) < radius);
}

__global__ __launch_bounds__(SW_TILE) COOCC_SCALAR_FP32 void k_sweeps_count(const uint32_t* __restrict__ raw, long long in_rows, int load_dim,
                                                                             const coocc_sweep_seg* __restrict__ segs, int nseg, long long total,
                                                                             float radius, int32_t* __restrict__ tile_count) {
  __shared__ long long start[SW_MAX_SEGS];
  __shared__ int wave_n[SW_TILE / 64];
  sw_load_starts(segs, nseg, start);
  const long long i = (long long)blockIdx.x * SW_TILE + threadIdx.x;
  bool keep = false;
  if (i < total) {
    const coocc_sweep_seg& g = segs[sw_find(start, nseg, i)];
    const long long r = sw_in_row(g, i, in_rows);
    keep = r >= 0 && sw_keep(g, raw + (size_t)r * load_dim, radius);
  }
  const unsigned long long m = __ballot(keep);
  if ((threadIdx.x & 63) == 0) wave_n[threadIdx.x >> 6] = __popcll(m);
  __syncthreads();
  if (threadIdx.x == 0) tile_count[blockIdx.x] = (wave_n[0] + wave_n[1]) + (wave_n[2] + wave_n[3]);
}

// one workgroup of 256: tile_off[t] = sum of tile_count[< t], *count = the sum of all.  ntiles < 2^23, every sum < 2^31.
__global__ __launch_bounds__(SW_TILE) void k_sweeps_scan(const int32_t* __restrict__ tile_count, int ntiles, int32_t* __restrict__ tile_off,
                                                          int32_t* __restrict__ count) {
  __shared__ int wave_sum[SW_TILE / 64];
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  int carry = 0;
  for (int base = 0; base < ntiles; base += SW_TILE) {
    const int t = base + threadIdx.x;
    const int v = t < ntiles ? tile_count[t] : 0;
    int inc = v;
    for (int d = 1; d < 64; d <<= 1) {
      const int up = __shfl_up(inc, d, 64);
      if (lane >= d) inc += up;
    }
    if (lane == 63) wave_sum[w] = inc;
    __syncthreads();
    int before = 0;
    for (int k = 0; k < w; ++k) before += wave_sum[k];
    const int all = (wave_sum[0] + wave_sum[1]) + (wave_sum[2] + wave_sum[3]);
    if (t < ntiles) tile_off[t] = carry + before + inc - v;
    carry += all;
    __syncthreads();
  }
  if (threadIdx.x == 0) *count = carry;
}

template <bool FILTER>
__global__ __launch_bounds__(SW_TILE) COOCC_SCALAR_FP32 void k_sweeps_merge(const uint32_t* __restrict__ raw, long long in_rows, int load_dim,
                                                                             const coocc_sweep_seg* __restrict__ segs, int nseg, long long total,
                                                                             float radius, sw_cols use, int vec4,
                                                                             const int32_t* __restrict__ tile_off, uint32_t* __restrict__ out,
                                                                             int32_t* __restrict__ count) {
  __shared__ long long start[SW_MAX_SEGS];
  __shared__ int wave_n[SW_TILE / 64];
  sw_load_starts(segs, nseg, start);
  const long long i = (long long)blockIdx.x * SW_TILE + threadIdx.x;
  const coocc_sweep_seg* g = nullptr;
  const uint32_t* row = nullptr;
  bool keep = false;
  if (i < total) {
    g = segs + sw_find(start, nseg, i);
    const long long r = sw_in_row(*g, i, in_rows);
    if (r >= 0) row = raw + (size_t)r * load_dim;
    keep = FILTER ? (row && sw_keep(*g, row, radius)) : true;
  }
  long long o = i;
  if (FILTER) {
    const unsigned long long m = __ballot(keep);
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    if (lane == 0) wave_n[w] = __popcll(m);
    __syncthreads();
    int before = 0;
    for (int k = 0; k < w; ++k) before += wave_n[k];
    o = (long long)tile_off[blockIdx.x] + before + __popcll(m & ((1ull << lane) - 1ull));          // <= i: kept rows before this one
  } else if (i == 0 && count) {
    *count = (int32_t)total;
  }
  if (!keep) return;
  uint32_t v[5] = {0u, 0u, 0u, 0u, 0u};          // columns 0 .. 4 of the output row before use_dim
  if (row) {
    v[0] = row[0]; v[1] = row[1]; v[2] = row[2]; v[3] = row[3];
    if (g->flags & COOCC_SWEEP_TRANSFORM) {
      const double x0 = (double)__uint_as_float(v[0]), x1 = (double)__uint_as_float(v[1]), x2 = (double)__uint_as_float(v[2]);
      for (int j = 0; j < 3; ++j) {
        const double* R = g->R + 3 * j;
        const float rot = (float)((x0 * R[0] + x1 * R[1]) + x2 * R[2]);          // the first rounding to fp32
        v[j] = __float_as_uint((float)((double)rot + g->t[j]));                  // the second
      }
    }
    v[4] = __float_as_uint(g->dt);
  }
  if (vec4) {
    uint4 q;
    q.x = use.col[0] < 5 ? v[use.col[0]] : (row ? row[use.col[0]] : 0u);
    q.y = use.col[1] < 5 ? v[use.col[1]] : (row ? row[use.col[1]] : 0u);
    q.z = use.col[2] < 5 ? v[use.col[2]] : (row ? row[use.col[2]] : 0u);
    q.w = use.col[3] < 5 ? v[use.col[3]] : (row ? row[use.col[3]] : 0u);
    reinterpret_cast<uint4*>(out)[o] = q;
    return;
  }
  uint32_t* dst = out + (size_t)o * use.n;
  for (int j = 0; j < use.n; ++j) {
    const int c = use.col[j];
    dst[j] = c < 5 ? v[c] : (row ? row[c] : 0u);
  }
}


extern "C" size_t coocc_sweeps_merge_ws(int64_t rows) {
  if (rows <= 0) return 256;
  const size_t ntiles = ((size_t)rows + SW_TILE - 1) / SW_TILE;
  return 2 * al256(sizeof(int32_t) * ntiles) + 256;
}

extern "C" int coocc_sweeps_merge(const float* raw, int64_t in_rows, int load_dim, const coocc_sweep_seg* segs,
                                  const coocc_sweep_seg* segs_host, int nseg, const int32_t* use_dim_host, int n_use, float radius, float* out,
                                  int64_t out_rows, int32_t* count, void* ws, size_t ws_bytes, void* stream) {
  COOCC_CHECK_ARG(segs && segs_host && use_dim_host && out, "sweeps_merge: null segs / segs_host / use_dim_host / out");
  COOCC_CHECK_ARG(nseg >= 1 && nseg <= SW_MAX_SEGS, "sweeps_merge: nseg = %d segments (1 .. %d: the key frame and sweeps_num <= 64)", nseg, SW_MAX_SEGS);
  COOCC_CHECK_ARG(load_dim >= 5 && load_dim <= 4096, "sweeps_merge: load_dim = %d floats per row (5 .. 4096)", load_dim);
  COOCC_CHECK_ARG(n_use >= 1 && n_use <= SW_MAX_USE, "sweeps_merge: %d output columns (1 .. %d)", n_use, SW_MAX_USE);
  COOCC_CHECK_ARG(in_rows >= 0 && in_rows < (1LL << 31), "sweeps_merge: in_rows = %lld raw rows (below 2^31)", (long long)in_rows);
  COOCC_CHECK_ARG(raw || in_rows == 0, "sweeps_merge: null raw with in_rows = %lld", (long long)in_rows);          // an empty buffer has no address
  COOCC_CHECK_ARG(radius == radius, "sweeps_merge: radius is NaN");
  sw_cols use;
  use.n = n_use;
  for (int j = 0; j < SW_MAX_USE; ++j) use.col[j] = 0;
  for (int j = 0; j < n_use; ++j) {
    COOCC_CHECK_ARG(use_dim_host[j] >= 0 && use_dim_host[j] < load_dim, "sweeps_merge: use_dim[%d] = %d with load_dim = %d", j, use_dim_host[j], load_dim);
    use.col[j] = use_dim_host[j];
  }
  long long total = 0;
  bool filter = false;
  for (int s = 0; s < nseg; ++s) {
    const coocc_sweep_seg& g = segs_host[s];
    COOCC_CHECK_ARG(g.n_rows >= 0 && g.in_row0 >= 0 && g.in_row0 <= in_rows && g.n_rows <= in_rows - g.in_row0,
                    "sweeps_merge: segment %d names rows %lld + %lld of %lld", s, (long long)g.in_row0, (long long)g.n_rows, (long long)in_rows);
    COOCC_CHECK_ARG(g.out_row0 == total, "sweeps_merge: segment %d starts at output row %lld, the segments before it end at %lld", s,
                    (long long)g.out_row0, total);
    COOCC_CHECK_ARG((g.flags & ~(COOCC_SWEEP_TRANSFORM | COOCC_SWEEP_FILTER)) == 0, "sweeps_merge: segment %d has flags 0x%x", s, (unsigned)g.flags);
    total += g.n_rows;
    COOCC_CHECK_ARG(total < (1LL << 31), "sweeps_merge: %lld output rows and more (below 2^31)", total);
    filter = filter || (g.flags & COOCC_SWEEP_FILTER);
  }
  COOCC_CHECK_ARG(out_rows >= total, "sweeps_merge: out holds %lld rows, the segments have %lld", (long long)out_rows, total);
  COOCC_CHECK_ARG(!filter || count, "sweeps_merge: a filtering segment needs count");
  hipStream_t st = as_stream(stream);
  if (total == 0) {
    if (count) COOCC_HIP(hipMemsetAsync(count, 0, sizeof(int32_t), st));
    return COOCC_OK;
  }
  const unsigned ntiles = cdiv(total, SW_TILE);
  const int vec4 = n_use == 4 && ((uintptr_t)out & 15) == 0;
  const uint32_t* rawu = reinterpret_cast<const uint32_t*>(raw);
  uint32_t* outu = reinterpret_cast<uint32_t*>(out);
  if (!filter) {
    hipLaunchKernelGGL(k_sweeps_merge<false>, dim3(ntiles), dim3(SW_TILE), 0, st, rawu, (long long)in_rows, load_dim, segs, nseg, total, radius,
                       use, vec4, (const int32_t*)nullptr, outu, count);
    COOCC_LAUNCH_CHECK("k_sweeps_merge");
    return COOCC_OK;
  }
  if (!ws || ws_bytes < coocc_sweeps_merge_ws(total)) return coocc_set_error(COOCC_ENOMEM, "sweeps_merge: workspace too small");
  char* c = ws_base256(ws);
  int32_t* tile_count = (int32_t*)c;
  int32_t* tile_off = (int32_t*)(c + al256(sizeof(int32_t) * (size_t)ntiles));
  hipLaunchKernelGGL(k_sweeps_count, dim3(ntiles), dim3(SW_TILE), 0, st, rawu, (long long)in_rows, load_dim, segs, nseg, total, radius, tile_count);
  COOCC_LAUNCH_CHECK("k_sweeps_count");
  hipLaunchKernelGGL(k_sweeps_scan, dim3(1), dim3(SW_TILE), 0, st, tile_count, (int)ntiles, tile_off, count);
  COOCC_LAUNCH_CHECK("k_sweeps_scan");
  hipLaunchKernelGGL(k_sweeps_merge<true>, dim3(ntiles), dim3(SW_TILE), 0, st, rawu, (long long)in_rows, load_dim, segs, nseg, total, radius, use,
                     vec4, tile_off, outu, count);
  COOCC_LAUNCH_CHECK("k_sweeps_merge");
  return COOCC_OK;
}
