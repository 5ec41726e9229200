// Occupancy pictures without OpenGL: the cubes of P/visualize/visualize_nusc.py (draw_nusc_occupancy) ray-cast on the device.
// co_occ_amd/visualize.py is the caller; DESIGN.md 19 has the definition of the picture and the argument why skipping empty space
// cannot change it.
//
//   labels [X][Y][Z] uint8 or int64 (upstream's argmax)
//   draw   [X][Y][Z] uint8: label 17 -> 20, then the ego-car block (labels 17 / 18 / 19) over the centre; drawn iff 0 < v < 20
//   masks  one buffer: col  uint16 [X][Y][zw], zw = ceil(Z / 16): bit k & 15 of word k >> 4 = cell (x, y, k) is drawn
//                      brick uint8 [bx][by][zw], bx = ceil(X / 8), by = ceil(Y / 8): any drawn cell in the 8 x 8 columns of that word
//          (col first, each part rounded up to 16 bytes)
//
// coocc_occ_view_prepare: one launch, a wave per 8 x 8 columns (a lane per column): the lane writes its draw bytes and its words, a
// ballot decides the brick byte.  No atomics, no host read.
//
// coocc_occ_view_cast: one launch for all views of a call.  A workgroup stages the masks once -- col and brick when they fit the
// LDS budget (16 KiB by default; up to 80 KiB on request: 200 x 200 x 16 is 80 000 + 640 bytes, two workgroups per CU), brick alone
// otherwise (col is then read through L2) -- and walks over 16 x 16 pixel tiles; a thread owns a pixel and casts its S x S samples one after the other.  The walk has three
// box sizes: an empty brick (8 x 8 x 16 cells) and an empty column word (1 x 1 x 16) are left in one step, a cell in one step; the
// slab test runs only in cells whose bit is set.  The exit plane of a box is org + (float)index * voxel_size from the integer
// plane index, never an accumulated position.
//
// The hit of a sample is a function of the ray and of the cube alone (ov_slab, every fp32 operation in the order written there,
// no contraction: build.py FILE_FLAGS), the winner among cubes is the smallest (t, linear voxel index): tests/occ_view_refs.py
// restates both over ALL drawn cubes and the kernel's ids, faces, t and bytes equal it.  The walk only chooses which cubes are asked.
#include <math.h>

#include "common.h"
#include "occ_views_walk.h"

constexpr int OV_LDS_SMALL = 16384;        // static LDS of the usual forms: brick alone, or col + brick where both fit; 8 workgroups a CU
constexpr int OV_LDS_LARGE = 81920;        // static LDS of the form a caller's budget asks for: col + brick of 200 x 200 x 16, 2 a CU
constexpr int OV_TILE = 16;                // 16 x 16 pixels a workgroup pass; a wave is 16 x 4 of them
constexpr int OV_MAX_SAMPLES = 8;

static inline size_t al16(size_t n) { return (n + 15) & ~(size_t)15; }

template <typename T>
__global__ __launch_bounds__(256) COOCC_SCALAR_FP32 void k_occ_view_prepare(const T* __restrict__ labels, int X, int Y, int Z, int zw, int bx, int by,
                                                          uint8_t* __restrict__ draw, uint16_t* __restrict__ col,
                                                          uint8_t* __restrict__ brick) {
  const int b = blockIdx.x * 4 + (threadIdx.x >> 6);          // wave-uniform: the whole wave leaves or stays
  if (b >= bx * by) return;
  const int lane = threadIdx.x & 63;
  const int x = (b / by) * 8 + (lane >> 3), y = (b % by) * 8 + (lane & 7);
  const bool valid = x < X && y < Y;
  for (int w = 0; w < zw; ++w) {
    unsigned word = 0;
    if (valid) {
      const size_t base = ((size_t)x * Y + y) * Z;
      const int k1 = min(Z, w * 16 + 16);
      for (int k = w * 16; k < k1; ++k) {
        int v = (int)(uint8_t)labels[base + k];
        if (v == 17) v = 20;
        const int car = ov_car_label(x, y, k, X, Y, Z);
        if (car >= 0) v = car;
        draw[base + k] = (uint8_t)v;
        if (v > 0 && v < 20) word |= 1u << (k & 15);
      }
      col[((size_t)x * Y + y) * zw + w] = (uint16_t)word;
    }
    const bool any = __ballot(word != 0) != 0;
    if (lane == 0) brick[(size_t)b * zw + w] = any ? 1 : 0;
  }
}

// faces: 0 +x, 1 -x, 2 +y, 3 -y, 4 +z, 5 -z
__constant__ int OV_SHADE[6] = {208, 208, 168, 168, 256, 128};

template <int LDS_BYTES, bool CELLS_LDS>
__global__ __launch_bounds__(256) COOCC_SCALAR_FP32 void k_occ_view_cast(const OvParams p, const uint8_t* __restrict__ draw,
                                                                         const uint32_t* __restrict__ masks, uint8_t* __restrict__ rgb,
                                                                         int32_t* __restrict__ ids, uint8_t* __restrict__ faces,
                                                                         float* __restrict__ tout, uint32_t* __restrict__ reads) {
  __shared__ __attribute__((aligned(16))) uint32_t s_m[LDS_BYTES / 4];
  if (CELLS_LDS) {
    for (int i = threadIdx.x; i < p.col_words + p.brick_words; i += 256) s_m[i] = masks[i];
  } else {
    for (int i = threadIdx.x; i < p.brick_words; i += 256) s_m[i] = masks[p.col_words + i];
  }
  __syncthreads();
  const uint16_t* col = CELLS_LDS ? reinterpret_cast<const uint16_t*>(s_m) : reinterpret_cast<const uint16_t*>(masks);
  const uint8_t* brick = reinterpret_cast<const uint8_t*>(s_m + (CELLS_LDS ? p.col_words : 0));

  const int tiles_x = (p.W + OV_TILE - 1) / OV_TILE, tiles_y = (p.H + OV_TILE - 1) / OV_TILE;
  const int ntiles = p.V * tiles_x * tiles_y;
  const int HS = p.H * p.S, WS = p.W * p.S;

  for (int tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
    const int v = tile / (tiles_x * tiles_y), rem = tile - v * tiles_x * tiles_y;
    const int px = (rem % tiles_x) * OV_TILE + (threadIdx.x & 15), py = (rem / tiles_x) * OV_TILE + (threadIdx.x >> 4);
    if (px >= p.W || py >= p.H) continue;
    const OvView& vw = p.view[v];
    unsigned sum[3] = {0, 0, 0};
    for (int sy = 0; sy < p.S; ++sy) {
      for (int sx = 0; sx < p.S; ++sx) {
        const int gx = (vw.col0 + px) * p.S + sx, gy = py * p.S + sy;
        float best_t;
        int best_id, best_face;
        unsigned nread[2];
        ov_cast_sample(p, vw, col, brick, gx, gy, best_id, best_face, best_t, nread);
        if (ids) {
          const size_t o = ((size_t)v * HS + gy) * WS + (size_t)px * p.S + sx;
          ids[o] = best_id; faces[o] = (uint8_t)best_face; tout[o] = best_t;
          if (reads) { reads[2 * o] = nread[0]; reads[2 * o + 1] = nread[1]; }
        }
        if (best_id >= 0) {
          const int cidx = (int)draw[best_id] - 1, sh8 = OV_SHADE[best_face];
#pragma unroll
          for (int k = 0; k < 3; ++k) sum[k] += ((unsigned)p.palette[cidx * 3 + k] * sh8 + 128) >> 8;
        } else {
          sum[0] += 255; sum[1] += 255; sum[2] += 255;
        }
      }
    }
    const unsigned n = p.S * p.S;
    uint8_t* o = rgb + (((size_t)v * p.H + py) * p.W + px) * 3;
#pragma unroll
    for (int k = 0; k < 3; ++k) o[k] = (uint8_t)((sum[k] + n / 2) / n);
  }
}

static bool ov_grid_ok(int X, int Y, int Z) {
  return X >= 12 && Y >= 12 && Z >= 10 && X <= 4096 && Y <= 4096 && Z <= 4096 && (long long)X * Y * Z < (1ll << 31);
}

extern "C" int64_t coocc_occ_view_prepare(const void* labels, int labels_i64, int X, int Y, int Z, uint8_t* draw, void* masks,
                                          size_t masks_bytes, void* stream) {
  COOCC_CHECK_ARG(ov_grid_ok(X, Y, Z), "occ_view_prepare: grid %d x %d x %d: X, Y >= 12 and Z >= 10 (the ego-car block), < 2^31 voxels", X,
                  Y, Z);
  const int zw = (Z + 15) / 16, bx = (X + 7) / 8, by = (Y + 7) / 8;
  const size_t col_bytes = al16((size_t)X * Y * zw * 2), brick_bytes = al16((size_t)bx * by * zw);
  if (!masks) return (int64_t)(col_bytes + brick_bytes);
  COOCC_CHECK_ARG(labels && draw, "occ_view_prepare: null labels or draw volume");
  COOCC_CHECK_ARG(((uintptr_t)masks & 15) == 0, "occ_view_prepare: masks must be 16-byte aligned");
  if (masks_bytes < col_bytes + brick_bytes)
    return coocc_set_error(COOCC_ENOMEM, "occ_view_prepare: masks too small (%zu < %zu bytes)", masks_bytes, col_bytes + brick_bytes);
  uint16_t* col = (uint16_t*)masks;
  uint8_t* brick = (uint8_t*)masks + col_bytes;
  hipStream_t s = as_stream(stream);
  if (labels_i64)
    hipLaunchKernelGGL(k_occ_view_prepare<int64_t>, dim3(cdiv(bx * by, 4)), dim3(256), 0, s, (const int64_t*)labels, X, Y, Z, zw, bx, by,
                       draw, col, brick);
  else
    hipLaunchKernelGGL(k_occ_view_prepare<uint8_t>, dim3(cdiv(bx * by, 4)), dim3(256), 0, s, (const uint8_t*)labels, X, Y, Z, zw, bx, by,
                       draw, col, brick);
  COOCC_LAUNCH_CHECK("k_occ_view_prepare");
  return COOCC_OK;
}

extern "C" int coocc_occ_view_cast(const uint8_t* draw, const void* masks, int X, int Y, int Z, const float* grid_host,
                                   const float* views_host, int V, int H, int W, int S, int FW, int FH, const uint8_t* palette_host,
                                   size_t lds_budget_bytes, uint8_t* rgb, int32_t* ids, uint8_t* faces, float* t, uint32_t* reads, void* stream) {
  COOCC_CHECK_ARG(ov_grid_ok(X, Y, Z), "occ_view_cast: grid %d x %d x %d: X, Y >= 12 and Z >= 10 (the ego-car block), < 2^31 voxels", X, Y, Z);
  COOCC_CHECK_ARG(V >= 1 && V <= OV_MAX_VIEWS, "occ_view_cast: 1 <= V <= %d views a call", OV_MAX_VIEWS);
  COOCC_CHECK_ARG(H >= 1 && W >= 1 && S >= 1 && S <= OV_MAX_SAMPLES && FW >= W && FH >= H && FW <= 16384 && FH <= 16384,
                  "occ_view_cast: 1 <= H <= FH, 1 <= W <= FW <= 16384, 1 <= S <= %d", OV_MAX_SAMPLES);
  COOCC_CHECK_ARG((long long)V * H * S * W * S < (1ll << 31), "occ_view_cast: V * H * W * S * S must stay below 2^31 samples");
  COOCC_CHECK_ARG(draw && masks && grid_host && views_host && palette_host && rgb, "occ_view_cast: null draw, masks, grid, views, palette or rgb");
  COOCC_CHECK_ARG((ids != nullptr) == (faces != nullptr) && (ids != nullptr) == (t != nullptr),
                  "occ_view_cast: ids, faces and t come together (all or none)");
  COOCC_CHECK_ARG(!reads || ids, "occ_view_cast: reads comes with ids, faces and t");
  COOCC_CHECK_ARG(((uintptr_t)masks & 15) == 0, "occ_view_cast: masks must be 16-byte aligned");
  OvParams p;
  p.V = V; p.H = H; p.W = W; p.S = S; p.FW = FW; p.FH = FH;
  p.rw = (float)(1.0 / ((double)FW * S)); p.rh = (float)(1.0 / ((double)FH * S));
  p.X = X; p.Y = Y; p.Z = Z; p.zw = (Z + 15) / 16; p.by = (Y + 7) / 8;
  const size_t col_bytes = al16((size_t)X * Y * p.zw * 2), brick_bytes = al16((size_t)((X + 7) / 8) * p.by * p.zw);
  p.col_words = (int)(col_bytes / 4); p.brick_words = (int)(brick_bytes / 4);
  for (int a = 0; a < 3; ++a) {
    p.org[a] = grid_host[a]; p.vs[a] = grid_host[3 + a];
    COOCC_CHECK_ARG(p.vs[a] > 0.f && isfinite(p.vs[a]) && isfinite(p.org[a]), "occ_view_cast: voxel sizes must be positive and finite");
    p.rvs[a] = (float)(1.0 / (double)p.vs[a]);
  }
  p.half = grid_host[6];
  COOCC_CHECK_ARG(p.half > 0.f && 2.f * p.half <= fminf(p.vs[0], fminf(p.vs[1], p.vs[2])),
                  "occ_view_cast: the cube edge %g does not fit the smallest voxel side", 2.0 * p.half);
  for (int v = 0; v < V; ++v) {
    const float* s = views_host + 16 * v;
    OvView& o = p.view[v];
    for (int a = 0; a < 3; ++a) { o.eye[a] = s[a]; o.fwd[a] = s[3 + a]; o.R[a] = s[6 + a]; o.U[a] = s[9 + a]; }
    o.near = s[12]; o.far = s[13]; o.col0 = (int)s[14]; o.pad = 0;
    for (int k = 0; k < 14; ++k) COOCC_CHECK_ARG(isfinite(s[k]), "occ_view_cast: view %d has a non-finite entry", v);
    COOCC_CHECK_ARG(o.near > 0.f && o.far >= o.near, "occ_view_cast: view %d: 0 < near <= far", v);
    COOCC_CHECK_ARG(o.col0 >= 0 && o.col0 + W <= FW && (float)o.col0 == s[14], "occ_view_cast: view %d: column window outside the frame", v);
  }
  for (int i = 0; i < 57; ++i) p.palette[i] = palette_host[i];
  // Where the column words are read.  Measured (profiles/occ_views_bench.json): with 80 KiB a workgroup a CU holds two of them and
  // the six camera views of 200 x 200 x 16 take 8.9 ms; with the words read from memory and eight workgroups a CU, 3.8 ms.  So the
  // default stages the words only where that costs no occupancy; the large form runs when the caller's budget asks for it.
  const size_t budget = lds_budget_bytes ? std::min<size_t>(lds_budget_bytes, OV_LDS_LARGE) : (size_t)OV_LDS_SMALL;
  const bool cells_lds = col_bytes + brick_bytes <= budget, large = cells_lds && col_bytes + brick_bytes > (size_t)OV_LDS_SMALL;
  COOCC_CHECK_ARG(cells_lds || brick_bytes <= (size_t)OV_LDS_SMALL, "occ_view_cast: the brick mask (%zu bytes) does not fit %d bytes of LDS",
                  brick_bytes, OV_LDS_SMALL);
  const long long ntiles = (long long)V * cdiv(W, OV_TILE) * cdiv(H, OV_TILE);
  // workgroups walk over tiles: as many as a CU holds at once
  int dev = 0, cus = 0;
  COOCC_HIP(hipGetDevice(&dev));
  COOCC_HIP(hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev));
  const int grid = (int)std::min<long long>(ntiles, (long long)std::max(cus, 1) * (large ? 2 : 8));
  hipStream_t s = as_stream(stream);
  const uint32_t* m = (const uint32_t*)masks;
  if (large)
    hipLaunchKernelGGL((k_occ_view_cast<OV_LDS_LARGE, true>), dim3(grid), dim3(256), 0, s, p, draw, m, rgb, ids, faces, t, reads);
  else if (cells_lds)
    hipLaunchKernelGGL((k_occ_view_cast<OV_LDS_SMALL, true>), dim3(grid), dim3(256), 0, s, p, draw, m, rgb, ids, faces, t, reads);
  else
    hipLaunchKernelGGL((k_occ_view_cast<OV_LDS_SMALL, false>), dim3(grid), dim3(256), 0, s, p, draw, m, rgb, ids, faces, t, reads);
  COOCC_LAUNCH_CHECK("k_occ_view_cast");
  return cells_lds ? COOCC_OK : 1;
}
