// Camera img_inputs from decoded uint8 frames (co_occ_amd/image_inputs.py): the per-pixel half of the reference's
// LoadMultiViewImageFromFiles_OccFormer (P/datasets/pipelines/loading_nusc_imgs.py:70-77, 185-188) -- Pillow's Image.resize
// (bicubic, anti-aliased), Image.crop, FLIP_LEFT_RIGHT and `uint8.float() / 255.` -- with Pillow's bits.
//
// Pillow's 8-bit resize is integer arithmetic once its coefficient tables exist (the host makes them in float64 and rounds them to
// 22-bit fixed point, image_inputs.pillow_coeffs): per output index a first source index, a tap count and the taps; a pass is
//   acc = 2^21 + sum_k src[xmin + k] * tap[k];   out = clamp(acc >> 22, 0, 255)        (int32; 255 * sum|tap| < 2^31 for bicubic)
// horizontal pass first, ROUNDED TO uint8, then the vertical pass; a pass whose size does not change is skipped.  Then the crop
// (zeros outside the resized image), the column mirror, and fp32 = __fdiv_rn(float(byte), 255.f): a true division, a reciprocal
// multiply gives other bits.  Channel k of the output is byte k of the input.
//
// k_frames_to_imgs: one workgroup per camera and 16 x 64 output tile; only what the crop keeps is computed.
//   1. the tile's taps (64 columns, 16 rows) go into LDS, clamped to the source so that a malformed table cannot index outside;
//   2. the source rows the tile's vertical taps span are walked `srows` at a time: the byte rectangle the horizontal taps span is
//      staged into LDS with 16-byte loads (a byte path where a 16-byte chunk would leave the frame), the horizontal pass writes
//      uint8 into the LDS H image [rows][64][3]; a thread makes the three channels of one pixel, so a tap is read once for three;
//   3. the vertical pass reads the H image and writes the tile's bytes into LDS;
//   4. the three fp32 planes are written along W, the canvas as whole tile rows of bytes.
// The staging buffer, the H image and the output tile are dynamic LDS, sized by the launcher from the call's largest ratios (the
// span of n outputs is below (n - 1) * scale + 2 * support + 1): 19.6 KB at the r50 shape (ratio 2.27: 16 staged rows of 496 bytes,
// 45 H-image rows), 38.3 KB at the limit of 8 (4 staged rows of 1648 bytes, 154 H-image rows); the taps take 11.3 KB more.
// No atomics and a fixed order: the same bits from run to run.  k_frames_crop is the unresized form (r101: resize 1.0, crop of four
// rows): a crop-and-convert pass with no LDS, taken when no camera of the call resizes; four pixels per thread (three 4-byte loads,
// three 16-byte stores, three 4-byte canvas stores) where the width and the addresses allow, one pixel otherwise.
#include <algorithm>

#include "common.h"

constexpr int II_TW = 64, II_TH = 16;        // output tile
constexpr int II_KMAX = 33;                  // taps per output index: bicubic at a downscale ratio of 8
constexpr int II_MAX_RATIO = 8;
constexpr int II_VSPAN = 160;                // H-image rows at most: 15 * 8 + 2 * 16 + 1 = 153 at the limit
constexpr int II_HSPAN = 544;                // staged source pixels per row at most: 63 * 8 + 2 * 16 + 1 = 537 at the limit
constexpr int II_STAGE_BYTES = 8192;         // the staging buffer holds as many rows as fit in this (1 .. 16)
constexpr int II_CAM_INTS = 12;              // per-camera header: newW newH crop_x0 crop_y0 flip htab hk vtab vk 0 0 0

// bytes per staged row: the span plus the 16-byte alignment slack on both sides, a multiple of 16
__host__ __device__ __forceinline__ int ii_sstride(int hcap) { return (hcap * 3 + 32 + 15) & ~15; }

__device__ __forceinline__ int ii_clamp(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }
__device__ __forceinline__ uint8_t ii_clip8(int acc) { return (uint8_t)ii_clamp(acc >> 22, 0, 255); }

// bounds (first index, count) and taps of output indices [first, first + count) of one table into LDS, clamped to [0, in_size)
__device__ __forceinline__ void ii_load_table(const int* __restrict__ T, int out_size, int ksize, int in_size, int first, int count,
                                              int* __restrict__ s_b, int* __restrict__ s_t) {
  for (int i = threadIdx.x; i < count; i += blockDim.x) {
    const int lo = ii_clamp(T[2 * (first + i)], 0, in_size);
    s_b[2 * i] = lo;
    s_b[2 * i + 1] = ii_clamp(T[2 * (first + i) + 1], 0, min(ksize, in_size - lo));
  }
  const int* taps = T + 2 * (size_t)out_size;
  for (int i = threadIdx.x; i < count * II_KMAX; i += blockDim.x) {
    const int j = i / II_KMAX, k = i - j * II_KMAX;
    s_t[i] = k < ksize ? taps[(size_t)(first + j) * ksize + k] : 0;
  }
}

// the source span [lo, lo + len) that `count` table entries cover, cut to `cap`; entries are trimmed to it
__device__ __forceinline__ void ii_span(int* __restrict__ s_b, int count, int cap, int& lo, int& len) {
  int a = 0x7fffffff, b = 0;
  for (int i = 0; i < count; ++i) {
    a = min(a, s_b[2 * i]);
    b = max(b, s_b[2 * i] + s_b[2 * i + 1]);
  }
  lo = a;
  len = ii_clamp(b - a, 0, cap);
  __syncthreads();
  for (int i = threadIdx.x; i < count; i += blockDim.x) s_b[2 * i + 1] = ii_clamp(s_b[2 * i + 1], 0, len - (s_b[2 * i] - a));
  __syncthreads();
}

// hcap / vcap: source pixels per staged row / H-image rows the dynamic LDS was sized for; srows: staged rows per round
__global__ __launch_bounds__(256) void k_frames_to_imgs(const uint8_t* __restrict__ frames, const uint8_t* const* __restrict__ frame_ptrs,
                                                        int Hs, int Ws, const int* __restrict__ params, const int* __restrict__ tables,
                                                        int fH, int fW, float* __restrict__ imgs, uint8_t* __restrict__ canvas, int hcap,
                                                        int vcap, int srows) {
  extern __shared__ __attribute__((aligned(16))) uint8_t s_dyn[];
  __shared__ int s_ht[II_TW * II_KMAX], s_vt[II_TH * II_KMAX], s_hb[II_TW * 2], s_vb[II_TH * 2];
  const int sstride = ii_sstride(hcap);
  uint8_t* const s_src = s_dyn;                                   // [srows][sstride]
  uint8_t* const s_h = s_src + srows * sstride;                   // [vcap][64][3]
  uint8_t* const s_out = s_h + vcap * (II_TW * 3);                // [16][64][3]
  const int cam = blockIdx.z, tid = threadIdx.x;
  const int* P = params + cam * II_CAM_INTS;
  const int newW = P[0], newH = P[1], cx0 = P[2], cy0 = P[3], flip = P[4], htab = P[5], hk = P[6], vtab = P[7], vk = P[8];
  const bool hpass = htab >= 0, vpass = vtab >= 0;
  const size_t frame_bytes = (size_t)Hs * Ws * 3;
  const uint8_t* src = frame_ptrs ? frame_ptrs[cam] : frames + (size_t)cam * frame_bytes;
  const int tx0 = blockIdx.x * II_TW, ty0 = blockIdx.y * II_TH;
  const int tw = min(II_TW, fW - tx0), th = min(II_TH, fH - ty0);
  // the tile in the resized image: columns [rx_lo, rx_lo + tw), rows [ry_lo, ry_lo + th); [rxa, rxb] x [rya, ryb] is the part inside it
  const int rx_lo = cx0 + (flip ? fW - tx0 - tw : tx0), ry_lo = cy0 + ty0;
  const int rxa = max(rx_lo, 0), rxb = min(rx_lo + tw - 1, newW - 1), rya = max(ry_lo, 0), ryb = min(ry_lo + th - 1, newH - 1);
  const int nx = rxb - rxa + 1, ny = ryb - rya + 1;
  const bool any = nx > 0 && ny > 0;          // uniform over the workgroup
  if (any) {
    if (hpass) ii_load_table(tables + htab, newW, hk, Ws, rxa, nx, s_hb, s_ht);
    if (vpass) ii_load_table(tables + vtab, newH, vk, Hs, rya, ny, s_vb, s_vt);
    __syncthreads();
    int c0 = rxa, ncols = nx, r0 = rya, nrows = ny;          // ny <= 16 <= vcap
    if (hpass) ii_span(s_hb, nx, hcap, c0, ncols);
    if (vpass) ii_span(s_vb, ny, vcap, r0, nrows);
    if (!hpass) {          // the H image is the source itself
      for (int idx = tid; idx < nrows * nx * 3; idx += 256) {
        const int i = idx / (nx * 3), b = idx - i * (nx * 3);
        s_h[i * (II_TW * 3) + b] = src[((size_t)(r0 + i) * Ws + rxa) * 3 + b];
      }
    } else {
      const int len = ncols * 3, cpr = (len + 30) / 16;          // 16-byte chunks a staged row can take: cpr * 16 <= sstride
      for (int rb = 0; rb < nrows; rb += srows) {
        const int rows = min(srows, nrows - rb);
        for (int idx = tid; idx < rows * cpr; idx += 256) {
          const int i = idx / cpr, j = idx - i * cpr;
          const uint8_t* a0 = src + ((size_t)(r0 + rb + i) * Ws + c0) * 3;          // first byte the row needs
          const uint8_t* p = a0 - ((uintptr_t)a0 & 15) + 16 * j;
          if (p >= a0 + len) continue;
          uint4 v;
          if (p >= src && p + 16 <= src + frame_bytes) {
            v = *reinterpret_cast<const uint4*>(p);
          } else {          // a chunk that would leave the frame: only the bytes the row needs, one at a time
            uint32_t w[4] = {0, 0, 0, 0};
            for (int b = 0; b < 16; ++b)
              if (p + b >= a0 && p + b < a0 + len) w[b >> 2] |= (uint32_t)p[b] << (8 * (b & 3));
            v = make_uint4(w[0], w[1], w[2], w[3]);
          }
          *reinterpret_cast<uint4*>(s_src + i * sstride + 16 * j) = v;
        }
        __syncthreads();
        for (int idx = tid; idx < rows * nx; idx += 256) {          // one pixel of the H image: three channels share the taps
          const int i = idx / nx, j = idx - i * nx;
          const uint8_t* a0 = src + ((size_t)(r0 + rb + i) * Ws + c0) * 3;
          const uint8_t* p = s_src + i * sstride + ((uintptr_t)a0 & 15) + (s_hb[2 * j] - c0) * 3;
          const int n = s_hb[2 * j + 1];
          const int* t = s_ht + j * II_KMAX;
          int acc0 = 1 << 21, acc1 = 1 << 21, acc2 = 1 << 21;
          for (int k = 0; k < n; ++k) {
            const int w = t[k];
            acc0 += (int)p[3 * k] * w;
            acc1 += (int)p[3 * k + 1] * w;
            acc2 += (int)p[3 * k + 2] * w;
          }
          uint8_t* o = s_h + ((rb + i) * II_TW + j) * 3;
          o[0] = ii_clip8(acc0); o[1] = ii_clip8(acc1); o[2] = ii_clip8(acc2);
        }
        __syncthreads();
      }
    }
    __syncthreads();
    for (int idx = tid; idx < th * tw; idx += 256) {
      const int oy = idx / tw, ox = idx - oy * tw;
      const int rx = rx_lo + (flip ? tw - 1 - ox : ox), ry = ry_lo + oy;
      uint8_t o0 = 0, o1 = 0, o2 = 0;
      if (rx >= rxa && rx <= rxb && ry >= rya && ry <= ryb) {
        const int j = rx - rxa, r = ry - rya;
        if (vpass) {
          const uint8_t* p = s_h + ((s_vb[2 * r] - r0) * II_TW + j) * 3;
          const int n = s_vb[2 * r + 1];
          const int* t = s_vt + r * II_KMAX;
          int acc0 = 1 << 21, acc1 = 1 << 21, acc2 = 1 << 21;
          for (int k = 0; k < n; ++k) {
            const int w = t[k];
            const uint8_t* q = p + k * (II_TW * 3);
            acc0 += (int)q[0] * w;
            acc1 += (int)q[1] * w;
            acc2 += (int)q[2] * w;
          }
          o0 = ii_clip8(acc0); o1 = ii_clip8(acc1); o2 = ii_clip8(acc2);
        } else {
          const uint8_t* q = s_h + (r * II_TW + j) * 3;
          o0 = q[0]; o1 = q[1]; o2 = q[2];
        }
      }
      uint8_t* o = s_out + (oy * II_TW + ox) * 3;
      o[0] = o0; o[1] = o1; o[2] = o2;
    }
  } else {
    for (int idx = tid; idx < II_TH * II_TW * 3; idx += 256) s_out[idx] = 0;
  }
  __syncthreads();
  for (int idx = tid; idx < 3 * th * tw; idx += 256) {
    const int c = idx / (th * tw), rem = idx - c * (th * tw), oy = rem / tw, ox = rem - oy * tw;
    imgs[(((size_t)cam * 3 + c) * fH + ty0 + oy) * fW + tx0 + ox] = __fdiv_rn((float)s_out[(oy * II_TW + ox) * 3 + c], 255.f);
  }
  if (canvas)
    for (int idx = tid; idx < th * tw * 3; idx += 256) {
      const int oy = idx / (tw * 3), b = idx - oy * (tw * 3);
      canvas[(((size_t)cam * fH + ty0 + oy) * fW + tx0) * 3 + b] = s_out[oy * (II_TW * 3) + b];
    }
}

// no camera resizes: crop (zeros outside), mirror, convert.  A thread takes V consecutive output pixels of one row, W fastest.
// V == 4: fW % 4 == 0, imgs 16-byte and canvas 4-byte aligned (the launcher checks), so the stores are whole 16 / 4 bytes.
template <int V>
__global__ __launch_bounds__(256) void k_frames_crop(const uint8_t* __restrict__ frames, const uint8_t* const* __restrict__ frame_ptrs, int Hs,
                                                     int Ws, const int* __restrict__ params, int fH, int fW, float* __restrict__ imgs,
                                                     uint8_t* __restrict__ canvas) {
  const int cam = blockIdx.z, oy = blockIdx.y, ox0 = (blockIdx.x * 256 + threadIdx.x) * V;
  if (ox0 >= fW) return;
  const int* P = params + cam * II_CAM_INTS;
  const int cx0 = P[2], flip = P[4], ry = P[3] + oy;
  const uint8_t* src = frame_ptrs ? frame_ptrs[cam] : frames + (size_t)cam * Hs * Ws * 3;
  const bool row_in = ry >= 0 && ry < Hs;
  uint8_t v[V * 3];
  bool loaded = false;
  if constexpr (V == 4) {
    const int rx0 = cx0 + ox0;
    if (row_in && !flip && rx0 >= 0 && rx0 + V <= Ws) {
      const uint8_t* p = src + ((size_t)ry * Ws + rx0) * 3;
      if (((uintptr_t)p & 3) == 0) {          // the 12 bytes of the four pixels as three words
        const uint32_t* w = reinterpret_cast<const uint32_t*>(p);
#pragma unroll
        for (int i = 0; i < 3; ++i) {
          const uint32_t x = w[i];
          v[4 * i] = x & 255; v[4 * i + 1] = (x >> 8) & 255; v[4 * i + 2] = (x >> 16) & 255; v[4 * i + 3] = x >> 24;
        }
        loaded = true;
      }
    }
  }
  if (!loaded) {
#pragma unroll
    for (int q = 0; q < V; ++q) {
      const int rx = cx0 + (flip ? fW - 1 - (ox0 + q) : ox0 + q);
      const bool in = row_in && rx >= 0 && rx < Ws;
      const uint8_t* p = src + ((size_t)(in ? ry : 0) * Ws + (in ? rx : 0)) * 3;
#pragma unroll
      for (int c = 0; c < 3; ++c) v[3 * q + c] = in ? p[c] : (uint8_t)0;
    }
  }
  const size_t pix = ((size_t)cam * fH + oy) * fW + ox0, plane = (size_t)fH * fW;
  float* o = imgs + ((size_t)cam * 3 * fH + oy) * fW + ox0;
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    if constexpr (V == 4) {
      *reinterpret_cast<float4*>(o + c * plane) = make_float4(__fdiv_rn((float)v[c], 255.f), __fdiv_rn((float)v[3 + c], 255.f),
                                                              __fdiv_rn((float)v[6 + c], 255.f), __fdiv_rn((float)v[9 + c], 255.f));
    } else {
      o[c * plane] = __fdiv_rn((float)v[c], 255.f);
    }
  }
  if (canvas) {
    if constexpr (V == 4) {
      uint32_t* cw = reinterpret_cast<uint32_t*>(canvas + pix * 3);
#pragma unroll
      for (int i = 0; i < 3; ++i)
        cw[i] = (uint32_t)v[4 * i] | ((uint32_t)v[4 * i + 1] << 8) | ((uint32_t)v[4 * i + 2] << 16) | ((uint32_t)v[4 * i + 3] << 24);
    } else {
      canvas[pix * 3] = v[0]; canvas[pix * 3 + 1] = v[1]; canvas[pix * 3 + 2] = v[2];
    }
  }
}

// taps Pillow's bicubic needs per output index: ceil(2 * max(in / out, 1)) * 2 + 1 (Resample.c precompute_coeffs)
static int ii_ksize(int in_size, int out_size) {
  const long long num = 2LL * (in_size > out_size ? in_size : out_size);          // ceil(2 * max(in, out) / out)
  return (int)((num + out_size - 1) / out_size) * 2 + 1;
}

// what n consecutive output indices span in the source at most: below (n - 1) * scale + 2 * support + 1 (first index above
// center - support - 1/2, end at most center + support + 1/2), one more for good measure, never more than the source or `limit`
static int ii_span_cap(int in_size, int out_size, int n, int limit) {
  const double scale = (double)in_size / out_size, support = 2.0 * (scale > 1.0 ? scale : 1.0);
  const int cap = (int)((n - 1) * scale + 2.0 * support + 1.0) + 1;
  return std::min(std::min(cap, in_size), limit);
}

extern "C" int coocc_frames_to_imgs(const uint8_t* frames, const void* const* frame_ptrs, int N, int Hs, int Ws, const int32_t* params,
                                    const int32_t* params_host, const int32_t* tables, int64_t table_ints, int fH, int fW, float* imgs,
                                    uint8_t* canvas, void* stream) {
  COOCC_CHECK_ARG(N >= 1 && N <= 65535, "frames_to_imgs: N = %d cameras (1 .. 65535)", N);
  COOCC_CHECK_ARG(Hs >= 1 && Ws >= 1 && (long long)Hs * Ws * 3 < (1LL << 31), "frames_to_imgs: frame size %d x %d", Hs, Ws);
  COOCC_CHECK_ARG(fH >= 1 && fW >= 1 && (long long)fH * fW * 3 < (1LL << 31) && fH <= 65535 * II_TH,
                  "frames_to_imgs: output size %d x %d", fH, fW);
  COOCC_CHECK_ARG((frames != nullptr) != (frame_ptrs != nullptr), "frames_to_imgs: exactly one of frames / frame_ptrs (null or both given)");
  COOCC_CHECK_ARG(params && params_host && imgs, "frames_to_imgs: null params / params_host / imgs");
  COOCC_CHECK_ARG(table_ints >= 0 && table_ints < (1LL << 31), "frames_to_imgs: table_ints = %lld", (long long)table_ints);
  bool resized = false;
  int hcap = 1, vcap = II_TH;
  for (int i = 0; i < N; ++i) {
    const int32_t* P = params_host + (size_t)i * II_CAM_INTS;
    const int newW = P[0], newH = P[1];
    COOCC_CHECK_ARG(newW >= 1 && newH >= 1 && newW < (1 << 24) && newH < (1 << 24), "frames_to_imgs: camera %d resize_dims %d x %d", i, newW, newH);
    COOCC_CHECK_ARG(abs(P[2]) < (1 << 24) && abs(P[3]) < (1 << 24), "frames_to_imgs: camera %d crop origin (%d, %d)", i, P[2], P[3]);
    const int in_size[2] = {Ws, Hs}, out_size[2] = {newW, newH};
    for (int a = 0; a < 2; ++a) {
      const int tab = P[5 + 2 * a], k = P[6 + 2 * a];
      if (tab < 0) {
        COOCC_CHECK_ARG(in_size[a] == out_size[a], "frames_to_imgs: camera %d has no %s table but resizes %d -> %d", i,
                        a ? "vertical" : "horizontal", in_size[a], out_size[a]);
        continue;
      }
      resized = true;
      const int need = ii_ksize(in_size[a], out_size[a]);
      COOCC_CHECK_ARG(need <= II_KMAX, "frames_to_imgs: camera %d %s ratio %d / %d = %.3f is beyond the limit of %d (%d taps, %d at most)", i,
                      a ? "vertical" : "horizontal", in_size[a], out_size[a], (double)in_size[a] / out_size[a], II_MAX_RATIO, need, II_KMAX);
      COOCC_CHECK_ARG(k == need, "frames_to_imgs: camera %d %s table has %d taps per index, %d -> %d takes %d", i,
                      a ? "vertical" : "horizontal", k, in_size[a], out_size[a], need);
      COOCC_CHECK_ARG(tables && (int64_t)tab + (int64_t)out_size[a] * (2 + k) <= table_ints,
                      "frames_to_imgs: camera %d %s table [%d, +%d * %d) leaves the %lld table ints (or tables is null)", i,
                      a ? "vertical" : "horizontal", tab, out_size[a], 2 + k, (long long)table_ints);
      if (a == 0) hcap = std::max(hcap, ii_span_cap(Ws, newW, II_TW, II_HSPAN));
      else vcap = std::max(vcap, ii_span_cap(Hs, newH, II_TH, II_VSPAN));
    }
  }
  const uint8_t* const* fp = reinterpret_cast<const uint8_t* const*>(frame_ptrs);
  if (resized) {
    const int sstride = ii_sstride(hcap), srows = std::max(1, std::min(16, II_STAGE_BYTES / sstride));
    const size_t lds = (size_t)srows * sstride + (size_t)vcap * II_TW * 3 + II_TH * II_TW * 3;          // 38.3 KB at the limit
    dim3 grid(cdiv(fW, II_TW), cdiv(fH, II_TH), N);
    hipLaunchKernelGGL(k_frames_to_imgs, grid, dim3(256), lds, as_stream(stream), frames, fp, Hs, Ws, params, tables, fH, fW, imgs, canvas,
                       hcap, vcap, srows);
    COOCC_LAUNCH_CHECK("k_frames_to_imgs");
  } else {
    COOCC_CHECK_ARG(fH <= 65535, "frames_to_imgs: output height %d", fH);
    if (fW % 4 == 0 && ((uintptr_t)imgs & 15) == 0 && ((uintptr_t)canvas & 3) == 0) {
      hipLaunchKernelGGL(k_frames_crop<4>, dim3(cdiv(fW, 1024), fH, N), dim3(256), 0, as_stream(stream), frames, fp, Hs, Ws, params, fH, fW,
                         imgs, canvas);
    } else {
      hipLaunchKernelGGL(k_frames_crop<1>, dim3(cdiv(fW, 256), fH, N), dim3(256), 0, as_stream(stream), frames, fp, Hs, Ws, params, fH, fW,
                         imgs, canvas);
    }
    COOCC_LAUNCH_CHECK("k_frames_crop");
  }
  return COOCC_OK;
}
