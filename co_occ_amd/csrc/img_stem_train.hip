// Training of the 2-D image backbone's stem (co_occ_amd/image_encoder.py, ResNet.train_enabled; the inference stem is
// csrc/img_stem.hip).  Under train() the stem runs unfused -- conv 7x7 / 2 (k_img_stem<false>, scale 1, bias 0) -> BatchNormRowsFn
// (batch statistics, ReLU) -> max-pool -- and these are the three kernels the engine lacked for it.  fp32 arithmetic, no atomics,
// the same bits from run to run; 32-bit index checks, null / alignment checks before any launch.
//
//   k_maxpool2d_rows       MaxPool2d(3, 2, 1) on channels-last rows [BN*Hc*Wc][stride] -> [BN*Hp*Wp][out_stride] (+ the H2 twin).
//     One thread = one pooled pixel x 4 channels.  The maximum is taken with `v > m ? v : m` from -inf over the window positions
//     INSIDE the map, in the window's row-major order: padding is never a candidate, and given the same pre-pool map the bits are
//     those of k_img_stem<true>.  Non-finite inputs are out of scope, as they are for the fused kernel (a NaN never wins `>`).
//   k_maxpool2d_rows_bwd   gather form, no index tensor: one thread = one PRE-pool pixel x 4 channels.  The pixel lies in at most
//     2 x 2 windows; for each, in ascending (ph, pw) order, the thread recomputes the window's first maximum in row-major window
//     order under strict `>` (torch's rule: ties go to the earliest element) and adds that window's dy when it is the pixel itself.
//     Every dx element is written exactly once, zeros included.
//   k_img_stem_wgrad       dW [147][64] (row (ci*7 + ky)*7 + kx, stem_pack's order) = patches^T . dy, the [147 x M] . [M x 64] product
//     with M = BN*Hc*Wc, in plain fp32 FMAs.  The conv map is cut into tiles of 8 x 16 outputs; workgroup g of P = min(tiles, 512)
//     walks tiles g, g + P, g + 2P, ... (a function of the problem's shape only, never of the device).  Per tile the 3 x 21 x 37 input
//     patch (zeros outside the image, the convolution's own padding) and the 128 x 64 dy tile (zeros outside the map) go to LDS;
//     thread (kg, cq) owns rows k = kg + 16 j (j < 10) x channels 4 cq .. 4 cq + 3 in 40 registers and walks the tile's pixels in
//     order.  Each workgroup writes ONE partial [147][64] into the caller's workspace (at most 512 x 37.6 KB = 19 MB, against
//     69 MB of dy at 6 x 256 x 704); k_img_stem_wgrad_sum adds the partials in ascending order.
#include "common.h"
#include "h2_rows.h"

int coocc_h2_flag_ptr(int** out);

#define SW_C0 64
#define SW_K 147
#define SW_TH 8
#define SW_TW 16
#define SW_NPIX (SW_TH * SW_TW)
#define SW_PH (2 * SW_TH + 5)
#define SW_PW (2 * SW_TW + 5)
#define SW_PWP 40                       /* padded patch row */
#define SW_PATCH (3 * SW_PH * SW_PWP)
#define SW_KJ 10                        /* rows of dW per thread: k = kg + 16 j */
#define SW_MAX_PARTIALS 512
static_assert(SW_PWP >= SW_PW && 16 * SW_KJ >= SW_K, "tile constants");

struct PoolK {
  const float* x;         // rows [BN*Hc*Wc][x_stride]
  const float* dy;        // rows [BN*Hp*Wp][dy_stride]      (backward)
  float* out;             // forward: rows [BN*Hp*Wp][out_stride]; backward: dx rows [BN*Hc*Wc][out_stride]
  void* out_h2t;
  int* h2_flag;
  int Hc, Wc, Hp, Wp, C, x_stride, dy_stride, out_stride;
  long long total;        // threads: rows x C / 4
};

__global__ __launch_bounds__(256) void k_maxpool2d_rows(PoolK p) {
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  if (i >= p.total) return;
  const int q = p.C >> 2;
  const int n = (int)(i % q) * 4;
  const long long row = i / q;
  const int pw = (int)(row % p.Wp);
  const long long t = row / p.Wp;
  const int ph = (int)(t % p.Hp);
  const long long b = t / p.Hp;
  const float* xb = p.x + (size_t)b * p.Hc * p.Wc * p.x_stride + n;
  f32x4 m = {-INFINITY, -INFINITY, -INFINITY, -INFINITY};
#pragma unroll
  for (int dr = 0; dr < 3; ++dr)
#pragma unroll
    for (int dc = 0; dc < 3; ++dc) {
      const int y = 2 * ph - 1 + dr, x = 2 * pw - 1 + dc;
      if ((unsigned)y < (unsigned)p.Hc && (unsigned)x < (unsigned)p.Wc) {
        const f32x4 v = *(const f32x4*)(xb + ((size_t)y * p.Wc + x) * p.x_stride);
#pragma unroll
        for (int e = 0; e < 4; ++e) m[e] = v[e] > m[e] ? v[e] : m[e];
      }
    }
  *(f32x4*)(p.out + (size_t)row * p.out_stride + n) = m;
  if (p.out_h2t) { store_h2(p.out_h2t, (size_t)row, p.C, n, m); h2_guard(p.h2_flag, m); }
}

__global__ __launch_bounds__(256) void k_maxpool2d_rows_bwd(PoolK p) {
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  if (i >= p.total) return;
  const int q = p.C >> 2;
  const int n = (int)(i % q) * 4;
  const long long row = i / q;
  const int x0 = (int)(row % p.Wc);
  const long long t = row / p.Wc;
  const int y0 = (int)(t % p.Hc);
  const long long b = t / p.Hc;
  const float* xb = p.x + (size_t)b * p.Hc * p.Wc * p.x_stride + n;
  const float* dyb = p.dy + (size_t)b * p.Hp * p.Wp * p.dy_stride + n;
  // the windows that contain (y0, x0): 2 ph - 1 <= y0 <= 2 ph + 1
  const int ph_lo = y0 >> 1, ph_hi = min((y0 + 1) >> 1, p.Hp - 1);
  const int pw_lo = x0 >> 1, pw_hi = min((x0 + 1) >> 1, p.Wp - 1);
  f32x4 g = {0.f, 0.f, 0.f, 0.f};
  for (int ph = ph_lo; ph <= ph_hi; ++ph)
    for (int pw = pw_lo; pw <= pw_hi; ++pw) {
      const int me = (y0 - (2 * ph - 1)) * 3 + (x0 - (2 * pw - 1));          // this pixel's position in the window
      f32x4 m = {-INFINITY, -INFINITY, -INFINITY, -INFINITY};
      int arg[4] = {-1, -1, -1, -1};
#pragma unroll
      for (int dr = 0; dr < 3; ++dr)
#pragma unroll
        for (int dc = 0; dc < 3; ++dc) {
          const int y = 2 * ph - 1 + dr, x = 2 * pw - 1 + dc;
          if ((unsigned)y < (unsigned)p.Hc && (unsigned)x < (unsigned)p.Wc) {
            const f32x4 v = *(const f32x4*)(xb + ((size_t)y * p.Wc + x) * p.x_stride);
#pragma unroll
            for (int e = 0; e < 4; ++e)
              if (v[e] > m[e]) { m[e] = v[e]; arg[e] = dr * 3 + dc; }
          }
        }
      const f32x4 d = *(const f32x4*)(dyb + ((size_t)ph * p.Wp + pw) * p.dy_stride);
#pragma unroll
      for (int e = 0; e < 4; ++e)
        if (arg[e] == me) g[e] += d[e];
    }
  *(f32x4*)(p.out + (size_t)row * p.out_stride + n) = g;
}

static int pool_args(const char* who, const float* x, int x_stride, int BN, int Hc, int Wc, int C, PoolK& k) {
  COOCC_CHECK_ARG(x, "%s: null pointer", who);
  COOCC_CHECK_ARG(BN > 0 && Hc > 0 && Wc > 0, "%s: bad map size", who);
  COOCC_CHECK_ARG(C > 0 && C % 4 == 0, "%s: C must be a positive multiple of 4", who);
  COOCC_CHECK_ARG(x_stride >= C && x_stride % 4 == 0, "%s: x_stride must be a multiple of 4, at least C", who);
  COOCC_CHECK_ARG((long long)BN * Hc * Wc < (1ll << 31), "%s: map too large (row indices are 32-bit)", who);
  k.x = x; k.dy = nullptr; k.out = nullptr; k.out_h2t = nullptr; k.h2_flag = nullptr;
  k.Hc = Hc; k.Wc = Wc; k.Hp = (Hc - 1) / 2 + 1; k.Wp = (Wc - 1) / 2 + 1; k.C = C;
  k.x_stride = x_stride; k.dy_stride = 0; k.out_stride = 0; k.total = 0;
  return COOCC_OK;
}

extern "C" int coocc_maxpool2d_rows(const float* x, int x_stride, int BN, int Hc, int Wc, int C, float* out, int out_stride,
                                    void* out_h2_twin, void* stream) {
  PoolK k;
  const int rc = pool_args("maxpool2d_rows", x, x_stride, BN, Hc, Wc, C, k);
  if (rc != COOCC_OK) return rc;
  COOCC_CHECK_ARG(out, "maxpool2d_rows: null pointer");
  COOCC_CHECK_ARG(out_stride >= C && out_stride % 4 == 0, "maxpool2d_rows: out_stride must be a multiple of 4, at least C");
  COOCC_CHECK_ARG((((uintptr_t)x | (uintptr_t)out | (uintptr_t)out_h2_twin) & 15) == 0, "maxpool2d_rows: x / out / twin must be 16-byte aligned");
  COOCC_CHECK_ARG(!out_h2_twin || C % 32 == 0, "maxpool2d_rows: an H2 twin needs C %% 32 == 0");
  k.out = out; k.out_stride = out_stride; k.out_h2t = out_h2_twin;
  k.total = (long long)BN * k.Hp * k.Wp * (C / 4);
  COOCC_CHECK_ARG((k.total + 255) / 256 < (1ll << 31), "maxpool2d_rows: too many rows x channels for one grid");
  if (out_h2_twin) {
    const int r2 = coocc_h2_flag_ptr(&k.h2_flag);
    if (r2 != COOCC_OK) return r2;
  }
  hipLaunchKernelGGL(k_maxpool2d_rows, dim3(cdiv(k.total, 256)), dim3(256), 0, as_stream(stream), k);
  COOCC_LAUNCH_CHECK("k_maxpool2d_rows");
  return COOCC_OK;
}

extern "C" int coocc_maxpool2d_rows_bwd(const float* x, int x_stride, const float* dy, int dy_stride, int BN, int Hc, int Wc, int C,
                                        float* dx, int dx_stride, void* stream) {
  PoolK k;
  const int rc = pool_args("maxpool2d_rows_bwd", x, x_stride, BN, Hc, Wc, C, k);
  if (rc != COOCC_OK) return rc;
  COOCC_CHECK_ARG(dy && dx, "maxpool2d_rows_bwd: null pointer");
  COOCC_CHECK_ARG(dy_stride >= C && dy_stride % 4 == 0 && dx_stride >= C && dx_stride % 4 == 0,
                  "maxpool2d_rows_bwd: dy_stride / dx_stride must be multiples of 4, at least C");
  COOCC_CHECK_ARG((((uintptr_t)x | (uintptr_t)dy | (uintptr_t)dx) & 15) == 0, "maxpool2d_rows_bwd: x / dy / dx must be 16-byte aligned");
  k.dy = dy; k.dy_stride = dy_stride; k.out = dx; k.out_stride = dx_stride;
  k.total = (long long)BN * Hc * Wc * (C / 4);
  COOCC_CHECK_ARG((k.total + 255) / 256 < (1ll << 31), "maxpool2d_rows_bwd: too many rows x channels for one grid");
  hipLaunchKernelGGL(k_maxpool2d_rows_bwd, dim3(cdiv(k.total, 256)), dim3(256), 0, as_stream(stream), k);
  COOCC_LAUNCH_CHECK("k_maxpool2d_rows_bwd");
  return COOCC_OK;
}

// ------------------------------------------------------------------ stem weight gradient
struct StemWgK {
  const float* img;       // [BN][3][H][W]
  const float* dy;        // rows [BN*Hc*Wc][dy_stride]
  float* part;            // [P][147][64]
  int H, W, Hc, Wc, dy_stride, TY, TX, tiles, P;
};

__global__ __launch_bounds__(256) void k_img_stem_wgrad(StemWgK p) {
  __shared__ __attribute__((aligned(16))) float dyl[SW_NPIX * SW_C0];
  __shared__ float patch[SW_PATCH];
  const int tid = threadIdx.x;
  const int cq = (tid & 15) * 4, kg = tid >> 4;
  int koff[SW_KJ];
#pragma unroll
  for (int j = 0; j < SW_KJ; ++j) {
    int k = kg + 16 * j;
    if (k >= SW_K) k = 0;                    // the spare rows accumulate row 0 again and store nothing
    const int ci = k / 49, r = k - ci * 49, ky = r / 7, kx = r - ky * 7;
    koff[j] = (ci * SW_PH + ky) * SW_PWP + kx;
  }
  float acc[SW_KJ][4];
#pragma unroll
  for (int j = 0; j < SW_KJ; ++j)
#pragma unroll
    for (int e = 0; e < 4; ++e) acc[j][e] = 0.f;

  for (int t = blockIdx.x; t < p.tiles; t += p.P) {
    const int tx = t % p.TX, r0 = t / p.TX, ty = r0 % p.TY, b = r0 / p.TY;
    const int cy0 = SW_TH * ty, cx0 = SW_TW * tx;
    const int iy0 = 2 * cy0 - 3, ix0 = 2 * cx0 - 3;
    __syncthreads();                         // the previous tile has been read for the last time
    const float* im = p.img + (size_t)b * 3 * p.H * p.W;
    for (int i = tid; i < 3 * SW_PH * SW_PW; i += 256) {
      const int ci = i / (SW_PH * SW_PW), r = i - ci * (SW_PH * SW_PW);
      const int py = r / SW_PW, px = r - py * SW_PW;
      const int gy = iy0 + py, gx = ix0 + px;
      float v = 0.f;
      if ((unsigned)gy < (unsigned)p.H && (unsigned)gx < (unsigned)p.W) v = im[((size_t)ci * p.H + gy) * p.W + gx];
      patch[(ci * SW_PH + py) * SW_PWP + px] = v;
    }
    for (int i = tid; i < SW_NPIX * 16; i += 256) {
      const int n = (i & 15) * 4, pix = i >> 4;
      const int gy = cy0 + pix / SW_TW, gx = cx0 + pix % SW_TW;
      f32x4 v = {0.f, 0.f, 0.f, 0.f};
      if (gy < p.Hc && gx < p.Wc) v = *(const f32x4*)(p.dy + (((size_t)b * p.Hc + gy) * p.Wc + gx) * p.dy_stride + n);
      *(f32x4*)(dyl + pix * SW_C0 + n) = v;
    }
    __syncthreads();
    for (int py = 0; py < SW_TH; ++py) {
      const float* prow = patch + 2 * py * SW_PWP;
      const float* drow = dyl + py * SW_TW * SW_C0 + cq;
#pragma unroll 4
      for (int px = 0; px < SW_TW; ++px) {
        const f32x4 d = *(const f32x4*)(drow + px * SW_C0);
#pragma unroll
        for (int j = 0; j < SW_KJ; ++j) {
          const float a = prow[koff[j] + 2 * px];
#pragma unroll
          for (int e = 0; e < 4; ++e) acc[j][e] = __builtin_fmaf(a, d[e], acc[j][e]);
        }
      }
    }
  }
  float* o = p.part + (size_t)blockIdx.x * SW_K * SW_C0;
#pragma unroll
  for (int j = 0; j < SW_KJ; ++j) {
    const int k = kg + 16 * j;
    if (k < SW_K) {
      f32x4 v;
#pragma unroll
      for (int e = 0; e < 4; ++e) v[e] = acc[j][e];
      *(f32x4*)(o + k * SW_C0 + cq) = v;
    }
  }
}

__global__ __launch_bounds__(256) void k_img_stem_wgrad_sum(const float* __restrict__ part, int P, float* __restrict__ dw) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= SW_K * SW_C0) return;
  float s = 0.f;
  for (int g = 0; g < P; ++g) s += part[(size_t)g * SW_K * SW_C0 + i];
  dw[i] = s;
}

static void stem_wgrad_tiles(int BN, int H, int W, StemWgK& k, long long& tiles) {
  k.H = H; k.W = W; k.Hc = (H - 1) / 2 + 1; k.Wc = (W - 1) / 2 + 1;
  k.TY = (k.Hc + SW_TH - 1) / SW_TH; k.TX = (k.Wc + SW_TW - 1) / SW_TW;
  tiles = (long long)BN * k.TY * k.TX;
}

extern "C" size_t coocc_img_stem_wgrad_ws(int BN, int H, int W) {
  if (BN <= 0 || H <= 0 || W <= 0) return 0;
  StemWgK k;
  long long tiles;
  stem_wgrad_tiles(BN, H, W, k, tiles);
  const long long P = tiles < SW_MAX_PARTIALS ? tiles : SW_MAX_PARTIALS;
  return (size_t)P * SW_K * SW_C0 * sizeof(float);
}

extern "C" int coocc_img_stem_wgrad(const float* img, int BN, int H, int W, const float* dy, int dy_stride, int C0, float* dw,
                                    void* ws, size_t ws_bytes, void* stream) {
  COOCC_CHECK_ARG(img && dy && dw && ws, "img_stem_wgrad: null pointer");
  COOCC_CHECK_ARG(BN > 0 && H > 0 && W > 0, "img_stem_wgrad: bad image size");
  COOCC_CHECK_ARG(C0 == SW_C0, "img_stem_wgrad: 64 stem channels only");
  COOCC_CHECK_ARG(dy_stride >= C0 && dy_stride % 4 == 0, "img_stem_wgrad: dy_stride must be a multiple of 4, at least C0");
  COOCC_CHECK_ARG((((uintptr_t)dy | (uintptr_t)dw | (uintptr_t)ws) & 15) == 0 && ((uintptr_t)img & 3) == 0,
                  "img_stem_wgrad: dy / dw / ws must be 16-byte aligned");
  StemWgK k;
  long long tiles;
  stem_wgrad_tiles(BN, H, W, k, tiles);
  COOCC_CHECK_ARG((long long)BN * k.Hc * k.Wc < (1ll << 31) && (long long)H * W < (1ll << 31) && tiles < (1ll << 31),
                  "img_stem_wgrad: map too large (row indices are 32-bit)");
  COOCC_CHECK_ARG(ws_bytes >= coocc_img_stem_wgrad_ws(BN, H, W), "img_stem_wgrad: workspace too small");
  k.img = img; k.dy = dy; k.part = (float*)ws; k.dy_stride = dy_stride;
  k.tiles = (int)tiles; k.P = (int)(tiles < SW_MAX_PARTIALS ? tiles : SW_MAX_PARTIALS);
  hipLaunchKernelGGL(k_img_stem_wgrad, dim3(k.P), dim3(256), 0, as_stream(stream), k);
  COOCC_LAUNCH_CHECK("k_img_stem_wgrad");
  hipLaunchKernelGGL(k_img_stem_wgrad_sum, dim3(cdiv(SW_K * SW_C0, 256)), dim3(256), 0, as_stream(stream), (const float*)k.part, k.P, dw);
  COOCC_LAUNCH_CHECK("k_img_stem_wgrad_sum");
  return COOCC_OK;
}
