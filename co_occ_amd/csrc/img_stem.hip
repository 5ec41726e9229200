// The stem of the 2-D image backbone (co_occ_amd/image_encoder.py; mmdet ResNet: conv1 7x7 stride 2 pad 3 -> bn1 -> ReLU ->
// MaxPool2d(3, 2, 1)), the one layer of ResNet + SECONDFPN whose input (3 channels, NCHW) fits none of the row kernels.
//
//   k_img_stem<POOL>   one workgroup = one tile of 9 x 17 convolution outputs x 64 channels of one image.
//     1. the 147 x 64 weight matrix (k = (ci*7 + ky)*7 + kx) and the 3 x 23 x 39 input patch the tile reads go to LDS; the patch is
//        read straight from the fp32 NCHW image (coalesced along W), zeros outside the image -- the convolution's own padding;
//     2. every thread owns 8 channels x 5 pixels (lanes 0-31 of a wave: 32 pixels of one channel octet, lanes 32-63 the next
//        octet) and walks k = 0..146 in order: one fp32 fma per (pixel, channel, k), a fixed chain, no atomics -- the same bits
//        from run to run and for a pixel whichever tile computes it;
//     3. folded BN (+ ReLU), then the 9 x 17 x 64 tile goes to LDS over the (dead) weights and patch;
//     4. POOL = false: the tile is written as channels-last rows [BN*Hc*Wc][64] (tests judge the convolution alone);
//        POOL = true: the tile is the 4 x 8 pooled outputs' windows, halo included (origin (2 ph0 - 1, 2 pw0 - 1)): each pooled
//        value is the maximum over the window positions that lie INSIDE the convolution map -- padding is never a candidate,
//        whatever sign the map has -- and only the pooled rows [BN*Hp*Wp][64] (+ their H2 twin on request) reach HBM.
// LDS: max(147*64 + 3*23*40, 153*64) floats = 48.7 KB, three workgroups per CU.
#include "common.h"
#include "h2_rows.h"

int coocc_h2_flag_ptr(int** out);

#define ST_C0 64
#define ST_K 147
#define ST_TPH 4
#define ST_TPW 8
#define ST_CH (2 * ST_TPH + 1)
#define ST_CW (2 * ST_TPW + 1)
#define ST_NPIX (ST_CH * ST_CW)
#define ST_PH (2 * ST_CH + 5)
#define ST_PW (2 * ST_CW + 5)
#define ST_PWP 40                       /* padded patch row */
#define ST_PATCH (3 * ST_PH * ST_PWP)
#define ST_LDS (ST_K * ST_C0 + ST_PATCH)
static_assert(ST_LDS >= ST_NPIX * ST_C0, "the output tile aliases the weights + patch");
static_assert(ST_PWP >= ST_PW && 5 * 32 >= ST_NPIX, "tile constants");

struct StemK {
  const float* img;       // [BN][3][H][W]
  const float* w;         // [147][64]
  const float* scale;     // [64]
  const float* bias;      // [64]
  float* out;             // rows [BN*Ho*Wo][out_stride]
  void* out_h2t;          // H2 twin [rows][64] or NULL
  int* h2_flag;
  int H, W, Hc, Wc, Ho, Wo, out_stride, relu;
};

template <bool POOL>
__global__ __launch_bounds__(256) void k_img_stem(StemK p) {
  __shared__ __attribute__((aligned(16))) float smem[ST_LDS];
  float* wl = smem;
  float* patch = smem + ST_K * ST_C0;
  const int tid = threadIdx.x;
  const int b = blockIdx.z;
  // convolution-map origin of the tile, and the input pixel its tap (0, 0) reads
  const int cy0 = POOL ? 2 * ST_TPH * (int)blockIdx.y - 1 : ST_CH * (int)blockIdx.y;
  const int cx0 = POOL ? 2 * ST_TPW * (int)blockIdx.x - 1 : ST_CW * (int)blockIdx.x;
  const int iy0 = 2 * cy0 - 3, ix0 = 2 * cx0 - 3;

  for (int i = tid; i < ST_K * ST_C0 / 4; i += 256) ((f32x4*)wl)[i] = ((const f32x4*)p.w)[i];
  const float* im = p.img + (size_t)b * 3 * p.H * p.W;
  for (int i = tid; i < 3 * ST_PH * ST_PW; i += 256) {
    const int ci = i / (ST_PH * ST_PW), r = i - ci * (ST_PH * ST_PW);
    const int py = r / ST_PW, px = r - py * ST_PW;
    const int gy = iy0 + py, gx = ix0 + px;
    float v = 0.f;
    if ((unsigned)gy < (unsigned)p.H && (unsigned)gx < (unsigned)p.W) v = im[((size_t)ci * p.H + gy) * p.W + gx];
    patch[(ci * ST_PH + py) * ST_PWP + px] = v;
  }
  __syncthreads();

  const int slot = tid & 31, c0 = (tid >> 5) * 8;
  int off[5];
#pragma unroll
  for (int j = 0; j < 5; ++j) {
    int pix = slot + 32 * j;
    if (pix >= ST_NPIX) pix = 0;            // the spare slots recompute pixel 0 and store nothing
    off[j] = 2 * (pix / ST_CW) * ST_PWP + 2 * (pix % ST_CW);
  }
  float acc[5][8];
#pragma unroll
  for (int j = 0; j < 5; ++j)
#pragma unroll
    for (int e = 0; e < 8; ++e) acc[j][e] = 0.f;
  for (int cy = 0; cy < 21; ++cy) {          // (ci, ky)
    const int ci = cy / 7, ky = cy - ci * 7;
    const float* prow = patch + (ci * ST_PH + ky) * ST_PWP;
    const float* wrow = wl + cy * 7 * ST_C0 + c0;
#pragma unroll
    for (int kx = 0; kx < 7; ++kx) {
      const f32x4 w0 = *(const f32x4*)(wrow + kx * ST_C0), w1 = *(const f32x4*)(wrow + kx * ST_C0 + 4);
#pragma unroll
      for (int j = 0; j < 5; ++j) {
        const float x = prow[off[j] + kx];
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          acc[j][e] = __builtin_fmaf(x, w0[e], acc[j][e]);
          acc[j][4 + e] = __builtin_fmaf(x, w1[e], acc[j][4 + e]);
        }
      }
    }
  }
  float sc[8], bi[8];
#pragma unroll
  for (int e = 0; e < 8; ++e) { sc[e] = p.scale[c0 + e]; bi[e] = p.bias[c0 + e]; }
  __syncthreads();                           // every thread has read the weights and the patch for the last time
  float* tile = smem;                        // [153][64]
#pragma unroll
  for (int j = 0; j < 5; ++j) {
    const int pix = slot + 32 * j;
    if (pix < ST_NPIX) {
      f32x4 v0, v1;
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        float a = __builtin_fmaf(acc[j][e], sc[e], bi[e]), c = __builtin_fmaf(acc[j][4 + e], sc[4 + e], bi[4 + e]);
        if (p.relu) { a = a > 0.f ? a : 0.f; c = c > 0.f ? c : 0.f; }
        v0[e] = a; v1[e] = c;
      }
      *(f32x4*)(tile + pix * ST_C0 + c0) = v0;
      *(f32x4*)(tile + pix * ST_C0 + c0 + 4) = v1;
    }
  }
  __syncthreads();

  if (POOL) {
    for (int i = tid; i < ST_TPH * ST_TPW * 16; i += 256) {
      const int n = (i & 15) * 4, pp = i >> 4;
      const int pr = pp / ST_TPW, pc = pp - pr * ST_TPW;
      const int ph = ST_TPH * (int)blockIdx.y + pr, pw = ST_TPW * (int)blockIdx.x + pc;
      if (ph >= p.Ho || pw >= p.Wo) continue;
      f32x4 m = {-INFINITY, -INFINITY, -INFINITY, -INFINITY};
#pragma unroll
      for (int dr = 0; dr < 3; ++dr)
#pragma unroll
        for (int dc = 0; dc < 3; ++dc) {
          const int lr = 2 * pr + dr, lc = 2 * pc + dc;             // tile-local; global = (cy0 + lr, cx0 + lc)
          if ((unsigned)(cy0 + lr) < (unsigned)p.Hc && (unsigned)(cx0 + lc) < (unsigned)p.Wc) {
            const f32x4 v = *(const f32x4*)(tile + (lr * ST_CW + lc) * ST_C0 + n);
#pragma unroll
            for (int e = 0; e < 4; ++e) m[e] = v[e] > m[e] ? v[e] : m[e];
          }
        }
      const size_t row = ((size_t)b * p.Ho + ph) * p.Wo + pw;
      *(f32x4*)(p.out + row * p.out_stride + n) = m;
      if (p.out_h2t) { store_h2(p.out_h2t, row, ST_C0, n, m); h2_guard(p.h2_flag, m); }
    }
  } else {
    for (int i = tid; i < ST_NPIX * 16; i += 256) {
      const int n = (i & 15) * 4, pix = i >> 4;
      const int gy = cy0 + pix / ST_CW, gx = cx0 + pix % ST_CW;
      if (gy >= p.Hc || gx >= p.Wc) continue;
      const f32x4 v = *(const f32x4*)(tile + pix * ST_C0 + n);
      const size_t row = ((size_t)b * p.Hc + gy) * p.Wc + gx;
      *(f32x4*)(p.out + row * p.out_stride + n) = v;
      if (p.out_h2t) { store_h2(p.out_h2t, row, ST_C0, n, v); h2_guard(p.h2_flag, v); }
    }
  }
}

extern "C" int coocc_img_stem(const float* img, int BN, int H, int W, const float* w, const float* scale, const float* bias, int C0,
                              int relu, int pool, float* out, int out_stride, void* out_h2_twin, void* stream) {
  COOCC_CHECK_ARG(img && w && scale && bias && out, "img_stem: null pointer");
  COOCC_CHECK_ARG(BN > 0 && H > 0 && W > 0, "img_stem: bad image size");
  COOCC_CHECK_ARG(C0 == ST_C0, "img_stem: 64 stem channels only");
  COOCC_CHECK_ARG(out_stride >= C0 && out_stride % 4 == 0, "img_stem: out_stride must be a multiple of 4, at least C0");
  COOCC_CHECK_ARG((((uintptr_t)w | (uintptr_t)out | (uintptr_t)out_h2_twin) & 15) == 0 && ((uintptr_t)img & 3) == 0,
                  "img_stem: w / out / twin must be 16-byte aligned");
  StemK k;
  k.img = img; k.w = w; k.scale = scale; k.bias = bias; k.out = out; k.out_h2t = out_h2_twin; k.h2_flag = nullptr;
  k.H = H; k.W = W; k.Hc = (H - 1) / 2 + 1; k.Wc = (W - 1) / 2 + 1;
  k.Ho = pool ? (k.Hc - 1) / 2 + 1 : k.Hc;
  k.Wo = pool ? (k.Wc - 1) / 2 + 1 : k.Wc;
  k.out_stride = out_stride; k.relu = relu ? 1 : 0;
  COOCC_CHECK_ARG((long long)BN * k.Hc * k.Wc < (1ll << 31) && (long long)H * W < (1ll << 31),
                  "img_stem: map too large (row indices are 32-bit)");
  const unsigned gx = pool ? cdiv(k.Wo, ST_TPW) : cdiv(k.Wc, ST_CW), gy = pool ? cdiv(k.Ho, ST_TPH) : cdiv(k.Hc, ST_CH);
  COOCC_CHECK_ARG(BN <= 65535 && gy <= 65535, "img_stem: BN and the tile rows must fit a grid dimension (65535)");
  if (out_h2_twin) {
    const int rc = coocc_h2_flag_ptr(&k.h2_flag);
    if (rc != COOCC_OK) return rc;
  }
  if (pool) hipLaunchKernelGGL(k_img_stem<true>, dim3(gx, gy, BN), dim3(256), 0, as_stream(stream), k);
  else hipLaunchKernelGGL(k_img_stem<false>, dim3(gx, gy, BN), dim3(256), 0, as_stream(stream), k);
  COOCC_LAUNCH_CHECK("k_img_stem");
  return COOCC_OK;
}
