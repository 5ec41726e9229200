// OccHead cascade ("fine") branch of a VOXEL-ONLY head (sample_from_voxel=True, sample_from_img=False: occ_head.py:205-214, 237),
// cascade ratio 2, in ONE launch with the foreground count on the device -- the form a captured dense stage needs
// (co_occ_amd/graph.py).  The LiDAR-only model's route to a prediction on the fine grid.
//
//   Q [V, 64] = fine_mlp[0].weight . out_voxel_feats (no bias: a Linear commutes with the trilinear interpolation that follows
//   it, and with its zero padding, W . 0 = 0), made by the caller with one pointwise GEMM over the V coarse voxels instead of over
//   the 8 n fine points.  Per foreground coarse voxel and each of its 8 children:
//     trilinear sample of Q (grid_sample: align_corners=False, padding_mode='zeros') -> + b0 -> GroupNorm(16 groups x 4) -> ReLU
//     -> Linear 64 -> ncls.
//
// Work split: 16 lanes per coarse voxel, lane l owns channels 4 l .. 4 l + 3 -- one 16-byte load per lane and neighbour row (a
// 256-byte row per 16 lanes) and exactly one GroupNorm group, so the normalisation needs no cross-lane traffic.  The 8 children
// read the same 3 x 3 x 3 neighbourhood: each of its 27 rows is fetched once per coarse voxel and feeds 8 register accumulators
// (the window and tap weights of k_fine_sample_voxel_r2, csrc/fine.hip, same expressions; out-of-grid taps are loaded from a
// clamped address and replaced by zero, so the four voxels of a wave do not diverge).  The hidden rows go through LDS for the
// second Linear (its 64 x ncls weights staged there once per workgroup): lane (child, class half) walks its classes with the row
// in registers.  The logits rows (68 bytes at ncls 17) are staged in LDS too and leave as 8 contiguous spans of 16 rows -- point
// f = o n + i is child-offset major, so the 16 voxels of a workgroup are neighbours in every one of the 8 offset blocks.
// No atomics, no cross-workgroup state: the same bits from run to run.  Workgroups past the device count leave at once.
#include "common.h"

typedef float f32x4 __attribute__((ext_vector_type(4)));

constexpr int FV_VOX = 16;   // coarse voxels per 256-thread workgroup
constexpr int FV_HP = 68;    // floats per hidden row in LDS: 64 + 4 keeps rows 16-byte aligned and the 8 children off each other's banks

struct FineVox {
  const float* Q;
  int X, Y, Z;
  const int32_t* lin;
  int n_cap;
  const int32_t* n_dev;
  float fx1, fy1, fz1;
  const float *b0, *gamma, *beta;
  float eps;
  const float *w3, *b3;
  int ncls;
  int64_t* xyz;
  float* out;
};

static inline size_t fv_lds_bytes(int ncls) { return sizeof(float) * ((size_t)FV_VOX * 8 * FV_HP + (size_t)ncls * 64 + (size_t)8 * FV_VOX * ncls); }

// base index and fraction of the two children of coarse index c along an axis of S coarse / f1 + 1 fine voxels: the reference's
// normalisation (q / (final - 1) - 0.5) * 2 and grid_sample's align_corners=False pixel ((g + 1) S - 1) / 2, as k_fine_sample_voxel
__device__ __forceinline__ void fv_axis(int c, float f1, int S, int (&i0)[2], float (&t)[2]) {
#pragma unroll
  for (int a = 0; a < 2; ++a) {
    const int q = c * 2 + a;
    const float g = ((float)q / f1 - 0.5f) * 2.f;
    const float p = ((g + 1.f) * (float)S - 1.f) / 2.f;
    const float fl = floorf(p);
    i0[a] = (int)fl; t[a] = p - fl;
  }
}
// tap weight of window position x for a child with base index b0 and fraction t
__device__ __forceinline__ float fv_tapw(int b0, float t, int x) { return (x == b0 ? 1.f - t : 0.f) + (x == b0 + 1 ? t : 0.f); }

__global__ COOCC_SCALAR_FP32 __launch_bounds__(256) void k_fine_vox(FineVox p) {
  extern __shared__ __attribute__((aligned(16))) char fv_smem[];
  int n = p.n_cap;
  if (p.n_dev) n = min(n, *p.n_dev);
  const int i_blk = blockIdx.x * FV_VOX;
  if (i_blk >= n) return;                                  // surplus workgroup (before any barrier: uniform)
  const int ncls = p.ncls;
  float* s_h = (float*)fv_smem;                            // [FV_VOX][8][FV_HP] hidden rows
  float* s_w = s_h + FV_VOX * 8 * FV_HP;                   // [ncls][64] fine_mlp[3].weight
  float* s_o = s_w + ncls * 64;                            // [8][FV_VOX][ncls] logits, offset-block major like the output
  const int tid = threadIdx.x, vl = tid >> 4, l16 = tid & 15;
  for (int k = tid; k < ncls * 16; k += 256) ((f32x4*)s_w)[k] = ((const f32x4*)p.w3)[k];
  const int i = i_blk + vl;
  const int X = p.X, Y = p.Y, Z = p.Z;
  f32x4 acc[8];
#pragma unroll
  for (int o = 0; o < 8; ++o) acc[o] = f32x4{0.f, 0.f, 0.f, 0.f};
  if (i < n) {
    int l = p.lin[i];
    const int cz = l % Z; l /= Z;
    const int cy = l % Y; const int cx = l / Y;             // B == 1
    int ix[2], iy[2], iz[2]; float tx[2], ty[2], tz[2];
    fv_axis(cx, p.fx1, X, ix, tx);
    fv_axis(cy, p.fy1, Y, iy, ty);
    fv_axis(cz, p.fz1, Z, iz, tz);
    if (l16 < 8) {
      const long long nf = (long long)n * 8, f = (long long)l16 * n + i;
      p.xyz[f] = cx * 2 + (l16 >> 2); p.xyz[nf + f] = cy * 2 + ((l16 >> 1) & 1); p.xyz[2 * nf + f] = cz * 2 + (l16 & 1);
    }
    const int wx0 = min(ix[0], ix[1]), wy0 = min(iy[0], iy[1]), wz0 = min(iz[0], iz[1]);
    const float* qc = p.Q + 4 * l16;
    // one x-plane of the window per trip: 9 independent 16-byte loads in flight, 27 rows per coarse voxel in all
#pragma unroll 1
    for (int kx = 0; kx < 3; ++kx) {
      const int x = wx0 + kx;
      const bool inx = (unsigned)x < (unsigned)X;
      const int xc = min(max(x, 0), X - 1);
      const float ax0 = fv_tapw(ix[0], tx[0], x), ax1 = fv_tapw(ix[1], tx[1], x);
      f32x4 v[3][3];
#pragma unroll
      for (int ky = 0; ky < 3; ++ky) {
        const int y = wy0 + ky;
        const bool iny = inx && (unsigned)y < (unsigned)Y;
        const int yc = min(max(y, 0), Y - 1);
#pragma unroll
        for (int kz = 0; kz < 3; ++kz) {
          const int z = wz0 + kz;
          const int zc = min(max(z, 0), Z - 1);
          const f32x4 r = *(const f32x4*)(qc + (((size_t)xc * Y + yc) * Z + zc) * 64);
          v[ky][kz] = (iny && (unsigned)z < (unsigned)Z) ? r : f32x4{0.f, 0.f, 0.f, 0.f};      // padding_mode='zeros'
        }
      }
#pragma unroll
      for (int ky = 0; ky < 3; ++ky) {
        const int y = wy0 + ky;
        const float by0 = fv_tapw(iy[0], ty[0], y), by1 = fv_tapw(iy[1], ty[1], y);
        const float w00 = ax0 * by0, w01 = ax0 * by1, w10 = ax1 * by0, w11 = ax1 * by1;
#pragma unroll
        for (int kz = 0; kz < 3; ++kz) {
          const int z = wz0 + kz;
          const float cz0 = fv_tapw(iz[0], tz[0], z), cz1 = fv_tapw(iz[1], tz[1], z);
          const f32x4 r = v[ky][kz];
          acc[0] = acc[0] + r * (w00 * cz0); acc[1] = acc[1] + r * (w00 * cz1);
          acc[2] = acc[2] + r * (w01 * cz0); acc[3] = acc[3] + r * (w01 * cz1);
          acc[4] = acc[4] + r * (w10 * cz0); acc[5] = acc[5] + r * (w10 * cz1);
          acc[6] = acc[6] + r * (w11 * cz0); acc[7] = acc[7] + r * (w11 * cz1);
        }
      }
    }
  }
  // + b0, GroupNorm over this lane's four channels (one group), ReLU -> LDS
  {
    const f32x4 b0 = *(const f32x4*)(p.b0 + 4 * l16), ga = *(const f32x4*)(p.gamma + 4 * l16), be = *(const f32x4*)(p.beta + 4 * l16);
#pragma unroll
    for (int o = 0; o < 8; ++o) {
      float y[4];
#pragma unroll
      for (int c = 0; c < 4; ++c) y[c] = acc[o][c] + b0[c];
      float mean, rstd;
      gn_group_stats<float>(y, 4, p.eps, mean, rstd);
      f32x4 h;
#pragma unroll
      for (int c = 0; c < 4; ++c) h[c] = fmaxf((y[c] - mean) * rstd * ga[c] + be[c], 0.f);
      *(f32x4*)(s_h + (vl * 8 + o) * FV_HP + 4 * l16) = h;
    }
  }
  __syncthreads();
  // Linear 64 -> ncls: lane (child, half) of a voxel's 16 lanes takes half of the classes of one child, the row in registers
  {
    const int ch = l16 & 7, nh = (ncls + 1) >> 1, c0 = (l16 >> 3) * nh, c1 = min(ncls, c0 + nh);
    const f32x4* hrow = (const f32x4*)(s_h + (vl * 8 + ch) * FV_HP);
    f32x4 hv[16];
#pragma unroll
    for (int k = 0; k < 16; ++k) hv[k] = hrow[k];
#pragma unroll 1
    for (int c = c0; c < c1; ++c) {
      const f32x4* wr = (const f32x4*)(s_w + c * 64);
      float s = 0.f;
#pragma unroll
      for (int k = 0; k < 16; ++k) {
        const f32x4 w = wr[k];
        s += hv[k][0] * w[0]; s += hv[k][1] * w[1]; s += hv[k][2] * w[2]; s += hv[k][3] * w[3];
      }
      s_o[(ch * FV_VOX + vl) * ncls + c] = s + p.b3[c];
    }
  }
  __syncthreads();
  // 8 spans of rows x ncls contiguous floats each (rows = the voxels of this workgroup that exist)
  const int span = min(FV_VOX, n - i_blk) * ncls;
  for (int e = tid; e < 8 * span; e += 256) {
    const int o = e / span, r = e - o * span;
    p.out[((size_t)o * n + i_blk) * ncls + r] = s_o[o * FV_VOX * ncls + r];
  }
}

extern "C" int coocc_fine_vox(const float* Q, int X, int Y, int Z, const int32_t* coarse_lin, int n_cap, const int32_t* n_dev,
                              const int* final_size_host, const float* b_f0, const float* gn_f0_w, const float* gn_f0_b, float eps_f0,
                              const float* w_f3, const float* b_f3, int ncls, int64_t* fine_xyz, float* out, void* stream) {
  COOCC_CHECK_ARG(Q && coarse_lin && final_size_host && b_f0 && gn_f0_w && gn_f0_b && w_f3 && b_f3 && fine_xyz && out,
                  "fine_vox: null pointer");
  COOCC_CHECK_ARG(X > 0 && Y > 0 && Z > 0 && n_cap >= 0 && ncls > 0 && ncls <= 32 && (long long)X * Y * Z < (1ll << 31) &&
                      n_cap <= (long long)X * Y * Z,
                  "fine_vox: ncls <= 32, n_cap <= X Y Z < 2^31");
  // the 3-wide window needs floor(p) of the two children of an axis to differ by <= 1: true for final == 2 * coarse
  COOCC_CHECK_ARG(final_size_host[0] == 2 * X && final_size_host[1] == 2 * Y && final_size_host[2] == 2 * Z,
                  "fine_vox: final_occ_size must be 2 x the coarse grid (cascade ratio 2)");
  COOCC_CHECK_ARG(((uintptr_t)Q | (uintptr_t)b_f0 | (uintptr_t)gn_f0_w | (uintptr_t)gn_f0_b | (uintptr_t)w_f3) % 16 == 0,
                  "fine_vox: arrays must be 16-byte aligned");
  if (n_cap == 0) return COOCC_OK;
  FineVox p;
  p.Q = Q; p.X = X; p.Y = Y; p.Z = Z; p.lin = coarse_lin; p.n_cap = n_cap; p.n_dev = n_dev;
  p.fx1 = (float)(final_size_host[0] - 1); p.fy1 = (float)(final_size_host[1] - 1); p.fz1 = (float)(final_size_host[2] - 1);
  p.b0 = b_f0; p.gamma = gn_f0_w; p.beta = gn_f0_b; p.eps = eps_f0; p.w3 = w_f3; p.b3 = b_f3; p.ncls = ncls;
  p.xyz = fine_xyz; p.out = out;
  hipLaunchKernelGGL(k_fine_vox, dim3(cdiv(n_cap, FV_VOX)), dim3(256), fv_lds_bytes(ncls), as_stream(stream), p);
  COOCC_LAUNCH_CHECK("k_fine_vox");
  return COOCC_OK;
}
