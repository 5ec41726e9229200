// One sample of an occupancy picture (occ_views.hip): the slab test that defines a hit and the walk through the grid that
// chooses which cubes are asked.  Host and device: the same text can be stepped through on a CPU against a brute-force cast.
// Compiled without contraction (build.py FILE_FLAGS lists occ_views.hip): every fp32 operation below rounds once, in the order
// written, which is the order tests/occ_view_refs.py restates.
#pragma once
#include <math.h>
#include <stddef.h>
#include <stdint.h>

#if defined(__HIP_DEVICE_COMPILE__)
#define OV_RCP(x) __fdiv_rn(1.0f, (x))
#else
#define OV_RCP(x) (1.0f / (x))
#endif
#if defined(__HIPCC__)
#define OV_FN __host__ __device__ __forceinline__
#else
#define OV_FN static inline
#endif

constexpr int OV_MAX_VIEWS = 8;
constexpr float OV_PARALLEL = 1e-30f;      // |d| below this: the axis is decided by containment, 1 / d is never formed

struct OvView {
  float eye[3], fwd[3], R[3], U[3], near, far;
  int col0, pad;
};

struct OvParams {
  OvView view[OV_MAX_VIEWS];
  int V, H, W, S, FW, FH;                  // H x W pixels written per view, S x S samples a pixel, FH x FW the full frame
  float rw, rh;                            // 1 / (FW * S), 1 / (FH * S)
  int X, Y, Z, zw, by;
  int col_words, brick_words;              // 32-bit words of the two parts of `masks`
  float org[3], vs[3], rvs[3], half;
  uint8_t palette[19 * 3];
};

// the ego-car block of draw_nusc_occupancy: x in [X/2 - 6, X/2 + 2), y likewise, z in [Z/2 - 5, Z/2 + 1); the label depends on
// y and z (car_label[y - y0][x - x0][z - z0] after the reference's meshgrid pairing): bands 0:3, 3:6, 6:8 of y, pairs of z
OV_FN int ov_car_label(int x, int y, int k, int X, int Y, int Z) {
  const int a = y - (Y / 2 - 6), b = x - (X / 2 - 6), c = k - (Z / 2 - 5);
  if (a < 0 || a >= 8 || b < 0 || b >= 8 || c < 0 || c >= 6) return -1;
  return 17 + ((a < 3 ? 0 : a < 6 ? 1 : 2) + c / 2) % 3;
}

struct OvRay {
  float e[3], d[3], inv[3];
  bool par[3];
};

// The slab test.  Per axis that is not parallel: ta = (lo - e) * inv, tb = (hi - e) * inv, entry = the larger of the three
// min(ta, tb) (the lowest axis among equals), exit = the smaller of the three max(ta, tb) (likewise).  A parallel axis must
// contain the eye and decides nothing else.
OV_FN bool ov_slab(const OvRay& r, const float (&lo)[3], const float (&hi)[3], float& ten, int& aen, float& tex, int& aex) {
  ten = -INFINITY; tex = INFINITY; aen = 0; aex = 0;
#pragma unroll
  for (int a = 0; a < 3; ++a) {
    if (r.par[a]) {
      if (r.e[a] < lo[a] || r.e[a] > hi[a]) return false;
    } else {
      const float ta = (lo[a] - r.e[a]) * r.inv[a], tb = (hi[a] - r.e[a]) * r.inv[a];
      const float tn = fminf(ta, tb), tf = fmaxf(ta, tb);
      if (tn > ten) { ten = tn; aen = a; }
      if (tf < tex) { tex = tf; aex = a; }
    }
  }
  return ten <= tex;
}

OV_FN int ov_imin(int a, int b) { return a < b ? a : b; }
OV_FN int ov_imax(int a, int b) { return a > b ? a : b; }

// Sample (gx, gy) of the FW*S x FH*S sample frame of view vw -> the winning cube's linear index (-1), the face (255) and t (+inf).
// col: uint16 [X][Y][zw] column words, brick: uint8 [bx][by][zw] flags; every index is clamped into the grid before it is used.
// reads[0] / reads[1]: how many brick flags / column words the walk read (the result does not depend on them).
OV_FN void ov_cast_sample(const OvParams& p, const OvView& vw, const uint16_t* col, const uint8_t* brick, int gx, int gy, int& best_id,
                          int& best_face, float& best_t, unsigned (&reads)[2]) {
  const int dim[3] = {p.X, p.Y, p.Z};
  OvRay r;
  // u, v from integer numerators; d = (fwd + u * R) + v * U
  const float u = (float)(2 * gx + 1 - p.FW * p.S) * p.rw, w = (float)(p.FH * p.S - 2 * gy - 1) * p.rh;
  int step[3];
  float glo[3], ghi[3];
#pragma unroll
  for (int a = 0; a < 3; ++a) {
    r.e[a] = vw.eye[a];
    r.d[a] = (vw.fwd[a] + u * vw.R[a]) + w * vw.U[a];
    r.par[a] = fabsf(r.d[a]) < OV_PARALLEL;
    r.inv[a] = r.par[a] ? INFINITY : OV_RCP(r.d[a]);
    step[a] = r.par[a] ? 0 : (r.d[a] > 0.f ? 1 : -1);
    glo[a] = p.org[a]; ghi[a] = p.org[a] + (float)dim[a] * p.vs[a];
  }
  best_t = INFINITY; best_id = -1; best_face = 255;
  float ten, tex;
  int aen, aex;
  reads[0] = reads[1] = 0;
  if (!ov_slab(r, glo, ghi, ten, aen, tex, aex) || tex < vw.near) return;
  float tcur = fmaxf(ten, 0.f), tlim = vw.far;
  int c[3];
#pragma unroll
  for (int a = 0; a < 3; ++a) {
    const int i = (int)floorf(((r.e[a] + tcur * r.d[a]) - p.org[a]) * p.rvs[a]);
    c[a] = ov_imin(ov_imax(i, 0), dim[a] - 1);
  }
  const int max_steps = 4 * (p.X + p.Y + p.Z) + 64;           // far above what a walk takes; no walk can run on without end
  for (int steps = 0; steps < max_steps && tcur <= tlim; ++steps) {
    // the box the walk leaves next: an empty brick, an empty column word, or the cell
    int sh[3] = {0, 0, 0};
    ++reads[0];
    if (!brick[((c[0] >> 3) * p.by + (c[1] >> 3)) * p.zw + (c[2] >> 4)]) {
      sh[0] = 3; sh[1] = 3; sh[2] = 4;
    } else {
      ++reads[1];
      const unsigned word = col[((size_t)c[0] * p.Y + c[1]) * p.zw + (c[2] >> 4)];
      if (!word) {
        sh[2] = 4;
      } else if ((word >> (c[2] & 15)) & 1) {
        float lo[3], hi[3];
#pragma unroll
        for (int a = 0; a < 3; ++a) {
          const float ctr = p.org[a] + ((float)c[a] + 0.5f) * p.vs[a];
          lo[a] = ctr - p.half; hi[a] = ctr + p.half;
        }
        float cen, cex;
        int cae, cax;
        if (ov_slab(r, lo, hi, cen, cae, cex, cax)) {
          float t = 0.f;
          int face = 0;
          bool hit = true;
          if (cen >= vw.near) { t = cen; face = 2 * cae + (r.d[cae] > 0.f ? 1 : 0); }
          else if (cex >= vw.near) { t = cex; face = 2 * cax + (r.d[cax] > 0.f ? 0 : 1); }
          else hit = false;
          if (hit && t <= vw.far) {
            const int id = (c[0] * p.Y + c[1]) * p.Z + c[2];
            if (t < best_t || (t == best_t && id < best_id)) { best_t = t; best_id = id; best_face = face; tlim = fminf(tlim, t); }
          }
        }
      }
    }
    float tnext = INFINITY;
    int ax = -1, plane = 0;
#pragma unroll
    for (int a = 0; a < 3; ++a) {
      if (step[a] != 0) {
        const int b = c[a] >> sh[a];
        const int pl = step[a] > 0 ? ov_imin((b + 1) << sh[a], dim[a]) : (b << sh[a]);
        const float tp = ((p.org[a] + (float)pl * p.vs[a]) - r.e[a]) * r.inv[a];      // from the integer plane index
        if (tp < tnext) { tnext = tp; ax = a; plane = pl; }
      }
    }
    if (ax < 0) break;
    tcur = fmaxf(tcur, tnext);
    bool out = false;
#pragma unroll
    for (int a = 0; a < 3; ++a) {
      if (a == ax) {
        c[a] = step[a] > 0 ? plane : plane - 1;
        out = c[a] < 0 || c[a] >= dim[a];
      } else if (sh[a] > 0) {
        // the other axes of a skipped box: the cell the ray is in where it leaves, kept inside the box it left
        const int b0 = (c[a] >> sh[a]) << sh[a], b1 = ov_imin(b0 + (1 << sh[a]), dim[a]) - 1;
        const int i = (int)floorf(((r.e[a] + tcur * r.d[a]) - p.org[a]) * p.rvs[a]);
        c[a] = ov_imin(ov_imax(i, b0), b1);
      }
    }
    if (out) break;
  }
}
