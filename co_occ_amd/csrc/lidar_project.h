// The LiDAR -> camera projection chain, once: depth_maps.hip (k_points_to_depth_maps) and occ_gt.hip (k_visible_min,
// k_visible_flag) both call lidar_project, so a point lands in the same pixel in the depth maps and in the visibility masks.
//
// The camera record is LIDAR_CAM_FLOATS floats: inv_rot[9] tran[3] intrin[9] post_rot 2x2 [4] post_tran[2] pad.  Three places must
// agree on it: depth_maps.CAM_FLOATS in Python (image_inputs.camera_table makes the records), this header, and include/coocc_hip.h's
// description of `cams` [N][28] at coocc_points_to_depth_maps and coocc_occ_visible_rows.
//
// Per point p, in the reference's fp32 operations and their order:
//   q = p - tran;  c = inv_rot @ q;  k = intrin @ c;  d = k[2];  uv = k[:2] / d;  uv = post_rot @ uv + post_tran
// ATen's CPU bmm of these small matrices rounds every product and adds them left to right, so a row is (a0*x0 + a1*x1) + a2*x2 with
// five roundings, and the division is IEEE (__fdiv_rn).  Every file that includes this header is compiled with -ffp-contract=off
// (build.FILE_FLAGS: a header takes the flags of the file that includes it); a fused chain gives other u, v or d for six pairs in ten.
// u, v and d come back unrounded: the validity test and the rounding to a pixel differ between the callers and stay with them.
#pragma once
#include "common.h"

constexpr int LIDAR_CAM_FLOATS = 28;

__device__ __forceinline__ void lidar_project(const float* __restrict__ C, float x, float y, float z, float& u, float& v, float& d) {
  const float q0 = x - C[9], q1 = y - C[10], q2 = z - C[11];
  const float c0 = (C[0] * q0 + C[1] * q1) + C[2] * q2;
  const float c1 = (C[3] * q0 + C[4] * q1) + C[5] * q2;
  const float c2 = (C[6] * q0 + C[7] * q1) + C[8] * q2;
  const float k0 = (C[12] * c0 + C[13] * c1) + C[14] * c2;
  const float k1 = (C[15] * c0 + C[16] * c1) + C[17] * c2;
  d = (C[18] * c0 + C[19] * c1) + C[20] * c2;
  const float u0 = __fdiv_rn(k0, d), v0 = __fdiv_rn(k1, d);
  u = (C[21] * u0 + C[22] * v0) + C[25];
  v = (C[23] * u0 + C[24] * v0) + C[26];
}
