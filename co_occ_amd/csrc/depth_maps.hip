// LiDAR depth maps from the raw point cloud (co_occ_amd/depth_maps.py): the reference's CreateDepthFromLiDAR
// (P/datasets/pipelines/lidar2depth.py:19-41, 63-85) -- the key-frame cloud projected into every camera and the nearest depth per
// pixel kept -- without the N x H x W map ever being made on the host.
//
// The projection (csrc/lidar_project.h, shared with occ_gt.hip) is the reference's fp32 operations in their order: this file is compiled
// with -ffp-contract=off (build.FILE_FLAGS).  A fused chain gives other u, v or d for six pairs in ten and changes one written pixel in six.
// A pair is valid where u >= 0 & v >= 0 & u <= W-1 & v <= H-1 & d > 0 on the unrounded values (a NaN fails every test); its pixel
// is (rint(v), rint(u)), half to even.
//
// The reference sorts by depth and lets an indexed assignment with repeated indices decide, which has no defined order.  Here a pixel
// holds the MINIMUM d over the valid pairs that round to it and 0 where there is none: order-independent, the same bits from run to
// run and for every order of the points.  d > 0 is part of the valid test, positive floats order as their bit patterns, so 0 is free
// to mean "empty" and the minimum is a compare-and-swap loop on the pixel's 32 bits -- no float atomics, no pass over the pixels but
// the zero fill.
//
// k_points_to_depth_maps: a thread owns one point and walks the cameras; a camera record is addressed by kernel arguments and the
// loop counter alone, so its 27 floats are scalar loads.  ~35 k points x 6 cameras against a 4 - 34 MB fill: latency-bound.
#include "common.h"
#include "lidar_project.h"

__global__ __launch_bounds__(256) COOCC_SCALAR_FP32 void k_points_to_depth_maps(const float* __restrict__ points, long long P, int point_stride,
                                                                                const float* __restrict__ cams, int N, int H, int W,
                                                                                unsigned int* __restrict__ maps) {
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  if (i >= P) return;
  const float* p = points + (size_t)i * point_stride;
  const float x = p[0], y = p[1], z = p[2];
  const float umax = (float)(W - 1), vmax = (float)(H - 1);
  for (int cam = 0; cam < N; ++cam) {
    float u, v, d;
    lidar_project(cams + (size_t)cam * LIDAR_CAM_FLOATS, x, y, z, u, v, d);
    if (!(u >= 0.f && v >= 0.f && u <= umax && v <= vmax && d > 0.f)) continue;
    const int px = (int)rintf(u), py = (int)rintf(v);          // 0 .. W-1, 0 .. H-1 by the test above
    unsigned int* cell = maps + ((size_t)cam * H + py) * W + px;
    const unsigned int mine = __float_as_uint(d);              // > 0
    unsigned int seen = __hip_atomic_load(cell, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    while (seen == 0u || mine < seen) {          // a failed exchange leaves the pixel's current bits in `seen`
      if (__hip_atomic_compare_exchange_strong(cell, &seen, mine, __ATOMIC_RELAXED, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) break;
    }
  }
}

extern "C" int coocc_points_to_depth_maps(const float* points, int64_t P, int point_stride, const float* cams, int N, int H, int W,
                                          float* maps, void* stream) {
  COOCC_CHECK_ARG((points || P == 0) && cams && maps, "points_to_depth_maps: null points / cams / maps");          // an empty cloud has no address
  COOCC_CHECK_ARG(N >= 1 && N <= 65535, "points_to_depth_maps: N = %d cameras (1 .. 65535)", N);
  COOCC_CHECK_ARG(H >= 1 && W >= 1 && H <= (1 << 24) && W <= (1 << 24), "points_to_depth_maps: map size %d x %d (1 .. 2^24 per side)", H, W);
  COOCC_CHECK_ARG(P >= 0 && P < (1LL << 38), "points_to_depth_maps: P = %lld points", (long long)P);
  COOCC_CHECK_ARG(point_stride >= 3, "points_to_depth_maps: point_stride = %d floats (3 at least)", point_stride);
  COOCC_HIP(hipMemsetAsync(maps, 0, (size_t)N * H * W * sizeof(float), as_stream(stream)));
  if (P == 0) return COOCC_OK;
  hipLaunchKernelGGL(k_points_to_depth_maps, dim3(cdiv(P, 256)), dim3(256), 0, as_stream(stream), points, (long long)P, point_stride, cams, N,
                     H, W, reinterpret_cast<unsigned int*>(maps));
  COOCC_LAUNCH_CHECK("k_points_to_depth_maps");
  return COOCC_OK;
}
