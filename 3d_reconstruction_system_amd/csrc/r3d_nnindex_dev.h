// The nearest-neighbour index's layout, shared by its query kernels (r3d_nnindex.hip) and the k-NN / outlier kernels that
// walk the same tables (r3d_knn.hip).  Internal to libr3d_hip.so.
#pragma once

#include "r3d_internal.h"

struct r3d_nn_index {
  r3d_ctx* ctx = nullptr;
  int device = 0;  // kept so that destroy never has to touch a ctx that may already be gone
  int64_t n = 0;
  int64_t capacity = 0;  // target points the allocations can hold (r3d_nn_index_rebuild reuses them)
  int64_t n_tiles = 0;
  int idx_bits = 1, axis_bits = 16;
  float* d_tgt = nullptr;      // [n][3] original order (tie winners of other groups, pair sums, the plane kernels' gathers)
  float4* d_tgt4 = nullptr;    // [n_tiles*1024] sorted, w = original index bits; padding has x = +inf
  float* d_tile_box = nullptr; // [n_tiles][6] lo xyz, hi xyz
  float* d_sub_box = nullptr;  // [n_tiles*4][6] boxes of the 256-target quarters of every tile
  float* d_group_box = nullptr;  // [n_tiles*32][6] boxes of the 32-target groups (staged in LDS with a swept tile)
  float* d_super_box = nullptr; // [ceil(n_tiles/16)][6] boxes of 16 consecutive tiles
  uint64_t* d_tile_code = nullptr;  // [n_tiles] Morton code (without index bits) of the tile's first target
  float* d_frame = nullptr;    // [8]: lo xyz, scale xyz, unused: quantisation frame shared by both clouds
  unsigned long long* d_knn_groups = nullptr;  // [1]: 32-target groups the last k-NN / outlier call evaluated, summed over waves
  void* d_slab = nullptr;      // ONE allocation holds every table above (eight hipMalloc / hipFree pairs per index were a
                               // measurable share of a 10 ms estimate)
  // warm start (see nn_cull_kernel): the buffers of the last presorted query against this build of the index
  const float* warm_src = nullptr;
  const uint32_t* warm_idx = nullptr;
  int64_t warm_n = 0;
};

namespace r3d_nn {

constexpr int kTile = 1024;
constexpr int kGroup = 32;
constexpr int kSub = 256;  // targets per sub-tile (wave-level culling inside a swept tile)
constexpr int kSuper = 16;  // tiles per super-box (workgroup-level culling of 16 tiles at once)
constexpr float kShrink = 1.0f - 16.0f * 5.9604645e-8f;  // (1 - 16u): makes the box bound a strict lower bound

struct __attribute__((packed, aligned(4))) P3 {
  float x, y, z;
};

__device__ __forceinline__ uint64_t spread3(uint32_t v) {
  uint64_t x = v & 0xffffu;
  x = (x | x << 16) & 0x0000ff0000ffull;
  x = (x | x << 8) & 0x00f00f00f00full;
  x = (x | x << 4) & 0x0c30c30c30c3ull;
  x = (x | x << 2) & 0x249249249249ull;
  return x;
}

__device__ __forceinline__ uint64_t point_code(const P3& p, const float* __restrict__ frame, int axis_bits) {
  const float top = (float)((1 << axis_bits) - 1);
  const float q[3] = {(p.x - frame[0]) * frame[3], (p.y - frame[1]) * frame[4], (p.z - frame[2]) * frame[5]};
  uint32_t k[3];
#pragma unroll
  for (int a = 0; a < 3; ++a) k[a] = (uint32_t)fminf(fmaxf(q[a], 0.f), top);  // NaN -> 0
  return spread3(k[0]) | (spread3(k[1]) << 1) | (spread3(k[2]) << 2);
}

}  // namespace r3d_nn
