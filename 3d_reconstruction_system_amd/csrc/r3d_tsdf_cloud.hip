// An oriented cloud into the dense TSDF volume (gfx950, MI355X): every voxel within sdf_trunc of the cloud takes the signed distance
// to the tangent plane of its NEAREST point (Hoppe et al.), as one more frame of the volume's running average.  The kernels and
// their launches; the drivers (workspaces, chunking, the NN query between centres and apply) are in r3d_tsdf_cloud_host.cpp.
// Semantics: include/r3d.h ("TSDF from an oriented cloud"); the volume itself: r3d_tsdf.hip / r3d_tsdf_dev.h.
//
// Most of a volume is farther than sdf_trunc from every point, so the work is limited to a band of 4 x 4 x 4 voxel blocks:
//   cloud_mark_kernel    one lane per point: the blocks its sdf_trunc box overlaps (widened by a voxel and by the f32 rounding of
//                        the centres, so the band is a superset of what the rule accepts) get their bit in a block bitmap.
//                        atomicOr is idempotent, so the bitmap does not depend on the order of the lanes; a bit that is set
//                        already is not set again.  Non-finite points and boxes that miss the volume mark nothing.
//   cloud_count_kernel   the compaction step of r3d_compact_dev.h over the bitmap's words: the marked blocks' numbers in ascending
//   cloud_list_kernel    order, fixed by construction.
//   cloud_centres_kernel one lane per voxel of a chunk of listed blocks (a wave is one block, x fastest): the voxel's centre as a
//                        query point; NaN for the voxels of a block that hang over the volume's faces (a NaN query matches nothing).
//   -- r3d_nn_index_query finds every centre's nearest point: the exact d2 expression and tie rule are inherited, not restated --
//   cloud_apply_kernel   the same lanes: d2 <= tr * tr and the normal decide; one 8-byte read and write of the voxel (one 16-byte
//                        pair of the colour record), four lanes contiguous along x.  The touched voxels are counted per workgroup
//                        and added to one counter with an integer atomic: the count does not depend on the order either.
#include "r3d_compact_dev.h"
#include "r3d_internal.h"
#include "r3d_tsdf_dev.h"

#include <cmath>

using namespace r3d_tsdf_dev;

namespace {

constexpr int kThreads = 256;
constexpr int kEdge = 4;                            // voxels per block edge
constexpr int kBlockVoxels = kEdge * kEdge * kEdge;   // = one wave
using r3d_compact::kPer;

struct BlockGrid {
  int bx, by, bz;   // blocks per axis
};

__global__ __launch_bounds__(kThreads) void cloud_mark_kernel(const float* __restrict__ tgt, int64_t n, TsdfGrid g, BlockGrid b,
                                                              uint32_t* bitmap) {
  const int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x;
  if (i >= n) return;
  const double p[3] = {(double)tgt[3 * i], (double)tgt[3 * i + 1], (double)tgt[3 * i + 2]};
  const double o[3] = {(double)g.ox, (double)g.oy, (double)g.oz}, dim[3] = {(double)g.nx, (double)g.ny, (double)g.nz};
  const double vs = (double)g.vs, tr = (double)g.tr;
  int lo[3], hi[3];
#pragma unroll
  for (int a = 0; a < 3; ++a) {
    if (!(fabs(p[a]) < INFINITY)) return;
    // In exact arithmetic voxel idx has its centre within tr of p iff (p - tr - o) / vs - 0.5 <= idx <= (p + tr - o) / vs - 0.5.
    // The rule's f32 centre, difference and d2 each move that by a few ulps of the magnitudes involved: 2^-20 of their sum
    // covers them all, and one voxel more is the margin.
    const double slack = 1.0 + (fabs(o[a]) + fabs(p[a]) + tr + dim[a] * vs) * 0x1p-20 / vs;
    const double l = floor((p[a] - tr - o[a]) / vs - 0.5 - slack), h = ceil((p[a] + tr - o[a]) / vs - 0.5 + slack);
    if (!(h >= 0.0 && l <= dim[a] - 1.0)) return;   // the box misses the volume (NaN too)
    lo[a] = (int)fmax(l, 0.0) / kEdge;
    hi[a] = (int)fmin(h, dim[a] - 1.0) / kEdge;
  }
  for (int z = lo[2]; z <= hi[2]; ++z)
    for (int y = lo[1]; y <= hi[1]; ++y)
      for (int x = lo[0]; x <= hi[0]; ++x) {
        const uint32_t id = (uint32_t)((z * b.by + y) * b.bx + x);   // < 2^31: fewer blocks than voxels
        const uint32_t bit = 1u << (id & 31u);
        // the plain read races with other lanes' atomicOr on purpose: a stale word costs one redundant atomic, never a lost bit
        if (!(bitmap[id >> 5] & bit)) atomicOr(&bitmap[id >> 5], bit);
      }
}

__global__ __launch_bounds__(kThreads) void cloud_count_kernel(const uint32_t* __restrict__ bitmap, int64_t n_words,
                                                               uint32_t* __restrict__ hist) {
  const int64_t base = r3d_compact::tile_base();
  uint32_t c = 0;
#pragma unroll 4
  for (int e = 0; e < kPer; ++e)
    if (base + e < n_words) c += (uint32_t)__popc(bitmap[base + e]);
  __shared__ uint32_t sh[kThreads / 64];
  r3d_compact::publish(hist, r3d_compact::block_sum(c, sh));
}

// hist: the tiles' exclusive prefixes
__global__ __launch_bounds__(kThreads) void cloud_list_kernel(const uint32_t* __restrict__ bitmap, int64_t n_words,
                                                              const uint32_t* __restrict__ hist, uint32_t* __restrict__ list) {
  const int64_t base = r3d_compact::tile_base();
  uint32_t mine = 0;
#pragma unroll 4
  for (int e = 0; e < kPer; ++e)
    if (base + e < n_words) mine += (uint32_t)__popc(bitmap[base + e]);
  __shared__ uint64_t wave_total[kThreads / 64];
  uint64_t at = r3d_compact::tile_start(hist, (uint64_t)mine, wave_total);
  if (!mine) return;
  for (int e = 0; e < kPer && base + e < n_words; ++e) {
    uint32_t w = bitmap[base + e];
    while (w) {
      const int bit = __ffs((int)w) - 1;
      w &= w - 1;
      list[at++] = (uint32_t)(base + e) * 32u + (uint32_t)bit;
    }
  }
}

// lane t of a chunk -> voxel (x, y, z); false when t is past the chunk or the voxel hangs over a face of the volume
__device__ __forceinline__ bool chunk_voxel(const uint32_t* __restrict__ list, uint32_t t, uint32_t n_lanes, const TsdfGrid& g,
                                            const BlockGrid& b, int& x, int& y, int& z) {
  if (t >= n_lanes) return false;
  const uint32_t id = list[t / kBlockVoxels], l = t % kBlockVoxels;
  const uint32_t row = id / (uint32_t)b.bx;
  const uint32_t bz = row / (uint32_t)b.by;
  x = (int)(id - row * (uint32_t)b.bx) * kEdge + (int)(l & 3u);
  y = (int)(row - bz * (uint32_t)b.by) * kEdge + (int)((l >> 2) & 3u);
  z = (int)bz * kEdge + (int)(l >> 4);
  return x < g.nx && y < g.ny && z < g.nz;
}

__global__ __launch_bounds__(kThreads) void cloud_centres_kernel(const uint32_t* __restrict__ list, uint32_t n_lanes, TsdfGrid g, BlockGrid b,
                                                                 float* __restrict__ q) {
  const uint32_t t = blockIdx.x * (uint32_t)kThreads + threadIdx.x;
  if (t >= n_lanes) return;
  int x, y, z;
  const bool inside = chunk_voxel(list, t, n_lanes, g, b, x, y, z);
  q[3 * (size_t)t + 0] = inside ? centre(g.ox, x, g.vs) : NAN;
  q[3 * (size_t)t + 1] = inside ? centre(g.oy, y, g.vs) : NAN;
  q[3 * (size_t)t + 2] = inside ? centre(g.oz, z, g.vs) : NAN;
}

template <bool COLOR>
__global__ __launch_bounds__(kThreads) void cloud_apply_kernel(const uint32_t* __restrict__ list, uint32_t n_lanes, TsdfGrid g, BlockGrid b,
                                                               const uint32_t* __restrict__ idx, const float* __restrict__ d2,
                                                               const float* __restrict__ tgt, const float* __restrict__ normals,
                                                               const uint32_t* __restrict__ rgba, uint32_t n_points,
                                                               float2* __restrict__ vol, uint4* __restrict__ col,
                                                               unsigned long long* __restrict__ touched) {
  const uint32_t t = blockIdx.x * (uint32_t)kThreads + threadIdx.x;
  int x, y, z;
  uint32_t hit = 0;
  if (chunk_voxel(list, t, n_lanes, g, b, x, y, z)) {
    const uint32_t j = idx[t];
    if (d2[t] <= g.tr * g.tr && j < n_points) {   // a voxel without a finite pair has d2 = +inf
      const float nx = normals[3 * (size_t)j], ny = normals[3 * (size_t)j + 1], nz = normals[3 * (size_t)j + 2];
      const bool finite = fabsf(nx) < INFINITY && fabsf(ny) < INFINITY && fabsf(nz) < INFINITY;
      if (finite && (nx != 0.0f || ny != 0.0f || nz != 0.0f)) {
        const float px = tgt[3 * (size_t)j], py = tgt[3 * (size_t)j + 1], pz = tgt[3 * (size_t)j + 2];
        const float cx = centre(g.ox, x, g.vs), cy = centre(g.oy, y, g.vs), cz = centre(g.oz, z, g.vs);
        const float s = ((cx - px) * nx + (cy - py) * ny) + (cz - pz) * nz;
        const float tn = fmaxf(-1.0f, fminf(1.0f, s / g.tr));
        const size_t i = ((size_t)z * (size_t)g.ny + (size_t)y) * (size_t)g.nx + (size_t)x;
        float2 v = vol[i];
        const float w1 = v.y + 1.0f;
        v.x = (v.x * v.y + tn) / w1;
        v.y = w1;
        vol[i] = v;
        if constexpr (COLOR) {
          const uint32_t word = rgba[j];
          uint4 c = col[i];
          c.x += word & 0xffu;
          c.y += (word >> 8) & 0xffu;
          c.z += (word >> 16) & 0xffu;
          c.w += 1u;
          col[i] = c;
        }
        hit = 1;
      }
    }
  }
  __shared__ uint32_t sh[kThreads / 64];
  const uint32_t total = r3d_compact::block_sum(hit, sh);
  if (threadIdx.x == 0 && total) atomicAdd(touched, (unsigned long long)total);
}

}  // namespace

// ---- the launches r3d_tsdf_cloud_host.cpp drives (asynchronous on the ctx stream, arguments checked by then) --------------------------
static BlockGrid block_grid(const TsdfGrid& g) { return BlockGrid{(g.nx + kEdge - 1) / kEdge, (g.ny + kEdge - 1) / kEdge, (g.nz + kEdge - 1) / kEdge}; }

int64_t r3d_tsdf_cloud_blocks(const TsdfGrid& g) {
  const BlockGrid b = block_grid(g);
  return (int64_t)b.bx * b.by * b.bz;
}

void r3d_tsdf_cloud_mark_launch(r3d_ctx* ctx, const float* d_tgt, int64_t n, const TsdfGrid& g, uint32_t* d_bitmap) {
  hipLaunchKernelGGL(cloud_mark_kernel, dim3((unsigned)((n + kThreads - 1) / kThreads)), dim3(kThreads), 0, ctx->stream, d_tgt, n, g,
                     block_grid(g), d_bitmap);
}

void r3d_tsdf_cloud_count_launch(r3d_ctx* ctx, const uint32_t* d_bitmap, int64_t n_words, int tiles, uint32_t* hist) {
  hipLaunchKernelGGL(cloud_count_kernel, dim3(tiles), dim3(kThreads), 0, ctx->stream, d_bitmap, n_words, hist);
}

void r3d_tsdf_cloud_list_launch(r3d_ctx* ctx, const uint32_t* d_bitmap, int64_t n_words, int tiles, const uint32_t* hist, uint32_t* d_list) {
  hipLaunchKernelGGL(cloud_list_kernel, dim3(tiles), dim3(kThreads), 0, ctx->stream, d_bitmap, n_words, hist, d_list);
}

void r3d_tsdf_cloud_centres_launch(r3d_ctx* ctx, const uint32_t* d_list, uint32_t n_blocks, const TsdfGrid& g, float* d_q) {
  const uint32_t lanes = n_blocks * (uint32_t)kBlockVoxels;
  hipLaunchKernelGGL(cloud_centres_kernel, dim3((lanes + kThreads - 1) / kThreads), dim3(kThreads), 0, ctx->stream, d_list, lanes, g,
                     block_grid(g), d_q);
}

void r3d_tsdf_cloud_apply_launch(r3d_ctx* ctx, const uint32_t* d_list, uint32_t n_blocks, const TsdfGrid& g, const uint32_t* d_idx,
                                 const float* d_d2, const float* d_tgt, const float* d_normals, const uint32_t* d_rgba, uint32_t n_points,
                                 float2* d_vol, uint4* d_col, unsigned long long* d_touched) {
  const uint32_t lanes = n_blocks * (uint32_t)kBlockVoxels;
  const auto kernel = d_rgba ? cloud_apply_kernel<true> : cloud_apply_kernel<false>;
  hipLaunchKernelGGL(kernel, dim3((lanes + kThreads - 1) / kThreads), dim3(kThreads), 0, ctx->stream, d_list, lanes, g, block_grid(g), d_idx,
                     d_d2, d_tgt, d_normals, d_rgba, n_points, d_vol, d_col, d_touched);
}
