// Multi-view depth consistency for gfx950 (MI355X): every pixel of every frame is checked against the depth maps of the frame's
// sources, and the kept rows of a fused cloud are compacted.  Semantics: include/r3d.h ("Depth consistency"); every output bit is a
// short chain of IEEE f32 operations in the order written there (the library builds with -ffp-contract=off).
//
//   consistency_kernel   one lane = one reference pixel, the source loop INSIDE: the reference depth is read once, every output is
//                        stored once.  One frame per blockIdx.y, so the frame's relative pose rows (and the source index each row
//                        carries in its padding) are wave-uniform and come through scalar loads.  The votes are a function of the
//                        pixel alone: no LDS, no atomics.
//                        Tile: a workgroup owns 32 x 8 pixels, a wave 32 x 2 (lane = 32 row + column).  A raster row is contiguous
//                        and a cache line is 128 bytes of it, so what a wave's gathers cost is the number of ROWS its footprint
//                        in the source touches: a 32 x 2 strip lands on 2-3 source rows under yaw and translation and on about
//                        32 sin(roll) more under roll, an 8 x 8 tile on 8-9 whatever the motion -- and 8 source pixels of a u8
//                        raster are 8 bytes of a 128-byte line.  The wave's own accesses come out whole: a row of the strip is 32 /
//                        64 / 128 contiguous bytes of the u8 / u16 / f32 raster, 64 bytes of the votes, 128 of the filtered raster.
//                        The four waves of a workgroup stack vertically, so the CU's L1 sees one compact 32 x 8 footprint.
//   mask_count_kernel    the filtered cloud, the compaction step of r3d_compact_dev.h: kept rows per tile of 4096, the tile scan,
//   mask_write_kernel    every tile writes its rows (and colour words) at its start, while they are below the caller's cap.
// This file is the device side: the kernels and their launches (declared in r3d_internal.h).  The entry points -- argument checks,
// the fp64 relative poses, workspaces, staging of host rasters -- are host code and live in r3d_consistency_host.cpp, the split of
// r3d_octree.hip and r3d_octree_host.cpp.
#include "r3d_compact_dev.h"
#include "r3d_internal.h"
#include "r3d_tsdf_dev.h"

#include <cmath>

using r3d_tsdf_dev::TsdfCam;
using r3d_tsdf_dev::TsdfPoseRow;

namespace {

constexpr int kThreads = 256;
constexpr int kTileW = 32, kTileH = 8;    // pixels of a workgroup's tile: four waves of 32 x 2, stacked
constexpr int kMaxGridY = 65535;          // frames per launch
using r3d_compact::kPer;

using Rule = r3d_consistency_rule;

// grid: (tiles_x * tiles_y, frames of this launch); rows: [F][n_sources] relative poses of ALL frames, frame0: the launch's first
template <typename D>
__global__ __launch_bounds__(kThreads) void consistency_kernel(const D* __restrict__ depth, TsdfCam cam, uint32_t height, uint32_t tiles_x,
                                                               const TsdfPoseRow* __restrict__ rows, int n_sources, uint32_t frame0,
                                                               Rule rule, uint8_t* __restrict__ votes, uint8_t* __restrict__ keep,
                                                               float* __restrict__ filtered) {
  const uint32_t tile_y = blockIdx.x / tiles_x, tile_x = blockIdx.x - tile_y * tiles_x;
  const uint32_t wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const uint32_t ui = tile_x * kTileW + (lane & 31);
  const uint32_t vi = tile_y * kTileH + wave * 2 + (lane >> 5);
  if (ui >= (uint32_t)cam.width || vi >= height) return;
  const uint32_t frame = frame0 + blockIdx.y;
  const size_t px = (size_t)frame * cam.frame_px + (vi * (uint32_t)cam.width + ui);   // < F H W < 2^31
  const float Z = (float)depth[px] * cam.scale;
  uint32_t consistent = 0, violations = 0;
  if (Z > 0.0f && Z < INFINITY) {
    const float x = (((float)ui - cam.cx) / cam.fx) * Z;
    const float y = (((float)vi - cam.cy) / cam.fy) * Z;
    const TsdfPoseRow* mine = rows + (size_t)frame * n_sources;
    for (int k = 0; k < n_sources; ++k) {
      const TsdfPoseRow fr = mine[k];   // wave-uniform: scalar loads
      const int s = __float_as_int(fr.pad[0]);   // the source's index rides in the row's padding (r3d_consistency_host.cpp); -1: empty
      if (s < 0) continue;
      float pz;
      uint32_t at;
      if (!r3d_tsdf_dev::project_to_pixel(fr, cam, x, y, Z, pz, at)) continue;
      const float d = (float)depth[(size_t)s * cam.frame_px + at] * cam.scale;
      if (!(d > 0.0f && d < INFINITY)) continue;
      const float diff = d - pz, tol = rule.rel_tol * pz;
      if (fabsf(diff) <= tol) ++consistent;
      else if (diff > 0.0f) ++violations;
    }
  }
  const bool kept = (int)consistent >= rule.min_consistent && (int)violations <= rule.max_violations && Z > 0.0f && Z < INFINITY;
  if (votes) *reinterpret_cast<uchar2*>(votes + 2 * px) = uchar2{(uint8_t)consistent, (uint8_t)violations};
  if (keep) keep[px] = kept ? 1 : 0;
  if (filtered) filtered[px] = kept ? Z : 0.0f;
}

__global__ __launch_bounds__(kThreads) void mask_count_kernel(const uint8_t* __restrict__ keep, int64_t n, uint32_t* __restrict__ hist) {
  const int64_t base = r3d_compact::tile_base();
  uint32_t c = 0;
#pragma unroll
  for (int e = 0; e < kPer; ++e)
    if (base + e < n) c += keep[base + e] != 0;
  __shared__ uint32_t sh[kThreads / 64];
  r3d_compact::publish(hist, r3d_compact::block_sum(c, sh));
}

struct P3 {
  float x, y, z;
};

// hist: the tiles' exclusive prefixes; rows at or beyond cap are not written
__global__ __launch_bounds__(kThreads) void mask_write_kernel(const float* __restrict__ xyz, const uint32_t* __restrict__ rgba, int64_t n,
                                                              const uint8_t* __restrict__ keep, const uint32_t* __restrict__ hist,
                                                              float* __restrict__ xyz_out, uint32_t* __restrict__ rgba_out, uint64_t cap) {
  const int64_t base = r3d_compact::tile_base();
  uint32_t mask = 0;
#pragma unroll
  for (int e = 0; e < kPer; ++e)
    if (base + e < n && keep[base + e] != 0) mask |= 1u << e;
  __shared__ uint64_t wave_total[kThreads / 64];
  uint64_t at = r3d_compact::tile_start(hist, (uint64_t)__popc(mask), wave_total);
  const P3* src = reinterpret_cast<const P3*>(xyz);
  P3* dst = reinterpret_cast<P3*>(xyz_out);
  while (mask && at < cap) {
    const int e = __ffs(mask) - 1;
    mask &= mask - 1;
    dst[at] = src[base + e];
    if (rgba_out) rgba_out[at] = rgba[base + e];
    ++at;
  }
}

template <typename D>
void launch_consistency(r3d_ctx* ctx, const TsdfCam& c, int height, const void* d_depth, const TsdfPoseRow* d_rows, int n_frames,
                        int n_sources, const Rule& rule, uint8_t* d_votes, uint8_t* d_keep, float* d_filtered) {
  const uint32_t tiles_x = ((uint32_t)c.width + kTileW - 1) / kTileW, tiles_y = ((uint32_t)height + kTileH - 1) / kTileH;
  for (int lo = 0; lo < n_frames; lo += kMaxGridY) {
    const int n = n_frames - lo < kMaxGridY ? n_frames - lo : kMaxGridY;
    hipLaunchKernelGGL(consistency_kernel<D>, dim3(tiles_x * tiles_y, (unsigned)n), dim3(kThreads), 0, ctx->stream,
                       static_cast<const D*>(d_depth), c, (uint32_t)height, tiles_x, d_rows, n_sources, (uint32_t)lo, rule, d_votes, d_keep,
                       d_filtered);
  }
}

}  // namespace

void r3d_consistency_launch(r3d_ctx* ctx, const r3d_camera* cam, double depth_scale, const void* d_depth, int depth_dtype, const void* d_rows,
                            int n_frames, int n_sources, const r3d_consistency_rule& rule, uint8_t* d_votes, uint8_t* d_keep,
                            float* d_filtered) {
  const TsdfCam c = r3d_tsdf_dev::tsdf_cam_of(cam, depth_scale);
  const TsdfPoseRow* rows = static_cast<const TsdfPoseRow*>(d_rows);
  if (depth_dtype == R3D_DEPTH_U8) launch_consistency<uint8_t>(ctx, c, cam->height, d_depth, rows, n_frames, n_sources, rule, d_votes, d_keep, d_filtered);
  else if (depth_dtype == R3D_DEPTH_U16) launch_consistency<uint16_t>(ctx, c, cam->height, d_depth, rows, n_frames, n_sources, rule, d_votes, d_keep, d_filtered);
  else launch_consistency<float>(ctx, c, cam->height, d_depth, rows, n_frames, n_sources, rule, d_votes, d_keep, d_filtered);
}

void r3d_mask_count_launch(r3d_ctx* ctx, const uint8_t* d_keep, int64_t n, int tiles, uint32_t* hist) {
  hipLaunchKernelGGL(mask_count_kernel, dim3(tiles), dim3(kThreads), 0, ctx->stream, d_keep, n, hist);
}

void r3d_mask_write_launch(r3d_ctx* ctx, const float* d_xyz, const uint32_t* d_rgba, int64_t n, const uint8_t* d_keep, int tiles,
                           const uint32_t* hist, float* d_xyz_out, uint32_t* d_rgba_out, uint64_t rows) {
  hipLaunchKernelGGL(mask_write_kernel, dim3(tiles), dim3(kThreads), 0, ctx->stream, d_xyz, d_rgba, n, d_keep, hist, d_xyz_out, d_rgba_out,
                     rows);
}
