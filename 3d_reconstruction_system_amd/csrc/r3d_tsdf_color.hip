// Colours of the TSDF volume's surface points for gfx950 (MI355X), from the colour plane that r3d_tsdf.hip's integration kernel
// fills (its <COLOR> variant; the r3d_tsdf_integrate_rgb* entry points are there too).  Semantics: include/r3d.h ("TSDF colour").
//
//   tsdf_emit_colors_kernel     r3d_tsdf_extract_points' write step (r3d_compact_dev.h) for the colours: r3d_tsdf.hip's count
//                               kernel and the tile scan give the tiles' prefixes (r3d_tsdf_count_points), every tile writes its
//                               colour words at its start -- the rows of the points, no atomics on the output cursor.
#include "r3d_compact_dev.h"
#include "r3d_internal.h"
#include "r3d_tsdf_dev.h"

using namespace r3d_tsdf_dev;

namespace {

constexpr int kThreads = 256;
using r3d_compact::kPer;   // consecutive voxels per thread of the extraction kernels

// prefix: the tiles' exclusive prefixes (r3d_tsdf_count_points)
__global__ __launch_bounds__(kThreads) void tsdf_emit_colors_kernel(const float2* __restrict__ vol, const uint4* __restrict__ col, TsdfGrid g,
                                                                    int64_t n, float mw, const uint32_t* __restrict__ prefix,
                                                                    uint32_t* __restrict__ rgba_out, uint64_t cap) {
  const int64_t base = r3d_compact::tile_base();
  uint64_t mask = 0;   // 3 bits per voxel, voxel-major: the order of the output
#pragma unroll 4
  for (int e = 0; e < kPer; ++e)
    if (base + e < n) mask |= (uint64_t)crossings(vol, g, base + e, mw) << (3 * e);
  __shared__ uint64_t wave_total[kThreads / 64];
  const uint64_t at = r3d_compact::tile_start(prefix, (uint64_t)__popcll(mask), wave_total);
  emit_colors(vol, col, g, base, mask, at, cap, rgba_out);
}

}  // namespace

int r3d_tsdf_colors(r3d_tsdf* v, uint32_t** d_sums_out, int64_t* n_voxels_out) {
  int rc = r3d_tsdf_require_color(v);
  if (rc) return rc;
  if (d_sums_out) *d_sums_out = reinterpret_cast<uint32_t*>(v->d_col);
  if (n_voxels_out) *n_voxels_out = v->n;
  return R3D_OK;
}

int r3d_tsdf_extract_colors(r3d_tsdf* v, double min_weight, uint32_t* d_rgba_out, int64_t cap, int64_t* n_out) {
  float mw = 0.0f;
  int rc = r3d_tsdf_extract_checks(v, n_out != nullptr, "n_out", min_weight, &mw, "cap", {{d_rgba_out, cap, "d_rgba_out", "cap"}});
  if (rc || (rc = r3d_tsdf_require_color(v))) return rc;
  const uint32_t* prefix = nullptr;
  int tiles = 0;
  int64_t m = 0;
  if ((rc = r3d_tsdf_count_points(v, mw, &prefix, &tiles, &m))) return rc;
  *n_out = m;
  const uint64_t rows = (uint64_t)(m < cap ? m : cap);
  if (rows == 0) return R3D_OK;
  r3d_wrote(v->ctx, d_rgba_out, (size_t)rows * 4);
  hipLaunchKernelGGL(tsdf_emit_colors_kernel, dim3(tiles), dim3(kThreads), 0, v->ctx->stream, (const float2*)v->d_vol,
                     (const uint4*)v->d_col, v->g, v->n, mw, prefix, d_rgba_out, rows);
  R3D_HIP(hipGetLastError());
  return R3D_OK;
}
