// Colour of the dense TSDF volume for gfx950 (MI355X): RGB integration into a second plane and the colours of the surface points.
// Semantics: include/r3d.h ("TSDF colour").  The tsdf / weight plane goes through the very rule the depth-only kernels apply
// (r3d_tsdf_dev.h's integrate_frame), so it comes out bit-identical; the colour plane holds integer sums, so it does not depend
// on the order of the frames or on how a batch is split into calls.
//
//   tsdf_integrate_rgb_kernel   the shape of r3d_tsdf.hip's tsdf_integrate_kernel: one lane = two voxels that follow each other in
//                               x, the frame loop inside, the wave-uniform pose from the volume's ring through scalar loads.  The
//                               lane also loads the pair's two colour records {sum_r, sum_g, sum_b, n} (one 16-byte load each:
//                               a record is 16-byte aligned whatever nx), adds the three bytes of the pixel an accepted frame
//                               read (byte gathers: a colour row is 3 W bytes) and stores every record a frame touched, once.
//                               No LDS, no atomics.
//   tsdf_emit_colors_kernel     r3d_tsdf_extract_points' write step (r3d_compact_dev.h) for the colours: r3d_tsdf.hip's count
//                               kernel and the tile scan give the tiles' prefixes (r3d_tsdf_count_points), every tile writes its
//                               colour words at its start -- the rows of the points, no atomics on the output cursor.
#include "r3d_compact_dev.h"
#include "r3d_internal.h"
#include "r3d_tsdf_dev.h"

using namespace r3d_tsdf_dev;

namespace {

constexpr int kThreads = 256;
constexpr int kChunk = R3D_TSDF_CHUNK;
using r3d_compact::kPer;   // consecutive voxels per thread of the extraction kernels

__device__ __forceinline__ void add_pixel(uint4& c, const uint8_t* __restrict__ rgb, uint32_t pixel) {
  const uint8_t* q = rgb + (size_t)pixel * 3;
  c.x += q[0];
  c.y += q[1];
  c.z += q[2];
  c.w += 1u;
}

// grid: ceil(rows * pairs_per_row / 256) workgroups; lane -> (row, pair) -> voxels x0 = 2 pair and x0 + 1 of row (y, z)
template <typename D, bool VEC>
__global__ __launch_bounds__(kThreads) void tsdf_integrate_rgb_kernel(float2* __restrict__ vol, uint4* __restrict__ col, TsdfGrid g,
                                                                      TsdfCam cam, const D* __restrict__ depth,
                                                                      const uint8_t* __restrict__ rgb, const TsdfPoseRow* __restrict__ table,
                                                                      int n_frames, uint32_t pairs_per_row, uint32_t n_pairs) {
  const uint32_t p = blockIdx.x * (uint32_t)kThreads + threadIdx.x;
  if (p >= n_pairs) return;
  const uint32_t row = p / pairs_per_row;
  const int x0 = (int)(p - row * pairs_per_row) * 2;
  const int z = (int)(row / (uint32_t)g.ny), y = (int)(row - (uint32_t)z * (uint32_t)g.ny);
  const bool has_b = x0 + 1 < g.nx;   // (always true when VEC: nx is even)
  const size_t i = (size_t)row * (size_t)g.nx + (size_t)x0;
  float2* at = vol + i;
  uint4* cat = col + i;
  float2 a, b = float2{0.0f, 0.0f};
  if (VEC) {
    const float4 q = *reinterpret_cast<const float4*>(at);
    a = float2{q.x, q.y};
    b = float2{q.z, q.w};
  } else {
    a = at[0];
    if (has_b) b = at[1];
  }
  uint4 ca = cat[0], cb = uint4{0u, 0u, 0u, 0u};
  if (has_b) cb = cat[1];
  const float cxa = centre(g.ox, x0, g.vs), cxb = centre(g.ox, x0 + 1, g.vs);
  const float cy_ = centre(g.oy, y, g.vs), cz_ = centre(g.oz, z, g.vs);
  bool ta = false, tb = false;
  for (int f = 0; f < n_frames; ++f) {
    const TsdfPoseRow fr = table[f];   // wave-uniform: scalar loads
    const D* frame = depth + (size_t)f * cam.frame_px;
    const uint8_t* image = rgb + (size_t)f * cam.frame_px * 3;
    uint32_t pixel;
    if (integrate_frame(fr, cam, frame, g.tr, cxa, cy_, cz_, a.x, a.y, pixel)) {
      add_pixel(ca, image, pixel);
      ta = true;
    }
    if (integrate_frame(fr, cam, frame, g.tr, cxb, cy_, cz_, b.x, b.y, pixel)) {
      add_pixel(cb, image, pixel);
      tb = true;
    }
  }
  if (VEC) {
    if (ta || tb) *reinterpret_cast<float4*>(at) = float4{a.x, a.y, b.x, b.y};
  } else {
    if (ta) at[0] = a;
    if (tb && has_b) at[1] = b;
  }
  if (ta) cat[0] = ca;
  if (tb && has_b) cat[1] = cb;
}

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

struct ColorVolume {
  r3d_ctx* ctx = nullptr;
  TsdfGrid g = {};
  float2* d_vol = nullptr;
  uint4* d_col = nullptr;
  int64_t n = 0;
};

// the volume's parts, or R3D_ERR_INVALID if it was created without the colour plane
int color_volume(r3d_tsdf* v, ColorVolume* out) {
  R3D_REQUIRE(v != nullptr, "TSDF volume is NULL");
  const float2* vol = nullptr;
  int rc = r3d_tsdf_device_view(v, &out->ctx, &out->g, &vol, &out->n);
  if (rc) return rc;
  out->d_vol = const_cast<float2*>(vol);
  if ((rc = r3d_tsdf_color_plane(v, &out->d_col))) return rc;
  R3D_REQUIRE(out->d_col != nullptr, "the volume was created without colour (r3d_tsdf_create_rgb makes one with)");
  return R3D_OK;
}

template <typename D>
void launch_integrate_rgb(const ColorVolume& cv, const TsdfCam& cam, const void* d_depth, const uint8_t* d_rgb, const TsdfPoseRow* table,
                          int n) {
  const TsdfGrid& g = cv.g;
  const uint32_t ppr = ((uint32_t)g.nx + 1) / 2;
  const uint32_t n_pairs = ppr * (uint32_t)((int64_t)g.ny * g.nz);   // <= nx ny nz < 2^31
  const dim3 grid((n_pairs + kThreads - 1) / kThreads), block(kThreads);
  if (g.nx % 2 == 0)
    hipLaunchKernelGGL((tsdf_integrate_rgb_kernel<D, true>), grid, block, 0, cv.ctx->stream, cv.d_vol, cv.d_col, g, cam,
                       static_cast<const D*>(d_depth), d_rgb, table, n, ppr, n_pairs);
  else
    hipLaunchKernelGGL((tsdf_integrate_rgb_kernel<D, false>), grid, block, 0, cv.ctx->stream, cv.d_vol, cv.d_col, g, cam,
                       static_cast<const D*>(d_depth), d_rgb, table, n, ppr, n_pairs);
}

int integrate_rgb_checks(r3d_tsdf* v, ColorVolume* cv, const r3d_camera* cam, const void* depth, int depth_dtype, int n_frames,
                         double depth_scale, const double* h_pose, const void* rgb) {
  int rc = color_volume(v, cv);
  if (rc) return rc;
  if ((rc = r3d_tsdf_integrate_checks(v, cam, depth, depth_dtype, n_frames, depth_scale, h_pose))) return rc;
  R3D_REQUIRE(n_frames == 0 || rgb != nullptr, "NULL colour pointer");
  return R3D_OK;
}

// the launches of one batch whose rasters and colour images are in HBM; asynchronous
int integrate_rgb_device(r3d_tsdf* v, const ColorVolume& cv, const r3d_camera* cam, const void* d_depth, int depth_dtype, int n_frames,
                         double depth_scale, const double* h_pose, const uint8_t* d_rgb) {
  r3d_ctx* ctx = cv.ctx;
  TsdfCam c;
  c.fx = (float)cam->fx, c.fy = (float)cam->fy, c.cx = (float)cam->cx, c.cy = (float)cam->cy;
  c.wf = (float)cam->width, c.hf = (float)cam->height, c.scale = (float)depth_scale;
  c.width = cam->width;
  c.frame_px = (uint32_t)cam->height * (uint32_t)cam->width;
  const size_t frame_bytes = (size_t)c.frame_px * r3d_depth_size(depth_dtype);
  for (int lo = 0; lo < n_frames; lo += kChunk) {
    const int n = n_frames - lo < kChunk ? n_frames - lo : kChunk;
    TsdfPoseRow *h = nullptr, *d = nullptr;
    hipEvent_t ev = nullptr;
    int rc = r3d_tsdf_pose_slot(v, &h, &d, &ev);
    if (rc) return rc;
    R3D_HIP(hipEventSynchronize(ev));   // the upload that read this slot of the pinned ring last is done
    for (int f = 0; f < n; ++f) {
      const double* p = h_pose + (size_t)(lo + f) * 12;
      for (int k = 0; k < 9; ++k) h[f].r[k] = (float)p[k];
      for (int k = 0; k < 3; ++k) h[f].t[k] = (float)p[9 + k];
      for (int k = 0; k < 4; ++k) h[f].pad[k] = 0.0f;
    }
    R3D_HIP(hipMemcpyAsync(d, h, sizeof(TsdfPoseRow) * n, hipMemcpyHostToDevice, ctx->stream));
    R3D_HIP(hipEventRecord(ev, ctx->stream));
    const void* depth = static_cast<const char*>(d_depth) + (size_t)lo * frame_bytes;
    const uint8_t* rgb = d_rgb + (size_t)lo * c.frame_px * 3;
    if (depth_dtype == R3D_DEPTH_U8) launch_integrate_rgb<uint8_t>(cv, c, depth, rgb, d, n);
    else if (depth_dtype == R3D_DEPTH_U16) launch_integrate_rgb<uint16_t>(cv, c, depth, rgb, d, n);
    else launch_integrate_rgb<float>(cv, c, depth, rgb, d, n);
    R3D_HIP(hipGetLastError());
  }
  return R3D_OK;
}

}  // namespace

int r3d_tsdf_integrate_rgb(r3d_tsdf* v, const r3d_camera* cam, const void* d_depth, int depth_dtype, int n_frames, double depth_scale,
                           const double* h_pose_w2c, const uint8_t* d_rgb) {
  ColorVolume cv;
  int rc = integrate_rgb_checks(v, &cv, cam, d_depth, depth_dtype, n_frames, depth_scale, h_pose_w2c, d_rgb);
  if (rc || n_frames == 0) return rc;
  if ((rc = r3d_ctx_enter(cv.ctx))) return rc;
  return integrate_rgb_device(v, cv, cam, d_depth, depth_dtype, n_frames, depth_scale, h_pose_w2c, d_rgb);
}

int r3d_tsdf_integrate_rgb_host(r3d_tsdf* v, const r3d_camera* cam, const void* h_depth, int depth_dtype, int n_frames, double depth_scale,
                                const double* h_pose_w2c, const uint8_t* h_rgb) {
  ColorVolume cv;
  int rc = integrate_rgb_checks(v, &cv, cam, h_depth, depth_dtype, n_frames, depth_scale, h_pose_w2c, h_rgb);
  if (rc || n_frames == 0) return rc;
  r3d_ctx* ctx = cv.ctx;
  if ((rc = r3d_ctx_enter(ctx))) return rc;
  // the batch goes up in slabs of whole frames through kWsIn, a slab's rasters first, then its colour
  // images (at a 256-byte boundary); every slab is one integrate call
  const size_t px = (size_t)cam->height * cam->width;
  const size_t depth_bytes = px * r3d_depth_size(depth_dtype), rgb_bytes = px * 3, frame_bytes = depth_bytes + rgb_bytes;
  int slab = (int)(((size_t)256 << 20) / (frame_bytes ? frame_bytes : 1));
  if (slab < 1) slab = 1;
  if (slab > n_frames) slab = n_frames;
  const size_t rgb_at = r3d_align_up((size_t)slab * depth_bytes, 256);
  void* d_in = nullptr;
  if ((rc = r3d_scratch(ctx, kWsIn, rgb_at + (size_t)slab * rgb_bytes, &d_in))) return rc;
  uint8_t* d_rgb = static_cast<uint8_t*>(d_in) + rgb_at;
  for (int lo = 0; lo < n_frames; lo += slab) {
    const int n = n_frames - lo < slab ? n_frames - lo : slab;
    if ((rc = r3d_memcpy_h2d(ctx, d_in, static_cast<const char*>(h_depth) + (size_t)lo * depth_bytes, (size_t)n * depth_bytes))) return rc;
    if ((rc = r3d_memcpy_h2d(ctx, d_rgb, h_rgb + (size_t)lo * rgb_bytes, (size_t)n * rgb_bytes))) return rc;
    if ((rc = integrate_rgb_device(v, cv, cam, d_in, depth_dtype, n, depth_scale, h_pose_w2c + (size_t)lo * 12, d_rgb))) return rc;
    R3D_HIP(hipStreamSynchronize(ctx->stream));   // the next slab overwrites the scratch; the caller's memory is free at return
  }
  return R3D_OK;
}

int r3d_tsdf_colors(r3d_tsdf* v, uint32_t** d_sums_out, int64_t* n_voxels_out) {
  ColorVolume cv;
  int rc = color_volume(v, &cv);
  if (rc) return rc;
  if (d_sums_out) *d_sums_out = reinterpret_cast<uint32_t*>(cv.d_col);
  if (n_voxels_out) *n_voxels_out = cv.n;
  return R3D_OK;
}

int r3d_tsdf_extract_colors(r3d_tsdf* v, double min_weight, uint32_t* d_rgba_out, int64_t cap, int64_t* n_out) {
  R3D_REQUIRE(v != nullptr, "TSDF volume is NULL");
  R3D_REQUIRE(n_out != nullptr, "n_out is NULL");
  const float mw = (float)min_weight;
  R3D_REQUIRE(mw > 0.0f, "min_weight must be > 0 in f32");
  R3D_REQUIRE(cap >= 0, "cap must be >= 0");
  R3D_REQUIRE(cap == 0 || d_rgba_out != nullptr, "d_rgba_out is NULL with cap > 0");
  ColorVolume cv;
  int rc = color_volume(v, &cv);
  if (rc) return rc;
  const uint32_t* prefix = nullptr;
  int tiles = 0;
  int64_t m = 0;
  if ((rc = r3d_tsdf_count_points(v, mw, &prefix, &tiles, &m))) return rc;
  *n_out = m;
  const uint64_t rows = (uint64_t)(m < cap ? m : cap);
  if (rows == 0) return R3D_OK;
  r3d_wrote(cv.ctx, d_rgba_out, (size_t)rows * 4);
  hipLaunchKernelGGL(tsdf_emit_colors_kernel, dim3(tiles), dim3(kThreads), 0, cv.ctx->stream, (const float2*)cv.d_vol,
                     (const uint4*)cv.d_col, cv.g, cv.n, mw, prefix, d_rgba_out, rows);
  R3D_HIP(hipGetLastError());
  return R3D_OK;
}
