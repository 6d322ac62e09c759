// Dense TSDF volume for gfx950 (MI355X): the volume itself, integration of depth frames with or without colour images (all four
// r3d_tsdf_integrate* entry points) and extraction of the zero level set as oriented points.  struct r3d_tsdf, the step through
// its pose ring and the device pieces other files share are in r3d_tsdf_dev.h; the points' colours in r3d_tsdf_color.hip.
// Semantics: include/r3d.h ("TSDF volume", "TSDF colour"); every output bit is a short chain of IEEE f32 operations in the order
// written there (the library builds with -ffp-contract=off; hipcc's f32 division and sqrt are correctly rounded by default).
//
//   tsdf_integrate_kernel   one lane = two voxels that follow each other in x (one 16-byte access when nx is even, two 8-byte
//                           ones otherwise: an odd nx leaves every second row 8-byte aligned only).  The frame loop is INSIDE:
//                           a lane loads its pair once, applies the chunk's frames from registers in ascending order and stores
//                           once -- and only if a frame touched it.  The per-frame pose (12 floats) is wave-uniform and comes
//                           from the volume's pose ring through scalar loads; the depth read is a gather, neighbouring lanes
//                           hitting neighbouring pixels.  No LDS, no atomics.
//                           <COLOR> also loads the pair's two colour records {sum_r, sum_g, sum_b, n} (one 16-byte load each: a
//                           record is 16-byte aligned whatever nx), adds the three bytes of the pixel an accepted frame read
//                           (byte gathers: a colour row is 3 W bytes) and stores every record a frame touched, once.  The tsdf /
//                           weight plane goes through the same statements either way, so it comes out bit-identical; the colour
//                           plane holds integer sums, so it does not depend on the order of the frames or on how a batch is
//                           split into calls.
//   tsdf_count_kernel       extraction, the compaction step of r3d_compact_dev.h: surface points per tile of 4096 voxels, the
//   tsdf_emit_kernel        tile scan, every tile writes its points at its start: linear voxel order, then x, y, z -- fixed by
//                           construction, no atomics on the output cursor.
#include "r3d_compact_dev.h"
#include "r3d_internal.h"
#include "r3d_tsdf_dev.h"

#include <cmath>
#include <new>

using namespace r3d_tsdf_dev;   // TsdfGrid, voxel indexing, crossings, emit_points: shared with r3d_tsdf_mesh.hip

namespace {

constexpr int kThreads = 256;
constexpr int kChunk = R3D_TSDF_CHUNK;   // frames per launch = rows of one slot of the pose ring
constexpr int kSlots = r3d_tsdf::kSlots;
using r3d_compact::kPer;                 // consecutive voxels per thread of the extraction kernels

__device__ __forceinline__ void add_pixel(uint4& c, const uint8_t* __restrict__ rgb, uint32_t pixel) {
  const uint8_t* q = rgb + (size_t)pixel * 3;
  c.x += q[0];
  c.y += q[1];
  c.z += q[2];
  c.w += 1u;
}

// grid: ceil(rows * pairs_per_row / 256) workgroups; lane -> (row, pair) -> voxels x0 = 2 pair and x0 + 1 of row (y, z).
// col, rgb: the colour plane and the frames' colour images when COLOR; unused, and NULL, otherwise (they come last, so the
// depth-only variant finds its arguments where it would without them)
template <typename D, bool VEC, bool COLOR>
__global__ __launch_bounds__(kThreads) void tsdf_integrate_kernel(float2* __restrict__ vol, TsdfGrid g, TsdfCam cam, const D* __restrict__ depth,
                                                                  const TsdfPoseRow* __restrict__ table, int n_frames,
                                                                  uint32_t pairs_per_row, uint32_t n_pairs, uint4* __restrict__ col,
                                                                  const uint8_t* __restrict__ rgb) {
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
  uint4 ca = uint4{0u, 0u, 0u, 0u}, cb = ca;
  if constexpr (COLOR) {
    ca = cat[0];
    if (has_b) cb = cat[1];
  }
  const float cxa = centre(g.ox, x0, g.vs), cxb = centre(g.ox, x0 + 1, g.vs);
  const float cy_ = centre(g.oy, y, g.vs), cz_ = centre(g.oz, z, g.vs);
  bool ta = false, tb = false;
  for (int f = 0; f < n_frames; ++f) {
    const TsdfPoseRow fr = table[f];   // wave-uniform: scalar loads
    const D* frame = depth + (size_t)f * cam.frame_px;
    const uint8_t* image = COLOR ? rgb + (size_t)f * cam.frame_px * 3 : nullptr;
    uint32_t pixel;
    const bool hit_a = integrate_frame(fr, cam, frame, g.tr, cxa, cy_, cz_, a.x, a.y, pixel);
    ta |= hit_a;
    if constexpr (COLOR) if (hit_a) add_pixel(ca, image, pixel);
    const bool hit_b = integrate_frame(fr, cam, frame, g.tr, cxb, cy_, cz_, b.x, b.y, pixel);
    tb |= hit_b;
    if constexpr (COLOR) if (hit_b) add_pixel(cb, image, pixel);
  }
  if (VEC) {
    if (ta || tb) *reinterpret_cast<float4*>(at) = float4{a.x, a.y, b.x, b.y};
  } else {
    if (ta) at[0] = a;
    if (tb && has_b) at[1] = b;
  }
  if constexpr (COLOR) {
    if (ta) cat[0] = ca;
    if (tb && has_b) cat[1] = cb;
  }
}

// ---- extraction ------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kThreads) void tsdf_count_kernel(const float2* __restrict__ vol, TsdfGrid g, int64_t n, float mw,
                                                              uint32_t* __restrict__ hist) {
  const int64_t base = r3d_compact::tile_base();
  uint32_t c = 0;
#pragma unroll 4
  for (int e = 0; e < kPer; ++e)
    if (base + e < n) c += (uint32_t)__popc(crossings(vol, g, base + e, mw));
  __shared__ uint32_t sh[kThreads / 64];
  r3d_compact::publish(hist, r3d_compact::block_sum(c, sh));
}

// hist: the tiles' exclusive prefixes
__global__ __launch_bounds__(kThreads) void tsdf_emit_kernel(const float2* __restrict__ vol, TsdfGrid g, int64_t n, float mw,
                                                             const uint32_t* __restrict__ hist, float* __restrict__ xyz_out,
                                                             float* __restrict__ normals_out, uint64_t cap) {
  const int64_t base = r3d_compact::tile_base();
  uint64_t mask = 0;   // 3 bits per voxel, voxel-major: the order of the output
#pragma unroll 4
  for (int e = 0; e < kPer; ++e)
    if (base + e < n) mask |= (uint64_t)crossings(vol, g, base + e, mw) << (3 * e);
  __shared__ uint64_t wave_total[kThreads / 64];
  const uint64_t at = r3d_compact::tile_start(hist, (uint64_t)__popcll(mask), wave_total);
  emit_points(vol, g, base, mw, mask, at, cap, xyz_out, normals_out);
}

}  // namespace

static int create_volume(r3d_ctx* ctx, const double* h_origin, double voxel_size, int nx, int ny, int nz, double sdf_trunc, bool color,
                         r3d_tsdf** out) {
  R3D_REQUIRE(out != nullptr, "out is NULL");
  *out = nullptr;
  R3D_REQUIRE(ctx != nullptr && h_origin != nullptr, "NULL argument");
  R3D_REQUIRE(nx >= 1 && ny >= 1 && nz >= 1 && (int64_t)nx * ny < ((int64_t)1 << 31) && (int64_t)nx * ny * nz < ((int64_t)1 << 31),
              "volume dimensions %d x %d x %d: every one must be >= 1 and their product below 2^31", nx, ny, nz);
  const float o[3] = {(float)h_origin[0], (float)h_origin[1], (float)h_origin[2]};
  const float vs = (float)voxel_size, tr = (float)sdf_trunc;
  R3D_REQUIRE(std::isfinite(o[0]) && std::isfinite(o[1]) && std::isfinite(o[2]), "origin must be finite in f32");
  R3D_REQUIRE(vs > 0.0f && std::isfinite(vs), "voxel_size must be positive and finite in f32");
  R3D_REQUIRE(tr > 0.0f && std::isfinite(tr), "sdf_trunc must be positive and finite in f32");
  int rc = r3d_ctx_enter(ctx);
  if (rc) return rc;
  r3d_tsdf* v = new (std::nothrow) r3d_tsdf();
  if (!v) {
    r3d_set_error("host allocation failed");
    return R3D_ERR_NOMEM;
  }
  v->ctx = ctx;
  v->device = ctx->device;
  v->g = TsdfGrid{nx, ny, nz, o[0], o[1], o[2], vs, tr};
  v->n = (int64_t)nx * ny * nz;
  hipError_t e = hipMalloc((void**)&v->d_vol, (size_t)v->n * sizeof(float2));
  if (e == hipSuccess && color) e = hipMalloc((void**)&v->d_col, (size_t)v->n * sizeof(uint4));
  if (e == hipSuccess) e = hipMalloc((void**)&v->d_table, sizeof(TsdfPoseRow) * kSlots * kChunk);
  if (e == hipSuccess) e = hipHostMalloc((void**)&v->h_table, sizeof(TsdfPoseRow) * kSlots * kChunk, hipHostMallocDefault);
  for (int s = 0; s < kSlots && e == hipSuccess; ++s) e = hipEventCreateWithFlags(&v->ev[s], hipEventDisableTiming);
  if (e != hipSuccess) {
    r3d_tsdf_destroy(v);
    if (e == hipErrorOutOfMemory) {
      r3d_set_error("a TSDF volume of %d x %d x %d voxels does not fit the device", nx, ny, nz);
      return R3D_ERR_NOMEM;
    }
    return r3d_fail_hip(e, "TSDF volume allocation", __FILE__, __LINE__);
  }
  if ((rc = r3d_tsdf_reset(v))) {
    r3d_tsdf_destroy(v);
    return rc;
  }
  *out = v;
  return R3D_OK;
}

int r3d_tsdf_create(r3d_ctx* ctx, const double* h_origin, double voxel_size, int nx, int ny, int nz, double sdf_trunc, r3d_tsdf** out) {
  return create_volume(ctx, h_origin, voxel_size, nx, ny, nz, sdf_trunc, false, out);
}

int r3d_tsdf_create_rgb(r3d_ctx* ctx, const double* h_origin, double voxel_size, int nx, int ny, int nz, double sdf_trunc, r3d_tsdf** out) {
  return create_volume(ctx, h_origin, voxel_size, nx, ny, nz, sdf_trunc, true, out);
}

int r3d_tsdf_destroy(r3d_tsdf* v) {
  if (!v) return R3D_OK;
  (void)hipSetDevice(v->device);
  (void)hipDeviceSynchronize();
  if (v->d_vol) (void)hipFree(v->d_vol);
  if (v->d_col) (void)hipFree(v->d_col);
  if (v->d_table) (void)hipFree(v->d_table);
  if (v->h_table) (void)hipHostFree(v->h_table);
  for (void* p : v->cloud_buf)
    if (p) (void)hipFree(p);
  for (int s = 0; s < kSlots; ++s)
    if (v->ev[s]) (void)hipEventDestroy(v->ev[s]);
  delete v;
  return R3D_OK;
}

int r3d_tsdf_reset(r3d_tsdf* v) {
  R3D_REQUIRE(v != nullptr, "TSDF volume is NULL");
  int rc = r3d_ctx_enter(v->ctx);
  if (rc) return rc;
  R3D_HIP(hipMemsetAsync(v->d_vol, 0, (size_t)v->n * sizeof(float2), v->ctx->stream));
  if (v->d_col) R3D_HIP(hipMemsetAsync(v->d_col, 0, (size_t)v->n * sizeof(uint4), v->ctx->stream));
  return R3D_OK;
}

int r3d_tsdf_volume(r3d_tsdf* v, float** d_tsdf_weight_out, int64_t* n_voxels_out) {
  R3D_REQUIRE(v != nullptr, "TSDF volume is NULL");
  if (d_tsdf_weight_out) *d_tsdf_weight_out = reinterpret_cast<float*>(v->d_vol);
  if (n_voxels_out) *n_voxels_out = v->n;
  return R3D_OK;
}

int r3d_tsdf_integrate_checks(r3d_tsdf* v, const r3d_camera* cam, const void* depth, int depth_dtype, int n_frames, double depth_scale,
                              const double* h_pose) {
  R3D_REQUIRE(v != nullptr, "TSDF volume is NULL");
  R3D_REQUIRE(cam != nullptr, "camera is NULL");
  R3D_REQUIRE(cam->ctx == v->ctx, "the camera belongs to another context than the volume");
  R3D_REQUIRE(depth_dtype >= R3D_DEPTH_U8 && depth_dtype <= R3D_DEPTH_F32, "unknown depth dtype %d", depth_dtype);
  R3D_REQUIRE(n_frames >= 0, "n_frames must be >= 0");
  if (n_frames == 0) return R3D_OK;
  R3D_REQUIRE(depth != nullptr && h_pose != nullptr, "NULL depth or pose pointer");
  R3D_REQUIRE(cam->width <= (1 << 24) && cam->height <= (1 << 24) && (int64_t)cam->width * cam->height < ((int64_t)1 << 31),
              "raster of %d x %d pixels is too large for the TSDF projection", cam->height, cam->width);
  R3D_REQUIRE(std::isfinite((float)depth_scale), "depth_scale must be finite in f32");
  return R3D_OK;
}

namespace {

// d_rgb: the chunk's colour images for the COLOR kernel into v->d_col, or NULL for the depth-only one (v->d_col is NULL then)
template <typename D>
void launch_integrate(r3d_tsdf* v, const TsdfCam& cam, const void* d_depth, const uint8_t* d_rgb, const TsdfPoseRow* table, int n) {
  const TsdfGrid& g = v->g;
  const uint32_t ppr = ((uint32_t)g.nx + 1) / 2;
  const uint32_t n_pairs = ppr * (uint32_t)((int64_t)g.ny * g.nz);   // <= nx ny nz < 2^31
  const dim3 grid((n_pairs + kThreads - 1) / kThreads), block(kThreads);
  const bool vec = g.nx % 2 == 0;
  const auto kernel = d_rgb ? (vec ? tsdf_integrate_kernel<D, true, true> : tsdf_integrate_kernel<D, false, true>)
                            : (vec ? tsdf_integrate_kernel<D, true, false> : tsdf_integrate_kernel<D, false, false>);
  hipLaunchKernelGGL(kernel, grid, block, 0, v->ctx->stream, v->d_vol, g, cam, static_cast<const D*>(d_depth), table, n, ppr, n_pairs,
                     v->d_col, d_rgb);
}

// the launches of one batch whose rasters (and colour images, unless d_rgb is NULL) are in HBM; asynchronous
int integrate_device(r3d_tsdf* v, const r3d_camera* cam, const void* d_depth, int depth_dtype, int n_frames, double depth_scale,
                     const double* h_pose, const uint8_t* d_rgb) {
  const TsdfCam c = tsdf_cam_of(cam, depth_scale);
  const size_t frame_bytes = (size_t)c.frame_px * r3d_depth_size(depth_dtype);
  for (int lo = 0; lo < n_frames; lo += kChunk) {
    const int n = n_frames - lo < kChunk ? n_frames - lo : kChunk;
    const TsdfPoseRow* d = nullptr;
    int rc = r3d_tsdf_send_rows(v, n, &d, [&](TsdfPoseRow* h) {
      for (int f = 0; f < n; ++f) {
        const double* p = h_pose + (size_t)(lo + f) * 12;
        for (int k = 0; k < 9; ++k) h[f].r[k] = (float)p[k];
        for (int k = 0; k < 3; ++k) h[f].t[k] = (float)p[9 + k];
        for (int k = 0; k < 4; ++k) h[f].pad[k] = 0.0f;
      }
    });
    if (rc) return rc;
    const void* depth = static_cast<const char*>(d_depth) + (size_t)lo * frame_bytes;
    const uint8_t* rgb = d_rgb ? d_rgb + (size_t)lo * c.frame_px * 3 : nullptr;
    if (depth_dtype == R3D_DEPTH_U8) launch_integrate<uint8_t>(v, c, depth, rgb, d, n);
    else if (depth_dtype == R3D_DEPTH_U16) launch_integrate<uint16_t>(v, c, depth, rgb, d, n);
    else launch_integrate<float>(v, c, depth, rgb, d, n);
    R3D_HIP(hipGetLastError());
  }
  return R3D_OK;
}

// The same for a batch in host memory: it goes up in slabs of whole frames through kWsIn, a slab's rasters first, then (unless
// h_rgb is NULL) its colour images at a 256-byte boundary; every slab is one integrate_device call.
int integrate_host(r3d_tsdf* v, const r3d_camera* cam, const void* h_depth, int depth_dtype, int n_frames, double depth_scale,
                   const double* h_pose, const uint8_t* h_rgb) {
  r3d_ctx* ctx = v->ctx;
  const size_t px = (size_t)cam->height * cam->width;
  const size_t depth_bytes = px * r3d_depth_size(depth_dtype), rgb_bytes = h_rgb ? px * 3 : 0, frame_bytes = depth_bytes + rgb_bytes;
  int slab = (int)(((size_t)256 << 20) / (frame_bytes ? frame_bytes : 1));
  if (slab < 1) slab = 1;
  if (slab > n_frames) slab = n_frames;
  r3d_carve in;
  const auto depth_h = in.take<char>((size_t)slab * depth_bytes);
  const auto rgb_h = in.take<uint8_t>((size_t)slab * rgb_bytes);
  int rc = r3d_scratch(ctx, kWsIn, in);
  if (rc) return rc;
  void* d_in = in.at(depth_h);
  uint8_t* d_rgb = h_rgb ? in.at(rgb_h) : nullptr;
  for (int lo = 0; lo < n_frames; lo += slab) {
    const int n = n_frames - lo < slab ? n_frames - lo : slab;
    if ((rc = r3d_memcpy_h2d(ctx, d_in, static_cast<const char*>(h_depth) + (size_t)lo * depth_bytes, (size_t)n * depth_bytes))) return rc;
    if (h_rgb && (rc = r3d_memcpy_h2d(ctx, d_rgb, h_rgb + (size_t)lo * rgb_bytes, (size_t)n * rgb_bytes))) return rc;
    if ((rc = integrate_device(v, cam, d_in, depth_dtype, n, depth_scale, h_pose + (size_t)lo * 12, d_rgb))) return rc;
    R3D_HIP(hipStreamSynchronize(ctx->stream));   // the next slab overwrites the scratch; the caller's memory is free at return
  }
  return R3D_OK;
}

// All four entry points.  rgb_call: the two that take colour images -- the volume must own the colour plane, and the depth-only
// two refuse one that does: its n would part from its w.
int integrate(r3d_tsdf* v, const r3d_camera* cam, const void* depth, int depth_dtype, int n_frames, double depth_scale, const double* h_pose,
              const uint8_t* rgb, bool rgb_call, bool host) {
  int rc = R3D_OK;
  if (rgb_call && (rc = r3d_tsdf_require_color(v))) return rc;
  R3D_REQUIRE(rgb_call || v == nullptr || v->d_col == nullptr, "the volume carries colour: integrate it with r3d_tsdf_integrate_rgb");
  if ((rc = r3d_tsdf_integrate_checks(v, cam, depth, depth_dtype, n_frames, depth_scale, h_pose)) || n_frames == 0) return rc;
  R3D_REQUIRE(!rgb_call || rgb != nullptr, "NULL colour pointer");
  if ((rc = r3d_ctx_enter(v->ctx))) return rc;
  return (host ? integrate_host : integrate_device)(v, cam, depth, depth_dtype, n_frames, depth_scale, h_pose, rgb);
}

}  // namespace

int r3d_tsdf_integrate(r3d_tsdf* v, const r3d_camera* cam, const void* d_depth, int depth_dtype, int n_frames, double depth_scale,
                       const double* h_pose_w2c) {
  return integrate(v, cam, d_depth, depth_dtype, n_frames, depth_scale, h_pose_w2c, nullptr, false, false);
}

int r3d_tsdf_integrate_host(r3d_tsdf* v, const r3d_camera* cam, const void* h_depth, int depth_dtype, int n_frames, double depth_scale,
                            const double* h_pose_w2c) {
  return integrate(v, cam, h_depth, depth_dtype, n_frames, depth_scale, h_pose_w2c, nullptr, false, true);
}

int r3d_tsdf_integrate_rgb(r3d_tsdf* v, const r3d_camera* cam, const void* d_depth, int depth_dtype, int n_frames, double depth_scale,
                           const double* h_pose_w2c, const uint8_t* d_rgb) {
  return integrate(v, cam, d_depth, depth_dtype, n_frames, depth_scale, h_pose_w2c, d_rgb, true, false);
}

int r3d_tsdf_integrate_rgb_host(r3d_tsdf* v, const r3d_camera* cam, const void* h_depth, int depth_dtype, int n_frames, double depth_scale,
                                const double* h_pose_w2c, const uint8_t* h_rgb) {
  return integrate(v, cam, h_depth, depth_dtype, n_frames, depth_scale, h_pose_w2c, h_rgb, true, true);
}

int r3d_tsdf_count_points(r3d_tsdf* v, float mw, const uint32_t** d_prefix, int* tiles_out, int64_t* n_points) {
  r3d_ctx* ctx = v->ctx;
  int rc = r3d_ctx_enter(ctx);
  if (rc) return rc;
  if (3 * v->n >= ((int64_t)1 << 32)) {   // the tile prefixes are 32-bit
    r3d_set_error("surface extraction takes volumes of fewer than 2^32 / 3 voxels");
    return R3D_ERR_UNSUPPORTED;
  }
  const int tiles = r3d_compact::tiles_of(v->n);
  r3d_compact::Counters cn(tiles, 1);
  void* ws = nullptr;
  if ((rc = r3d_scratch(ctx, kWsCounts, cn.bytes, &ws))) return rc;
  cn.place(ws);
  hipLaunchKernelGGL(tsdf_count_kernel, dim3(tiles), dim3(kThreads), 0, ctx->stream, (const float2*)v->d_vol, v->g, v->n, mw, cn.hist);
  uint32_t m = 0;
  if ((rc = r3d_compact::scan_totals(ctx, cn, &m))) return rc;
  *d_prefix = cn.hist;
  *tiles_out = tiles;
  *n_points = (int64_t)m;
  return R3D_OK;
}

int r3d_tsdf_extract_points(r3d_tsdf* v, double min_weight, float* d_xyz_out, float* d_normals_out, int64_t cap, int64_t* n_out) {
  float mw = 0.0f;
  int rc = r3d_tsdf_extract_checks(v, n_out != nullptr, "n_out", min_weight, &mw, "cap", {{d_xyz_out, cap, "d_xyz_out", "cap"}});
  if (rc) return rc;
  r3d_ctx* ctx = v->ctx;
  const uint32_t* hist = nullptr;
  int tiles = 0;
  int64_t m = 0;
  if ((rc = r3d_tsdf_count_points(v, mw, &hist, &tiles, &m))) return rc;
  hipStream_t st = ctx->stream;
  *n_out = m;
  const uint64_t rows = (uint64_t)(m < cap ? m : cap);
  if (rows == 0) return R3D_OK;
  r3d_wrote(ctx, d_xyz_out, (size_t)rows * 12);
  if (d_normals_out) r3d_wrote(ctx, d_normals_out, (size_t)rows * 12);
  hipLaunchKernelGGL(tsdf_emit_kernel, dim3(tiles), dim3(kThreads), 0, st, (const float2*)v->d_vol, v->g, v->n, mw, hist,
                     d_xyz_out, d_normals_out, rows);
  R3D_HIP(hipGetLastError());
  return R3D_OK;
}
