// What the TSDF volume's sources share (r3d_tsdf.hip, r3d_tsdf_color.hip, r3d_tsdf_mesh.hip, r3d_tsdf_raycast.hip, r3d_track.hip),
// and the projection rule r3d_consistency.hip shares with them.
// Internal to libr3d_hip.so.  Semantics: include/r3d.h ("TSDF volume", "TSDF colour").
//   device   voxel indexing, the crossing predicate and the surface point of a crossing (emit_points: the mesh's vertices ARE the
//            points, bit for bit), the colour of a surface point (emit_colors), the cell loads of ray casting, and the one
//            statement of the per-frame integration rule (integrate_frame) over the one of the projection (project_to_pixel);
//   host     struct r3d_tsdf itself, the one step through its pose ring (r3d_tsdf_send_rows), and the argument checks that more
//            than one entry point makes.
#pragma once

#include "r3d_internal.h"

#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>
#include <initializer_list>

namespace r3d_tsdf_dev {

struct TsdfGrid {
  int nx, ny, nz;
  float ox, oy, oz, vs, tr;
};

// One row of the volume's pose ring (r3d_tsdf below), f32, 64 bytes: the world -> camera rotation, row-major, and a vector t --
// the pose's translation for integration (p_cam = R p_w + t), the camera centre in the world for ray casting.
struct TsdfPoseRow {
  float r[9];
  float t[3];
  float pad[4];
};
static_assert(sizeof(TsdfPoseRow) == 64, "one pose row is 64 bytes");

__device__ __forceinline__ float centre(float o, int idx, float vs) { return o + ((float)idx + 0.5f) * vs; }

struct TsdfCam {
  float fx, fy, cx, cy, wf, hf, scale;
  int width;
  uint32_t frame_px;   // height * width
};

// the intrinsics, the raster's shape and the depth scale as the kernels take them: each rounded once to f32
inline TsdfCam tsdf_cam_of(const r3d_camera* cam, double depth_scale) {
  TsdfCam c;
  c.fx = (float)cam->fx, c.fy = (float)cam->fy, c.cx = (float)cam->cx, c.cy = (float)cam->cy;
  c.wf = (float)cam->width, c.hf = (float)cam->height, c.scale = (float)depth_scale;
  c.width = cam->width;
  c.frame_px = (uint32_t)cam->height * (uint32_t)cam->width;
  return c;
}

// The projection rule, stated once (integration, r3d_consistency.hip): the point (x, y, z) of the frame fr maps from goes to
// p = R (x, y, z) + t; false unless p.z > 0 and p falls into a pixel of the raster (nearest pixel); then pz = p.z and at =
// vi * width + ui, that pixel.
__device__ __forceinline__ bool project_to_pixel(const TsdfPoseRow& fr, const TsdfCam& cam, float x, float y, float z, float& pz, uint32_t& at) {
  const float px = ((fr.r[0] * x + fr.r[1] * y) + fr.r[2] * z) + fr.t[0];
  const float py = ((fr.r[3] * x + fr.r[4] * y) + fr.r[5] * z) + fr.t[1];
  pz = ((fr.r[6] * x + fr.r[7] * y) + fr.r[8] * z) + fr.t[2];
  if (!(pz > 0.0f)) return false;
  const float u = cam.fx * (px / pz) + cam.cx;
  const float v = cam.fy * (py / pz) + cam.cy;
  const float ui = floorf(u + 0.5f), vi = floorf(v + 0.5f);
  if (!(ui >= 0.0f && ui < cam.wf && vi >= 0.0f && vi < cam.hf)) return false;   // NaN fails every comparison
  at = (uint32_t)(int)vi * (uint32_t)cam.width + (uint32_t)(int)ui;
  return true;
}

// One frame into one voxel; returns whether the frame touched it, and then pixel = vi * width + ui, the pixel it read (the
// integration kernel's colour variant gathers the same pixel of the colour image; the depth-only one drops it).
template <typename D>
__device__ __forceinline__ bool integrate_frame(const TsdfPoseRow& fr, const TsdfCam& cam, const D* __restrict__ depth, float tr, float cx_,
                                                float cy_, float cz_, float& tsdf, float& w, uint32_t& pixel) {
  float pz;
  uint32_t at;
  if (!project_to_pixel(fr, cam, cx_, cy_, cz_, pz, at)) return false;
  const float d = (float)depth[at] * cam.scale;
  if (!(d > 0.0f && d < INFINITY)) return false;
  const float sdf = d - pz;
  if (sdf < -tr) return false;
  const float tn = fminf(1.0f, sdf / tr);
  const float w1 = w + 1.0f;
  tsdf = (tsdf * w + tn) / w1;
  w = w1;
  pixel = at;
  return true;
}

struct Vox {
  int x, y, z;
};

__device__ __forceinline__ Vox vox_of(int64_t i, const TsdfGrid& g) {
  const uint32_t row = (uint32_t)i / (uint32_t)g.nx;   // i < 2^31
  Vox v;
  v.x = (int)((uint32_t)i - row * (uint32_t)g.nx);
  v.z = (int)(row / (uint32_t)g.ny);
  v.y = (int)(row - (uint32_t)v.z * (uint32_t)g.ny);
  return v;
}

__device__ __forceinline__ int64_t step_of(int a, const TsdfGrid& g) { return a == 0 ? 1 : a == 1 ? (int64_t)g.nx : (int64_t)g.nx * g.ny; }
__device__ __forceinline__ int coord_of(const Vox& v, int a) { return a == 0 ? v.x : a == 1 ? v.y : v.z; }
__device__ __forceinline__ int dim_of(const TsdfGrid& g, int a) { return a == 0 ? g.nx : a == 1 ? g.ny : g.nz; }

// bit a: the edge from voxel i towards +axis a carries a surface point
__device__ __forceinline__ uint32_t crossings(const float2* __restrict__ vol, const TsdfGrid& g, int64_t i, float mw) {
  const float2 A = vol[i];
  if (!(A.y >= mw)) return 0;
  const Vox v = vox_of(i, g);
  uint32_t m = 0;
#pragma unroll
  for (int a = 0; a < 3; ++a) {
    if (coord_of(v, a) + 1 >= dim_of(g, a)) continue;
    const float2 B = vol[i + step_of(a, g)];
    if (B.y >= mw && ((A.x < 0.0f) != (B.x < 0.0f))) m |= 1u << a;
  }
  return m;
}

// the neighbour's tsdf if it is inside the volume and valid, else the voxel's own
__device__ __forceinline__ float tsdf_or(const float2* __restrict__ vol, int64_t j, bool inside, float mw, float own) {
  if (!inside) return own;
  const float2 q = vol[j];
  return q.y >= mw ? q.x : own;
}

__device__ __forceinline__ void gradient(const float2* __restrict__ vol, const TsdfGrid& g, int64_t i, const Vox& v, float mw, float (&out)[3]) {
  const float own = vol[i].x;
#pragma unroll
  for (int b = 0; b < 3; ++b) {
    const int64_t s = step_of(b, g);
    const int c = coord_of(v, b);
    out[b] = tsdf_or(vol, i + s, c + 1 < dim_of(g, b), mw, own) - tsdf_or(vol, i - s, c >= 1, mw, own);
  }
}

// The surface points of the crossing bits in `mask` (3 bits per voxel from voxel `base` on, voxel-major: the order of the output)
// go to rows at, at + 1, ... while at < cap.
__device__ __forceinline__ void emit_points(const float2* __restrict__ vol, const TsdfGrid& g, int64_t base, float mw, uint64_t mask,
                                            uint64_t at, uint64_t cap, float* __restrict__ xyz_out, float* __restrict__ normals_out) {
  while (mask && at < cap) {
    const int bit = __ffsll((long long)mask) - 1;
    mask &= mask - 1;
    const int e = bit / 3, a = bit - 3 * e;
    const int64_t i = base + e, j = i + step_of(a, g);
    const Vox v = vox_of(i, g);
    Vox w = v;
    if (a == 0) ++w.x; else if (a == 1) ++w.y; else ++w.z;
    const float A = vol[i].x, B = vol[j].x;
    const float r = A / (A - B);
    float pos[3] = {centre(g.ox, v.x, g.vs), centre(g.oy, v.y, g.vs), centre(g.oz, v.z, g.vs)};
    const float moved = pos[a] + r * g.vs;
    if (a == 0) pos[0] = moved; else if (a == 1) pos[1] = moved; else pos[2] = moved;
    if (xyz_out) {
      xyz_out[3 * at + 0] = pos[0];
      xyz_out[3 * at + 1] = pos[1];
      xyz_out[3 * at + 2] = pos[2];
    }
    if (normals_out) {
      float gv[3], gn[3], m[3];
      gradient(vol, g, i, v, mw, gv);
      gradient(vol, g, j, w, mw, gn);
#pragma unroll
      for (int b = 0; b < 3; ++b) m[b] = gv[b] + r * (gn[b] - gv[b]);
      const float len = sqrtf((m[0] * m[0] + m[1] * m[1]) + m[2] * m[2]);
      const bool ok = len > 0.0f;
#pragma unroll
      for (int b = 0; b < 3; ++b) normals_out[3 * at + b] = ok ? m[b] / len : 0.0f;
    }
    ++at;
  }
}

// an interpolated channel mean as a byte: rounded half up and clamped
__device__ __forceinline__ uint32_t color_byte(float m) { return (uint32_t)fminf(fmaxf(floorf(m + 0.5f), 0.0f), 255.0f); }

// One channel of a surface point's colour ("TSDF colour"): the two voxels' mean colours, interpolated like the position, rounded
// half up and clamped to a byte.  n == 0 gives a mean of 0 (a valid voxel has n >= 1).
__device__ __forceinline__ uint32_t color_channel(uint32_t sum_v, uint32_t n_v, uint32_t sum_u, uint32_t n_u, float r) {
  const float mv = n_v ? (float)sum_v / (float)n_v : 0.0f;
  const float mu = n_u ? (float)sum_u / (float)n_u : 0.0f;
  return color_byte(mv + r * (mu - mv));
}

// emit_points' sibling: the colour words r | g << 8 | b << 16 of the same crossings, to the same rows under the same at < cap rule
__device__ __forceinline__ void emit_colors(const float2* __restrict__ vol, const uint4* __restrict__ col, const TsdfGrid& g, int64_t base,
                                            uint64_t mask, uint64_t at, uint64_t cap, uint32_t* __restrict__ rgba_out) {
  while (mask && at < cap) {
    const int bit = __ffsll((long long)mask) - 1;
    mask &= mask - 1;
    const int e = bit / 3, a = bit - 3 * e;
    const int64_t i = base + e, j = i + step_of(a, g);
    const float A = vol[i].x, B = vol[j].x;
    const float r = A / (A - B);
    const uint4 cv = col[i], cu = col[j];
    rgba_out[at] = color_channel(cv.x, cv.w, cu.x, cu.w, r) | color_channel(cv.y, cv.w, cu.y, cu.w, r) << 8 |
                   color_channel(cv.z, cv.w, cu.z, cu.w, r) << 16;
    ++at;
  }
}

// The eight voxels of the cell whose corner 0 is voxel i (which has a neighbour on every + side): q[k], k = dx + 2 dy + 4 dz, the
// mesh's corner numbering.  {tsdf, weight} of a voxel is one 8-byte load; the x pair of a row is 16 contiguous bytes.  With V =
// uint4 and the colour plane: the same corners' colour records, one 16-byte load each.
template <typename V>
__device__ __forceinline__ void load_cell(const V* __restrict__ vol, const TsdfGrid& g, int64_t i, V (&q)[8]) {
  const int64_t sy = g.nx, sz = (int64_t)g.nx * g.ny;
#pragma unroll
  for (int k = 0; k < 8; k += 2) {
    const V* row = vol + (i + (int64_t)((k >> 1) & 1) * sy + (int64_t)(k >> 2) * sz);
    q[k] = row[0];
    q[k + 1] = row[1];
  }
}

// S = the trilinear value of the cell's tsdf T[k] at fractions f = (f_x, f_y, f_z): x first, then y, then z
__device__ __forceinline__ float trilinear(const float (&T)[8], const float (&f)[3]) {
  const float c00 = T[0] + f[0] * (T[1] - T[0]), c10 = T[2] + f[0] * (T[3] - T[2]);   // c[jy][jz]
  const float c01 = T[4] + f[0] * (T[5] - T[4]), c11 = T[6] + f[0] * (T[7] - T[6]);
  const float b0 = c00 + f[1] * (c10 - c00), b1 = c01 + f[1] * (c11 - c01);
  return b0 + f[2] * (b1 - b0);
}

}  // namespace r3d_tsdf_dev

struct r3d_tsdf {
  static constexpr int kSlots = 4;   // slots of the pose ring: a call's chunks ride it without waiting for each other
  r3d_ctx* ctx = nullptr;
  int device = 0;   // for destroy, which must not dereference ctx
  r3d_tsdf_dev::TsdfGrid g = {};
  int64_t n = 0;    // voxels
  float2* d_vol = nullptr;
  uint4* d_col = nullptr;                         // the colour plane {sum_r, sum_g, sum_b, n} of a volume created with colour, else NULL
  r3d_tsdf_dev::TsdfPoseRow* d_table = nullptr;   // the pose ring: [kSlots][R3D_TSDF_CHUNK]
  r3d_tsdf_dev::TsdfPoseRow* h_table = nullptr;   // the same, pinned: what the uploads read
  hipEvent_t ev[kSlots] = {};                     // slot s of h_table has been read by its upload
  unsigned next_slot = 0;
  // r3d_tsdf_cloud.hip's grow-only device buffers (block list, one chunk's queries and matches, the host entry's upload): the NN
  // query in the middle of a cloud call takes the context's shared workspaces, so what lives across it belongs to the volume
  static constexpr int kCloudBufs = 3;
  void* cloud_buf[kCloudBufs] = {};
  size_t cloud_bytes[kCloudBufs] = {};
};

// One step through the volume's pose ring, for every launch that reads poses: takes the next slot, waits until the upload that
// read its pinned rows last is done (an event never recorded returns at once), has fill(rows) write n <= R3D_TSDF_CHUNK of them,
// sends them on the ctx stream and records the slot's event there.  *d_rows: the rows in HBM.
template <typename Fill>
int r3d_tsdf_send_rows(r3d_tsdf* v, int n, const r3d_tsdf_dev::TsdfPoseRow** d_rows, Fill fill) {
  const size_t s = v->next_slot++ % r3d_tsdf::kSlots;
  R3D_HIP(hipEventSynchronize(v->ev[s]));
  r3d_tsdf_dev::TsdfPoseRow *h = v->h_table + s * R3D_TSDF_CHUNK, *d = v->d_table + s * R3D_TSDF_CHUNK;
  fill(h);
  R3D_HIP(hipMemcpyAsync(d, h, sizeof(*h) * n, hipMemcpyHostToDevice, v->ctx->stream));
  R3D_HIP(hipEventRecord(v->ev[s], v->ctx->stream));
  *d_rows = d;
  return R3D_OK;
}

// R3D_ERR_INVALID unless the volume is there and was created with the colour plane
inline int r3d_tsdf_require_color(const r3d_tsdf* v) {
  R3D_REQUIRE(v != nullptr, "TSDF volume is NULL");
  R3D_REQUIRE(v->d_col != nullptr, "the volume was created without colour (r3d_tsdf_create_rgb makes one with)");
  return R3D_OK;
}

// What r3d_tsdf_extract_points, _colors and _mesh check first, in this order: the volume, the count pointers (have_counts; counts
// names them), min_weight (*mw: in f32), every output's cap (caps names them all), every output's pointer.
struct r3d_tsdf_out {
  const void* p;
  int64_t cap;
  const char *name, *cap_name;
};
inline int r3d_tsdf_extract_checks(const r3d_tsdf* v, bool have_counts, const char* counts, double min_weight, float* mw, const char* caps,
                                   std::initializer_list<r3d_tsdf_out> outs) {
  R3D_REQUIRE(v != nullptr, "TSDF volume is NULL");
  R3D_REQUIRE(have_counts, "%s is NULL", counts);
  *mw = (float)min_weight;
  R3D_REQUIRE(*mw > 0.0f, "min_weight must be > 0 in f32");
  for (const r3d_tsdf_out& o : outs) R3D_REQUIRE(o.cap >= 0, "%s must be >= 0", caps);
  for (const r3d_tsdf_out& o : outs) R3D_REQUIRE(o.cap == 0 || o.p != nullptr, "%s is NULL with %s > 0", o.name, o.cap_name);
  return R3D_OK;
}

// r3d_tsdf_cloud.hip: the launches r3d_tsdf_cloud_host.cpp drives (asynchronous on the ctx stream, arguments checked by then).  The
// band is made of blocks of 4 x 4 x 4 voxels, numbered (bz by + by) bx + bx with b* = ceil(n* / 4): _blocks is their number.  _mark:
// the bit of every block that the sdf_trunc box of one of the n points at d_tgt overlaps is set in d_bitmap (zeroed by the caller,
// ceil(blocks / 32) words).  _count / _list: the compaction step of r3d_compact_dev.h over those words -- hist holds the tiles'
// counts after _count, their exclusive prefixes for _list, which writes the marked blocks' numbers in ascending order.  _centres:
// the 64 voxel centres of each of n_blocks listed blocks as query points d_q [n_blocks * 64][3] (NaN where a block hangs over the
// volume).  _apply: the rule for the same voxels from their matches d_idx / d_d2; d_rgba != NULL: into d_col too; *d_touched
// grows by the number of voxels updated.
int64_t r3d_tsdf_cloud_blocks(const r3d_tsdf_dev::TsdfGrid& g);
void r3d_tsdf_cloud_mark_launch(r3d_ctx* ctx, const float* d_tgt, int64_t n, const r3d_tsdf_dev::TsdfGrid& g, uint32_t* d_bitmap);
void r3d_tsdf_cloud_count_launch(r3d_ctx* ctx, const uint32_t* d_bitmap, int64_t n_words, int tiles, uint32_t* hist);
void r3d_tsdf_cloud_list_launch(r3d_ctx* ctx, const uint32_t* d_bitmap, int64_t n_words, int tiles, const uint32_t* hist, uint32_t* d_list);
void r3d_tsdf_cloud_centres_launch(r3d_ctx* ctx, const uint32_t* d_list, uint32_t n_blocks, const r3d_tsdf_dev::TsdfGrid& g, float* d_q);
void r3d_tsdf_cloud_apply_launch(r3d_ctx* ctx, const uint32_t* d_list, uint32_t n_blocks, const r3d_tsdf_dev::TsdfGrid& g,
                                 const uint32_t* d_idx, const float* d_d2, const float* d_tgt, const float* d_normals, const uint32_t* d_rgba,
                                 uint32_t n_points, float2* d_vol, uint4* d_col, unsigned long long* d_touched);

// r3d_tsdf.hip: the argument checks r3d_tsdf_integrate makes (R3D_OK with n_frames == 0 too: the caller returns then);
int r3d_tsdf_integrate_checks(r3d_tsdf* vol, const r3d_camera* cam, const void* depth, int depth_dtype, int n_frames, double depth_scale,
                              const double* h_pose);
// and the first half of r3d_tsdf_extract_points: tsdf_count_kernel + the tile scan into kWsCounts, the count read back
// (synchronises).  *d_prefix: the tiles' exclusive prefixes, *tiles their number, *n_points the count.
int r3d_tsdf_count_points(r3d_tsdf* vol, float mw, const uint32_t** d_prefix, int* tiles, int64_t* n_points);
