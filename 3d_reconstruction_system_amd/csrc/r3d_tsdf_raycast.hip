// Ray casting of the TSDF volume for gfx950 (MI355X): the depth, vertex and normal map the volume predicts for a camera pose.
// Semantics: include/r3d.h ("TSDF ray casting"); every output bit is a chain of IEEE f32 operations in the order written there
// (the library builds with -ffp-contract=off and without any flush-to-zero or fast-math flag: f32 denormals are kept; hipcc's f32
// division and sqrt are correctly rounded by default).
//
//   tsdf_raycast_kernel   one lane = one pixel = one ray.  A wave covers an 8 x 8 pixel tile (lane = 8 row + column), a workgroup
//                         of four waves 16 x 16: neighbouring rays walk neighbouring cells, so the eight 8-byte gathers of a
//                         sample fall into few cache lines across the wave, and a tile row still stores 32 contiguous bytes of
//                         depth.  Tiles are linear on grid.x (a raster may have more than 65535 tile rows), views on grid.z.  The
//                         view's pose (R and the camera centre, 12 floats) is wave-uniform and comes from the volume's pose ring
//                         through scalar loads.  A lane leaves the march at its hit or when t_k > tmax; the loop counter is an
//                         integer with a fixed bound, so a NaN ends a ray instead of spinning it.  The volume is only read.
//                         No LDS, no atomics; every output word is written once, with vector stores.
//                         <false> is that kernel and what r3d_tsdf_raycast launches: the flag removes every colour statement, and
//                         its instructions are the ones it had before the flag existed (the body stays in the kernel: moved into
//                         an inlined function it allocates its scalar registers differently).  <true>, for r3d_tsdf_raycast_rgb
//                         ("TSDF ray-cast colour"), is the same ray through the same statements, so the three geometry maps are
//                         the same bits.  At the hit it also gathers the cell's eight colour records -- eight 16-byte loads, all
//                         issued before the first is used, once per ray and not per march step --, interpolates the three channel
//                         means like the tsdf and stores three bytes (a tile row of 8 pixels is 24 contiguous bytes).
#include "r3d_internal.h"
#include "r3d_tsdf_dev.h"

#include <cmath>

using namespace r3d_tsdf_dev;

namespace {

constexpr int kThreads = 256;
constexpr int kTile = 16;           // pixels a side of a workgroup's tile: 2 x 2 waves of 8 x 8
constexpr int kChunk = R3D_TSDF_CHUNK;   // views per launch = rows of one slot of the pose ring
constexpr int kMaxSteps = 65536;    // the march's last k

struct RayCam {
  float fx, fy, cx, cy;
  uint32_t width, height;
  uint32_t frame_px;   // height * width
  uint32_t tiles_x;
};

struct RayMarch {
  float mw, s, t_near, t_far;
};

// The cell around p and the fractions inside it; false unless the cell exists and its eight voxels are valid.  cell: the linear
// index of its corner 0.
__device__ __forceinline__ bool sample_cell(const float2* __restrict__ vol, const TsdfGrid& g, float ivs, float mw, const float (&p)[3],
                                            float (&T)[8], float (&f)[3], int64_t& cell) {
  const float gx = (p[0] - g.ox) * ivs - 0.5f, gy = (p[1] - g.oy) * ivs - 0.5f, gz = (p[2] - g.oz) * ivs - 0.5f;
  const float ix = floorf(gx), iy = floorf(gy), iz = floorf(gz);
  if (!(ix >= 0.0f && ix <= (float)(g.nx - 2) && iy >= 0.0f && iy <= (float)(g.ny - 2) && iz >= 0.0f && iz <= (float)(g.nz - 2)))
    return false;   // NaN fails every comparison
  const int x = (int)ix, y = (int)iy, z = (int)iz;
  if (x > g.nx - 2 || y > g.ny - 2 || z > g.nz - 2) return false;   // (float)(n - 2) rounded up: n > 2^24 + 2 only
  f[0] = gx - ix, f[1] = gy - iy, f[2] = gz - iz;
  float2 q[8];
  cell = ((int64_t)z * g.ny + y) * g.nx + x;
  load_cell(vol, g, cell, q);
  bool ok = true;
#pragma unroll
  for (int k = 0; k < 8; ++k) {
    ok = ok && (q[k].y >= mw);
    T[k] = q[k].x;
  }
  return ok;
}

// G_a of the cell: the differences along axis a, interpolated over the other two axes in ascending order.  k0 / sa: corner of
// (a = 0, jb = 0, jc = 0) and the corner step of a; sb, sc: the corner steps of b and c.
__device__ __forceinline__ float cell_gradient(const float (&T)[8], int sa, int sb, int sc, float fb, float fc) {
  const float d00 = T[sa] - T[0], d10 = T[sa + sb] - T[sb];             // D[jb][jc]
  const float d01 = T[sa + sc] - T[sc], d11 = T[sa + sb + sc] - T[sb + sc];
  const float e0 = d00 + fb * (d10 - d00), e1 = d01 + fb * (d11 - d01);
  return e0 + fc * (e1 - e0);
}

// The colour of a hit ("TSDF ray-cast colour") from the colour records c[k] of the cell's corners: per channel the eight means
// (0 where n == 0), interpolated like the tsdf, rounded half up and clamped to a byte
__device__ __forceinline__ void cell_color(const uint4 (&c)[8], const float (&f)[3], uint8_t (&q)[3]) {
  float M[3][8];
#pragma unroll
  for (int k = 0; k < 8; ++k) {
    const float n = (float)c[k].w;
    M[0][k] = c[k].w ? (float)c[k].x / n : 0.0f;
    M[1][k] = c[k].w ? (float)c[k].y / n : 0.0f;
    M[2][k] = c[k].w ? (float)c[k].z / n : 0.0f;
  }
#pragma unroll
  for (int a = 0; a < 3; ++a) q[a] = (uint8_t)color_byte(trilinear(M[a], f));
}

// grid: (tiles_x * tiles_y, 1, views of this launch); 256 threads = 2 x 2 waves of 8 x 8 pixels.  kColor: also the colour image,
// from the colour plane col into rgb_out (both unused, and NULL, otherwise)
template <bool kColor>
__global__ __launch_bounds__(kThreads) void tsdf_raycast_kernel(const float2* __restrict__ vol, const uint4* __restrict__ col, TsdfGrid g,
                                                                RayCam cam, const TsdfPoseRow* __restrict__ table, RayMarch m,
                                                                float* __restrict__ depth_out, float* __restrict__ vertex_out,
                                                                float* __restrict__ normal_out, uint8_t* __restrict__ rgb_out) {
  const uint32_t tile_y = blockIdx.x / cam.tiles_x, tile_x = blockIdx.x - tile_y * cam.tiles_x;
  const uint32_t wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const uint32_t ui = tile_x * kTile + (wave & 1) * 8 + (lane & 7);
  const uint32_t vi = tile_y * kTile + (wave >> 1) * 8 + (lane >> 3);
  if (ui >= cam.width || vi >= cam.height) return;
  const TsdfPoseRow P = table[blockIdx.z];   // wave-uniform: scalar loads; P.t is the camera centre C
  const size_t px = (size_t)blockIdx.z * cam.frame_px + (vi * cam.width + ui);

  const float x = ((float)ui - cam.cx) / cam.fx, y = ((float)vi - cam.cy) / cam.fy;
  const float len = sqrtf((x * x + y * y) + 1.0f);
  const float n[3] = {x / len, y / len, 1.0f / len};
  float dw[3];
#pragma unroll
  for (int k = 0; k < 3; ++k) dw[k] = (P.r[k] * n[0] + P.r[3 + k] * n[1]) + P.r[6 + k] * n[2];

  // sample domain: the box of voxel centres, by slabs
  const float o[3] = {g.ox, g.oy, g.oz};
  const int dim[3] = {g.nx, g.ny, g.nz};
  float tmin = m.t_near, tmax = m.t_far;
  bool alive = g.nx >= 2 && g.ny >= 2 && g.nz >= 2;   // a volume without cells: every pixel is a miss
#pragma unroll
  for (int a = 0; a < 3; ++a) {
    const float lo = o[a] + 0.5f * g.vs, hi = o[a] + ((float)(dim[a] - 1) + 0.5f) * g.vs;
    if (dw[a] == 0.0f) {
      if (!(lo <= P.t[a] && P.t[a] <= hi)) alive = false;
    } else {
      const float q1 = (lo - P.t[a]) / dw[a], q2 = (hi - P.t[a]) / dw[a];
      tmin = fmaxf(tmin, fminf(q1, q2));
      tmax = fminf(tmax, fmaxf(q1, q2));
    }
  }
  if (!(tmin <= tmax)) alive = false;

  const float ivs = 1.0f / g.vs;
  float T[8], f[3], p[3];
  int64_t cell = 0;
  bool hit = false;
  float tstar = 0.0f;
  if (alive) {
    bool prev_ok = false;
    float A = 0.0f;
    for (int k = 0; k <= kMaxSteps; ++k) {
      const float t = tmin + (float)k * m.s;
      if (!(t <= tmax)) break;
#pragma unroll
      for (int a = 0; a < 3; ++a) p[a] = P.t[a] + t * dw[a];
      const bool ok = sample_cell(vol, g, ivs, m.mw, p, T, f, cell);
      const float B = ok ? trilinear(T, f) : 0.0f;
      if (prev_ok && ok && A > 0.0f && B <= 0.0f) {   // (prev_ok: k >= 1)
        const float r = A / (A - B);
        tstar = (tmin + (float)(k - 1) * m.s) + r * m.s;
        hit = true;
        break;
      }
      prev_ok = ok;
      A = B;
    }
  }

  float G[3] = {0.0f, 0.0f, 0.0f}, L = 0.0f;
  uint4 c[8];   // (kColor) the colour records of the hit cell's corners
  if (hit) {
#pragma unroll
    for (int a = 0; a < 3; ++a) p[a] = P.t[a] + tstar * dw[a];
    hit = sample_cell(vol, g, ivs, m.mw, p, T, f, cell);
    if (hit) {
      if constexpr (kColor) load_cell(col, g, cell, c);   // all eight in flight while the gradient is computed
      G[0] = cell_gradient(T, 1, 2, 4, f[1], f[2]);
      G[1] = cell_gradient(T, 2, 1, 4, f[0], f[2]);
      G[2] = cell_gradient(T, 4, 1, 2, f[0], f[1]);
      L = sqrtf((G[0] * G[0] + G[1] * G[1]) + G[2] * G[2]);
      hit = L > 0.0f;
    }
  }

  const float none = __uint_as_float(0x7FC00000u);   // a missing row; a point at the world origin is a legitimate point
  if (depth_out) depth_out[px] = hit ? tstar * n[2] : 0.0f;
  if (vertex_out) {
#pragma unroll
    for (int a = 0; a < 3; ++a) vertex_out[3 * px + a] = hit ? P.t[a] + tstar * dw[a] : none;
  }
  if (normal_out) {
#pragma unroll
    for (int a = 0; a < 3; ++a) normal_out[3 * px + a] = hit ? G[a] / L : none;
  }
  if constexpr (kColor) {
    uint8_t q[3] = {0, 0, 0};   // a miss: depth 0 marks it, black is a legitimate colour
    if (hit) cell_color(c, f, q);
#pragma unroll
    for (int a = 0; a < 3; ++a) rgb_out[3 * px + a] = q[a];
  }
}

// Both entry points.  rgb_call: r3d_tsdf_raycast_rgb -- the volume must own the colour plane, whatever the pointers; with
// d_rgb_out == NULL it launches the depth-only kernel, like r3d_tsdf_raycast.
int raycast(r3d_tsdf* v, const r3d_camera* cam, int n_views, const double* h_pose_w2c, double min_weight, double step, double t_near,
            double t_far, float* d_depth_out, float* d_vertex_out, float* d_normal_out, uint8_t* d_rgb_out, bool rgb_call) {
  R3D_REQUIRE(v != nullptr, "TSDF volume is NULL");
  R3D_REQUIRE(cam != nullptr, "camera is NULL");
  int rc = R3D_OK;
  if (rgb_call && (rc = r3d_tsdf_require_color(v))) return rc;
  r3d_ctx* ctx = v->ctx;
  const TsdfGrid& g = v->g;
  const float2* vol = v->d_vol;
  const uint4* col = rgb_call ? v->d_col : nullptr;
  const int64_t n = v->n;
  R3D_REQUIRE(cam->ctx == ctx, "the camera belongs to another context than the volume");
  R3D_REQUIRE(n_views >= 0, "n_views must be >= 0");
  RayMarch m;
  m.mw = (float)min_weight, m.s = (float)step, m.t_near = (float)t_near, m.t_far = (float)t_far;
  R3D_REQUIRE(m.mw > 0.0f && std::isfinite(m.mw), "min_weight must be positive and finite in f32");
  R3D_REQUIRE(m.s > 0.0f && std::isfinite(m.s), "step must be positive and finite in f32");
  R3D_REQUIRE(std::isfinite(m.t_near) && m.t_near >= 0.0f, "t_near must be finite and >= 0 in f32");
  R3D_REQUIRE(m.t_far > m.t_near, "t_far must be > t_near (+inf is allowed)");
  {   // the longest march crosses the box of voxel centres along its diagonal
    const double dx = g.nx - 1, dy = g.ny - 1, dz = g.nz - 1;
    R3D_REQUIRE((double)g.vs * std::sqrt((dx * dx + dy * dy) + dz * dz) / (double)m.s < (double)kMaxSteps,
                "step is too small for this volume: a ray could take %d samples or more", kMaxSteps);
  }
  if (n_views == 0) return R3D_OK;
  R3D_REQUIRE(h_pose_w2c != nullptr, "NULL pose pointer");
  R3D_REQUIRE(cam->width <= (1 << 24) && cam->height <= (1 << 24) && (int64_t)cam->width * cam->height < ((int64_t)1 << 31),
              "raster of %d x %d pixels is too large for the TSDF ray casting", cam->height, cam->width);
  RayCam c;
  c.fx = (float)cam->fx, c.fy = (float)cam->fy, c.cx = (float)cam->cx, c.cy = (float)cam->cy;
  c.width = (uint32_t)cam->width, c.height = (uint32_t)cam->height;
  c.frame_px = c.height * c.width;
  c.tiles_x = (c.width + kTile - 1) / kTile;
  const uint32_t tiles = c.tiles_x * ((c.height + kTile - 1) / kTile);   // <= 2^31 / 256 + two edges
  const size_t map = (size_t)n_views * c.frame_px * sizeof(float);
  const struct {
    const void* p;
    size_t bytes;
  } out[4] = {{d_depth_out, map}, {d_vertex_out, 3 * map}, {d_normal_out, 3 * map}, {d_rgb_out, (size_t)n_views * c.frame_px * 3}};
  for (int a = 0; a < 4; ++a) {
    R3D_REQUIRE(!r3d_ranges_overlap(out[a].p, out[a].bytes, vol, (size_t)n * sizeof(float2)), "an output overlaps the volume");
    // the colour plane is read only when there is a colour image to write
    R3D_REQUIRE(!d_rgb_out || !r3d_ranges_overlap(out[a].p, out[a].bytes, col, (size_t)n * sizeof(uint4)),
                "an output overlaps the colour plane");
    for (int b = a + 1; b < 4; ++b) R3D_REQUIRE(!r3d_ranges_overlap(out[a].p, out[a].bytes, out[b].p, out[b].bytes), "outputs overlap each other");
  }
  if ((!d_depth_out && !d_vertex_out && !d_normal_out && !d_rgb_out) || c.frame_px == 0) return R3D_OK;
  if ((rc = r3d_ctx_enter(ctx))) return rc;
  for (int a = 0; a < 4; ++a)
    if (out[a].p) r3d_wrote(ctx, out[a].p, out[a].bytes);
  for (int lo = 0; lo < n_views; lo += kChunk) {
    const int nv = n_views - lo < kChunk ? n_views - lo : kChunk;
    const TsdfPoseRow* d_rows = nullptr;
    rc = r3d_tsdf_send_rows(v, nv, &d_rows, [&](TsdfPoseRow* h) {
      for (int f = 0; f < nv; ++f) {
        const double* R = h_pose_w2c + (size_t)(lo + f) * 12;
        const double* t = R + 9;
        for (int k = 0; k < 9; ++k) h[f].r[k] = (float)R[k];
        for (int k = 0; k < 3; ++k) h[f].t[k] = (float)(-((R[k] * t[0] + R[3 + k] * t[1]) + R[6 + k] * t[2]));   // C = -R^T t, in double
        for (int k = 0; k < 4; ++k) h[f].pad[k] = 0.0f;
      }
    });
    if (rc) return rc;
    const size_t at = (size_t)lo * c.frame_px;
    float* depth = d_depth_out ? d_depth_out + at : nullptr;
    float* vertex = d_vertex_out ? d_vertex_out + 3 * at : nullptr;
    float* normal = d_normal_out ? d_normal_out + 3 * at : nullptr;
    if (d_rgb_out)
      hipLaunchKernelGGL(tsdf_raycast_kernel<true>, dim3(tiles, 1, (unsigned)nv), dim3(kThreads), 0, ctx->stream, vol, col, g, c, d_rows, m,
                         depth, vertex, normal, d_rgb_out + 3 * at);
    else
      hipLaunchKernelGGL(tsdf_raycast_kernel<false>, dim3(tiles, 1, (unsigned)nv), dim3(kThreads), 0, ctx->stream, vol, (const uint4*)nullptr, g,
                         c, d_rows, m, depth, vertex, normal, (uint8_t*)nullptr);
    R3D_HIP(hipGetLastError());
  }
  return R3D_OK;
}

}  // namespace

int r3d_tsdf_raycast(r3d_tsdf* v, const r3d_camera* cam, int n_views, const double* h_pose_w2c, double min_weight, double step,
                     double t_near, double t_far, float* d_depth_out, float* d_vertex_out, float* d_normal_out) {
  return raycast(v, cam, n_views, h_pose_w2c, min_weight, step, t_near, t_far, d_depth_out, d_vertex_out, d_normal_out, nullptr, false);
}

int r3d_tsdf_raycast_rgb(r3d_tsdf* v, const r3d_camera* cam, int n_views, const double* h_pose_w2c, double min_weight, double step,
                         double t_near, double t_far, float* d_depth_out, float* d_vertex_out, float* d_normal_out, uint8_t* d_rgb_out) {
  return raycast(v, cam, n_views, h_pose_w2c, min_weight, step, t_near, t_far, d_depth_out, d_vertex_out, d_normal_out, d_rgb_out, true);
}
