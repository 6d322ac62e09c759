// Depth bilateral filter for gfx950 (MI355X): the edge-preserving smoothing of a depth raster in front of its vertex and normal
// maps.  NOT IN THE REFERENCE: build-defined, specified in include/r3d.h ("Depth bilateral filter").
//
//   depth_bilateral_kernel   one lane per OUTPUT pixel; a 256-thread workgroup owns a 32 x 8 tile (a wave: two rows of 128
//                            contiguous bytes) and stages the tile plus its `radius` halo -- at most 24 x 48 floats -- into LDS once,
//                            invalid and out-of-raster cells as 0.0f, so the tap loop tests `d > 0` and no bounds.  With in_stride 1
//                            the staging loads of a tile row are consecutive dwords, with in_stride 3 (the z column of a vertex map)
//                            12 bytes apart.  Both weight tables are copied into LDS next to the tile: a tap's spatial weight is one
//                            address for the whole wave (a broadcast read), its range weight a per-lane gather from 1 KB.  A tile
//                            row is read by one 32-lane half of the wave as 32 consecutive dwords: no bank conflict at any radius.
//                            No transcendental arithmetic, no atomics, no scratch; the tap loops run to a runtime radius.  A
//                            workgroup walks tiles grid-stride (one tile each for every raster of practical size), and an output is
//                            a function of its own window alone, so the result does not depend on the launch geometry.
#include <cmath>

#include "r3d_internal.h"

namespace {

constexpr int kThreads = 256;
constexpr int kTileW = 32, kTileH = 8;
constexpr int kMaxR = R3D_BILATERAL_MAX_RADIUS, kBins = R3D_BILATERAL_RANGE_BINS;
constexpr int kMaxSide = 2 * kMaxR + 1;
constexpr int kTableFloats = kBins + kMaxSide * kMaxSide;   // the device copy: range[256], then spatial[(2r+1)^2], in kWsBilateral
constexpr int kMaxBlocks = 1 << 20;
constexpr int kTrackTile = 1024;   // the raster-size limit of the tracking calls (r3d_track.hip: kTile)

__global__ __launch_bounds__(kThreads) void depth_bilateral_kernel(const float* __restrict__ in, int in_stride, int height, int width,
                                                                   int radius, const float* __restrict__ tables, float cut,
                                                                   float inv_step, int tiles_x, int n_tiles, float* __restrict__ out) {
  __shared__ float s_tile[(kTileH + 2 * kMaxR) * (kTileW + 2 * kMaxR)];
  __shared__ float s_range[kBins];
  __shared__ float s_spatial[kMaxSide * kMaxSide];
  const int tid = (int)threadIdx.x, tx = tid & (kTileW - 1), ty = tid >> 5;
  const int side = 2 * radius + 1, pitch = kTileW + 2 * radius, cells = (kTileH + 2 * radius) * pitch;
  s_range[tid] = tables[tid];   // kBins == kThreads
  for (int i = tid; i < side * side; i += kThreads) s_spatial[i] = tables[kBins + i];
  for (int tile = (int)blockIdx.x; tile < n_tiles; tile += (int)gridDim.x) {
    const int tile_y = tile / tiles_x, tile_x = tile - tile_y * tiles_x;
    const int u0 = tile_x * kTileW, v0 = tile_y * kTileH;   // tile_y * 8 < height + 8, tile_x * 32 < width + 32
    for (int i = tid; i < cells; i += kThreads) {
      const int ry = i / pitch, rx = i - ry * pitch;
      const int v = v0 - radius + ry, u = u0 - radius + rx;
      float d = 0.0f;
      if (v >= 0 && v < height && u >= 0 && u < width) {
        d = in[((int64_t)v * width + u) * in_stride];
        if (!(isfinite(d) && d > 0.0f)) d = 0.0f;
      }
      s_tile[i] = d;
    }
    __syncthreads();
    const int u = u0 + tx, v = v0 + ty;
    if (u < width && v < height) {
      const float dc = s_tile[(ty + radius) * pitch + tx + radius];
      float result = 0.0f;
      if (dc > 0.0f) {
        float num = 0.0f, den = 0.0f;
        const float* row = s_tile + ty * pitch + tx;   // the window's top-left tap
        const float* sp = s_spatial;
        for (int dy = 0; dy < side; ++dy, row += pitch, sp += side) {
#pragma unroll 1
          for (int dx = 0; dx < side; ++dx) {
            const float d = row[dx];
            const float a = fabsf(d - dc);
            if (d > 0.0f && a <= cut) {
              const int k = min(kBins - 1, (int)(a * inv_step));
              const float w = sp[dx] * s_range[k];
              num = num + w * d;
              den = den + w;
            }
          }
        }
        result = __fdiv_rn(num, den);   // the centre tap entered with w == 1: den >= 1
      }
      out[(int64_t)v * width + u] = result;
    }
    __syncthreads();   // the next tile's staging overwrites s_tile
  }
}

// Are (radius, sigma_s, sigma_r) valid at all?  Every call asks, whatever the context has cached.  On success *cut and *inv_step
// hold the two scalars; nothing is written otherwise.
int bilateral_check(int radius, double sigma_s, double sigma_r, float* cut, float* inv_step) {
  R3D_REQUIRE(radius >= 0 && radius <= kMaxR, "radius must be in [0, %d], got %d", kMaxR, radius);
  R3D_REQUIRE(std::isfinite(sigma_s) && sigma_s > 0.0, "sigma_s must be finite and > 0");
  R3D_REQUIRE(std::isfinite(sigma_r) && sigma_r > 0.0, "sigma_r must be finite and > 0");
  const float c = (float)(3.0 * sigma_r), s = (float)((double)kBins / (3.0 * sigma_r));
  R3D_REQUIRE(std::isfinite(c) && c > 0.0f && std::isfinite(s) && s > 0.0f,
              "sigma_r = %g leaves the f32 range: cut = %g, inv_step = %g", sigma_r, (double)c, (double)s);
  *cut = c;
  *inv_step = s;
  return R3D_OK;
}

// The tables of VALID (radius, sigma_s, sigma_r) as the header specifies them: the one body behind r3d_bilateral_weights and the
// device call.
void bilateral_tables(int radius, double sigma_s, float* spatial, float* range) {
  const int side = 2 * radius + 1;
  for (int dy = -radius; dy <= radius; ++dy)
    for (int dx = -radius; dx <= radius; ++dx)
      spatial[(dy + radius) * side + (dx + radius)] = (float)std::exp(-(double)(dx * dx + dy * dy) / (2.0 * sigma_s * sigma_s));
  for (int k = 0; k < kBins; ++k) {
    const double t = 3.0 * (double)k / (double)kBins;
    range[k] = (float)std::exp(-0.5 * t * t);
  }
}

}  // namespace

extern "C" {

int r3d_bilateral_weights(int radius, double sigma_s, double sigma_r, float* h_spatial, float* h_range, float* h_cut,
                          float* h_inv_step) {
  R3D_REQUIRE(h_spatial != nullptr && h_range != nullptr && h_cut != nullptr && h_inv_step != nullptr, "NULL output pointer");
  float cut = 0.0f, inv_step = 0.0f;
  int rc = bilateral_check(radius, sigma_s, sigma_r, &cut, &inv_step);
  if (rc) return rc;
  bilateral_tables(radius, sigma_s, h_spatial, h_range);
  *h_cut = cut;
  *h_inv_step = inv_step;
  return R3D_OK;
}

int r3d_depth_bilateral(r3d_ctx* ctx, const float* d_in, int in_stride, int height, int width, int radius, double sigma_s,
                        double sigma_r, float* d_out) {
  R3D_REQUIRE(ctx != nullptr, "ctx is NULL");
  R3D_REQUIRE(d_in != nullptr && d_out != nullptr, "NULL raster pointer");
  R3D_REQUIRE(in_stride == 1 || in_stride == 3, "in_stride must be 1 (a depth raster) or 3 (the z column of a vertex map), got %d",
              in_stride);
  R3D_REQUIRE(height >= 1 && width >= 1, "a %d x %d raster is empty", height, width);
  R3D_REQUIRE((int64_t)width * height < ((int64_t)1 << 31) - kTrackTile, "raster of %d x %d pixels is too large for tracking", height,
              width);
  float cut = 0.0f, inv_step = 0.0f;
  int rc = bilateral_check(radius, sigma_s, sigma_r, &cut, &inv_step);   // always: the cache below is never asked about invalid arguments
  if (rc) return rc;
  const size_t n = (size_t)height * width;
  const size_t in_bytes = ((n - 1) * (size_t)in_stride + 1) * sizeof(float), out_bytes = n * sizeof(float);
  R3D_REQUIRE(!r3d_ranges_overlap(d_in, in_bytes, d_out, out_bytes), "the output overlaps the input");
  // a valid radius is >= 0, so the empty key (bilateral_radius == -1) matches no call
  const bool cached = ctx->bilateral_radius == radius && ctx->bilateral_sigma_s == sigma_s && ctx->bilateral_sigma_r == sigma_r;
  float h_tables[kTableFloats];
  if (!cached) bilateral_tables(radius, sigma_s, h_tables + kBins, h_tables);
  rc = r3d_ctx_enter(ctx);
  if (rc) return rc;
  void* d_tables = nullptr;
  rc = r3d_scratch(ctx, kWsBilateral, kTableFloats * sizeof(float), &d_tables);
  if (rc) return rc;
  if (!cached) {
    // stream-ordered behind every earlier launch that reads the old tables; the key is set only once the copy is enqueued
    ctx->bilateral_radius = -1;
    const int side = 2 * radius + 1;
    R3D_HIP(hipMemcpyAsync(d_tables, h_tables, (size_t)(kBins + side * side) * sizeof(float), hipMemcpyHostToDevice, ctx->stream));
    ctx->bilateral_radius = radius, ctx->bilateral_sigma_s = sigma_s, ctx->bilateral_sigma_r = sigma_r;
  }
  r3d_wrote(ctx, d_out, out_bytes);
  const int tiles_x = (width + kTileW - 1) / kTileW;
  const int64_t n_tiles = (int64_t)tiles_x * ((height + kTileH - 1) / kTileH);   // < 2^31 / 8 + 2^31 / 32 + 1
  const int blocks = (int)(n_tiles < kMaxBlocks ? n_tiles : kMaxBlocks);
  hipLaunchKernelGGL(depth_bilateral_kernel, dim3(blocks), dim3(kThreads), 0, ctx->stream, d_in, in_stride, height, width, radius,
                     (const float*)d_tables, cut, inv_step, tiles_x, (int)n_tiles, d_out);
  R3D_HIP(hipGetLastError());
  return R3D_OK;
}

}  // extern "C"
