// Intensity and gradient maps for gfx950 (MI355X): what the photometric term of frame-to-model tracking (r3d_track.hip:
// track_rgb_kernel) reads on both sides.  NOT IN THE REFERENCE: build-defined, specified in include/r3d.h ("TSDF colour tracking").
//
//   intensity_map_kernel  one lane per pixel: the f32 luma of its own three bytes and of its four neighbours' (recomputed from their
//                         bytes: no second pass), the validity value of the five (one dword each, in_stride 1 or 3 floats apart),
//                         central differences that stop at the raster's border, at an invalid pixel and at a depth edge.  Stores one
//                         dword (intensity) and / or one 16-byte row {I, gx, gy, 0} (so that a bilinear tap of the tracker is one
//                         16-byte load).  No LDS, no atomics, no scratch; every output is a function of its own 5-pixel cross, so
//                         the result does not depend on the launch geometry.
#include <cmath>

#include "r3d_internal.h"

namespace {

constexpr int kThreads = 256;
constexpr int kTrackTile = 1024;   // the raster-size limit of the tracking calls (r3d_track.hip: kTile)

__device__ __forceinline__ bool valid_depth(float d) { return isfinite(d) && d > 0.0f; }

// I = (0.299f R + 0.587f G) + 0.114f B of pixel i ([n][3] bytes)
__device__ __forceinline__ float luma(const uint8_t* __restrict__ rgb, int64_t i) {
  const float r = (float)rgb[3 * i], g = (float)rgb[3 * i + 1], b = (float)rgb[3 * i + 2];
  return (0.299f * r + 0.587f * g) + 0.114f * b;
}

// 0.5f (I(i + s) - I(i - s)), or NaN where either neighbour is invalid or across a depth jump; the caller has checked that both
// neighbours are inside the raster and that pixel i itself is valid with depth d
__device__ __forceinline__ float central(const uint8_t* __restrict__ rgb, const float* __restrict__ valid, int stride, int64_t i, int64_t s,
                                         float d, float max_jump) {
  const float dm = valid[(i - s) * stride], dp = valid[(i + s) * stride];
  if (!valid_depth(dm) || !valid_depth(dp) || fabsf(dm - d) > max_jump || fabsf(dp - d) > max_jump) return NAN;
  return 0.5f * (luma(rgb, i + s) - luma(rgb, i - s));
}

__global__ __launch_bounds__(kThreads) void intensity_map_kernel(const uint8_t* __restrict__ rgb, const float* __restrict__ valid, int stride,
                                                                 int height, int width, float max_jump, float* __restrict__ intensity_out,
                                                                 float4* __restrict__ packed_out) {
  const int i = (int)blockIdx.x * kThreads + (int)threadIdx.x;   // n_px < 2^31 - 1024
  if (i >= height * width) return;
  const int v = i / width, u = i - v * width;
  const float d = valid[(int64_t)i * stride];
  float I = NAN, gx = NAN, gy = NAN;
  if (valid_depth(d)) {
    I = luma(rgb, i);
    if (u > 0 && u < width - 1) gx = central(rgb, valid, stride, i, 1, d, max_jump);
    if (v > 0 && v < height - 1) gy = central(rgb, valid, stride, i, width, d, max_jump);
  }
  if (intensity_out) intensity_out[i] = I;
  if (packed_out) packed_out[i] = make_float4(I, gx, gy, 0.0f);
}

}  // namespace

extern "C" {

int r3d_intensity_map(r3d_ctx* ctx, const uint8_t* d_rgb, const float* d_valid, int valid_stride, int height, int width, float max_jump,
                      float* d_intensity_out, float* d_packed_out) {
  R3D_REQUIRE(ctx != nullptr, "ctx is NULL");
  R3D_REQUIRE(d_rgb != nullptr && d_valid != nullptr, "NULL input pointer");
  R3D_REQUIRE(valid_stride == 1 || valid_stride == 3,
              "valid_stride must be 1 (a depth raster) or 3 (the z column of a vertex map), got %d", valid_stride);
  R3D_REQUIRE(height >= 1 && width >= 1, "a %d x %d raster has no pixels", height, width);
  R3D_REQUIRE((int64_t)width * height < ((int64_t)1 << 31) - kTrackTile, "raster of %d x %d pixels is too large for tracking", height,
              width);
  R3D_REQUIRE(max_jump >= 0.f, "max_jump must be >= 0");   // NaN fails
  R3D_REQUIRE(((uintptr_t)d_packed_out & 15) == 0, "d_packed_out must be 16-byte aligned");
  const size_t n = (size_t)height * width;
  const void* buf[4] = {d_rgb, d_valid, d_intensity_out, d_packed_out};
  const size_t bytes[4] = {n * 3, ((n - 1) * (size_t)valid_stride + 1) * sizeof(float), n * 4, n * 16};
  for (int a = 2; a < 4; ++a) {
    if (!buf[a]) continue;
    for (int b = 0; b < a; ++b)
      R3D_REQUIRE(!buf[b] || !r3d_ranges_overlap(buf[a], bytes[a], buf[b], bytes[b]), "an output overlaps an input or the other output");
  }
  int rc = r3d_ctx_enter(ctx);
  if (rc) return rc;
  if (!d_intensity_out && !d_packed_out) return R3D_OK;
  for (int a = 2; a < 4; ++a)
    if (buf[a]) r3d_wrote(ctx, buf[a], bytes[a]);
  hipLaunchKernelGGL(intensity_map_kernel, dim3((unsigned)((n + kThreads - 1) / kThreads)), dim3(kThreads), 0, ctx->stream, d_rgb, d_valid,
                     valid_stride, height, width, max_jump, d_intensity_out, reinterpret_cast<float4*>(d_packed_out));
  R3D_HIP(hipGetLastError());
  return R3D_OK;
}

}  // extern "C"
