// Depth pyramid for gfx950 (MI355X): the level camera and the depth-aware half-sampler that coarse-to-fine tracking
// (r3d_track.hip: r3d_tsdf_track_pyramid) walks.  NOT IN THE REFERENCE: build-defined, specified in include/r3d.h ("Depth pyramid").
//
//   depth_half_kernel   one lane per OUTPUT pixel: its 2 x 2 input block, the minimum of the valid depths, the f32 mean of the
//                       valid depths within max_jump of that minimum (foreground wins), one dword stored.  With in_stride 1 a
//                       lane reads each of its two rows as ONE 8-byte load where that row's pairs are 8-byte aligned -- a property
//                       of the base address and the parity of `width`, uniform over the launch -- and as two 4-byte loads where
//                       they are not; with in_stride 3 (the z column of a vertex map) four 4-byte loads 12 / 24 bytes apart.  A
//                       wave's loads cover 512 consecutive bytes per row, its store 256.  No LDS, no atomics, no scratch; every
//                       output is a function of its own block alone, so the result does not depend on the launch geometry.
#include <cmath>

#include "r3d_internal.h"

namespace {

constexpr int kThreads = 256;
constexpr int kTrackTile = 1024;   // the raster-size limit of the tracking calls (r3d_track.hip: kTile)

__device__ __forceinline__ bool valid_depth(float d) { return isfinite(d) && d > 0.0f; }

__global__ __launch_bounds__(kThreads) void depth_half_kernel(const float* __restrict__ in, int in_stride, int width, int out_width,
                                                              int n_out, bool pair0, bool pair1, float max_jump,
                                                              float* __restrict__ out) {
  const int i = (int)blockIdx.x * kThreads + (int)threadIdx.x;   // n_out < 2^29
  if (i >= n_out) return;
  const int vo = i / out_width, uo = i - vo * out_width;
  const int64_t p0 = (int64_t)(2 * vo) * width + 2 * uo, p1 = p0 + width;   // pixel indices of the block's two rows
  float d[4];
  if (in_stride == 1) {
    if (pair0) {
      const float2 a = *reinterpret_cast<const float2*>(in + p0);
      d[0] = a.x, d[1] = a.y;
    } else {
      d[0] = in[p0], d[1] = in[p0 + 1];
    }
    if (pair1) {
      const float2 b = *reinterpret_cast<const float2*>(in + p1);
      d[2] = b.x, d[3] = b.y;
    } else {
      d[2] = in[p1], d[3] = in[p1 + 1];
    }
  } else {
    d[0] = in[p0 * 3], d[1] = in[(p0 + 1) * 3], d[2] = in[p1 * 3], d[3] = in[(p1 + 1) * 3];
  }
  bool ok[4];
  bool any = false;
  float m = 0.0f;
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    ok[k] = valid_depth(d[k]);
    if (ok[k] && (!any || d[k] < m)) m = d[k];
    any = any || ok[k];
  }
  float s = 0.0f;
  int count = 0;
#pragma unroll
  for (int k = 0; k < 4; ++k)
    if (ok[k] && d[k] - m <= max_jump) {
      s += d[k];
      ++count;
    }
  out[i] = any ? __fdiv_rn(s, (float)count) : 0.0f;   // the minimum itself is always included: count >= 1
}

}  // namespace

extern "C" {

int r3d_camera_half(const r3d_camera* cam, r3d_camera** out) {
  R3D_REQUIRE(cam != nullptr, "camera is NULL");
  R3D_REQUIRE(out != nullptr, "out is NULL");
  R3D_REQUIRE(cam->height >= 2 && cam->width >= 2, "a %d x %d raster cannot be halved", cam->height, cam->width);
  const double fx = 0.5 * cam->fx, fy = 0.5 * cam->fy, cx = 0.5 * (cam->cx - 0.5), cy = 0.5 * (cam->cy - 0.5);
  r3d_camera* half = nullptr;
  int rc = r3d_camera_create(cam->ctx, cam->height >> 1, cam->width >> 1, fx, fy, cx, cy, &half);
  if (rc) return rc;
  *out = half;
  return R3D_OK;
}

int r3d_depth_half(r3d_ctx* ctx, const float* d_in, int in_stride, int height, int width, float max_jump, float* d_out) {
  R3D_REQUIRE(ctx != nullptr, "ctx is NULL");
  R3D_REQUIRE(d_in != nullptr && d_out != nullptr, "NULL raster pointer");
  R3D_REQUIRE(in_stride == 1 || in_stride == 3, "in_stride must be 1 (a depth raster) or 3 (the z column of a vertex map), got %d",
              in_stride);
  R3D_REQUIRE(height >= 2 && width >= 2, "a %d x %d raster cannot be halved", height, width);
  R3D_REQUIRE((int64_t)width * height < ((int64_t)1 << 31) - kTrackTile, "raster of %d x %d pixels is too large for tracking", height,
              width);
  R3D_REQUIRE(max_jump >= 0.f, "max_jump must be >= 0");   // NaN fails
  const size_t n_in = (size_t)height * width;
  const int out_h = height >> 1, out_w = width >> 1;
  const size_t in_bytes = ((n_in - 1) * (size_t)in_stride + 1) * sizeof(float), out_bytes = (size_t)out_h * out_w * sizeof(float);
  R3D_REQUIRE(!r3d_ranges_overlap(d_in, in_bytes, d_out, out_bytes), "the output overlaps the input");
  int rc = r3d_ctx_enter(ctx);
  if (rc) return rc;
  r3d_wrote(ctx, d_out, out_bytes);
  // a row's pixel pairs start at even pixel indices in row 2 v' and at `width` + an even index in row 2 v' + 1
  const bool base8 = ((uintptr_t)d_in & 7) == 0, odd = (width & 1) != 0;
  const bool pair0 = base8, pair1 = base8 != odd;
  const int n_out = out_h * out_w;
  hipLaunchKernelGGL(depth_half_kernel, dim3((n_out + kThreads - 1) / kThreads), dim3(kThreads), 0, ctx->stream, d_in, in_stride, width,
                     out_w, n_out, pair0, pair1, max_jump, d_out);
  R3D_HIP(hipGetLastError());
  return R3D_OK;
}

}  // extern "C"
