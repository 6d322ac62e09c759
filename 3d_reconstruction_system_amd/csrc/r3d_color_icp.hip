// Coloured ICP between two unorganised clouds for gfx950 (MI355X): Park, Zhou and Koltun's colour-assisted point-to-plane
// registration (ICCV 2017).  NOT IN THE REFERENCE: build-defined, specified in include/r3d.h ("Coloured ICP"), DESIGN.md 4.5t.
//
//   color_gradient_kernel    one lane per point of an index's own cloud: the f32 intensity of its colour word, and the gradient
//                            of the intensity over its tangent plane from its k nearest neighbours -- a 3x3 fp64 least-squares
//                            system with the constraint row c n, solved by the adjugate.  The neighbour lists are the stored ones
//                            of r3d_nn_index_knn_self (in a buffer of this file's own), as r3d_fpfh_knn reads them.
//   color_accumulate_kernel  the 29 fp64 sums of the untrimmed plane pair (r3d_plane_sums.h: plane_residual, pair_accumulate)
//                            plus, per accepted pair, the photometric term through jacobian_accumulate, its count and sum rI^2
// The finish (r3d_plane::plane_finish_kernel<31>: rows in fixed order -> 31 sums -> the plane solver on the first 29 -> the ICP
// state in HBM) and the grid of the sums pass are r3d_plane_sums.h's; the loop schedule is r3d_icp_loop_run (r3d_icp.hip).
// No float atomics anywhere: bitwise repeatable run to run.
#include <cmath>

#include "r3d_internal.h"
#include "r3d_plane_sums.h"

namespace {

constexpr int kThreads = 256;
constexpr int kSums = R3D_COLOR_ICP_SUMS;
constexpr uint32_t kNoRow = 0xffffffffu;
static_assert(kSums == r3d_plane::kSums + 2, "the plane sums, then the photometric count and sum rI^2");

using r3d_plane::P3;

// r3d_intensity_map's rule on a colour word (r | g << 8 | b << 16; the alpha byte is never read)
__device__ __forceinline__ float word_intensity(uint32_t w) {
  const float r = (float)(w & 255u), g = (float)((w >> 8) & 255u), b = (float)((w >> 16) & 255u);
  return (0.299f * r + 0.587f * g) + 0.114f * b;
}

__global__ __launch_bounds__(kThreads) void color_gradient_kernel(const float* __restrict__ xyz, const float* __restrict__ nrm,
                                                                  const uint32_t* __restrict__ rgba, const uint32_t* __restrict__ idx,
                                                                  const float* __restrict__ d2l, int64_t n, int k, float r2,
                                                                  float* __restrict__ inten_out, float* __restrict__ grad_out,
                                                                  uint32_t* __restrict__ count_out) {
  const int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x;
  if (i >= n) return;
  const P3* __restrict__ P = reinterpret_cast<const P3*>(xyz);
  const P3 ps = P[i], ns = reinterpret_cast<const P3*>(nrm)[i];
  const float Ii = word_intensity(rgba[i]);
  inten_out[i] = Ii;
  const double px = (double)ps.x, py = (double)ps.y, pz = (double)ps.z;
  const double n0 = (double)ns.x, n1 = (double)ns.y, n2 = (double)ns.z;
  double A00 = 0.0, A01 = 0.0, A02 = 0.0, A11 = 0.0, A12 = 0.0, A22 = 0.0, b0 = 0.0, b1 = 0.0, b2 = 0.0;
  uint32_t c = 0;
  for (int t = 0; t < k; ++t) {
    const uint32_t j = idx[i * k + t];
    if (j == kNoRow || (int64_t)j >= n) break;   // the tail of a short list
    if (d2l[i * k + t] > r2) break;              // ascending: everything behind is farther still
    ++c;
    const P3 q = P[j];
    const double e0 = (double)q.x - px, e1 = (double)q.y - py, e2 = (double)q.z - pz;
    const double h = (e0 * n0 + e1 * n1) + e2 * n2;
    const double t0 = e0 - h * n0, t1 = e1 - h * n1, t2 = e2 - h * n2;
    const double dI = (double)word_intensity(rgba[j]) - (double)Ii;
    A00 += t0 * t0;
    A01 += t0 * t1;
    A02 += t0 * t2;
    A11 += t1 * t1;
    A12 += t1 * t2;
    A22 += t2 * t2;
    b0 += t0 * dI;
    b1 += t1 * dI;
    b2 += t2 * dI;
  }
  if (count_out) count_out[i] = c;
  const double cc = (double)c, c2 = cc * cc;
  A00 += (c2 * n0) * n0;
  A01 += (c2 * n0) * n1;
  A02 += (c2 * n0) * n2;
  A11 += (c2 * n1) * n1;
  A12 += (c2 * n1) * n2;
  A22 += (c2 * n2) * n2;
  const double C00 = A11 * A22 - A12 * A12, C01 = A02 * A12 - A01 * A22, C02 = A01 * A12 - A02 * A11;
  const double C11 = A00 * A22 - A02 * A02, C12 = A01 * A02 - A00 * A12, C22 = A00 * A11 - A01 * A01;
  const double det = (A00 * C00 + A01 * C01) + A02 * C02, tr = (A00 + A11) + A22;
  bool ok = isfinite((px + py) + pz) && isfinite((n0 + n1) + n2) && !(ns.x == 0.f && ns.y == 0.f && ns.z == 0.f) && c >= 3u;
  ok = ok && isfinite(det) && det > R3D_COLOR_GRADIENT_FLOOR * ((tr * tr) * tr);
  P3 g;
  g.x = g.y = g.z = __uint_as_float(0x7fc00000u);
  if (ok) {
    g.x = (float)(((C00 * b0 + C01 * b1) + C02 * b2) / det);
    g.y = (float)(((C01 * b0 + C11 * b1) + C12 * b2) / det);
    g.z = (float)(((C02 * b0 + C12 * b1) + C22 * b2) / det);
  }
  reinterpret_cast<P3*>(grad_out)[i] = g;
}

__global__ __launch_bounds__(kThreads) void color_accumulate_kernel(const float* __restrict__ src, const float* __restrict__ src_I,
                                                                    int64_t n_src, const float* __restrict__ tgt,
                                                                    const float* __restrict__ nrm, const float* __restrict__ tgt_I,
                                                                    const float* __restrict__ tgt_g, int64_t n_tgt,
                                                                    const uint32_t* __restrict__ idx, const float* __restrict__ d2,
                                                                    float max_d2, double w_photo, double i_max,
                                                                    double* __restrict__ partials, float* __restrict__ photo_out) {
  __shared__ double red[kThreads / 64][kSums];
  double acc[kSums];
#pragma unroll
  for (int k = 0; k < kSums; ++k) acc[k] = 0.0;
  for (int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x; i < n_src; i += (int64_t)gridDim.x * kThreads) {
    float photo = __uint_as_float(0x7fc00000u);
    do {
      // the untrimmed plane pair of r3d_plane.hip (plane_pair), test for test
      const int64_t j = (int64_t)idx[i];
      if (j >= n_tgt) break;                                   // a caller's index array is data
      if (max_d2 >= 0.f && !(d2[i] <= max_d2)) break;
      const P3 ps = reinterpret_cast<const P3*>(src)[i], qs = reinterpret_cast<const P3*>(tgt)[j],
               ns = reinterpret_cast<const P3*>(nrm)[j];
      const double p[3] = {(double)ps.x, (double)ps.y, (double)ps.z};
      const double n[3] = {(double)ns.x, (double)ns.y, (double)ns.z};
      const double q[3] = {(double)qs.x, (double)qs.y, (double)qs.z};
      if (ns.x == 0.f && ns.y == 0.f && ns.z == 0.f) break;    // no plane at this target point
      const double r = r3d_plane::plane_residual(p, q, n);
      if (!isfinite(r) || !isfinite((p[0] + p[1]) + p[2])) break;
      r3d_plane::pair_accumulate(acc, 1.0, p, n, r);
      // the photometric term
      const P3 gs = reinterpret_cast<const P3*>(tgt_g)[j];
      const double g[3] = {(double)gs.x, (double)gs.y, (double)gs.z};
      const double d0 = (p[0] - r * n[0]) - q[0], d1 = (p[1] - r * n[1]) - q[1], d2p = (p[2] - r * n[2]) - q[2];
      const double rI = ((double)tgt_I[j] + ((g[0] * d0 + g[1] * d1) + g[2] * d2p)) - (double)src_I[i];
      const double gn = (g[0] * n[0] + g[1] * n[1]) + g[2] * n[2];
      const double a[3] = {g[0] - gn * n[0], g[1] - gn * n[1], g[2] - gn * n[2]};
      if (!(isfinite(rI) && isfinite(a[0]) && isfinite(a[1]) && isfinite(a[2]) && fabs(rI) <= i_max)) break;
      r3d_plane::jacobian_accumulate(acc, w_photo, p, a, rI);
      acc[29] += 1.0;
      acc[30] += rI * rI;
      photo = (float)rI;
    } while (false);
    if (photo_out) photo_out[i] = photo;
  }
  r3d_sums::block_reduce_store<kSums>(acc, red, partials + (int64_t)blockIdx.x * kSums);
}

struct ColorPass {
  const float *src_I, *nrm, *tgt_I, *tgt_g;
  float max_d2;
  double w_photo, i_max;
};

// kWsColorRows: the partial rows, then the 31 sums (64 kB at the most), are this file's alone and always asked for at their largest
// size, as r3d_registration_sums keeps its own: nothing here depends on, or disturbs, what other calls leave in the shared workspaces.
// one sums pass: partial rows -> d_sums (the 31 doubles behind the rows when NULL is given) [-> the state]
int color_sums_enqueue(r3d_ctx* ctx, const float* d_src, int64_t n_src, const float* d_tgt, int64_t n_tgt, const uint32_t* d_idx,
                       const float* d_d2, const ColorPass& c, double* d_sums, double* d_state, float* d_photo_out,
                       double** d_sums_used) {
  const int blocks = r3d_plane::accumulate_blocks(ctx->num_cus, n_src);
  void* rows_v = nullptr;
  int rc = r3d_scratch(ctx, kWsColorRows, ((size_t)ctx->num_cus + 1) * kSums * sizeof(double), &rows_v);
  if (rc) return rc;
  double* rows = static_cast<double*>(rows_v);
  if (!d_sums && d_sums_used) d_sums = rows + (size_t)blocks * kSums;
  hipLaunchKernelGGL(color_accumulate_kernel, dim3(blocks), dim3(kThreads), 0, ctx->stream, d_src, c.src_I, n_src, d_tgt, c.nrm, c.tgt_I,
                     c.tgt_g, n_tgt, d_idx, d_d2, c.max_d2 >= 0.f ? c.max_d2 : -1.f, c.w_photo, c.i_max, rows, d_photo_out);
  hipLaunchKernelGGL(r3d_plane::plane_finish_kernel<kSums>, dim3(1), dim3(kThreads), 0, ctx->stream, (const double*)rows, blocks, d_sums, d_state);
  R3D_HIP(hipGetLastError());
  if (d_sums_used) *d_sums_used = d_sums;
  return R3D_OK;
}

}  // namespace

extern "C" {

int r3d_color_gradient_knn(r3d_nn_index* index, int k, double radius, const float* d_normals, const uint32_t* d_rgba,
                           float* d_intensity_out, float* d_grad_out, uint32_t* d_count_out) {
  R3D_REQUIRE(index != nullptr, "nn index is NULL");
  R3D_REQUIRE(k >= 3 && k <= 32, "k must be in [3, 32], got %d", k);
  R3D_REQUIRE(!std::isnan(radius), "radius is NaN");
  R3D_REQUIRE(d_normals && d_rgba && d_intensity_out && d_grad_out, "d_normals, d_rgba, d_intensity_out or d_grad_out is NULL");
  const float* d_xyz = nullptr;
  int64_t n = 0;
  r3d_ctx* ctx = nullptr;
  int rc = r3d_nn_index_target(index, &d_xyz, &n, &ctx);
  if (rc) return rc;
  const r3d_range outs[3] = {{d_intensity_out, (size_t)n * 4}, {d_grad_out, (size_t)n * 12}, {d_count_out, (size_t)n * 4}};
  const r3d_range ins[3] = {{d_xyz, (size_t)n * 12}, {d_normals, (size_t)n * 12}, {d_rgba, (size_t)n * 4}};
  R3D_REQUIRE(!r3d_any_overlap(outs, 3, ins, 3), "an output overlaps another output, the normals, the colours or the index's cloud");
  if ((rc = r3d_ctx_enter(ctx))) return rc;
  if (n == 0) return R3D_OK;
  // the lists (idx | d2), stored as r3d_fpfh_knn stores them, in a workspace of this file's own
  r3d_carve lists;
  const auto idx_h = lists.take<uint32_t>((size_t)n * k);
  const auto d2l_h = lists.take<float>((size_t)n * k);
  if ((rc = r3d_scratch(ctx, kWsColorLists, lists))) return rc;
  uint32_t* idx = lists.at(idx_h);
  float* d2l = lists.at(d2l_h);
  if ((rc = r3d_nn_index_knn_self(index, k, idx, d2l))) return rc;
  for (int i = 0; i < 3; ++i)
    if (outs[i].p) r3d_wrote(ctx, outs[i].p, outs[i].bytes);
  const float r2 = radius > 0.0 ? (float)(radius * radius) : INFINITY;
  hipLaunchKernelGGL(color_gradient_kernel, dim3((unsigned)((n + kThreads - 1) / kThreads)), dim3(kThreads), 0, ctx->stream, d_xyz,
                     d_normals, d_rgba, (const uint32_t*)idx, (const float*)d2l, n, k, r2, d_intensity_out, d_grad_out, d_count_out);
  R3D_HIP(hipGetLastError());
  return R3D_OK;
}

int r3d_icp_color_accumulate(r3d_ctx* ctx, const float* d_src, const float* d_src_intensity, int64_t n_src, const float* d_tgt,
                             const float* d_tgt_normals, const float* d_tgt_intensity, const float* d_tgt_grad, int64_t n_tgt,
                             const uint32_t* d_idx, const float* d_d2, float max_d2, double w_photo, double i_max, double* h_sums,
                             float* d_photo_out) {
  int rc = r3d_ctx_enter(ctx);
  if (rc) return rc;
  R3D_REQUIRE(h_sums != nullptr, "h_sums is NULL");
  R3D_REQUIRE(n_src >= 0 && n_tgt >= 0, "negative cloud size");
  R3D_REQUIRE(!std::isnan(max_d2), "max_d2 is NaN");
  R3D_REQUIRE(std::isfinite(w_photo) && w_photo >= 0.0, "w_photo must be finite and >= 0, got %g", w_photo);
  R3D_REQUIRE(std::isfinite(i_max) && i_max > 0.0, "i_max must be finite and > 0, got %g", i_max);
  if (n_src == 0) {
    for (int k = 0; k < kSums; ++k) h_sums[k] = 0.0;
    return R3D_OK;
  }
  R3D_REQUIRE(d_src && d_src_intensity && d_tgt && d_tgt_normals && d_tgt_intensity && d_tgt_grad && d_idx, "NULL device pointer");
  R3D_REQUIRE(!(max_d2 >= 0.f) || d_d2 != nullptr, "max_d2 >= 0 needs the d2 array");
  const r3d_range outs[1] = {{d_photo_out, (size_t)n_src * 4}};
  const r3d_range ins[8] = {{d_src, (size_t)n_src * 12},         {d_src_intensity, (size_t)n_src * 4}, {d_tgt, (size_t)n_tgt * 12},
                            {d_tgt_normals, (size_t)n_tgt * 12}, {d_tgt_intensity, (size_t)n_tgt * 4}, {d_tgt_grad, (size_t)n_tgt * 12},
                            {d_idx, (size_t)n_src * 4},          {d_d2, (size_t)n_src * 4}};
  R3D_REQUIRE(!r3d_any_overlap(outs, 1, ins, 8), "d_photo_out overlaps an input");
  if (d_photo_out) r3d_wrote(ctx, d_photo_out, (size_t)n_src * 4);
  const ColorPass c = {d_src_intensity, d_tgt_normals, d_tgt_intensity, d_tgt_grad, max_d2, w_photo, i_max};
  double* d_sums = nullptr;
  if ((rc = color_sums_enqueue(ctx, d_src, n_src, d_tgt, n_tgt, d_idx, d_d2, c, nullptr, nullptr, d_photo_out, &d_sums))) return rc;
  R3D_HIP(hipMemcpyAsync(h_sums, d_sums, kSums * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
  R3D_HIP(hipStreamSynchronize(ctx->stream));
  return R3D_OK;
}

int r3d_icp_iterate_color(r3d_ctx* ctx, r3d_nn_index* index, const float* d_src_orig, float* d_src, const float* d_src_intensity,
                          int64_t n_src, const float* d_tgt_normals, const float* d_tgt_intensity, const float* d_tgt_grad,
                          uint32_t* d_idx, float* d_d2, int n_iters, float max_d2, double w_photo, double i_max, double* d_state,
                          double* d_sums_out) {
  int rc = r3d_ctx_enter(ctx);
  if (rc) return rc;
  R3D_REQUIRE(index != nullptr, "nn index is NULL");
  R3D_REQUIRE(n_iters >= 0, "n_iters must be >= 0");
  R3D_REQUIRE(n_src >= 6, "need at least 6 source points");
  R3D_REQUIRE(!std::isnan(max_d2), "max_d2 is NaN");
  R3D_REQUIRE(std::isfinite(w_photo) && w_photo >= 0.0, "w_photo must be finite and >= 0, got %g", w_photo);
  R3D_REQUIRE(std::isfinite(i_max) && i_max > 0.0, "i_max must be finite and > 0, got %g", i_max);
  R3D_REQUIRE(d_src && d_src_intensity && d_tgt_normals && d_tgt_intensity && d_tgt_grad && d_idx && d_d2 && d_state,
              "NULL device pointer");
  R3D_REQUIRE(d_src_orig != d_src, "d_src_orig must be a separate buffer (or NULL)");
  const float* d_tgt = nullptr;
  int64_t n_tgt = 0;
  r3d_ctx* ictx = nullptr;
  if ((rc = r3d_nn_index_target(index, &d_tgt, &n_tgt, &ictx))) return rc;
  R3D_REQUIRE(ictx == ctx, "the index belongs to another context");
  const r3d_range outs[5] = {{d_src, (size_t)n_src * 12},
                             {d_idx, (size_t)n_src * 4},
                             {d_d2, (size_t)n_src * 4},
                             {d_state, R3D_ICP_STATE_DOUBLES * sizeof(double)},
                             {d_sums_out, kSums * sizeof(double)}};
  const r3d_range ins[6] = {{d_src_orig, (size_t)n_src * 12},    {d_src_intensity, (size_t)n_src * 4}, {d_tgt, (size_t)n_tgt * 12},
                            {d_tgt_normals, (size_t)n_tgt * 12}, {d_tgt_intensity, (size_t)n_tgt * 4}, {d_tgt_grad, (size_t)n_tgt * 12}};
  R3D_REQUIRE(!r3d_any_overlap(outs, 5, ins, 6), "d_src, d_idx, d_d2, d_state or d_sums_out overlaps another of them or an input");
  const ColorPass c = {d_src_intensity, d_tgt_normals, d_tgt_intensity, d_tgt_grad, max_d2, w_photo, i_max};
  rc = r3d_icp_loop_run(ctx, index, d_src_orig, d_src, n_src, d_idx, d_d2, n_iters, d_state, [&](bool last) {
    return color_sums_enqueue(ctx, d_src, n_src, d_tgt, n_tgt, d_idx, d_d2, c, last ? d_sums_out : nullptr, d_state, nullptr, nullptr);
  });
  if (rc) return rc;
  if (n_iters > 0 && d_sums_out) r3d_wrote(ctx, d_sums_out, kSums * sizeof(double));
  return R3D_OK;
}

}  // extern "C"
