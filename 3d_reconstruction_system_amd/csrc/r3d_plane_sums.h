// Point-to-plane rigid ICP step, stated once for the estimators that take it: plane ICP (r3d_plane.hip), coloured ICP
// (r3d_color_icp.hip) and frame-to-model tracking with and without its colour term (r3d_track.hip).  Here: what a pair adds
// to the 29 fp64 sums of the linearised 6x6 normal equations, the solve (Cholesky + exponential map) as host+device code --
// the ICP loop runs without a host round trip per iteration and the very same arithmetic is callable on a CPU-only box
// (r3d_plane_step_from_sums) -- the one finish kernel over it (plane_finish_kernel<K>, K = 29, or 31 with the photometric count
// and sum behind the 29), and the grid of a cloud's sums pass (accumulate_blocks).  The rows' deterministic reduction and the
// ICP state: r3d_sums_dev.h.  The schedule of the two cloud loops: r3d_icp_loop_run (r3d_icp.hip).  Which pairs may take part
// stays with each accumulate kernel (plane_pair in r3d_plane.hip, restated in color_accumulate_kernel): DESIGN.md 4.5v.
//
// NOT IN THE REFERENCE (ICP estimation is build-defined).  What it serves IS the reference's use of
// ICP: "match the point clouds corresponding to two images" (readme.md:25) -- the relative pose of two single-view
// camera clouds, ./point/0.txt and ./point/24.txt (other_tools/transfer_T_icp.py:107-108), which the reference
// obtained by hand in CloudCompare and stored as T_data.txt (icp:99).
//
// One matched pair (p = moved source point, q = its nearest target point, n = unit normal of the target surface at q):
//   residual r = n . (p - q);  a small rigid motion (omega, v) changes it by  (p x n) . omega + n . v,  so with
//   J = [p x n ; n] (6 numbers) the step minimises sum w (r + J . x)^2:   (sum w J J^T) x = - sum w J r.
// Sums: [0] sum w, [1] sum w r^2, [2..7] sum w J r, [8..28] upper triangle of sum w J J^T, row-major.
#pragma once

#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdint>

#include "r3d_sums_dev.h"

namespace r3d_plane {

constexpr int kSums = 29;

// One workgroup per CU at the most: every workgroup of a cloud's sums pass pays a K-value fp64 tree reduction and leaves a row for
// plane_finish_kernel to read (four per CU: accumulate 20 us + finish 19 us per iteration on a 307k-pair cloud, mostly those
// reductions)
inline int accumulate_blocks(int num_cus, int64_t n_src) {
  const int blocks = (int)std::min<int64_t>((n_src + r3d_sums::kThreads - 1) / r3d_sums::kThreads, (int64_t)num_cus);
  return blocks < 1 ? 1 : blocks;
}

#if defined(__HIPCC__)
struct __attribute__((packed, aligned(4))) P3 {
  float x, y, z;
};

// r = n . (p - q), evaluated left to right in fp64 (the differences of fp32 inputs are exact there)
__device__ __forceinline__ double plane_residual(const double p[3], const double q[3], const double n[3]) {
  return n[0] * (p[0] - q[0]) + n[1] * (p[1] - q[1]) + n[2] * (p[2] - q[2]);
}

// what a residual r with J = [p x n ; n] adds to the normal equations alone, [2..28]: the plane pair below, and any other term
// whose linearisation has that shape (the photometric term of r3d_track.hip, where n is the pulled-back image gradient)
__device__ __forceinline__ void jacobian_accumulate(double* acc, double w, const double p[3], const double n[3], double r) {
  const double J[6] = {p[1] * n[2] - p[2] * n[1], p[2] * n[0] - p[0] * n[2], p[0] * n[1] - p[1] * n[0], n[0], n[1], n[2]};
  int k = 8;
#pragma unroll
  for (int a = 0; a < 6; ++a) {
    const double wj = w * J[a];
    acc[2 + a] += wj * r;
#pragma unroll
    for (int b = a; b < 6; ++b) acc[k++] += wj * J[b];
  }
}

__device__ __forceinline__ void pair_accumulate(double acc[kSums], double w, const double p[3], const double n[3], double r) {
  acc[0] += w;
  acc[1] += w * r * r;
  jacobian_accumulate(acc, w, p, n, r);
}
#endif

// T (row-major 4x4, rigid) from the 29 sums.  Returns 0, or 1 when the step is undefined (fewer than 6 pairs, or the
// normal equations are singular to working precision: the matched normals do not constrain all six freedoms -- one
// plane, two parallel walls, ..., or no finite T follows from the sums): T is then the identity.  *rms_out (optional) = sqrt(sum w r^2 / sum w).
R3D_HD inline int step_from_sums(const double s[kSums], double T[16], double* rms_out) {
  for (int k = 0; k < 16; ++k) T[k] = (k % 5 == 0) ? 1.0 : 0.0;
  const double n = s[0];
  if (rms_out) *rms_out = n > 0.0 ? sqrt((s[1] > 0.0 ? s[1] : 0.0) / n) : 0.0;
  if (!(n >= 6.0)) return 1;
  double A[6][6], x[6];
  int k = 8;
  for (int a = 0; a < 6; ++a)
    for (int b = a; b < 6; ++b) {
      A[a][b] = s[k];
      A[b][a] = s[k];
      ++k;
    }
  // the rotation block is in (length)^2, the translation block dimensionless: scale the unknowns so that the pivot
  // test means the same for a cloud in millimetres and one in kilometres
  double tr_rot = A[0][0] + A[1][1] + A[2][2], tr_tra = A[3][3] + A[4][4] + A[5][5];
  if (!(tr_rot > 0.0) || !(tr_tra > 0.0)) return 1;
  const double len = sqrt(tr_rot / tr_tra);   // a typical lever arm
  double sc[6] = {1.0 / len, 1.0 / len, 1.0 / len, 1.0, 1.0, 1.0};
  double g[6];
  for (int a = 0; a < 6; ++a) {
    g[a] = -s[2 + a] * sc[a];
    for (int b = 0; b < 6; ++b) A[a][b] *= sc[a] * sc[b];
  }
  double trace = 0.0;
  for (int a = 0; a < 6; ++a) trace += A[a][a];
  // Cholesky A = L L^T in place (lower triangle)
  for (int j = 0; j < 6; ++j) {
    double d = A[j][j];
    for (int m = 0; m < j; ++m) d -= A[j][m] * A[j][m];
    if (!(d > 1e-10 * trace)) return 1;
    d = sqrt(d);
    A[j][j] = d;
    for (int i = j + 1; i < 6; ++i) {
      double v = A[i][j];
      for (int m = 0; m < j; ++m) v -= A[i][m] * A[j][m];
      A[i][j] = v / d;
    }
  }
  for (int i = 0; i < 6; ++i) {   // L y = g
    double v = g[i];
    for (int m = 0; m < i; ++m) v -= A[i][m] * x[m];
    x[i] = v / A[i][i];
  }
  for (int i = 5; i >= 0; --i) {  // L^T x = y
    double v = x[i];
    for (int m = i + 1; m < 6; ++m) v -= A[m][i] * x[m];
    x[i] = v / A[i][i];
  }
  for (int a = 0; a < 6; ++a) {
    x[a] *= sc[a];
    if (!(fabs(x[a]) < 1e300)) return 1;   // also catches NaN
  }
  // rotation = exp([omega]x) (Rodrigues): exactly orthogonal whatever the step size
  const double wx = x[0], wy = x[1], wz = x[2];
  const double th2 = wx * wx + wy * wy + wz * wz, th = sqrt(th2);
  double a_, b_;                       // R = I + a [w]x + b [w]x^2
  if (th < 1e-6) {
    a_ = 1.0 - th2 / 6.0;
    b_ = 0.5 - th2 / 24.0;
  } else {
    a_ = sin(th) / th;
    b_ = (1.0 - cos(th)) / th2;
  }
  const double K[9] = {0, -wz, wy, wz, 0, -wx, -wy, wx, 0};
  double K2[9];
  for (int r = 0; r < 3; ++r)
    for (int c = 0; c < 3; ++c) K2[3 * r + c] = K[3 * r] * K[c] + K[3 * r + 1] * K[3 + c] + K[3 * r + 2] * K[6 + c];
  for (int r = 0; r < 3; ++r) {
    for (int c = 0; c < 3; ++c) T[4 * r + c] = (r == c ? 1.0 : 0.0) + a_ * K[3 * r + c] + b_ * K2[3 * r + c];
    T[4 * r + 3] = x[3 + r];
  }
  // a finite omega beyond 1e154 passes the test above and overflows th2 (sin(inf) is NaN): a step that is not finite is no step
  double chk = 0.0;
  for (int k = 0; k < 12; ++k) chk += fabs(T[k]);
  if (!(chk < INFINITY)) {
    for (int k = 0; k < 16; ++k) T[k] = (k % 5 == 0) ? 1.0 : 0.0;
    return 1;
  }
  return 0;
}

#if defined(__HIPCC__)
// ONE workgroup (r3d_sums::finish_rows): partial rows in fixed order -> the K sums -> optionally the step solved from the first
// 29 and the ICP state.  The state update is the one every loop shares, so every loop's state means the same (a degenerate
// step is the identity: T_total stays).  static: every source that launches it has its own copy, as r3d_consensus_dev.h's fold.
template <int K>
static __global__ __launch_bounds__(r3d_sums::kThreads) void plane_finish_kernel(const double* __restrict__ partials, int n_rows,
                                                                                 double* __restrict__ sums_out,
                                                                                 double* __restrict__ state) {
  static_assert(K >= kSums, "the step is solved from the first 29 sums");
  r3d_sums::finish_rows<K>(partials, n_rows, sums_out, state,
                           [](const double* s, double* T, double* rms) { return step_from_sums(s, T, rms); });
}
#endif

}  // namespace r3d_plane
