// fp64 sums rows and the device-resident ICP state, stated once for every estimation loop of the library: the similarity ICP
// (r3d_icp.hip, r3d_nnindex.hip: 18 sums), the point-to-plane ICP and frame-to-model tracking (r3d_plane.hip, r3d_track.hip:
// 29 sums) and the RANSAC refit (r3d_ransac.hip: 10 sums).  A sums pass is
//   per-lane accumulators -> block_reduce_store: one partial row per 256-thread workgroup
//   -> finish_rows (ONE workgroup): fold_rows + block_reduce_store -> the sums [-> a step solved from them -> icp_state_advance]
// and every order in it is fixed, so the sums are the same bits run to run (no float atomics).  What a pair adds to a row, and
// the solver that turns a row into a step, stay with their estimator (r3d_icp_sums.h, r3d_plane_sums.h).
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

#if defined(__HIPCC__)
#define R3D_HD __host__ __device__
#else
#define R3D_HD
#endif

namespace r3d_sums {

constexpr int kThreads = 256;   // every kernel that reduces a row runs 4 waves

// ---- device-resident ICP state (R3D_ICP_STATE_DOUBLES doubles, see include/r3d.h) ----
constexpr int kStateTTotal = 0;    // [16] row-major 4x4: product of all steps so far (maps the ORIGINAL source)
constexpr int kStateTStep = 16;    // [16] the last step
constexpr int kStateIters = 32;    // iterations solved so far
constexpr int kStateStatus = 33;   // 0 ok; 1 = a step was degenerate (too few pairs / no spread / singular equations) and was skipped
constexpr int kStateRms = 34;      // weighted RMS match distance seen by the last step (before it was applied)
constexpr int kStatePairs = 35;    // weight sum (= pair count when unweighted) of the last step
constexpr int kStateHistory = 48;  // rms of step k at [48 + k] while it fits
constexpr int kStateDoubles = 512;

#if defined(__HIPCC__)
__device__ __forceinline__ double wave_sum(double v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off, 64);
  return v;
}

// Workgroup (256 threads) reduction of per-lane accumulators into one row of K partials: shuffle tree over the 64 lanes, LDS
// across the 4 waves, fixed order -> bitwise repeatable.  `red` is __shared__ [4][K].
template <int K>
__device__ __forceinline__ void block_reduce_store(double acc[K], double (*red)[K], double* __restrict__ row) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
  for (int k = 0; k < K; ++k) {
    const double v = wave_sum(acc[k]);
    if (lane == 0) red[wave][k] = v;
  }
  __syncthreads();
  if (threadIdx.x < K) {
    double v = 0.0;
    for (int w = 0; w < kThreads / 64; ++w) v += red[w][threadIdx.x];
    row[threadIdx.x] = v;
  }
}

// First stage of a finish: thread t adds the partial rows t, t + 256, ... to its accumulators, in that order.
template <int K>
__device__ __forceinline__ void fold_rows(double acc[K], const double* __restrict__ partials, int n_rows) {
  for (int b = threadIdx.x; b < n_rows; b += kThreads) {
#pragma unroll
    for (int k = 0; k < K; ++k) acc[k] += partials[(int64_t)b * K + k];
  }
}

// One thread: T_total <- step . T_total; step, history, iteration count, status, rms and weight of the step.  `bad` (the solver
// found the step undefined and left T the identity) is sticky in the status.  Every loop's state means the same because every
// loop updates it here.
__device__ inline void icp_state_advance(const double T[16], double rms, int bad, double weight, double* __restrict__ st) {
  double tot[16], nt[16];
  for (int k = 0; k < 16; ++k) tot[k] = st[kStateTTotal + k];
  for (int r = 0; r < 4; ++r)
    for (int c = 0; c < 4; ++c) {
      double v = 0.0;
      for (int m = 0; m < 4; ++m) v += T[4 * r + m] * tot[4 * m + c];
      nt[4 * r + c] = v;
    }
  for (int k = 0; k < 16; ++k) {
    st[kStateTStep + k] = T[k];
    st[kStateTTotal + k] = nt[k];
  }
  const int it = (int)st[kStateIters];
  if (kStateHistory + it < kStateDoubles) st[kStateHistory + it] = rms;
  st[kStateIters] = (double)(it + 1);
  if (bad) st[kStateStatus] = 1.0;
  st[kStateRms] = rms;
  st[kStatePairs] = weight;
}

// The body of a finish kernel (ONE workgroup of 256 threads): partial rows in fixed order -> the K sums in LDS -> sums_out
// (NULL: not written) and, with a state, the step `solve(s, T, &rms)` makes of them (returns non-zero when it is undefined)
// and the state update, by thread 0.  One launch instead of (final reduction, solve).
template <int K, class Solve>
__device__ __forceinline__ void finish_rows(const double* __restrict__ partials, int n_rows, double* __restrict__ sums_out,
                                            double* __restrict__ state, Solve solve) {
  __shared__ double red[kThreads / 64][K];
  __shared__ double total[K];
  double acc[K];
#pragma unroll
  for (int k = 0; k < K; ++k) acc[k] = 0.0;
  fold_rows<K>(acc, partials, n_rows);
  block_reduce_store<K>(acc, red, total);
  __syncthreads();
  if (threadIdx.x < K && sums_out) sums_out[threadIdx.x] = total[threadIdx.x];
  if (threadIdx.x == 0 && state != nullptr) {
    double s[K], T[16], rms = 0.0;
    for (int k = 0; k < K; ++k) s[k] = total[k];
    const int bad = solve(s, T, &rms);
    icp_state_advance(T, rms, bad, s[0], state);
  }
}
#endif

}  // namespace r3d_sums
