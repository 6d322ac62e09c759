// RANSAC plane segmentation of a fused cloud for gfx950 (MI355X).
//
// NOT IN THE REFERENCE (its data are indoor scenes -- floor, ceiling, walls -- and users of this kind of pipeline call Open3D's
// segment_plane on the fused cloud; no parity with Open3D is claimed).  Semantics: include/r3d.h (r3d_segment_plane) and
// DESIGN.md section 4.5h.
//
// The sampler, the launch plan, the scratch layout and the fold and best kernels are r3d_consensus_dev.h's (shared with
// r3d_register.hip); this file has what a plane is:
//   hypothesis_kernel   one lane per hypothesis: the counter-based sampler, three row gathers, the fp64 cross product, validity;
//                       writes the anchor and the f32 unit normal as six SoA floats (an invalid hypothesis gets NaN normals,
//                       so every one of its tests compares false) and its rows.
//   count_kernel<R>     the hot path: every hypothesis against every point.  Lanes own hypotheses, R of them each, held in
//                       registers with one u32 count apiece; the workgroup's chunk of points goes through LDS in double-buffered
//                       tiles of float4 and every lane reads the SAME point -- one conflict-free broadcast ds_read_b128 serves
//                       64 R pairs.  Grid = point chunks x hypothesis blocks; each workgroup writes its partial counts
//                       [chunk][h] with plain stores.  No atomics, no ballot, no scratch; the tile loop runs to the number of
//                       points the tile holds, so tail slots are never evaluated.
//   refit_kernel       the best hypothesis' inliers by the same f32 test; their ten fp64 sums about the anchor, one row per
//                       workgroup (shuffle tree -> LDS, fixed order: r3d_sums_dev.h)
//   refit_fold_kernel   one wave folds the rows in a fixed order; also fetches the best hypothesis' three points
//   mask_kernel         the final fp64 test against the refined plane; per-workgroup inlier counts, integer atomics
// The 3x3 eigenproblem (r3d_sym3.h) is solved on the host, as r3d_umeyama_from_sums does its SVD, between refit_fold and mask.
#include <algorithm>
#include <cmath>

#include "r3d_consensus_dev.h"
#include "r3d_internal.h"
#include "r3d_sums_dev.h"
#include "r3d_sym3.h"

namespace {

using r3d_consensus::kThreads;
using r3d_consensus::sample_row;
constexpr int kTile = 512;            // points per LDS tile: 2 per thread, 8 KiB as float4, two buffers
constexpr int kSums = 10;             // m, S1 (3), S2 (6)

// what the host reads back after the refit, one copy
struct Misc {
  r3d_consensus::BestHead head;
  float abc[12];          // the best hypothesis' three points, xyz each
  double sums[kSums];
  unsigned long long n_inliers;
};

struct Plane64 {
  double n[3], l2;
  bool valid;
};

// N = (b - a) x (c - a) and l2 = N . N in fp64 as written; the unit normal N / sqrt(l2)
__host__ __device__ __forceinline__ Plane64 plane_of(const float* a, const float* b, const float* c, bool rows_differ) {
  const double ax = a[0], ay = a[1], az = a[2];
  const double ux = (double)b[0] - ax, uy = (double)b[1] - ay, uz = (double)b[2] - az;
  const double vx = (double)c[0] - ax, vy = (double)c[1] - ay, vz = (double)c[2] - az;
  const double nx = uy * vz - uz * vy, ny = uz * vx - ux * vz, nz = ux * vy - uy * vx;
  Plane64 p;
  p.l2 = (nx * nx + ny * ny) + nz * nz;
  p.valid = rows_differ && p.l2 > 0.0 && p.l2 < INFINITY;
  const double len = sqrt(p.l2);
  p.n[0] = nx / len;
  p.n[1] = ny / len;
  p.n[2] = nz / len;
  return p;
}

// hyp: six rows of h_pad floats (ax ay az nx ny nz); rows [H][3]; valid [H]
__global__ __launch_bounds__(kThreads) void hypothesis_kernel(const float* __restrict__ xyz, uint64_t n, int H, int h_pad, uint64_t seed,
                                                              float* __restrict__ hyp, uint32_t* __restrict__ rows,
                                                              uint32_t* __restrict__ valid) {
  const int h = blockIdx.x * kThreads + threadIdx.x;
  if (h >= h_pad) return;
  float out[6] = {0.f, 0.f, 0.f, NAN, NAN, NAN};   // padding lanes of the count kernel: never an inlier, never stored
  if (h < H) {
    const uint32_t r0 = sample_row(seed, (uint64_t)h, 0, n), r1 = sample_row(seed, (uint64_t)h, 1, n), r2 = sample_row(seed, (uint64_t)h, 2, n);
    float a[3], b[3], c[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      a[k] = xyz[(size_t)r0 * 3 + k];
      b[k] = xyz[(size_t)r1 * 3 + k];
      c[k] = xyz[(size_t)r2 * 3 + k];
    }
    const Plane64 p = plane_of(a, b, c, r0 != r1 && r0 != r2 && r1 != r2);
    rows[3 * h] = r0;
    rows[3 * h + 1] = r1;
    rows[3 * h + 2] = r2;
    valid[h] = p.valid ? 1u : 0u;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      out[k] = a[k];
      if (p.valid) out[3 + k] = (float)p.n[k];
    }
  }
#pragma unroll
  for (int k = 0; k < 6; ++k) hyp[(size_t)k * h_pad + h] = out[k];
}

// the f32 inlier test of include/r3d.h: separate roundings of the three products and the two sums (-ffp-contract=off)
__device__ __forceinline__ bool inlier_f32(float px, float py, float pz, float ax, float ay, float az, float nx, float ny, float nz,
                                           float thr) {
  const float ex = px - ax, ey = py - ay, ez = pz - az;
  const float s = (nx * ex + ny * ey) + nz * ez;
  return fabsf(s) <= thr;
}

__device__ __forceinline__ float4 load_point(const float* __restrict__ xyz, int64_t i, int64_t end) {
  float4 q = make_float4(0.f, 0.f, 0.f, 0.f);
  if (i < end) {
    q.x = xyz[i * 3];
    q.y = xyz[i * 3 + 1];
    q.z = xyz[i * 3 + 2];
  }
  return q;
}

// blockIdx.x = chunk of chunk_points points (a multiple of kTile), blockIdx.y = block of kThreads * R hypotheses; lane t of the
// block owns hypotheses hb + t + r * kThreads.  partial [chunks][h_pad].
template <int R>
__global__ __launch_bounds__(kThreads) void count_kernel(const float* __restrict__ xyz, int64_t n, int64_t chunk_points,
                                                         const float* __restrict__ hyp, int h_pad, float thr,
                                                         uint32_t* __restrict__ partial) {
  __shared__ float4 tile[2][kTile];
  const int t = threadIdx.x;
  const int hb = blockIdx.y * (kThreads * R);
  float ax[R], ay[R], az[R], nx[R], ny[R], nz[R];
  uint32_t cnt[R];
#pragma unroll
  for (int r = 0; r < R; ++r) {
    const int h = hb + t + r * kThreads;   // < h_pad: h_pad is a multiple of kThreads * R
    ax[r] = hyp[h];
    ay[r] = hyp[(size_t)h_pad + h];
    az[r] = hyp[(size_t)2 * h_pad + h];
    nx[r] = hyp[(size_t)3 * h_pad + h];
    ny[r] = hyp[(size_t)4 * h_pad + h];
    nz[r] = hyp[(size_t)5 * h_pad + h];
    cnt[r] = 0;
  }
  const int64_t begin = (int64_t)blockIdx.x * chunk_points;
  const int64_t end = begin + chunk_points < n ? begin + chunk_points : n;
  float4 q0 = load_point(xyz, begin + t, end), q1 = load_point(xyz, begin + kThreads + t, end);
  int buf = 0;
  for (int64_t base = begin; base < end; base += kTile, buf ^= 1) {
    tile[buf][t] = q0;
    tile[buf][kThreads + t] = q1;
    __syncthreads();   // the other buffer was last read before the previous iteration's barrier
    const int64_t next = base + kTile;
    if (next < end) {
      q0 = load_point(xyz, next + t, end);
      q1 = load_point(xyz, next + kThreads + t, end);
    }
    const int m = (int)(end - base < kTile ? end - base : kTile);   // tail slots are not evaluated
    const float4* __restrict__ tp = tile[buf];
    int p = 0;
    for (; p + 4 <= m; p += 4) {
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        const float4 q = tp[p + u];
#pragma unroll
        for (int r = 0; r < R; ++r) cnt[r] += inlier_f32(q.x, q.y, q.z, ax[r], ay[r], az[r], nx[r], ny[r], nz[r], thr) ? 1u : 0u;
      }
    }
    for (; p < m; ++p) {
      const float4 q = tp[p];
#pragma unroll
      for (int r = 0; r < R; ++r) cnt[r] += inlier_f32(q.x, q.y, q.z, ax[r], ay[r], az[r], nx[r], ny[r], nz[r], thr) ? 1u : 0u;
    }
  }
#pragma unroll
  for (int r = 0; r < R; ++r) partial[(size_t)blockIdx.x * h_pad + hb + t + r * kThreads] = cnt[r];
}

struct NoTail {
  __device__ void operator()(Misc*, int, uint32_t) const {}
};

// grid-stride over the points: the best hypothesis' inliers and their sums about the anchor -> partial rows [gridDim.x][kSums]
__global__ __launch_bounds__(kThreads) void refit_kernel(const float* __restrict__ xyz, int64_t n, const float* __restrict__ hyp, int h_pad,
                                                         float thr, const Misc* __restrict__ misc, double* __restrict__ part) {
  const uint32_t h = misc->head.best_h;
  const float ax = hyp[h], ay = hyp[(size_t)h_pad + h], az = hyp[(size_t)2 * h_pad + h];
  const float nx = hyp[(size_t)3 * h_pad + h], ny = hyp[(size_t)4 * h_pad + h], nz = hyp[(size_t)5 * h_pad + h];
  double acc[kSums] = {};
  for (int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x; i < n; i += (int64_t)gridDim.x * kThreads) {
    const float px = xyz[i * 3], py = xyz[i * 3 + 1], pz = xyz[i * 3 + 2];
    if (inlier_f32(px, py, pz, ax, ay, az, nx, ny, nz, thr)) {
      const double ex = (double)px - (double)ax, ey = (double)py - (double)ay, ez = (double)pz - (double)az;
      acc[0] += 1.0;
      acc[1] += ex;
      acc[2] += ey;
      acc[3] += ez;
      acc[4] += ex * ex;
      acc[5] += ex * ey;
      acc[6] += ex * ez;
      acc[7] += ey * ey;
      acc[8] += ey * ez;
      acc[9] += ez * ez;
    }
  }
  __shared__ double red[kThreads / 64][kSums];
  r3d_sums::block_reduce_store<kSums>(acc, red, part + (size_t)blockIdx.x * kSums);
}

// one wave: lane k < kSums adds the rows' k-th entries in row order; lanes 16..24 fetch the best hypothesis' three points
__global__ __launch_bounds__(64) void refit_fold_kernel(const double* __restrict__ part, int n_rows, const float* __restrict__ xyz,
                                                        Misc* __restrict__ misc) {
  const int k = threadIdx.x;
  if (k < kSums) {
    double v = 0.0;
    for (int r = 0; r < n_rows; ++r) v += part[(size_t)r * kSums + k];
    misc->sums[k] = v;
  } else if (k >= 16 && k < 25) {
    const int j = (k - 16) / 3, a = (k - 16) % 3;
    misc->abc[3 * j + a] = xyz[(size_t)misc->head.rows[j] * 3 + a];
  }
}

struct Refined {
  double n[3], c[3], thr;
};

__global__ __launch_bounds__(kThreads) void mask_kernel(const float* __restrict__ xyz, int64_t n, const Refined pl,
                                                        uint8_t* __restrict__ inlier, unsigned long long* __restrict__ total) {
  uint32_t c = 0;
  for (int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x; i < n; i += (int64_t)gridDim.x * kThreads) {
    const double x = xyz[i * 3], y = xyz[i * 3 + 1], z = xyz[i * 3 + 2];
    const double t = (pl.n[0] * (x - pl.c[0]) + pl.n[1] * (y - pl.c[1])) + pl.n[2] * (z - pl.c[2]);
    const bool in = fabs(t) <= pl.thr;
    inlier[i] = in ? 1 : 0;
    c += in ? 1u : 0u;
  }
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) c += __shfl_down(c, off, 64);
  __shared__ uint32_t sh[kThreads / 64];
  if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = c;
  __syncthreads();
  if (threadIdx.x == 0) {
    const uint32_t s = sh[0] + sh[1] + sh[2] + sh[3];
    if (s) atomicAdd(total, (unsigned long long)s);
  }
}

// the component of largest magnitude is positive, the lowest axis winning ties
void orient(double n[3]) {
  int k = 0;
  if (std::fabs(n[1]) > std::fabs(n[k])) k = 1;
  if (std::fabs(n[2]) > std::fabs(n[k])) k = 2;
  if (n[k] < 0.0)
    for (int a = 0; a < 3; ++a) n[a] = -n[a];
}

template <int R>
void launch_count(hipStream_t st, int chunks, int h_pad, const float* xyz, int64_t n, int64_t chunk_points, const float* hyp, float thr,
                  uint32_t* partial) {
  hipLaunchKernelGGL((count_kernel<R>), dim3((unsigned)chunks, (unsigned)(h_pad / (kThreads * R))), dim3(kThreads), 0, st, xyz, n,
                     chunk_points, hyp, h_pad, thr, partial);
}

}  // namespace

extern "C" {

int r3d_ransac_rows(uint64_t seed, uint64_t h, int64_t n, uint32_t* rows) {
  R3D_REQUIRE(rows != nullptr, "rows is NULL");
  R3D_REQUIRE(n >= 1 && n < ((int64_t)1 << 32), "bad cloud size %lld", (long long)n);
  for (int j = 0; j < 3; ++j) rows[j] = sample_row(seed, h, j, (uint64_t)n);
  return R3D_OK;
}

int r3d_segment_plane(r3d_ctx* ctx, const float* d_xyz, int64_t n, double thr, int H, uint64_t seed, uint8_t* d_inlier_out,
                      uint32_t* d_counts_out, double* h_result, int64_t* n_inliers_out) {
  R3D_REQUIRE(ctx != nullptr, "ctx is NULL");
  R3D_REQUIRE(d_xyz && d_inlier_out && h_result && n_inliers_out, "NULL pointer");
  R3D_REQUIRE(n >= 3 && n < ((int64_t)1 << 32), "the cloud needs 3 <= n < 2^32 rows, got %lld", (long long)n);
  int rc = r3d_consensus::check_args(H, thr);
  if (rc) return rc;
  const size_t xb = (size_t)n * 12, cb = d_counts_out ? (size_t)H * 4 : 0;
  R3D_REQUIRE(!r3d_ranges_overlap(d_inlier_out, (size_t)n, d_xyz, xb) && !r3d_ranges_overlap(d_counts_out, cb, d_xyz, xb) &&
                  !r3d_ranges_overlap(d_counts_out, cb, d_inlier_out, (size_t)n),
              "an output overlaps the cloud or the other output");
  if ((rc = r3d_ctx_enter(ctx))) return rc;

  const r3d_consensus::Plan pn = r3d_consensus::plan(n, H, kTile);
  r3d_consensus::Layout lay;
  if ((rc = r3d_consensus::layout(ctx, pn, 6, kSums, sizeof(Misc), &lay))) return rc;
  Misc* misc = static_cast<Misc*>(lay.misc);
  const int h_pad = pn.h_pad, rblocks = pn.rblocks;

  r3d_wrote(ctx, d_inlier_out, (size_t)n);
  if (d_counts_out) r3d_wrote(ctx, d_counts_out, cb);
  hipStream_t st = ctx->stream;
  const float thr_f = (float)thr;
  R3D_HIP(hipMemsetAsync(misc, 0, sizeof(Misc), st));
  hipLaunchKernelGGL(hypothesis_kernel, dim3((unsigned)(h_pad / kThreads)), dim3(kThreads), 0, st, d_xyz, (uint64_t)n, H, h_pad, seed, lay.hyp,
                     lay.rows, lay.valid);
  if (pn.R == 4) launch_count<4>(st, pn.chunks, h_pad, d_xyz, n, pn.chunk_items, lay.hyp, thr_f, lay.partial);
  else if (pn.R == 2) launch_count<2>(st, pn.chunks, h_pad, d_xyz, n, pn.chunk_items, lay.hyp, thr_f, lay.partial);
  else launch_count<1>(st, pn.chunks, h_pad, d_xyz, n, pn.chunk_items, lay.hyp, thr_f, lay.partial);
  hipLaunchKernelGGL(r3d_consensus::fold_kernel, dim3((unsigned)((H + kThreads - 1) / kThreads)), dim3(kThreads), 0, st,
                     (const uint32_t*)lay.partial, pn.chunks, h_pad, H, (const uint32_t*)lay.valid, lay.counts, d_counts_out);
  hipLaunchKernelGGL((r3d_consensus::best_kernel<Misc, NoTail>), dim3(1), dim3(kThreads), 0, st, (const uint32_t*)lay.counts,
                     (const uint32_t*)lay.valid, (const uint32_t*)lay.rows, H, NoTail(), misc);
  hipLaunchKernelGGL(refit_kernel, dim3((unsigned)rblocks), dim3(kThreads), 0, st, d_xyz, n, (const float*)lay.hyp, h_pad, thr_f,
                     (const Misc*)misc, lay.part);
  hipLaunchKernelGGL(refit_fold_kernel, dim3(1), dim3(64), 0, st, (const double*)lay.part, rblocks, d_xyz, misc);
  R3D_HIP(hipGetLastError());
  Misc m;
  R3D_HIP(hipMemcpyAsync(&m, misc, sizeof(Misc), hipMemcpyDeviceToHost, st));
  R3D_HIP(hipStreamSynchronize(st));

  double res[16];
  for (int k = 0; k < 10; ++k) res[k] = NAN;
  res[10] = m.head.best_h;
  res[11] = m.head.c_best;
  for (int j = 0; j < 3; ++j) res[12 + j] = m.head.rows[j];
  res[15] = m.head.n_valid;
  if (m.head.c_best < 3) {
    R3D_HIP(hipMemsetAsync(d_inlier_out, 0, (size_t)n, st));
    R3D_HIP(hipStreamSynchronize(st));
    memcpy(h_result, res, sizeof(res));
    *n_inliers_out = 0;
    return R3D_OK;
  }
  const double* s = m.sums;
  const double cnt = s[0];
  Refined pl;
  double C[6], l[3];
  for (int a = 0; a < 3; ++a) pl.c[a] = (double)m.abc[a] + s[1 + a] / cnt;
  {
    int k = 0;
    for (int a = 0; a < 3; ++a)
      for (int b = a; b < 3; ++b, ++k) C[k] = (s[4 + k] - s[1 + a] * s[1 + b] / cnt) / cnt;
  }
  r3d_sym3::sym3_smallest(C, l, pl.n);
  if (!(l[1] > 0.0)) {   // collinear inliers: the hypothesis' own plane through a
    const Plane64 hp = plane_of(m.abc, m.abc + 3, m.abc + 6, true);
    for (int a = 0; a < 3; ++a) {
      pl.n[a] = hp.n[a];
      pl.c[a] = (double)m.abc[a];
    }
  }
  orient(pl.n);
  pl.thr = thr;
  for (int a = 0; a < 3; ++a) {
    res[a] = pl.n[a];
    res[4 + a] = pl.c[a];
    res[7 + a] = l[a];
  }
  res[3] = -((pl.n[0] * pl.c[0] + pl.n[1] * pl.c[1]) + pl.n[2] * pl.c[2]);
  hipLaunchKernelGGL(mask_kernel, dim3((unsigned)rblocks), dim3(kThreads), 0, st, d_xyz, n, pl, d_inlier_out, &misc->n_inliers);
  R3D_HIP(hipGetLastError());
  unsigned long long total = 0;
  R3D_HIP(hipMemcpyAsync(&total, &misc->n_inliers, sizeof(total), hipMemcpyDeviceToHost, st));
  R3D_HIP(hipStreamSynchronize(st));
  memcpy(h_result, res, sizeof(res));
  *n_inliers_out = (int64_t)total;
  return R3D_OK;
}

}  // extern "C"
