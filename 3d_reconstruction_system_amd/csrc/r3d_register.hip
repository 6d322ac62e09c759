// Global registration for gfx950 (MI355X): the mutual filter over nearest feature rows and RANSAC over correspondences.
//
// NOT IN THE REFERENCE (users of this kind of pipeline call Open3D's registration_ransac_based_on_feature_matching in front of
// ICP; no parity with Open3D is claimed).  Semantics: include/r3d.h (r3d_feature_match, r3d_register_ransac) and DESIGN.md
// section 4.5r.
//
//   r3d_feature_match    the nearest-row search of r3d_fpfh.hip in one or both directions, then
//     keep_count_kernel  per workgroup of 256 source rows, how many pass the filter
//     (scan)             r3d_compact_dev.h's, over that one row of counts: exclusive prefixes and the total
//     keep_write_kernel  the kept rows in ascending order: ballot ranks inside a wave, the waves in order (one row per thread)
//   r3d_register_ransac
//     pair_kernel        gathers the m correspondences into two float4 per pair (source point, target point); a row number
//                        outside its cloud gives NaN points, which are nobody's inlier and make a hypothesis invalid
//     pose_kernel        one lane per hypothesis: the counter-based sampler, the closed-form fp64 pose from three pairs,
//                        validity; R^ and t^ as twelve SoA floats (NaN when invalid: every test compares false)
//     count_kernel<R>    the hot path, the shape of r3d_ransac.hip's: lanes own R hypotheses in registers with one u32 count
//                        apiece, the workgroup's chunk of pairs goes through LDS in tiles and every lane reads the SAME pair
//                        (two broadcast ds_read_b128 per 64 R tests); partial counts [chunk][h], plain stores, no atomics
//     fold / best        r3d_consensus_dev.h's, as are the sampler, the launch plan and the scratch layout: integer sums over
//                        the chunks; the lowest h of maximal count, the number of valid hypotheses; FetchPairs, best's tail
//                        here, also fetches the winner's three pairs
//     refit_kernel       the best pose's inliers by the same f32 test -> the 18 fp64 pair sums about the anchors, one row per
//                        workgroup, folded by one workgroup in fixed order (r3d_sums_dev.h)
//     mask_kernel        the final f32 test with the refitted pose; inlier count and sum of squared distances through the same
//                        fixed-order reduction
// The Umeyama solve (no scale) runs on the host between refit and mask: r3d_icp_sums.h, the code of r3d_umeyama_from_sums.
#include <algorithm>
#include <cmath>

#include "r3d_compact_dev.h"
#include "r3d_consensus_dev.h"
#include "r3d_icp_sums.h"
#include "r3d_internal.h"
#include "r3d_sums_dev.h"

namespace {

using r3d_consensus::kThreads;
using r3d_consensus::sample_row;
constexpr int kDim = R3D_FPFH_DIM;
constexpr uint32_t kNone = 0xffffffffu;

// ---- the mutual filter and its compaction ---------------------------------------------------------------------------------------
__device__ __forceinline__ bool kept(const uint32_t* __restrict__ idx_a, const uint32_t* __restrict__ idx_b, int64_t na, int64_t nb,
                                     int64_t i) {
  if (i >= na) return false;
  const uint32_t j = idx_a[i];
  if (j == kNone || (int64_t)j >= nb) return false;
  return idx_b == nullptr || idx_b[j] == (uint32_t)i;
}

__global__ __launch_bounds__(kThreads) void keep_count_kernel(const uint32_t* __restrict__ idx_a, const uint32_t* __restrict__ idx_b,
                                                              int64_t na, int64_t nb, uint32_t* __restrict__ block_counts) {
  const int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x;
  __shared__ uint32_t sh[kThreads / 64];
  r3d_compact::publish(block_counts, r3d_compact::block_sum<uint32_t>(kept(idx_a, idx_b, na, nb, i), sh));
}

__global__ __launch_bounds__(kThreads) void keep_write_kernel(const uint32_t* __restrict__ idx_a, const uint32_t* __restrict__ idx_b,
                                                              int64_t na, int64_t nb, const uint32_t* __restrict__ block_starts,
                                                              uint32_t* __restrict__ corr) {
  const int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x;
  const bool k = kept(idx_a, idx_b, na, nb, i);
  const unsigned long long mask = __ballot(k);
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  __shared__ uint32_t sh[kThreads / 64];
  if (lane == 0) sh[wave] = (uint32_t)__popcll(mask);
  __syncthreads();
  if (!k) return;
  uint32_t at = block_starts[blockIdx.x] + (uint32_t)__popcll(mask & ((1ull << lane) - 1ull));
  for (int w = 0; w < wave; ++w) at += sh[w];
  corr[2 * (size_t)at] = (uint32_t)i;
  corr[2 * (size_t)at + 1] = idx_a[i];
}

// ---- RANSAC over correspondences --------------------------------------------------------------------------------------------------
constexpr int kTile = 256;              // pairs per LDS tile: one per thread, 8 KiB as two float4, two buffers
constexpr int kSums = r3d_icp::kSums;   // 18
constexpr int kMaskSums = 2;            // inliers, sum of their squared distances

struct Misc {
  r3d_consensus::BestHead head;
  float pts[24];          // the best hypothesis' three pairs as gathered: source xyz_, target xyz_ each
  double sums[kSums];
  double mask_sums[kMaskSums];
};

__global__ __launch_bounds__(kThreads) void pair_kernel(const float* __restrict__ src, int64_t ns, const float* __restrict__ tgt, int64_t nt,
                                                        const uint32_t* __restrict__ corr, int64_t m, float4* __restrict__ pairs) {
  const int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x;
  if (i >= m) return;
  const uint32_t a = corr[2 * i], b = corr[2 * i + 1];
  float4 p = make_float4(NAN, NAN, NAN, 0.f), q = p;
  if ((int64_t)a < ns) p = make_float4(src[(int64_t)a * 3], src[(int64_t)a * 3 + 1], src[(int64_t)a * 3 + 2], 0.f);
  if ((int64_t)b < nt) q = make_float4(tgt[(int64_t)b * 3], tgt[(int64_t)b * 3 + 1], tgt[(int64_t)b * 3 + 2], 0.f);
  pairs[2 * i] = p;
  pairs[2 * i + 1] = q;
}

struct Frame64 {
  double e1[3], e2[3], e3[3], len[3];   // len: |b - a|, |c - a|, |c - b|
  bool ok;
};

__host__ __device__ __forceinline__ double sq3(const double v[3]) { return (v[0] * v[0] + v[1] * v[1]) + v[2] * v[2]; }

// e1 = (b - a) / |b - a|, e3 = N / |N| with N = (b - a) x (c - a), e2 = e3 x e1; fp64 as written
__host__ __device__ __forceinline__ Frame64 frame_of(const float* a, const float* b, const float* c) {
  double u[3], v[3], w[3], N[3];
  for (int k = 0; k < 3; ++k) {
    u[k] = (double)b[k] - (double)a[k];
    v[k] = (double)c[k] - (double)a[k];
    w[k] = (double)c[k] - (double)b[k];
  }
  N[0] = u[1] * v[2] - u[2] * v[1];
  N[1] = u[2] * v[0] - u[0] * v[2];
  N[2] = u[0] * v[1] - u[1] * v[0];
  const double lu2 = sq3(u), ln2 = sq3(N);
  Frame64 f;
  f.ok = lu2 > 0.0 && lu2 < INFINITY && ln2 > 0.0 && ln2 < INFINITY;
  const double lu = sqrt(lu2), ln = sqrt(ln2);
  for (int k = 0; k < 3; ++k) {
    f.e1[k] = u[k] / lu;
    f.e3[k] = N[k] / ln;
  }
  f.e2[0] = f.e3[1] * f.e1[2] - f.e3[2] * f.e1[1];
  f.e2[1] = f.e3[2] * f.e1[0] - f.e3[0] * f.e1[2];
  f.e2[2] = f.e3[0] * f.e1[1] - f.e3[1] * f.e1[0];
  f.len[0] = lu;
  f.len[1] = sqrt(sq3(v));
  f.len[2] = sqrt(sq3(w));
  return f;
}

// pts: three pairs of (source xyz_, target xyz_) floats.  Rt[12] = R row-major, then t.  Returns the geometric validity.
__host__ __device__ __forceinline__ bool pose_of(const float* pts, double thr, double Rt[12]) {
  const Frame64 s = frame_of(pts, pts + 8, pts + 16), d = frame_of(pts + 4, pts + 12, pts + 20);
  bool ok = s.ok && d.ok;
  for (int k = 0; k < 3; ++k) ok = ok && fabs(s.len[k] - d.len[k]) <= 2.0 * thr;
  for (int r = 0; r < 3; ++r) {
    for (int c = 0; c < 3; ++c) Rt[3 * r + c] = (d.e1[r] * s.e1[c] + d.e2[r] * s.e2[c]) + d.e3[r] * s.e3[c];
    Rt[9 + r] = (double)pts[4 + r] - ((Rt[3 * r] * (double)pts[0] + Rt[3 * r + 1] * (double)pts[1]) + Rt[3 * r + 2] * (double)pts[2]);
  }
  return ok;
}

// hyp: twelve rows of h_pad floats (R row-major, t); rows [H][3]; valid [H]
__global__ __launch_bounds__(kThreads) void pose_kernel(const float4* __restrict__ pairs, const uint32_t* __restrict__ corr, uint64_t m,
                                                        double thr, int H, int h_pad, uint64_t seed, float* __restrict__ hyp,
                                                        uint32_t* __restrict__ rows, uint32_t* __restrict__ valid) {
  const int h = blockIdx.x * kThreads + threadIdx.x;
  if (h >= h_pad) return;
  float out[12];
#pragma unroll
  for (int k = 0; k < 12; ++k) out[k] = NAN;
  if (h < H) {
    uint32_t r[3];
    float pts[24];
    uint32_t cs[3], ct[3];
#pragma unroll
    for (int j = 0; j < 3; ++j) {
      r[j] = sample_row(seed, (uint64_t)h, j, m);
      const float4 p = pairs[2 * (size_t)r[j]], q = pairs[2 * (size_t)r[j] + 1];
      pts[8 * j] = p.x, pts[8 * j + 1] = p.y, pts[8 * j + 2] = p.z, pts[8 * j + 3] = 0.f;
      pts[8 * j + 4] = q.x, pts[8 * j + 5] = q.y, pts[8 * j + 6] = q.z, pts[8 * j + 7] = 0.f;
      cs[j] = corr[2 * (size_t)r[j]];
      ct[j] = corr[2 * (size_t)r[j] + 1];
      rows[3 * h + j] = r[j];
    }
    const bool differ = cs[0] != cs[1] && cs[0] != cs[2] && cs[1] != cs[2] && ct[0] != ct[1] && ct[0] != ct[2] && ct[1] != ct[2];
    double Rt[12];
    const bool ok = pose_of(pts, thr, Rt) && differ;
    valid[h] = ok ? 1u : 0u;
    if (ok) {
#pragma unroll
      for (int k = 0; k < 12; ++k) out[k] = (float)Rt[k];
    }
  }
#pragma unroll
  for (int k = 0; k < 12; ++k) hyp[(size_t)k * h_pad + h] = out[k];
}

// the squared f32 distance of include/r3d.h's test: an inlier iff it is <= thr2 (NaN compares false)
__device__ __forceinline__ float dist2_f32(const float4 p, const float4 q, const float* __restrict__ P) {
  const float x = ((P[0] * p.x + P[1] * p.y) + P[2] * p.z) + P[9];
  const float y = ((P[3] * p.x + P[4] * p.y) + P[5] * p.z) + P[10];
  const float z = ((P[6] * p.x + P[7] * p.y) + P[8] * p.z) + P[11];
  const float ex = x - q.x, ey = y - q.y, ez = z - q.z;
  return (ex * ex + ey * ey) + ez * ez;
}

// blockIdx.x = chunk of chunk_pairs pairs (a multiple of kTile), blockIdx.y = block of kThreads * R hypotheses
template <int R>
__global__ __launch_bounds__(kThreads) void count_kernel(const float4* __restrict__ pairs, int64_t m, int64_t chunk_pairs,
                                                         const float* __restrict__ hyp, int h_pad, float thr2,
                                                         uint32_t* __restrict__ partial) {
  __shared__ float4 tile[2][2 * kTile];
  const int t = threadIdx.x;
  const int hb = blockIdx.y * (kThreads * R);
  float P[R][12];
  uint32_t cnt[R];
#pragma unroll
  for (int r = 0; r < R; ++r) {
    const int h = hb + t + r * kThreads;   // < h_pad: h_pad is a multiple of kThreads * R
#pragma unroll
    for (int k = 0; k < 12; ++k) P[r][k] = hyp[(size_t)k * h_pad + h];
    cnt[r] = 0;
  }
  const int64_t begin = (int64_t)blockIdx.x * chunk_pairs;
  const int64_t end = begin + chunk_pairs < m ? begin + chunk_pairs : m;
  const float4 none = make_float4(NAN, NAN, NAN, 0.f);
  float4 p0 = none, q0 = none;
  if (begin + t < end) {
    p0 = pairs[2 * (begin + t)];
    q0 = pairs[2 * (begin + t) + 1];
  }
  int buf = 0;
  for (int64_t base = begin; base < end; base += kTile, buf ^= 1) {
    tile[buf][2 * t] = p0;
    tile[buf][2 * t + 1] = q0;
    __syncthreads();   // the other buffer was last read before the previous iteration's barrier
    const int64_t next = base + kTile + t;
    if (next < end) {
      p0 = pairs[2 * next];
      q0 = pairs[2 * next + 1];
    }
    const int mt = (int)(end - base < kTile ? end - base : kTile);   // tail slots are not evaluated
    const float4* __restrict__ tp = tile[buf];
    for (int p = 0; p < mt; ++p) {
      const float4 a = tp[2 * p], b = tp[2 * p + 1];
#pragma unroll
      for (int r = 0; r < R; ++r) cnt[r] += dist2_f32(a, b, P[r]) <= thr2 ? 1u : 0u;
    }
  }
#pragma unroll
  for (int r = 0; r < R; ++r) partial[(size_t)blockIdx.x * h_pad + hb + t + r * kThreads] = cnt[r];
}

// best_kernel's tail: the best hypothesis' three pairs as gathered
struct FetchPairs {
  const float4* __restrict__ pairs;
  __device__ void operator()(Misc* __restrict__ misc, int j, uint32_t r) const {
    const float4 p = pairs[2 * (size_t)r], q = pairs[2 * (size_t)r + 1];
    float* d = misc->pts + 8 * j;
    d[0] = p.x, d[1] = p.y, d[2] = p.z, d[3] = 0.f, d[4] = q.x, d[5] = q.y, d[6] = q.z, d[7] = 0.f;
  }
};

// grid-stride over the pairs: the best pose's inliers and their 18 sums about the anchors (the first pair of the hypothesis)
__global__ __launch_bounds__(kThreads) void refit_kernel(const float4* __restrict__ pairs, int64_t m, const float* __restrict__ hyp, int h_pad,
                                                         float thr2, const Misc* __restrict__ misc, double* __restrict__ part) {
  const uint32_t h = misc->head.best_h;
  float P[12];
#pragma unroll
  for (int k = 0; k < 12; ++k) P[k] = hyp[(size_t)k * h_pad + h];
  const double a[3] = {(double)misc->pts[0], (double)misc->pts[1], (double)misc->pts[2]};
  const double b[3] = {(double)misc->pts[4], (double)misc->pts[5], (double)misc->pts[6]};
  double acc[kSums];
#pragma unroll
  for (int k = 0; k < kSums; ++k) acc[k] = 0.0;
  for (int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x; i < m; i += (int64_t)gridDim.x * kThreads) {
    const float4 p = pairs[2 * i], q = pairs[2 * i + 1];
    if (dist2_f32(p, q, P) <= thr2) {
      const double pc[3] = {(double)p.x - a[0], (double)p.y - a[1], (double)p.z - a[2]};
      const double qc[3] = {(double)q.x - b[0], (double)q.y - b[1], (double)q.z - b[2]};
      r3d_icp::pair_accumulate(acc, 1.0, pc, qc);
    }
  }
  __shared__ double red[kThreads / 64][kSums];
  r3d_sums::block_reduce_store<kSums>(acc, red, part + (size_t)blockIdx.x * kSums);
}

struct NoSolve {
  __device__ int operator()(const double*, double*, double*) const { return 0; }
};

template <int K>
__global__ __launch_bounds__(kThreads) void finish_kernel(const double* __restrict__ part, int n_rows, double* __restrict__ sums_out) {
  r3d_sums::finish_rows<K>(part, n_rows, sums_out, nullptr, NoSolve());
}

struct Pose32 {
  float P[12];
};

__global__ __launch_bounds__(kThreads) void mask_kernel(const float4* __restrict__ pairs, int64_t m, const Pose32 pose, float thr2,
                                                        uint8_t* __restrict__ inlier, double* __restrict__ part) {
  double acc[kMaskSums] = {0.0, 0.0};
  for (int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x; i < m; i += (int64_t)gridDim.x * kThreads) {
    const float s2 = dist2_f32(pairs[2 * i], pairs[2 * i + 1], pose.P);
    const bool in = s2 <= thr2;
    inlier[i] = in ? 1 : 0;
    if (in) {
      acc[0] += 1.0;
      acc[1] += (double)s2;
    }
  }
  __shared__ double red[kThreads / 64][kMaskSums];
  r3d_sums::block_reduce_store<kMaskSums>(acc, red, part + (size_t)blockIdx.x * kMaskSums);
}

template <int R>
void launch_count(hipStream_t st, int chunks, int h_pad, const float4* pairs, int64_t m, int64_t chunk_pairs, const float* hyp, float thr2,
                  uint32_t* partial) {
  hipLaunchKernelGGL((count_kernel<R>), dim3((unsigned)chunks, (unsigned)(h_pad / (kThreads * R))), dim3(kThreads), 0, st, pairs, m,
                     chunk_pairs, hyp, h_pad, thr2, partial);
}

}  // namespace

extern "C" {

int r3d_feature_match(r3d_ctx* ctx, const float* d_a, int64_t na, const float* d_b, int64_t nb, int mutual, uint32_t* d_idx_out,
                      float* d_dist_out, uint32_t* d_corr_out, int64_t* h_m_out) {
  R3D_REQUIRE(ctx != nullptr, "ctx is NULL");
  R3D_REQUIRE(d_a && d_b && d_idx_out, "NULL pointer");
  R3D_REQUIRE(na >= 1 && na < ((int64_t)1 << 32) && nb >= 1 && nb < ((int64_t)1 << 32), "feature sets need 1 <= rows < 2^32, got %lld, %lld",
              (long long)na, (long long)nb);
  R3D_REQUIRE(mutual == 0 || mutual == 1, "mutual must be 0 or 1, got %d", mutual);
  R3D_REQUIRE((d_corr_out == nullptr) == (h_m_out == nullptr), "d_corr_out and h_m_out go together");
  R3D_REQUIRE(d_corr_out != nullptr || mutual == 0, "mutual = 1 needs d_corr_out");
  const size_t ab = (size_t)na * kDim * 4, bb = (size_t)nb * kDim * 4;
  const struct {
    const void* p;
    size_t bytes;
  } out[3] = {{d_idx_out, (size_t)na * 4}, {d_dist_out, (size_t)na * 4}, {d_corr_out, (size_t)na * 8}};
  for (int i = 0; i < 3; ++i) {
    R3D_REQUIRE(!r3d_ranges_overlap(out[i].p, out[i].bytes, d_a, ab) && !r3d_ranges_overlap(out[i].p, out[i].bytes, d_b, bb),
                "an output overlaps a feature set");
    for (int j = i + 1; j < 3; ++j) R3D_REQUIRE(!r3d_ranges_overlap(out[i].p, out[i].bytes, out[j].p, out[j].bytes), "outputs overlap each other");
  }
  int rc = r3d_ctx_enter(ctx);
  if (rc) return rc;
  // kWsPartials / kWsSpare: the partial minima of a -> b / b -> a; kWsCounts: the b -> a rows; kWsMisc: the per-workgroup keep counts
  const int n_blocks = (int)((na + kThreads - 1) / kThreads);
  r3d_compact::Counters cn(n_blocks, 1);
  void *idx_b_v = nullptr, *counts_v = nullptr;
  if (mutual && (rc = r3d_scratch(ctx, kWsCounts, (size_t)nb * 4, &idx_b_v))) return rc;
  if (d_corr_out && (rc = r3d_scratch(ctx, kWsMisc, cn.bytes, &counts_v))) return rc;
  for (int i = 0; i < 3; ++i)
    if (out[i].p) r3d_wrote(ctx, out[i].p, out[i].bytes);
  if ((rc = r3d_match_nearest(ctx, d_a, na, d_b, nb, d_idx_out, d_dist_out, kWsPartials))) return rc;
  if (!d_corr_out) return R3D_OK;
  uint32_t* idx_b = static_cast<uint32_t*>(idx_b_v);
  if (mutual && (rc = r3d_match_nearest(ctx, d_b, nb, d_a, na, idx_b, nullptr, kWsSpare))) return rc;
  cn.place(counts_v);
  hipStream_t st = ctx->stream;
  hipLaunchKernelGGL(keep_count_kernel, dim3((unsigned)n_blocks), dim3(kThreads), 0, st, (const uint32_t*)d_idx_out, (const uint32_t*)idx_b,
                     na, nb, cn.hist);
  r3d_compact::launch_scan(ctx, cn);
  hipLaunchKernelGGL(keep_write_kernel, dim3((unsigned)n_blocks), dim3(kThreads), 0, st, (const uint32_t*)d_idx_out,
                     (const uint32_t*)idx_b, na, nb, (const uint32_t*)cn.hist, d_corr_out);
  uint32_t total = 0;
  if ((rc = r3d_compact::read_totals(ctx, cn, &total, 1))) return rc;
  *h_m_out = (int64_t)total;
  return R3D_OK;
}

int r3d_register_ransac(r3d_ctx* ctx, const float* d_src, int64_t ns, const float* d_tgt, int64_t nt, const uint32_t* d_corr, int64_t m,
                        double thr, int H, uint64_t seed, uint8_t* d_inlier_out, uint32_t* d_counts_out, double* h_result) {
  R3D_REQUIRE(ctx != nullptr, "ctx is NULL");
  R3D_REQUIRE(d_src && d_tgt && d_corr && d_inlier_out && h_result, "NULL pointer");
  R3D_REQUIRE(ns >= 1 && ns < ((int64_t)1 << 32) && nt >= 1 && nt < ((int64_t)1 << 32), "the clouds need 1 <= n < 2^32 rows, got %lld, %lld",
              (long long)ns, (long long)nt);
  R3D_REQUIRE(m >= 3 && m < ((int64_t)1 << 32), "need 3 <= m < 2^32 correspondences, got %lld", (long long)m);
  int rc = r3d_consensus::check_args(H, thr);
  if (rc) return rc;
  const size_t cb = d_counts_out ? (size_t)H * 4 : 0;
  const struct {
    const void* p;
    size_t bytes;
  } in[3] = {{d_src, (size_t)ns * 12}, {d_tgt, (size_t)nt * 12}, {d_corr, (size_t)m * 8}};
  for (int i = 0; i < 3; ++i)
    R3D_REQUIRE(!r3d_ranges_overlap(d_inlier_out, (size_t)m, in[i].p, in[i].bytes) && !r3d_ranges_overlap(d_counts_out, cb, in[i].p, in[i].bytes),
                "an output overlaps an input");
  R3D_REQUIRE(!r3d_ranges_overlap(d_counts_out, cb, d_inlier_out, (size_t)m), "the outputs overlap each other");
  if ((rc = r3d_ctx_enter(ctx))) return rc;

  // kWsIn: the gathered pairs; kWsMisc and kWsPartials: the consensus layout
  const r3d_consensus::Plan pn = r3d_consensus::plan(m, H, kTile);
  void* s0 = nullptr;
  if ((rc = r3d_scratch(ctx, kWsIn, (size_t)m * 32, &s0))) return rc;
  r3d_consensus::Layout lay;
  if ((rc = r3d_consensus::layout(ctx, pn, 12, kSums, sizeof(Misc), &lay))) return rc;
  float4* pairs = static_cast<float4*>(s0);
  Misc* misc = static_cast<Misc*>(lay.misc);
  double* part = lay.part;
  const int h_pad = pn.h_pad, rblocks = pn.rblocks;

  r3d_wrote(ctx, d_inlier_out, (size_t)m);
  if (d_counts_out) r3d_wrote(ctx, d_counts_out, cb);
  hipStream_t st = ctx->stream;
  const float thr2 = (float)(thr * thr);
  R3D_HIP(hipMemsetAsync(misc, 0, sizeof(Misc), st));
  hipLaunchKernelGGL(pair_kernel, dim3((unsigned)((m + kThreads - 1) / kThreads)), dim3(kThreads), 0, st, d_src, ns, d_tgt, nt, d_corr, m,
                     pairs);
  hipLaunchKernelGGL(pose_kernel, dim3((unsigned)(h_pad / kThreads)), dim3(kThreads), 0, st, (const float4*)pairs, d_corr, (uint64_t)m, thr,
                     H, h_pad, seed, lay.hyp, lay.rows, lay.valid);
  if (pn.R == 4) launch_count<4>(st, pn.chunks, h_pad, pairs, m, pn.chunk_items, lay.hyp, thr2, lay.partial);
  else if (pn.R == 2) launch_count<2>(st, pn.chunks, h_pad, pairs, m, pn.chunk_items, lay.hyp, thr2, lay.partial);
  else launch_count<1>(st, pn.chunks, h_pad, pairs, m, pn.chunk_items, lay.hyp, thr2, lay.partial);
  hipLaunchKernelGGL(r3d_consensus::fold_kernel, dim3((unsigned)((H + kThreads - 1) / kThreads)), dim3(kThreads), 0, st,
                     (const uint32_t*)lay.partial, pn.chunks, h_pad, H, (const uint32_t*)lay.valid, lay.counts, d_counts_out);
  hipLaunchKernelGGL((r3d_consensus::best_kernel<Misc, FetchPairs>), dim3(1), dim3(kThreads), 0, st, (const uint32_t*)lay.counts,
                     (const uint32_t*)lay.valid, (const uint32_t*)lay.rows, H, FetchPairs{pairs}, misc);
  hipLaunchKernelGGL(refit_kernel, dim3((unsigned)rblocks), dim3(kThreads), 0, st, (const float4*)pairs, m, (const float*)lay.hyp, h_pad, thr2,
                     (const Misc*)misc, part);
  hipLaunchKernelGGL((finish_kernel<kSums>), dim3(1), dim3(kThreads), 0, st, (const double*)part, rblocks, misc->sums);
  R3D_HIP(hipGetLastError());
  Misc mi;
  R3D_HIP(hipMemcpyAsync(&mi, misc, sizeof(Misc), hipMemcpyDeviceToHost, st));
  R3D_HIP(hipStreamSynchronize(st));

  double res[R3D_REGISTER_RESULT_DOUBLES];
  for (int k = 0; k < R3D_REGISTER_RESULT_DOUBLES; ++k) res[k] = 0.0;
  for (int k = 0; k < 16; ++k) res[k] = NAN;
  res[16] = mi.head.best_h;
  res[17] = mi.head.c_best;
  for (int j = 0; j < 3; ++j) res[18 + j] = mi.head.rows[j];
  res[21] = mi.head.n_valid;
  res[23] = NAN;
  if (mi.head.c_best < 3) {
    R3D_HIP(hipMemsetAsync(d_inlier_out, 0, (size_t)m, st));
    R3D_HIP(hipStreamSynchronize(st));
    memcpy(h_result, res, sizeof(res));
    return R3D_OK;
  }
  // the hypothesis' own fp64 pose, then the refit about the anchors a (source) and a' (target): T = [R, a' + t_c - R a]
  double Rt[12], Tc[16];
  pose_of(mi.pts, thr, Rt);
  const int degenerate = r3d_icp::umeyama_from_sums(mi.sums, 0, Tc, nullptr);
  if (!degenerate) {
    for (int r = 0; r < 3; ++r) {
      for (int c = 0; c < 3; ++c) Rt[3 * r + c] = Tc[4 * r + c];
      Rt[9 + r] = ((double)mi.pts[4 + r] + Tc[4 * r + 3]) -
                  ((Rt[3 * r] * (double)mi.pts[0] + Rt[3 * r + 1] * (double)mi.pts[1]) + Rt[3 * r + 2] * (double)mi.pts[2]);
    }
  }
  Pose32 pose;
  for (int k = 0; k < 12; ++k) pose.P[k] = (float)Rt[k];
  hipLaunchKernelGGL(mask_kernel, dim3((unsigned)rblocks), dim3(kThreads), 0, st, (const float4*)pairs, m, pose, thr2, d_inlier_out, part);
  hipLaunchKernelGGL((finish_kernel<kMaskSums>), dim3(1), dim3(kThreads), 0, st, (const double*)part, rblocks, misc->mask_sums);
  R3D_HIP(hipGetLastError());
  double ms[kMaskSums];
  R3D_HIP(hipMemcpyAsync(ms, misc->mask_sums, sizeof(ms), hipMemcpyDeviceToHost, st));
  R3D_HIP(hipStreamSynchronize(st));
  for (int r = 0; r < 3; ++r) {
    for (int c = 0; c < 3; ++c) res[4 * r + c] = Rt[3 * r + c];
    res[4 * r + 3] = Rt[9 + r];
  }
  res[12] = res[13] = res[14] = 0.0;
  res[15] = 1.0;
  res[22] = ms[0];
  res[23] = ms[0] > 0.0 ? std::sqrt(ms[1] / ms[0]) : NAN;
  res[24] = degenerate ? 1.0 : 0.0;
  memcpy(h_result, res, sizeof(res));
  return R3D_OK;
}

}  // extern "C"
