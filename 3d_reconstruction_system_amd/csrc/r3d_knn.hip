// k nearest neighbours of an index's own points, and the outlier filters built on them, for gfx950 (MI355X).
//
// NOT IN THE REFERENCE (it pins Open3D, whose remove_statistical_outlier / remove_radius_outlier users reach for after
// fusion; no parity with Open3D is claimed).  Semantics: include/r3d.h and DESIGN.md section 4.5e.
//
//   knn_kernel<MODE, K>   one lane per point of the index, the sources being the index's own sorted tgt4 (w = original row):
//       a workgroup's 256 points are a quarter of one tile, spatially compact without a sort.  The walk is nn_cull_kernel's:
//       super-boxes outward from the workgroup's own tile, then tiles, 256-target quarters and 32-target groups, each skipped
//       when no lane can still gain inside its box.  The bound is the lane's current k-th entry (+inf until the list is full).
//         kList   exact (d2, j) lists: K slots of 64-bit keys (d2 bits << 32 | j) in registers, compile-time indices only; a
//                 box is skipped only when lb > k-th d2 (an equal distance with a lower j could still enter).
//         kScore  the statistical filter's m_i: K + 1 slots of d2 alone, self included (its d2 is 0, the smallest value, so the
//                 k + 1 smallest of "self + others" are 0 + the k smallest of the others, whether or not self is met).  Equal
//                 distances do not enter and a box is skipped when lb >= k-th: a cluster of D identical points costs O(D k)
//                 instead of O(D^2).  Writes m_i and one (sum m, V) row per workgroup; the lists never leave registers.
//         kRadius no list: the count of d2 <= r2, self included; the bound is r2 and the workgroup stops once every lane has
//                 min_points + 1.
//         kNormals kList's search unchanged; the epilogue walks the slots in order, gathers each neighbour from the original-order
//                 cloud, accumulates the nine fp64 sums about the query point, solves the 3x3 covariance for its smallest
//                 eigenvector (cyclic Jacobi, fp64: r3d_sym3.h) and orients it: 12 to 44 bytes per point leave, the lists never do.
//       Unused front slots hold a sentinel below every real entry, so the last slot is always the k-th real one.
//   sor_mean / sor_dev / sor_threshold / sor_keep: fixed-order fp64 reductions (one row per workgroup, one-wave folds) for
//       mu, sigma and T, then the mask -- no float atomics, the same bits on every run.
//   select_count / select_write: order-preserving row selection, the compaction step of r3d_compact_dev.h.
#include <algorithm>
#include <cmath>

#include "r3d_compact_dev.h"
#include "r3d_internal.h"
#include "r3d_magic_div.h"
#include "r3d_nnindex_dev.h"
#include "r3d_sums_dev.h"
#include "r3d_sym3.h"

namespace {

constexpr int kThreads = 256;
using r3d_nn::kGroup;
using r3d_nn::kShrink;
using r3d_nn::kSub;
using r3d_nn::kSuper;
using r3d_nn::kTile;
using r3d_nn::P3;

typedef float f32x2 __attribute__((ext_vector_type(2)));

enum Mode { kList = 0, kScore = 1, kRadius = 2, kNormals = 3 };

constexpr uint64_t kKeyTail = 0x7f80000000000000ull;  // key of (+inf, row 0): above every candidate, whose d2 is finite
constexpr int kReduceBlocks = 1024;                    // workgroups of the grid-stride passes (one row / atomic each)

struct KnnArgs {
  const float4* tgt4;
  int64_t n, n_tiles;
  const float *tile_box, *sub_box, *group_box, *super_box;
  int k;
  float r2;               // kRadius: candidates with d2 <= r2 count (FLT_MAX when radius^2 overflows: finite d2 only)
                          // kNormals: list entries with d2 <= r2 are members (+inf: no radius)
  uint64_t min_points;    // kRadius: min(min_points, n) -- nobody reaches more than n - 1
  uint32_t* idx_out;      // kList: [n][k]
  float* d2_out;          // kList: [n][k] or NULL
  double* score_out;      // kScore: [n] m_i
  double* partials;       // kScore: [blocks][2] (sum of finite m, V)
  uint8_t* keep_out;      // kRadius
  uint32_t* count_out;    // kRadius: min(c, min_points) or NULL; kNormals: c_i or NULL
  unsigned long long* n_kept;   // kRadius
  unsigned long long* groups;   // 32-target groups evaluated, summed over waves
  // kNormals (behind everything else: the other modes' kernel-argument offsets stay where they were)
  const float* tgt;       // [n][3] original order: the neighbour gathers
  float* nrm_out;         // [n][3]
  float* curv_out;        // [n] or NULL
  double* cov_out;        // [n][6] or NULL
  const double* views;    // [n_views][3] or NULL (orient by the largest component)
  uint32_t n_views, v_magic, v_shift;   // row i belongs to view min(i / points_per_view, n_views - 1): make_magic(points_per_view)
};

// strict lower bound of the squared distance from a point to a box (lo xyz at b[0..2], hi xyz at b[3..5]); an empty box
// (+inf, -inf) is infinitely far.  POINT_EXACT: a box of one point (lo == hi: identical copies) gets no shrink -- its
// ex, ey, ez are then |dx|, |dy|, |dz| and the bound IS every member's d2, bit for bit, so `lb >= k-th` can skip the copies
// that sit exactly at the k-th distance (a background point next to a cluster of identical points would otherwise evaluate
// every copy).
template <bool POINT_EXACT>
__device__ __forceinline__ float box_lb(float lx, float ly, float lz, float hx, float hy, float hz, float px, float py, float pz) {
  const float ex = fmaxf(fmaxf(lx - px, px - hx), 0.f);
  const float ey = fmaxf(fmaxf(ly - py, py - hy), 0.f);
  const float ez = fmaxf(fmaxf(lz - pz, pz - hz), 0.f);
  const float d = fmaf(ez, ez, fmaf(ey, ey, ex * ex));
  return POINT_EXACT && lx == hx && ly == hy && lz == hz ? d : d * kShrink;
}
template <bool POINT_EXACT>
__device__ __forceinline__ float box_lb(const float* __restrict__ b, float px, float py, float pz) {
  return box_lb<POINT_EXACT>(b[0], b[1], b[2], b[3], b[4], b[5], px, py, pz);
}

using r3d_sums::wave_sum;   // the fp64 shuffle tree every sums row of the library goes through

// the sum of one double per thread of a 256-thread workgroup, in a fixed order; valid in thread 0
__device__ __forceinline__ double block_sum_f64(double v, double* sh) {
  v = wave_sum(v);
  if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = v;
  __syncthreads();
  double t = 0.0;
  if (threadIdx.x == 0)
    for (int w = 0; w < kThreads / 64; ++w) t += sh[w];
  return t;
}

// ---- kNormals' epilogue ------------------------------------------------------------------------------------------------------
// The lane's point (row `me`, coordinates sx sy sz, act = all finite) and its finished list -> count, covariance, curvature
// and oriented normal (include/r3d.h: r3d_normals_knn).  A slot that is no member gathers the lane's own row instead: its
// e = 0 adds +0.0 to sums that are never -0.0, which changes no bit, and the K loads need no branch between them.
template <int K>
__device__ __forceinline__ void normals_epilogue(const KnnArgs& a, const uint64_t (&kl)[K], int front, bool act, uint32_t me,
                                                 float sx, float sy, float sz) {
  const P3* __restrict__ tgt = reinterpret_cast<const P3*>(a.tgt);
  const double px = (double)sx, py = (double)sy, pz = (double)sz;
  double s1x = 0.0, s1y = 0.0, s1z = 0.0, sxx = 0.0, sxy = 0.0, sxz = 0.0, syy = 0.0, syz = 0.0, szz = 0.0;
  uint32_t c = 0;
#pragma unroll
  for (int t = 0; t < K; ++t) {
    const uint64_t key = kl[t];
    const bool in = act && t >= front && key < kKeyTail && __uint_as_float((uint32_t)(key >> 32)) <= a.r2;
    const P3 q = tgt[in ? (uint32_t)key : me];
    c += in ? 1u : 0u;
    const double ex = in ? (double)q.x - px : 0.0, ey = in ? (double)q.y - py : 0.0, ez = in ? (double)q.z - pz : 0.0;
    s1x += ex;
    s1y += ey;
    s1z += ez;
    sxx += ex * ex;
    sxy += ex * ey;
    sxz += ex * ez;
    syy += ey * ey;
    syz += ey * ez;
    szz += ez * ez;
  }
  const double m = (double)(c + 1u);   // the point itself is a member with e = 0
  double C[6] = {(sxx - s1x * s1x / m) / m, (sxy - s1x * s1y / m) / m, (sxz - s1x * s1z / m) / m,
                 (syy - s1y * s1y / m) / m, (syz - s1y * s1z / m) / m, (szz - s1z * s1z / m) / m};
  double l[3] = {0.0, 0.0, 0.0}, nv[3] = {0.0, 0.0, 0.0};
  bool plane = act && c >= 2u;
  if (plane) {
    r3d_sym3::sym3_smallest(C, l, nv);
    plane = l[1] > 0.0;
  }
  float curv = 0.f;
  if (plane) {
    bool flip;
    if (a.views) {
      const uint32_t v = min(r3d_magic::magic_div(me, a.v_magic, a.v_shift), a.n_views - 1u);
      const double* __restrict__ vp = a.views + (size_t)v * 3;
      flip = nv[0] * (vp[0] - px) + nv[1] * (vp[1] - py) + nv[2] * (vp[2] - pz) < 0.0;
    } else {
      const double ax = fabs(nv[0]), ay = fabs(nv[1]), az = fabs(nv[2]);
      flip = (ax >= ay && ax >= az ? nv[0] : ay >= az ? nv[1] : nv[2]) < 0.0;
    }
    if (flip) nv[0] = -nv[0], nv[1] = -nv[1], nv[2] = -nv[2];
    const double l0 = fmax(l[0], 0.0), sum = l0 + l[1] + l[2];
    curv = sum > 0.0 ? (float)(l0 / sum) : 0.f;
  } else {
    nv[0] = nv[1] = nv[2] = 0.0;
#pragma unroll
    for (int e = 0; e < 6; ++e) C[e] = 0.0;
  }
  P3 out;
  out.x = (float)nv[0], out.y = (float)nv[1], out.z = (float)nv[2];
  reinterpret_cast<P3*>(a.nrm_out)[me] = out;
  if (a.curv_out) a.curv_out[me] = curv;
  if (a.count_out) a.count_out[me] = c;
  if (a.cov_out) {
#pragma unroll
    for (int e = 0; e < 6; ++e) a.cov_out[(size_t)me * 6 + e] = C[e];
  }
}

template <int MODE, int K>
__global__ __launch_bounds__(kThreads) void knn_kernel(const KnnArgs a) {
  constexpr bool LIST = MODE == kList || MODE == kNormals;               // exact (d2, j) lists in registers
  constexpr int NS = LIST ? K : MODE == kScore ? K + 1 : 1;   // list slots
  constexpr int kUnrollQ = MODE == kRadius ? kGroup / 4 : 1;
  __shared__ __attribute__((aligned(16))) float tx[kTile];
  __shared__ __attribute__((aligned(16))) float ty[kTile];
  __shared__ __attribute__((aligned(16))) float tz[kTile];
  __shared__ __attribute__((aligned(16))) uint32_t tw[LIST ? kTile : 4];
  __shared__ __attribute__((aligned(16))) float gbox[kTile / kGroup][8];  // lo xyz, hi xyz of every 32-target group (+ pad)

  const uint32_t tid = threadIdx.x;
  const int64_t p = (int64_t)blockIdx.x * kThreads + tid;   // this lane's point: sorted slot p of the index
  const bool ok = p < a.n;
  const float4 me4 = ok ? a.tgt4[p] : make_float4(0.f, 0.f, 0.f, 0.f);
  const float sx = me4.x, sy = me4.y, sz = me4.z;
  const uint32_t me = __float_as_uint(me4.w);
  // a point with a NaN / inf coordinate has no candidates: it takes no part in the walk or the votes
  const bool act = ok && (sx - sx == 0.f) && (sy - sy == 0.f) && (sz - sz == 0.f);

  float fl[MODE == kScore ? NS : 1];
  uint64_t kl[LIST ? NS : 1];
  uint32_t cnt = 0;
  const int front = K - a.k;   // sentinel slots in front of the k (kScore: k + 1) real ones
#pragma unroll
  for (int t = 0; t < NS; ++t) {
    if (MODE == kScore) fl[t] = t < front ? -1.f : INFINITY;
    if (LIST) kl[t] = t < front ? 0ull : kKeyTail;
  }
  (void)fl;
  (void)kl;
  (void)front;

  // may a box whose strict lower bound is lb still change this lane's answer?  (NaN bounds never allow a skip)
  auto wants = [&](float lb) -> bool {
    if (!act) return false;
    if (LIST) return !(lb > __uint_as_float((uint32_t)(kl[NS - 1] >> 32)));
    if (MODE == kScore) return !(lb >= fl[NS - 1]);
    return !(lb > a.r2) && (uint64_t)cnt <= a.min_points;   // cnt holds self: min_points + 1 reached = done
  };

  const int64_t t0 = (int64_t)blockIdx.x / (kTile / kThreads);
  unsigned groups_done = 0;
  const int64_t n_super = (a.n_tiles + kSuper - 1) / kSuper;
  const int64_t s0 = t0 / kSuper;
  for (int64_t sstep = 0; sstep < 2 * n_super; ++sstep) {
    const int64_t sup = (sstep & 1) ? s0 + ((sstep + 1) >> 1) : s0 - (sstep >> 1);
    if (sup < 0 || sup >= n_super) continue;  // uniform
    if (MODE == kRadius && !__syncthreads_or(act && (uint64_t)cnt <= a.min_points)) break;   // every lane has its count
    if (!__syncthreads_or(wants(box_lb<MODE == kScore>(a.super_box + sup * 6, sx, sy, sz)))) continue;
    for (int kk = 0; kk < kSuper; ++kk) {
      const int64_t tile = sup * kSuper + ((t0 + kk) & (kSuper - 1));
      if (tile >= a.n_tiles) continue;  // uniform
      const bool need = wants(box_lb<MODE == kScore>(a.tile_box + tile * 6, sx, sy, sz));
      if (!__syncthreads_or(need)) continue;
      const int64_t t_base = tile * kTile;
      for (uint32_t k = tid; k < kTile; k += kThreads) {
        const float4 q = a.tgt4[t_base + k];
        tx[k] = q.x; ty[k] = q.y; tz[k] = q.z;
        if (LIST) tw[k] = __float_as_uint(q.w);
      }
      if (tid < (kTile / kGroup) * 6) gbox[tid / 6][tid % 6] = a.group_box[tile * ((kTile / kGroup) * 6) + tid];
      __syncthreads();
      if (__any(need)) {
        for (int g = 0; g < kTile / kGroup; ++g) {
          if ((g & (kSub / kGroup - 1)) == 0 &&
              !__any(wants(box_lb<MODE == kScore>(a.sub_box + (tile * (kTile / kSub) + g / (kSub / kGroup)) * 6, sx, sy, sz)))) {
            g += kSub / kGroup - 1;   // the whole wave skips this 256-target quarter
            continue;
          }
          {
            const float4 glo = *reinterpret_cast<const float4*>(gbox[g]);
            const float4 ghi = *reinterpret_cast<const float4*>(gbox[g] + 4);   // [lo.x lo.y lo.z hi.x | hi.y hi.z pad pad]
            if (!__any(wants(box_lb<MODE == kScore>(glo.x, glo.y, glo.z, glo.w, ghi.x, ghi.y, sx, sy, sz)))) continue;
          }
          ++groups_done;
          // the radius count is a few instructions per pair: unrolled; an insert is K + 1 (kList: ~6 K) instructions
          // behind a branch, and 32 copies of it would not fit the instruction cache
#pragma unroll kUnrollQ
          for (int q = 0; q < kGroup / 4; ++q) {
            const float4 X = reinterpret_cast<const float4*>(tx)[g * (kGroup / 4) + q];
            const float4 Y = reinterpret_cast<const float4*>(ty)[g * (kGroup / 4) + q];
            const float4 Z = reinterpret_cast<const float4*>(tz)[g * (kGroup / 4) + q];
            // two targets per instruction: the same IEEE operations as fmaf(dz,dz,fmaf(dy,dy,dx*dx)), the same bits
            const f32x2 px = {sx, sx}, py = {sy, sy}, pz = {sz, sz};
            const f32x2 ax = px - f32x2{X.x, X.y}, ay = py - f32x2{Y.x, Y.y}, az = pz - f32x2{Z.x, Z.y};
            const f32x2 bx = px - f32x2{X.z, X.w}, by = py - f32x2{Y.z, Y.w}, bz = pz - f32x2{Z.z, Z.w};
            const f32x2 da = __builtin_elementwise_fma(az, az, __builtin_elementwise_fma(ay, ay, ax * ax));
            const f32x2 db = __builtin_elementwise_fma(bz, bz, __builtin_elementwise_fma(by, by, bx * bx));
            const float d[4] = {da.x, da.y, db.x, db.y};
            if (MODE == kRadius) {
#pragma unroll
              for (int c = 0; c < 4; ++c) cnt += d[c] <= a.r2 ? 1u : 0u;
            } else if (MODE == kScore) {
#pragma unroll
              for (int c = 0; c < 4; ++c) {
                const float v = d[c];
                if (act && v < fl[NS - 1]) {
                  // ascending insert, the largest drops out: slot t <- median(slot t-1, v, slot t)
#pragma unroll
                  for (int t = NS - 1; t > 0; --t) fl[t] = __builtin_amdgcn_fmed3f(fl[t - 1], v, fl[t]);
                  fl[0] = fminf(fl[0], v);
                }
              }
            } else {
              const uint4 W = reinterpret_cast<const uint4*>(tw)[g * (kGroup / 4) + q];
              const uint32_t w[4] = {W.x, W.y, W.z, W.w};
#pragma unroll
              for (int c = 0; c < 4; ++c) {
                const uint64_t key = ((uint64_t)__float_as_uint(d[c]) << 32) | w[c];
                if (act && key < kl[NS - 1] && w[c] != me) {
#pragma unroll
                  for (int t = NS - 1; t > 0; --t) {
                    const uint64_t hi = kl[t - 1] > key ? kl[t - 1] : key;
                    kl[t] = kl[t] < hi ? kl[t] : hi;
                  }
                  kl[0] = kl[0] < key ? kl[0] : key;
                }
              }
            }
          }
        }
      }
      __syncthreads();
    }
  }

  if (MODE == kList) {
    if (ok) {
#pragma unroll
      for (int t = 0; t < NS; ++t) {
        if (t >= front) {
          const uint64_t key = kl[t];
          const bool real = key < kKeyTail;
          const int64_t o = (int64_t)me * a.k + (t - front);
          a.idx_out[o] = real ? (uint32_t)key : 0xffffffffu;
          if (a.d2_out) a.d2_out[o] = real ? __uint_as_float((uint32_t)(key >> 32)) : INFINITY;
        }
      }
    }
  } else if constexpr (MODE == kNormals) {
    if (ok) normals_epilogue<K>(a, kl, front, act, me, sx, sy, sz);
  } else if (MODE == kScore) {
    // m_i = (sum of sqrt((double) d2) over the k real entries, ascending) / k; slot `front` is self's 0
    double m = INFINITY;
    if (fl[NS - 1] < INFINITY) {
      double s = 0.0;
#pragma unroll
      for (int t = 0; t < NS; ++t)
        if (t > front) s += sqrt((double)fl[t]);
      m = s / (double)a.k;
    }
    if (ok) a.score_out[me] = m;
    const bool scored = m < INFINITY;
    __shared__ double sh[kThreads / 64];
    const double sum = block_sum_f64(scored ? m : 0.0, sh);
    const unsigned v = (unsigned)__popcll(__ballot(scored));
    __shared__ unsigned shv[kThreads / 64];
    if ((tid & 63) == 0) shv[tid >> 6] = v;
    __syncthreads();
    if (tid == 0) {
      unsigned t = 0;
      for (int w = 0; w < kThreads / 64; ++w) t += shv[w];
      a.partials[(int64_t)blockIdx.x * 2] = sum;
      a.partials[(int64_t)blockIdx.x * 2 + 1] = (double)t;
    }
  } else {
    // cnt counts self unless the walk stopped before meeting it -- and then cnt - 1 >= min_points already
    const uint64_t c = act ? (uint64_t)cnt - 1 : 0;
    const bool keep = ok && c >= a.min_points;
    if (ok) {
      a.keep_out[me] = keep ? 1 : 0;
      if (a.count_out) a.count_out[me] = (uint32_t)(c < a.min_points ? c : a.min_points);
    }
    const unsigned kept = (unsigned)__popcll(__ballot(keep));
    __shared__ unsigned shk[kThreads / 64];
    if ((tid & 63) == 0) shk[tid >> 6] = kept;
    __syncthreads();
    if (tid == 0) {
      unsigned t = 0;
      for (int w = 0; w < kThreads / 64; ++w) t += shk[w];
      if (t) atomicAdd(a.n_kept, (unsigned long long)t);
    }
  }
  if ((tid & 63) == 0 && groups_done) atomicAdd(a.groups, (unsigned long long)groups_done);
}

// one wave: fold rows of (sum, V) -> stats[0] = V, stats[1] = mu
__global__ __launch_bounds__(64) void sor_mean_kernel(const double* __restrict__ partials, int n_rows, double* __restrict__ stats) {
  double s = 0.0, v = 0.0;
  for (int r = threadIdx.x; r < n_rows; r += 64) {
    s += partials[2 * r];
    v += partials[2 * r + 1];
  }
  s = wave_sum(s);
  v = wave_sum(v);
  if (threadIdx.x == 0) {
    stats[0] = v;
    stats[1] = s / v;   // V = 0: NaN (nothing is scored, nothing is kept)
  }
}

// grid-stride over the rows in original order: one row of sum (m - mu)^2 over the scored points per workgroup
__global__ __launch_bounds__(kThreads) void sor_dev_kernel(const double* __restrict__ score, int64_t n, const double* __restrict__ stats,
                                                           double* __restrict__ partials) {
  const double mu = stats[1];
  double s = 0.0;
  for (int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x; i < n; i += (int64_t)gridDim.x * kThreads) {
    const double m = score[i];
    if (m < INFINITY) s += (m - mu) * (m - mu);
  }
  __shared__ double sh[kThreads / 64];
  s = block_sum_f64(s, sh);
  if (threadIdx.x == 0) partials[blockIdx.x] = s;
}

// one wave: sigma (0 when V <= 1) and T = mu + ratio sigma -> stats[2], stats[3]
__global__ __launch_bounds__(64) void sor_threshold_kernel(const double* __restrict__ partials, int n_rows, double std_ratio,
                                                           double* __restrict__ stats) {
  double s = 0.0;
  for (int r = threadIdx.x; r < n_rows; r += 64) s += partials[r];
  s = wave_sum(s);
  if (threadIdx.x == 0) {
    const double v = stats[0];
    const double sigma = v > 1.0 ? sqrt(s / (v - 1.0)) : 0.0;
    stats[2] = sigma;
    stats[3] = stats[1] + std_ratio * sigma;
  }
}

__global__ __launch_bounds__(kThreads) void sor_keep_kernel(const double* __restrict__ score, int64_t n, const double* __restrict__ stats,
                                                            uint8_t* __restrict__ keep, unsigned long long* __restrict__ n_kept) {
  const double T = stats[3];
  unsigned kept = 0;
  for (int64_t i0 = (int64_t)blockIdx.x * kThreads; i0 < n; i0 += (int64_t)gridDim.x * kThreads) {
    const int64_t i = i0 + threadIdx.x;
    const bool k = i < n && score[i] <= T;   // unscored: +inf, never kept
    if (i < n) keep[i] = k ? 1 : 0;
    kept += (unsigned)__popcll(__ballot(k));
  }
  __shared__ unsigned sh[kThreads / 64];
  if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = kept;
  __syncthreads();
  if (threadIdx.x == 0) {
    unsigned t = 0;
    for (int w = 0; w < kThreads / 64; ++w) t += sh[w];
    if (t) atomicAdd(n_kept, (unsigned long long)t);
  }
}

// ---- order-preserving row selection: 4096 flags per workgroup, 16 consecutive ones per thread -------------------------------
using r3d_compact::kPer;
__global__ __launch_bounds__(kThreads) void select_count_kernel(const uint8_t* __restrict__ keep, int64_t n, uint32_t* __restrict__ hist) {
  const int64_t base = r3d_compact::tile_base();
  uint32_t c = 0;
#pragma unroll
  for (int e = 0; e < kPer; ++e)
    if (base + e < n) c += keep[base + e] != 0;
  // r3d_compact::block_sum written out: behind a function boundary the byte compares change encoding, 245 instructions for 260
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) c += __shfl_down(c, off, 64);
  __shared__ uint32_t sh[kThreads / 64];
  if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = c;
  __syncthreads();
  r3d_compact::publish(hist, sh[0] + sh[1] + sh[2] + sh[3]);
}

// hist: the tiles' exclusive prefixes
__global__ __launch_bounds__(kThreads) void select_write_kernel(const float* __restrict__ xyz, int64_t n, const uint8_t* __restrict__ keep,
                                                                const uint32_t* __restrict__ hist, float* __restrict__ xyz_out,
                                                                uint32_t* __restrict__ rows_out) {
  const int64_t base = r3d_compact::tile_base();
  uint32_t mask = 0;
#pragma unroll
  for (int e = 0; e < kPer; ++e)
    if (base + e < n && keep[base + e] != 0) mask |= 1u << e;
  __shared__ uint64_t wave_total[kThreads / 64];
  uint64_t at = r3d_compact::tile_start(hist, (uint64_t)__popc(mask), wave_total);
  const P3* src = reinterpret_cast<const P3*>(xyz);
  P3* dst = reinterpret_cast<P3*>(xyz_out);
  while (mask) {
    const int e = __ffs(mask) - 1;
    mask &= mask - 1;
    dst[at] = src[base + e];
    if (rows_out) rows_out[at] = (uint32_t)(base + e);
    ++at;
  }
}

// launches knn_kernel for MODE with the smallest K >= k (asynchronous); resets the index's group counter first
template <int MODE>
int knn_launch(r3d_nn_index* ix, KnnArgs& a) {
  r3d_ctx* ctx = ix->ctx;
  a.tgt4 = ix->d_tgt4;
  a.n = ix->n;
  a.n_tiles = ix->n_tiles;
  a.tile_box = ix->d_tile_box;
  a.sub_box = ix->d_sub_box;
  a.group_box = ix->d_group_box;
  a.super_box = ix->d_super_box;
  a.groups = ix->d_knn_groups;
  R3D_HIP(hipMemsetAsync(ix->d_knn_groups, 0, sizeof(unsigned long long), ctx->stream));
  const dim3 grid((unsigned)(ix->n_tiles * (kTile / kThreads))), block(kThreads);
  a.tgt = ix->d_tgt;
  if constexpr (MODE == kRadius) hipLaunchKernelGGL((knn_kernel<kRadius, 1>), grid, block, 0, ctx->stream, a);
  else if (a.k <= 8) hipLaunchKernelGGL((knn_kernel<MODE, 8>), grid, block, 0, ctx->stream, a);
  else if (a.k <= 16) hipLaunchKernelGGL((knn_kernel<MODE, 16>), grid, block, 0, ctx->stream, a);
  else hipLaunchKernelGGL((knn_kernel<MODE, 32>), grid, block, 0, ctx->stream, a);
  R3D_HIP(hipGetLastError());
  return R3D_OK;
}

int reduce_blocks(int64_t n) { return (int)std::min<int64_t>((n + kThreads - 1) / kThreads, kReduceBlocks); }

}  // namespace

extern "C" {

int r3d_nn_index_knn_self(r3d_nn_index* ix, int k, uint32_t* d_idx_out, float* d_d2_out) {
  R3D_REQUIRE(ix != nullptr, "nn index is NULL");
  R3D_REQUIRE(k >= 1 && k <= 32, "k must be in [1, 32], got %d", k);
  R3D_REQUIRE(d_idx_out != nullptr, "d_idx_out is NULL");
  const size_t bytes = (size_t)ix->n * k * 4;
  R3D_REQUIRE(!r3d_ranges_overlap(d_idx_out, bytes, d_d2_out, bytes), "d_idx_out and d_d2_out overlap");
  int rc = r3d_ctx_enter(ix->ctx);
  if (rc) return rc;
  r3d_wrote(ix->ctx, d_idx_out, bytes);
  if (d_d2_out) r3d_wrote(ix->ctx, d_d2_out, bytes);
  KnnArgs a = {};
  a.k = k;
  a.idx_out = d_idx_out;
  a.d2_out = d_d2_out;
  return knn_launch<kList>(ix, a);
}

int r3d_normals_knn(r3d_nn_index* ix, int k, double radius, const double* h_viewpoints, int64_t n_views, int64_t points_per_view,
                    float* d_normals_out, float* d_curvature_out, double* d_cov_out, uint32_t* d_count_out) {
  R3D_REQUIRE(ix != nullptr, "nn index is NULL");
  R3D_REQUIRE(k >= 3 && k <= 32, "k must be in [3, 32], got %d", k);
  R3D_REQUIRE(!std::isnan(radius), "radius is NaN");
  R3D_REQUIRE(n_views >= 0, "n_views must be >= 0, got %lld", (long long)n_views);
  R3D_REQUIRE(n_views == 0 || (h_viewpoints != nullptr && points_per_view >= 1),
              "n_views > 0 needs a viewpoint table and points_per_view >= 1");
  R3D_REQUIRE(d_normals_out != nullptr, "d_normals_out is NULL");
  const int64_t n = ix->n;
  const bool divide = n_views > 1 && points_per_view < n;   // otherwise every row belongs to view 0
  R3D_REQUIRE(!divide || n <= ((int64_t)1 << 31), "per-view orientation needs a cloud of at most 2^31 rows");
  const struct {
    const void* p;
    size_t bytes;
  } out[4] = {{d_normals_out, (size_t)n * 12}, {d_curvature_out, (size_t)n * 4}, {d_cov_out, (size_t)n * 48}, {d_count_out, (size_t)n * 4}};
  for (int i = 0; i < 4; ++i) {
    R3D_REQUIRE(!r3d_ranges_overlap(out[i].p, out[i].bytes, ix->d_tgt, (size_t)n * 12), "an output overlaps the index's cloud");
    for (int j = i + 1; j < 4; ++j) R3D_REQUIRE(!r3d_ranges_overlap(out[i].p, out[i].bytes, out[j].p, out[j].bytes), "outputs overlap each other");
  }
  r3d_ctx* ctx = ix->ctx;
  int rc = r3d_ctx_enter(ctx);
  if (rc) return rc;
  KnnArgs a = {};
  if (n_views > 0) {
    // at most a few thousand rows of 24 bytes: one upload per call into the library's own buffer
    void* views = nullptr;
    if ((rc = r3d_scratch(ctx, kWsMisc, (size_t)n_views * 24, &views))) return rc;
    R3D_HIP(hipMemcpyAsync(views, h_viewpoints, (size_t)n_views * 24, hipMemcpyHostToDevice, ctx->stream));
    a.views = static_cast<const double*>(views);
    a.n_views = divide ? (uint32_t)std::min<int64_t>(n_views, n) : 1u;
    r3d_magic::make_magic(divide ? (uint32_t)points_per_view : 1u, &a.v_magic, &a.v_shift);
  }
  for (int i = 0; i < 4; ++i)
    if (out[i].p) r3d_wrote(ctx, out[i].p, out[i].bytes);
  a.k = k;
  const float r2 = (float)(radius * radius);
  a.r2 = radius > 0.0 ? r2 : INFINITY;
  a.nrm_out = d_normals_out;
  a.curv_out = d_curvature_out;
  a.cov_out = d_cov_out;
  a.count_out = d_count_out;
  return knn_launch<kNormals>(ix, a);
}

int r3d_outlier_statistical(r3d_nn_index* ix, int k, double std_ratio, uint8_t* d_keep_out, double* d_score_out,
                            double* h_stats_out, int64_t* h_n_kept) {
  R3D_REQUIRE(ix != nullptr, "nn index is NULL");
  R3D_REQUIRE(k >= 1 && k <= 32, "k must be in [1, 32], got %d", k);
  R3D_REQUIRE(std::isfinite(std_ratio) && std_ratio > 0.0, "std_ratio must be finite and > 0, got %g", std_ratio);
  R3D_REQUIRE(d_keep_out != nullptr, "d_keep_out is NULL");
  const int64_t n = ix->n;
  R3D_REQUIRE(!r3d_ranges_overlap(d_keep_out, (size_t)n, d_score_out, (size_t)n * 8), "d_keep_out and d_score_out overlap");
  r3d_ctx* ctx = ix->ctx;
  int rc = r3d_ctx_enter(ctx);
  if (rc) return rc;
  const int blocks = (int)(ix->n_tiles * (kTile / kThreads)), rblocks = reduce_blocks(n);
  void* score = d_score_out;
  if (!score && (rc = r3d_scratch(ctx, kWsOut, (size_t)n * 8, &score))) return rc;
  r3d_carve rows, misc;
  const auto rows1_h = rows.take<double>((size_t)2 * blocks), rows2_h = rows.take<double>(rblocks);
  // the four statistics fill their 32 bytes, so the kept count, taken at the same alignment, lies right behind them: one copy of
  // five words reads both
  const auto stats_h = misc.take<double>(4, 32);   // V, mu, sigma, T
  const auto kept_h = misc.take<unsigned long long>(1, 32);
  if ((rc = r3d_scratch(ctx, kWsPartials, rows)) || (rc = r3d_scratch(ctx, kWsMisc, misc))) return rc;
  double *stats = misc.at(stats_h), *rows1 = rows.at(rows1_h), *rows2 = rows.at(rows2_h);
  unsigned long long* kept = misc.at(kept_h);
  r3d_wrote(ctx, d_keep_out, (size_t)n);
  if (d_score_out) r3d_wrote(ctx, d_score_out, (size_t)n * 8);
  hipStream_t st = ctx->stream;
  R3D_HIP(hipMemsetAsync(kept, 0, sizeof(unsigned long long), st));
  KnnArgs a = {};
  a.k = k;
  a.score_out = static_cast<double*>(score);
  a.partials = rows1;
  if ((rc = knn_launch<kScore>(ix, a))) return rc;
  hipLaunchKernelGGL(sor_mean_kernel, dim3(1), dim3(64), 0, st, (const double*)rows1, blocks, stats);
  hipLaunchKernelGGL(sor_dev_kernel, dim3(rblocks), dim3(kThreads), 0, st, (const double*)score, n, (const double*)stats, rows2);
  hipLaunchKernelGGL(sor_threshold_kernel, dim3(1), dim3(64), 0, st, (const double*)rows2, rblocks, std_ratio, stats);
  hipLaunchKernelGGL(sor_keep_kernel, dim3(rblocks), dim3(kThreads), 0, st, (const double*)score, n, (const double*)stats, d_keep_out,
                     kept);
  R3D_HIP(hipGetLastError());
  double h[5];
  R3D_HIP(hipMemcpyAsync(h, stats, sizeof(h), hipMemcpyDeviceToHost, st));
  R3D_HIP(hipStreamSynchronize(st));
  if (h_stats_out) memcpy(h_stats_out, h, 4 * sizeof(double));
  if (h_n_kept) {
    unsigned long long v;
    memcpy(&v, &h[4], sizeof(v));
    *h_n_kept = (int64_t)v;
  }
  return R3D_OK;
}

int r3d_outlier_radius(r3d_nn_index* ix, double radius, int64_t min_points, uint8_t* d_keep_out, uint32_t* d_count_out,
                       int64_t* h_n_kept) {
  R3D_REQUIRE(ix != nullptr, "nn index is NULL");
  R3D_REQUIRE(std::isfinite(radius) && radius > 0.0, "radius must be finite and > 0, got %g", radius);
  R3D_REQUIRE(min_points >= 1, "min_points must be >= 1, got %lld", (long long)min_points);
  R3D_REQUIRE(d_keep_out != nullptr, "d_keep_out is NULL");
  const int64_t n = ix->n;
  R3D_REQUIRE(!r3d_ranges_overlap(d_keep_out, (size_t)n, d_count_out, (size_t)n * 4), "d_keep_out and d_count_out overlap");
  r3d_ctx* ctx = ix->ctx;
  int rc = r3d_ctx_enter(ctx);
  if (rc) return rc;
  void* misc = nullptr;
  if ((rc = r3d_scratch(ctx, kWsMisc, 64, &misc))) return rc;
  unsigned long long* kept = static_cast<unsigned long long*>(misc);
  r3d_wrote(ctx, d_keep_out, (size_t)n);
  if (d_count_out) r3d_wrote(ctx, d_count_out, (size_t)n * 4);
  R3D_HIP(hipMemsetAsync(kept, 0, sizeof(unsigned long long), ctx->stream));
  KnnArgs a = {};
  a.k = 1;
  const float r2 = (float)(radius * radius);
  a.r2 = r2 < INFINITY ? r2 : 3.40282347e+38f;
  a.min_points = (uint64_t)std::min<int64_t>(min_points, n);
  a.keep_out = d_keep_out;
  a.count_out = d_count_out;
  a.n_kept = kept;
  if ((rc = knn_launch<kRadius>(ix, a))) return rc;
  unsigned long long v = 0;
  R3D_HIP(hipMemcpyAsync(&v, kept, sizeof(v), hipMemcpyDeviceToHost, ctx->stream));
  R3D_HIP(hipStreamSynchronize(ctx->stream));
  if (h_n_kept) *h_n_kept = (int64_t)v;
  return R3D_OK;
}

int r3d_select_rows(r3d_ctx* ctx, const float* d_xyz, int64_t n, const uint8_t* d_keep, float* d_xyz_out, uint32_t* d_rows_out,
                    int64_t* h_n_out) {
  int rc = r3d_ctx_enter(ctx);
  if (rc) return rc;
  R3D_REQUIRE(h_n_out != nullptr, "h_n_out is NULL");
  R3D_REQUIRE(n >= 0 && n < ((int64_t)1 << 32), "bad cloud size %lld", (long long)n);
  if (n == 0) {
    *h_n_out = 0;
    return R3D_OK;
  }
  R3D_REQUIRE(d_xyz && d_keep && d_xyz_out, "NULL device pointer");
  const size_t xb = (size_t)n * 12;
  R3D_REQUIRE(!r3d_ranges_overlap(d_keep, (size_t)n, d_xyz, xb), "d_keep overlaps d_xyz");
  const int tiles = r3d_compact::tiles_of(n);
  r3d_compact::Counters cn(tiles, 1);
  void* ws = nullptr;
  if ((rc = r3d_scratch(ctx, kWsCounts, cn.bytes, &ws))) return rc;
  cn.place(ws);
  hipStream_t st = ctx->stream;
  hipLaunchKernelGGL(select_count_kernel, dim3(tiles), dim3(kThreads), 0, st, d_keep, n, cn.hist);
  uint32_t m = 0;
  if ((rc = r3d_compact::scan_totals(ctx, cn, &m))) return rc;
  // the outputs need room for the kept rows only; none of them may overlap an input or the other output
  const size_t ob = (size_t)m * 12, rb = d_rows_out ? (size_t)m * 4 : 0;
  R3D_REQUIRE(!r3d_ranges_overlap(d_xyz_out, ob, d_xyz, xb) && !r3d_ranges_overlap(d_xyz_out, ob, d_keep, (size_t)n) &&
                  !r3d_ranges_overlap(d_rows_out, rb, d_xyz, xb) && !r3d_ranges_overlap(d_rows_out, rb, d_keep, (size_t)n) &&
                  !r3d_ranges_overlap(d_rows_out, rb, d_xyz_out, ob),
              "an output range overlaps an input or the other output");
  *h_n_out = (int64_t)m;
  if (m == 0) return R3D_OK;
  r3d_wrote(ctx, d_xyz_out, ob);
  if (d_rows_out) r3d_wrote(ctx, d_rows_out, rb);
  hipLaunchKernelGGL(select_write_kernel, dim3(tiles), dim3(kThreads), 0, st, d_xyz, n, d_keep, (const uint32_t*)cn.hist, d_xyz_out,
                     d_rows_out);
  R3D_HIP(hipGetLastError());
  return R3D_OK;
}

int r3d_nn_index_knn_stats(r3d_nn_index* ix, int64_t* h_pairs) {
  R3D_REQUIRE(ix != nullptr && h_pairs != nullptr, "NULL argument");
  int rc = r3d_ctx_enter(ix->ctx);
  if (rc) return rc;
  unsigned long long g = 0;
  R3D_HIP(hipMemcpyAsync(&g, ix->d_knn_groups, sizeof(g), hipMemcpyDeviceToHost, ix->ctx->stream));
  R3D_HIP(hipStreamSynchronize(ix->ctx->stream));
  *h_pairs = (int64_t)(g * kGroup * 64);
  return R3D_OK;
}

}  // extern "C"
