// Reconstruction evaluation for gfx950 (MI355X): exact point-to-triangle-mesh distance, distance statistics, the f32 root and the
// distance colour ramp.  NOT IN THE REFERENCE (its readme leaves the comparison to CloudCompare); include/r3d.h ("Reconstruction
// evaluation") is the specification, tests/compare_ref.py restates it in NumPy.  None of these kernels has been timed on a card.
//
// r3d_mesh_index_create -- the index owns a copy of the mesh's VALID triangles, sorted by the Morton code of their centroid in
//   the quantisation frame of the valid vertices' bounding box (r3d_nn::point_code, r3d_radix_sort_u64):
//   md_bbox_kernel    indices checked before they are addresses, nine coordinates finite -> the box, by integer atomicMin / Max on
//                     order-preserving encodings of the f32 bounds (one per wave and bound)
//   md_keys_kernel    key = centroid code << idx_bits | triangle; an invalid triangle gets the code above all codes
//   md_gather_kernel  sorted slot -> 12 floats (a, b, c, original index, 2 unused); md_group_kernel: the f32 box and the first
//                     code of every 32-triangle group
// r3d_mesh_index_query -- the points are sorted by the same code; one wave takes 64 consecutive sorted points, one per lane:
//   md_query_kernel   starts at the group whose first code is the last one <= the wave's first point's, walks outwards group by
//                     group, and skips a group only when its box's lower bound is STRICTLY above every lane's current best.  The
//                     lower bound is made conservative (kSlack) so that it never exceeds the d2 the definition computes for any
//                     triangle in the box; the best is kept as (d2, original index) in lexicographic order, so the answer is the
//                     brute-force one bit for bit, whatever the order the groups are met in.  Triangles are read with
//                     wave-uniform addresses.  No 1024-triangle tile level yet: a wave tests every group's box.
// r3d_distance_stats -- one row of partials per 256 elements (r3d_sums::block_reduce_store), one finish workgroup
//   (r3d_sums::finish_rows): fixed order, the same bits run to run.  Counts and the histogram: LDS integer atomics, flushed with
//   64-bit integer atomics.
#include <cmath>
#include <new>

#include "r3d_nnindex_dev.h"
#include "r3d_sums_dev.h"

struct r3d_mesh_index {
  r3d_ctx* ctx = nullptr;
  int device = 0;           // destroy never touches a ctx that may already be gone
  int64_t n_valid = 0;      // valid triangles = sorted slots in use
  int64_t n_groups = 0;     // ceil(n_valid / 32)
  float* d_tri = nullptr;   // [n_groups * 32][12]: ax ay az bx by bz cx cy cz, original index bits, 2 unused
  float* d_group_box = nullptr;     // [n_groups][6] lo xyz, hi xyz
  uint64_t* d_group_code = nullptr; // [n_groups] code of the group's first triangle
  float* d_frame = nullptr;         // [8] lo xyz, scale xyz, unused
  uint32_t* d_bounds = nullptr;     // [6] encoded lo xyz, hi xyz
  unsigned long long* d_counters = nullptr;  // [0] valid triangles, [1] group evaluations of the last counted query
  void* d_slab = nullptr;
};

namespace {

constexpr int kThreads = 256;
constexpr int kGroup = 32;
constexpr int kAxisBits = 10;
constexpr int kTriFloats = 12;
constexpr uint32_t kNoTriangle = 0xFFFFFFFFu;
constexpr double kSlack = 9.094947017729282e-13;   // 2^-40: see box_lower_bound
constexpr int kStatsRow = 256;                      // elements per row of partials
constexpr int kMaxThresholds = 8, kMaxBins = 4096;

using r3d_nn::P3;
using r3d_nn::point_code;

inline unsigned blocks_of(int64_t n) { return (unsigned)((n + kThreads - 1) / kThreads); }

int bits_for(int64_t n) {
  int b = 1;
  while (((int64_t)1 << b) < n) ++b;
  return b;
}

__device__ __forceinline__ bool finite3(const P3& p) { return (p.x - p.x == 0.f) && (p.y - p.y == 0.f) && (p.z - p.z == 0.f); }

// f32 -> u32 whose unsigned order is the order of the floats
__device__ __forceinline__ uint32_t enc(float f) {
  const uint32_t u = __float_as_uint(f);
  return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ float dec(uint32_t e) { return __uint_as_float((e & 0x80000000u) ? (e & 0x7FFFFFFFu) : ~e); }

// the triangle's vertices where it is valid: indices in [0, nv) (checked before they are addresses), nine finite coordinates
__device__ __forceinline__ bool load_triangle(const float* __restrict__ xyz, uint32_t nv, const int32_t* __restrict__ tri, int64_t t,
                                              P3& a, P3& b, P3& c) {
  const int32_t ia = tri[3 * t], ib = tri[3 * t + 1], ic = tri[3 * t + 2];
  if (!((uint32_t)ia < nv && (uint32_t)ib < nv && (uint32_t)ic < nv)) return false;   // a negative index is >= 2^31 as unsigned
  const P3* V = reinterpret_cast<const P3*>(xyz);
  a = V[ia];
  b = V[ib];
  c = V[ic];
  return finite3(a) && finite3(b) && finite3(c);
}

__global__ __launch_bounds__(kThreads) void md_init_kernel(uint32_t* __restrict__ bounds, unsigned long long* __restrict__ counters) {
  if (threadIdx.x < 3) bounds[threadIdx.x] = 0xFFFFFFFFu;
  else if (threadIdx.x < 6) bounds[threadIdx.x] = 0u;
  else if (threadIdx.x < 8) counters[threadIdx.x - 6] = 0ull;
}

__global__ __launch_bounds__(kThreads) void md_bbox_kernel(const float* __restrict__ xyz, uint32_t nv, const int32_t* __restrict__ tri,
                                                           int64_t nt, uint32_t* __restrict__ bounds, unsigned long long* __restrict__ counters) {
  const int64_t t = (int64_t)blockIdx.x * kThreads + threadIdx.x;
  P3 a, b, c;
  const bool valid = t < nt && load_triangle(xyz, nv, tri, t, a, b, c);
  uint32_t lo[3] = {0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu}, hi[3] = {0u, 0u, 0u};
  if (valid) {
    const float v[3][3] = {{a.x, b.x, c.x}, {a.y, b.y, c.y}, {a.z, b.z, c.z}};
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      lo[k] = enc(fminf(fminf(v[k][0], v[k][1]), v[k][2]));
      hi[k] = enc(fmaxf(fmaxf(v[k][0], v[k][1]), v[k][2]));
    }
  }
#pragma unroll
  for (int k = 0; k < 3; ++k) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
      lo[k] = min(lo[k], (uint32_t)__shfl_down((int)lo[k], off, 64));
      hi[k] = max(hi[k], (uint32_t)__shfl_down((int)hi[k], off, 64));
    }
  }
  const unsigned long long any = __ballot(valid);
  if ((threadIdx.x & 63) == 0 && any) {
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      atomicMin(bounds + k, lo[k]);
      atomicMax(bounds + 3 + k, hi[k]);
    }
    atomicAdd(counters, (unsigned long long)__popcll(any));
  }
}

// one thread: the quantisation frame of the box (no valid triangle: scale 0, every code 0)
__global__ void md_frame_kernel(const uint32_t* __restrict__ bounds, float* __restrict__ frame) {
  if (threadIdx.x >= 3) return;
  const int k = threadIdx.x;
  const float lo = dec(bounds[k]), hi = dec(bounds[3 + k]);
  const float ext = hi - lo;
  frame[k] = (lo - lo == 0.f) ? lo : 0.f;
  frame[3 + k] = (ext > 0.f && ext - ext == 0.f) ? (float)((1 << kAxisBits) - 1) / ext : 0.f;
}

__global__ __launch_bounds__(kThreads) void md_keys_kernel(const float* __restrict__ xyz, uint32_t nv, const int32_t* __restrict__ tri,
                                                           int64_t nt, const float* __restrict__ frame, int idx_bits,
                                                           uint64_t* __restrict__ keys) {
  const int64_t t = (int64_t)blockIdx.x * kThreads + threadIdx.x;
  if (t >= nt) return;
  P3 a, b, c;
  uint64_t code = (uint64_t)1 << (3 * kAxisBits);
  if (load_triangle(xyz, nv, tri, t, a, b, c)) {
    const float third = 1.f / 3.f;   // (only the order of the slots depends on the centroid; an overflow clamps in point_code)
    const P3 m{a.x * third + b.x * third + c.x * third, a.y * third + b.y * third + c.y * third, a.z * third + b.z * third + c.z * third};
    code = point_code(m, frame, kAxisBits);
  }
  keys[t] = (code << idx_bits) | (uint64_t)t;
}

__global__ __launch_bounds__(kThreads) void md_gather_kernel(const float* __restrict__ xyz, const int32_t* __restrict__ tri,
                                                             const uint64_t* __restrict__ keys, int64_t n_valid, int64_t n_slots,
                                                             int idx_bits, float* __restrict__ out) {
  const int64_t j = (int64_t)blockIdx.x * kThreads + threadIdx.x;
  if (j >= n_slots) return;
  float* o = out + j * kTriFloats;
  if (j < n_valid) {   // the valid triangles sort in front: their indices have been checked
    const uint32_t t = (uint32_t)(keys[j] & (((uint64_t)1 << idx_bits) - 1));
    const P3* V = reinterpret_cast<const P3*>(xyz);
    const P3 a = V[tri[3 * (int64_t)t]], b = V[tri[3 * (int64_t)t + 1]], c = V[tri[3 * (int64_t)t + 2]];
    o[0] = a.x, o[1] = a.y, o[2] = a.z, o[3] = b.x, o[4] = b.y, o[5] = b.z, o[6] = c.x, o[7] = c.y, o[8] = c.z;
    o[9] = __uint_as_float(t);
  } else {             // padding of the last group: never read (the query stops at n_valid)
    for (int k = 0; k < 9; ++k) o[k] = 0.f;
    o[9] = __uint_as_float(kNoTriangle);
  }
  o[10] = 0.f;
  o[11] = 0.f;
}

// a thread per group: its f32 box (exact: minima and maxima of f32 values) and the code of its first triangle
__global__ __launch_bounds__(kThreads) void md_group_kernel(const float* __restrict__ tris, const uint64_t* __restrict__ keys, int64_t n_valid,
                                                            int64_t n_groups, int idx_bits, float* __restrict__ box,
                                                            uint64_t* __restrict__ code) {
  const int64_t g = (int64_t)blockIdx.x * kThreads + threadIdx.x;
  if (g >= n_groups) return;
  float lo[3] = {INFINITY, INFINITY, INFINITY}, hi[3] = {-INFINITY, -INFINITY, -INFINITY};
  const int64_t first = g * kGroup, last = first + kGroup < n_valid ? first + kGroup : n_valid;
  for (int64_t j = first; j < last; ++j) {
    const float* T = tris + j * kTriFloats;
    for (int v = 0; v < 3; ++v)
      for (int k = 0; k < 3; ++k) {
        lo[k] = fminf(lo[k], T[3 * v + k]);
        hi[k] = fmaxf(hi[k], T[3 * v + k]);
      }
  }
  for (int k = 0; k < 3; ++k) {
    box[g * 6 + k] = lo[k];
    box[g * 6 + 3 + k] = hi[k];
  }
  code[g] = keys[first] >> idx_bits;
}

__global__ __launch_bounds__(kThreads) void md_point_keys_kernel(const float* __restrict__ pts, int64_t n, const float* __restrict__ frame,
                                                                 int idx_bits, uint64_t* __restrict__ keys) {
  const int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x;
  if (i >= n) return;
  const P3 p = reinterpret_cast<const P3*>(pts)[i];
  const uint64_t code = finite3(p) ? point_code(p, frame, kAxisBits) : ((uint64_t)1 << (3 * kAxisBits));
  keys[i] = (code << idx_bits) | (uint64_t)i;
}

// ---- the definition (include/r3d.h): closest point of the closed triangle, region form, fp64, selects only --------------------
struct Hit {
  double d2, qx, qy, qz;
};

__device__ __forceinline__ double dot3(double ax, double ay, double az, double bx, double by, double bz) {
  return ax * bx + ay * by + az * bz;
}

__device__ __forceinline__ Hit closest_on_triangle(double px, double py, double pz, const float* __restrict__ T) {
  const double ax = (double)T[0], ay = (double)T[1], az = (double)T[2];
  const double bx = (double)T[3], by = (double)T[4], bz = (double)T[5];
  const double cx = (double)T[6], cy = (double)T[7], cz = (double)T[8];
  const double abx = bx - ax, aby = by - ay, abz = bz - az;
  const double acx = cx - ax, acy = cy - ay, acz = cz - az;
  const double bcx = cx - bx, bcy = cy - by, bcz = cz - bz;
  const double apx = px - ax, apy = py - ay, apz = pz - az;
  const double bpx = px - bx, bpy = py - by, bpz = pz - bz;
  const double cpx = px - cx, cpy = py - cy, cpz = pz - cz;
  const double d1 = dot3(abx, aby, abz, apx, apy, apz), d2 = dot3(acx, acy, acz, apx, apy, apz);
  const double d3 = dot3(abx, aby, abz, bpx, bpy, bpz), d4 = dot3(acx, acy, acz, bpx, bpy, bpz);
  const double d5 = dot3(abx, aby, abz, cpx, cpy, cpz), d6 = dot3(acx, acy, acz, cpx, cpy, cpz);
  const double vc = d1 * d4 - d3 * d2, vb = d5 * d2 - d1 * d6, va = d3 * d6 - d5 * d4;
  const double e43 = d4 - d3, e56 = d5 - d6;
  const double den_ab = d1 - d3, den_ac = d2 - d6, den_bc = e43 + e56;   // |ab|^2, |ac|^2, |bc|^2 but for rounding
  const bool in_a = d1 <= 0.0 && d2 <= 0.0;
  const bool in_b = !in_a && d3 >= 0.0 && d4 <= d3;
  const bool in_ab = !in_a && !in_b && vc <= 0.0 && d1 >= 0.0 && d3 <= 0.0 && den_ab > 0.0;
  const bool done3 = in_a || in_b || in_ab;
  const bool in_c = !done3 && d6 >= 0.0 && d5 <= d6;
  const bool in_ac = !done3 && !in_c && vb <= 0.0 && d2 >= 0.0 && d6 <= 0.0 && den_ac > 0.0;
  const bool done5 = done3 || in_c || in_ac;
  const bool in_bc = !done5 && va <= 0.0 && e43 >= 0.0 && e56 >= 0.0 && den_bc > 0.0;
  const bool face = !done5 && !in_bc;
  const bool vertex = in_a || in_b || in_c;
  // ONE quotient num / den.  An edge region is taken only with den > 0 (an edge of no length is left to its end points'
  // regions); the face's quotient is taken as 0 where den > 0 does not hold.  No zero-area triangle reaches a division by 0.
  const double num = in_ab ? d1 : in_ac ? d2 : in_bc ? e43 : 1.0;
  const double den = in_ab ? den_ab : in_ac ? den_ac : in_bc ? den_bc : (va + vb) + vc;
  const double r = den > 0.0 ? num / den : 0.0;
  double v = vb * r, w = vc * r;            // face only
  v = v > 0.0 ? v : 0.0;                    // (a NaN becomes 0)
  v = v < 1.0 ? v : 1.0;
  const double wmax = 1.0 - v;
  w = w > 0.0 ? w : 0.0;
  w = w < wmax ? w : wmax;
  const double t1 = face ? v : (in_ab || in_bc) ? r : 0.0;
  const double t2 = face ? w : in_ac ? r : 0.0;
  const bool from_b = in_b || in_bc;
  const double sx = in_c ? cx : from_b ? bx : ax, sy = in_c ? cy : from_b ? by : ay, sz = in_c ? cz : from_b ? bz : az;
  const double ex = in_bc ? bcx : abx, ey = in_bc ? bcy : aby, ez = in_bc ? bcz : abz;
  Hit h;
  // a vertex region returns the vertex itself (exactly: no products are added to it)
  h.qx = vertex ? sx : (sx + ex * t1) + acx * t2;
  h.qy = vertex ? sy : (sy + ey * t1) + acy * t2;
  h.qz = vertex ? sz : (sz + ez * t1) + acz * t2;
  const double dx = px - h.qx, dy = py - h.qy, dz = pz - h.qz;
  h.d2 = dx * dx + dy * dy + dz * dz;
  return h;
}

// A lower bound of the d2 that closest_on_triangle computes for ANY triangle inside the f32 box.  The exact closest point lies in
// the box; the computed one is within a few fp64 roundings of coordinates no larger than the box's (< 2^-50 of `scale`), and the
// squares and sums round by 2^-52 of their values.  kSlack = 2^-40 of the largest coordinate in play, taken off every axis gap,
// and again off the sum, covers both many times over: a group is never skipped wrongly, so culling cannot change a bit.
__device__ __forceinline__ double box_lower_bound(double px, double py, double pz, double pscale, const float* __restrict__ box) {
  const double lx = (double)box[0], ly = (double)box[1], lz = (double)box[2], hx = (double)box[3], hy = (double)box[4], hz = (double)box[5];
  double scale = pscale;
  scale = fmax(scale, fmax(fabs(lx), fabs(hx)));
  scale = fmax(scale, fmax(fabs(ly), fabs(hy)));
  scale = fmax(scale, fmax(fabs(lz), fabs(hz)));
  const double slack = scale * kSlack;
  const double gx = fmax(fmax(lx - px, px - hx) - slack, 0.0);
  const double gy = fmax(fmax(ly - py, py - hy) - slack, 0.0);
  const double gz = fmax(fmax(lz - pz, pz - hz) - slack, 0.0);
  return (gx * gx + gy * gy + gz * gz) * (1.0 - kSlack);
}

struct Best {
  double d2;
  uint32_t tri;     // original index
  int64_t slot;     // where the winner sits in the sorted table
};

__device__ __forceinline__ void visit_group(int64_t g, const float* __restrict__ tris, const float* __restrict__ group_box, int64_t n_valid,
                                            double px, double py, double pz, double pscale, bool valid, Best& best,
                                            unsigned long long& evaluated) {
  const double lb = box_lower_bound(px, py, pz, pscale, group_box + g * 6);
  if (__ballot(valid && !(lb > best.d2)) == 0ull) return;   // strictly above EVERY lane's best: nothing in it can win or tie
  ++evaluated;
  const int64_t first = g * kGroup;
  const int cnt = (int)(n_valid - first < kGroup ? n_valid - first : kGroup);
  for (int k = 0; k < cnt; ++k) {
    const float* T = tris + (first + k) * kTriFloats;   // wave-uniform address
    const uint32_t t = __float_as_uint(T[9]);
    const Hit h = closest_on_triangle(px, py, pz, T);
    const bool better = valid && (h.d2 < best.d2 || (h.d2 == best.d2 && t < best.tri));
    best.d2 = better ? h.d2 : best.d2;
    best.tri = better ? t : best.tri;
    best.slot = better ? first + k : best.slot;
  }
}

__global__ __launch_bounds__(kThreads) void md_query_kernel(const float* __restrict__ pts, const uint64_t* __restrict__ keys, int64_t n,
                                                            int idx_bits, const float* __restrict__ tris,
                                                            const float* __restrict__ group_box, const uint64_t* __restrict__ group_code,
                                                            int64_t n_valid, int64_t n_groups, int flags, float* __restrict__ dist_out,
                                                            uint32_t* __restrict__ tri_out, float* __restrict__ closest_out,
                                                            unsigned long long* __restrict__ counter) {
  const int lane = threadIdx.x & 63;
  const int64_t wave_first = ((int64_t)blockIdx.x * (kThreads / 64) + (threadIdx.x >> 6)) * 64;
  if (wave_first >= n) return;   // the whole wave
  const int64_t j = wave_first + lane;
  const bool active = j < n;
  const uint64_t key = keys[active ? j : wave_first];
  const uint32_t i = (uint32_t)(key & (((uint64_t)1 << idx_bits) - 1));
  const P3 p = reinterpret_cast<const P3*>(pts)[i];
  const bool valid = active && finite3(p);
  const double px = (double)p.x, py = (double)p.y, pz = (double)p.z;
  const double pscale = fmax(fabs(px), fmax(fabs(py), fabs(pz)));
  Best best{INFINITY, kNoTriangle, 0};
  unsigned long long evaluated = 0;
  if (n_groups > 0) {
    // the wave's own neighbourhood first: the last group whose first code is <= the code of the wave's first point
    const uint64_t code0 = keys[wave_first] >> idx_bits;
    int64_t lo = 0, hi = n_groups;   // group_code[lo] <= code0 < group_code[hi], with group_code[0] taken as -inf
    while (hi - lo > 1) {
      const int64_t mid = lo + (hi - lo) / 2;
      if (group_code[mid] <= code0) lo = mid;
      else hi = mid;
    }
    const int64_t seed = lo;
    visit_group(seed, tris, group_box, n_valid, px, py, pz, pscale, valid, best, evaluated);
    for (int64_t step = 1; seed - step >= 0 || seed + step < n_groups; ++step) {
      if (seed - step >= 0) visit_group(seed - step, tris, group_box, n_valid, px, py, pz, pscale, valid, best, evaluated);
      if (seed + step < n_groups) visit_group(seed + step, tris, group_box, n_valid, px, py, pz, pscale, valid, best, evaluated);
    }
  }
  if (counter && lane == 0) atomicAdd(counter, evaluated);
  if (!active) return;
  float d = INFINITY, q[3] = {__builtin_nanf(""), __builtin_nanf(""), __builtin_nanf("")};
  if (best.tri != kNoTriangle) {
    const float* T = tris + best.slot * kTriFloats;
    const Hit h = closest_on_triangle(px, py, pz, T);   // the winner again: the same bits
    d = (float)__dsqrt_rn(h.d2);
    if (flags & R3D_MESHDIST_SIGNED) {
      const double ax = (double)T[0], ay = (double)T[1], az = (double)T[2];
      const double abx = (double)T[3] - ax, aby = (double)T[4] - ay, abz = (double)T[5] - az;
      const double acx = (double)T[6] - ax, acy = (double)T[7] - ay, acz = (double)T[8] - az;
      const double nx = aby * acz - abz * acy, ny = abz * acx - abx * acz, nz = abx * acy - aby * acx;
      const double s = nx * (px - h.qx) + ny * (py - h.qy) + nz * (pz - h.qz);
      if (s < 0.0) d = -d;
    }
    q[0] = (float)h.qx, q[1] = (float)h.qy, q[2] = (float)h.qz;
  }
  dist_out[i] = d;
  if (tri_out) tri_out[i] = best.tri;
  if (closest_out) {
    closest_out[3 * (int64_t)i] = q[0];
    closest_out[3 * (int64_t)i + 1] = q[1];
    closest_out[3 * (int64_t)i + 2] = q[2];
  }
}

// ---- statistics -----------------------------------------------------------------------------------------------------------
struct StatsArgs {
  double thr[kMaxThresholds];
  double bin_width;
  int n_thr, n_bins, squared;
};

// Row r = elements [256 r, 256 r + 256), one per thread.  part_sums [rows][4] = {finite, non-finite, sum, sum of squares},
// part_mm [rows][2] = {min, max}; counts [8 + n_bins] u64.  sh: [8 + n_bins] u32 (a workgroup sees fewer than 2^32 elements).
__global__ __launch_bounds__(kThreads) void stats_rows_kernel(const float* __restrict__ v, int64_t n, int64_t n_rows, StatsArgs a,
                                                              double* __restrict__ part_sums, double* __restrict__ part_mm,
                                                              unsigned long long* __restrict__ counts) {
  extern __shared__ uint32_t sh[];
  __shared__ double red[kThreads / 64][4];
  __shared__ double mm[kThreads / 64][2];
  const int n_sh = kMaxThresholds + a.n_bins;
  for (int k = threadIdx.x; k < n_sh; k += kThreads) sh[k] = 0u;
  __syncthreads();
  for (int64_t row = blockIdx.x; row < n_rows; row += gridDim.x) {
    const int64_t i = row * kStatsRow + threadIdx.x;
    double acc[4] = {0.0, 0.0, 0.0, 0.0}, mn = INFINITY, mx = -INFINITY;
    if (i < n) {
      double x = (double)v[i];
      if (a.squared) x = __dsqrt_rn(x);
      if (x - x == 0.0) {
        acc[0] = 1.0;
        acc[2] = x;
        acc[3] = x * x;
        mn = mx = x;
        for (int t = 0; t < a.n_thr; ++t)
          if (x <= a.thr[t]) atomicAdd(sh + t, 1u);
        if (a.n_bins > 0) {
          const double q = floor(x / a.bin_width);
          const int top = a.n_bins - 1;
          const int bin = q >= (double)top ? top : q > 0.0 ? (int)q : 0;
          atomicAdd(sh + kMaxThresholds + bin, 1u);
        }
      } else {
        acc[1] = 1.0;
      }
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
      mn = fmin(mn, __shfl_down(mn, off, 64));
      mx = fmax(mx, __shfl_down(mx, off, 64));
    }
    if ((threadIdx.x & 63) == 0) {
      mm[threadIdx.x >> 6][0] = mn;
      mm[threadIdx.x >> 6][1] = mx;
    }
    r3d_sums::block_reduce_store<4>(acc, red, part_sums + row * 4);   // (its barrier publishes mm too)
    if (threadIdx.x == 64) {
      double lo = mm[0][0], hi = mm[0][1];
      for (int w = 1; w < kThreads / 64; ++w) {
        lo = fmin(lo, mm[w][0]);
        hi = fmax(hi, mm[w][1]);
      }
      part_mm[row * 2] = lo;
      part_mm[row * 2 + 1] = hi;
    }
    __syncthreads();   // red and mm are free again
  }
  for (int k = threadIdx.x; k < n_sh; k += kThreads)
    if (sh[k]) atomicAdd(counts + k, (unsigned long long)sh[k]);
}

// ONE workgroup: out[0..3] = the sums, out[4] = min + 0.0, out[5] = max + 0.0 (a zero is reported as +0)
__global__ __launch_bounds__(kThreads) void stats_finish_kernel(const double* __restrict__ part_sums, const double* __restrict__ part_mm,
                                                                int n_rows, double* __restrict__ out) {
  __shared__ double mm[kThreads / 64][2];
  r3d_sums::finish_rows<4>(part_sums, n_rows, out, (double*)nullptr, [](double*, double*, double*) { return 0; });
  double mn = INFINITY, mx = -INFINITY;
  for (int r = threadIdx.x; r < n_rows; r += kThreads) {
    mn = fmin(mn, part_mm[2 * (int64_t)r]);
    mx = fmax(mx, part_mm[2 * (int64_t)r + 1]);
  }
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    mn = fmin(mn, __shfl_down(mn, off, 64));
    mx = fmax(mx, __shfl_down(mx, off, 64));
  }
  if ((threadIdx.x & 63) == 0) {
    mm[threadIdx.x >> 6][0] = mn;
    mm[threadIdx.x >> 6][1] = mx;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    for (int w = 1; w < kThreads / 64; ++w) {
      mn = fmin(mn, mm[w][0]);
      mx = fmax(mx, mm[w][1]);
    }
    out[4] = mn + 0.0;
    out[5] = mx + 0.0;
  }
}

__global__ __launch_bounds__(kThreads) void sqrt_inplace_kernel(float* __restrict__ v, int64_t n) {
  const int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x;
  if (i < n) v[i] = (float)__dsqrt_rn((double)v[i]);
}

__global__ __launch_bounds__(kThreads) void colors_kernel(const float* __restrict__ d, int64_t n, double d_max, uint32_t* __restrict__ out) {
  const int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x;
  if (i >= n) return;
  const double x = fabs((double)d[i]);
  uint32_t r = 128u, g = 128u, b = 128u;
  if (x - x == 0.0) {
    double t = x / d_max;
    t = t < 1.0 ? t : 1.0;
    const uint32_t q = (uint32_t)floor(t * 765.0);   // 0 .. 765
    if (q <= 255u) r = 0u, g = q, b = 255u - q;                  // blue -> green
    else if (q <= 510u) r = q - 255u, g = 255u, b = 0u;          // green -> yellow
    else r = 255u, g = 255u - (q - 510u), b = 0u;                // yellow -> red
  }
  out[i] = r | (g << 8) | (b << 16);
}

int too_large(const char* what, int64_t a, int64_t b) {
  if (a > (int64_t)INT32_MAX || b > (int64_t)INT32_MAX) {
    r3d_set_error("%s take at most 2^31 - 1 items (got %lld and %lld)", what, (long long)a, (long long)b);
    return R3D_ERR_UNSUPPORTED;
  }
  return R3D_OK;
}

}  // namespace

extern "C" {

int r3d_mesh_index_destroy(r3d_mesh_index* ix) {
  if (!ix) return R3D_OK;
  (void)hipSetDevice(ix->device);
  (void)hipDeviceSynchronize();
  if (ix->d_slab) (void)hipFree(ix->d_slab);
  delete ix;
  return R3D_OK;
}

int r3d_mesh_index_create(r3d_ctx* ctx, const float* d_xyz, int64_t n_vertices, const int32_t* d_tri, int64_t n_triangles,
                          r3d_mesh_index** index_out) {
  R3D_REQUIRE(ctx != nullptr, "ctx is NULL");
  R3D_REQUIRE(index_out != nullptr, "index_out is NULL");
  *index_out = nullptr;
  R3D_REQUIRE(n_triangles >= 0 && n_vertices >= 0, "negative mesh size (%lld triangles, %lld vertices)", (long long)n_triangles,
              (long long)n_vertices);
  R3D_REQUIRE(n_triangles == 0 || d_tri != nullptr, "d_tri is NULL with n_triangles > 0");
  R3D_REQUIRE(n_vertices == 0 || d_xyz != nullptr, "d_xyz is NULL with n_vertices > 0");
  int rc = too_large("mesh indices", n_vertices, n_triangles);
  if (rc) return rc;
  if ((rc = r3d_ctx_enter(ctx))) return rc;
  r3d_mesh_index* ix = new (std::nothrow) r3d_mesh_index();
  if (!ix) {
    r3d_set_error("host allocation failed");
    return R3D_ERR_NOMEM;
  }
  ix->ctx = ctx;
  ix->device = ctx->device;
  const int64_t nt = n_triangles, max_groups = (nt + kGroup - 1) / kGroup;
  r3d_carve slab;
  const auto tri = slab.take<float>((size_t)max_groups * kGroup * kTriFloats), box = slab.take<float>((size_t)max_groups * 6);
  const auto code = slab.take<uint64_t>(max_groups);
  const auto frame = slab.take<float>(8);
  const auto bounds = slab.take<uint32_t>(6);
  const auto cnt = slab.take<unsigned long long>(2);
  hipError_t e = r3d_carve_malloc(slab, &ix->d_slab);
  if (e != hipSuccess) {
    r3d_mesh_index_destroy(ix);
    return r3d_fail_hip(e, "mesh index allocation", __FILE__, __LINE__);
  }
  ix->d_tri = slab.at(tri), ix->d_group_box = slab.at(box), ix->d_group_code = slab.at(code);
  ix->d_frame = slab.at(frame), ix->d_bounds = slab.at(bounds), ix->d_counters = slab.at(cnt);
  auto fail = [ix](int code) {
    r3d_mesh_index_destroy(ix);
    return code;
  };
  hipStream_t st = ctx->stream;
  hipLaunchKernelGGL(md_init_kernel, dim3(1), dim3(kThreads), 0, st, ix->d_bounds, ix->d_counters);
  if (nt > 0) {
    const uint32_t nv = (uint32_t)n_vertices;
    const int idx_bits = bits_for(nt);
    r3d_carve ws;
    const auto keys_h = ws.take<uint64_t>(nt), tmp_h = ws.take<uint64_t>(nt);
    if ((rc = r3d_scratch(ctx, kWsMeshDist, ws))) return fail(rc);
    uint64_t *keys = ws.at(keys_h), *tmp = ws.at(tmp_h);
    hipLaunchKernelGGL(md_bbox_kernel, dim3(blocks_of(nt)), dim3(kThreads), 0, st, d_xyz, nv, d_tri, nt, ix->d_bounds, ix->d_counters);
    hipLaunchKernelGGL(md_frame_kernel, dim3(1), dim3(64), 0, st, (const uint32_t*)ix->d_bounds, ix->d_frame);
    hipLaunchKernelGGL(md_keys_kernel, dim3(blocks_of(nt)), dim3(kThreads), 0, st, d_xyz, nv, d_tri, nt, (const float*)ix->d_frame, idx_bits,
                       keys);
    if ((e = hipGetLastError()) != hipSuccess) return fail(r3d_fail_hip(e, "mesh index build", __FILE__, __LINE__));
    // (the low idx_bits hold the triangle number, which already ascends: the stable sort skips those digits)
    if ((rc = r3d_radix_sort_u64(ctx, keys, tmp, nt, 3 * kAxisBits + 1 + idx_bits, idx_bits))) return fail(rc);
    unsigned long long n_valid = 0;
    if ((e = hipMemcpyAsync(&n_valid, ix->d_counters, sizeof n_valid, hipMemcpyDeviceToHost, st)) != hipSuccess ||
        (e = hipStreamSynchronize(st)) != hipSuccess)
      return fail(r3d_fail_hip(e, "mesh index build", __FILE__, __LINE__));
    ix->n_valid = (int64_t)n_valid;
    ix->n_groups = (ix->n_valid + kGroup - 1) / kGroup;
    if (ix->n_groups > 0) {
      const int64_t n_slots = ix->n_groups * kGroup;
      hipLaunchKernelGGL(md_gather_kernel, dim3(blocks_of(n_slots)), dim3(kThreads), 0, st, d_xyz, d_tri, (const uint64_t*)keys, ix->n_valid,
                         n_slots, idx_bits, ix->d_tri);
      hipLaunchKernelGGL(md_group_kernel, dim3(blocks_of(ix->n_groups)), dim3(kThreads), 0, st, (const float*)ix->d_tri, (const uint64_t*)keys,
                         ix->n_valid, ix->n_groups, idx_bits, ix->d_group_box, ix->d_group_code);
    }
  }
  // the caller may free or rewrite the mesh when this returns
  if ((e = hipGetLastError()) != hipSuccess || (e = hipStreamSynchronize(st)) != hipSuccess)
    return fail(r3d_fail_hip(e, "mesh index build", __FILE__, __LINE__));
  *index_out = ix;
  return R3D_OK;
}

int r3d_mesh_index_query(r3d_mesh_index* ix, const float* d_points, int64_t n_points, int flags, float* d_dist_out, uint32_t* d_tri_out,
                         float* d_closest_out, int64_t* h_groups_evaluated) {
  R3D_REQUIRE(ix != nullptr, "mesh index is NULL");
  R3D_REQUIRE(n_points >= 0, "negative n_points (%lld)", (long long)n_points);
  R3D_REQUIRE((flags & ~R3D_MESHDIST_SIGNED) == 0, "unknown flags 0x%x", flags);
  R3D_REQUIRE(n_points == 0 || d_points != nullptr, "d_points is NULL with n_points > 0");
  R3D_REQUIRE(n_points == 0 || d_dist_out != nullptr, "d_dist_out is NULL with n_points > 0");
  const int64_t n = n_points;
  const r3d_range outs[3] = {{d_dist_out, (size_t)n * 4}, {d_tri_out, (size_t)n * 4}, {d_closest_out, (size_t)n * 12}};
  const r3d_range ins[1] = {{d_points, (size_t)n * 12}};
  R3D_REQUIRE(!r3d_any_overlap(outs, 3, ins, 1), "an output overlaps the points or another output");
  int rc = too_large("mesh distance queries", n_points, 0);
  if (rc) return rc;
  r3d_ctx* ctx = ix->ctx;
  if ((rc = r3d_ctx_enter(ctx))) return rc;
  hipStream_t st = ctx->stream;
  if (n > 0) {
    const int idx_bits = bits_for(n);
    r3d_carve ws;
    const auto keys_h = ws.take<uint64_t>(n), tmp_h = ws.take<uint64_t>(n);
    if ((rc = r3d_scratch(ctx, kWsMeshDist, ws))) return rc;
    uint64_t *keys = ws.at(keys_h), *tmp = ws.at(tmp_h);
    hipLaunchKernelGGL(md_point_keys_kernel, dim3(blocks_of(n)), dim3(kThreads), 0, st, d_points, n, (const float*)ix->d_frame, idx_bits,
                       keys);
    R3D_HIP(hipGetLastError());
    if ((rc = r3d_radix_sort_u64(ctx, keys, tmp, n, 3 * kAxisBits + 1 + idx_bits, idx_bits))) return rc;
    unsigned long long* counter = h_groups_evaluated ? ix->d_counters + 1 : nullptr;
    if (counter) R3D_HIP(hipMemsetAsync(counter, 0, sizeof *counter, st));
    r3d_wrote(ctx, d_dist_out, (size_t)n * 4);
    if (d_tri_out) r3d_wrote(ctx, d_tri_out, (size_t)n * 4);
    if (d_closest_out) r3d_wrote(ctx, d_closest_out, (size_t)n * 12);
    hipLaunchKernelGGL(md_query_kernel, dim3(blocks_of(n)), dim3(kThreads), 0, st, d_points, (const uint64_t*)keys, n, idx_bits,
                       (const float*)ix->d_tri, (const float*)ix->d_group_box, (const uint64_t*)ix->d_group_code, ix->n_valid, ix->n_groups,
                       flags, d_dist_out, d_tri_out, d_closest_out, counter);
    R3D_HIP(hipGetLastError());
  }
  if (h_groups_evaluated) {
    unsigned long long c = 0;
    if (n > 0) {
      R3D_HIP(hipMemcpyAsync(&c, ix->d_counters + 1, sizeof c, hipMemcpyDeviceToHost, st));
      R3D_HIP(hipStreamSynchronize(st));
    }
    *h_groups_evaluated = (int64_t)c;
  }
  return R3D_OK;
}

int r3d_distance_stats(r3d_ctx* ctx, const float* d_values, int64_t n, int squared_input, const double* h_thresholds, int n_thresholds,
                       double bin_width, int n_bins, double* h_stats_out, int64_t* h_count_le_out, uint64_t* h_hist_out) {
  R3D_REQUIRE(ctx != nullptr, "ctx is NULL");
  R3D_REQUIRE(n >= 0, "negative n (%lld)", (long long)n);
  R3D_REQUIRE(n == 0 || d_values != nullptr, "d_values is NULL with n > 0");
  R3D_REQUIRE(h_stats_out != nullptr, "h_stats_out is NULL");
  R3D_REQUIRE(n_thresholds >= 0 && n_thresholds <= kMaxThresholds, "n_thresholds must be in [0, %d] (got %d)", kMaxThresholds, n_thresholds);
  R3D_REQUIRE(n_thresholds == 0 || (h_thresholds != nullptr && h_count_le_out != nullptr), "h_thresholds or h_count_le_out is NULL");
  R3D_REQUIRE(n_bins >= 0 && n_bins <= kMaxBins, "n_bins must be in [0, %d] (got %d)", kMaxBins, n_bins);
  R3D_REQUIRE(n_bins == 0 || h_hist_out != nullptr, "h_hist_out is NULL with n_bins > 0");
  R3D_REQUIRE(n_bins == 0 || (bin_width > 0.0 && std::isfinite(bin_width)), "bin_width must be finite and > 0 (got %g)", bin_width);
  StatsArgs a{};
  for (int t = 0; t < n_thresholds; ++t) {
    R3D_REQUIRE(!std::isnan(h_thresholds[t]), "threshold %d is NaN", t);
    a.thr[t] = h_thresholds[t];
  }
  a.bin_width = n_bins ? bin_width : 1.0;
  a.n_thr = n_thresholds;
  a.n_bins = n_bins;
  a.squared = squared_input != 0;
  int rc = too_large("distance statistics", n, 0);
  if (rc) return rc;
  if ((rc = r3d_ctx_enter(ctx))) return rc;
  double stats[6] = {0.0, 0.0, 0.0, 0.0, INFINITY, -INFINITY};
  unsigned long long counts[kMaxThresholds + kMaxBins] = {};
  if (n > 0) {
    const int64_t n_rows = (n + kStatsRow - 1) / kStatsRow;
    const int n_counts = kMaxThresholds + n_bins;
    const size_t b_counts = (size_t)n_counts * 8;
    r3d_carve ws;
    const auto sums_h = ws.take<double>((size_t)n_rows * 4), mm_h = ws.take<double>((size_t)n_rows * 2), out_h = ws.take<double>(8);
    const auto counts_h = ws.take<unsigned long long>(n_counts);   // read back by a copy of its own
    if ((rc = r3d_scratch(ctx, kWsMeshDist, ws))) return rc;
    double *part_sums = ws.at(sums_h), *part_mm = ws.at(mm_h), *out = ws.at(out_h);
    unsigned long long* d_counts = ws.at(counts_h);
    hipStream_t st = ctx->stream;
    R3D_HIP(hipMemsetAsync(d_counts, 0, b_counts, st));
    const int64_t max_blocks = (int64_t)ctx->num_cus * 4;
    hipLaunchKernelGGL(stats_rows_kernel, dim3((unsigned)(n_rows < max_blocks ? n_rows : max_blocks)), dim3(kThreads),
                       (size_t)n_counts * sizeof(uint32_t), st, d_values, n, n_rows, a, part_sums, part_mm, d_counts);
    hipLaunchKernelGGL(stats_finish_kernel, dim3(1), dim3(kThreads), 0, st, (const double*)part_sums, (const double*)part_mm, (int)n_rows, out);
    R3D_HIP(hipGetLastError());
    R3D_HIP(hipMemcpyAsync(stats, out, sizeof stats, hipMemcpyDeviceToHost, st));
    R3D_HIP(hipMemcpyAsync(counts, d_counts, b_counts, hipMemcpyDeviceToHost, st));
    R3D_HIP(hipStreamSynchronize(st));
  }
  for (int k = 0; k < 6; ++k) h_stats_out[k] = stats[k];
  for (int t = 0; t < n_thresholds; ++t) h_count_le_out[t] = (int64_t)counts[t];
  for (int b = 0; b < n_bins; ++b) h_hist_out[b] = (uint64_t)counts[kMaxThresholds + b];
  return R3D_OK;
}

int r3d_sqrt_f32_inplace(r3d_ctx* ctx, float* d_values, int64_t n) {
  R3D_REQUIRE(ctx != nullptr, "ctx is NULL");
  R3D_REQUIRE(n >= 0, "negative n (%lld)", (long long)n);
  R3D_REQUIRE(n == 0 || d_values != nullptr, "d_values is NULL with n > 0");
  int rc = too_large("roots", n, 0);
  if (rc) return rc;
  if ((rc = r3d_ctx_enter(ctx))) return rc;
  if (n == 0) return R3D_OK;
  r3d_wrote(ctx, d_values, (size_t)n * 4);
  hipLaunchKernelGGL(sqrt_inplace_kernel, dim3(blocks_of(n)), dim3(kThreads), 0, ctx->stream, d_values, n);
  R3D_HIP(hipGetLastError());
  return R3D_OK;
}

int r3d_distance_colors(r3d_ctx* ctx, const float* d_dist, int64_t n, double d_max, uint32_t* d_rgba_out) {
  R3D_REQUIRE(ctx != nullptr, "ctx is NULL");
  R3D_REQUIRE(n >= 0, "negative n (%lld)", (long long)n);
  R3D_REQUIRE(n == 0 || (d_dist != nullptr && d_rgba_out != nullptr), "d_dist or d_rgba_out is NULL with n > 0");
  R3D_REQUIRE(d_max > 0.0 && std::isfinite(d_max), "d_max must be finite and > 0 (got %g)", d_max);
  R3D_REQUIRE(!r3d_ranges_overlap(d_dist, (size_t)n * 4, d_rgba_out, (size_t)n * 4), "the output overlaps the distances");
  int rc = too_large("distance colours", n, 0);
  if (rc) return rc;
  if ((rc = r3d_ctx_enter(ctx))) return rc;
  if (n == 0) return R3D_OK;
  r3d_wrote(ctx, d_rgba_out, (size_t)n * 4);
  hipLaunchKernelGGL(colors_kernel, dim3(blocks_of(n)), dim3(kThreads), 0, ctx->stream, d_dist, n, d_max, d_rgba_out);
  R3D_HIP(hipGetLastError());
  return R3D_OK;
}

}  // extern "C"
