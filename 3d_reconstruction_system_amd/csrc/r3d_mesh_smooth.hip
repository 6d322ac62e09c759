// Mesh smoothing for gfx950 (MI355X), the kernels: vertex adjacency (one-ring CSR and boundary flags), umbrella steps (Laplacian,
// Taubin) and area-weighted vertex normals of an indexed triangle mesh.  NOT IN THE REFERENCE; include/r3d.h ("Mesh smoothing") is
// the specification, tests/mesh_smooth_ref.py restates it in NumPy.  The entry points -- checks, the workspace, the sorts, the
// sequencing -- are in r3d_mesh_smooth_host.cpp; this file claims no workspace.  Timed once, without a gate (DESIGN.md 4.5j'').
//
// adjacency -- integer-exact, whatever the launch geometry or the order of the triangles:
//   ms_side_keys_kernel    a thread per triangle: six keys (u << vb | v), both directions of its three sides, vb = the bits of a
//                          vertex index; an invalid triangle and a side with u == v give the key 1 << 2vb, which sorts last
//   (r3d_radix_sort_u64 over the 2vb + 1 bits in use)
//   ms_heads_count_kernel / ms_heads_write_kernel   run heads = the distinct (u, v), compacted in order (r3d_compact_dev.h) into the
//                          workspace; a run of length 1 is an edge one side has: boundary[u] = 1 (every writer stores the same byte)
//   ms_rows_kernel         row_start[u] = the lower bound of u << vb among the distinct keys; neighbours[i] = the low vb bits
// smoothing -- ms_step_kernel, a lane per vertex and a launch per step: the lane walks its row in ascending index and sums the
//   neighbours' positions in fp64 in that order, so no bit depends on the launch geometry; no atomics, no LDS.  Roofline: per
//   vertex 12 B own + 4 B row_start + deg x (4 B index + 12 B gather) + 12 B store; marching-cubes vertices come in voxel-linear
//   order, so the gathers of a wave fall into a few rows and slabs and are mostly L2 hits.  Rows are packed [n][3] f32 everywhere:
//   a gather is one global_load_dwordx3 (DESIGN.md 4.5j'').
// normals -- ms_corner_keys_kernel: (v << 32 | 3t + c) per corner, sorted on the v bits alone, so the stable sort leaves a vertex's
//   corners in ascending triangle; ms_normals_kernel: a lane per vertex finds its run by lower bound and adds the face normals in
//   fp64 in that order.
#include "r3d_compact_dev.h"
#include "r3d_internal.h"
#include "r3d_mesh_dev.h"

using namespace r3d_compact;   // kPer consecutive items per thread of the compaction kernels
using r3d_mesh::tri_valid;

namespace {

constexpr int kThreads = 256;

inline unsigned blocks_of(int64_t n) { return (unsigned)((n + kThreads - 1) / kThreads); }

__global__ __launch_bounds__(kThreads) void ms_side_keys_kernel(const int32_t* __restrict__ tri, int64_t nt, uint32_t nv, int vb,
                                                                uint64_t* __restrict__ keys) {
  const int64_t t = (int64_t)blockIdx.x * kThreads + threadIdx.x;
  if (t >= nt) return;
  const int32_t idx[3] = {tri[3 * t], tri[3 * t + 1], tri[3 * t + 2]};
  const bool ok = tri_valid(idx[0], idx[1], idx[2], nv);
  const uint64_t none = 1ull << (2 * vb);
#pragma unroll
  for (int s = 0; s < 3; ++s) {
    const uint64_t u = (uint32_t)idx[s], v = (uint32_t)idx[(s + 1) % 3];
    const bool side = ok && u != v;
    keys[6 * t + 2 * s] = side ? (u << vb) | v : none;
    keys[6 * t + 2 * s + 1] = side ? (v << vb) | u : none;
  }
}

// is sorted[i] the first of a run of equal keys of a side?
__device__ __forceinline__ bool is_head(const uint64_t* __restrict__ sorted, int64_t i, uint64_t none) {
  const uint64_t k = sorted[i];
  return k < none && (i == 0 || sorted[i - 1] != k);
}

__global__ __launch_bounds__(kThreads) void ms_heads_count_kernel(const uint64_t* __restrict__ sorted, int64_t n, int vb,
                                                                  uint32_t* __restrict__ hist) {
  __shared__ uint32_t sh[kThreads / 64];
  const uint64_t none = 1ull << (2 * vb);
  const int64_t base = tile_base();
  uint32_t c = 0;
  for (int e = 0; e < kPer; ++e)
    if (base + e < n && is_head(sorted, base + e, none)) ++c;
  publish(hist, block_sum(c, sh));
}

// hist: the tiles' exclusive prefixes.  distinct holds as many keys as sorted: every head has its place.
__global__ __launch_bounds__(kThreads) void ms_heads_write_kernel(const uint64_t* __restrict__ sorted, int64_t n, int vb,
                                                                  const uint32_t* __restrict__ hist, uint64_t* __restrict__ distinct,
                                                                  uint8_t* __restrict__ boundary) {
  __shared__ uint64_t wave_total[kThreads / 64];
  const uint64_t none = 1ull << (2 * vb);
  const int64_t base = tile_base();
  uint32_t flags = 0;
  for (int e = 0; e < kPer; ++e)
    if (base + e < n && is_head(sorted, base + e, none)) flags |= 1u << e;
  uint64_t at = tile_start(hist, (uint64_t)__popc(flags), wave_total);
  for (int e = 0; e < kPer; ++e) {
    if (!((flags >> e) & 1u)) continue;
    const int64_t i = base + e;
    const uint64_t k = sorted[i];
    distinct[at++] = k;
    if (boundary && (i + 1 == n || sorted[i + 1] != k)) boundary[k >> vb] = 1;   // k < none: k >> vb is a valid vertex
  }
}

// thread i: row_start[i] for i <= nv, neighbours[i] for i < rows (rows <= n_distinct)
__global__ __launch_bounds__(kThreads) void ms_rows_kernel(const uint64_t* __restrict__ distinct, uint32_t n_distinct, uint32_t nv, int vb,
                                                           uint32_t* __restrict__ row_start, uint32_t* __restrict__ neighbours,
                                                           uint32_t rows) {
  const int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x;
  if (i <= (int64_t)nv) {
    const uint64_t want = (uint64_t)i << vb;   // the first key of vertex i; i == nv: above every key
    uint32_t lo = 0, hi = n_distinct;
    while (lo < hi) {
      const uint32_t mid = lo + (hi - lo) / 2;
      if (distinct[mid] < want) lo = mid + 1;
      else hi = mid;
    }
    row_start[i] = lo;
  }
  if (i < (int64_t)rows) neighbours[i] = (uint32_t)(distinct[i] & ((1ull << vb) - 1));
}

// One umbrella step (include/r3d.h "Mesh smoothing"), a lane per vertex.  in and out are different arrays.
__global__ __launch_bounds__(kThreads) void ms_step_kernel(const float* __restrict__ in, float* __restrict__ out, uint32_t nv,
                                                           const uint32_t* __restrict__ row_start, const uint32_t* __restrict__ neighbours,
                                                           const uint8_t* __restrict__ locked, double f) {
  const uint32_t i = blockIdx.x * kThreads + threadIdx.x;
  if (i >= nv) return;
  const uint32_t r0 = row_start[i], r1 = row_start[i + 1];
  const float px = in[3 * (size_t)i], py = in[3 * (size_t)i + 1], pz = in[3 * (size_t)i + 2];
  float ox = px, oy = py, oz = pz;   // a vertex that does not move keeps its bits
  if (r1 > r0 && !(locked && locked[i])) {
    uint32_t j = neighbours[r0];
    double sx = (double)in[3 * (size_t)j], sy = (double)in[3 * (size_t)j + 1], sz = (double)in[3 * (size_t)j + 2];
    for (uint32_t r = r0 + 1; r < r1; ++r) {
      j = neighbours[r];
      sx += (double)in[3 * (size_t)j];
      sy += (double)in[3 * (size_t)j + 1];
      sz += (double)in[3 * (size_t)j + 2];
    }
    const double d = (double)(r1 - r0);
    const double mx = sx / d, my = sy / d, mz = sz / d;
    ox = (float)((double)px + f * (mx - (double)px));
    oy = (float)((double)py + f * (my - (double)py));
    oz = (float)((double)pz + f * (mz - (double)pz));
  }
  out[3 * (size_t)i] = ox;
  out[3 * (size_t)i + 1] = oy;
  out[3 * (size_t)i + 2] = oz;
}

__global__ __launch_bounds__(kThreads) void ms_corner_keys_kernel(const int32_t* __restrict__ tri, int64_t nt, uint32_t nv, int vb,
                                                                  uint64_t* __restrict__ keys) {
  const int64_t t = (int64_t)blockIdx.x * kThreads + threadIdx.x;
  if (t >= nt) return;
  const int32_t idx[3] = {tri[3 * t], tri[3 * t + 1], tri[3 * t + 2]};
  const bool ok = tri_valid(idx[0], idx[1], idx[2], nv);
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    const uint64_t v = ok ? (uint64_t)(uint32_t)idx[c] : 1ull << vb;   // an invalid triangle's corners sort behind every vertex
    keys[3 * t + c] = (v << 32) | (uint64_t)(3 * t + c);
  }
}

// sorted: the corner keys by vertex, a vertex's corners in ascending 3t + c; every key below 2^vb << 32 names a valid triangle
__global__ __launch_bounds__(kThreads) void ms_normals_kernel(const float* __restrict__ xyz, uint32_t nv, const int32_t* __restrict__ tri,
                                                              const uint64_t* __restrict__ sorted, uint32_t n_keys,
                                                              const float* __restrict__ fallback, float* __restrict__ out) {
  const uint32_t i = blockIdx.x * kThreads + threadIdx.x;
  if (i >= nv) return;
  uint32_t lo = 0, hi = n_keys;
  while (lo < hi) {
    const uint32_t mid = lo + (hi - lo) / 2;
    if ((uint32_t)(sorted[mid] >> 32) < i) lo = mid + 1;
    else hi = mid;
  }
  double sx = 0.0, sy = 0.0, sz = 0.0;
  for (uint32_t k = lo; k < n_keys; ++k) {
    const uint64_t key = sorted[k];
    if ((uint32_t)(key >> 32) != i) break;
    const size_t t = (uint32_t)key / 3u;
    const size_t a = (size_t)tri[3 * t], b = (size_t)tri[3 * t + 1], c = (size_t)tri[3 * t + 2];
    const double ax = (double)xyz[3 * a], ay = (double)xyz[3 * a + 1], az = (double)xyz[3 * a + 2];
    const double e1x = (double)xyz[3 * b] - ax, e1y = (double)xyz[3 * b + 1] - ay, e1z = (double)xyz[3 * b + 2] - az;
    const double e2x = (double)xyz[3 * c] - ax, e2y = (double)xyz[3 * c + 1] - ay, e2z = (double)xyz[3 * c + 2] - az;
    sx += e1y * e2z - e1z * e2y;
    sy += e1z * e2x - e1x * e2z;
    sz += e1x * e2y - e1y * e2x;
  }
  const double len = sqrt((sx * sx + sy * sy) + sz * sz);
  float ox = 0.0f, oy = 0.0f, oz = 0.0f;
  if (len > 0.0 && len < (double)INFINITY) {
    ox = (float)(sx / len);
    oy = (float)(sy / len);
    oz = (float)(sz / len);
  } else if (fallback) {
    ox = fallback[3 * (size_t)i];
    oy = fallback[3 * (size_t)i + 1];
    oz = fallback[3 * (size_t)i + 2];
  }
  out[3 * (size_t)i] = ox;
  out[3 * (size_t)i + 1] = oy;
  out[3 * (size_t)i + 2] = oz;
}

}  // namespace

void r3d_mesh_side_keys_launch(r3d_ctx* ctx, const int32_t* d_tri, int64_t nt, uint32_t nv, int vb, uint64_t* d_keys) {
  hipLaunchKernelGGL(ms_side_keys_kernel, dim3(blocks_of(nt)), dim3(kThreads), 0, ctx->stream, d_tri, nt, nv, vb, d_keys);
}

void r3d_mesh_heads_count_launch(r3d_ctx* ctx, const uint64_t* d_sorted, int64_t n, int vb, int tiles, uint32_t* hist) {
  hipLaunchKernelGGL(ms_heads_count_kernel, dim3(tiles), dim3(kThreads), 0, ctx->stream, d_sorted, n, vb, hist);
}

void r3d_mesh_heads_write_launch(r3d_ctx* ctx, const uint64_t* d_sorted, int64_t n, int vb, int tiles, const uint32_t* hist,
                                 uint64_t* d_distinct, uint8_t* d_boundary) {
  hipLaunchKernelGGL(ms_heads_write_kernel, dim3(tiles), dim3(kThreads), 0, ctx->stream, d_sorted, n, vb, hist, d_distinct, d_boundary);
}

void r3d_mesh_rows_launch(r3d_ctx* ctx, const uint64_t* d_distinct, uint32_t n_distinct, uint32_t nv, int vb, uint32_t* d_row_start,
                          uint32_t* d_neighbours, uint32_t rows) {
  const int64_t threads = (int64_t)nv + 1 > (int64_t)rows ? (int64_t)nv + 1 : (int64_t)rows;
  hipLaunchKernelGGL(ms_rows_kernel, dim3(blocks_of(threads)), dim3(kThreads), 0, ctx->stream, d_distinct, n_distinct, nv, vb, d_row_start,
                     d_neighbours, rows);
}

void r3d_mesh_step_launch(r3d_ctx* ctx, const float* d_in, float* d_out, uint32_t nv, const uint32_t* d_row_start,
                          const uint32_t* d_neighbours, const uint8_t* d_locked, double factor) {
  hipLaunchKernelGGL(ms_step_kernel, dim3(blocks_of(nv)), dim3(kThreads), 0, ctx->stream, d_in, d_out, nv, d_row_start, d_neighbours,
                     d_locked, factor);
}

void r3d_mesh_corner_keys_launch(r3d_ctx* ctx, const int32_t* d_tri, int64_t nt, uint32_t nv, int vb, uint64_t* d_keys) {
  hipLaunchKernelGGL(ms_corner_keys_kernel, dim3(blocks_of(nt)), dim3(kThreads), 0, ctx->stream, d_tri, nt, nv, vb, d_keys);
}

void r3d_mesh_normals_launch(r3d_ctx* ctx, const float* d_xyz, uint32_t nv, const int32_t* d_tri, const uint64_t* d_sorted, uint32_t n_keys,
                             const float* d_fallback, float* d_out) {
  hipLaunchKernelGGL(ms_normals_kernel, dim3(blocks_of(nv)), dim3(kThreads), 0, ctx->stream, d_xyz, nv, d_tri, d_sorted, n_keys, d_fallback,
                     d_out);
}
