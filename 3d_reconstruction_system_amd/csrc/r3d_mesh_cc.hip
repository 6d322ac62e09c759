// Connected components of an indexed triangle mesh for gfx950 (MI355X): label, count, drop small pieces.  NOT IN THE REFERENCE;
// include/r3d.h ("Mesh components") is the specification.  Everything here is integer-exact: the same bits whatever the launch
// geometry, the scheduling or the order of the triangles.
//
// r3d_mesh_components -- roofline: latency of dependent random reads into the label array (4 B per vertex); the triangles stream
//   once per pass (12 B each).  Marching-cubes order keeps a triangle's three indices, and consecutive triangles, close together,
//   so a thread takes triangle t and a wave touches a few cache lines of the array.
//   cc_init_kernel     label[v] = v
//   cc_hook_kernel     a thread per triangle: indices checked, then hook(a, b), hook(a, c) -- lock-free union-find with atomicMin
//                      hooks and path halving (r3d_unionfind_dev.h); nobody waits for anybody
//   cc_flatten_kernel  (next launch: the roots are final) label[v] = its root, in place
//   cc_count_kernel    triangle labels; vertices and valid triangles per label with integer atomics, one add per wave and label
//                      where the lanes agree (they mostly do)
//   cc_rows_*          components = roots with a triangle, compacted in ascending label (r3d_compact_dev.h)
// r3d_mesh_filter_components -- recounts per label, picks the largest with one 64-bit atomicMax per root, marks the vertices of the
//   kept triangles, and compacts vertices and triangles in order by the same step, both rows of counters in one scan (no cursor).
// Workspace: kWsMeshCc of the context, grown on demand, touched by these two synchronous calls alone.
#include "r3d_compact_dev.h"
#include "r3d_internal.h"
#include "r3d_mesh_dev.h"
#include "r3d_unionfind_dev.h"

using namespace r3d_compact;   // kPer consecutive items per thread of the compaction kernels

namespace {

constexpr int kThreads = 256;
constexpr uint32_t kNoLabel = 0xFFFFFFFFu;

using r3d_mesh::tri_valid;   // all three indices in [0, nv) (r3d_mesh_dev.h: the smoothing kernels take the same rule)

// cnt[label] += 1 for the active lanes; every lane of the wave calls this.  The lanes that share the first active lane's label
// add once, together; the others add for themselves.  Integer adds: the sums do not depend on who adds.
__device__ __forceinline__ void count_label(uint32_t* __restrict__ cnt, uint32_t label, bool active) {
  const unsigned long long act = __ballot(active);
  if (!act) return;
  const int lane = threadIdx.x & 63, leader = __ffsll((long long)act) - 1;
  const uint32_t first = (uint32_t)__shfl((int)label, leader, 64);
  const unsigned long long same = __ballot(active && label == first);
  if (!active) return;
  if (label != first) atomicAdd(cnt + label, 1u);
  else if (lane == leader) atomicAdd(cnt + first, (uint32_t)__popcll(same));
}

__global__ __launch_bounds__(kThreads) void cc_init_kernel(uint32_t* __restrict__ label, uint32_t nv) {
  const uint32_t v = blockIdx.x * kThreads + threadIdx.x;
  if (v < nv) label[v] = v;
}

__global__ __launch_bounds__(kThreads) void cc_hook_kernel(const int32_t* __restrict__ tri, int64_t nt, uint32_t nv, uint32_t* label,
                                                           uint32_t* __restrict__ n_invalid) {
  const int64_t t = (int64_t)blockIdx.x * kThreads + threadIdx.x;
  if (t >= nt) return;
  const int32_t a = tri[3 * t], b = tri[3 * t + 1], c = tri[3 * t + 2];
  if (!tri_valid(a, b, c, nv)) {   // checked before any index becomes an address
    atomicAdd(n_invalid, 1u);
    return;
  }
  if (a != b) r3d_uf::hook(label, (uint32_t)a, (uint32_t)b);
  if (a != c) r3d_uf::hook(label, (uint32_t)a, (uint32_t)c);
}

// In place: another lane reads either this vertex's old parent or its root -- both ancestors, and the roots no longer move.
__global__ __launch_bounds__(kThreads) void cc_flatten_kernel(uint32_t* label, uint32_t nv) {
  const uint32_t v = blockIdx.x * kThreads + threadIdx.x;
  if (v >= nv) return;
  const uint32_t r = r3d_uf::find_root(label, v);
  __hip_atomic_store(label + v, r, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// thread i: triangle i and vertex i.  cnt_v / cnt_t may be NULL (the filter recounts triangles only).  A label >= nv (labels are
// data for the filter) makes the triangle invalid: it is never used as an address.
__global__ __launch_bounds__(kThreads) void cc_count_kernel(const int32_t* __restrict__ tri, int64_t nt, uint32_t nv,
                                                            const uint32_t* __restrict__ label, uint32_t* __restrict__ tri_label,
                                                            uint32_t* __restrict__ cnt_v, uint32_t* __restrict__ cnt_t) {
  const int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x;
  uint32_t l = kNoLabel;
  if (i < nt) {
    const int32_t a = tri[3 * i], b = tri[3 * i + 1], c = tri[3 * i + 2];
    if (tri_valid(a, b, c, nv)) l = label[a];
    if (l >= nv) l = kNoLabel;
    if (tri_label) tri_label[i] = l;
  }
  count_label(cnt_t, l, l != kNoLabel);
  if (cnt_v) {
    const uint32_t lv = i < (int64_t)nv ? label[i] : kNoLabel;
    count_label(cnt_v, lv, lv < nv);
  }
}

__device__ __forceinline__ bool is_component(const uint32_t* __restrict__ label, const uint32_t* __restrict__ cnt_t, int64_t v) {
  return label[v] == (uint32_t)v && cnt_t[v] > 0;
}

__global__ __launch_bounds__(kThreads) void cc_rows_count_kernel(const uint32_t* __restrict__ label, const uint32_t* __restrict__ cnt_t,
                                                                 int64_t nv, uint32_t* __restrict__ hist) {
  __shared__ uint32_t sh[kThreads / 64];
  const int64_t base = tile_base();
  uint32_t n = 0;
  for (int e = 0; e < kPer; ++e)
    if (base + e < nv && is_component(label, cnt_t, base + e)) ++n;
  publish(hist, block_sum(n, sh));
}

// hist: the tiles' exclusive prefixes
__global__ __launch_bounds__(kThreads) void cc_rows_write_kernel(const uint32_t* __restrict__ label, const uint32_t* __restrict__ cnt_v,
                                                                 const uint32_t* __restrict__ cnt_t, int64_t nv,
                                                                 const uint32_t* __restrict__ hist, uint32_t* __restrict__ rows, uint64_t cap) {
  __shared__ uint64_t wave_total[kThreads / 64];
  const int64_t base = tile_base();
  uint32_t flags = 0;
  for (int e = 0; e < kPer; ++e)
    if (base + e < nv && is_component(label, cnt_t, base + e)) flags |= 1u << e;
  uint64_t at = tile_start(hist, (uint64_t)__popc(flags), wave_total);
  for (int e = 0; e < kPer && at < cap; ++e) {
    if (!((flags >> e) & 1u)) continue;
    rows[3 * at] = (uint32_t)(base + e);
    rows[3 * at + 1] = cnt_v[base + e];
    rows[3 * at + 2] = cnt_t[base + e];
    ++at;
  }
}

// best = max over the roots with a triangle of (count << 32 | ~label): the greatest count, ties to the smallest label
__global__ __launch_bounds__(kThreads) void cc_best_kernel(const uint32_t* __restrict__ cnt_t, uint32_t nv, unsigned long long* __restrict__ best) {
  const uint32_t v = blockIdx.x * kThreads + threadIdx.x;
  if (v >= nv) return;
  const uint32_t c = cnt_t[v];
  if (c) atomicMax(best, ((unsigned long long)c << 32) | (unsigned long long)(~v));
}

struct Keep {
  int64_t min_triangles;
  int largest;
};

// is triangle t kept?  (a, b, c) come back for the caller
__device__ __forceinline__ bool tri_kept(const int32_t* __restrict__ tri, int64_t t, uint32_t nv, const uint32_t* __restrict__ label,
                                         const uint32_t* __restrict__ cnt_t, unsigned long long best, Keep k, int32_t (&idx)[3]) {
  idx[0] = tri[3 * t];
  idx[1] = tri[3 * t + 1];
  idx[2] = tri[3 * t + 2];
  if (!tri_valid(idx[0], idx[1], idx[2], nv)) return false;
  const uint32_t l = label[idx[0]];
  if (l >= nv) return false;
  if ((int64_t)cnt_t[l] < k.min_triangles) return false;
  return !k.largest || l == ~(uint32_t)best;
}

// vflag[v] = 1 for every vertex a kept triangle names (all writers store the same word); hist_t[tile] = kept triangles
__global__ __launch_bounds__(kThreads) void cc_mark_kernel(const int32_t* __restrict__ tri, int64_t nt, uint32_t nv,
                                                           const uint32_t* __restrict__ label, const uint32_t* __restrict__ cnt_t,
                                                           const unsigned long long* __restrict__ best, Keep k,
                                                           uint32_t* __restrict__ vflag, uint32_t* __restrict__ hist_t) {
  __shared__ uint32_t sh[kThreads / 64];
  const unsigned long long bw = *best;
  const int64_t base = tile_base();
  uint32_t n = 0;
  for (int e = 0; e < kPer; ++e) {
    int32_t idx[3];
    if (base + e < nt && tri_kept(tri, base + e, nv, label, cnt_t, bw, k, idx)) {
      ++n;
      vflag[idx[0]] = 1u;
      vflag[idx[1]] = 1u;
      vflag[idx[2]] = 1u;
    }
  }
  publish(hist_t, block_sum(n, sh));
}

__global__ __launch_bounds__(kThreads) void cc_vertex_count_kernel(const uint32_t* __restrict__ vflag, int64_t nv, uint32_t* __restrict__ hist_v) {
  __shared__ uint32_t sh[kThreads / 64];
  const int64_t base = tile_base();
  uint32_t n = 0;
  for (int e = 0; e < kPer; ++e)
    if (base + e < nv && vflag[base + e]) ++n;
  publish(hist_v, block_sum(n, sh));
}

// vflag[v] becomes v's new index where v is kept (a thread reads its own 16 words, then writes them); kept_out[new] = old
__global__ __launch_bounds__(kThreads) void cc_vertex_write_kernel(uint32_t* __restrict__ vflag, int64_t nv, const uint32_t* __restrict__ hist_v,
                                                                   uint32_t* __restrict__ kept_out, uint64_t cap) {
  __shared__ uint64_t wave_total[kThreads / 64];
  const int64_t base = tile_base();
  uint32_t flags = 0;
  for (int e = 0; e < kPer; ++e)
    if (base + e < nv && vflag[base + e]) flags |= 1u << e;
  uint64_t at = tile_start(hist_v, (uint64_t)__popc(flags), wave_total);
  for (int e = 0; e < kPer; ++e) {
    if (!((flags >> e) & 1u)) continue;
    vflag[base + e] = (uint32_t)at;
    if (at < cap) kept_out[at] = (uint32_t)(base + e);
    ++at;
  }
}

// newidx = vflag after cc_vertex_write_kernel
__global__ __launch_bounds__(kThreads) void cc_tri_write_kernel(const int32_t* __restrict__ tri, int64_t nt, uint32_t nv,
                                                                const uint32_t* __restrict__ label, const uint32_t* __restrict__ cnt_t,
                                                                const unsigned long long* __restrict__ best, Keep k,
                                                                const uint32_t* __restrict__ newidx, const uint32_t* __restrict__ hist_t,
                                                                int32_t* __restrict__ tri_out, uint64_t cap) {
  __shared__ uint64_t wave_total[kThreads / 64];
  const unsigned long long bw = *best;
  const int64_t base = tile_base();
  uint32_t flags = 0;
  for (int e = 0; e < kPer; ++e) {
    int32_t idx[3];
    if (base + e < nt && tri_kept(tri, base + e, nv, label, cnt_t, bw, k, idx)) flags |= 1u << e;
  }
  uint64_t at = tile_start(hist_t, (uint64_t)__popc(flags), wave_total);
  for (int e = 0; e < kPer && at < cap; ++e) {
    if (!((flags >> e) & 1u)) continue;
    const int64_t t = base + e;   // kept: its three indices are < nv
    tri_out[3 * at] = (int32_t)newidx[tri[3 * t]];
    tri_out[3 * at + 1] = (int32_t)newidx[tri[3 * t + 1]];
    tri_out[3 * at + 2] = (int32_t)newidx[tri[3 * t + 2]];
    ++at;
  }
}

inline unsigned blocks_of(int64_t n) { return (unsigned)((n + kThreads - 1) / kThreads); }

// what both calls check of the mesh itself, before anything else; the size limit (check_size) comes after every R3D_ERR_INVALID
int check_mesh(const r3d_ctx* ctx, const int32_t* d_tri, int64_t n_triangles, int64_t n_vertices) {
  R3D_REQUIRE(ctx != nullptr, "ctx is NULL");
  R3D_REQUIRE(n_triangles >= 0 && n_vertices >= 0, "negative mesh size (%lld triangles, %lld vertices)", (long long)n_triangles,
              (long long)n_vertices);
  R3D_REQUIRE(n_triangles == 0 || d_tri != nullptr, "d_tri is NULL with n_triangles > 0");
  return R3D_OK;
}

int check_size(int64_t n_triangles, int64_t n_vertices) {
  if (n_vertices > (int64_t)INT32_MAX || n_triangles > (int64_t)INT32_MAX) {
    r3d_set_error("mesh components take at most 2^31 - 1 vertices and triangles (got %lld and %lld)", (long long)n_vertices,
                  (long long)n_triangles);
    return R3D_ERR_UNSUPPORTED;
  }
  return R3D_OK;
}

}  // namespace

extern "C" {

int r3d_mesh_components(r3d_ctx* ctx, const int32_t* d_tri, int64_t n_triangles, int64_t n_vertices, uint32_t* d_vertex_label_out,
                        uint32_t* d_tri_label_out, uint32_t* d_comp_out, int64_t cap_components, int64_t* n_components_out,
                        int64_t* n_invalid_out) {
  int rc = check_mesh(ctx, d_tri, n_triangles, n_vertices);
  if (rc) return rc;
  R3D_REQUIRE(n_components_out != nullptr && n_invalid_out != nullptr, "n_components_out or n_invalid_out is NULL");
  R3D_REQUIRE(cap_components >= 0, "cap_components must be >= 0");
  R3D_REQUIRE(n_vertices == 0 || d_vertex_label_out != nullptr, "d_vertex_label_out is NULL with n_vertices > 0");
  R3D_REQUIRE(cap_components == 0 || d_comp_out != nullptr, "d_comp_out is NULL with cap_components > 0");
  if ((rc = check_size(n_triangles, n_vertices))) return rc;
  const int64_t nt = n_triangles, nv = n_vertices;
  const int64_t comp_rows = cap_components < nv ? cap_components : nv;   // there are at most nv components
  const size_t tri_b = (size_t)nt * 12, vl_b = (size_t)nv * 4, tl_b = d_tri_label_out ? (size_t)nt * 4 : 0, comp_b = (size_t)comp_rows * 12;
  R3D_REQUIRE(!r3d_ranges_overlap(d_vertex_label_out, vl_b, d_tri, tri_b) && !r3d_ranges_overlap(d_tri_label_out, tl_b, d_tri, tri_b) &&
                  !r3d_ranges_overlap(d_comp_out, comp_b, d_tri, tri_b),
              "an output overlaps the triangles");
  R3D_REQUIRE(!r3d_ranges_overlap(d_vertex_label_out, vl_b, d_tri_label_out, tl_b) &&
                  !r3d_ranges_overlap(d_vertex_label_out, vl_b, d_comp_out, comp_b) &&
                  !r3d_ranges_overlap(d_tri_label_out, tl_b, d_comp_out, comp_b),
              "two outputs overlap");
  if ((rc = r3d_ctx_enter(ctx))) return rc;
  // workspace: cnt_v [nv] | cnt_t [nv] | the tile counters (64-byte aligned) | {n_components, n_invalid}
  const int tiles = tiles_of(nv);
  Counters cn(tiles, 1);
  r3d_carve ws;
  const auto cnt_v_h = ws.take<uint32_t>(nv, 64), cnt_t_h = ws.take<uint32_t>(nv, 64);
  const auto cn_h = ws.take<char>(cn.bytes, 64);
  if ((rc = r3d_scratch(ctx, kWsMeshCc, ws))) return rc;
  uint32_t *cnt_v = ws.at(cnt_v_h), *cnt_t = ws.at(cnt_t_h);
  cn.place(ws.at(cn_h));
  uint32_t *hist = cn.hist, *totals = cn.totals;
  hipStream_t st = ctx->stream;
  R3D_HIP(hipMemsetAsync(ws.block, 0, ws.bytes, st));   // every piece
  uint32_t* label = d_vertex_label_out;
  if (nv) {
    r3d_wrote(ctx, label, vl_b);
    hipLaunchKernelGGL(cc_init_kernel, dim3(blocks_of(nv)), dim3(kThreads), 0, st, label, (uint32_t)nv);
  }
  if (nt) {
    hipLaunchKernelGGL(cc_hook_kernel, dim3(blocks_of(nt)), dim3(kThreads), 0, st, d_tri, nt, (uint32_t)nv, label, totals + 1);
    if (nv) hipLaunchKernelGGL(cc_flatten_kernel, dim3(blocks_of(nv)), dim3(kThreads), 0, st, label, (uint32_t)nv);
    if (tl_b) r3d_wrote(ctx, d_tri_label_out, tl_b);
  }
  if (nt || nv)
    hipLaunchKernelGGL(cc_count_kernel, dim3(blocks_of(nt > nv ? nt : nv)), dim3(kThreads), 0, st, d_tri, nt, (uint32_t)nv,
                       (const uint32_t*)label, d_tri_label_out, cnt_v, cnt_t);
  if (nv) {
    hipLaunchKernelGGL(cc_rows_count_kernel, dim3(tiles), dim3(kThreads), 0, st, (const uint32_t*)label, (const uint32_t*)cnt_t, nv, hist);
    launch_scan(ctx, cn);
    if (comp_rows) {
      r3d_wrote(ctx, d_comp_out, comp_b);
      hipLaunchKernelGGL(cc_rows_write_kernel, dim3(tiles), dim3(kThreads), 0, st, (const uint32_t*)label, (const uint32_t*)cnt_v,
                         (const uint32_t*)cnt_t, nv, (const uint32_t*)hist, d_comp_out, (uint64_t)comp_rows);
    }
  }
  uint32_t m[2] = {0, 0};
  if ((rc = read_totals(ctx, cn, m, 2))) return rc;
  *n_components_out = (int64_t)m[0];
  *n_invalid_out = (int64_t)m[1];
  return R3D_OK;
}

int r3d_mesh_filter_components(r3d_ctx* ctx, const int32_t* d_tri, int64_t n_triangles, int64_t n_vertices, const uint32_t* d_vertex_label,
                               int64_t min_triangles, int keep_largest, uint32_t* d_kept_vertices_out, int64_t cap_vertices,
                               int32_t* d_tri_out, int64_t cap_triangles, int64_t* n_vertices_out, int64_t* n_triangles_out) {
  int rc = check_mesh(ctx, d_tri, n_triangles, n_vertices);
  if (rc) return rc;
  R3D_REQUIRE(n_vertices_out != nullptr && n_triangles_out != nullptr, "n_vertices_out or n_triangles_out is NULL");
  R3D_REQUIRE(min_triangles >= 1, "min_triangles must be >= 1 (got %lld)", (long long)min_triangles);
  R3D_REQUIRE(cap_vertices >= 0 && cap_triangles >= 0, "cap_vertices and cap_triangles must be >= 0");
  R3D_REQUIRE(n_vertices == 0 || d_vertex_label != nullptr, "d_vertex_label is NULL with n_vertices > 0");
  R3D_REQUIRE(cap_vertices == 0 || d_kept_vertices_out != nullptr, "d_kept_vertices_out is NULL with cap_vertices > 0");
  R3D_REQUIRE(cap_triangles == 0 || d_tri_out != nullptr, "d_tri_out is NULL with cap_triangles > 0");
  if ((rc = check_size(n_triangles, n_vertices))) return rc;
  const int64_t nt = n_triangles, nv = n_vertices;
  const int64_t vrows = cap_vertices < nv ? cap_vertices : nv, trows = cap_triangles < nt ? cap_triangles : nt;
  const size_t tri_b = (size_t)nt * 12, vl_b = (size_t)nv * 4, kept_b = (size_t)vrows * 4, out_b = (size_t)trows * 12;
  R3D_REQUIRE(!r3d_ranges_overlap(d_kept_vertices_out, kept_b, d_tri, tri_b) && !r3d_ranges_overlap(d_kept_vertices_out, kept_b, d_vertex_label, vl_b) &&
                  !r3d_ranges_overlap(d_tri_out, out_b, d_tri, tri_b) && !r3d_ranges_overlap(d_tri_out, out_b, d_vertex_label, vl_b),
              "an output overlaps an input");
  R3D_REQUIRE(!r3d_ranges_overlap(d_kept_vertices_out, kept_b, d_tri_out, out_b), "the two outputs overlap");
  if ((rc = r3d_ctx_enter(ctx))) return rc;
  // workspace: cnt_t [nv] | vflag [nv] | the tile counters (64-byte aligned; row 0 vertices, row 1 triangles) | totals [2] | best u64
  const int tiles_v = tiles_of(nv), tiles_t = tiles_of(nt);
  Counters cn(tiles_v > tiles_t ? tiles_v : tiles_t, 2);
  r3d_carve ws;
  const auto cnt_t_h = ws.take<uint32_t>(nv, 64), vflag_h = ws.take<uint32_t>(nv, 64);
  const auto cn_h = ws.take<char>(cn.bytes, 64);   // one piece: the counters' 64-byte tail holds the totals and, behind them, `best`
  if ((rc = r3d_scratch(ctx, kWsMeshCc, ws))) return rc;
  uint32_t *cnt_t = ws.at(cnt_t_h), *vflag = ws.at(vflag_h);
  cn.place(ws.at(cn_h));
  uint32_t* totals = cn.totals;
  unsigned long long* best = reinterpret_cast<unsigned long long*>(totals + 2);   // 8-byte aligned: stride is a multiple of 8 words
  hipStream_t st = ctx->stream;
  R3D_HIP(hipMemsetAsync(ws.block, 0, ws.bytes, st));   // every piece (the tile counters beyond either row's own tiles must read 0 in the scan)
  const Keep keep{min_triangles, keep_largest != 0 ? 1 : 0};
  if (nt && nv) {
    hipLaunchKernelGGL(cc_count_kernel, dim3(blocks_of(nt)), dim3(kThreads), 0, st, d_tri, nt, (uint32_t)nv, d_vertex_label,
                       (uint32_t*)nullptr, (uint32_t*)nullptr, cnt_t);
    hipLaunchKernelGGL(cc_best_kernel, dim3(blocks_of(nv)), dim3(kThreads), 0, st, (const uint32_t*)cnt_t, (uint32_t)nv, best);
    hipLaunchKernelGGL(cc_mark_kernel, dim3(tiles_t), dim3(kThreads), 0, st, d_tri, nt, (uint32_t)nv, d_vertex_label, (const uint32_t*)cnt_t,
                       (const unsigned long long*)best, keep, vflag, cn.row(1));
    hipLaunchKernelGGL(cc_vertex_count_kernel, dim3(tiles_v), dim3(kThreads), 0, st, (const uint32_t*)vflag, nv, cn.row(0));
    launch_scan(ctx, cn);
    if (vrows) r3d_wrote(ctx, d_kept_vertices_out, kept_b);
    // (the triangles need every kept vertex's new index even when no vertex row is wanted)
    hipLaunchKernelGGL(cc_vertex_write_kernel, dim3(tiles_v), dim3(kThreads), 0, st, vflag, nv, (const uint32_t*)cn.row(0), d_kept_vertices_out,
                       (uint64_t)vrows);
    if (trows) {
      r3d_wrote(ctx, d_tri_out, out_b);
      hipLaunchKernelGGL(cc_tri_write_kernel, dim3(tiles_t), dim3(kThreads), 0, st, d_tri, nt, (uint32_t)nv, d_vertex_label,
                         (const uint32_t*)cnt_t, (const unsigned long long*)best, keep, (const uint32_t*)vflag,
                         (const uint32_t*)cn.row(1), d_tri_out, (uint64_t)trows);
    }
  }
  uint32_t m[2] = {0, 0};
  if ((rc = read_totals(ctx, cn, m, 2))) return rc;
  *n_vertices_out = (int64_t)m[0];
  *n_triangles_out = (int64_t)m[1];
  return R3D_OK;
}

}  // extern "C"
