// Mesh smoothing, the host side: the entry points of include/r3d.h "Mesh smoothing" -- argument checks, the workspace, the sorts
// and the sequencing.  The kernels and their launches are in r3d_mesh_smooth.hip (declared in r3d_internal.h).
//   kWsMeshSmooth  r3d_mesh_adjacency: side keys [6M] u64 | the sort's spare [6M] u64 (the distinct keys go where the sorted ones
//                  are not) | the compaction's tile counters;  r3d_mesh_smooth: the two ping-pong position arrays;
//                  r3d_mesh_vertex_normals: corner keys [3M] u64 | the sort's spare [3M] u64
//   kWsCounts      the sorts' histogram (r3d_radix_sort_u64 takes it; nothing of this file's lives there)
#include "r3d_compact_dev.h"
#include "r3d_internal.h"

#include <cmath>

namespace {

constexpr int kMaxFactors = 4096;

// the bits of a vertex index: the smallest vb >= 1 with n_vertices <= 2^vb
int vertex_bits(int64_t n_vertices) {
  int vb = 1;
  while (((int64_t)1 << vb) < n_vertices) ++vb;
  return vb;
}

int check_mesh(const r3d_ctx* ctx, const int32_t* d_tri, int64_t n_triangles, int64_t n_vertices) {
  R3D_REQUIRE(ctx != nullptr, "ctx is NULL");
  R3D_REQUIRE(n_triangles >= 0 && n_vertices >= 0, "negative mesh size (%lld triangles, %lld vertices)", (long long)n_triangles,
              (long long)n_vertices);
  R3D_REQUIRE(n_triangles == 0 || d_tri != nullptr, "d_tri is NULL with n_triangles > 0");
  return R3D_OK;
}

// the keys of a call (6 or 3 per triangle) are counted in 32 bits
int check_size(int64_t n_triangles, int64_t n_vertices) {
  if (n_vertices > (int64_t)INT32_MAX || n_triangles >= (((int64_t)1 << 32) + 5) / 6) {
    r3d_set_error("mesh smoothing takes at most 2^31 - 1 vertices and fewer than 2^32 / 6 triangles (got %lld and %lld)",
                  (long long)n_vertices, (long long)n_triangles);
    return R3D_ERR_UNSUPPORTED;
  }
  return R3D_OK;
}

}  // namespace

extern "C" {

int r3d_mesh_adjacency(r3d_ctx* ctx, const int32_t* d_tri, int64_t n_triangles, int64_t n_vertices, uint32_t* d_row_start_out,
                       uint32_t* d_neighbours_out, int64_t cap_neighbours, uint8_t* d_boundary_out, int64_t* n_neighbours_out) {
  int rc = check_mesh(ctx, d_tri, n_triangles, n_vertices);
  if (rc) return rc;
  R3D_REQUIRE(n_neighbours_out != nullptr, "n_neighbours_out is NULL");
  R3D_REQUIRE(cap_neighbours >= 0, "cap_neighbours must be >= 0 (got %lld)", (long long)cap_neighbours);
  R3D_REQUIRE(d_row_start_out != nullptr, "d_row_start_out is NULL");
  R3D_REQUIRE(cap_neighbours == 0 || d_neighbours_out != nullptr, "d_neighbours_out is NULL with cap_neighbours > 0");
  if ((rc = check_size(n_triangles, n_vertices))) return rc;
  const int64_t nt = n_triangles, nv = n_vertices, n_keys = 6 * nt;
  const int64_t nb_rows = cap_neighbours < n_keys ? cap_neighbours : n_keys;   // there are at most 6M neighbour entries
  const size_t rs_b = (size_t)(nv + 1) * 4, nb_b = (size_t)nb_rows * 4, bd_b = d_boundary_out ? (size_t)nv : 0;
  const r3d_range outs[3] = {{d_row_start_out, rs_b}, {d_neighbours_out, nb_b}, {d_boundary_out, bd_b}};
  const r3d_range in = {d_tri, (size_t)nt * 12};
  R3D_REQUIRE(!r3d_any_overlap(outs, 3, &in, 1), "an output overlaps the triangles or another output");
  if ((rc = r3d_ctx_enter(ctx))) return rc;
  hipStream_t st = ctx->stream;
  r3d_wrote(ctx, d_row_start_out, rs_b);
  if (bd_b) {
    r3d_wrote(ctx, d_boundary_out, bd_b);
    R3D_HIP(hipMemsetAsync(d_boundary_out, 0, bd_b, st));
  }
  *n_neighbours_out = 0;
  if (nt == 0 || nv == 0) {   // no valid triangle: every row is empty
    R3D_HIP(hipMemsetAsync(d_row_start_out, 0, rs_b, st));
    R3D_HIP(hipStreamSynchronize(st));
    return R3D_OK;
  }
  const int vb = vertex_bits(nv), tiles = r3d_compact::tiles_of(n_keys);
  r3d_compact::Counters cn(tiles, 1);
  r3d_carve ws;
  const auto keys_h = ws.take<uint64_t>(n_keys, 64), tmp_h = ws.take<uint64_t>(n_keys, 64);
  const auto cn_h = ws.take<char>(cn.bytes, 64);
  if ((rc = r3d_scratch(ctx, kWsMeshSmooth, ws))) return rc;
  uint64_t *keys = ws.at(keys_h), *tmp = ws.at(tmp_h), *sorted = nullptr;
  cn.place(ws.at(cn_h));
  r3d_mesh_side_keys_launch(ctx, d_tri, nt, (uint32_t)nv, vb, keys);
  R3D_HIP(hipGetLastError());
  if ((rc = r3d_radix_sort_u64(ctx, keys, tmp, n_keys, 2 * vb + 1, 0, &sorted))) return rc;
  uint64_t* distinct = sorted == keys ? tmp : keys;
  r3d_mesh_heads_count_launch(ctx, sorted, n_keys, vb, tiles, cn.hist);
  uint32_t e = 0;
  if ((rc = r3d_compact::scan_totals(ctx, cn, &e))) return rc;   // (synchronises: the rows kernel is sized by E)
  r3d_mesh_heads_write_launch(ctx, sorted, n_keys, vb, tiles, cn.hist, distinct, d_boundary_out);
  const uint32_t rows = (uint32_t)((int64_t)e < cap_neighbours ? (int64_t)e : cap_neighbours);
  if (rows) r3d_wrote(ctx, d_neighbours_out, (size_t)rows * 4);
  r3d_mesh_rows_launch(ctx, distinct, e, (uint32_t)nv, vb, d_row_start_out, d_neighbours_out, rows);
  R3D_HIP(hipGetLastError());
  R3D_HIP(hipStreamSynchronize(st));
  *n_neighbours_out = (int64_t)e;
  return R3D_OK;
}

int r3d_mesh_smooth(r3d_ctx* ctx, const float* d_xyz_in, float* d_xyz_out, int64_t n_vertices, const uint32_t* d_row_start,
                    const uint32_t* d_neighbours, const uint8_t* d_locked, const double* factors, int n_factors) {
  R3D_REQUIRE(ctx != nullptr, "ctx is NULL");
  R3D_REQUIRE(n_vertices >= 0, "n_vertices must be >= 0 (got %lld)", (long long)n_vertices);
  R3D_REQUIRE(n_factors >= 0 && n_factors <= kMaxFactors, "n_factors must be in [0, %d], got %d", kMaxFactors, n_factors);
  R3D_REQUIRE(n_factors == 0 || factors != nullptr, "factors is NULL with n_factors > 0");
  for (int k = 0; k < n_factors; ++k) R3D_REQUIRE(std::isfinite(factors[k]), "factor %d is not finite (%g)", k, factors[k]);
  R3D_REQUIRE(n_vertices == 0 || (d_xyz_in != nullptr && d_xyz_out != nullptr), "d_xyz_in or d_xyz_out is NULL with n_vertices > 0");
  R3D_REQUIRE(n_vertices == 0 || n_factors == 0 || d_row_start != nullptr, "d_row_start is NULL");
  if (n_vertices > (int64_t)INT32_MAX) {
    r3d_set_error("mesh smoothing takes at most 2^31 - 1 vertices (got %lld)", (long long)n_vertices);
    return R3D_ERR_UNSUPPORTED;
  }
  const int64_t nv = n_vertices;
  const size_t xyz_b = (size_t)nv * 12;
  const r3d_range out = {d_xyz_out, xyz_b};
  // (the neighbour list's length is device data: its first word stands for it)
  const r3d_range ins[4] = {{d_xyz_in, xyz_b}, {d_row_start, (size_t)(nv + 1) * 4}, {d_neighbours, 4}, {d_locked, (size_t)nv}};
  R3D_REQUIRE(!r3d_any_overlap(&out, 1, ins, 4), "d_xyz_out overlaps an input");
  int rc = r3d_ctx_enter(ctx);
  if (rc) return rc;
  if (nv == 0) return R3D_OK;
  r3d_wrote(ctx, d_xyz_out, xyz_b);
  if (n_factors == 0) {
    R3D_HIP(hipMemcpyAsync(d_xyz_out, d_xyz_in, xyz_b, hipMemcpyDeviceToDevice, ctx->stream));
    return R3D_OK;
  }
  // step k reads what step k - 1 wrote: in -> ws[0] -> ws[1] -> ws[0] ... -> out
  float* pp[2] = {nullptr, nullptr};
  if (n_factors > 1) {
    r3d_carve ws;
    const auto p0 = ws.take<float>((size_t)nv * 3, 64), p1 = ws.take<float>(n_factors > 2 ? (size_t)nv * 3 : 0, 64);   // two steps need one
    if ((rc = r3d_scratch(ctx, kWsMeshSmooth, ws))) return rc;
    pp[0] = ws.at(p0), pp[1] = ws.at(p1);
  }
  const float* src = d_xyz_in;
  for (int k = 0; k < n_factors; ++k) {
    float* dst = k == n_factors - 1 ? d_xyz_out : pp[k & 1];
    r3d_mesh_step_launch(ctx, src, dst, (uint32_t)nv, d_row_start, d_neighbours, d_locked, factors[k]);
    src = dst;
  }
  R3D_HIP(hipGetLastError());
  return R3D_OK;
}

int r3d_mesh_vertex_normals(r3d_ctx* ctx, const float* d_xyz, int64_t n_vertices, const int32_t* d_tri, int64_t n_triangles,
                            const float* d_fallback, float* d_normals_out) {
  int rc = check_mesh(ctx, d_tri, n_triangles, n_vertices);
  if (rc) return rc;
  R3D_REQUIRE(n_vertices == 0 || (d_xyz != nullptr && d_normals_out != nullptr), "d_xyz or d_normals_out is NULL with n_vertices > 0");
  if ((rc = check_size(n_triangles, n_vertices))) return rc;
  const int64_t nt = n_triangles, nv = n_vertices, n_keys = 3 * nt;
  const size_t xyz_b = (size_t)nv * 12;
  const r3d_range out = {d_normals_out, xyz_b};
  const r3d_range ins[3] = {{d_xyz, xyz_b}, {d_tri, (size_t)nt * 12}, {d_fallback, xyz_b}};
  R3D_REQUIRE(!r3d_any_overlap(&out, 1, ins, 3), "d_normals_out overlaps an input");
  if ((rc = r3d_ctx_enter(ctx))) return rc;
  if (nv == 0) return R3D_OK;
  r3d_wrote(ctx, d_normals_out, xyz_b);
  uint64_t* sorted = nullptr;
  if (nt > 0) {
    const int vb = vertex_bits(nv);
    r3d_carve ws;
    const auto keys_h = ws.take<uint64_t>(n_keys, 64), tmp_h = ws.take<uint64_t>(n_keys, 64);
    if ((rc = r3d_scratch(ctx, kWsMeshSmooth, ws))) return rc;
    uint64_t *keys = ws.at(keys_h), *tmp = ws.at(tmp_h);
    r3d_mesh_corner_keys_launch(ctx, d_tri, nt, (uint32_t)nv, vb, keys);
    R3D_HIP(hipGetLastError());
    // (the low 32 bits hold 3t + c, which already ascends: the stable sort skips those digits)
    if ((rc = r3d_radix_sort_u64(ctx, keys, tmp, n_keys, 32 + vb + 1, 32, &sorted))) return rc;
  }
  r3d_mesh_normals_launch(ctx, d_xyz, (uint32_t)nv, d_tri, sorted, (uint32_t)n_keys, d_fallback, d_normals_out);
  R3D_HIP(hipGetLastError());
  return R3D_OK;
}

}  // extern "C"
