// Multi-view depth consistency, the host side: the entry points of include/r3d.h "Depth consistency" -- argument checks in the
// stated order, the fp64 relative poses, the context's workspaces, staging of host rasters -- and of the filtered cloud's
// compaction.  The kernels and their launches are in r3d_consistency.hip (declared in r3d_internal.h).
//   kWsSpare   the relative pose rows, [F][S] x 64 bytes shaped like TsdfPoseRow, the source index in each row's pad[0]
//   kWsIn      the rasters of the _host call;  kWsOut  its outputs, filtered | votes | keep
//   kWsCounts  the compaction's tile counters (r3d_compact_dev.h)
#include "r3d_compact_dev.h"
#include "r3d_internal.h"
#include "r3d_tsdf_dev.h"

#include <cmath>
#include <vector>

using r3d_tsdf_dev::TsdfPoseRow;
using Rule = r3d_consistency_rule;

namespace {

// the source index a relative row carries in pad[0] (-1: an empty slot); the kernel reads it back with __float_as_int
void set_source(TsdfPoseRow& row, int32_t s) { memcpy(&row.pad[0], &s, sizeof(s)); }

// What both entry points check first, in the order include/r3d.h states; R3D_OK with n_frames == 0 too (the caller returns then)
int consistency_checks(r3d_ctx* ctx, const r3d_camera* cam, int depth_dtype, int n_frames, double depth_scale, const double* h_pose,
                       const int32_t* h_sources, int n_sources, double rel_tol, int min_consistent, int max_violations) {
  R3D_REQUIRE(depth_dtype >= R3D_DEPTH_U8 && depth_dtype <= R3D_DEPTH_F32, "unknown depth dtype %d", depth_dtype);
  R3D_REQUIRE(n_frames >= 0, "n_frames must be >= 0");
  R3D_REQUIRE(n_sources >= 1 && n_sources <= R3D_CONSISTENCY_MAX_SOURCES, "n_sources must be in [1, %d], got %d",
              R3D_CONSISTENCY_MAX_SOURCES, n_sources);
  const float tol = (float)rel_tol;
  R3D_REQUIRE(std::isfinite(tol) && tol > 0.0f, "rel_tol must be finite and > 0 in f32");
  R3D_REQUIRE(min_consistent >= 0 && min_consistent <= 255, "min_consistent must be in [0, 255], got %d", min_consistent);
  R3D_REQUIRE(max_violations >= 0 && max_violations <= 255, "max_violations must be in [0, 255], got %d", max_violations);
  R3D_REQUIRE(std::isfinite((float)depth_scale), "depth_scale must be finite in f32");
  if (n_frames > 0) {
    R3D_REQUIRE(h_pose != nullptr && h_sources != nullptr, "NULL pose or source table pointer");
    const size_t slots = (size_t)n_frames * n_sources;
    for (size_t i = 0; i < slots; ++i)
      R3D_REQUIRE(h_sources[i] >= -1 && h_sources[i] < n_frames, "source %d of frame %d is %d: not -1 and not in [0, %d)",
                  (int)(i % n_sources), (int)(i / n_sources), h_sources[i], n_frames);
    for (size_t i = 0; i < slots; ++i)
      R3D_REQUIRE(h_sources[i] != (int32_t)(i / n_sources), "frame %d lists itself as source %d", h_sources[i], (int)(i % n_sources));
  }
  R3D_REQUIRE(ctx != nullptr, "ctx is NULL");
  R3D_REQUIRE(cam != nullptr, "camera is NULL");
  R3D_REQUIRE(cam->ctx == ctx, "the camera belongs to another context");
  if (n_frames == 0) return R3D_OK;
  R3D_REQUIRE(cam->width <= (1 << 24) && cam->height <= (1 << 24) && (int64_t)n_frames * cam->height * cam->width < ((int64_t)1 << 31),
              "%d rasters of %d x %d pixels: a side above 2^24 or 2^31 pixels and more in all", n_frames, cam->height, cam->width);
  return R3D_OK;
}

// slot (r, k) of the table -> its row: the relative pose of "Depth consistency" in fp64, each number rounded once, and the source
void relative_row(const double* h_pose, int r, int s, TsdfPoseRow& row) {
  for (int k = 0; k < 4; ++k) row.pad[k] = 0.0f;
  set_source(row, s);
  if (s < 0) {
    for (int k = 0; k < 9; ++k) row.r[k] = 0.0f;
    for (int k = 0; k < 3; ++k) row.t[k] = 0.0f;
    return;
  }
  const double *Rr = h_pose + (size_t)r * 12, *tr = Rr + 9, *Rs = h_pose + (size_t)s * 12, *ts = Rs + 9;
  for (int i = 0; i < 3; ++i) {
    double R[3];
    for (int j = 0; j < 3; ++j) R[j] = (Rs[3 * i] * Rr[3 * j] + Rs[3 * i + 1] * Rr[3 * j + 1]) + Rs[3 * i + 2] * Rr[3 * j + 2];
    for (int j = 0; j < 3; ++j) row.r[3 * i + j] = (float)R[j];
    row.t[i] = (float)(ts[i] - ((R[0] * tr[0] + R[1] * tr[1]) + R[2] * tr[2]));
  }
}

// The rows go up through kWsSpare and the launches follow; the arguments are checked and the ctx is entered.  Asynchronous.
int consistency_device(r3d_ctx* ctx, const r3d_camera* cam, const void* d_depth, int depth_dtype, int n_frames, double depth_scale,
                       const double* h_pose, const int32_t* h_sources, int n_sources, const Rule& rule, uint8_t* d_votes, uint8_t* d_keep,
                       float* d_filtered) {
  const size_t slots = (size_t)n_frames * n_sources;
  std::vector<TsdfPoseRow> h_rows(slots);
  for (size_t i = 0; i < slots; ++i) relative_row(h_pose, (int)(i / n_sources), h_sources[i], h_rows[i]);
  void* d_rows = nullptr;
  int rc = r3d_scratch(ctx, kWsSpare, slots * sizeof(TsdfPoseRow), &d_rows);
  if (rc) return rc;
  // from pageable memory: the copy has read h_rows when the call returns
  R3D_HIP(hipMemcpyAsync(d_rows, h_rows.data(), slots * sizeof(TsdfPoseRow), hipMemcpyHostToDevice, ctx->stream));
  const size_t n = (size_t)n_frames * cam->height * cam->width;
  if (d_votes) r3d_wrote(ctx, d_votes, n * 2);
  if (d_keep) r3d_wrote(ctx, d_keep, n);
  if (d_filtered) r3d_wrote(ctx, d_filtered, n * 4);
  r3d_consistency_launch(ctx, cam, depth_scale, d_depth, depth_dtype, d_rows, n_frames, n_sources, rule, d_votes, d_keep, d_filtered);
  R3D_HIP(hipGetLastError());
  return R3D_OK;
}

}  // namespace

extern "C" {

int r3d_depth_consistency(r3d_ctx* ctx, const r3d_camera* cam, const void* d_depth, int depth_dtype, int n_frames, double depth_scale,
                          const double* h_pose_w2c, const int32_t* h_sources, int n_sources, double rel_tol, int min_consistent,
                          int max_violations, uint8_t* d_votes_out, uint8_t* d_keep_out, float* d_filtered_out) {
  int rc = consistency_checks(ctx, cam, depth_dtype, n_frames, depth_scale, h_pose_w2c, h_sources, n_sources, rel_tol, min_consistent,
                              max_violations);
  if (rc || n_frames == 0) return rc;
  R3D_REQUIRE(d_depth != nullptr, "NULL depth pointer");
  R3D_REQUIRE(d_votes_out || d_keep_out || d_filtered_out, "no output given: votes, keep and filtered are all NULL");
  R3D_REQUIRE(((uintptr_t)d_votes_out & 1) == 0, "d_votes_out must be 2-byte aligned");
  const size_t n = (size_t)n_frames * cam->height * cam->width;
  const r3d_range outs[3] = {{d_votes_out, n * 2}, {d_keep_out, n}, {d_filtered_out, n * 4}};
  const r3d_range in = {d_depth, n * r3d_depth_size(depth_dtype)};
  R3D_REQUIRE(!r3d_any_overlap(outs, 3, &in, 1), "an output overlaps the rasters or another output");
  if ((rc = r3d_ctx_enter(ctx))) return rc;
  return consistency_device(ctx, cam, d_depth, depth_dtype, n_frames, depth_scale, h_pose_w2c, h_sources, n_sources,
                            Rule{(float)rel_tol, min_consistent, max_violations}, d_votes_out, d_keep_out, d_filtered_out);
}

int r3d_depth_consistency_host(r3d_ctx* ctx, const r3d_camera* cam, const void* h_depth, int depth_dtype, int n_frames,
                               double depth_scale, const double* h_pose_w2c, const int32_t* h_sources, int n_sources, double rel_tol,
                               int min_consistent, int max_violations, uint8_t* h_votes_out, uint8_t* h_keep_out,
                               float* h_filtered_out) {
  int rc = consistency_checks(ctx, cam, depth_dtype, n_frames, depth_scale, h_pose_w2c, h_sources, n_sources, rel_tol, min_consistent,
                              max_violations);
  if (rc || n_frames == 0) return rc;
  R3D_REQUIRE(h_depth != nullptr, "NULL depth pointer");
  R3D_REQUIRE(h_votes_out || h_keep_out || h_filtered_out, "no output given: votes, keep and filtered are all NULL");
  const size_t n = (size_t)n_frames * cam->height * cam->width, in_bytes = n * r3d_depth_size(depth_dtype);
  const r3d_range outs[3] = {{h_votes_out, n * 2}, {h_keep_out, n}, {h_filtered_out, n * 4}};
  const r3d_range in = {h_depth, in_bytes};
  R3D_REQUIRE(!r3d_any_overlap(outs, 3, &in, 1), "an output overlaps the rasters or another output");
  if ((rc = r3d_ctx_enter(ctx))) return rc;
  // the rasters through kWsIn; the requested outputs through kWsOut: filtered | votes | keep, so each is aligned for its type
  const size_t filtered_bytes = h_filtered_out ? n * 4 : 0, votes_bytes = h_votes_out ? n * 2 : 0, keep_bytes = h_keep_out ? n : 0;
  void* d_in = nullptr;
  r3d_carve out;
  const auto filtered_h = out.take<float>(filtered_bytes / 4);
  const auto votes_h = out.take<uint8_t>(votes_bytes), keep_h = out.take<uint8_t>(keep_bytes);
  if ((rc = r3d_scratch(ctx, kWsIn, in_bytes, &d_in)) || (rc = r3d_scratch(ctx, kWsOut, out))) return rc;
  float* d_filtered = h_filtered_out ? out.at(filtered_h) : nullptr;
  uint8_t* d_votes = h_votes_out ? out.at(votes_h) : nullptr;
  uint8_t* d_keep = h_keep_out ? out.at(keep_h) : nullptr;
  if ((rc = r3d_memcpy_h2d(ctx, d_in, h_depth, in_bytes))) return rc;
  if ((rc = consistency_device(ctx, cam, d_in, depth_dtype, n_frames, depth_scale, h_pose_w2c, h_sources, n_sources,
                               Rule{(float)rel_tol, min_consistent, max_violations}, d_votes, d_keep, d_filtered)))
    return rc;
  if (h_filtered_out && (rc = r3d_download_pageable(ctx, h_filtered_out, d_filtered, filtered_bytes))) return rc;
  if (h_votes_out && (rc = r3d_download_pageable(ctx, h_votes_out, d_votes, votes_bytes))) return rc;
  if (h_keep_out && (rc = r3d_download_pageable(ctx, h_keep_out, d_keep, keep_bytes))) return rc;
  R3D_HIP(hipStreamSynchronize(ctx->stream));
  return R3D_OK;
}

int r3d_compact_rows_by_mask(r3d_ctx* ctx, const float* d_xyz, const uint32_t* d_rgba, int64_t n, const uint8_t* d_keep,
                             float* d_xyz_out, uint32_t* d_rgba_out, int64_t cap, int64_t* n_out) {
  R3D_REQUIRE(n_out != nullptr, "n_out is NULL");
  R3D_REQUIRE(n >= 0 && n < ((int64_t)1 << 32), "bad cloud size %lld", (long long)n);
  R3D_REQUIRE(cap >= 0, "cap must be >= 0");
  int rc = r3d_ctx_enter(ctx);
  if (rc) return rc;
  if (n == 0) {
    *n_out = 0;
    return R3D_OK;
  }
  R3D_REQUIRE(d_xyz && d_keep, "NULL device pointer");
  R3D_REQUIRE(cap == 0 || d_xyz_out != nullptr, "d_xyz_out is NULL with cap > 0");
  R3D_REQUIRE((cap == 0 || !d_rgba || d_rgba_out) && (!d_rgba_out || d_rgba), "d_rgba and d_rgba_out go together");
  const int tiles = r3d_compact::tiles_of(n);
  r3d_compact::Counters cn(tiles, 1);
  void* ws = nullptr;
  if ((rc = r3d_scratch(ctx, kWsCounts, cn.bytes, &ws))) return rc;
  cn.place(ws);
  r3d_mask_count_launch(ctx, d_keep, n, tiles, cn.hist);
  uint32_t m = 0;
  if ((rc = r3d_compact::scan_totals(ctx, cn, &m))) return rc;
  const uint64_t rows = (uint64_t)((int64_t)m < cap ? (int64_t)m : cap);
  // the outputs need room for the written rows only
  const r3d_range outs[2] = {{d_xyz_out, (size_t)rows * 12}, {d_rgba_out, (size_t)rows * 4}};
  const r3d_range ins[3] = {{d_xyz, (size_t)n * 12}, {d_rgba, (size_t)n * 4}, {d_keep, (size_t)n}};
  R3D_REQUIRE(!r3d_any_overlap(outs, 2, ins, 3), "an output range overlaps an input or the other output");
  *n_out = (int64_t)m;
  if (rows == 0) return R3D_OK;
  r3d_wrote(ctx, d_xyz_out, (size_t)rows * 12);
  if (d_rgba_out) r3d_wrote(ctx, d_rgba_out, (size_t)rows * 4);
  r3d_mask_write_launch(ctx, d_xyz, d_rgba, n, d_keep, tiles, cn.hist, d_xyz_out, d_rgba_out, rows);
  R3D_HIP(hipGetLastError());
  return R3D_OK;
}

}  // extern "C"
