// r3d_tsdf_integrate_cloud and r3d_tsdf_integrate_cloud_host: the drivers of the kernels in r3d_tsdf_cloud.hip.
// Semantics: include/r3d.h ("TSDF from an oriented cloud").
//
//   mark -> count -> scan -> (one 4-byte read-back: the number of marked blocks) -> list -> per chunk: centres, r3d_nn_index_query, apply
//
// The query takes the context's shared workspaces (kWsIn, kWsOut, kWsSpare, kWsCounts, kWsMisc), so what has to live across it -- the
// block list with the touched-voxel counter in front, one chunk's queries and matches, the host entry's upload -- sits in buffers the
// VOLUME owns (r3d_tsdf::cloud_buf, grow-only, freed by r3d_tsdf_destroy).  The block bitmap (kWsSpare) and the compaction's
// counters (kWsCounts) are read for the last time by the list launch, in stream order in front of the first query.  The band is
// processed in chunks of a fixed number of blocks (tuning key "tsdf_cloud_chunk"), which bounds the chunk buffer; every voxel is
// decided by its own lane from its own match, so the result does not depend on the chunking.
#include "r3d_compact_dev.h"
#include "r3d_internal.h"
#include "r3d_nnindex_dev.h"
#include "r3d_tsdf_dev.h"

using namespace r3d_tsdf_dev;

namespace {

constexpr int kChunkBlocks = 16384;           // blocks per chunk unless "tsdf_cloud_chunk" says otherwise: 2^20 queries, 20 MiB
enum { kBufList = 0, kBufChunk, kBufHost };   // r3d_tsdf::cloud_buf
static_assert(kBufHost + 1 == r3d_tsdf::kCloudBufs, "one r3d_tsdf::cloud_buf entry per buffer");

// *p = at least `bytes` bytes of the volume's own buffer `which` (grow-only; the contents are not kept across growing)
int cloud_buffer(r3d_tsdf* v, int which, size_t bytes, void** p) {
  if (v->cloud_bytes[which] < bytes) {
    R3D_HIP(hipStreamSynchronize(v->ctx->stream));   // work in flight may still read the old block
    if (v->cloud_buf[which]) (void)hipFree(v->cloud_buf[which]);
    v->cloud_buf[which] = nullptr;
    v->cloud_bytes[which] = 0;
    const hipError_t e = hipMalloc(&v->cloud_buf[which], bytes);
    if (e == hipErrorOutOfMemory) {
      r3d_set_error("the cloud integration's workspace of %zu bytes does not fit the device", bytes);
      return R3D_ERR_NOMEM;
    }
    R3D_HIP(e);
    v->cloud_bytes[which] = bytes;
  }
  *p = v->cloud_buf[which];
  return R3D_OK;
}
int cloud_buffer(r3d_tsdf* v, int which, r3d_carve& c) {   // ... holding c.bytes, c placed there
  void* p = nullptr;
  const int rc = cloud_buffer(v, which, c.bytes, &p);
  c.place(p);
  return rc;
}

// what both entry points check about the colours of a volume that is there: rgba goes with the colour plane and only with it (a
// colour volume without rgba would let n part from w, as r3d_tsdf_integrate on such a volume would)
int cloud_checks(r3d_tsdf* v, const void* rgba) {
  int rc = R3D_OK;
  if (rgba && (rc = r3d_tsdf_require_color(v))) return rc;
  R3D_REQUIRE(rgba || v->d_col == nullptr, "the volume carries colour: a cloud goes into it with its colours (rgba)");
  return R3D_OK;
}

}  // namespace

int r3d_tsdf_integrate_cloud(r3d_tsdf* v, r3d_nn_index* ix, const float* d_normals, const uint32_t* d_rgba, int64_t* n_touched_out) {
  R3D_REQUIRE(v != nullptr, "TSDF volume is NULL");
  R3D_REQUIRE(ix != nullptr, "nn index is NULL");
  R3D_REQUIRE(d_normals != nullptr, "d_normals is NULL");
  R3D_REQUIRE(ix->ctx == v->ctx, "the index belongs to another context than the volume");
  int rc = cloud_checks(v, d_rgba);
  if (rc) return rc;
  if (n_touched_out) *n_touched_out = 0;
  if (ix->n == 0) return R3D_OK;
  r3d_ctx* ctx = v->ctx;
  if ((rc = r3d_ctx_enter(ctx))) return rc;
  hipStream_t st = ctx->stream;
  const TsdfGrid& g = v->g;
  const int64_t n_words = (r3d_tsdf_cloud_blocks(g) + 31) / 32;

  // mark -> count -> scan: the bitmap in kWsSpare, the tiles' counters in kWsCounts
  void *bm = nullptr, *ws = nullptr;
  if ((rc = r3d_scratch(ctx, kWsSpare, (size_t)n_words * 4, &bm))) return rc;
  uint32_t* bitmap = static_cast<uint32_t*>(bm);
  const int tiles = r3d_compact::tiles_of(n_words);
  r3d_compact::Counters cn(tiles, 1);
  if ((rc = r3d_scratch(ctx, kWsCounts, cn.bytes, &ws))) return rc;
  cn.place(ws);
  R3D_HIP(hipMemsetAsync(bitmap, 0, (size_t)n_words * 4, st));
  r3d_tsdf_cloud_mark_launch(ctx, ix->d_tgt, ix->n, g, bitmap);
  r3d_tsdf_cloud_count_launch(ctx, bitmap, n_words, tiles, cn.hist);
  uint32_t n_marked = 0;
  if ((rc = r3d_compact::scan_totals(ctx, cn, &n_marked))) return rc;
  if (n_marked == 0) return R3D_OK;

  // the list of marked blocks, behind the counter of touched voxels
  r3d_carve lb;
  const auto touched_h = lb.take<unsigned long long>(1);
  const auto list_h = lb.take<uint32_t>(n_marked);
  if ((rc = cloud_buffer(v, kBufList, lb))) return rc;
  unsigned long long* touched = lb.at(touched_h);
  uint32_t* list = lb.at(list_h);
  R3D_HIP(hipMemsetAsync(touched, 0, sizeof(*touched), st));
  r3d_tsdf_cloud_list_launch(ctx, bitmap, n_words, tiles, cn.hist, list);
  R3D_HIP(hipGetLastError());

  // the band, a chunk of blocks at a time: centres -> nearest points -> the rule
  uint32_t chunk = ctx->tsdf_cloud_chunk > 0 ? (uint32_t)ctx->tsdf_cloud_chunk : (uint32_t)kChunkBlocks;
  if (chunk > (1u << 24)) chunk = 1u << 24;   // the lanes of a chunk fit 32 bits
  if (chunk > n_marked) chunk = n_marked;
  const size_t lanes_max = (size_t)chunk * 64;
  r3d_carve cb;
  const auto q_h = cb.take<float>(lanes_max * 3);
  const auto idx_h = cb.take<uint32_t>(lanes_max);
  const auto d2_h = cb.take<float>(lanes_max);
  if ((rc = cloud_buffer(v, kBufChunk, cb))) return rc;
  float *q = cb.at(q_h), *d2 = cb.at(d2_h);
  uint32_t* idx = cb.at(idx_h);
  for (uint32_t lo = 0; lo < n_marked; lo += chunk) {
    const uint32_t nb = n_marked - lo < chunk ? n_marked - lo : chunk;
    r3d_tsdf_cloud_centres_launch(ctx, list + lo, nb, g, q);
    R3D_HIP(hipGetLastError());
    if ((rc = r3d_nn_index_query(ix, q, (int64_t)nb * 64, idx, d2, 0, nullptr))) return rc;
    r3d_tsdf_cloud_apply_launch(ctx, list + lo, nb, g, idx, d2, ix->d_tgt, d_normals, d_rgba, (uint32_t)ix->n, v->d_vol, v->d_col, touched);
    R3D_HIP(hipGetLastError());
  }
  if (n_touched_out) {
    unsigned long long h = 0;
    R3D_HIP(hipMemcpyAsync(&h, touched, sizeof(h), hipMemcpyDeviceToHost, st));
    R3D_HIP(hipStreamSynchronize(st));
    *n_touched_out = (int64_t)h;
  }
  return R3D_OK;
}

int r3d_tsdf_integrate_cloud_host(r3d_tsdf* v, const float* h_xyz, const float* h_normals, const uint32_t* h_rgba, int64_t n,
                                  int64_t* n_touched_out) {
  R3D_REQUIRE(v != nullptr, "TSDF volume is NULL");
  R3D_REQUIRE(n >= 0, "negative cloud size");
  R3D_REQUIRE(n == 0 || (h_xyz != nullptr && h_normals != nullptr), "NULL cloud or normals pointer");
  R3D_REQUIRE(n < ((int64_t)1 << 32), "cloud too large for uint32 indices");
  int rc = cloud_checks(v, h_rgba);
  if (rc) return rc;
  if (n_touched_out) *n_touched_out = 0;
  if (n == 0) return R3D_OK;
  r3d_ctx* ctx = v->ctx;
  if ((rc = r3d_ctx_enter(ctx))) return rc;
  r3d_carve in;
  const auto xyz_h = in.take<float>((size_t)n * 3), normals_h = in.take<float>((size_t)n * 3);
  const auto rgba_h = in.take<uint32_t>(h_rgba ? (size_t)n : 0);
  if ((rc = cloud_buffer(v, kBufHost, in))) return rc;
  float *d_xyz = in.at(xyz_h), *d_normals = in.at(normals_h);
  uint32_t* d_rgba = h_rgba ? in.at(rgba_h) : nullptr;
  if ((rc = r3d_memcpy_h2d(ctx, d_xyz, h_xyz, (size_t)n * 12)) || (rc = r3d_memcpy_h2d(ctx, d_normals, h_normals, (size_t)n * 12))) return rc;
  if (h_rgba && (rc = r3d_memcpy_h2d(ctx, d_rgba, h_rgba, (size_t)n * 4))) return rc;
  r3d_nn_index* ix = nullptr;
  if ((rc = r3d_nn_index_create(ctx, d_xyz, n, &ix))) return rc;
  rc = r3d_tsdf_integrate_cloud(v, ix, d_normals, d_rgba, n_touched_out);
  const hipError_t e = hipStreamSynchronize(ctx->stream);   // the caller's memory is free at return, and so is the index
  r3d_nn_index_destroy(ix);
  if (rc) return rc;
  R3D_HIP(e);
  return R3D_OK;
}
