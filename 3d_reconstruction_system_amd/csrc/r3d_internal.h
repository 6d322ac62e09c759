// Internal declarations shared by the translation units of libr3d_hip.so.
// Public surface: include/r3d.h.  gfx950 (MI355X) only.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdarg>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <functional>

#include "r3d.h"
#include "r3d_carve.h"
#include "r3d_internal_api.h"

// The context's grow-only device workspaces (r3d_ctx::scratch), claimed by name through r3d_scratch.  A SHARED entry is taken by
// many entry points one after the other in stream order; nobody may expect to find in it what an earlier call left (tests/
// test_gpu_call_order.py), and a helper takes one only if no caller above it holds data there.  A PRIVATE entry is one file's.
// A claim that holds more than one array is an r3d_carve (r3d_carve.h): the claimant take()s its pieces in the order given below
// ("a | b": b behind a), r3d_scratch(ctx, which, carve) asks for their sum, and carve.at(piece) is the only pointer arithmetic.
//   kWsIn          shared   staged input of the *_host calls (fuse, apply, ICP source, voxel and grid points, consistency rasters);
//                           TSDF slabs (depth | rgb); NN sort keys; FPFH k-NN lists (idx | d2); r3d_register_ransac's gathered pairs; octree
//                           records; the voxel union's list
//   kWsOut         shared   staged output of the *_host calls (ICP: the target; consistency: filtered | votes | keep); the sorted voxel codes; NN query `src4` / sorted
//                           copy; SOR scores; FPFH rows; merge remainders
//   kWsSpare       shared   the radix sort's `tmp` where the caller has none (NN, voxel codes, r3d_sort_u64); fuse pose tables;
//                           r3d_depth_consistency's relative pose rows ([F][S] x 64 bytes, the source index in each row's padding);
//                           octree meta | pre; merge segments (rem | hi); host ICP idx; feature match's b -> a partial minima (dist | idx); the block bitmap of
//                           r3d_tsdf_integrate_cloud (dead before its first NN query)
//   kWsCounts      shared   hist | totals of EVERY radix sort (r3d_radix_sort_workspace; the private files sort too); compaction
//                           Counters of knn, tsdf, tsdf_mesh (masks | group_first | Counters), tsdf_cloud, r3d_compact_rows_by_mask; the octree's
//                           flags | tile_base | tile_cnt | tile_leaf; host ICP d2 and sums; fuse rgb; feature match's b -> a rows; the voxel union's counts
//   kWsPartials    shared   partial rows of the sums passes (ICP, NN query + solve, tracking, SOR); NN bound rows; consensus
//                           partial | part; r3d_apply_T_many's table; grad_P partials; fuse rgba; grid colours; a -> b partial minima (dist | idx);
//                           SOR rows1 | rows2
//   kWsMisc        shared   what the host reads back: NN `misc`, SOR stats | kept (one copy), consensus misc | hyp | rows | valid | counts, feature
//                           match's keep counts, the voxel set's 64 bytes; viewpoint table; textfmt flags | off | len (flags | off: one copy);
//                           sort-merge partials | starts | hist | totals | spill count | flags | cursors | spill (count .. cursors: one memset);
//                           brute-force ICP idx | d2
//   kWsSelect      shared   r3d_plane.hip alone: hist | state | out | rows (hist | state: one memset).  r3d_ctx::select_ws records that the
//                           histogram, the block's first piece, is all zero; r3d_scratch forgets that when it reallocates the entry
//   kWsTrack       shared   r3d_track.hip: every level's four maps | the upper levels' depth | ICP state, or (colour) four maps | model packed |
//                           model depth | source intensity | model rgb | state; r3d_plane.hip's rank-trimming r2 | class (never inside one call)
//   kWsBilateral   private  r3d_bilateral.hip: the weight tables, keyed by r3d_ctx::bilateral_*; the contents outlive the call
//   kWsRegSums     private  r3d_reginfo.hip: partial rows + 11 sums, always asked for at the largest size (never regrows)
//   kWsColorRows   private  r3d_color_icp.hip: partial rows + 31 sums, always asked for at the largest size (never regrows)
//   kWsColorLists  private  r3d_color_icp.hip: the k-NN lists (idx | d2) of r3d_color_gradient_knn
//   kWsMeshCc      private  r3d_mesh_cc.hip: two per-vertex arrays | Counters (its 64-byte tail: totals, then `best`); cleared whole by one memset
//   kWsMeshDist    private  r3d_meshdist.hip: keys | tmp of an index build or query; r3d_distance_stats' sums | min-max | out | counts
//   kWsMeshSmooth  private  r3d_mesh_smooth_host.cpp: adjacency keys | tmp | Counters; the smoothing steps' two ping-pong position
//                           arrays; the normals' keys | tmp (one call at a time, nothing outlives it)
// Hand-over rules between nested claims:
//   * a sort holds kWsCounts (r3d_sort_u64 also kWsSpare) until its last pass is enqueued: its callers keep nothing of theirs
//     there across it (the voxel code list lives in kWsOut, the NN keys in kWsIn);
//   * r3d_voxelset_sorted_codes_device returns with the codes in kWsOut and kWsSpare / kWsCounts released: r3d_octree.hip takes
//     those two for meta and tile places and kWsIn for the records, in stream order behind the sort;
//   * r3d_consensus::layout takes kWsMisc and kWsPartials whole: r3d_register_ransac keeps its pairs in kWsIn, and feature
//     matching (keep counts in kWsMisc, partial minima where r3d_match_nearest is told: kWsPartials, kWsSpare) runs no consensus;
//   * growing frees the old block once both streams are idle: no pointer into an entry survives a larger r3d_scratch of it, so
//     a loop reserves its largest size up front (r3d_track.hip's rows) and a carve is claimed once, before its first at();
//   * pieces that one copy or one memset spans are taken next to each other and the length is the distance between two pieces'
//     offsets (or the comment at the take() says why they touch); a Counters block is one piece (cn.bytes), its tail included.
enum r3d_workspace : int {
  kWsIn = 0,
  kWsOut,
  kWsSpare,
  kWsCounts,
  kWsPartials,
  kWsMisc,
  kWsSelect,
  kWsTrack,
  kWsBilateral,
  kWsRegSums,
  kWsColorRows,
  kWsColorLists,
  kWsMeshCc,
  kWsMeshDist,
  kWsMeshSmooth,
  kWsEnd
};

struct r3d_ctx {
  int device = -1;
  hipStream_t stream = nullptr;
  bool owns_stream = false;
  int num_cus = 256;
  // tuning knobs (r3d_ctx_set_tuning)
  int fuse_blocks = 0;   // 0 auto
  int fuse_prefetch = 0; // 0 auto, 1 off, 2 on: stage the inputs of a launch in the Infinity Cache with a read-only sweep first
  int fuse_chunk_mb = 0; // 0 auto: input bytes staged (and fused) per step when the prefetch is on
  // fuse_prefetch auto: stage a launch's small-share inputs when they exceed this many MB.  Round 2 had 64 ("less than that
  // is usually still in the cache from its producer"); measured in round 3 (bench.py --workload regimes): a 49 MB raster that
  // an H2D copy has just written is NOT in the Infinity Cache -- the launch runs at 0.49 of peak plain, 0.82 staged -- while
  // staging a raster that IS cached costs 4 %.  Below ~8 MB the extra launch eats the gain.
  int fuse_stage_auto_mb = 8;
  // ... and, since round 4, only when those inputs are NOT presumed to sit in the Infinity Cache already: the library keeps a
  // per-device record of the input ranges its launches have read lately (r3d_inputs_* below) and forgets a range the moment
  // it writes it from outside the cache (H2D copies, the host pipeline's uploads, collective receives, frees).  This many MB
  // of inputs are presumed to survive in the 256 MiB cache while a launch's write stream passes through it.
  int fuse_resident_mb = 128;
  // 1: a staged f32 lane launch reads its depth chunk in its own first workgroups (no separate sweep launch); 0: the sweep of
  // rounds 1-5 in front (A/B, escape hatch)
  int fuse_stage_fold = 1;
  int fuse_sweeps = 0;        // read-only statistic: staging sweeps the fused launches of this ctx have enqueued so far
  int fuse_inputs_fresh = 0;  // write-only knob: a foreign producer (torch, another library) has rewritten input buffers
  int nn_variant = 0;     // sources per lane (1, 2, 4; 0 = auto)
  // the ICP loop that ran last on this ctx (r3d_icp_iterate / _plane): a call with the same state, source, match buffer and
  // index and no state reset / write to that source through the library in between is the SAME loop going on -- its first
  // iteration may start from the previous matches like every other one (nn_warm_kernel)
  const void *loop_state = nullptr, *loop_src = nullptr, *loop_idx = nullptr, *loop_index = nullptr;
  size_t loop_src_bytes = 0;          // ... and the extent of that source cloud: r3d_wrote() ends the loop on ANY overlapping write
  const void* select_ws = nullptr;   // the selection workspace (r3d_plane.hip) whose histogram is known to be all zero ...
  int select_ws_buckets = 0;         // ... for this many classes
  int nn_warm = 0;        // 0 auto: repeated presorted queries start from the previous matches' distances, ICP loops use
                          // nn_warm_kernel from their second iteration on; 1 off; 2 / 3: never / always nn_warm_kernel (A/B)
  int apply_blocks = 0;
  int voxel_path = 0;     // big inserts: 0 auto (a sample of the cloud decides), 1 LDS-set + CAS kernel, 2 sort-merge (r3d_voxel_merge.hip)
  int voxel_last_path = 0; // read-only: the path the last r3d_voxelset_insert took (1 / 2)
  int octree_timing = 0;  // 1: the device octree serialiser puts HIP events around its four launches and waits for them ...
  int octree_us[4] = {};  // ... read-only: microseconds of count, scan, own, link of the last such call (r3d_octree.hip)
  int tsdf_cloud_chunk = 0;  // 4 x 4 x 4 voxel blocks per chunk of r3d_tsdf_integrate_cloud's band (0 auto: 16384); results never depend on it
  int voxel_dedupe = 0;   // 0 auto (on), 1 off, 2 on: per-workgroup LDS dedupe in front of the global hash set; 3: on, with the
                          // flush barrier inside its `if` (A/B against DESIGN 4.5b's finding only)
  // HIP-event stopwatch
  hipEvent_t ev_start = nullptr, ev_stop = nullptr;
  // the grow-only device workspaces, one per r3d_workspace entry (the table above); r3d_scratch is their only allocator
  static constexpr int kScratchSlots = 15;
  void* scratch[kScratchSlots] = {};
  size_t scratch_bytes[kScratchSlots] = {};
  // the (radius, sigma_s, sigma_r) whose tables sit in kWsBilateral: a repeated r3d_depth_bilateral uploads nothing.  radius -1 =
  // none; the call validates its arguments before it compares them with this key, so no call matches the empty key
  int bilateral_radius = -1;
  double bilateral_sigma_s = 0, bilateral_sigma_r = 0;
  // pinned staging buffers of the host pipeline: slot = ((direction * kPipeBufs + array) * 2 + parity)
  static constexpr int kPipeBufs = 2;   // arrays per direction (depth + colour in, xyz + rgba out)
  static constexpr int kPinnedSlots = 2 * kPipeBufs * 2;
  void* pinned[kPinnedSlots] = {};
  size_t pinned_bytes[kPinnedSlots] = {};
  hipEvent_t ev_pipe[6] = {};           // host pipeline: done[2], uploaded[2], entry, spare
  hipStream_t upload_stream = nullptr;  // H2D side of the host pipeline (full-duplex PCIe)
};
static_assert(kWsEnd == r3d_ctx::kScratchSlots, "one r3d_ctx::scratch entry per r3d_workspace");

struct r3d_voxelset {   // r3d_voxel.hip; its fields are also read by the sort-merge insert (r3d_voxel_merge.hip)
  r3d_ctx* ctx = nullptr;
  int device = 0;  // kept so that destroy never has to touch a ctx that may already be gone
  double res = 0.1;
  double factor = 10.0;
  uint64_t* d_table = nullptr;
  uint64_t capacity = 0;  // power of two
  int log2cap = 0;
  unsigned long long* d_counters = nullptr;  // [0] voxels, [1] ignored points, [2] overflow, [3] compaction cursor
  bool pristine = true;   // nothing has gone into the table since it was created / cleared (the merge then need not read it)
};

struct r3d_camera {
  r3d_ctx* ctx = nullptr;
  int device = 0;  // for destroy, which must not dereference ctx
  int height = 0, width = 0;
  double fx = 0, fy = 0, cx = 0, cy = 0;
  double* d_u = nullptr;  // [width]  (i-cx)/fx
  double* d_v = nullptr;  // [height] (j-cy)/fy
};

// thread-local error text
void r3d_set_error(const char* fmt, ...);
int r3d_fail_hip(hipError_t e, const char* what, const char* file, int line);

#define R3D_HIP(call)                                                       \
  do {                                                                      \
    hipError_t e_ = (call);                                                 \
    if (e_ != hipSuccess) return r3d_fail_hip(e_, #call, __FILE__, __LINE__); \
  } while (0)

#define R3D_REQUIRE(cond, ...)  \
  do {                          \
    if (!(cond)) {              \
      r3d_set_error(__VA_ARGS__); \
      return R3D_ERR_INVALID;   \
    }                           \
  } while (0)

// make the ctx's device current for the calling thread
int r3d_ctx_enter(r3d_ctx* ctx);
// the context a communicator was created on (its collectives run on that context's stream); r3d_comm.hip
struct r3d_comm;
r3d_ctx* r3d_comm_context(const r3d_comm* comm);

// Which input ranges are presumed to sit in the device's Infinity Cache (r3d_ctx.hip; one record per device, shared by its
// contexts).  _resident: [p, p+bytes) was read by a launch of the library and fewer than `budget_bytes` of other inputs have
// gone through since.  _read: a launch has just been enqueued that reads the range.  _written: the range has been (or is
// about to be) written from outside the cache, or freed -- forget it.  _forget_all: the hint for foreign producers.
bool r3d_inputs_resident(r3d_ctx* ctx, const void* p, size_t bytes, size_t budget_bytes);
void r3d_inputs_read(r3d_ctx* ctx, const void* p, size_t bytes, size_t budget_bytes);
void r3d_inputs_written(r3d_ctx* ctx, const void* p, size_t bytes);
void r3d_inputs_forget_all(r3d_ctx* ctx);
int r3d_inputs_tracked(r3d_ctx* ctx);

// Every entry point that writes a CALLER's device range (or frees one) says so here: the range is no longer presumed cached
// (r3d_inputs_written) and an ICP loop whose source cloud it overlaps is over (its next call starts cold, not "warm" from
// matches that describe other points).  Results never depend on either record; speed does.
void r3d_wrote(r3d_ctx* ctx, const void* p, size_t bytes);

// The one allocator of the context's workspaces (device memory, grow-only): *p = at least `bytes` bytes (16 for 0) of `which`.
// Growing waits for both streams, drops the old range from the residency record and frees it; the contents are not kept.
int r3d_scratch(r3d_ctx* ctx, r3d_workspace which, size_t bytes, void** p);
// ... and of a block that is divided (r3d_carve.h): `which` holds c.bytes and c is placed there.  carve.at() is the only way in.
inline int r3d_scratch(r3d_ctx* ctx, r3d_workspace which, r3d_carve& c) {
  void* p = nullptr;
  const int rc = r3d_scratch(ctx, which, c.bytes, &p);
  c.place(p);
  return rc;
}
// The same for a slab an object owns for its lifetime (the NN index, the mesh index): *slab = hipMalloc(c.bytes), c placed there.
inline hipError_t r3d_carve_malloc(r3d_carve& c, void** slab) {
  const hipError_t e = hipMalloc(slab, c.bytes);
  c.place(e == hipSuccess ? *slab : nullptr);
  return e;
}

// Chunked, double-buffered host<->device pipeline (r3d_hostpipe.hip).  Items [lo, lo+n) of the batch are uploaded
// to d_in + lo*in_item_bytes, `launch(lo, n)` enqueues the kernel for them, and d_out + lo*out_item_bytes comes back.
int r3d_host_pipeline(r3d_ctx* ctx, int64_t n_items, size_t in_item_bytes, size_t out_item_bytes, const void* h_in,
                      void* h_out, void* d_in, void* d_out, const std::function<int(int64_t, int64_t)>& launch);
// The same with up to r3d_ctx::kPipeBufs arrays per direction travelling together (e.g. depth + colour in, xyz + rgba out).
struct r3d_pipe_buf {
  void* h;            // host array (pageable or pinned); inputs are only read
  void* d;            // whole-batch device array
  size_t item_bytes;  // bytes per item (frame)
};
int r3d_host_pipeline_multi(r3d_ctx* ctx, int64_t n_items, const r3d_pipe_buf* ins, int n_in, const r3d_pipe_buf* outs,
                            int n_out, const std::function<int(int64_t, int64_t)>& launch);

// r3d_voxel.hip: what a kernel outside that file needs to insert into a voxel set (r3d_fuse.hip's fused RGBD + voxel launch)
int r3d_voxelset_device_view(r3d_voxelset* vs, r3d_ctx** ctx, double* factor, uint64_t** d_table, int* log2cap,
                             unsigned long long** d_counters);

// the two insert paths of a voxel set, and how a big insert chooses between them (r3d_voxel.hip; path 2 and whether it is
// possible at all: r3d_voxel_merge.hip, whose one entry point r3d_voxelset_insert_path calls and nobody else)
bool r3d_voxelset_sort_feasible(const r3d_voxelset* vs, int64_t n_points, bool forced);
__attribute__((visibility("hidden"))) int r3d_voxelset_insert_sorted(r3d_voxelset* vs, const float* d_xyz, int64_t n_points);
int r3d_voxelset_sample(r3d_voxelset* vs, const float* d_xyz, int64_t n_points, int64_t n_insert, double cas_base_ps, bool* sort_out);
int r3d_voxelset_insert_path(r3d_voxelset* vs, const float* d_xyz, int64_t n_points, int path);
// A table of packed keys (kEmpty = free) holding `n` keys -> their ascending Morton codes in kWsOut (kWsSpare is the sort's
// spare, d_counters[3] the compaction cursor); asynchronous.  Shared by the voxel set and the voxel grid (r3d_voxelgrid.hip).
int r3d_voxel_table_sorted_codes(r3d_ctx* ctx, const uint64_t* d_table, uint64_t capacity, unsigned long long* d_counters,
                                 int64_t n, uint64_t** d_list_out);

// The set's distinct voxels as ascending Morton codes in HBM (kWsOut of its context, which is entered; kWsSpare and kWsCounts are
// free again when this returns); an overflowed set -> R3D_ERR_NOMEM as r3d_voxelset_codes reports it.  For r3d_octree.hip.
int r3d_voxelset_sorted_codes_device(r3d_voxelset* vs, r3d_ctx** ctx, double* resolution, uint64_t** d_list_out, int64_t* n_out);

// Device -> pageable host memory through pinned staging chunks (r3d_hostpipe.hip); synchronous.
int r3d_download_pageable(r3d_ctx* ctx, void* h_dst, const void* d_src, size_t bytes);

// Stable LSD radix sort of 64-bit keys by their bits [first_bit, bits) (r3d_sort.hip); d_tmp holds n keys.
int r3d_radix_sort_u64(r3d_ctx* ctx, uint64_t* d_keys, uint64_t* d_tmp, int64_t n, int bits, int first_bit = 0,
                       uint64_t** d_result = nullptr, bool first_hist_done = false);
constexpr int kSortTile = 4096;   // keys per workgroup of every sort kernel
int r3d_radix_sort_workspace(r3d_ctx* ctx, int64_t n, uint32_t** hist_out, uint32_t** totals_out, int* n_blocks_out);
constexpr int r3d_sort_stride(int n_blocks) { return (n_blocks + 7) & ~7; }   // counters per histogram row (32-byte aligned rows)
// hist[bin][tile] (n_bins rows of `stride` counters) -> exclusive prefixes over the tiles, in place; totals[bin] = the bin's count
void r3d_sort_launch_scan(r3d_ctx* ctx, uint32_t* hist, int n_blocks, int stride, uint32_t* totals, int n_bins = 256);

// r3d_fpfh.hip: idx / dist of the nearest 33-float row of b for every row of a; the partial minima go to the workspace `part`
int r3d_match_nearest(r3d_ctx* ctx, const float* d_a, int64_t na, const float* d_b, int64_t nb, uint32_t* d_idx_out, float* d_dist_out,
                      r3d_workspace part);

// r3d_consistency.hip: the launches r3d_consistency_host.cpp drives (asynchronous on the ctx stream, arguments checked by then).
// d_rows: [n_frames][n_sources] relative pose rows shaped like r3d_tsdf_dev::TsdfPoseRow, the source index in pad[0].  The mask
// pair is the compaction step of r3d_compact_dev.h: hist holds the tiles' counts after _count, their exclusive prefixes for _write.
struct r3d_consistency_rule {
  float rel_tol;
  int min_consistent, max_violations;
};
void r3d_consistency_launch(r3d_ctx* ctx, const r3d_camera* cam, double depth_scale, const void* d_depth, int depth_dtype, const void* d_rows,
                            int n_frames, int n_sources, const r3d_consistency_rule& rule, uint8_t* d_votes, uint8_t* d_keep,
                            float* d_filtered);
void r3d_mask_count_launch(r3d_ctx* ctx, const uint8_t* d_keep, int64_t n, int tiles, uint32_t* hist);
void r3d_mask_write_launch(r3d_ctx* ctx, const float* d_xyz, const uint32_t* d_rgba, int64_t n, const uint8_t* d_keep, int tiles,
                           const uint32_t* hist, float* d_xyz_out, uint32_t* d_rgba_out, uint64_t rows);

// r3d_mesh_smooth.hip: the launches r3d_mesh_smooth_host.cpp drives (asynchronous on the ctx stream, arguments checked by then).
// vb: the bits of a vertex index.  Side keys are (u << vb | v), 1 << 2vb for no side; corner keys (v << 32 | 3t + c), v = 1 << vb
// for an invalid triangle.  The heads pair is the compaction step of r3d_compact_dev.h over the sorted side keys: the distinct ones
// go to d_distinct (room for n), a run of length 1 sets d_boundary (may be NULL).  _rows: row_start[0 .. nv] by lower bound in
// the distinct keys, and the first `rows` neighbour entries.  _step: one umbrella step, d_in != d_out.
void r3d_mesh_side_keys_launch(r3d_ctx* ctx, const int32_t* d_tri, int64_t nt, uint32_t nv, int vb, uint64_t* d_keys);
void r3d_mesh_heads_count_launch(r3d_ctx* ctx, const uint64_t* d_sorted, int64_t n, int vb, int tiles, uint32_t* hist);
void r3d_mesh_heads_write_launch(r3d_ctx* ctx, const uint64_t* d_sorted, int64_t n, int vb, int tiles, const uint32_t* hist,
                                 uint64_t* d_distinct, uint8_t* d_boundary);
void r3d_mesh_rows_launch(r3d_ctx* ctx, const uint64_t* d_distinct, uint32_t n_distinct, uint32_t nv, int vb, uint32_t* d_row_start,
                          uint32_t* d_neighbours, uint32_t rows);
void r3d_mesh_step_launch(r3d_ctx* ctx, const float* d_in, float* d_out, uint32_t nv, const uint32_t* d_row_start,
                          const uint32_t* d_neighbours, const uint8_t* d_locked, double factor);
void r3d_mesh_corner_keys_launch(r3d_ctx* ctx, const int32_t* d_tri, int64_t nt, uint32_t nv, int vb, uint64_t* d_keys);
void r3d_mesh_normals_launch(r3d_ctx* ctx, const float* d_xyz, uint32_t nv, const int32_t* d_tri, const uint64_t* d_sorted, uint32_t n_keys,
                             const float* d_fallback, float* d_out);

// r3d_nnindex.hip: the index's own copy of the target cloud (original order), its size and its context
int r3d_nn_index_target(r3d_nn_index* index, const float** d_tgt, int64_t* n_tgt, r3d_ctx** ctx);
// r3d_icp.hip: last kernel of a sums pass (partial rows -> 18 sums [-> solve + ICP state])
int r3d_icp_sums_finish(r3d_ctx* ctx, const double* d_partials, int n_rows, double* d_sums_out, int with_scale, double* d_state);
// r3d_nnindex.hip: presorted culled query + fused sums + device solve (one iteration's worth, used by r3d_icp_iterate)
int r3d_nn_index_query_solve(r3d_nn_index* index, const float* d_src, int64_t n_src, uint32_t* d_idx_out, float* d_d2_out,
                             float max_d2, double* d_sums_out, int with_scale, double* d_state, int small_motion);
// presorted query of an ICP loop; small_motion: the sources moved by one ICP step since this same query ran last (its matches,
// still in d_idx_out, bound the new search tightly: wave-local kernel).  d_src_orig + d_T_move (device, 12 doubles of a 4x4):
// when the wave-local kernel runs, it first writes d_src = T . d_src_orig itself (*moved_out = 1) -- the caller then skips
// its move launch; otherwise d_src is searched as it is (*moved_out = 0).
int r3d_nn_index_query_step(r3d_nn_index* index, const float* d_src, int64_t n_src, uint32_t* d_idx_out, float* d_d2_out,
                            int small_motion, const float* d_src_orig, const double* d_T_move, int* moved_out);

// The continuity record of the ICP loops (r3d_ctx::loop_*).  _going_on: is this call the loop that ran last on the ctx, with
// nothing in between that ended it (r3d_icp_state_reset, r3d_wrote on the source)?  Its first iteration then starts from the
// previous matches too.  _remember: a call that ran at least one iteration over an index says so when it is done.
static inline bool r3d_icp_loop_going_on(const r3d_ctx* ctx, const void* index, const void* d_state, const void* d_src, const void* d_idx) {
  return index && ctx->loop_state == d_state && ctx->loop_src == d_src && ctx->loop_idx == d_idx && ctx->loop_index == index;
}
static inline void r3d_icp_loop_remember(r3d_ctx* ctx, const void* index, const void* d_state, const void* d_src, int64_t n_src,
                                         const void* d_idx) {
  ctx->loop_state = d_state;
  ctx->loop_src = d_src;
  ctx->loop_src_bytes = (size_t)n_src * 12;
  ctx->loop_idx = d_idx;
  ctx->loop_index = index;
}
// r3d_icp.hip: n_iters iterations of (presorted query, sums pass, move) for the loops whose sums pass is their own -- plane and
// coloured ICP.  enqueue_sums(last) enqueues one pass over d_src / d_idx / d_d2 that ends in the state update; `last` is true in
// the call's final iteration.  d_src_orig (or NULL): the cloud as it was before the loop began.  Keeps the continuity record.
int r3d_icp_loop_run(r3d_ctx* ctx, r3d_nn_index* index, const float* d_src_orig, float* d_src, int64_t n_src, uint32_t* d_idx,
                     float* d_d2, int n_iters, double* d_state, const std::function<int(bool)>& enqueue_sums);

// Do the byte ranges [a, a + a_bytes) and [b, b + b_bytes) share a byte?  A NULL pointer or an empty range overlaps nothing.
static inline bool r3d_ranges_overlap(const void* a, size_t a_bytes, const void* b, size_t b_bytes) {
  if (!a || !b || !a_bytes || !b_bytes) return false;
  const uintptr_t a0 = (uintptr_t)a, b0 = (uintptr_t)b;
  return a0 < b0 + b_bytes && b0 < a0 + a_bytes;
}
// Does any of the n_out output ranges overlap a later one of them, or any of the n_in input ranges?
struct r3d_range {
  const void* p;
  size_t bytes;
};
static inline bool r3d_any_overlap(const r3d_range* outs, int n_out, const r3d_range* ins, int n_in) {
  for (int i = 0; i < n_out; ++i) {
    for (int j = i + 1; j < n_out; ++j)
      if (r3d_ranges_overlap(outs[i].p, outs[i].bytes, outs[j].p, outs[j].bytes)) return true;
    for (int j = 0; j < n_in; ++j)
      if (r3d_ranges_overlap(outs[i].p, outs[i].bytes, ins[j].p, ins[j].bytes)) return true;
  }
  return false;
}

static inline size_t r3d_depth_size(int dt) { return dt == R3D_DEPTH_U8 ? 1 : dt == R3D_DEPTH_U16 ? 2 : 4; }
static inline size_t r3d_xyz_size(int dt) { return dt == R3D_F32 ? 4 : 8; }
