// OctoMap ".bt" records of the pruned octree, built on the GPU from ascending unique 48-bit Morton codes (gfx950 / MI355X).
// Byte-identical to the host serialiser (build_bt in r3d_octree_host.cpp); DESIGN.md 4.5f has the derivation and the measurements.
//
// One uint16 record per INNER node, depth-first pre-order; child c's 2-bit field at bits 2c..2c+1 (10 leaf, 11 inner).  No
// recursion: for code j (3-bit digits, digit 0 on top)
//   cpl[j]  leading digits shared with code j-1 (-1 for j = 0): a node of depth e STARTS at j iff e > cpl[j];
//   top[j]  min(15, f - 1), f = depth of the topmost FULL subtree that holds code j (16: none) -- the deepest inner depth
//           that starts at j.  A subtree of depth d is full iff the 8^(16-d) codes with the same d-digit prefix are all there:
//           codes ascend, so the first and the last of them sitting 8^(16-d) - 1 places apart says it all (two loads per depth);
//   the inner nodes that start at j are those of depths cpl+1 .. top: pre-order = (start index, depth), so the record of
//   depth d sits at base[j] + d - cpl - 1, base = exclusive prefix of cnt[j] = max(0, top - cpl).
// Every emitted node tells its parent's record its field.  For all but the topmost node that starts at j the parent starts at j
// too: plain stores, every record has exactly one owner (own_kernel).  The topmost one's parent is owned by the first code with
// the same cpl[j]-digit prefix (a galloping lower bound backwards from j): ONE foreign OR per code, in a later launch
// (link_kernel).  OR commutes: the bytes do not depend on launch geometry or timing.
//
//   count_kernel  tile of 4096 codes per workgroup: validation, cpl | top -> meta (1 B/code), the tile's record and leaf counts
//   scan_kernel   one workgroup: 64-bit exclusive prefix of the tiles' record counts, totals
//   own_kernel    prefix inside the tile (wave shuffle scans), the owned records, every code's place in its tile (2 B/code)
//   link_kernel   one no-return 32-bit atomic OR per code into the word that holds its parent's record
// The records are built in ctx scratch (4-byte aligned, padded to whole words): the atomics never touch a caller's bytes.
#include <string>

#include "r3d_internal.h"
#include "r3d_sort_dev.h"

namespace {

constexpr int kThreads = 256;
constexpr int kOctreeTile = 4096;   // codes per workgroup of count_kernel / own_kernel
constexpr int kRounds = kOctreeTile / kThreads;
constexpr int kWaves = kThreads / 64;
constexpr int kPerWave = kOctreeTile / kWaves;
constexpr int64_t kMaxCodes = (int64_t)1 << 36;   // far beyond any HBM; keeps every tile index inside 32 bits
static_assert(kOctreeTile == r3d_sort::kTile && kThreads == r3d_sort::kThreads, "the tile layout is the sort's");

// flags[0] smallest index whose code is not above its predecessor, [1] some code has bits above 48, [2] records, [3] leaves
constexpr int kFlags = 4;

// leading 3-bit digits two 48-bit codes share, 0..15 (equal or oversized codes are refused before anything is built from this)
__device__ __forceinline__ int shared_digits(uint64_t a, uint64_t b) {
  const uint64_t x = a ^ b;
  if (x == 0) return 15;
  const int s = 15 - (63 - __clzll((long long)x)) / 3;
  return s < 0 ? 0 : s;
}

// min(15, f - 1): walks up from depth 15 while the subtree around code j is full
__device__ __forceinline__ int top_inner_depth(const uint64_t* __restrict__ codes, int64_t n, int64_t j, uint64_t c) {
  int top = 15;
#pragma unroll 1   // (most codes leave at depth 15; unrolled 15 x 16 rounds the kernel outgrows the instruction cache)
  for (int d = 15; d >= 1; --d) {
    const int64_t sz = (int64_t)1 << (3 * (16 - d));
    const uint64_t m = (uint64_t)sz - 1;
    if (sz > n) break;
    const int64_t first = j - (int64_t)(c & m);
    if (first < 0 || first + sz > n) break;
    if (codes[first] != (c & ~m) || codes[first + sz - 1] != (c | m)) break;
    top = d - 1;
  }
  return top;
}

// element e of a tile: lane (e & 63) of wave (e >> 10), round ((e >> 6) & 15) -- consecutive lanes, consecutive codes
__device__ __forceinline__ int64_t tile_first(int64_t tile) {
  return tile * kOctreeTile + (int64_t)(threadIdx.x >> 6) * kPerWave + (threadIdx.x & 63);
}

__global__ __launch_bounds__(kThreads) void octree_count_kernel(const uint64_t* __restrict__ codes, int64_t n, uint8_t* __restrict__ meta,
                                                                uint32_t* __restrict__ tile_cnt, uint32_t* __restrict__ tile_leaf,
                                                                unsigned long long* __restrict__ flags) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int64_t first = tile_first(blockIdx.x);
  uint64_t c[kRounds];
#pragma unroll
  for (int r = 0; r < kRounds; ++r) {
    const int64_t j = first + r * 64;
    c[r] = j < n ? codes[j] : 0;
  }
  uint32_t cnt = 0, leaf = 0;
  unsigned long long bad = ~0ull;
  bool big = false;
#pragma unroll
  for (int r = 0; r < kRounds; ++r) {
    const int64_t j = first + r * 64;
    uint64_t prev = __shfl_up(c[r], 1, 64);   // the code in front: the neighbouring lane's, or (lane 0) the last of the round before
    if (lane == 0) prev = (j > 0 && j < n) ? codes[j - 1] : 0;
    if (j < n) {
      if (j > 0 && c[r] <= prev && (unsigned long long)j < bad) bad = (unsigned long long)j;
      big |= (c[r] >> 48) != 0;
      const int cpl = j > 0 ? shared_digits(c[r], prev) : -1;
      const int top = top_inner_depth(codes, n, j, c[r]);
      meta[j] = (uint8_t)((top << 4) | (cpl & 15));
      cnt += top > cpl ? (uint32_t)(top - cpl) : 0u;
      leaf += top >= cpl ? 1u : 0u;
    }
  }
  if (bad != ~0ull) atomicMin(&flags[0], bad);
  if (big) atomicOr(&flags[1], 1ull);
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    cnt += __shfl_down(cnt, off, 64);
    leaf += __shfl_down(leaf, off, 64);
  }
  __shared__ uint32_t sh[2][kWaves];
  if (lane == 0) {
    sh[0][wave] = cnt;
    sh[1][wave] = leaf;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    tile_cnt[blockIdx.x] = sh[0][0] + sh[0][1] + sh[0][2] + sh[0][3];
    tile_leaf[blockIdx.x] = sh[1][0] + sh[1][1] + sh[1][2] + sh[1][3];
  }
}

// one workgroup: tile_base = exclusive prefix of tile_cnt in 64 bits (16 records per code can pass 2^32), the two totals
__global__ __launch_bounds__(kThreads) void octree_scan_kernel(const uint32_t* __restrict__ tile_cnt, const uint32_t* __restrict__ tile_leaf,
                                                               int64_t tiles, uint64_t* __restrict__ tile_base,
                                                               unsigned long long* __restrict__ flags) {
  __shared__ uint64_t wave_total[kWaves];
  __shared__ uint64_t leaf_total[kWaves];
  uint64_t carry = 0, leaves = 0;
  for (int64_t seg = 0; seg < tiles; seg += kThreads) {
    const int64_t i = seg + threadIdx.x;
    const uint64_t v = i < tiles ? tile_cnt[i] : 0;
    leaves += i < tiles ? tile_leaf[i] : 0;
    const uint64_t before = r3d_sort::block_exclusive_scan_256(v, wave_total);
    if (i < tiles) tile_base[i] = carry + before;
    carry += wave_total[0] + wave_total[1] + wave_total[2] + wave_total[3];
    __syncthreads();   // wave_total is rewritten by the next segment
  }
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) leaves += __shfl_down(leaves, off, 64);
  if ((threadIdx.x & 63) == 0) leaf_total[threadIdx.x >> 6] = leaves;
  __syncthreads();
  if (threadIdx.x == 0) {
    flags[2] = carry;
    flags[3] = leaf_total[0] + leaf_total[1] + leaf_total[2] + leaf_total[3];
  }
}

// the records every code owns: depths cpl+1 .. top, each naming the child that starts at the same code (11 while the chain goes
// on, 10 at its end: a voxel or a pruned subtree).  pre[j] = the first of them, counted from the tile's base.
__global__ __launch_bounds__(kThreads) void octree_own_kernel(const uint64_t* __restrict__ codes, int64_t n, const uint8_t* __restrict__ meta,
                                                              const uint64_t* __restrict__ tile_base, uint16_t* __restrict__ pre,
                                                              uint16_t* __restrict__ rec) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int64_t first = tile_first(blockIdx.x);
  uint64_t c[kRounds];
  uint32_t m[kRounds];
#pragma unroll
  for (int r = 0; r < kRounds; ++r) {
    const int64_t j = first + r * 64;
    c[r] = j < n ? codes[j] : 0;
    m[r] = j < n ? meta[j] : 0xfu;   // top 0, cpl 15: owns nothing
  }
  // where the lane's records start inside the wave's quarter: wave scans of the counts, two rounds to a word (a wave's round
  // holds at most 64 x 16 records)
  uint32_t off[kRounds], run = 0;
#pragma unroll
  for (int r = 0; r < kRounds; r += 2) {
    uint32_t cn[2];
#pragma unroll
    for (int q = 0; q < 2; ++q) {
      const int64_t j = first + (r + q) * 64;
      const int start = j == 0 ? 0 : (int)(m[r + q] & 15u) + 1, top = (int)(m[r + q] >> 4);
      cn[q] = top >= start ? (uint32_t)(top - start + 1) : 0u;
    }
    const uint32_t inc = r3d_sort::wave_inclusive_scan(cn[0] | (cn[1] << 16), lane);
    const uint32_t tot = (uint32_t)__shfl((int)inc, 63, 64);
    off[r] = run + (inc & 0xffffu) - cn[0];
    run += tot & 0xffffu;
    off[r + 1] = run + (inc >> 16) - cn[1];
    run += tot >> 16;
  }
  __shared__ uint32_t wave_sum[kWaves];
  if (lane == 0) wave_sum[wave] = run;
  __syncthreads();
  uint32_t wave_base = 0;
  for (int w = 0; w < wave; ++w) wave_base += wave_sum[w];
  const uint64_t base = tile_base[blockIdx.x];
#pragma unroll
  for (int r = 0; r < kRounds; ++r) {
    const int64_t j = first + r * 64;
    if (j >= n) continue;
    const uint32_t local = wave_base + off[r];   // <= 4095 x 16
    pre[j] = (uint16_t)local;
    const int start = j == 0 ? 0 : (int)(m[r] & 15u) + 1, top = (int)(m[r] >> 4);
    uint16_t* out = rec + base + local;
#pragma unroll
    for (int k = 0; k < 16; ++k) {
      const int d = start + k;
      if (d <= top) out[k] = (uint16_t)((d < top ? 3u : 2u) << (2 * (uint32_t)((c[r] >> (3 * (15 - d))) & 7)));
    }
  }
}

// the topmost node that starts at code j (depth cpl + 1) into its parent's record: the depth-cpl node around j, owned by the
// first code with j's cpl-digit prefix.  That code is found by galloping backwards (j - 1, j - 3, j - 7 ...: neighbouring lanes
// read neighbouring codes) and bisecting the last stride -- a handful of probes for the deep nodes most codes hang from.
__global__ __launch_bounds__(kThreads) void octree_link_kernel(const uint64_t* __restrict__ codes, int64_t n, const uint8_t* __restrict__ meta,
                                                               const uint64_t* __restrict__ tile_base, const uint16_t* __restrict__ pre,
                                                               uint64_t n_records, uint32_t* __restrict__ rec32) {
  const int64_t j = (int64_t)blockIdx.x * kThreads + threadIdx.x;
  if (j == 0 || j >= n) return;
  const uint32_t m = meta[j];
  const int d = (int)(m & 15u), top = (int)(m >> 4);
  if (top < d) return;   // inside a pruned subtree: nothing starts here
  const uint64_t c = codes[j];
  int64_t j0 = 0;
  if (d > 0) {
    const uint64_t want = c & ~(((uint64_t)1 << (3 * (16 - d))) - 1);   // the first code the parent could hold
    int64_t hi = j, lo = j - 1, step = 2;                              // codes[hi] >= want; find lo with codes[lo] < want (or -1)
    while (lo >= 0 && codes[lo] >= want) {
      hi = lo;
      lo = hi - step;
      step <<= 1;
    }
    if (lo < -1) lo = -1;
    while (hi - lo > 1) {
      const int64_t mid = lo + ((hi - lo) >> 1);
      if (codes[mid] >= want) hi = mid;
      else lo = mid;
    }
    j0 = hi;
  }
  const int start0 = j0 == 0 ? 0 : (int)(meta[j0] & 15u) + 1;
  const uint64_t pos = tile_base[j0 / kOctreeTile] + pre[j0] + (uint64_t)(d - start0);
  const uint32_t field = (d < top ? 3u : 2u) << (2 * (uint32_t)((c >> (3 * (15 - d))) & 7));
  if (pos < n_records) atomicOr(&rec32[pos >> 1], field << (16 * (uint32_t)(pos & 1)));   // result unused: a no-return atomic
}

struct Workspace {
  uint8_t* meta = nullptr;
  uint16_t* pre = nullptr;
  unsigned long long* flags = nullptr;
  uint64_t* tile_base = nullptr;
  uint32_t *tile_cnt = nullptr, *tile_leaf = nullptr;
  int64_t tiles = 0;
  hipEvent_t ev[5] = {};   // "octree_timing": around count, scan, own, link
};

// "octree_timing" 1: HIP events around the four launches; the elapsed microseconds land in the ctx (octree_*_us tuning keys)
int timing_mark(r3d_ctx* ctx, Workspace& w, int k) {
  if (!ctx->octree_timing) return R3D_OK;
  if (!w.ev[k]) R3D_HIP(hipEventCreate(&w.ev[k]));
  R3D_HIP(hipEventRecord(w.ev[k], ctx->stream));
  return R3D_OK;
}

void timing_finish(r3d_ctx* ctx, Workspace& w, bool filled) {
  if (ctx->octree_timing && w.ev[0] && w.ev[2] && (!filled || w.ev[4])) {
    const int last = filled ? 4 : 2;
    if (hipEventSynchronize(w.ev[last]) == hipSuccess)
      for (int k = 0; k < last; ++k) {
        float ms = 0.f;
        if (hipEventElapsedTime(&ms, w.ev[k], w.ev[k + 1]) == hipSuccess) ctx->octree_us[k] = (int)(ms * 1000.f + 0.5f);
      }
  }
  for (hipEvent_t& e : w.ev)
    if (e) {
      (void)hipEventDestroy(e);
      e = nullptr;
    }
}

// count + scan; waits for the sizes; refuses bad codes.  Nothing a caller can see has been written when this returns.
int octree_sizes(r3d_ctx* ctx, const uint64_t* d_codes, int64_t n, Workspace& w, int64_t* n_records, int64_t* n_leaves) {
  int rc;
  w.tiles = (n + kOctreeTile - 1) / kOctreeTile;
  r3d_carve a, b;
  const auto meta = a.take<uint8_t>(n, 16);
  const auto pre = a.take<uint16_t>(n, 16);
  const auto flags = b.take<unsigned long long>(kFlags, 64);
  const auto tile_base = b.take<uint64_t>(w.tiles, 64);
  const auto tile_cnt = b.take<uint32_t>(w.tiles, 16), tile_leaf = b.take<uint32_t>(w.tiles, 16);
  if ((rc = r3d_scratch(ctx, kWsSpare, a)) || (rc = r3d_scratch(ctx, kWsCounts, b))) return rc;
  w.meta = a.at(meta), w.pre = a.at(pre);
  w.flags = b.at(flags), w.tile_base = b.at(tile_base), w.tile_cnt = b.at(tile_cnt), w.tile_leaf = b.at(tile_leaf);
  hipStream_t st = ctx->stream;
  static const unsigned long long init[kFlags] = {~0ull, 0, 0, 0};
  R3D_HIP(hipMemcpyAsync(w.flags, init, sizeof(init), hipMemcpyHostToDevice, st));
  if ((rc = timing_mark(ctx, w, 0))) return rc;
  hipLaunchKernelGGL(octree_count_kernel, dim3((unsigned)w.tiles), dim3(kThreads), 0, st, d_codes, n, w.meta, w.tile_cnt, w.tile_leaf, w.flags);
  if ((rc = timing_mark(ctx, w, 1))) return rc;
  hipLaunchKernelGGL(octree_scan_kernel, dim3(1), dim3(kThreads), 0, st, (const uint32_t*)w.tile_cnt, (const uint32_t*)w.tile_leaf, w.tiles,
                     w.tile_base, w.flags);
  if ((rc = timing_mark(ctx, w, 2))) return rc;
  R3D_HIP(hipGetLastError());
  unsigned long long h[kFlags];
  R3D_HIP(hipMemcpyAsync(h, w.flags, sizeof(h), hipMemcpyDeviceToHost, st));
  R3D_HIP(hipStreamSynchronize(st));
  R3D_REQUIRE(h[0] == ~0ull, "octree export needs strictly ascending Morton codes (violated at index %lld)", (long long)h[0]);
  R3D_REQUIRE(h[1] == 0, "Morton code above 48 bits");
  *n_records = (int64_t)h[2];
  *n_leaves = (int64_t)h[3];
  return R3D_OK;
}

// own + link into kWsIn (asynchronous); *d_rec = the records
int octree_fill(r3d_ctx* ctx, const uint64_t* d_codes, int64_t n, Workspace& w, int64_t n_records, uint16_t** d_rec) {
  void* r = nullptr;
  int rc = r3d_scratch(ctx, kWsIn, r3d_align_up((size_t)n_records, 2) * 2, &r);
  if (rc) return rc;
  hipStream_t st = ctx->stream;
  hipLaunchKernelGGL(octree_own_kernel, dim3((unsigned)w.tiles), dim3(kThreads), 0, st, d_codes, n, (const uint8_t*)w.meta,
                     (const uint64_t*)w.tile_base, w.pre, static_cast<uint16_t*>(r));
  if ((rc = timing_mark(ctx, w, 3))) return rc;
  hipLaunchKernelGGL(octree_link_kernel, dim3((unsigned)((n + kThreads - 1) / kThreads)), dim3(kThreads), 0, st, d_codes, n,
                     (const uint8_t*)w.meta, (const uint64_t*)w.tile_base, (const uint16_t*)w.pre, (uint64_t)n_records,
                     static_cast<uint32_t*>(r));
  if ((rc = timing_mark(ctx, w, 4))) return rc;
  R3D_HIP(hipGetLastError());
  *d_rec = static_cast<uint16_t*>(r);
  return R3D_OK;
}

// sorted codes of a set (device) -> sizes [-> records in scratch]; the set's context is entered
int voxelset_records(r3d_voxelset* vs, bool fill, r3d_ctx** ctx_out, double* res_out, uint16_t** d_rec, int64_t* n_records, int64_t* n_nodes) {
  uint64_t* d_codes = nullptr;
  int64_t n = 0;
  int rc = r3d_voxelset_sorted_codes_device(vs, ctx_out, res_out, &d_codes, &n);
  if (rc) return rc;
  *d_rec = nullptr;
  *n_records = *n_nodes = 0;
  if (n == 0) return R3D_OK;
  r3d_ctx* ctx = *ctx_out;
  Workspace w;
  int64_t leaves = 0;
  rc = octree_sizes(ctx, d_codes, n, w, n_records, &leaves);
  if (!rc && fill) rc = octree_fill(ctx, d_codes, n, w, *n_records, d_rec);
  timing_finish(ctx, w, !rc && fill);
  *n_nodes = *n_records + leaves;
  return rc;
}

}  // namespace

extern "C" {

int r3d_octree_bt_header(int64_t n_nodes, double resolution, char* h_buf, size_t buf_cap, size_t* n_bytes_out) {
  R3D_REQUIRE(n_bytes_out != nullptr, "r3d_octree_bt_header: n_bytes_out is NULL");
  R3D_REQUIRE(n_nodes >= 0 && resolution > 0.0, "r3d_octree_bt_header: bad argument");
  char head[256];
  const int k = snprintf(head, sizeof(head),
                         "# Octomap OcTree binary file\n# (feel free to add / change comments, but leave the first line as it is!)\n#\n"
                         "id OcTree\nsize %lld\nres %g\ndata\n",
                         (long long)n_nodes, resolution);
  R3D_REQUIRE(k > 0 && (size_t)k < sizeof(head), "r3d_octree_bt_header: header does not fit");
  *n_bytes_out = (size_t)k;
  if (!h_buf) return R3D_OK;
  R3D_REQUIRE(buf_cap >= (size_t)k, "r3d_octree_bt_header: buffer of %zu bytes is too small for %d", buf_cap, k);
  memcpy(h_buf, head, (size_t)k);
  return R3D_OK;
}

int r3d_octree_records_device(r3d_ctx* ctx, const uint64_t* d_codes_sorted, int64_t n_codes, uint16_t* d_records_out, int64_t cap_records,
                              int64_t* n_records_out, int64_t* n_nodes_out) {
  int rc = r3d_ctx_enter(ctx);
  if (rc) return rc;
  R3D_REQUIRE(n_records_out != nullptr && n_nodes_out != nullptr, "NULL size pointer");
  R3D_REQUIRE(n_codes >= 0 && n_codes < kMaxCodes, "bad number of codes %lld", (long long)n_codes);
  R3D_REQUIRE(d_records_out == nullptr || cap_records >= 0, "cap_records must be >= 0");
  *n_records_out = *n_nodes_out = 0;
  if (n_codes == 0) return R3D_OK;
  R3D_REQUIRE(d_codes_sorted != nullptr, "NULL device pointer");
  Workspace w;
  int64_t n_rec = 0, leaves = 0;
  rc = octree_sizes(ctx, d_codes_sorted, n_codes, w, &n_rec, &leaves);
  uint16_t* d_rec = nullptr;
  bool fill = false;
  if (!rc) {
    *n_records_out = n_rec;
    *n_nodes_out = n_rec + leaves;
    if (d_records_out) {
      if (cap_records < n_rec) {
        r3d_set_error("buffer holds %lld records, the tree has %lld", (long long)cap_records, (long long)n_rec);
        rc = R3D_ERR_INVALID;
      } else if (r3d_ranges_overlap(d_records_out, (size_t)n_rec * 2, d_codes_sorted, (size_t)n_codes * 8)) {
        r3d_set_error("d_records_out overlaps d_codes_sorted");
        rc = R3D_ERR_INVALID;
      } else {
        fill = true;
        rc = octree_fill(ctx, d_codes_sorted, n_codes, w, n_rec, &d_rec);
      }
    }
  }
  timing_finish(ctx, w, !rc && fill);
  if (rc || !fill) return rc;
  r3d_wrote(ctx, d_records_out, (size_t)n_rec * 2);
  R3D_HIP(hipMemcpyAsync(d_records_out, d_rec, (size_t)n_rec * 2, hipMemcpyDeviceToDevice, ctx->stream));
  return R3D_OK;
}

int r3d_voxelset_format_bt(r3d_voxelset* vs, char* h_buf, size_t buf_cap, size_t* n_bytes_out, int64_t* n_nodes_out) {
  R3D_REQUIRE(vs != nullptr && n_bytes_out != nullptr, "NULL argument");
  r3d_ctx* ctx = nullptr;
  double res = 0;
  uint16_t* d_rec = nullptr;
  int64_t n_rec = 0, nodes = 0;
  int rc = voxelset_records(vs, h_buf != nullptr, &ctx, &res, &d_rec, &n_rec, &nodes);
  if (rc) return rc;
  char head[256];
  size_t head_bytes = 0;
  if ((rc = r3d_octree_bt_header(nodes, res, head, sizeof(head), &head_bytes))) return rc;
  *n_bytes_out = head_bytes + (size_t)n_rec * 2;
  if (n_nodes_out) *n_nodes_out = nodes;
  if (!h_buf) return R3D_OK;
  if (buf_cap < *n_bytes_out) {
    r3d_set_error("r3d_voxelset_format_bt: buffer of %zu bytes is too small for %zu", buf_cap, *n_bytes_out);
    return R3D_ERR_NOMEM;
  }
  memcpy(h_buf, head, head_bytes);
  if (n_rec == 0) return R3D_OK;
  return r3d_download_pageable(ctx, h_buf + head_bytes, d_rec, (size_t)n_rec * 2);
}

int r3d_voxelset_write_bt(r3d_voxelset* vs, const char* path, int64_t* n_nodes_out) {
  R3D_REQUIRE(vs != nullptr && path != nullptr, "NULL argument");
  r3d_ctx* ctx = nullptr;
  double res = 0;
  uint16_t* d_rec = nullptr;
  int64_t n_rec = 0, nodes = 0;
  int rc = voxelset_records(vs, true, &ctx, &res, &d_rec, &n_rec, &nodes);
  if (rc) return rc;
  char head[256];
  size_t head_bytes = 0;
  if ((rc = r3d_octree_bt_header(nodes, res, head, sizeof(head), &head_bytes))) return rc;
  const r3d_text_file f = {path, head, head_bytes, d_rec, (size_t)n_rec * 2, nullptr, 0};
  if ((rc = r3d_write_device_text_files(ctx, &f, 1))) return rc;
  if (n_nodes_out) *n_nodes_out = nodes;
  return R3D_OK;
}

}  // extern "C"
