// Order-preserving compaction, stated once: keep the items that pass a predicate, in input order, every survivor
// at its output index, no atomic on a cursor.  A workgroup of 256 threads takes a tile of kSortTile items, kPer consecutive ones
// per thread (r3d_register.hip: one):  count  the threads' counts -> block_sum -> publish: one counter per tile and row;
//   scan   r3d_sort.hip's digit_scan_kernel, a workgroup per row: exclusive prefixes in place and the row's total;
//   write  tile_start = the tile's prefix + a block scan of the threads' counts, then the thread walks its own items.
// The kernels, their predicates and their store loops stay with their files.
#pragma once

#include "r3d_internal.h"
#include "r3d_sort_dev.h"

namespace r3d_compact {

constexpr int kPer = kSortTile / 256;   // consecutive items per thread
inline int tiles_of(int64_t n) { return (int)((n + kSortTile - 1) / kSortTile); }

// The counters inside a block the caller provides (kWsCounts, kWsMisc, kWsMeshCc): `rows` rows of `stride` counters,
// 32-byte aligned when the block is, then 64 bytes that begin with the rows' totals (a caller may keep words of its own behind
// them).  A call without a tile still gets one tile's row, so `totals` never aliases `hist`.
struct Counters {
  int tiles, rows, stride;
  size_t bytes;
  uint32_t *hist = nullptr, *totals = nullptr;
  Counters(int t, int r) : tiles(t), rows(r), stride(r3d_sort_stride(t > 0 ? t : 1)), bytes((size_t)r * stride * 4 + 64) {}
  void place(void* block) { hist = static_cast<uint32_t*>(block), totals = hist + (size_t)rows * stride; }
  uint32_t* row(int r) const { return hist + (size_t)r * stride; }
};

// counts -> exclusive prefixes in place, every row's total at `totals`; asynchronous
inline void launch_scan(r3d_ctx* ctx, const Counters& c) { r3d_sort_launch_scan(ctx, c.hist, c.tiles, c.stride, c.totals, c.rows); }
// the launches so far checked, the first `words` words at `totals` on the host, the stream synchronised
inline int read_totals(r3d_ctx* ctx, const Counters& c, uint32_t* h_totals, int words) {
  R3D_HIP(hipGetLastError());
  R3D_HIP(hipMemcpyAsync(h_totals, c.totals, (size_t)words * 4, hipMemcpyDeviceToHost, ctx->stream));
  R3D_HIP(hipStreamSynchronize(ctx->stream));
  return R3D_OK;
}
inline int scan_totals(r3d_ctx* ctx, const Counters& c, uint32_t* h_totals) {   // both: h_totals[r] = row r's total
  launch_scan(ctx, c);
  return read_totals(ctx, c, h_totals, c.rows);
}

__device__ __forceinline__ int64_t tile_base() { return (int64_t)blockIdx.x * kSortTile + (int64_t)threadIdx.x * kPer; }   // the thread's first item

// sum over the workgroup's 256 threads (uint32_t or uint64_t), valid in thread 0; `sh` holds 4 words
template <typename T>
__device__ __forceinline__ T block_sum(T mine, T* sh) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) mine += __shfl_down(mine, off, 64);
  if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = mine;
  __syncthreads();
  return sh[0] + sh[1] + sh[2] + sh[3];
}
__device__ __forceinline__ void publish(uint32_t* __restrict__ hist, uint32_t total) {   // the tile's counter
  if (threadIdx.x == 0) hist[blockIdx.x] = total;
}
// where the thread's first survivor goes: hist holds the tiles' exclusive prefixes, `mine` is the thread's count
__device__ __forceinline__ uint64_t tile_start(const uint32_t* __restrict__ hist, uint64_t mine, uint64_t* wave_total) {
  return hist[blockIdx.x] + r3d_sort::block_exclusive_scan_256(mine, wave_total);
}

}  // namespace r3d_compact
