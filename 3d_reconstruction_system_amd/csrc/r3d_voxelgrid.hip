// Voxel-grid downsampling on gfx950 (MI355X): one output point per occupied voxel -- the centroid of the voxel's points, their
// count and their mean colour (Open3D's voxel_down_sample, CloudCompare's spatial subsample).
//
// The voxel of a point is the voxel set's (r3d_voxel.hip): key = floor((1/res) * (double)x) + 32768 per axis, 16 bits each;
// points without a key (non-finite, outside the key range) are ignored and counted.  So the grid's voxels ARE the set's, and
// its codes go to r3d_octree_write_bt as they are.
//
// Determinism: every output bit is independent of launch geometry, of how the points are split into inserts and of their
// order, because nothing is summed in floating point.  Per axis u = factor * (double)x, k = floor(u), f = u - k in [0, 1)
// (exact), and q = floor(f * 2^31) is accumulated in a u64; colour channels are integer sums as well.  Integer adds commute,
// so LDS pre-aggregation and no-return 64-bit global atomics give the same sums in any order.  The centroid is
// (k + sum(q) / (n 2^31)) / factor in fp64, rounded once to f32: within ulp_f32 + res 2^-28 of the exact mean (the truncation to
// q costs < res 2^-31).  Colour: floor((2 S + n) / (2 n)) per channel, exact round-half-up.
//
//   grid_insert_kernel  12 B/point (+ 4 colour) read.  A workgroup walks a contiguous run of 512-point tiles and folds them into
//                       an LDS table of (key, count, sums) -- the voxel set's LDS set with accumulators beside it.  When the
//                       table holds kGridKeepBelow keys (and at the end of the run) every entry goes to HBM: one 64-bit CAS
//                       claims the voxel's slot in the key array (home_slot / hash48, linear probing: the voxel set's table
//                       layout), no-return u64 adds put the count and sums into the slot's accumulator row.
//   extract             the key array -> Morton codes (r3d_voxel_table_sorted_codes: compaction + radix sort, as for the set);
//                       grid_rows_kernel probes each code back to its slot and writes the rows in Morton order.
#include <cmath>

#include "r3d_internal.h"
#include "r3d_voxel_dev.h"

struct r3d_voxelgrid {
  r3d_ctx* ctx = nullptr;
  int device = 0;  // kept so that destroy never has to touch a ctx that may already be gone
  double res = 0.1;
  double factor = 10.0;
  bool rgb = false;
  uint64_t* d_table = nullptr;              // packed keys, kEmpty = free (the probe loops read this array only)
  unsigned long long* d_acc = nullptr;      // [slot][kAccWords]: count, sum qx, qy, qz [, sum r, g, b, unused]
  uint64_t capacity = 0;                    // power of two
  int log2cap = 0;
  unsigned long long* d_counters = nullptr; // [0] voxels, [1] ignored points, [2] points that found no slot, [3] compaction
                                            // cursor, [4] voxels holding more than 2^32 - 1 points (extract's check)
  uint64_t points_in = 0;                   // points inserted since create / clear (only above 2^32 - 1 can a count be too big)
};

namespace {

constexpr int kThreads = 256;
constexpr int kPerThread = 2;
constexpr int kTile = kThreads * kPerThread;   // points per tile
constexpr int kGridLdsLog2 = 10;
constexpr int kGridLds = 1 << kGridLdsLog2;    // LDS table entries: 1024 x (8 key + 4 count + 24 sums [+ 12 colour]) = 36 / 48 KB
constexpr int kGridKeepBelow = 256;            // flushed once it holds this many keys: a tile adds <= 512, so <= 767 of 1024 used
constexpr int64_t kMaxTilesPerWg = (int64_t)1 << 15;   // <= 2^24 points per workgroup: LDS counts and colour sums fit u32
constexpr double kFracScale = 2147483648.0;    // 2^31
using r3d_vox::kEmpty;
using r3d_vox::P3;

template <bool RGB>
constexpr int acc_words() { return RGB ? 8 : 4; }   // 64 / 32 bytes per slot: a row never straddles a 64-byte line

// One voxel's partial sums into HBM: claim the key's slot (CAS on the key array only), then no-return adds into its row.
// A key that finds no slot loses its points: they are counted in n_over.
template <bool RGB>
__device__ __forceinline__ void grid_add_global(uint64_t* __restrict__ table, unsigned long long* __restrict__ acc, uint64_t mask,
                                                int log2cap, uint64_t key, unsigned cnt, const unsigned long long q[3],
                                                const unsigned c[3], unsigned& n_new, unsigned& n_over) {
  uint64_t slot = r3d_vox::home_slot(key, log2cap);
  bool placed = false;
  for (uint64_t probe = 0; probe <= mask && !placed; ++probe) {
    const unsigned long long old = atomicCAS(reinterpret_cast<unsigned long long*>(&table[slot]), (unsigned long long)kEmpty,
                                             (unsigned long long)key);
    if (old == kEmpty) {
      ++n_new;
      placed = true;
    } else if (old == key) {
      placed = true;
    } else {
      slot = (slot + 1) & mask;
    }
  }
  if (!placed) {
    n_over += cnt;
    return;
  }
  unsigned long long* row = acc + slot * acc_words<RGB>();
  atomicAdd(&row[0], (unsigned long long)cnt);
#pragma unroll
  for (int a = 0; a < 3; ++a) atomicAdd(&row[1 + a], q[a]);
  if (RGB) {
#pragma unroll
    for (int a = 0; a < 3; ++a) atomicAdd(&row[4 + a], (unsigned long long)c[a]);
  }
}

// The LDS entry of a key: found or claimed (*mine: by this lane).  -1 only when the table is full, which the flush threshold
// rules out; the caller then sends the point to HBM directly.
__device__ __forceinline__ int lds_grid_slot(unsigned long long* s_key, uint64_t key, bool* mine_out) {
  uint32_t slot = (((uint32_t)key * 0x9E3779B1u) ^ ((uint32_t)(key >> 32) * 0x85EBCA77u)) >> (32 - kGridLdsLog2);
  int found = -1;
  bool mine = false;
  if (s_key[slot] == key) found = (int)slot;   // most points of a surface land in a voxel their neighbours already put there
  for (int probe = 0; probe < kGridLds && found < 0; ++probe) {
    const unsigned long long old = atomicCAS(&s_key[slot], (unsigned long long)kEmpty, (unsigned long long)key);
    if (old == kEmpty) {
      mine = true;
      found = (int)slot;
    } else if (old == key) {
      found = (int)slot;
    } else {
      slot = (slot + 1) & (kGridLds - 1);
    }
  }
  *mine_out = mine;
  return found;
}

template <bool RGB>
__global__ __launch_bounds__(kThreads) void grid_insert_kernel(const float* __restrict__ xyz, const uint32_t* __restrict__ rgba,
                                                               int64_t n, double factor, uint64_t* __restrict__ table,
                                                               unsigned long long* __restrict__ acc, int log2cap,
                                                               unsigned long long* __restrict__ counters) {
  __shared__ unsigned long long s_key[kGridLds];
  __shared__ unsigned long long s_q[3][kGridLds];
  __shared__ unsigned s_cnt[kGridLds];
  __shared__ unsigned s_col[RGB ? 3 : 1][RGB ? kGridLds : 1];
  // keys gained per tile, three counters in rotation (as in voxel_insert_kernel): tile j adds into [j % 3], everyone reads it
  // after the next barrier, thread 0 zeroes [(j + 1) % 3] there, so the running total is the same in every thread and the
  // decision to flush is workgroup-uniform
  __shared__ unsigned s_fill[3];
  const uint64_t mask = ((uint64_t)1 << log2cap) - 1;
  const int lane = threadIdx.x & 63;
  unsigned n_new = 0, n_ignored = 0, n_over = 0;
  const int64_t n_tiles = (n + kTile - 1) / kTile;
  const int64_t per_wg = (n_tiles + gridDim.x - 1) / gridDim.x;
  const int64_t tile_lo = (int64_t)blockIdx.x * per_wg, tile_hi = tile_lo + per_wg < n_tiles ? tile_lo + per_wg : n_tiles;
  for (int k = threadIdx.x; k < kGridLds; k += kThreads) {
    s_key[k] = kEmpty;
    s_cnt[k] = 0;
#pragma unroll
    for (int a = 0; a < 3; ++a) s_q[a][k] = 0;
    if (RGB) {
#pragma unroll
      for (int a = 0; a < 3; ++a) s_col[a][k] = 0;
    }
  }
  if (threadIdx.x < 3) s_fill[threadIdx.x] = 0;
  // every entry of the LDS table into HBM, the table emptied (its free entries always hold zero sums): all lanes at once
  auto flush = [&]() {
#pragma unroll
    for (int k = 0; k < kGridLds / kThreads; ++k) {
      const int s = k * kThreads + threadIdx.x;
      const uint64_t key = s_key[s];
      if (key != kEmpty) {
        unsigned long long q[3];
        unsigned c[3] = {0, 0, 0};
        const unsigned cnt = s_cnt[s];
        s_key[s] = kEmpty;
        s_cnt[s] = 0;
#pragma unroll
        for (int a = 0; a < 3; ++a) {
          q[a] = s_q[a][s];
          s_q[a][s] = 0;
        }
        if (RGB) {
#pragma unroll
          for (int a = 0; a < 3; ++a) {
            c[a] = s_col[a][s];
            s_col[a][s] = 0;
          }
        }
        grid_add_global<RGB>(table, acc, mask, log2cap, key, cnt, q, c, n_new, n_over);
      }
    }
  };
  unsigned total = 0, j = 0;  // keys in the LDS table (same value in every thread), tiles done by this workgroup
  // the next tile's points are in flight while this tile's are folded in (clamped addresses: unconditional loads)
  P3 pn[kPerThread];
  uint32_t cn[kPerThread];
  if (tile_lo < tile_hi) {
#pragma unroll
    for (int r = 0; r < kPerThread; ++r) {
      int64_t i = tile_lo * kTile + threadIdx.x + (int64_t)r * kThreads;
      i = i < n ? i : n - 1;
      pn[r] = reinterpret_cast<const P3*>(xyz)[i];
      cn[r] = RGB ? rgba[i] : 0u;
    }
  }
  for (int64_t tile = tile_lo; tile < tile_hi; ++tile, ++j) {
    r3d_vox::lds_settle();
    __syncthreads();  // the previous tile's adds and its count are done (first tile: the wipe above has landed)
    if (j > 0) total += s_fill[(j - 1) % 3];
    if (threadIdx.x == 0) s_fill[(j + 1) % 3] = 0;
    if (total >= (unsigned)kGridKeepBelow) {   // workgroup-uniform
      flush();
      total = 0;
    }
    r3d_vox::lds_settle();
    __syncthreads();  // the flush's wipes have landed before this tile claims entries
    const int64_t base = tile * kTile + threadIdx.x;
    P3 p[kPerThread];
    uint32_t c[kPerThread];
#pragma unroll
    for (int r = 0; r < kPerThread; ++r) {
      p[r] = pn[r];
      c[r] = cn[r];
    }
    if (tile + 1 < tile_hi) {
#pragma unroll
      for (int r = 0; r < kPerThread; ++r) {
        int64_t i = base + kTile + (int64_t)r * kThreads;
        i = i < n ? i : n - 1;
        pn[r] = reinterpret_cast<const P3*>(xyz)[i];
        cn[r] = RGB ? rgba[i] : 0u;
      }
    }
    unsigned claimed = 0;
#pragma unroll
    for (int r = 0; r < kPerThread; ++r) {
      if (base + (int64_t)r * kThreads >= n) continue;
      uint64_t key = kEmpty;
      double u[3];
      if (!r3d_vox::voxel_key_u(p[r].x, p[r].y, p[r].z, factor, &key, u)) {
        ++n_ignored;
        continue;
      }
      unsigned long long q[3];
#pragma unroll
      for (int a = 0; a < 3; ++a) q[a] = (unsigned long long)((u[a] - floor(u[a])) * kFracScale);   // f exact, < 2^31
      const unsigned col[3] = {c[r] & 0xffu, (c[r] >> 8) & 0xffu, (c[r] >> 16) & 0xffu};
      bool mine = false;
      const int s = lds_grid_slot(s_key, key, &mine);
      if (s >= 0) {
        claimed += mine ? 1u : 0u;
        atomicAdd(&s_cnt[s], 1u);
#pragma unroll
        for (int a = 0; a < 3; ++a) atomicAdd(&s_q[a][s], q[a]);
        if (RGB) {
#pragma unroll
          for (int a = 0; a < 3; ++a) atomicAdd(&s_col[a][s], col[a]);
        }
      } else {
        grid_add_global<RGB>(table, acc, mask, log2cap, key, 1u, q, col, n_new, n_over);
      }
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) claimed += __shfl_down(claimed, off, 64);
    if (lane == 0 && claimed) atomicAdd(&s_fill[j % 3], claimed);
  }
  r3d_vox::lds_settle();
  __syncthreads();   // every lane's last adds have landed
  flush();
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {   // (not r3d_vox::wave_sum: as a call, it moved an instruction of this kernel)
    n_new += __shfl_down(n_new, off, 64);
    n_ignored += __shfl_down(n_ignored, off, 64);
    n_over += __shfl_down(n_over, off, 64);
  }
  if (lane == 0) {
    if (n_new) atomicAdd(&counters[0], (unsigned long long)n_new);
    if (n_ignored) atomicAdd(&counters[1], (unsigned long long)n_ignored);
    if (n_over) atomicAdd(&counters[2], (unsigned long long)n_over);
  }
}

// One row per code (ascending Morton order): the code's slot found again by probing the key array, the row computed from its
// integer sums.  All outputs NULL: only checks that every count fits 32 bits (counters[4] counts those that do not).
template <bool RGB>
__global__ __launch_bounds__(kThreads) void grid_rows_kernel(const uint64_t* __restrict__ codes, int64_t n,
                                                             const uint64_t* __restrict__ table,
                                                             const unsigned long long* __restrict__ acc, int log2cap,
                                                             double factor, float* __restrict__ xyz_out,
                                                             uint32_t* __restrict__ rgba_out, uint32_t* __restrict__ count_out,
                                                             uint64_t* __restrict__ codes_out,
                                                             unsigned long long* __restrict__ counters) {
  const uint64_t mask = ((uint64_t)1 << log2cap) - 1;
  for (int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x; i < n; i += (int64_t)gridDim.x * kThreads) {
    const uint64_t code = codes[i];
    const uint64_t key = r3d_vox::key_of_morton(code);
    uint64_t slot = r3d_vox::home_slot(key, log2cap);
    for (uint64_t probe = 0; probe < mask && table[slot] != key; ++probe) slot = (slot + 1) & mask;   // it is there: it was listed
    const unsigned long long* row = acc + slot * acc_words<RGB>();
    const unsigned long long cnt = row[0];
    if (cnt > 0xffffffffull) atomicAdd(&counters[4], 1ull);
    if (codes_out) codes_out[i] = code;
    if (count_out) count_out[i] = (uint32_t)cnt;
    if (xyz_out) {
      const double denom = (double)cnt * kFracScale;
      float c[3];
#pragma unroll
      for (int a = 0; a < 3; ++a) {
        const int k = (int)((key >> (16 * a)) & 0xffffu) - r3d_vox::kTreeMaxVal;
        c[a] = (float)(((double)k + (double)row[1 + a] / denom) / factor);
      }
      P3 v;
      v.x = c[0];
      v.y = c[1];
      v.z = c[2];
      reinterpret_cast<P3*>(xyz_out)[i] = v;
    }
    if (RGB && rgba_out) {
      uint32_t w = 0;
#pragma unroll
      for (int a = 0; a < 3; ++a) w |= (uint32_t)((2 * row[4 + a] + cnt) / (2 * cnt)) << (8 * a);
      rgba_out[i] = w;
    }
  }
}

}  // namespace

extern "C" {

int r3d_voxelgrid_create(r3d_ctx* ctx, double resolution, int64_t capacity, int flags, r3d_voxelgrid** vg_out) {
  int rc = r3d_ctx_enter(ctx);
  if (rc) return rc;
  R3D_REQUIRE(vg_out != nullptr, "vg_out is NULL");
  *vg_out = nullptr;
  R3D_REQUIRE(resolution > 0.0 && std::isfinite(resolution), "resolution must be positive");
  R3D_REQUIRE(capacity >= 0, "capacity must be >= 0");
  R3D_REQUIRE((flags & ~R3D_VOXELGRID_RGB) == 0, "unknown voxel grid flags 0x%x", flags);
  r3d_voxelgrid* vg = new (std::nothrow) r3d_voxelgrid();
  if (!vg) {
    r3d_set_error("host allocation failed");
    return R3D_ERR_NOMEM;
  }
  vg->ctx = ctx;
  vg->device = ctx->device;
  vg->res = resolution;
  vg->factor = 1.0 / resolution;  // the voxel set's factor: the same keys
  vg->rgb = (flags & R3D_VOXELGRID_RGB) != 0;
  vg->log2cap = 10;
  while (((int64_t)1 << vg->log2cap) < capacity && vg->log2cap < 40) ++vg->log2cap;
  vg->capacity = (uint64_t)1 << vg->log2cap;
  const size_t acc_bytes = vg->capacity * (vg->rgb ? acc_words<true>() : acc_words<false>()) * sizeof(unsigned long long);
  hipError_t e = hipMalloc((void**)&vg->d_table, vg->capacity * sizeof(uint64_t));
  if (e == hipSuccess) e = hipMalloc((void**)&vg->d_acc, acc_bytes);
  if (e == hipSuccess) e = hipMalloc((void**)&vg->d_counters, 5 * sizeof(unsigned long long));
  if (e != hipSuccess) {
    const unsigned long long slots = vg->capacity;
    r3d_voxelgrid_destroy(vg);
    if (e == hipErrorOutOfMemory) {
      r3d_set_error("voxel grid of %llu slots does not fit the device", slots);
      return R3D_ERR_NOMEM;
    }
    return r3d_fail_hip(e, "voxel grid allocation", __FILE__, __LINE__);
  }
  if ((rc = r3d_voxelgrid_clear(vg))) {
    r3d_voxelgrid_destroy(vg);
    return rc;
  }
  *vg_out = vg;
  return R3D_OK;
}

int r3d_voxelgrid_destroy(r3d_voxelgrid* vg) {
  if (!vg) return R3D_OK;
  (void)hipSetDevice(vg->device);
  (void)hipDeviceSynchronize();
  if (vg->d_table) (void)hipFree(vg->d_table);
  if (vg->d_acc) (void)hipFree(vg->d_acc);
  if (vg->d_counters) (void)hipFree(vg->d_counters);
  delete vg;
  return R3D_OK;
}

int r3d_voxelgrid_clear(r3d_voxelgrid* vg) {
  R3D_REQUIRE(vg != nullptr, "voxel grid is NULL");
  int rc = r3d_ctx_enter(vg->ctx);
  if (rc) return rc;
  const size_t acc_bytes = vg->capacity * (vg->rgb ? acc_words<true>() : acc_words<false>()) * sizeof(unsigned long long);
  R3D_HIP(hipMemsetAsync(vg->d_table, 0xff, vg->capacity * sizeof(uint64_t), vg->ctx->stream));
  R3D_HIP(hipMemsetAsync(vg->d_acc, 0, acc_bytes, vg->ctx->stream));
  R3D_HIP(hipMemsetAsync(vg->d_counters, 0, 5 * sizeof(unsigned long long), vg->ctx->stream));
  vg->points_in = 0;
  return R3D_OK;
}

int r3d_voxelgrid_insert(r3d_voxelgrid* vg, const float* d_xyz, const uint32_t* d_rgba, int64_t n_points) {
  R3D_REQUIRE(vg != nullptr, "voxel grid is NULL");
  int rc = r3d_ctx_enter(vg->ctx);
  if (rc) return rc;
  R3D_REQUIRE(n_points >= 0, "n_points must be >= 0");
  R3D_REQUIRE(!d_rgba || vg->rgb, "colour given to a voxel grid created without R3D_VOXELGRID_RGB");
  R3D_REQUIRE(d_rgba || !vg->rgb, "a voxel grid created with R3D_VOXELGRID_RGB needs a colour word per point");
  if (n_points == 0) return R3D_OK;
  R3D_REQUIRE(d_xyz != nullptr, "NULL device pointer");
  const int64_t n_tiles = (n_points + kTile - 1) / kTile;
  int64_t blocks = (int64_t)vg->ctx->num_cus * 8;
  const int64_t at_least = (n_tiles + kMaxTilesPerWg - 1) / kMaxTilesPerWg;
  if (blocks < at_least) blocks = at_least;
  if (blocks > n_tiles) blocks = n_tiles;
  if (vg->rgb)
    hipLaunchKernelGGL(grid_insert_kernel<true>, dim3((unsigned)blocks), dim3(kThreads), 0, vg->ctx->stream, d_xyz, d_rgba,
                       n_points, vg->factor, vg->d_table, vg->d_acc, vg->log2cap, vg->d_counters);
  else
    hipLaunchKernelGGL(grid_insert_kernel<false>, dim3((unsigned)blocks), dim3(kThreads), 0, vg->ctx->stream, d_xyz, nullptr,
                       n_points, vg->factor, vg->d_table, vg->d_acc, vg->log2cap, vg->d_counters);
  R3D_HIP(hipGetLastError());
  vg->points_in += (uint64_t)n_points;
  return R3D_OK;
}

int r3d_voxelgrid_insert_host(r3d_voxelgrid* vg, const float* h_xyz, const uint32_t* h_rgba, int64_t n_points) {
  R3D_REQUIRE(vg != nullptr, "voxel grid is NULL");
  int rc = r3d_ctx_enter(vg->ctx);
  if (rc) return rc;
  R3D_REQUIRE(n_points >= 0, "n_points must be >= 0");
  R3D_REQUIRE(!h_rgba || vg->rgb, "colour given to a voxel grid created without R3D_VOXELGRID_RGB");
  R3D_REQUIRE(h_rgba || !vg->rgb, "a voxel grid created with R3D_VOXELGRID_RGB needs a colour word per point");
  if (n_points == 0) return R3D_OK;
  R3D_REQUIRE(h_xyz != nullptr, "NULL host pointer");
  void *d = nullptr, *d_c = nullptr;
  if ((rc = r3d_scratch(vg->ctx, kWsIn, (size_t)n_points * 12, &d))) return rc;
  R3D_HIP(hipMemcpyAsync(d, h_xyz, (size_t)n_points * 12, hipMemcpyHostToDevice, vg->ctx->stream));
  if (h_rgba) {
    if ((rc = r3d_scratch(vg->ctx, kWsPartials, (size_t)n_points * 4, &d_c))) return rc;
    R3D_HIP(hipMemcpyAsync(d_c, h_rgba, (size_t)n_points * 4, hipMemcpyHostToDevice, vg->ctx->stream));
  }
  if ((rc = r3d_voxelgrid_insert(vg, static_cast<const float*>(d), static_cast<const uint32_t*>(d_c), n_points))) return rc;
  R3D_HIP(hipStreamSynchronize(vg->ctx->stream));
  return R3D_OK;
}

int r3d_voxelgrid_stats(r3d_voxelgrid* vg, int64_t* n_voxels, int64_t* n_ignored, int64_t* n_overflow) {
  R3D_REQUIRE(vg != nullptr, "voxel grid is NULL");
  int rc = r3d_ctx_enter(vg->ctx);
  if (rc) return rc;
  unsigned long long c[3];
  R3D_HIP(hipMemcpyAsync(c, vg->d_counters, sizeof(c), hipMemcpyDeviceToHost, vg->ctx->stream));
  R3D_HIP(hipStreamSynchronize(vg->ctx->stream));
  if (n_voxels) *n_voxels = (int64_t)c[0];
  if (n_ignored) *n_ignored = (int64_t)c[1];
  if (n_overflow) *n_overflow = (int64_t)c[2];
  return R3D_OK;
}

int r3d_voxelgrid_extract(r3d_voxelgrid* vg, float* d_xyz_out, uint32_t* d_rgba_out, uint32_t* d_count_out,
                          uint64_t* d_codes_out, int64_t cap, int64_t* n_out) {
  R3D_REQUIRE(vg != nullptr && n_out != nullptr, "NULL argument");
  R3D_REQUIRE(!d_rgba_out || vg->rgb, "colour asked of a voxel grid created without R3D_VOXELGRID_RGB");
  int64_t n = 0, ign = 0, over = 0;
  int rc = r3d_voxelgrid_stats(vg, &n, &ign, &over);
  if (rc) return rc;
  *n_out = n;
  if (over > 0) {
    r3d_set_error("voxel grid overflowed (%lld points found no slot): create it with a larger capacity", (long long)over);
    return R3D_ERR_NOMEM;
  }
  if (!d_xyz_out && !d_rgba_out && !d_count_out && !d_codes_out) return R3D_OK;   // count only
  R3D_REQUIRE(cap >= n, "buffers hold %lld rows, the grid has %lld voxels", (long long)cap, (long long)n);
  const void* out[4] = {d_xyz_out, d_rgba_out, d_count_out, d_codes_out};
  const size_t bytes[4] = {(size_t)n * 12, (size_t)n * 4, (size_t)n * 4, (size_t)n * 8};
  for (int a = 0; a < 4; ++a)
    for (int b = a + 1; b < 4; ++b) R3D_REQUIRE(!r3d_ranges_overlap(out[a], bytes[a], out[b], bytes[b]), "output ranges overlap");
  if (n == 0) return R3D_OK;
  uint64_t* d_codes = nullptr;
  if ((rc = r3d_voxel_table_sorted_codes(vg->ctx, vg->d_table, vg->capacity, vg->d_counters, n, &d_codes))) return rc;
  int64_t blocks = (n + kThreads - 1) / kThreads;
  if (blocks > (int64_t)vg->ctx->num_cus * 16) blocks = (int64_t)vg->ctx->num_cus * 16;
  auto rows = [&](float* xyz, uint32_t* rgba, uint32_t* cnt, uint64_t* codes) {
    if (vg->rgb)
      hipLaunchKernelGGL(grid_rows_kernel<true>, dim3((unsigned)blocks), dim3(kThreads), 0, vg->ctx->stream, d_codes, n,
                         vg->d_table, vg->d_acc, vg->log2cap, vg->factor, xyz, rgba, cnt, codes, vg->d_counters);
    else
      hipLaunchKernelGGL(grid_rows_kernel<false>, dim3((unsigned)blocks), dim3(kThreads), 0, vg->ctx->stream, d_codes, n,
                         vg->d_table, vg->d_acc, vg->log2cap, vg->factor, xyz, nullptr, cnt, codes, vg->d_counters);
    return hipGetLastError();
  };
  if (vg->points_in > 0xffffffffull) {   // only then can a voxel hold too many points: check before anything is written
    unsigned long long too_big = 0;
    R3D_HIP(hipMemsetAsync(vg->d_counters + 4, 0, sizeof(unsigned long long), vg->ctx->stream));
    R3D_HIP(rows(nullptr, nullptr, nullptr, nullptr));
    R3D_HIP(hipMemcpyAsync(&too_big, vg->d_counters + 4, sizeof(too_big), hipMemcpyDeviceToHost, vg->ctx->stream));
    R3D_HIP(hipStreamSynchronize(vg->ctx->stream));
    R3D_REQUIRE(too_big == 0, "%llu voxels hold more than 2^32 - 1 points: their counts do not fit the uint32 output",
                too_big);
  }
  R3D_HIP(rows(d_xyz_out, d_rgba_out, d_count_out, d_codes_out));
  for (int a = 0; a < 4; ++a) r3d_wrote(vg->ctx, out[a], out[a] ? bytes[a] : 0);
  R3D_HIP(hipStreamSynchronize(vg->ctx->stream));
  return R3D_OK;
}

}  // extern "C"
