// Occupied-voxel set of a world cloud on gfx950 (MI355X) + OctoMap binary (.bt) export.
//
// Replaces the per-point `tree.updateNode(xyz, True)` loop, `updateInnerOccupancy()` and
// `writeBinary()` of octomap/txt_transfer_octomap.py:16-36 (== octomap/ply_transfer_octomap.py:16-48).
// The arithmetic of that path lives in the third-party OctoMap library (not vendored, not pinned by the
// reference): restated from its published semantics; parity unpinned.
//
// A hits-only tree written with writeBinary() depends only on the SET of voxels that received a point
// (toMaxLikelihood makes every hit leaf "occupied"), so the GPU's job is a set insert:
//   * voxel_insert_kernel (12 B/point read): lane-per-point 12-byte loads, key per axis
//     = (int)floor((1/res) * (double)x) + 32768 in fp64 like OcTreeBaseImpl::coordToKey, the three 16-bit keys
//     packed into one word, lanes whose predecessor lane holds the same word drop out, the rest go into an
//     open-addressing hash set in HBM (64-bit atomicCAS, multiplicative hash, linear probing).
//   * voxel_compact_kernel: table -> dense list of 48-bit Morton codes (x lowest, as OctoMap's child index): the
//     interleave is paid per distinct voxel here, not per point in the insert (r3d_voxel_dev.h).
// The distinct codes are radix-sorted on the GPU (r3d_sort.hip) and serialised as a pruned octree: on the device by
// r3d_octree.hip, on the host by r3d_octree_host.cpp.
// This file: the set object and its C ABI, the LDS-set + CAS insert (path 1), the sample that chooses between the two insert
// paths, insert-codes, compact, union, codes and stats.  Path 2, the sort-merge insert, is r3d_voxel_merge.hip.
#include <algorithm>
#include <cmath>
#include <vector>

#include "r3d_internal.h"
#include "r3d_voxel_dev.h"

namespace {

constexpr int kThreads = 256;
using r3d_vox::kEmpty;
using r3d_vox::kLdsKeepBelow;
using r3d_vox::kLdsSlots;
using r3d_vox::lds_set_claim;
using r3d_vox::P3;
using r3d_vox::prev_lane_u64;
using r3d_vox::table_insert;
using r3d_vox::wave_sum;

// DEDUPE: a workgroup funnels its codes through a small LDS hash set and walks a CONTIGUOUS run of tiles (neighbouring
// image rows fall into the SAME voxels), keeping the set from tile to tile.  Round 2 sent every newly claimed code to the
// global table on the spot: a handful of returning global atomics per tile, each a ~2 us round trip that the whole wave sat
// out (PMC: waves waiting 85 % of their cycles, 109 VALU instructions per 64 points; in-kernel clocks: 46 % in those atomics).
// Round 3: while it walks its tiles a workgroup touches LDS only -- a claimed code simply STAYS in the set -- and the set is
// flushed to the global table as a whole, all 256 lanes inserting in parallel, when it has collected kLdsKeepBelow codes and
// at the end of the run: the round trips are paid once per ~512 codes instead of once per tile.  A code that finds the set full
// (cannot happen below 75 % load) goes to the global table directly.
template <bool DEDUPE, bool COND_BARRIER = false>
__global__ __launch_bounds__(kThreads) void voxel_insert_kernel(const float* __restrict__ xyz, int64_t n, double factor,
                                                                uint64_t* __restrict__ table, int log2cap,
                                                                unsigned long long* __restrict__ counters) {
  __shared__ unsigned long long local_set[DEDUPE ? kLdsSlots : 1];
  // codes gained per tile, three counters in rotation: tile j adds into [j % 3], everyone reads it after the next barrier,
  // thread 0 zeroes [(j + 1) % 3] there -- whose last readers all passed that barrier -- so the running total every thread
  // keeps in a register is the same in all of them and the decision to flush is workgroup-uniform
  __shared__ unsigned local_fill[3];
  const uint64_t mask = ((uint64_t)1 << log2cap) - 1;
  const int lane = threadIdx.x & 63;
  // statistics stay in registers and reach the three global counters once per wave: a per-insert atomicAdd on one word would
  // cap the kernel at that word's ~0.09 G atomics/s.  (Once per WORKGROUP -- flush_counts, r3d_voxel_dev.h -- was tried in round
  // 4 after the merge kernel's lesson: here the 8192 adds trickle in over milliseconds and never queue, and the extra
  // barriers + LDS hop changed the main loop's code generation: 216-222 -> 182 Gpoints/s on scans, 3.26 -> 3.65 ms on the worst
  // case.  Reverted.)
  unsigned n_new = 0, n_ignored = 0, n_over = 0;
  const int64_t n_tiles = (n + kThreads * 4 - 1) / (kThreads * 4);
  const int64_t per_wg = (n_tiles + gridDim.x - 1) / gridDim.x;  // a contiguous run of tiles per workgroup
  const int64_t tile_lo = (int64_t)blockIdx.x * per_wg, tile_hi = tile_lo + per_wg < n_tiles ? tile_lo + per_wg : n_tiles;
  if (DEDUPE) {
    for (int k = threadIdx.x; k < kLdsSlots; k += kThreads) local_set[k] = kEmpty;
    if (threadIdx.x < 3) local_fill[threadIdx.x] = 0;
  }
  // every code of the set into the global table, the set emptied: all lanes at once, kLdsSlots / kThreads slots each
  auto flush = [&]() {
#pragma unroll
    for (int k = 0; k < kLdsSlots / kThreads; ++k) {
      const int s = k * kThreads + threadIdx.x;
      const uint64_t code = local_set[s];
      if (code != kEmpty) {
        local_set[s] = kEmpty;
        const int r = table_insert(table, mask, log2cap, code);
        n_new += r > 0 ? 1u : 0u;
        n_over += r < 0 ? 1u : 0u;
      }
    }
  };
  unsigned total = 0, j = 0;  // codes in the set (same value in every thread), tiles done by this workgroup
  // the next tile's points, in flight.  (Round 5: as nontemporal loads -- a 3-float vector type of 4-byte alignment, so that the
  // compiler still tracks them -- 223 vs 223 and 231 vs 214 Gpoints/s on scans, same process: within the noise, not kept.  Inline-asm
  // loads whose wait is a second asm statement further down are not an option at all: the compiler copies and re-uses their
  // destination registers in between, and a load that lands in what has become an address register is a memory fault.)
  P3 pn[4];
  if (tile_lo < tile_hi) {
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int64_t i = tile_lo * (kThreads * 4) + threadIdx.x + (int64_t)r * kThreads;
      pn[r] = reinterpret_cast<const P3*>(xyz)[i < n ? i : n - 1];
    }
  }
  for (int64_t tile = tile_lo; tile < tile_hi; ++tile, ++j) {
    if (DEDUPE) {
      r3d_vox::lds_settle();
      __syncthreads();  // the previous tile's lookups and its count are done (first tile: the wipe above has landed)
      if (j > 0) total += local_fill[(j - 1) % 3];
      if (threadIdx.x == 0) local_fill[(j + 1) % 3] = 0;
      if (COND_BARRIER) {
        if (total >= (unsigned)kLdsKeepBelow) {  // workgroup-uniform
          flush();
          total = 0;
          __syncthreads();
        }
      } else {
        if (total >= (unsigned)kLdsKeepBelow) {
          flush();
          total = 0;
        }
        r3d_vox::lds_settle();
        __syncthreads();
      }
    }
    const int64_t base = tile * (kThreads * 4) + threadIdx.x;
    // the NEXT tile's points are requested before this tile's are worked on (clamped addresses: unconditional loads), so
    // that the HBM round trip of tile k+1 runs under the key arithmetic and the LDS lookups of tile k
    P3 p[4];
#pragma unroll
    for (int r = 0; r < 4; ++r) p[r] = pn[r];
    if (tile + 1 < tile_hi) {
      const int64_t nbase = base + kThreads * 4;
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int64_t i = nbase + (int64_t)r * kThreads;
        pn[r] = reinterpret_cast<const P3*>(xyz)[i < n ? i : n - 1];
      }
    }
    unsigned claimed = 0;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int64_t i = base + (int64_t)r * kThreads;
      uint64_t code = kEmpty;
      bool live = i < n;
      if (live && !r3d_vox::voxel_key(p[r].x, p[r].y, p[r].z, factor, &code)) {
        ++n_ignored;
        live = false;
        code = kEmpty;
      }
      // neighbouring pixels mostly fall into the same voxel: a lane whose predecessor carries the same
      // code leaves the insert to it
      const uint64_t prev = prev_lane_u64(code);
      if (live && lane > 0 && prev == code) live = false;
      if (DEDUPE && live) {
        bool mine = false;
        const bool done = lds_set_claim(local_set, code, &mine);
        claimed += mine ? 1u : 0u;
        live = !done;  // a full set (cannot happen: < 512 + 1024 codes in 2048 slots) sends the code on directly
      }
      if (live) {
        const int r2 = table_insert(table, mask, log2cap, code);
        n_new += r2 > 0 ? 1u : 0u;
        n_over += r2 < 0 ? 1u : 0u;
      }
    }
    if (DEDUPE) {  // one LDS add per wave: how many codes the set gained in this tile
#pragma unroll
      for (int off = 32; off > 0; off >>= 1) claimed += __shfl_down(claimed, off, 64);
      if (lane == 0 && claimed) atomicAdd(&local_fill[j % 3], claimed);
    }
  }
  if (DEDUPE) {
    __syncthreads();   // every lane's last lookups have landed
    flush();
  }
  const auto [w_new, w_ignored, w_over] = wave_sum(n_new, n_ignored, n_over);
  if (lane == 0) {
    if (w_new) atomicAdd(&counters[0], (unsigned long long)w_new);
    if (w_ignored) atomicAdd(&counters[1], (unsigned long long)w_ignored);
    if (w_over) atomicAdd(&counters[2], (unsigned long long)w_over);
  }
}

// How alike are neighbouring points?  Each sampling workgroup takes 4 consecutive tiles (4096 points: a few image rows) and
// counts the distinct voxels among them in an LDS set; sums[0] += points that have a key, sums[1] += distinct keys.
constexpr int kSampleSlots = 8192;
__global__ __launch_bounds__(kThreads) void voxel_sample_kernel(const float* __restrict__ xyz, int64_t n, double factor, int64_t stride_tiles,
                                                                unsigned long long* __restrict__ sums) {
  __shared__ unsigned long long set[kSampleSlots];
  for (int k = threadIdx.x; k < kSampleSlots; k += kThreads) set[k] = kEmpty;
  __syncthreads();
  const int64_t first = (int64_t)blockIdx.x * stride_tiles * (kThreads * 4);
  unsigned valid = 0, distinct = 0;
  for (int r = 0; r < 16; ++r) {
    const int64_t i = first + (int64_t)r * kThreads + threadIdx.x;
    if (i >= n) break;   // (every thread still reaches the barriers of flush_counts below)
    const P3 p = reinterpret_cast<const P3*>(xyz)[i];
    uint64_t key;
    if (!r3d_vox::voxel_key(p.x, p.y, p.z, factor, &key)) continue;
    ++valid;
    uint32_t s = (((uint32_t)key * 0x9E3779B1u) ^ ((uint32_t)(key >> 32) * 0x85EBCA77u)) >> 19;   // 13 bits
    for (int probe = 0; probe < kSampleSlots; ++probe) {   // <= 4096 keys in 8192 slots: always ends
      const unsigned long long old = atomicCAS(&set[s], (unsigned long long)kEmpty, (unsigned long long)key);
      if (old == kEmpty) {
        ++distinct;
        break;
      }
      if (old == key) break;
      s = (s + 1) & (kSampleSlots - 1);
    }
  }
  __shared__ unsigned wg_counts[3];
  r3d_vox::flush_counts(valid, distinct, 0u, wg_counts, sums);   // sums[0] += valid, sums[1] += distinct: one add per workgroup
}

// Insert ready-made 48-bit Morton codes (another rank's occupied voxels: the union step of a sharded map).
__global__ __launch_bounds__(kThreads) void voxel_insert_codes_kernel(const uint64_t* __restrict__ codes, int64_t n,
                                                                      uint64_t* __restrict__ table, int log2cap,
                                                                      unsigned long long* __restrict__ counters) {
  const uint64_t mask = ((uint64_t)1 << log2cap) - 1;
  const int lane = threadIdx.x & 63;
  unsigned n_new = 0, n_ignored = 0, n_over = 0;
  for (int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x; i < n + lane; i += (int64_t)gridDim.x * kThreads) {
    // (the loop bound keeps whole waves together for the shuffle below)
    uint64_t code = i < n ? codes[i] : kEmpty;
    bool live = i < n;
    if (live && (code >> 48) != 0) {  // not a depth-16 octree key
      ++n_ignored;
      live = false;
      code = kEmpty;
    }
    const uint64_t prev = __shfl_up(code, 1, 64);
    if (live && lane > 0 && prev == code) live = false;  // sorted inputs repeat a code in neighbouring lanes
    if (live) {
      code = r3d_vox::key_of_morton(code);  // the table holds packed keys (r3d_voxel_dev.h)
      uint64_t slot = r3d_vox::home_slot(code, log2cap);
      bool done = false;
      for (uint64_t probe = 0; probe <= mask && !done; ++probe) {
        const uint64_t old = atomicCAS(reinterpret_cast<unsigned long long*>(&table[slot]), (unsigned long long)kEmpty,
                                       (unsigned long long)code);
        if (old == kEmpty) {
          ++n_new;
          done = true;
        } else if (old == code) {
          done = true;
        } else {
          slot = (slot + 1) & mask;
        }
      }
      if (!done) ++n_over;
    }
  }
  const auto [w_new, w_ignored, w_over] = wave_sum(n_new, n_ignored, n_over);
  if (lane == 0) {
    if (w_new) atomicAdd(&counters[0], (unsigned long long)w_new);
    if (w_ignored) atomicAdd(&counters[1], (unsigned long long)w_ignored);
    if (w_over) atomicAdd(&counters[2], (unsigned long long)w_over);
  }
}

// table (packed keys) -> dense list of Morton codes (order irrelevant: the radix sort follows).  One cursor bump per WORKGROUP-STEP of
// kCompactSlots table words held in registers (round 2 bumped the one global cursor once per wave per 64 words: ~2 M
// same-address returning atomics for a 1 GB table = 25 ms = 0.8 % of HBM; a same-address returning atomic completes at
// ~0.09 G/s, so the count per bump decides everything).  Steps that hold no code skip the atomic.
constexpr int kCompactPerThread = 32;                            // table words per thread per step: 16 x 16-byte loads
constexpr int kCompactSlots = kThreads * kCompactPerThread;      // 8192 words = 64 KB per workgroup-step

__global__ __launch_bounds__(kThreads) void voxel_compact_kernel(const uint64_t* __restrict__ table, uint64_t capacity,
                                                                 uint64_t* __restrict__ out,
                                                                 unsigned long long* __restrict__ counters) {
  __shared__ unsigned wave_total[kThreads / 64];
  __shared__ unsigned long long step_base;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const uint64_t n_steps = (capacity + kCompactSlots - 1) / kCompactSlots;
  for (uint64_t step = blockIdx.x; step < n_steps; step += gridDim.x) {   // workgroup-uniform trip count
    // thread t holds words (2t, 2t+1) + k * 512 of the step: every wave instruction reads 1 KB contiguous
    const uint64_t lo = step * kCompactSlots + 2 * (uint64_t)threadIdx.x;
    uint64_t v[kCompactPerThread];
#pragma unroll
    for (int k = 0; k < kCompactPerThread / 2; ++k) {
      const uint64_t i = lo + (uint64_t)k * (2 * kThreads);
      if (i + 1 < capacity) {   // capacity is a power of two >= 1024: pairs never straddle the end
        const ulonglong2 w = *reinterpret_cast<const ulonglong2*>(table + i);
        v[2 * k] = w.x;
        v[2 * k + 1] = w.y;
      } else {
        v[2 * k] = kEmpty;
        v[2 * k + 1] = kEmpty;
      }
    }
    // per word slot k the wave's hits leave as ONE contiguous run (ballot-ranked): the counts are wave-uniform scalars
    unsigned wave_cnt = 0;
#pragma unroll
    for (int k = 0; k < kCompactPerThread; ++k) wave_cnt += (unsigned)__popcll(__ballot(v[k] != kEmpty));
    if (lane == 0) wave_total[wave] = wave_cnt;
    __syncthreads();
    unsigned before = 0, total = 0;
#pragma unroll
    for (int w = 0; w < kThreads / 64; ++w) {
      const unsigned t = wave_total[w];
      if (w < wave) before += t;
      total += t;
    }
    if (threadIdx.x == 0 && total) step_base = atomicAdd(&counters[3], (unsigned long long)total);
    __syncthreads();
    if (total) {
      unsigned long long at = step_base + before;
      const unsigned long long below = (1ull << lane) - 1;
#pragma unroll
      for (int k = 0; k < kCompactPerThread; ++k) {
        const bool hit = v[k] != kEmpty;
        const unsigned long long ballot = __ballot(hit);
        if (hit) out[at + __popcll(ballot & below)] = r3d_vox::morton_of_key(v[k]);  // packed key -> Morton code on the way out
        at += __popcll(ballot);
      }
    }
    // (the next step's first barrier separates this step's reads of wave_total / step_base from their next writes)
  }
}

}  // namespace

int r3d_voxelset_device_view(r3d_voxelset* vs, r3d_ctx** ctx, double* factor, uint64_t** d_table, int* log2cap,
                             unsigned long long** d_counters) {
  R3D_REQUIRE(vs != nullptr, "voxel set is NULL");
  *ctx = vs->ctx;
  *factor = vs->factor;
  *d_table = vs->d_table;
  *log2cap = vs->log2cap;
  *d_counters = vs->d_counters;
  vs->pristine = false;   // whoever asks for the table is about to write it
  return R3D_OK;
}


extern "C" {

int r3d_voxelset_create(r3d_ctx* ctx, double resolution, int64_t capacity, r3d_voxelset** vs_out) {
  int rc = r3d_ctx_enter(ctx);
  if (rc) return rc;
  R3D_REQUIRE(vs_out != nullptr, "vs_out is NULL");
  *vs_out = nullptr;
  R3D_REQUIRE(resolution > 0.0 && std::isfinite(resolution), "resolution must be positive");
  R3D_REQUIRE(capacity >= 0, "capacity must be >= 0");
  r3d_voxelset* vs = new (std::nothrow) r3d_voxelset();
  if (!vs) {
    r3d_set_error("host allocation failed");
    return R3D_ERR_NOMEM;
  }
  vs->ctx = ctx;
  vs->device = ctx->device;
  vs->res = resolution;
  vs->factor = 1.0 / resolution;  // OcTreeBaseImpl::resolution_factor
  vs->log2cap = 10;
  while (((int64_t)1 << vs->log2cap) < capacity && vs->log2cap < 40) ++vs->log2cap;
  vs->capacity = (uint64_t)1 << vs->log2cap;
  hipError_t e = hipMalloc((void**)&vs->d_table, vs->capacity * sizeof(uint64_t));
  if (e == hipSuccess) e = hipMalloc((void**)&vs->d_counters, 4 * sizeof(unsigned long long));
  if (e == hipSuccess) e = hipMemsetAsync(vs->d_table, 0xff, vs->capacity * sizeof(uint64_t), ctx->stream);
  if (e == hipSuccess) e = hipMemsetAsync(vs->d_counters, 0, 4 * sizeof(unsigned long long), ctx->stream);
  if (e != hipSuccess) {
    r3d_voxelset_destroy(vs);
    return r3d_fail_hip(e, "voxel set allocation", __FILE__, __LINE__);
  }
  *vs_out = vs;
  return R3D_OK;
}

int r3d_voxelset_destroy(r3d_voxelset* vs) {
  if (!vs) return R3D_OK;
  (void)hipSetDevice(vs->device);
  (void)hipDeviceSynchronize();
  if (vs->d_table) (void)hipFree(vs->d_table);
  if (vs->d_counters) (void)hipFree(vs->d_counters);
  delete vs;
  return R3D_OK;
}

int r3d_voxelset_clear(r3d_voxelset* vs) {
  R3D_REQUIRE(vs != nullptr, "voxel set is NULL");
  int rc = r3d_ctx_enter(vs->ctx);
  if (rc) return rc;
  R3D_HIP(hipMemsetAsync(vs->d_table, 0xff, vs->capacity * sizeof(uint64_t), vs->ctx->stream));
  R3D_HIP(hipMemsetAsync(vs->d_counters, 0, 4 * sizeof(unsigned long long), vs->ctx->stream));
  vs->pristine = true;
  return R3D_OK;
}

int r3d_voxelset_insert(r3d_voxelset* vs, const float* d_xyz, int64_t n_points) {
  R3D_REQUIRE(vs != nullptr, "voxel set is NULL");
  int rc = r3d_ctx_enter(vs->ctx);
  if (rc) return rc;
  R3D_REQUIRE(n_points >= 0, "n_points must be >= 0");
  if (n_points == 0) return R3D_OK;
  R3D_REQUIRE(d_xyz != nullptr, "NULL device pointer");
  // big inserts: a sample of the cloud decides between the two paths ("voxel_path": 1 / 2 force one)
  int path = 1;
  if (vs->ctx->voxel_path == 2 && r3d_voxelset_sort_feasible(vs, n_points, true)) {
    path = 2;
  } else if (vs->ctx->voxel_path == 0 && r3d_voxelset_sort_feasible(vs, n_points, false)) {
    bool sort = false;
    if ((rc = r3d_voxelset_sample(vs, d_xyz, n_points, n_points, 4.5, &sort))) return rc;
    path = sort ? 2 : 1;
  }
  return r3d_voxelset_insert_path(vs, d_xyz, n_points, path);
}

}  // extern "C"

// *sort_out = by the sample, the sort-merge insert of `n_insert` points into this set's table will be the faster one.  The sample
// gives r = distinct voxels per point among neighbours (256 groups of 4096 consecutive points); the two paths' costs on this chip,
// from tools/voxel_path_crossover.py and the stage profiles (round 5):
//   sort-merge   7.5 ps per point (both passes) + 2 ps per table slot (the merge streams the whole table) + 40 us of launches;
//   LDS set + CAS   (4.5 + 62 r) ps per point -- 66 ps for a voxel per point (3.26 ms for C2), 6.7 ps at 28 points per voxel;
//   `cas_base_ps`: the 4.5 (r3d_fuse_frames_voxel's one-launch kernel does not read the cloud back: 1.5).
// Rounds 2-5 asked for >= 1 distinct voxel per 2 points, which left clouds of 2.7 / 5 / 10 points per voxel with the CAS path
// at 1.55 / 0.97 / 0.62 ms where the sort-merge path takes 0.52 / 0.50 / 0.49.  Synchronises the stream (16 bytes come back).
int r3d_voxelset_sample(r3d_voxelset* vs, const float* d_xyz, int64_t n_points, int64_t n_insert, double cas_base_ps, bool* sort_out) {
  *sort_out = false;
  r3d_ctx* ctx = vs->ctx;
  const int64_t n_tiles = (n_points + kThreads * 4 - 1) / (kThreads * 4);
  const int64_t samples = std::max<int64_t>(1, std::min<int64_t>(256, n_tiles / 4));
  void* ws = nullptr;
  int rc = r3d_scratch(ctx, kWsMisc, 64, &ws);
  if (rc) return rc;
  unsigned long long* d_sums = static_cast<unsigned long long*>(ws);
  R3D_HIP(hipMemsetAsync(d_sums, 0, 16, ctx->stream));
  hipLaunchKernelGGL(voxel_sample_kernel, dim3((unsigned)samples), dim3(kThreads), 0, ctx->stream, d_xyz, n_points, vs->factor,
                     n_tiles / samples, d_sums);
  R3D_HIP(hipGetLastError());
  unsigned long long h[2] = {0, 0};
  R3D_HIP(hipMemcpyAsync(h, d_sums, sizeof(h), hipMemcpyDeviceToHost, ctx->stream));
  R3D_HIP(hipStreamSynchronize(ctx->stream));
  if (h[0] > 0) {
    const double r = (double)h[1] / (double)h[0];
    const double us_sort = (double)n_insert * 7.5e-6 + (double)vs->capacity * 2.0e-6 + 40.0;
    const double us_cas = (double)n_insert * (cas_base_ps + 62.0 * r) * 1e-6;
    *sort_out = us_sort < us_cas;
  }
  return R3D_OK;
}

// path 1: the LDS-set + CAS kernel; path 2: sort-merge, r3d_voxel_merge.hip (the caller has checked r3d_voxelset_sort_feasible)
int r3d_voxelset_insert_path(r3d_voxelset* vs, const float* d_xyz, int64_t n_points, int path) {
  if (n_points <= 0) return R3D_OK;
  vs->ctx->voxel_last_path = path;
  if (path == 2) return r3d_voxelset_insert_sorted(vs, d_xyz, n_points);
  vs->pristine = false;
  const int64_t n_tiles = (n_points + kThreads * 4 - 1) / (kThreads * 4);
  int blocks = vs->ctx->num_cus * 8;
  if ((int64_t)blocks > n_tiles) blocks = (int)n_tiles;
  if (vs->ctx->voxel_dedupe == 3)
    hipLaunchKernelGGL((voxel_insert_kernel<true, true>), dim3(blocks), dim3(kThreads), 0, vs->ctx->stream, d_xyz, n_points,
                       vs->factor, vs->d_table, vs->log2cap, vs->d_counters);
  else if (vs->ctx->voxel_dedupe != 1)  // 0 auto / 2 on: LDS dedupe; 1: off
    hipLaunchKernelGGL(voxel_insert_kernel<true>, dim3(blocks), dim3(kThreads), 0, vs->ctx->stream, d_xyz, n_points,
                       vs->factor, vs->d_table, vs->log2cap, vs->d_counters);
  else
    hipLaunchKernelGGL(voxel_insert_kernel<false>, dim3(blocks), dim3(kThreads), 0, vs->ctx->stream, d_xyz, n_points,
                       vs->factor, vs->d_table, vs->log2cap, vs->d_counters);
  R3D_HIP(hipGetLastError());
  return R3D_OK;
}

extern "C" {

int r3d_voxelset_insert_host(r3d_voxelset* vs, const float* h_xyz, int64_t n_points) {
  R3D_REQUIRE(vs != nullptr, "voxel set is NULL");
  int rc = r3d_ctx_enter(vs->ctx);
  if (rc) return rc;
  R3D_REQUIRE(n_points >= 0, "n_points must be >= 0");
  if (n_points == 0) return R3D_OK;
  R3D_REQUIRE(h_xyz != nullptr, "NULL host pointer");
  void* d = nullptr;
  if ((rc = r3d_scratch(vs->ctx, kWsIn, (size_t)n_points * 12, &d))) return rc;
  R3D_HIP(hipMemcpyAsync(d, h_xyz, (size_t)n_points * 12, hipMemcpyHostToDevice, vs->ctx->stream));
  if ((rc = r3d_voxelset_insert(vs, static_cast<const float*>(d), n_points))) return rc;
  R3D_HIP(hipStreamSynchronize(vs->ctx->stream));
  return R3D_OK;
}

int r3d_voxelset_stats(r3d_voxelset* vs, int64_t* n_voxels, int64_t* n_ignored, int64_t* n_overflow) {
  R3D_REQUIRE(vs != nullptr, "voxel set is NULL");
  int rc = r3d_ctx_enter(vs->ctx);
  if (rc) return rc;
  unsigned long long c[4];
  R3D_HIP(hipMemcpyAsync(c, vs->d_counters, sizeof(c), hipMemcpyDeviceToHost, vs->ctx->stream));
  R3D_HIP(hipStreamSynchronize(vs->ctx->stream));
  if (n_voxels) *n_voxels = (int64_t)c[0];
  if (n_ignored) *n_ignored = (int64_t)c[1];
  if (n_overflow) *n_overflow = (int64_t)c[2];
  return R3D_OK;
}

int r3d_voxelset_insert_codes(r3d_voxelset* vs, const uint64_t* d_codes, int64_t n_codes) {
  R3D_REQUIRE(vs != nullptr, "voxel set is NULL");
  int rc = r3d_ctx_enter(vs->ctx);
  if (rc) return rc;
  R3D_REQUIRE(n_codes >= 0, "n_codes must be >= 0");
  if (n_codes == 0) return R3D_OK;
  R3D_REQUIRE(d_codes != nullptr, "NULL device pointer");
  vs->pristine = false;
  int64_t blocks = (n_codes + kThreads - 1) / kThreads;
  if (blocks > (int64_t)vs->ctx->num_cus * 16) blocks = (int64_t)vs->ctx->num_cus * 16;
  hipLaunchKernelGGL(voxel_insert_codes_kernel, dim3((unsigned)blocks), dim3(kThreads), 0, vs->ctx->stream, d_codes, n_codes,
                     vs->d_table, vs->log2cap, vs->d_counters);
  R3D_HIP(hipGetLastError());
  return R3D_OK;
}

// distinct codes of the set as a sorted list in HBM (kWsOut); *n_out = how many
static int codes_to_device_list(r3d_voxelset* vs, uint64_t** d_list_out, int64_t* n_out) {
  int64_t n = 0, ign = 0, over = 0;
  int rc = r3d_voxelset_stats(vs, &n, &ign, &over);
  if (rc) return rc;
  *n_out = n;
  *d_list_out = nullptr;
  if (over > 0) {
    r3d_set_error("voxel set overflowed (%lld points found no slot): create it with a larger capacity", (long long)over);
    return R3D_ERR_NOMEM;
  }
  if (n == 0) return R3D_OK;
  return r3d_voxel_table_sorted_codes(vs->ctx, vs->d_table, vs->capacity, vs->d_counters, n, d_list_out);
}

}  // extern "C"

int r3d_voxelset_sorted_codes_device(r3d_voxelset* vs, r3d_ctx** ctx, double* resolution, uint64_t** d_list_out, int64_t* n_out) {
  R3D_REQUIRE(vs != nullptr, "voxel set is NULL");
  int rc = r3d_ctx_enter(vs->ctx);
  if (rc) return rc;
  *ctx = vs->ctx;
  *resolution = vs->res;
  return codes_to_device_list(vs, d_list_out, n_out);
}

int r3d_voxel_table_sorted_codes(r3d_ctx* ctx, const uint64_t* d_table, uint64_t capacity, unsigned long long* d_counters,
                                 int64_t n, uint64_t** d_list_out) {
  void *d_list = nullptr, *d_tmp = nullptr;
  int rc = r3d_scratch(ctx, kWsOut, (size_t)n * sizeof(uint64_t), &d_list);
  if (rc) return rc;
  if ((rc = r3d_scratch(ctx, kWsSpare, (size_t)n * sizeof(uint64_t), &d_tmp))) return rc;
  R3D_HIP(hipMemsetAsync(d_counters + 3, 0, sizeof(unsigned long long), ctx->stream));
  int blocks = ctx->num_cus * 8;
  const uint64_t need = (capacity + kCompactSlots - 1) / kCompactSlots;
  if ((uint64_t)blocks > need) blocks = (int)need;
  hipLaunchKernelGGL(voxel_compact_kernel, dim3(blocks), dim3(kThreads), 0, ctx->stream, d_table, capacity,
                     static_cast<uint64_t*>(d_list), d_counters);
  R3D_HIP(hipGetLastError());
  if ((rc = r3d_radix_sort_u64(ctx, static_cast<uint64_t*>(d_list), static_cast<uint64_t*>(d_tmp), n, 48))) return rc;
  *d_list_out = static_cast<uint64_t*>(d_list);
  return R3D_OK;
}

extern "C" {

// Config 5 (frames sharded, ONE map): every rank voxelises its own shard of the world cloud into its own HBM hash set --
// 12 B/point never leave the GPU -- then the ranks exchange only their DISTINCT codes (8 B/voxel, unequal shards) and
// each folds the others' into its set.  Afterwards every rank holds the union.
int r3d_voxelset_union(r3d_voxelset* vs, r3d_comm* comm) {
  R3D_REQUIRE(vs != nullptr && comm != nullptr, "NULL argument");
  int rank = 0, world = 1;
  int rc = r3d_comm_info(comm, &rank, &world, nullptr);
  if (rc) return rc;
  // the exchange runs on the communicator's stream, the set's kernels on the set's: one context orders them
  R3D_REQUIRE(r3d_comm_context(comm) == vs->ctx, "create the communicator on the voxel set's context");
  uint64_t* d_mine = nullptr;
  int64_t n_mine = 0;
  const int rc_mine = codes_to_device_list(vs, &d_mine, &n_mine);
  if (world == 1) return rc_mine;
  // how many codes every rank brings: an all-gather of one int64 each.  A rank whose set cannot be listed (overflow)
  // still takes part and says -1, so that EVERY rank returns the error instead of waiting for it forever.
  if (rc_mine) n_mine = -1;
  void* d_cnt = nullptr;
  if ((rc = r3d_scratch(vs->ctx, kWsCounts, (size_t)(world + 1) * sizeof(int64_t), &d_cnt))) return rc;
  int64_t* d_counts = static_cast<int64_t*>(d_cnt);
  R3D_HIP(hipMemcpyAsync(d_counts + world, &n_mine, sizeof(int64_t), hipMemcpyHostToDevice, vs->ctx->stream));
  std::vector<int64_t> eight((size_t)world, (int64_t)sizeof(int64_t)), counts((size_t)world), bytes((size_t)world);
  if ((rc = r3d_comm_allgather(comm, d_counts + world, eight.data(), d_counts, R3D_GATHER_AUTO))) return rc;
  R3D_HIP(hipMemcpyAsync(counts.data(), d_counts, (size_t)world * sizeof(int64_t), hipMemcpyDeviceToHost, vs->ctx->stream));
  R3D_HIP(hipStreamSynchronize(vs->ctx->stream));
  if (rc_mine) return rc_mine;  // this rank's own error message stands
  int64_t total = 0;
  for (int r = 0; r < world; ++r) {
    if (counts[r] < 0) {
      r3d_set_error("rank %d could not list its voxel set (overflow): no union was formed", r);
      return R3D_ERR_NOMEM;
    }
    bytes[r] = counts[r] * (int64_t)sizeof(uint64_t);
    total += counts[r];
  }
  if (total == 0) return R3D_OK;
  void* d_all = nullptr;
  if ((rc = r3d_scratch(vs->ctx, kWsIn, (size_t)total * sizeof(uint64_t), &d_all))) return rc;
  if ((rc = r3d_comm_allgather(comm, d_mine, bytes.data(), d_all, R3D_GATHER_AUTO))) return rc;
  return r3d_voxelset_insert_codes(vs, static_cast<const uint64_t*>(d_all), total);
}

int r3d_voxelset_codes(r3d_voxelset* vs, uint64_t* h_codes_sorted, int64_t cap, int64_t* n_out) {
  R3D_REQUIRE(vs != nullptr && n_out != nullptr, "NULL argument");
  if (!h_codes_sorted) {   // count only
    int64_t n = 0, ign = 0, over = 0;
    int rc = r3d_voxelset_stats(vs, &n, &ign, &over);
    if (rc) return rc;
    *n_out = n;
    if (over > 0) {
      r3d_set_error("voxel set overflowed (%lld points found no slot): create it with a larger capacity", (long long)over);
      return R3D_ERR_NOMEM;
    }
    return R3D_OK;
  }
  uint64_t* d_list = nullptr;
  int64_t n = 0;
  int rc = codes_to_device_list(vs, &d_list, &n);
  *n_out = n;
  if (rc) return rc;
  R3D_REQUIRE(cap >= n, "buffer holds %lld codes, set has %lld", (long long)cap, (long long)n);
  if (n == 0) return R3D_OK;
  return r3d_download_pageable(vs->ctx, h_codes_sorted, d_list, (size_t)n * sizeof(uint64_t));
}

}  // extern "C"
