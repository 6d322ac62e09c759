// RANSAC consensus, stated once for every estimator of the library: the plane of a cloud (r3d_ransac.hip: items are points,
// a hypothesis is 6 floats) and the pose between two clouds (r3d_register.hip: items are point pairs, 12 floats).  A call is
//   sample_row           the counter-based sampler: hypothesis h draws its three items (also on the host: r3d_ransac_rows)
//   the estimator's own hypothesis kernel -> hyp: SoA rows of h_pad floats (NaN when invalid), rows [H][3], valid [H]
//   the estimator's own count_kernel<R>, the hot path: every hypothesis against every item -> partial counts [chunk][h]
//   fold_kernel          per hypothesis, the sum over the chunks (integers: the same bits for every chunking) -> counts
//   best_kernel          one workgroup: the lowest h among the maximal counts, the number of valid hypotheses -> BestHead,
//                        then the estimator's tail
//   the estimator's own refit, host solve and mask
// plan() fixes the launch geometry and layout() carves kWsMisc and kWsPartials for all of it.  The two count kernels have one
// shape (lanes own R hypotheses in registers, the chunk goes through two LDS tile buffers, every lane reads the same item) but
// stay apart: written as one template over an item trait, the plane instantiations came out of the compiler with two more
// VGPRs (130 at R = 2: a wave per SIMD fewer), see DESIGN 4.5h.
#pragma once

#include <algorithm>
#include <cmath>

#include "r3d_internal.h"

namespace r3d_consensus {

constexpr int kThreads = 256;
constexpr int kMaxWorkgroups = 4096;  // chunks x hypothesis blocks is kept near this: the partial counts stay <= 16 MiB
constexpr int kMinTiles = 4;
constexpr int kRefitBlocks = 1024;

__host__ __device__ __forceinline__ uint64_t splitmix64(uint64_t z) {
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  return z ^ (z >> 31);
}

__host__ __device__ __forceinline__ uint32_t sample_row(uint64_t seed, uint64_t h, int j, uint64_t n) {
  const uint64_t a = splitmix64(seed + (3 * h + (uint64_t)j + 1) * 0x9E3779B97F4A7C15ull);
#if defined(__HIP_DEVICE_COMPILE__)
  return (uint32_t)__umul64hi(a, n);
#else
  return (uint32_t)(((unsigned __int128)a * n) >> 64);
#endif
}

// what the estimators' entry points ask of the hypothesis count and the threshold
inline int check_args(int H, double thr) {
  R3D_REQUIRE(H >= 1 && H <= 65536, "n_hypotheses must be in [1, 65536], got %d", H);
  R3D_REQUIRE(std::isfinite(thr) && thr > 0.0, "distance_threshold must be finite and > 0, got %g", thr);
  return R3D_OK;
}

struct Plan {
  int H;
  int R;                // hypotheses per lane: the most the hypothesis count fills one workgroup with
  int h_pad, h_blocks;  // H rounded up to whole blocks of kThreads * R hypotheses
  int64_t chunk_items;  // items per workgroup of the count kernel, a multiple of the tile
  int chunks;
  int rblocks;          // workgroups of the grid-stride passes over the items (refit, mask)
};

inline Plan plan(int64_t n_items, int H, int tile_items) {
  Plan p;
  p.H = H;
  p.R = H >= 4 * kThreads ? 4 : H >= 2 * kThreads ? 2 : 1;
  const int per_block = kThreads * p.R;
  p.h_pad = (H + per_block - 1) / per_block * per_block;
  p.h_blocks = p.h_pad / per_block;
  const int64_t tiles = (n_items + tile_items - 1) / tile_items;
  const int64_t max_chunks = std::max<int64_t>(1, kMaxWorkgroups / p.h_blocks);
  // at least kMinTiles tiles per chunk: a workgroup's hypothesis loads and partial-count stores are paid per chunk
  p.chunk_items = std::max<int64_t>((tiles + max_chunks - 1) / max_chunks, std::min<int64_t>(tiles, kMinTiles)) * tile_items;
  p.chunks = (int)((n_items + p.chunk_items - 1) / p.chunk_items);
  p.rblocks = (int)std::min<int64_t>((n_items + kThreads - 1) / kThreads, kRefitBlocks);
  return p;
}

// kWsMisc: what the host reads (the estimator's Misc), the hypotheses, their rows, validity and counts; kWsPartials: the
// partial counts, then the refit's sum rows
struct Layout {
  void* misc;
  float* hyp;
  uint32_t *rows, *valid, *counts, *partial;
  double* part;
};

inline int layout(r3d_ctx* ctx, const Plan& p, int params, int sums, size_t misc_bytes, Layout* out) {
  r3d_carve s5, s4;
  const auto misc = s5.take<char>(misc_bytes);   // one piece: the estimator's Misc struct, read back in one copy
  const auto hyp = s5.take<float>((size_t)params * p.h_pad);
  const auto rows = s5.take<uint32_t>((size_t)3 * p.H), valid = s5.take<uint32_t>(p.H), counts = s5.take<uint32_t>(p.H);
  const auto partial = s4.take<uint32_t>((size_t)p.chunks * p.h_pad);
  const auto part = s4.take<double>((size_t)p.rblocks * sums);
  int rc;
  if ((rc = r3d_scratch(ctx, kWsMisc, s5)) || (rc = r3d_scratch(ctx, kWsPartials, s4))) return rc;
  *out = {s5.at(misc), s5.at(hyp), s5.at(rows), s5.at(valid), s5.at(counts), s4.at(partial), s4.at(part)};
  return R3D_OK;
}

// the head of every estimator's Misc (the one copy the host reads back): best_kernel's result
struct BestHead {
  uint32_t best_h, c_best, n_valid, pad;
  uint32_t rows[4];
};

#if defined(__HIPCC__)
// counts[h] = valid[h] ? sum over the chunks : 0
static __global__ __launch_bounds__(kThreads) void fold_kernel(const uint32_t* __restrict__ partial, int chunks, int h_pad, int H,
                                                               const uint32_t* __restrict__ valid, uint32_t* __restrict__ counts,
                                                               uint32_t* __restrict__ counts_out) {
  const int h = blockIdx.x * kThreads + threadIdx.x;
  if (h >= H) return;
  uint32_t c = 0;
  for (int k = 0; k < chunks; ++k) c += partial[(size_t)k * h_pad + h];
  if (!valid[h]) c = 0;
  counts[h] = c;
  if (counts_out) counts_out[h] = c;
}

// one workgroup: key = count << 32 | ~h, the maximum is the lowest h among the maximal counts.  Misc has a BestHead `head`;
// thread 0 fills it and calls tail(misc, j, r) with the best hypothesis' j-th row r as it reads it.
template <class Misc, class Tail>
__global__ __launch_bounds__(kThreads) void best_kernel(const uint32_t* __restrict__ counts, const uint32_t* __restrict__ valid,
                                                        const uint32_t* __restrict__ rows, int H, const Tail tail,
                                                        Misc* __restrict__ misc) {
  uint64_t key = 0;
  uint32_t nv = 0;
  for (int h = threadIdx.x; h < H; h += kThreads) {
    const uint64_t k = ((uint64_t)counts[h] << 32) | (uint32_t)~(uint32_t)h;
    key = k > key ? k : key;
    nv += valid[h];
  }
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    const uint64_t o = __shfl_down(key, off, 64);
    key = o > key ? o : key;
    nv += __shfl_down(nv, off, 64);
  }
  __shared__ uint64_t sk[kThreads / 64];
  __shared__ uint32_t sv[kThreads / 64];
  if ((threadIdx.x & 63) == 0) {
    sk[threadIdx.x >> 6] = key;
    sv[threadIdx.x >> 6] = nv;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    for (int w = 1; w < kThreads / 64; ++w) {
      key = sk[w] > key ? sk[w] : key;
      nv += sv[w];
    }
    const uint32_t h = ~(uint32_t)key;
    BestHead& head = misc->head;
    head.best_h = h;
    head.c_best = (uint32_t)(key >> 32);
    head.n_valid = nv;
    head.pad = 0;
    for (int j = 0; j < 3; ++j) {
      const uint32_t r = rows[3 * h + j];
      head.rows[j] = r;
      tail(misc, j, r);
    }
    head.rows[3] = 0;
  }
}
#endif

}  // namespace r3d_consensus
