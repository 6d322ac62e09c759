// FPFH descriptors of an index's own cloud and brute-force nearest feature rows for gfx950 (MI355X).
//
// NOT IN THE REFERENCE (users of this kind of pipeline call Open3D's compute_fpfh_feature and its feature matching to START a
// registration; no parity with Open3D or PCL is claimed).  Semantics: include/r3d.h (r3d_fpfh_knn, r3d_feature_match) and
// DESIGN.md section 4.5r.
//
//   r3d_fpfh_knn       three launches over stored lists: the index's exact k-NN lists (r3d_nn_index_knn_self) into scratch, then
//     spfh_kernel      one lane per point: the pair features of its list in f32, three 11-bin integer histograms kept as bytes in
//                      LDS (36-byte rows: 9 dwords per lane, a stride of 9 banks, conflict-free), written as one 36-byte row per
//                      point (33 counts + 3 zero bytes) so that the gather of the next pass is nine aligned dword loads
//     fpfh_kernel      one lane per point: 33 f32 accumulators in registers, the list walked in order, every neighbour's byte row
//                      gathered and weighted by 1 / d2; the count of a row is the sum of its first 11 bytes
//   r3d_feature_match  match_kernel<R>: lanes own R source rows (33 VGPRs each) and a running (dist, j) minimum; the workgroup's
//                      chunk of target rows goes through LDS in tiles of 128 rows padded to 36 floats, and every lane reads the
//                      SAME row: nine broadcast ds_read_b128 serve 64 R rows.  Grid = source blocks x target chunks; each
//                      workgroup writes its partial minima [chunk][row]; match_fold_kernel takes the chunks in ascending order
//                      with a strict <, so the lowest j of equal distances wins whatever the chunking.  The mutual filter and
//                      the compaction: r3d_register.hip.
// Every sum is its own f32 operation in the order the header writes (-ffp-contract=off), divisions and square roots are IEEE.
#include <algorithm>
#include <cmath>

#include "r3d_internal.h"

namespace {

constexpr int kThreads = 256;
constexpr int kBins = 11;
constexpr int kDim = R3D_FPFH_DIM;       // 33
constexpr int kRowBytes = 36;            // a stored histogram row: 33 counts + 3 zero bytes
constexpr uint32_t kNone = 0xffffffffu;

constexpr float kThetaCos[10] = R3D_FPFH_THETA_COS;
constexpr float kThetaSin[10] = R3D_FPFH_THETA_SIN;

__device__ __forceinline__ float dot3(float ax, float ay, float az, float bx, float by, float bz) { return (ax * bx + ay * by) + az * bz; }

__device__ __forceinline__ bool normal_ok(float x, float y, float z) {
  return isfinite(x) && isfinite(y) && isfinite(z) && !(x == 0.f && y == 0.f && z == 0.f);
}

__device__ __forceinline__ int bin11(float f) {
  const float t = (f + 1.0f) * 5.5f;
  return t < 1.0f ? 0 : t >= 10.0f ? 10 : (int)t;
}

__device__ __forceinline__ int theta_bin(float x, float y) {
  int b = 0;
#pragma unroll
  for (int m = 0; m < 10; ++m) {
    const float cr = kThetaCos[m] * y - kThetaSin[m] * x;
    const bool past = m < 5 ? (y >= 0.f || cr >= 0.f) : (y >= 0.f && cr >= 0.f);
    b += past ? 1 : 0;
  }
  return b;
}

// rows36 [n][36] u8 (always), spfh_out [n][33] u8 and count_out [n] u32 (optional)
__global__ __launch_bounds__(kThreads) void spfh_kernel(const float* __restrict__ xyz, const float* __restrict__ nrm,
                                                        const uint32_t* __restrict__ idx, const float* __restrict__ d2l, int64_t n, int k,
                                                        float r2, uint8_t* __restrict__ rows36, uint8_t* __restrict__ spfh_out,
                                                        uint32_t* __restrict__ count_out) {
  __shared__ __attribute__((aligned(16))) uint8_t hist[kThreads][kRowBytes];
  const int t = threadIdx.x;
  const int64_t base = (int64_t)blockIdx.x * kThreads, i = base + t;
  uint32_t* hw = reinterpret_cast<uint32_t*>(hist[t]);
#pragma unroll
  for (int q = 0; q < kRowBytes / 4; ++q) hw[q] = 0;
  uint32_t cnt = 0;
  if (i < n) {
    const float px = xyz[i * 3], py = xyz[i * 3 + 1], pz = xyz[i * 3 + 2];
    const float nix = nrm[i * 3], niy = nrm[i * 3 + 1], niz = nrm[i * 3 + 2];
    const bool ok_i = normal_ok(nix, niy, niz);
    for (int s = 0; s < k && ok_i; ++s) {
      const uint32_t j = idx[i * k + s];
      if (j == kNone || (int64_t)j >= n) break;
      if (d2l[i * k + s] > r2) break;
      const float njx = nrm[(int64_t)j * 3], njy = nrm[(int64_t)j * 3 + 1], njz = nrm[(int64_t)j * 3 + 2];
      if (!normal_ok(njx, njy, njz)) continue;
      float dx = xyz[(int64_t)j * 3] - px, dy = xyz[(int64_t)j * 3 + 1] - py, dz = xyz[(int64_t)j * 3 + 2] - pz;
      const float L = sqrtf((dx * dx + dy * dy) + dz * dz);
      if (!(L > 0.f) || !isfinite(L)) continue;
      const float ai = dot3(nix, niy, niz, dx, dy, dz), aj = dot3(njx, njy, njz, dx, dy, dz);
      float ux = nix, uy = niy, uz = niz, tx = njx, ty = njy, tz = njz;
      if (fabsf(aj) > fabsf(ai)) {
        ux = njx, uy = njy, uz = njz, tx = nix, ty = niy, tz = niz;
        dx = -dx, dy = -dy, dz = -dz;
      }
      const float hx = dx / L, hy = dy / L, hz = dz / L;
      const float vx = hy * uz - hz * uy, vy = hz * ux - hx * uz, vz = hx * uy - hy * ux;
      const float lv = sqrtf((vx * vx + vy * vy) + vz * vz);
      if (!(lv > 0.f) || !isfinite(lv)) continue;
      const float ex = vx / lv, ey = vy / lv, ez = vz / lv;
      const float wx = uy * ez - uz * ey, wy = uz * ex - ux * ez, wz = ux * ey - uy * ex;
      const float alpha = dot3(ex, ey, ez, tx, ty, tz), phi = dot3(ux, uy, uz, hx, hy, hz);
      const float x = dot3(ux, uy, uz, tx, ty, tz), y = dot3(wx, wy, wz, tx, ty, tz);
      if (!isfinite(alpha) || !isfinite(phi) || !isfinite(x) || !isfinite(y) || (x == 0.f && y == 0.f)) continue;
      hist[t][theta_bin(x, y)] += 1;
      hist[t][kBins + bin11(alpha)] += 1;
      hist[t][2 * kBins + bin11(phi)] += 1;
      ++cnt;
    }
    uint32_t* dst = reinterpret_cast<uint32_t*>(rows36 + i * kRowBytes);
#pragma unroll
    for (int q = 0; q < kRowBytes / 4; ++q) dst[q] = hw[q];
    if (count_out) count_out[i] = cnt;
  }
  if (spfh_out) {
    __syncthreads();
    const int rows = (int)(n - base < kThreads ? n - base : kThreads);
    for (int e = t; e < rows * kDim; e += kThreads) spfh_out[base * kDim + e] = hist[e / kDim][e % kDim];
  }
}

__global__ __launch_bounds__(kThreads) void fpfh_kernel(const uint32_t* __restrict__ idx, const float* __restrict__ d2l, int64_t n, int k,
                                                        float r2, const uint8_t* __restrict__ rows36, float* __restrict__ out) {
  const int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x;
  if (i >= n) return;
  float A[kDim];
#pragma unroll
  for (int b = 0; b < kDim; ++b) A[b] = 0.0f;
  uint32_t w[kRowBytes / 4];
  for (int s = 0; s < k; ++s) {
    const uint32_t j = idx[i * k + s];
    if (j == kNone || (int64_t)j >= n) break;
    const float d2 = d2l[i * k + s];
    if (d2 > r2) break;
    if (!(d2 > 0.f) || !isfinite(d2)) continue;
    const uint32_t* rj = reinterpret_cast<const uint32_t*>(rows36 + (int64_t)j * kRowBytes);
#pragma unroll
    for (int q = 0; q < kRowBytes / 4; ++q) w[q] = rj[q];
    uint32_t cj = 0;
#pragma unroll
    for (int b = 0; b < kBins; ++b) cj += (w[b >> 2] >> (8 * (b & 3))) & 255u;
    if (cj == 0) continue;   // an all-zero P_j adds +0.0 to sums that are never -0.0
    const float scale = 100.0f / (float)cj;
#pragma unroll
    for (int b = 0; b < kDim; ++b) {
      const float P = (float)((w[b >> 2] >> (8 * (b & 3))) & 255u) * scale;
      A[b] = A[b] + P / d2;
    }
  }
  const uint32_t* ri = reinterpret_cast<const uint32_t*>(rows36 + i * kRowBytes);
#pragma unroll
  for (int q = 0; q < kRowBytes / 4; ++q) w[q] = ri[q];
  uint32_t ci = 0;
#pragma unroll
  for (int b = 0; b < kBins; ++b) ci += (w[b >> 2] >> (8 * (b & 3))) & 255u;
  const float scale_i = ci ? 100.0f / (float)ci : 0.0f;
#pragma unroll
  for (int s3 = 0; s3 < 3; ++s3) {
    float T = 0.0f;
#pragma unroll
    for (int b = 0; b < kBins; ++b) T = T + A[s3 * kBins + b];
    const bool some = T > 0.f;
    const float f = some ? 100.0f / T : 0.0f;
#pragma unroll
    for (int b = 0; b < kBins; ++b) {
      const int e = s3 * kBins + b;
      const float P = ci ? (float)((w[e >> 2] >> (8 * (e & 3))) & 255u) * scale_i : 0.0f;
      out[i * kDim + e] = P + (some ? A[e] * f : 0.0f);
    }
  }
}

// ---- nearest feature row ---------------------------------------------------------------------------------------------------------
constexpr int kTileRows = 128;
constexpr int kTileStride = 36;   // floats per tile row: 33 + 3 of padding, rows 16-byte aligned
constexpr int kTargetBlocks = 2048;

// blockIdx.x = block of kThreads * R source rows (lane t owns rows ab + t + r * kThreads), blockIdx.y = chunk of chunk_rows target
// rows (a multiple of kTileRows).  part_d / part_j [chunks][na].
template <int R>
__global__ __launch_bounds__(kThreads) void match_kernel(const float* __restrict__ fa, int64_t na, const float* __restrict__ fb, int64_t nb,
                                                         int64_t chunk_rows, float* __restrict__ part_d, uint32_t* __restrict__ part_j) {
  __shared__ __attribute__((aligned(16))) float tile[kTileRows * kTileStride];
  const int t = threadIdx.x;
  const int64_t ab = (int64_t)blockIdx.x * (kThreads * R);
  float a[R][kDim], best[R];
  uint32_t bj[R];
#pragma unroll
  for (int r = 0; r < R; ++r) {
    const int64_t row = ab + t + (int64_t)r * kThreads;
#pragma unroll
    for (int b = 0; b < kDim; ++b) a[r][b] = row < na ? fa[row * kDim + b] : 0.0f;
    best[r] = INFINITY;
    bj[r] = kNone;
  }
  const int64_t begin = (int64_t)blockIdx.y * chunk_rows;
  const int64_t end = begin + chunk_rows < nb ? begin + chunk_rows : nb;
  for (int64_t base = begin; base < end; base += kTileRows) {
    const int m = (int)(end - base < kTileRows ? end - base : kTileRows);
    __syncthreads();   // the previous tile has been read
    for (int e = t; e < m * kDim; e += kThreads) tile[(e / kDim) * kTileStride + (e % kDim)] = fb[base * kDim + e];
    __syncthreads();
    for (int p = 0; p < m; ++p) {
      const float4* __restrict__ tp = reinterpret_cast<const float4*>(tile + p * kTileStride);
      float v[kTileStride];
#pragma unroll
      for (int q = 0; q < kTileStride / 4; ++q) {
        const float4 f = tp[q];
        v[4 * q] = f.x;
        v[4 * q + 1] = f.y;
        v[4 * q + 2] = f.z;
        v[4 * q + 3] = f.w;
      }
      const uint32_t j = (uint32_t)(base + p);
#pragma unroll
      for (int r = 0; r < R; ++r) {
        float d = 0.0f;
#pragma unroll
        for (int b = 0; b < kDim; ++b) {
          const float e = a[r][b] - v[b];
          d = d + e * e;
        }
        if (d < best[r]) {   // NaN and +inf never win; ascending j: the first of equal distances stays
          best[r] = d;
          bj[r] = j;
        }
      }
    }
  }
#pragma unroll
  for (int r = 0; r < R; ++r) {
    const int64_t row = ab + t + (int64_t)r * kThreads;
    if (row < na) {
      part_d[(int64_t)blockIdx.y * na + row] = best[r];
      part_j[(int64_t)blockIdx.y * na + row] = bj[r];
    }
  }
}

__global__ __launch_bounds__(kThreads) void match_fold_kernel(const float* __restrict__ part_d, const uint32_t* __restrict__ part_j,
                                                              int chunks, int64_t na, uint32_t* __restrict__ idx_out,
                                                              float* __restrict__ dist_out) {
  const int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x;
  if (i >= na) return;
  float best = INFINITY;
  uint32_t bj = kNone;
  for (int c = 0; c < chunks; ++c) {
    const float d = part_d[(int64_t)c * na + i];
    if (d < best) {
      best = d;
      bj = part_j[(int64_t)c * na + i];
    }
  }
  idx_out[i] = bj;
  if (dist_out) dist_out[i] = best;
}

}  // namespace

// idx / dist of the nearest row of b for every row of a (asynchronous); the partial minima go to the workspace `part`
int r3d_match_nearest(r3d_ctx* ctx, const float* d_a, int64_t na, const float* d_b, int64_t nb, uint32_t* d_idx_out, float* d_dist_out,
                      r3d_workspace part) {
  const int R = na >= (int64_t)2 * kThreads * 256 ? 2 : 1;   // two rows per lane once that still leaves a block per CU
  const int64_t a_blocks = (na + kThreads * R - 1) / (kThreads * R);
  const int64_t tiles = (nb + kTileRows - 1) / kTileRows;
  const int64_t want = std::max<int64_t>(1, kTargetBlocks / a_blocks);
  const int64_t chunk_tiles = (tiles + std::min(tiles, want) - 1) / std::min(tiles, want);
  const int64_t chunk_rows = chunk_tiles * kTileRows;
  const int chunks = (int)((nb + chunk_rows - 1) / chunk_rows);
  r3d_carve ws;
  const auto part_d_h = ws.take<float>((size_t)chunks * na);
  const auto part_j_h = ws.take<uint32_t>((size_t)chunks * na);
  int rc = r3d_scratch(ctx, part, ws);
  if (rc) return rc;
  float* part_d = ws.at(part_d_h);
  uint32_t* part_j = ws.at(part_j_h);
  const dim3 grid((unsigned)a_blocks, (unsigned)chunks);
  if (R == 2) hipLaunchKernelGGL((match_kernel<2>), grid, dim3(kThreads), 0, ctx->stream, d_a, na, d_b, nb, chunk_rows, part_d, part_j);
  else hipLaunchKernelGGL((match_kernel<1>), grid, dim3(kThreads), 0, ctx->stream, d_a, na, d_b, nb, chunk_rows, part_d, part_j);
  hipLaunchKernelGGL(match_fold_kernel, dim3((unsigned)((na + kThreads - 1) / kThreads)), dim3(kThreads), 0, ctx->stream,
                     (const float*)part_d, (const uint32_t*)part_j, chunks, na, d_idx_out, d_dist_out);
  R3D_HIP(hipGetLastError());
  return R3D_OK;
}

extern "C" {

int r3d_fpfh_knn(r3d_nn_index* index, int k, double radius, const float* d_normals, float* d_fpfh_out, uint8_t* d_spfh_out,
                 uint32_t* d_count_out) {
  R3D_REQUIRE(index != nullptr, "nn index is NULL");
  R3D_REQUIRE(k >= 3 && k <= 32, "k must be in [3, 32], got %d", k);
  R3D_REQUIRE(!std::isnan(radius), "radius is NaN");
  R3D_REQUIRE(d_normals != nullptr && d_fpfh_out != nullptr, "d_normals or d_fpfh_out is NULL");
  const float* d_xyz = nullptr;
  int64_t n = 0;
  r3d_ctx* ctx = nullptr;
  int rc = r3d_nn_index_target(index, &d_xyz, &n, &ctx);
  if (rc) return rc;
  const struct {
    const void* p;
    size_t bytes;
  } out[3] = {{d_fpfh_out, (size_t)n * kDim * 4}, {d_spfh_out, (size_t)n * kDim}, {d_count_out, (size_t)n * 4}};
  for (int i = 0; i < 3; ++i) {
    R3D_REQUIRE(!r3d_ranges_overlap(out[i].p, out[i].bytes, d_xyz, (size_t)n * 12), "an output overlaps the index's cloud");
    R3D_REQUIRE(!r3d_ranges_overlap(out[i].p, out[i].bytes, d_normals, (size_t)n * 12), "an output overlaps the normals");
    for (int j = i + 1; j < 3; ++j) R3D_REQUIRE(!r3d_ranges_overlap(out[i].p, out[i].bytes, out[j].p, out[j].bytes), "outputs overlap each other");
  }
  if ((rc = r3d_ctx_enter(ctx))) return rc;
  // kWsIn: the lists (idx | d2); kWsOut: the 36-byte histogram rows.  The index's own search takes no workspace.
  r3d_carve lists;
  const auto idx_h = lists.take<uint32_t>((size_t)n * k);
  const auto d2l_h = lists.take<float>((size_t)n * k);
  void* rows = nullptr;
  if ((rc = r3d_scratch(ctx, kWsIn, lists))) return rc;
  if ((rc = r3d_scratch(ctx, kWsOut, (size_t)n * kRowBytes, &rows))) return rc;
  uint32_t* idx = lists.at(idx_h);
  float* d2l = lists.at(d2l_h);
  if ((rc = r3d_nn_index_knn_self(index, k, idx, d2l))) return rc;
  for (int i = 0; i < 3; ++i)
    if (out[i].p) r3d_wrote(ctx, out[i].p, out[i].bytes);
  const float r2 = radius > 0.0 ? (float)(radius * radius) : INFINITY;
  const dim3 grid((unsigned)((n + kThreads - 1) / kThreads));
  hipLaunchKernelGGL(spfh_kernel, grid, dim3(kThreads), 0, ctx->stream, d_xyz, d_normals, (const uint32_t*)idx, (const float*)d2l, n, k, r2,
                     static_cast<uint8_t*>(rows), d_spfh_out, d_count_out);
  hipLaunchKernelGGL(fpfh_kernel, grid, dim3(kThreads), 0, ctx->stream, (const uint32_t*)idx, (const float*)d2l, n, k, r2,
                     (const uint8_t*)rows, d_fpfh_out);
  R3D_HIP(hipGetLastError());
  return R3D_OK;
}

}  // extern "C"
