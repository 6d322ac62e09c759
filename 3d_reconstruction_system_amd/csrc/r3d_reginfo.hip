// Pair sums of a registration for gfx950 (MI355X): what the information matrix, the fitness and the rmse of a pose under test are
// made of (r3d_information_from_sums, r3d_posegraph.cpp).  NOT IN THE REFERENCE; include/r3d.h is the specification.
//
// r3d_registration_sums -- roofline: HBM / L2 gather, 20 B/row streamed (12 src + 4 idx + 4 d2) + 12 B gathered from the target
//   per kept pair; latency-bound on the gather and tiny next to the nearest-neighbour query that wrote idx / d2.
//   One lane per source row, grid-stride; 11 fp64 accumulators per lane; wavefront shuffle tree -> LDS across the 4 waves -> one
//   partial row per workgroup -> one fixed-order finish workgroup (r3d_sums_dev.h).  No float atomics: the same bits run to run.
#include <cmath>

#include "r3d_internal.h"
#include "r3d_sums_dev.h"

namespace {

constexpr int kThreads = r3d_sums::kThreads;
constexpr int kSums = R3D_REGISTRATION_SUMS;

__global__ __launch_bounds__(kThreads) void registration_sums_kernel(const float* __restrict__ src, int64_t n_src,
                                                                     const float* __restrict__ tgt, int64_t n_tgt,
                                                                     const uint32_t* __restrict__ idx, const float* __restrict__ d2,
                                                                     float max_d2, double* __restrict__ partials) {
  __shared__ double red[kThreads / 64][kSums];
  double acc[kSums];
#pragma unroll
  for (int k = 0; k < kSums; ++k) acc[k] = 0.0;
  for (int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x; i < n_src; i += (int64_t)gridDim.x * kThreads) {
    const float d = d2[i];
    if (!(d <= max_d2)) continue;   // the pair AT max_d2 is in; a NaN d2 is out
    const int64_t j = (int64_t)idx[i];
    if (j >= n_tgt) continue;       // the index array is data: never read past the target cloud
    const double p[3] = {(double)src[i * 3 + 0], (double)src[i * 3 + 1], (double)src[i * 3 + 2]};
    const double q[3] = {(double)tgt[j * 3 + 0], (double)tgt[j * 3 + 1], (double)tgt[j * 3 + 2]};
    // the six values come from fp32, so their fp64 sum is finite exactly when all of them are
    if (!isfinite(((p[0] + p[1]) + p[2]) + ((q[0] + q[1]) + q[2]))) continue;
    acc[0] += 1.0;
    acc[1] += q[0];
    acc[2] += q[1];
    acc[3] += q[2];
    acc[4] += q[0] * q[0];
    acc[5] += q[0] * q[1];
    acc[6] += q[0] * q[2];
    acc[7] += q[1] * q[1];
    acc[8] += q[1] * q[2];
    acc[9] += q[2] * q[2];
    acc[10] += (double)d;
  }
  r3d_sums::block_reduce_store<kSums>(acc, red, partials + (int64_t)blockIdx.x * kSums);
}

// ONE workgroup: the partial rows in fixed order -> the 11 sums.  No state, no solve.
__global__ __launch_bounds__(kThreads) void registration_sums_finish_kernel(const double* __restrict__ partials, int n_rows,
                                                                            double* __restrict__ sums_out) {
  r3d_sums::finish_rows<kSums>(partials, n_rows, sums_out, nullptr, [](const double*, double*, double*) { return 0; });
}

// d_work: [blocks][11] partial rows followed by the 11 sums.  Both launches, the copy and the wait; h_sums is written on success.
int sums_pass(r3d_ctx* ctx, const float* d_src, int64_t n_src, const float* d_tgt, int64_t n_tgt, const uint32_t* d_idx,
              const float* d_d2, float max_d2, double* d_work, int blocks, double* h_sums) {
  double* d_sums = d_work + (size_t)blocks * kSums;
  hipLaunchKernelGGL(registration_sums_kernel, dim3((unsigned)blocks), dim3(kThreads), 0, ctx->stream, d_src, n_src, d_tgt, n_tgt,
                     d_idx, d_d2, max_d2, d_work);
  R3D_HIP(hipGetLastError());
  hipLaunchKernelGGL(registration_sums_finish_kernel, dim3(1), dim3(kThreads), 0, ctx->stream, d_work, blocks, d_sums);
  R3D_HIP(hipGetLastError());
  double sums[kSums];
  R3D_HIP(hipMemcpyAsync(sums, d_sums, sizeof(sums), hipMemcpyDeviceToHost, ctx->stream));
  R3D_HIP(hipStreamSynchronize(ctx->stream));
  for (int k = 0; k < kSums; ++k) h_sums[k] = sums[k];
  return R3D_OK;
}

}  // namespace

extern "C" {

int r3d_registration_sums(r3d_ctx* ctx, const float* d_src, int64_t n_src, const float* d_tgt, int64_t n_tgt, const uint32_t* d_idx,
                          const float* d_d2, float max_d2, double* h_sums) {
  R3D_REQUIRE(ctx != nullptr, "ctx is NULL");
  R3D_REQUIRE(h_sums != nullptr, "h_sums is NULL");
  R3D_REQUIRE(n_src >= 0 && n_tgt >= 0, "negative cloud size");
  R3D_REQUIRE(n_tgt < ((int64_t)1 << 32), "target cloud too large for uint32 indices");
  R3D_REQUIRE(max_d2 >= 0.f, "max_d2 must be >= 0 (got %g): an information matrix needs a distance gate", (double)max_d2);
  R3D_REQUIRE(n_src == 0 || (d_src && d_tgt && d_idx && d_d2), "NULL device pointer");
  int rc = r3d_ctx_enter(ctx);
  if (rc) return rc;
  if (n_src == 0) {
    for (int k = 0; k < kSums; ++k) h_sums[k] = 0.0;
    return R3D_OK;
  }
  int64_t blocks = (n_src + kThreads - 1) / kThreads;
  if (blocks > (int64_t)ctx->num_cus * 4) blocks = (int64_t)ctx->num_cus * 4;
  // kWsRegSums (the partial rows, then the 11 sums; 90 kB at the most) is this synchronous entry point's alone, always asked for at
  // its largest size: nothing here depends on, or disturbs, what other calls leave in the context's shared workspaces.
  void* ws = nullptr;
  if ((rc = r3d_scratch(ctx, kWsRegSums, ((size_t)ctx->num_cus * 4 + 1) * kSums * sizeof(double), &ws))) return rc;
  return sums_pass(ctx, d_src, n_src, d_tgt, n_tgt, d_idx, d_d2, max_d2, static_cast<double*>(ws), (int)blocks, h_sums);
}

}  // extern "C"
