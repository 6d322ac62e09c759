// Frame-to-model tracking for gfx950 (MI355X): projective point-to-plane ICP of a new depth frame against the maps the TSDF
// volume predicts for a pose (r3d_tsdf_raycast) -- the fourth leg of integrate / extract / ray cast / track.  NOT IN THE
// REFERENCE (its poses come from COLMAP): build-defined, specified in include/r3d.h ("TSDF tracking").
//
//   track_kernel<kRgb>   one lane per source pixel: move it by M = T_total . S, project it into the model camera, gather the
//                        model vertex and normal at the nearest pixel, gate, and add the pair to the 29 fp64 sums of
//                        r3d_plane_sums.h.  A 256-thread workgroup owns 1024 consecutive pixels (thread t: base + t + 256 k,
//                        k = 0..3) and leaves one partial row (r3d_sums_dev.h's reduction): the launch shape is a function of
//                        the raster alone, so the sums
//                        are the same bits on every device and under every tuning.  Source rows are read coalesced (12 B per
//                        lane, consecutive); the gather lands near the lane's own pixel for the small motions tracking sees.
//                        M, the model pose and the intrinsics are wave-uniform.  The only LDS is the reduction's.
//                        kRgb adds the photometric term ("TSDF colour tracking"): for an accepted pair, a bilinear tap of the
//                        model's packed {I, gx, gy, 0} map (r3d_photo.hip), the gradient pulled back to the world, and the pair
//                        into the same normal equations -- 31 sums, the same tile, reduction, finish and state
//   the finish           r3d_plane::plane_finish_kernel<29 or 31> (r3d_plane_sums.h), ONE workgroup: partial rows in fixed order ->
//                        the sums -> Cholesky solve + exponential map -> the ICP state in HBM, as in r3d_plane.hip
//   track_levels         host: the whole step for one frame -- r3d_tsdf_track (one level) and r3d_tsdf_track_pyramid (coarse to fine
//                        over the depth pyramid of r3d_pyramid.hip, every level's model maps ray-cast at the guess) share it
//   track_rgb            host: the one-level step with the colour term; the passes, the guess's inverse and the read-back of the
//                        state are the ones track_levels uses
// No atomics: bitwise repeatable.  No search structure, no sort, no index: the association is one projection and one gather.
#include <cmath>

#include "r3d_internal.h"
#include "r3d_plane_sums.h"
#include "r3d_tsdf_dev.h"

namespace {

constexpr int kThreads = r3d_sums::kThreads;
constexpr int kPerLane = 4;
constexpr int kTile = kThreads * kPerLane;   // pixels per workgroup: part of the specification
using r3d_plane::kSums;
using r3d_plane::P3;
constexpr int kSumsRgb = kSums + 2;   // with the colour term: [29] the photometric pair count, [30] the sum of rI^2

struct TrackParams {
  double fx, fy, cx, cy;   // the camera's doubles
  double rm[9], tm[3];     // the pose the model maps were cast from, world -> camera
  double s[16];            // the guess: source camera -> world, row-major 4x4
  double dist2;            // dist_max * dist_max
  double cos_min;
  double wd, hd;           // (double) W, (double) H
  int width;
  int n_px;
};

__device__ __forceinline__ bool finite3(const P3& p) { return isfinite(p.x) && isfinite(p.y) && isfinite(p.z); }

// M = T_total . S, the loop of the solve's T_total update: every entry summed over m = 0..3 from 0.0 (rows 0..2 are used)
__device__ __forceinline__ void compose_M(const TrackParams& a, const double* __restrict__ state, double M[12]) {
#pragma unroll
  for (int r = 0; r < 3; ++r)
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      double v = 0.0;
#pragma unroll
      for (int m = 0; m < 4; ++m) {
        const double t = state ? state[r3d_sums::kStateTTotal + 4 * r + m] : (r == m ? 1.0 : 0.0);
        v += t * a.s[4 * m + c];
      }
      M[4 * r + c] = v;
    }
}

// what steps 1..10 leave of an accepted pair for the steps that follow them
struct Pair {
  double p[3], pm[3];   // the source point in the world and in the model camera
  double u, v;          // its projection, before rounding
  double r;             // the plane residual
};

// Steps 1..10 of "TSDF tracking" for source pixel i: the reject code, or the model pixel j after the pair has entered acc[0..28]
__device__ __forceinline__ int32_t associate(const TrackParams& a, const double M[12], const P3* __restrict__ SV, const P3* __restrict__ SN,
                                             const P3* __restrict__ MV, const P3* __restrict__ MN, int i, double* acc, Pair& o) {
  const P3 sv = SV[i];
  o.r = 0.0;
  if (!(finite3(sv) && sv.z > 0.0f)) return -1;
  const double x = (double)sv.x, y = (double)sv.y, z = (double)sv.z;
#pragma unroll
  for (int c = 0; c < 3; ++c) o.p[c] = ((M[4 * c] * x + M[4 * c + 1] * y) + M[4 * c + 2] * z) + M[4 * c + 3];
#pragma unroll
  for (int c = 0; c < 3; ++c) o.pm[c] = ((a.rm[3 * c] * o.p[0] + a.rm[3 * c + 1] * o.p[1]) + a.rm[3 * c + 2] * o.p[2]) + a.tm[c];
  if (!(o.pm[2] > 0.0)) return -2;
  o.u = a.fx * (o.pm[0] / o.pm[2]) + a.cx, o.v = a.fy * (o.pm[1] / o.pm[2]) + a.cy;
  const double uj = floor(o.u + 0.5), vj = floor(o.v + 0.5);
  if (!(uj >= 0.0 && uj < a.wd && vj >= 0.0 && vj < a.hd)) return -2;   // NaN fails every comparison
  const int j = (int)vj * a.width + (int)uj;                             // inside [0, n_px)
  const P3 qv = MV[j], qn = MN[j];
  if (!(finite3(qv) && finite3(qn) && !(qn.x == 0.0f && qn.y == 0.0f && qn.z == 0.0f))) return -3;
  const double q[3] = {(double)qv.x, (double)qv.y, (double)qv.z};
  const double n[3] = {(double)qn.x, (double)qn.y, (double)qn.z};
  const double d0 = o.p[0] - q[0], d1 = o.p[1] - q[1], d2 = o.p[2] - q[2];
  if (!((d0 * d0 + d1 * d1) + d2 * d2 <= a.dist2)) return -4;
  if (SN) {
    const P3 sn = SN[i];
    if (!(finite3(sn) && !(sn.x == 0.0f && sn.y == 0.0f && sn.z == 0.0f))) return -5;
    const double n0 = (double)sn.x, n1 = (double)sn.y, n2 = (double)sn.z;
    double g[3];
#pragma unroll
    for (int c = 0; c < 3; ++c) g[c] = (M[4 * c] * n0 + M[4 * c + 1] * n1) + M[4 * c + 2] * n2;
    if (!((g[0] * n[0] + g[1] * n[1]) + g[2] * n[2] >= a.cos_min)) return -5;
  }
  o.r = r3d_plane::plane_residual(o.p, q, n);
  r3d_plane::pair_accumulate(acc, 1.0, o.p, n, o.r);
  return j;
}

// ---- the photometric term ("TSDF colour tracking") ---------------------------------------------------------------------------------
struct PhotoParams {
  double w, i_max;   // w_photo (metres^2 per intensity^2) and the residual gate
};

// Steps 11..16 for a pixel whose geometric pair was accepted: the bilinear tap of the model's packed {I, gx, gy, 0} map at (u, v),
// the gradient pulled back to a world-space vector a, and the pair into [2..28] with J = [p x a ; a].  Returns (float) rI, or NaN
// where there is no photometric pair.  The four taps are four 16-byte gathers next to the lane's own pixel.
__device__ __forceinline__ float photo_pair(const TrackParams& a, const PhotoParams& ph, const float4* __restrict__ MP, float Is_f,
                                            const Pair& o, double* acc) {
  const double u0 = floor(o.u), v0 = floor(o.v);
  if (!(u0 >= 0.0 && u0 + 1.0 <= a.wd - 1.0 && v0 >= 0.0 && v0 + 1.0 <= a.hd - 1.0)) return NAN;
  const double fu = o.u - u0, fv = o.v - v0;
  const int j = (int)v0 * a.width + (int)u0;   // j + width + 1 <= n_px - 1
  const float4 t00 = MP[j], t01 = MP[j + 1], t10 = MP[j + a.width], t11 = MP[j + a.width + 1];
  const double c00[3] = {(double)t00.x, (double)t00.y, (double)t00.z}, c01[3] = {(double)t01.x, (double)t01.y, (double)t01.z};
  const double c10[3] = {(double)t10.x, (double)t10.y, (double)t10.z}, c11[3] = {(double)t11.x, (double)t11.y, (double)t11.z};
  double val[3];   // Im, gx, gy: a NaN tap makes its value NaN
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    const double top = c00[c] + fu * (c01[c] - c00[c]), bot = c10[c] + fu * (c11[c] - c10[c]);
    val[c] = top + fv * (bot - top);
  }
  const double rI = val[0] - (double)Is_f;
  const double gfx = val[1] * a.fx, gfy = val[2] * a.fy;
  const double b0 = gfx / o.pm[2], b1 = gfy / o.pm[2], b2 = -(gfx * o.pm[0] + gfy * o.pm[1]) / (o.pm[2] * o.pm[2]);
  double g[3];   // Rm^T b
#pragma unroll
  for (int c = 0; c < 3; ++c) g[c] = (a.rm[c] * b0 + a.rm[3 + c] * b1) + a.rm[6 + c] * b2;
  if (!(isfinite(rI) && isfinite(g[0]) && isfinite(g[1]) && isfinite(g[2]) && fabs(rI) <= ph.i_max)) return NAN;
  r3d_plane::jacobian_accumulate(acc, ph.w, o.p, g, rI);
  acc[kSums] += 1.0;
  acc[kSums + 1] += rI * rI;
  return (float)rI;
}

// One pass over the raster.  kRgb: with the colour term -- 31 sums per row (62 VGPRs of accumulators) instead of 29, photo_pair after
// an accepted pair, and a third output; the tile and the order are the same, and M, the poses and the intrinsics stay wave-uniform.
// Without it src_intensity, model_packed, ph and photo_out are never read.
template <bool kRgb>
__global__ __launch_bounds__(kThreads) void track_kernel(const float* __restrict__ src_vertex, const float* __restrict__ src_normal,
                                                         const float* __restrict__ model_vertex,
                                                         const float* __restrict__ model_normal,
                                                         const float* __restrict__ src_intensity,
                                                         const float4* __restrict__ model_packed, const TrackParams a,
                                                         const PhotoParams ph, const double* __restrict__ state,
                                                         double* __restrict__ partials, int32_t* __restrict__ match_out,
                                                         float* __restrict__ residual_out, float* __restrict__ photo_out) {
  constexpr int K = kRgb ? kSumsRgb : kSums;
  __shared__ double red[kThreads / 64][K];
  double M[12];
  compose_M(a, state, M);
  double acc[K];
#pragma unroll
  for (int k = 0; k < K; ++k) acc[k] = 0.0;
  const P3* SV = reinterpret_cast<const P3*>(src_vertex);
  const P3* SN = reinterpret_cast<const P3*>(src_normal);
  const P3* MV = reinterpret_cast<const P3*>(model_vertex);
  const P3* MN = reinterpret_cast<const P3*>(model_normal);
  const int base = (int)blockIdx.x * kTile + (int)threadIdx.x;   // n_px < 2^31 - kTile (checked by the host)
  for (int k = 0; k < kPerLane; ++k) {
    const int i = base + k * kThreads;
    if (i >= a.n_px) break;
    Pair o;
    const int32_t code = associate(a, M, SV, SN, MV, MN, i, acc, o);
    float rI = NAN;
    if (kRgb && code >= 0) rI = photo_pair(a, ph, model_packed, src_intensity[i], o, acc);
    if (match_out) match_out[i] = code;
    if (residual_out) residual_out[i] = code >= 0 ? (float)o.r : 0.0f;
    if (kRgb && photo_out) photo_out[i] = rI;
  }
  r3d_sums::block_reduce_store<K>(acc, red, partials + (int64_t)blockIdx.x * K);
}

struct Maps {
  const float *src_vertex, *src_normal, *model_vertex, *model_normal;
  const float *src_intensity = nullptr, *model_packed = nullptr;   // the colour term's: [H][W] f32 and [H][W][4] f32 {I, gx, gy, 0}
};

// the colour term's own argument checks; fills *ph
int photo_checks(const Maps& m, double w_photo, double i_max, PhotoParams* ph) {
  R3D_REQUIRE(m.src_intensity && m.model_packed, "NULL intensity map pointer");
  R3D_REQUIRE(((uintptr_t)m.model_packed & 15) == 0, "d_model_packed must be 16-byte aligned");
  R3D_REQUIRE(w_photo >= 0.0 && std::isfinite(w_photo), "w_photo must be >= 0 and finite");
  R3D_REQUIRE(i_max > 0.0 && std::isfinite(i_max), "i_max must be positive and finite");
  ph->w = w_photo, ph->i_max = i_max;
  return R3D_OK;
}

// the argument checks the three entry points share; fills *p
int track_checks(r3d_ctx* ctx, const r3d_camera* cam, const Maps& m, const double* h_model_pose_w2c, const double* h_S, double dist_max,
                 double cos_min, TrackParams* p) {
  R3D_REQUIRE(ctx != nullptr, "ctx is NULL");
  R3D_REQUIRE(cam != nullptr, "camera is NULL");
  R3D_REQUIRE(cam->ctx == ctx, "the camera belongs to another context");
  R3D_REQUIRE(m.src_vertex && m.model_vertex && m.model_normal, "NULL map pointer");
  R3D_REQUIRE(h_model_pose_w2c && h_S, "NULL pose pointer");
  R3D_REQUIRE(dist_max > 0.0 && std::isfinite(dist_max), "dist_max must be positive and finite");
  R3D_REQUIRE(cos_min >= -1.0 && cos_min <= 1.0, "cos_min must be in [-1, 1]");
  R3D_REQUIRE((int64_t)cam->width * cam->height < ((int64_t)1 << 31) - kTile, "raster of %d x %d pixels is too large for tracking",
              cam->height, cam->width);
  p->fx = cam->fx, p->fy = cam->fy, p->cx = cam->cx, p->cy = cam->cy;
  for (int k = 0; k < 9; ++k) p->rm[k] = h_model_pose_w2c[k];
  for (int k = 0; k < 3; ++k) p->tm[k] = h_model_pose_w2c[9 + k];
  for (int k = 0; k < 16; ++k) p->s[k] = h_S[k];
  p->dist2 = dist_max * dist_max;
  p->cos_min = cos_min;
  p->wd = (double)cam->width, p->hd = (double)cam->height;
  p->width = cam->width;
  p->n_px = cam->width * cam->height;
  return R3D_OK;
}

// the caller's device outputs against the input maps and against each other
int output_checks(const TrackParams& p, const Maps& m, const r3d_range* outs, int n_outs) {
  const size_t map = (size_t)p.n_px * 12;
  const r3d_range ins[6] = {{m.src_vertex, map},   {m.src_normal, map},                   {m.model_vertex, map},
                            {m.model_normal, map}, {m.src_intensity, (size_t)p.n_px * 4}, {m.model_packed, (size_t)p.n_px * 16}};
  for (int a = 0; a < n_outs; ++a) {   // output by output, so that the first offender decides which of the two messages it is
    R3D_REQUIRE(!r3d_any_overlap(outs + a, 1, ins, 6), "an output overlaps an input map");
    R3D_REQUIRE(!r3d_any_overlap(outs + a, 1, outs + a + 1, n_outs - a - 1), "outputs overlap each other");
  }
  return R3D_OK;
}

int n_tiles(const TrackParams& p) { return (p.n_px + kTile - 1) / kTile; }

// partial rows (+ one row for the sums) in kWsPartials, where the other paths keep their partial rows
int rows_workspace(r3d_ctx* ctx, int tiles, double** rows, int k_sums = kSums) {
  void* v = nullptr;
  int rc = r3d_scratch(ctx, kWsPartials, ((size_t)tiles + 2) * k_sums * sizeof(double), &v);
  if (rc) return rc;
  *rows = static_cast<double*>(v);
  return R3D_OK;
}

template <bool kRgb>
void launch_pass(r3d_ctx* ctx, const TrackParams& p, const PhotoParams& ph, const Maps& m, const double* d_state_in, double* rows,
                 double* d_sums_out, double* d_state, int32_t* d_match_out, float* d_residual_out, float* d_photo_out) {
  const int tiles = n_tiles(p);
  hipLaunchKernelGGL(track_kernel<kRgb>, dim3(tiles), dim3(kThreads), 0, ctx->stream, m.src_vertex, m.src_normal, m.model_vertex,
                     m.model_normal, m.src_intensity, reinterpret_cast<const float4*>(m.model_packed), p, ph, d_state_in, rows,
                     d_match_out, d_residual_out, d_photo_out);
  hipLaunchKernelGGL(r3d_plane::plane_finish_kernel<kRgb ? kSumsRgb : kSums>, dim3(1), dim3(kThreads), 0, ctx->stream,
                     (const double*)rows, tiles, d_sums_out, d_state);
}

// one pass on the stream: association + sums, then the finish (and, with a state, the solve).  ph: the colour term's parameters, or
// NULL for the pass without it (29 sums per row instead of 31, no photo output)
void enqueue_pass(r3d_ctx* ctx, const TrackParams& p, const PhotoParams* ph, const Maps& m, const double* d_state_in, double* rows,
                  double* d_sums_out, double* d_state, int32_t* d_match_out, float* d_residual_out, float* d_photo_out) {
  if (ph)
    launch_pass<true>(ctx, p, *ph, m, d_state_in, rows, d_sums_out, d_state, d_match_out, d_residual_out, d_photo_out);
  else
    launch_pass<false>(ctx, p, PhotoParams{}, m, d_state_in, rows, d_sums_out, d_state, d_match_out, d_residual_out, nullptr);
}

// n_iters passes on one state.  With the colour term every pass leaves its 31 sums in the row after the partial rows: the last
// pass's photometric count and sum are read from there (*d_sums_out); without it no pass writes its sums anywhere.
int iterate_impl(r3d_ctx* ctx, const TrackParams& p, const PhotoParams* ph, const Maps& m, int n_iters, double* d_state,
                 double** d_sums_out = nullptr) {
  double* rows = nullptr;
  const int tiles = n_tiles(p), k_sums = ph ? kSumsRgb : kSums;
  int rc = rows_workspace(ctx, tiles, &rows, k_sums);
  if (rc) return rc;
  double* d_sums = ph ? rows + (size_t)tiles * k_sums : nullptr;
  for (int it = 0; it < n_iters; ++it) enqueue_pass(ctx, p, ph, m, d_state, rows, d_sums, d_state, nullptr, nullptr, nullptr);
  R3D_HIP(hipGetLastError());
  if (d_sums_out) *d_sums_out = d_sums;
  return R3D_OK;
}

// r3d_track_accumulate and _accumulate_rgb (rgb: m carries the two intensity maps): one pass from the identity, its sums to the host
int accumulate_entry(r3d_ctx* ctx, const r3d_camera* cam, const Maps& m, const double* h_model_pose_w2c, const double* h_S, double dist_max,
                     double cos_min, bool rgb, double w_photo, double i_max, double* h_sums, int32_t* d_match_out, float* d_residual_out,
                     float* d_photo_out) {
  TrackParams p;
  PhotoParams ph;
  int rc = track_checks(ctx, cam, m, h_model_pose_w2c, h_S, dist_max, cos_min, &p);
  if (rc) return rc;
  if (rgb && (rc = photo_checks(m, w_photo, i_max, &ph))) return rc;
  R3D_REQUIRE(h_sums != nullptr, "h_sums is NULL");
  const size_t plane = (size_t)p.n_px * 4;
  const r3d_range outs[3] = {{d_match_out, plane}, {d_residual_out, plane}, {d_photo_out, plane}};
  if ((rc = output_checks(p, m, outs, 3))) return rc;
  if ((rc = r3d_ctx_enter(ctx))) return rc;
  double* rows = nullptr;
  const int tiles = n_tiles(p), k_sums = rgb ? kSumsRgb : kSums;
  if ((rc = rows_workspace(ctx, tiles, &rows, k_sums))) return rc;
  for (int a = 0; a < 3; ++a)
    if (outs[a].p) r3d_wrote(ctx, outs[a].p, outs[a].bytes);
  double* d_sums = rows + (size_t)tiles * k_sums;
  enqueue_pass(ctx, p, rgb ? &ph : nullptr, m, nullptr, rows, d_sums, nullptr, d_match_out, d_residual_out, d_photo_out);
  R3D_HIP(hipGetLastError());
  R3D_HIP(hipMemcpyAsync(h_sums, d_sums, k_sums * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
  R3D_HIP(hipStreamSynchronize(ctx->stream));
  return R3D_OK;
}

constexpr int kMaxIters = R3D_ICP_STATE_DOUBLES - R3D_ICP_STATE_HISTORY;   // what the history holds

// r3d_track_iterate and _iterate_rgb: n_iters passes on the caller's state
int iterate_entry(r3d_ctx* ctx, const r3d_camera* cam, const Maps& m, const double* h_model_pose_w2c, const double* h_S, double dist_max,
                  double cos_min, bool rgb, double w_photo, double i_max, int n_iters, double* d_state) {
  TrackParams p;
  PhotoParams ph;
  int rc = track_checks(ctx, cam, m, h_model_pose_w2c, h_S, dist_max, cos_min, &p);
  if (rc) return rc;
  if (rgb && (rc = photo_checks(m, w_photo, i_max, &ph))) return rc;
  R3D_REQUIRE(d_state != nullptr, "d_state is NULL");
  R3D_REQUIRE(n_iters >= 0 && n_iters <= kMaxIters, "n_iters must be in [0, %d]", kMaxIters);
  const r3d_range out = {d_state, R3D_ICP_STATE_DOUBLES * sizeof(double)};
  if ((rc = output_checks(p, m, &out, 1))) return rc;
  if ((rc = r3d_ctx_enter(ctx))) return rc;
  if (n_iters == 0) return R3D_OK;
  r3d_wrote(ctx, d_state, out.bytes);
  return iterate_impl(ctx, p, rgb ? &ph : nullptr, m, n_iters, d_state);
}

// The whole-frame drivers' host arguments: the finite guess G (world -> camera, 12 doubles) and S = its inverse, in double: the
// transposed rotation and C_k = -((R[0][k] t0 + R[1][k] t1) + R[2][k] t2)
int guess_inverse(const double* G, double S[16]) {
  for (int k = 0; k < 12; ++k) R3D_REQUIRE(std::isfinite(G[k]), "the pose guess must be finite");
  for (int a = 0; a < 3; ++a) {
    for (int b = 0; b < 3; ++b) S[4 * a + b] = G[3 * b + a];
    S[4 * a + 3] = -((G[a] * G[9] + G[3 + a] * G[10]) + G[6 + a] * G[11]);
    S[12 + a] = 0.0;
  }
  S[15] = 1.0;
  return R3D_OK;
}

// ... their outputs: the pose row and the info cannot overlap each other or the guess
int frame_output_checks(const double* G, const double* h_pose_out, const double* h_info_out, int n_info, float max_jump) {
  R3D_REQUIRE(h_pose_out && h_info_out, "NULL output pointer");
  const r3d_range outs[2] = {{h_pose_out, 12 * sizeof(double)}, {h_info_out, (size_t)n_info * sizeof(double)}};
  const r3d_range in = {G, 12 * sizeof(double)};
  R3D_REQUIRE(!r3d_any_overlap(outs, 2, &in, 1), "an output overlaps the guess or the other output");
  R3D_REQUIRE(max_jump >= 0.f, "max_jump must be >= 0");
  return R3D_OK;
}

// ... and what they make of the state they read back (st: its first kStatePairs + 1 doubles): T_total . S -> the world-to-camera
// row, or the guess as it was given after a degenerate step, and info[0..3] = pairs, rms, status, iterations
void pose_and_info(const double* st, const double* G, const double* S, double* h_pose_out, double* h_info_out) {
  const bool bad = st[r3d_sums::kStateStatus] != 0.0;
  if (bad) {
    for (int k = 0; k < 12; ++k) h_pose_out[k] = G[k];
  } else {
    double M[16];
    for (int r = 0; r < 4; ++r)
      for (int cc = 0; cc < 4; ++cc) {
        double v = 0.0;
        for (int k = 0; k < 4; ++k) v += st[r3d_sums::kStateTTotal + 4 * r + k] * S[4 * k + cc];
        M[4 * r + cc] = v;
      }
    for (int a = 0; a < 3; ++a) {
      for (int b = 0; b < 3; ++b) h_pose_out[3 * a + b] = M[4 * b + a];
      h_pose_out[9 + a] = -((M[a] * M[3] + M[4 + a] * M[7]) + M[8 + a] * M[11]);
    }
  }
  h_info_out[0] = st[r3d_sums::kStatePairs];
  h_info_out[1] = st[r3d_sums::kStateRms];
  h_info_out[2] = bad ? 1.0 : 0.0;
  h_info_out[3] = st[r3d_sums::kStateIters];
}

// The whole step for one frame with the colour term, one level ("TSDF colour tracking"): track_levels' one-level case with the
// model's colour image ray-cast next to its maps and the two intensity maps made of it and of the frame's image.  The two stay two
// drivers: this one's ray cast, its two intensity maps, its workspace layout and its six-entry info would each be a flag in the other.
int track_rgb(r3d_tsdf* vol, const r3d_camera* cam, const void* d_depth, int depth_dtype, double depth_scale, const uint8_t* d_rgb,
              const double* h_pose_guess_w2c, double min_weight, double step, double t_near, double t_far, float max_jump, double dist_max,
              double cos_min, double w_photo, double i_max, int n_iters, double* h_pose_out, double* h_info_out) {
  int rc = r3d_tsdf_integrate_checks(vol, cam, d_depth, depth_dtype, 1, depth_scale, h_pose_guess_w2c);
  if (rc) return rc;
  R3D_REQUIRE(d_rgb != nullptr, "d_rgb is NULL");
  const double* G = h_pose_guess_w2c;
  if ((rc = frame_output_checks(G, h_pose_out, h_info_out, 6, max_jump))) return rc;
  R3D_REQUIRE(n_iters >= 0 && n_iters <= kMaxIters, "n_iters must be in [0, %d]", kMaxIters);
  r3d_ctx* ctx = cam->ctx;
  double S[16];
  if ((rc = guess_inverse(G, S))) return rc;
  const bool gate = cos_min > -1.0;
  TrackParams p;
  PhotoParams ph;
  const float dummy = 0.f;
  alignas(16) const float dummy4[4] = {0.f, 0.f, 0.f, 0.f};
  Maps probe = {&dummy, nullptr, &dummy, &dummy};
  probe.src_intensity = &dummy, probe.model_packed = dummy4;
  if ((rc = track_checks(ctx, cam, probe, G, S, dist_max, cos_min, &p))) return rc;
  if ((rc = photo_checks(probe, w_photo, i_max, &ph))) return rc;
  // the ray cast's own argument checks and the colour plane's presence: with no output it validates and does nothing else
  if ((rc = r3d_tsdf_raycast_rgb(vol, cam, 1, G, min_weight, step, t_near, t_far, nullptr, nullptr, nullptr, nullptr))) return rc;
  if ((rc = r3d_ctx_enter(ctx))) return rc;
  // kWsTrack: four vertex / normal maps, the model's packed intensity map (float4 loads), its depth, the source intensity,
  // the model's colour image and the ICP state
  const size_t n = (size_t)p.n_px;
  r3d_carve ws;
  const auto model_vertex_h = ws.take<float>(n * 3), model_normal_h = ws.take<float>(n * 3);
  const auto src_vertex_h = ws.take<float>(n * 3), src_normal_h = ws.take<float>(n * 3);
  const auto model_packed_h = ws.take<float>(n * 4), model_depth_h = ws.take<float>(n), src_intensity_h = ws.take<float>(n);
  const auto model_rgb_h = ws.take<uint8_t>(n * 3);
  const auto state_h = ws.take<double>(R3D_ICP_STATE_DOUBLES);
  if ((rc = r3d_scratch(ctx, kWsTrack, ws))) return rc;
  float *model_vertex = ws.at(model_vertex_h), *model_normal = ws.at(model_normal_h);
  float *src_vertex = ws.at(src_vertex_h), *src_normal = ws.at(src_normal_h);
  float *model_packed = ws.at(model_packed_h), *model_depth = ws.at(model_depth_h), *src_intensity = ws.at(src_intensity_h);
  uint8_t* model_rgb = ws.at(model_rgb_h);
  double* d_state = ws.at(state_h);
  if ((rc = r3d_tsdf_raycast_rgb(vol, cam, 1, G, min_weight, step, t_near, t_far, model_depth, model_vertex, model_normal, model_rgb)))
    return rc;
  if ((rc = r3d_intensity_map(ctx, model_rgb, model_depth, 1, cam->height, cam->width, max_jump, nullptr, model_packed))) return rc;
  if ((rc = r3d_unproject(ctx, cam, d_depth, depth_dtype, 1, depth_scale, src_vertex, R3D_F32))) return rc;
  if ((rc = r3d_intensity_map(ctx, d_rgb, src_vertex + 2, 3, cam->height, cam->width, max_jump, src_intensity, nullptr))) return rc;
  if (gate && (rc = r3d_normals_organized(ctx, src_vertex, 1, cam->height, cam->width, max_jump, nullptr, src_normal))) return rc;
  Maps m = {src_vertex, gate ? src_normal : nullptr, model_vertex, model_normal};
  m.src_intensity = src_intensity, m.model_packed = model_packed;
  if ((rc = r3d_icp_state_reset(ctx, d_state))) return rc;
  double* d_sums = nullptr;
  if (n_iters > 0 && (rc = iterate_impl(ctx, p, &ph, m, n_iters, d_state, &d_sums))) return rc;
  double st[r3d_sums::kStatePairs + 1], sums[kSumsRgb] = {0.0};
  R3D_HIP(hipMemcpyAsync(st, d_state, sizeof(st), hipMemcpyDeviceToHost, ctx->stream));
  if (d_sums) R3D_HIP(hipMemcpyAsync(sums, d_sums, sizeof(sums), hipMemcpyDeviceToHost, ctx->stream));
  R3D_HIP(hipStreamSynchronize(ctx->stream));
  pose_and_info(st, G, S, h_pose_out, h_info_out);
  h_info_out[4] = sums[kSums];
  h_info_out[5] = sums[kSums] > 0.0 ? std::sqrt(sums[kSums + 1] / sums[kSums]) : 0.0;
  return R3D_OK;
}

// The whole step for one frame over n_levels pyramid levels, fine (0) to coarse; r3d_tsdf_track is the one-level case.  The
// caller has checked that cams and iters hold n_levels entries (cams[0] may still be NULL: the volume's checks refuse it).
int track_levels(r3d_tsdf* vol, const r3d_camera* const* cams, int n_levels, const int* iters, const void* d_depth, int depth_dtype,
                 double depth_scale, const double* h_pose_guess_w2c, double min_weight, double step, double t_near, double t_far,
                 float max_jump, double dist_max, double cos_min, double* h_pose_out, double* h_info_out, double* h_rms_out) {
  int rc = r3d_tsdf_integrate_checks(vol, cams[0], d_depth, depth_dtype, 1, depth_scale, h_pose_guess_w2c);
  if (rc) return rc;
  const double* G = h_pose_guess_w2c;
  if ((rc = frame_output_checks(G, h_pose_out, h_info_out, 4, max_jump))) return rc;
  int64_t total = 0;
  for (int l = 0; l < n_levels; ++l) {
    R3D_REQUIRE(iters[l] >= 0, "the iteration count of level %d is negative", l);
    total += iters[l];
  }
  R3D_REQUIRE(total <= kMaxIters, "the iteration counts must add up to at most %d", kMaxIters);
  if (h_rms_out) {
    const size_t rms_bytes = (size_t)total * sizeof(double);
    R3D_REQUIRE(!r3d_ranges_overlap(h_rms_out, rms_bytes, h_pose_out, 12 * sizeof(double)) &&
                    !r3d_ranges_overlap(h_rms_out, rms_bytes, h_info_out, 4 * sizeof(double)) &&
                    !r3d_ranges_overlap(h_rms_out, rms_bytes, h_pose_guess_w2c, 12 * sizeof(double)) &&
                    !r3d_ranges_overlap(h_rms_out, rms_bytes, iters, (size_t)n_levels * sizeof(int)) &&
                    !r3d_ranges_overlap(h_rms_out, rms_bytes, cams, (size_t)n_levels * sizeof(*cams)),
                "h_rms_out overlaps another host argument");
  }
  r3d_ctx* ctx = cams[0]->ctx;
  double S[16];
  if ((rc = guess_inverse(G, S))) return rc;
  const bool gate = cos_min > -1.0;   // -1 admits every angle: the source normals are neither computed nor asked for
  TrackParams p[R3D_TRACK_MAX_LEVELS];
  for (int l = 0; l < n_levels; ++l) {   // the checks that need no buffer, before anything is enqueued
    R3D_REQUIRE(cams[l] != nullptr, "the camera of level %d is NULL", l);
    if (l > 0)
      R3D_REQUIRE(cams[l]->height == cams[l - 1]->height >> 1 && cams[l]->width == cams[l - 1]->width >> 1,
                  "the camera of level %d is %d x %d, half of level %d's %d x %d is %d x %d", l, cams[l]->height, cams[l]->width, l - 1,
                  cams[l - 1]->height, cams[l - 1]->width, cams[l - 1]->height >> 1, cams[l - 1]->width >> 1);
    const float dummy = 0.f;
    const Maps probe = {&dummy, nullptr, &dummy, &dummy};
    if ((rc = track_checks(ctx, cams[l], probe, G, S, dist_max, cos_min, &p[l]))) return rc;
    // the ray cast's own argument checks, before anything is reserved: with no output it validates and does nothing else
    if ((rc = r3d_tsdf_raycast(vol, cams[l], 1, G, min_weight, step, t_near, t_far, nullptr, nullptr, nullptr))) return rc;
  }
  if ((rc = r3d_ctx_enter(ctx))) return rc;
  // every level's four maps, the depth rasters of the levels above 0 and the state: kWsTrack (the rank-trimming residuals'
  // workspace too; nothing of that path runs in here).  A level has a quarter of the pixels of the one below: 4/3 of level 0's maps.
  r3d_carve ws;
  r3d_carve::piece<float> maps[R3D_TRACK_MAX_LEVELS][4], depth[R3D_TRACK_MAX_LEVELS];   // model vertex, model normal, source vertex, source normal
  for (int l = 0; l < n_levels; ++l)
    for (auto& map : maps[l]) map = ws.take<float>((size_t)p[l].n_px * 3);
  for (int l = 1; l < n_levels; ++l) depth[l] = ws.take<float>((size_t)p[l].n_px);
  const auto state_h = ws.take<double>(R3D_ICP_STATE_DOUBLES);
  if ((rc = r3d_scratch(ctx, kWsTrack, ws))) return rc;
  double* d_state = ws.at(state_h);
  double* rows = nullptr;
  if ((rc = rows_workspace(ctx, n_tiles(p[0]), &rows))) return rc;   // the largest level's rows: kWsPartials never grows mid-loop
  Maps m[R3D_TRACK_MAX_LEVELS];
  for (int l = 0; l < n_levels; ++l) {
    float *model_vertex = ws.at(maps[l][0]), *model_normal = ws.at(maps[l][1]);
    float *src_vertex = ws.at(maps[l][2]), *src_normal = ws.at(maps[l][3]);
    const bool used = iters[l] > 0;
    if (used && (rc = r3d_tsdf_raycast(vol, cams[l], 1, G, min_weight, step, t_near, t_far, nullptr, model_vertex, model_normal)))
      return rc;
    if (l == 0) {
      if ((rc = r3d_unproject(ctx, cams[0], d_depth, depth_dtype, 1, depth_scale, src_vertex, R3D_F32))) return rc;
    } else {
      // the depth of the level below: level 0's is the z column of its vertex map, whatever dtype the frame came in
      float* d = ws.at(depth[l]);
      const float* below = l == 1 ? m[0].src_vertex + 2 : ws.at(depth[l - 1]);
      if ((rc = r3d_depth_half(ctx, below, l == 1 ? 3 : 1, cams[l - 1]->height, cams[l - 1]->width, max_jump, d))) return rc;
      if (used && (rc = r3d_unproject(ctx, cams[l], d, R3D_DEPTH_F32, 1, 1.0, src_vertex, R3D_F32))) return rc;
    }
    if (used && gate && (rc = r3d_normals_organized(ctx, src_vertex, 1, cams[l]->height, cams[l]->width, max_jump, nullptr, src_normal)))
      return rc;
    m[l] = {src_vertex, gate ? src_normal : nullptr, model_vertex, model_normal};
  }
  if ((rc = r3d_icp_state_reset(ctx, d_state))) return rc;
  for (int l = n_levels - 1; l >= 0; --l)   // coarse to fine on the one state: T_total, the count and the rms history carry over
    if (iters[l] > 0 && (rc = iterate_impl(ctx, p[l], nullptr, m[l], iters[l], d_state))) return rc;
  double st[R3D_ICP_STATE_DOUBLES];
  const size_t n_read = h_rms_out ? (size_t)R3D_ICP_STATE_HISTORY + (size_t)total : (size_t)r3d_sums::kStatePairs + 1;
  R3D_HIP(hipMemcpyAsync(st, d_state, n_read * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
  R3D_HIP(hipStreamSynchronize(ctx->stream));
  pose_and_info(st, G, S, h_pose_out, h_info_out);
  for (int64_t k = 0; h_rms_out && k < total; ++k) h_rms_out[k] = st[R3D_ICP_STATE_HISTORY + k];
  return R3D_OK;
}

}  // namespace

extern "C" {

int r3d_track_accumulate(r3d_ctx* ctx, const r3d_camera* cam, const float* d_src_vertex, const float* d_src_normal,
                         const float* d_model_vertex, const float* d_model_normal, const double* h_model_pose_w2c, const double* h_S,
                         double dist_max, double cos_min, double* h_sums, int32_t* d_match_out, float* d_residual_out) {
  const Maps m = {d_src_vertex, d_src_normal, d_model_vertex, d_model_normal};
  return accumulate_entry(ctx, cam, m, h_model_pose_w2c, h_S, dist_max, cos_min, false, 0.0, 0.0, h_sums, d_match_out, d_residual_out,
                          nullptr);
}

int r3d_track_iterate(r3d_ctx* ctx, const r3d_camera* cam, const float* d_src_vertex, const float* d_src_normal,
                      const float* d_model_vertex, const float* d_model_normal, const double* h_model_pose_w2c, const double* h_S,
                      double dist_max, double cos_min, int n_iters, double* d_state) {
  const Maps m = {d_src_vertex, d_src_normal, d_model_vertex, d_model_normal};
  return iterate_entry(ctx, cam, m, h_model_pose_w2c, h_S, dist_max, cos_min, false, 0.0, 0.0, n_iters, d_state);
}

int r3d_track_accumulate_rgb(r3d_ctx* ctx, const r3d_camera* cam, const float* d_src_vertex, const float* d_src_normal,
                             const float* d_model_vertex, const float* d_model_normal, const double* h_model_pose_w2c, const double* h_S,
                             double dist_max, double cos_min, const float* d_src_intensity, const float* d_model_packed, double w_photo,
                             double i_max, double* h_sums, int32_t* d_match_out, float* d_residual_out, float* d_photo_out) {
  Maps m = {d_src_vertex, d_src_normal, d_model_vertex, d_model_normal};
  m.src_intensity = d_src_intensity, m.model_packed = d_model_packed;
  return accumulate_entry(ctx, cam, m, h_model_pose_w2c, h_S, dist_max, cos_min, true, w_photo, i_max, h_sums, d_match_out, d_residual_out,
                          d_photo_out);
}

int r3d_track_iterate_rgb(r3d_ctx* ctx, const r3d_camera* cam, const float* d_src_vertex, const float* d_src_normal,
                          const float* d_model_vertex, const float* d_model_normal, const double* h_model_pose_w2c, const double* h_S,
                          double dist_max, double cos_min, const float* d_src_intensity, const float* d_model_packed, double w_photo,
                          double i_max, int n_iters, double* d_state) {
  Maps m = {d_src_vertex, d_src_normal, d_model_vertex, d_model_normal};
  m.src_intensity = d_src_intensity, m.model_packed = d_model_packed;
  return iterate_entry(ctx, cam, m, h_model_pose_w2c, h_S, dist_max, cos_min, true, w_photo, i_max, n_iters, d_state);
}

int r3d_tsdf_track_rgb(r3d_tsdf* vol, const r3d_camera* cam, const void* d_depth, int depth_dtype, double depth_scale,
                       const uint8_t* d_rgb, const double* h_pose_guess_w2c, double min_weight, double step, double t_near, double t_far,
                       float max_jump, double dist_max, double cos_min, double w_photo, double i_max, int n_iters, double* h_pose_out,
                       double* h_info_out) {
  return track_rgb(vol, cam, d_depth, depth_dtype, depth_scale, d_rgb, h_pose_guess_w2c, min_weight, step, t_near, t_far, max_jump,
                   dist_max, cos_min, w_photo, i_max, n_iters, h_pose_out, h_info_out);
}

int r3d_tsdf_track(r3d_tsdf* vol, const r3d_camera* cam, const void* d_depth, int depth_dtype, double depth_scale,
                   const double* h_pose_guess_w2c, double min_weight, double step, double t_near, double t_far, float max_jump,
                   double dist_max, double cos_min, int n_iters, double* h_pose_out, double* h_info_out) {
  return track_levels(vol, &cam, 1, &n_iters, d_depth, depth_dtype, depth_scale, h_pose_guess_w2c, min_weight, step, t_near, t_far,
                      max_jump, dist_max, cos_min, h_pose_out, h_info_out, nullptr);
}

int r3d_tsdf_track_pyramid(r3d_tsdf* vol, const r3d_camera* const* cams, int n_levels, const int* h_iters, const void* d_depth,
                           int depth_dtype, double depth_scale, const double* h_pose_guess_w2c, double min_weight, double step,
                           double t_near, double t_far, float max_jump, double dist_max, double cos_min, double* h_pose_out,
                           double* h_info_out, double* h_rms_out) {
  R3D_REQUIRE(n_levels >= 1 && n_levels <= R3D_TRACK_MAX_LEVELS, "n_levels must be in [1, %d], got %d", R3D_TRACK_MAX_LEVELS, n_levels);
  R3D_REQUIRE(cams != nullptr && h_iters != nullptr, "NULL cams or h_iters");
  return track_levels(vol, cams, n_levels, h_iters, d_depth, depth_dtype, depth_scale, h_pose_guess_w2c, min_weight, step, t_near, t_far,
                      max_jump, dist_max, cos_min, h_pose_out, h_info_out, h_rms_out);
}

}  // extern "C"
