/*
 * r3d.h -- C ABI of libr3d_hip.so: the MI355X (gfx950) depth -> world point-cloud
 * fusion path.  This is the drop-in boundary: plain pointers and sizes, no C++ or
 * torch types.  A Python host binds it with ctypes; the
 * reference (rainfall1998/3D_reconstruction_system) has no FFI of its own, so each
 * entry point names the reference *function* whose arithmetic it replaces.
 *
 * Conventions
 *   - every function returns an int status: R3D_OK (0) or a negative R3D_ERR_*;
 *     r3d_last_error() returns a thread-local human-readable message for the last
 *     failure on the calling thread.  Nothing throws, nothing aborts.
 *   - "d_" pointers are device (HBM) addresses valid on the ctx's GPU; "h_" pointers
 *     are host addresses owned by the caller.  The library never frees caller memory.
 *   - device-pointer entry points are ASYNCHRONOUS on the ctx's HIP stream; *_host
 *     entry points are synchronous (H2D, kernel, D2H, stream sync).
 *   - one ctx = one GPU + one stream.  Calls on one ctx are not thread-safe; different
 *     ctxs are independent.  Objects created from a ctx (r3d_camera, r3d_voxelset, r3d_nn_index,
 *     r3d_dev_alloc / r3d_host_alloc memory) must not be USED after r3d_ctx_destroy; destroying
 *     them afterwards is allowed (their destroy functions do not touch the ctx).
 *   - point clouds are AoS xyz, row-major [n][3], float32 (R3D_F32) or float64
 *     (R3D_F64).  All arithmetic is done in fp64 registers in the reference's evaluation
 *     order -- products and differences exactly as written there; the 3-term dot products of the
 *     SE(3) / 4x4 apply are an fma chain fma(r2,dz, fma(r1,dy, r0*dx)) -- and rounded ONCE on
 *     store, so R3D_F32 output is the correctly rounded fp64 result (<= 6e-8 relative per
 *     component; f32 denormals kept on input and output: gradual underflow, ties to even,
 *     +-inf past FLT_MAX), R3D_F64 unprojection is bit-identical to the reference and R3D_F64 world
 *     points equal the reference's fp64 up to that dot-product's rounding (~1e-16 relative).
 */
#ifndef R3D_H
#define R3D_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define R3D_VERSION 200 /* 0.2.0 */

/* status codes */
#define R3D_OK 0
#define R3D_ERR_INVALID (-1)     /* bad argument (null pointer, negative size, unknown enum) */
#define R3D_ERR_HIP (-2)         /* a HIP runtime call failed; see r3d_last_error() */
#define R3D_ERR_NOMEM (-3)       /* device or host allocation failed */
#define R3D_ERR_NODEVICE (-4)    /* no usable gfx950 device / device index out of range */
#define R3D_ERR_UNSUPPORTED (-5) /* valid request the library does not implement */

/* depth raster element types (reference: uint8 from cv.imread(...,IMREAD_GRAYSCALE),
 * camera_to_world.py:160; u16 / f32 cover 16-bit PNG and metric depth rasters) */
#define R3D_DEPTH_U8 0
#define R3D_DEPTH_U16 1
#define R3D_DEPTH_F32 2

/* point-cloud element types */
#define R3D_F32 0
#define R3D_F64 1

typedef struct r3d_ctx r3d_ctx;       /* one GPU + one HIP stream + scratch buffers */
typedef struct r3d_camera r3d_camera; /* pinhole intrinsics + per-column/per-row ray tables in HBM */

/* ---- library / context ------------------------------------------------------------ */
int r3d_version(void);
const char* r3d_last_error(void);
int r3d_device_count(int* n_out);
/* flags = 0: the ctx creates and owns a non-blocking stream (`stream` is ignored).
 * flags & R3D_CTX_EXTERNAL_STREAM: launch on the caller's hipStream_t `stream` (e.g. torch's current
 * stream); NULL then means the device's default stream.  The ctx never destroys an external stream. */
#define R3D_CTX_EXTERNAL_STREAM 1
int r3d_ctx_create(int device, void* stream, int flags, r3d_ctx** ctx_out);
int r3d_ctx_destroy(r3d_ctx* ctx);
int r3d_ctx_sync(r3d_ctx* ctx);
int r3d_ctx_stream(r3d_ctx* ctx, void** stream_out);
/* tuning knobs (integers; 0 = auto everywhere): launch geometry only -- "fuse_blocks", "apply_blocks"
 * (workgroup counts), "nn_variant" (sources per lane of the NN sweeps: 1/2/4), "nn_warm" (0 auto: a presorted
 * index query with the same source / output buffers as the previous one starts from that one's matches as bounds, and the ICP
 * loops run their later iterations on the wave-local kernel; 1 off; 2 never the wave-local kernel; 3 always when there are bounds: A/B), "voxel_dedupe" (0 auto, 1 off, 2 on, 3 = the pre-round-3 form with the flush barrier inside its `if`: A/B only),
 * "fuse_prefetch" (0 auto, 1 off, 2 on: a read-only sweep stages a fused launch's inputs in the 256 MiB Infinity Cache first,
 * chunk by chunk -- "fuse_chunk_mb", 0 = 96 -- so that the kernel's reads do not mix with its write stream at the DRAM.  auto
 * stages BY PROVENANCE: a launch whose small-share inputs exceed "fuse_stage_auto_mb" (default 8) MB is staged unless those very
 * bytes are presumed to be in the cache already -- i.e. a launch of this library on this device read them and fewer than
 * "fuse_resident_mb" (default 128) MB of other inputs went through since.  r3d_memcpy_h2d / _d2d / r3d_memset, the *_host
 * pipeline's uploads, r3d_comm_allgather's receives and r3d_dev_free make the library forget the ranges they touch (measured:
 * a raster an H2D copy has just written runs at 0.49 of the HBM peak plain, 0.82 staged; staging a cached one costs 8 %).
 * A FOREIGN producer (torch, another library) that rewrites an input buffer in place says so with
 * r3d_ctx_set_tuning(ctx, "fuse_inputs_fresh", 1): an event, not a state -- nothing on the device is presumed cached any more;
 * reading the key back gives the number of ranges on record; "fuse_sweeps" counts the staging sweeps enqueued so far, one per
 * staged input chunk).  "fuse_stage_fold" (default 1): a staged launch of the f32-xyz kernel without colour reads its depth
 * chunk in its own first workgroups instead of a separate sweep launch in front; 0 = the separate sweep (A/B, escape hatch).
 * No knob changes any result bit.  Unknown key -> R3D_ERR_INVALID.  (Kernel A/B variants live in tools/ab_kernels.hip,
 * not in the library.) */
int r3d_ctx_set_tuning(r3d_ctx* ctx, const char* key, int value);
int r3d_ctx_get_tuning(r3d_ctx* ctx, const char* key, int* value_out);

/* Read-only sweep of a device buffer on the ctx stream: leaves (up to ~100 MB of) it in the 256 MiB Infinity Cache, so that a
 * write-heavy kernel enqueued next reads it from there instead of mixing reads into its HBM write stream (the fused kernels do
 * this themselves where it pays, see "fuse_prefetch" -- and they take a range swept here as cached).  Asynchronous; changes nothing. */
int r3d_cache_prefetch(r3d_ctx* ctx, const void* d_ptr, size_t bytes);

/* ---- device memory + timing helpers (so a ctypes host needs nothing but this library) */
int r3d_dev_alloc(r3d_ctx* ctx, size_t bytes, void** d_ptr_out);
int r3d_dev_free(r3d_ctx* ctx, void* d_ptr);
int r3d_memcpy_h2d(r3d_ctx* ctx, void* d_dst, const void* h_src, size_t bytes); /* async on ctx stream */
int r3d_memcpy_d2h(r3d_ctx* ctx, void* h_dst, const void* d_src, size_t bytes); /* async on ctx stream */
int r3d_memcpy_d2d(r3d_ctx* ctx, void* d_dst, const void* d_src, size_t bytes); /* async on ctx stream */
/* Synchronous device -> host copy that reaches the pinned PCIe rate into PAGEABLE memory (a NumPy array): 32 MiB chunks through
 * pinned staging buffers, the pageable copies spread over host threads (a plain copy runs at ~12 GB/s on this host).  Returns
 * when h_dst holds the data; everything enqueued on the ctx stream before it has completed by then. */
int r3d_download(r3d_ctx* ctx, void* h_dst, const void* d_src, size_t bytes);
int r3d_memset(r3d_ctx* ctx, void* d_dst, int byte_value, size_t bytes);
/* Pinned (page-locked) host memory.  The *_host entry points detect pinned buffers and DMA straight from/to them;
 * pageable buffers go through the library's own pinned staging ring with multi-threaded copies. */
int r3d_host_alloc(r3d_ctx* ctx, size_t bytes, void** h_ptr_out);
int r3d_host_free(r3d_ctx* ctx, void* h_ptr);
/* HIP-event stopwatch on the ctx's stream: start records an event, stop records a second
 * one, synchronises on it and returns the elapsed milliseconds between them. */
int r3d_timer_start(r3d_ctx* ctx);
int r3d_timer_stop(r3d_ctx* ctx, float* ms_out);

/* ---- camera (replaces the hard-coded fx,fy,cx,cy of pixel_to_camera.py:25-28 and
 * camera_to_world.py:68-71).  Builds u[i]=(i-cx)/fx, v[j]=(j-cy)/fy in fp64 on the host
 * with the reference's evaluation order and keeps them in HBM. */
int r3d_camera_create(r3d_ctx* ctx, int height, int width, double fx, double fy, double cx, double cy,
                      r3d_camera** cam_out);
int r3d_camera_destroy(r3d_camera* cam);


/* ---- a1/a2: per-pixel back-projection.  Replaces gentxtcord() (pixel_to_camera.py:24-44,
 * camera_to_world.py:67-83): Z=depth[j,i]*depth_scale, X=(i-cx)/fx*Z, Y=(j-cy)/fy*Z, row-major,
 * every pixel emitted, no masking.  n_frames rasters of cam's HxW -> [n_frames*H*W][3]. */
int r3d_unproject(r3d_ctx* ctx, const r3d_camera* cam, const void* d_depth, int depth_dtype, int n_frames,
                  double depth_scale, void* d_xyz_out, int out_dtype);
int r3d_unproject_host(r3d_ctx* ctx, const r3d_camera* cam, const void* h_depth, int depth_dtype, int n_frames,
                       double depth_scale, void* h_xyz_out, int out_dtype);

/* ---- a2+a3+a4 fused, batched: unproject + per-frame SE(3), frames concatenated in order.
 * Replaces the frame loop of get_file_name() (camera_to_world.py:149-172) =
 * gentxtcord (c2w:67-83) + get_pointdata/point_camera (c2w:86-105, 57-59):
 *     p_world = Rinv_f . (p_cam - t_f)
 * pose: n_frames x 12 doubles, [Rinv row-major (9), t (3)] per frame; Rinv is what
 * scipy_transfer() (c2w:53-55) returns -- computed on the host in fp64. */
int r3d_fuse_frames(r3d_ctx* ctx, const r3d_camera* cam, const void* d_depth, int depth_dtype, int n_frames,
                    double depth_scale, const double* d_pose, void* d_xyz_out, int out_dtype);
int r3d_fuse_frames_host(r3d_ctx* ctx, const r3d_camera* cam, const void* h_depth, int depth_dtype, int n_frames,
                         double depth_scale, const double* h_pose, void* h_xyz_out, int out_dtype);

/* f4 colour attach (genply_noRGB, pixel_to_camera.py:55-91; BASELINE config 5 "RGBD"): the same fused launch also
 * carries the frames' colour.  d_rgb: [n_frames][H][W][3] uint8, R,G,B per pixel (the image the depth raster belongs
 * to).  d_rgba_out: [n_frames*H*W] uint32 = r | g<<8 | b<<16, i.e. bytes R,G,B,0 -- the "R G B 0" of the reference's
 * PLY rows -- point k takes the colour of pixel k.  d_pose == NULL: camera-frame points (pixel_to_camera.py).
 * +7 B/point of HBM traffic (3 read, 4 written). */
int r3d_fuse_frames_rgb(r3d_ctx* ctx, const r3d_camera* cam, const void* d_depth, int depth_dtype, int n_frames,
                        double depth_scale, const double* d_pose, const unsigned char* d_rgb, void* d_xyz_out,
                        int out_dtype, uint32_t* d_rgba_out);
/* The same from / to host arrays (pageable or pinned): depth + colour stream in and xyz + rgba stream out chunk by chunk
 * through the library's pinned staging pipeline, both PCIe directions busy at once.  Synchronous. */
int r3d_fuse_frames_rgb_host(r3d_ctx* ctx, const r3d_camera* cam, const void* h_depth, int depth_dtype, int n_frames,
                             double depth_scale, const double* h_pose, const unsigned char* h_rgb, void* h_xyz_out,
                             int out_dtype, uint32_t* h_rgba_out);

/* f4, torch-facing: the BackprojectDepth layer the reference's trainer calls (monodepth2/trainer.py:150-160, 387-390;
 * upstream monodepth2 layers.py, not vendored by the reference):
 *     cam_points[b][c][p] = depth[b][p] * (inv_K[b][c][0]*x + inv_K[b][c][1]*y + inv_K[b][c][2]),  c = 0..2;  [b][3][p] = 1
 * with p = y*W + x, all fp32 like the layer.  d_depth [B][H*W], d_inv_K [B][4][4] row-major, d_cam_points [B][4][H*W].
 * The _grad entry point is the layer's backward with respect to depth: grad_depth[b][p] = sum_c grad_cam[b][c][p]*ray_c.
 * f32 evaluation order (the upstream layer's; one rounding per operation, no fused multiply-add, f32 denormals kept, x and y
 * converted exactly):
 *     ray_c = (k_c0*x + k_c1*y) + k_c2          cam_c = z * ray_c          the fourth plane is exactly 1.0f
 *     grad_depth = (g0*ray_0 + g1*ray_1) + g2*ray_2
 * Every per-pixel output of these four entry points is therefore specified bit for bit (NaN sign and payload excepted). */
int r3d_backproject_depth_f32(r3d_ctx* ctx, const float* d_depth, const float* d_inv_K, int batch, int height, int width,
                              float* d_cam_points);
int r3d_backproject_depth_grad_f32(r3d_ctx* ctx, const float* d_grad_cam_points, const float* d_inv_K, int batch, int height,
                                   int width, float* d_grad_depth);

/* Its partner in the same trainer lines, Project3D (trainer.py:150-160, 389-390; upstream layers.py):
 *     c = P[b] . points[b][:, p]   (P = (K @ T)[:, :3, :], [B][3][4] row-major, formed by the caller: sixteen numbers per image)
 *     pix[b][p] = ( (c0 / (c2 + eps) / (W-1) - 0.5) * 2,  (c1 / (c2 + eps) / (H-1) - 0.5) * 2 )        grid_sample coordinates
 * d_points [B][4][H*W] (the BackprojectDepth layout), d_pix [B][H][W][2], fp32; upstream eps = 1e-7.
 * The _grad entry point is the backward pass: d_grad_points [B][4][H*W] and/or d_grad_P [B][3][4] (either may be NULL);
 * d_grad_P is a two-stage fixed-order reduction (bitwise repeatable).
 * f32 evaluation order, with (px, py, pz, pw) = points[b][0..3][p] and g = grad_pix[b][p]:
 *     c_i = ((P_i0*px + P_i1*py) + P_i2*pz) + P_i3*pw          den = c2 + eps
 *     pix = ( ((c0/den)/(W-1) - 0.5) * 2,  ((c1/den)/(H-1) - 0.5) * 2 )          divisions correctly rounded, f32 denormals kept
 *     inv = 1/den      d0 = (g.x * (2/(W-1))) * inv      d1 = (g.y * (2/(H-1))) * inv      d2 = (-(d0*c0 + d1*c1)) * inv
 *     grad_points_k = (P_0k*d0 + P_1k*d1) + P_2k*d2,  k = 0..3          (2/(W-1), 2/(H-1): f32 quotients formed once)
 *     grad_P_ik = sum over the image's pixels of d_i * x_k; each term is one f32 product of the d_i above.  The order of the
 *     summation is build-defined and fixed: bitwise repeatable, independent of the other images of the batch, not specified.
 * H == 1 or W == 1 -> R3D_ERR_INVALID (BackprojectDepth accepts them); batch == 0 -> R3D_OK, nothing written;
 * batch > 65535, a NULL required pointer with batch > 0 -> R3D_ERR_INVALID, nothing written; both outputs of _grad NULL -> R3D_OK. */
int r3d_project3d_f32(r3d_ctx* ctx, const float* d_points, const float* d_P, int batch, int height, int width, float eps,
                      float* d_pix);
int r3d_project3d_grad_f32(r3d_ctx* ctx, const float* d_grad_pix, const float* d_points, const float* d_P, int batch,
                           int height, int width, float eps, float* d_grad_points, float* d_grad_P);

/* ---- a4 on an existing cloud: p_world = Rinv . (p_cam - t), the evaluation order of point_camera()
 * (camera_to_world.py:57-59) and of the fused kernel, so fuse_frames(depth) == se3_apply(unproject(depth))
 * bit for bit.  h_pose is ALWAYS a host pointer: 12 doubles [Rinv row-major (9), t (3)].  In-place allowed
 * (d_xyz_out == d_xyz_in, equal dtypes); any other overlap of the input and output ranges -> R3D_ERR_INVALID. */
int r3d_se3_apply(r3d_ctx* ctx, const void* d_xyz_in, int in_dtype, int64_t n_points, const double* h_pose,
                  void* d_xyz_out, int out_dtype);
int r3d_se3_apply_host(r3d_ctx* ctx, const void* h_xyz_in, int in_dtype, int64_t n_points, const double* h_pose,
                       void* h_xyz_out, int out_dtype);

/* ---- a7: p' = (T . [x,y,z,1]^T)[0:3] for a general row-major 4x4.
 * Replaces local_world(flag=True)/point_camera (transfer_T_icp.py:71-97, 10-12).
 * h_T is ALWAYS a host pointer (16 doubles); in-place (d_xyz_out == d_xyz_in, equal dtypes) is allowed; any other
 * overlap of the input and output ranges -> R3D_ERR_INVALID. */
int r3d_apply_T(r3d_ctx* ctx, const void* d_xyz_in, int in_dtype, int64_t n_points, const double* h_T,
                void* d_xyz_out, int out_dtype);
int r3d_apply_T_host(r3d_ctx* ctx, const void* h_xyz_in, int in_dtype, int64_t n_points, const double* h_T,
                     void* h_xyz_out, int out_dtype);

/* ---- a8: ICP estimation kernels (NOT in the reference -- transfer_T_icp.py only consumes a
 * T_data.txt made by an external tool; build-defined per SURVEY.md 8(a8)).
 * r3d_icp_nn: for each source point the index of the nearest target point under squared L2
 * computed in fp32 as d2 = fmaf(dz,dz, fmaf(dy,dy, dx*dx)) with dx = sx-tx, dy = sy-ty, dz = sz-tz (one rounding
 * for dx*dx, one per fused multiply-add; no other contraction; f32 denormals kept: a subnormal d2 ranks as its value, not as 0),
 * lowest index wins exact ties.  This expression IS
 * the specification: brute force, culled index and oracle all evaluate exactly it.
 * Non-finite input: a pair whose d2 is NaN or +inf never wins; a source with no finite d2 at all (it, or every target,
 * has a NaN / inf coordinate) gets index 0 and d2 = +inf; the pair sums leave rows with non-finite coordinates out.
 * src/tgt are float32 xyz AoS.  d_idx_out [n_src] uint32, d_d2_out [n_src] float32 (may be NULL). */
int r3d_icp_nn(r3d_ctx* ctx, const float* d_src, int64_t n_src, const float* d_tgt, int64_t n_tgt,
               uint32_t* d_idx_out, float* d_d2_out);
int r3d_icp_nn_host(r3d_ctx* ctx, const float* h_src, int64_t n_src, const float* h_tgt, int64_t n_tgt,
                    uint32_t* h_idx_out, float* h_d2_out);
/* The same answer as r3d_icp_nn with spatial culling: the target cloud is Morton-sorted once into 1024-point tiles
 * with bounding boxes; a query sorts its sources the same way and sweeps only tiles whose box can still hold a
 * closer point.  Exactness is kept: identical fp32 distance expression, lowest original target index on ties
 * (a source that meets its minimum again in another group of targets looks through that group on the spot).  create and query
 * are asynchronous on the ctx stream
 * unless h_tiles_swept != NULL (then it synchronises and reports how many tile sweeps all workgroups did). */
typedef struct r3d_nn_index r3d_nn_index;
int r3d_nn_index_create(r3d_ctx* ctx, const float* d_tgt, int64_t n_tgt, r3d_nn_index** index_out);
int r3d_nn_index_destroy(r3d_nn_index* index);
/* presorted = 0: the call sorts a copy of the sources into index order itself (any source order is fine).
 * presorted = 1: the caller keeps the sources spatially coherent -- r3d_nn_index_sort_cloud once, then rigid /
 * similarity moves of the whole cloud (ICP) preserve it -- and the sort is skipped.  Results are the same either way
 * and always land at the source's position in d_src. */
int r3d_nn_index_query(r3d_nn_index* index, const float* d_src, int64_t n_src, uint32_t* d_idx_out, float* d_d2_out,
                       int presorted, int64_t* h_tiles_swept);
/* Permutes an xyz cloud in place into the index's Morton order; d_perm_out (optional, [n] uint32) receives the original
 * position of every row.  Asynchronous on the ctx stream. */
int r3d_nn_index_sort_cloud(r3d_nn_index* index, float* d_xyz, int64_t n_points, uint32_t* d_perm_out);
/* r3d_icp_accumulate: the 18 fp64 sums Umeyama needs over the matched pairs (p=src[k], q=tgt[idx[k]]),
 * pairs with d2 > max_d2 skipped when max_d2 >= 0 (d_d2 may be NULL when max_d2 < 0):
 *   sums[0]=n, [1..3]=sum p, [4..6]=sum q, [7..15]=sum p_a*q_b (a major), [16]=sum |p|^2, [17]=sum |q|^2.
 * Deterministic (fixed two-stage tree, no float atomics).  h_sums is a host pointer; synchronous.
 * Pairs whose idx[k] >= n_tgt are skipped (the index array is data; the kernel never reads past the target cloud), and so
 * are pairs in which p or q has a NaN / inf coordinate (in every sums pass of this library, fused ones included). */
int r3d_icp_accumulate(r3d_ctx* ctx, const float* d_src, int64_t n_src, const float* d_tgt, int64_t n_tgt,
                       const uint32_t* d_idx, const float* d_d2, float max_d2, double* h_sums);

/* Closed-form similarity from the 18 sums (Umeyama 1991): h_T (16 doubles, row-major 4x4) = [sR t; 0 1] minimising
 * sum w |q - (sRp + t)|^2; with_scale = 0 pins s = 1.  h_rms_out (optional) = sqrt(sum w|p-q|^2 / sum w) before the
 * step.  Pure host arithmetic (3x3 one-sided Jacobi SVD, fp64), no GPU needed -- and the very code the device-side
 * solve runs.  R3D_ERR_INVALID (h_T = identity) when the fit is undefined: weight sum < 3, no spread, or sums -- a NaN / inf
 * among them -- from which no finite T follows. */
int r3d_umeyama_from_sums(const double* h_sums, int with_scale, double* h_T, double* h_rms_out);
/* Device-resident ICP state: R3D_ICP_STATE_DOUBLES doubles in HBM.
 *   [0..15] T_total (row-major 4x4, maps the ORIGINAL source onto the target), [16..31] the last step,
 *   [32] steps solved, [33] status (1 = some step was degenerate and skipped), [34] rms seen by the last step,
 *   [35] its weight sum, [36..47] reserved (zero after a reset, never written), [48+k] rms seen by step k for k < 464.
 * A degenerate step counts like any other: [32] goes up, its rms and weight go to [34] / [35] and its rms into the history;
 * the step is the identity, T_total keeps its bits, and [33] stays 1 until the next reset (later good steps still compose
 * onto T_total).  r3d_icp_iterate and r3d_icp_iterate_plane take any number of steps: past 464 the history is full and is
 * left as it is while [32], [34] and [35] go on ([32] is then larger than the number of history entries);
 * r3d_track_iterate refuses a call of more than 464 iterations. */
#define R3D_ICP_STATE_DOUBLES 512
#define R3D_ICP_STATE_HISTORY 48
int r3d_icp_state_reset(r3d_ctx* ctx, double* d_state);
/* n_iters whole ICP iterations enqueued back to back with NO host round trip: nearest neighbours (+ fused sums) ->
 * device solve -> source cloud moved in place by the step (r3d_apply_T_dev).  index != NULL: culled exact NN, d_src must
 * be in the index's order (r3d_nn_index_sort_cloud; similarity moves preserve it); index == NULL: brute force against
 * d_tgt.  The host reads d_state whenever it wants to look at the rms history / convergence. */
int r3d_icp_iterate(r3d_ctx* ctx, r3d_nn_index* index, float* d_src, int64_t n_src, const float* d_tgt, int64_t n_tgt,
                    uint32_t* d_idx, float* d_d2, int n_iters, int with_scale, float max_d2, double* d_state);

/* ---- a8 continued: RIGID POINT-TO-PLANE registration of two partially overlapping single-view clouds -- the reference's
 * own use of ICP ("match the point clouds corresponding to two images", readme.md:25; transfer_T_icp.py:107-108 merges the
 * camera clouds ./point/0.txt and ./point/24.txt with the T this produces).  Build-defined; this text is the specification.
 *
 * r3d_normals_organized: unit normals of an ORGANISED cloud [n_frames][height][width][3] f32 -- the row-major raster order
 * gentxtcord emits (pixel_to_camera.py:34-44).  For an interior pixel: a = p[j][i+1] - p[j][i-1], b = p[j+1][i] - p[j-1][i],
 * n = a x b normalised (fp64 throughout, rounded once to f32), turned towards the viewpoint (h_viewpoint, 3 doubles; NULL =
 * the origin, i.e. a camera-frame cloud).  The zero vector ("no plane here") is written for raster-border pixels, when the
 * centre or a neighbour is non-finite or AT the viewpoint (Z = 0 pixels: the reference emits every pixel, p2c:24-44), when a
 * neighbour's range differs from the centre's by more than max_jump x that range (a depth edge), and when a x b vanishes. */
int r3d_normals_organized(r3d_ctx* ctx, const float* d_xyz, int64_t n_frames, int height, int width, float max_jump,
                          const double* h_viewpoint, float* d_normals_out);
/* n_iters whole point-to-plane iterations with NO host round trip: culled exact NN (d_src in the index's order,
 * r3d_nn_index_sort_cloud; rigid moves preserve it) -> residuals + classes -> per-class selection -> 29 sums -> device solve
 * -> source moved.  d_tgt_normals: normals of the index's target cloud in its ORIGINAL order.  d_src_orig != NULL: the cloud
 * as it was when d_state was reset (same order as d_src); every iteration then writes d_src = T_total . d_src_orig (one
 * rounding per point however many steps were taken); NULL: d_src is moved in place step by step.  d_state: the
 * R3D_ICP_STATE_DOUBLES layout above ([34] / history = rms of r over the kept pairs).  Asynchronous. */
int r3d_icp_iterate_plane(r3d_ctx* ctx, r3d_nn_index* index, const float* d_src_orig, float* d_src, int64_t n_src,
                          const float* d_tgt_normals, uint32_t* d_idx, float* d_d2, int n_iters, float trim_q, float gate_scale,
                          float max_d2, double* d_state);

/* ---- (e) multi-GPU: one process per GPU, frames sharded in contiguous blocks (the frame loop of camera_to_world.py:149-172
 * carries no state between frames), ONE exchange step: an all-gather over RCCL / xGMI.  The reference has no
 * counterpart (single process, no collective); these entry points let a ctypes or plain-C host shard without torch.
 * librccl is dlopen'ed on first use (an RCCL already in the process is reused); without it they return
 * R3D_ERR_UNSUPPORTED.  All transfers are asynchronous on the ctx's stream. */
typedef struct r3d_comm r3d_comm;
#define R3D_COMM_ID_BYTES 128
/* rank 0 makes the id (ncclGetUniqueId) and hands the 128 bytes to every rank by any means (file, pipe, MPI, torch). */
int r3d_comm_unique_id(void* id_out);
/* collective over all ranks (ncclCommInitRank on the ctx's GPU); one GPU per rank. */
int r3d_comm_create(r3d_ctx* ctx, const void* id, int rank, int world, r3d_comm** comm_out);
int r3d_comm_destroy(r3d_comm* comm);
/* any out pointer may be NULL; *rccl_origin_out says which librccl was bound */
int r3d_comm_info(const r3d_comm* comm, int* rank_out, int* world_out, const char** rccl_origin_out);
/* What the communicator says about ITSELF: ncclCommCount / ncclCommUserRank / ncclCommCuDevice / ncclGetVersion (-1 where the
 * bound library lacks the call); any out pointer may be NULL. */
int r3d_comm_rccl_report(const r3d_comm* comm, int* count_out, int* user_rank_out, int* device_out, int* version_out);
/* All-gather of byte shards of possibly UNEQUAL length: rank r's h_counts[r] bytes land at offset sum(h_counts[0..r))
 * of d_recv on every rank (rank order = pose-file order).  d_send may already be this rank's slot of d_recv (in place).
 * algo: R3D_GATHER_AUTO (ncclAllGather when the shards are equal, else direct), R3D_GATHER_NCCL (equal shards only),
 * R3D_GATHER_DIRECT (one grouped ncclSend/ncclRecv per peer: each shard crosses its own xGMI link once). */
#define R3D_GATHER_AUTO 0
#define R3D_GATHER_NCCL 1
#define R3D_GATHER_DIRECT 2
int r3d_comm_allgather(r3d_comm* comm, const void* d_send, const int64_t* h_counts, void* d_recv, int algo);
/* "outputs" assembly: all-gather of the world-frame xyz shards (12 or 24 B/point over the fabric). */
int r3d_allgather_xyz(r3d_comm* comm, const void* d_shard, const int64_t* h_points_per_rank, int dtype, void* d_full,
                      int algo);
/* "inputs" assembly: all-gather of the depth rasters (+ pose rows when d_pose_all != NULL), 1-4 B/point over the fabric;
 * every rank then runs r3d_fuse_frames over all frames locally (same kernel, same bits as the xyz all-gather). */
int r3d_allgather_inputs(r3d_comm* comm, const void* d_depth, int depth_dtype, const int64_t* h_frames_per_rank, int height,
                         int width, const double* d_pose, void* d_depth_all, double* d_pose_all, int algo);
/* in-place sum over ranks (e.g. the 18 ICP sums of a sharded source cloud) */
int r3d_comm_allreduce_sum_f64(r3d_comm* comm, double* d_buf, int64_t n);

/* ---- f1: reference-layout ASCII serialisation on the host (multi-threaded C++).
 * r3d_format_ply: the byte layout of genply() (camera_to_world.py:112-134): header with 4-space
 * indents, "%.4f %.4f %.4f \n" rows, "\n    " trailer.  Two-call protocol: with h_buf == NULL
 * returns the exact byte count in *n_bytes_out; otherwise writes at most buf_cap bytes. */
int r3d_format_ply(const void* h_xyz, int dtype, int64_t n_points, char* h_buf, size_t buf_cap,
                   size_t* n_bytes_out);
/* Same bytes straight to a file (formatted and written in slabs; replaces the open/write of c2w:122-132). */
int r3d_write_ply(const char* path, const void* h_xyz, int dtype, int64_t n_points);
/* f1's optional binary flag: the same vertices as a STANDARD binary_little_endian PLY (float x, y, z; the header without the
 * reference template's indents).  12 bytes per vertex; not the reference's bytes -- an opt-in. */
int r3d_write_ply_binary(const char* path, const void* h_xyz, int dtype, int64_t n_points);
/* f4: the coloured layout of genply_noRGB() (pixel_to_camera.py:55-91): uchar red/green/blue/alpha header lines and
 * "%.4f %.4f %.4f R G B 0\n" rows; h_rgb is [n][3] uint8 in R,G,B order, point k takes colour k. */
int r3d_write_ply_rgb(const char* path, const void* h_xyz, int dtype, const unsigned char* h_rgb, int64_t n_points);
/* The same file from the rgba words r3d_fuse_frames_rgb produces ([n] uint32, bytes R,G,B,0 in memory). */
int r3d_write_ply_rgba(const char* path, const void* h_xyz, int dtype, const uint32_t* h_rgba, int64_t n_points);
/* "X,Y,Z\n" lines with Python repr() float formatting -- the camera / world txt of
 * camera_to_world.py:80-81, 103-104 and transfer_T_icp.py:87,93.  If h_z_raw != NULL the third column
 * is printed as that raw integer raster value (the reference's camera txt prints str(np.uint8));
 * z_raw_dtype is R3D_DEPTH_U8 or R3D_DEPTH_U16.  append: 0 truncates ('w'), 1 appends ('a'). */
int r3d_write_xyz_txt(const char* path, const void* h_xyz, int dtype, int64_t n_points, const void* h_z_raw,
                      int z_raw_dtype, int append);
/* One such file per frame -- the ./point/<stem>.txt that camera_to_world.py:163-165 leaves for every pose line: file k takes
 * points [k * points_per_file, (k + 1) * points_per_file) of h_xyz (and of h_z_raw).  Files are spread over the host threads
 * the process may use; same bytes as n_files calls of r3d_write_xyz_txt(..., append = 0). */
int r3d_write_xyz_txt_batch(const char* const* paths, int n_files, const void* h_xyz, int dtype, int64_t points_per_file,
                            const void* h_z_raw, int z_raw_dtype);
/* The same text into a caller buffer; two-call protocol like r3d_format_ply. */
int r3d_format_xyz_txt(const void* h_xyz, int dtype, int64_t n_points, const void* h_z_raw, int z_raw_dtype,
                       char* h_buf, size_t buf_cap, size_t* n_bytes_out);
/* The way back (f1: "a fast X,Y,Z parser"): rows of text -> [n][3] fp64 on host threads.  separator ',' reads the txt
 * lines above the way get_pointdata / local_world do (camera_to_world.py:92-98, transfer_T_icp.py:74-80): the first three
 * comma-separated fields of every non-blank line, extra fields ignored; separator ' ' reads blank-separated rows (the
 * body of the PLY layout).  Numbers are parsed correctly rounded (= Python float()).  h_xyz_out == NULL only counts.
 * A line that does not parse returns R3D_ERR_INVALID with its 1-based number in *bad_line_out (may be NULL). */
int r3d_parse_xyz_text(const char* h_text, size_t n_bytes, int separator, double* h_xyz_out, int64_t cap_points,
                       int64_t* n_points_out, int64_t* bad_line_out);

/* ---- f1 on the device: the same text formatted by the GPU (csrc/r3d_textfmt.hip), so that the TEXT leaves the device
 * (41 B/point of camera txt) instead of fp64 clouds into pageable memory, and the host only copies it into files.
 * kind R3D_TEXT_XYZ_TXT: the lines of r3d_write_xyz_txt (d_aux = the integer third column, u8 / u16 per aux_dtype, or NULL);
 * R3D_TEXT_PLY_ROWS: the vertex rows of r3d_write_ply ("%.4f %.4f %.4f \n", no header / trailer); R3D_TEXT_PLY_ROWS_RGB: the
 * rows of r3d_write_ply_rgb / _rgba (d_aux = colours, aux_dtype = 3 or 4 bytes apart).  Byte-identical to the host formatter.
 * d_xyz is a device [n][3] cloud; rows appear in point order in d_text (device, text_cap bytes).  Two-call protocol:
 * d_text == NULL only computes *n_bytes_out and the segment offsets.  segment_points > 0: h_segment_offsets_out
 * [ceil(n / segment_points) + 1] receives the byte offset of the first row of every block of segment_points points (a frame's
 * camera txt) and, last, the total.  Synchronises the ctx's stream once (the sizes come to the host); the rows themselves are
 * enqueued.  R3D_ERR_UNSUPPORTED when a "%.4f" coordinate has magnitude >= 2^40 (more digits than a device row holds): format
 * that cloud on the host. */
#define R3D_TEXT_XYZ_TXT 0
#define R3D_TEXT_PLY_ROWS 1
#define R3D_TEXT_PLY_ROWS_RGB 2
int r3d_format_text_device(r3d_ctx* ctx, int kind, const void* d_xyz, int dtype, int64_t n_points, const void* d_aux, int aux_dtype,
                           int64_t segment_points, char* d_text, size_t text_cap, int64_t* h_segment_offsets_out,
                           int64_t* n_bytes_out);
/* Device bytes -> files: file k = head (host bytes), then d_bytes[0 .. n_bytes) (device memory: text made by
 * r3d_format_text_device, or any other bytes -- the f32 cloud itself for a binary PLY), then tail (host bytes).
 * Host threads take the files largest first, each through its own pinned 1 MiB pieces and stream (PCIe and write() overlap);
 * one file is one sequential write stream, different files are written side by side.  Waits for the ctx's stream first. */
typedef struct r3d_text_file {
  const char* path;
  const char* head;
  size_t head_bytes;
  const void* d_bytes;
  size_t n_bytes;
  const char* tail;
  size_t tail_bytes;
} r3d_text_file;
int r3d_write_device_text_files(r3d_ctx* ctx, const r3d_text_file* files, int n_files);

/* ---- f3 ingestion: the depth rasters of camera_to_world.py:160 (`cv.imread(path, IMREAD_GRAYSCALE)`) decoded by host
 * threads.  Native path: non-interlaced greyscale PNG, 8 bits (-> uint8, same bytes as OpenCV) or 16 bits (-> uint16);
 * any other PNG flavour returns R3D_ERR_UNSUPPORTED (the Python host then falls back to cv2 / PIL).
 * r3d_png_gray_info: header only.  r3d_png_gray_decode_batch: n files of identical height x width x bit_depth into one
 * contiguous [n][height][width] buffer (pageable or pinned). */
int r3d_png_gray_info(const char* path, int* height, int* width, int* bit_depth);
int r3d_png_gray_decode_batch(const char* const* paths, int n_files, void* h_out, int height, int width, int bit_depth);
/* The SAME raster cv.imread(path, IMREAD_GRAYSCALE) returns, for every non-interlaced 8/16-bit PNG: uint8 [n][height][width].
 * 8-bit grey: as stored; 16-bit: the high byte (libpng's strip_16, OpenCV's choice); alpha: dropped; RGB(A): converted by
 * `rule` --
 *   R3D_GRAY_OPENCV_PNG  (9797 R + 19234 G + 3737 B) >> 15, a pixel with R = G = B keeps its value: libpng's
 *                        png_set_rgb_to_gray(1, 0.299, 0.587), which is what OpenCV's PNG reader (4.2.0, the reference's pin,
 *                        and later) calls instead of cvtColor; the reference's camera_to_world.py:160 on a PNG file;
 *   R3D_GRAY_CVTCOLOR    (4899 R + 9617 G + 1868 B + 8192) >> 14: cv.cvtColor(BGR2GRAY), imread's rule for the formats whose
 *                        decoders deliver colour (BMP, TIFF, WebP).
 * (Files carrying gamma information -- gAMA / sRGB / iCCP chunks -- make libpng convert in linear light: not restated; a pixel
 * with differing channels in such a file -> R3D_ERR_UNSUPPORTED under R3D_GRAY_OPENCV_PNG, equal channels pass through as in libpng.
 * Palette, interlaced and sub-byte PNGs: R3D_ERR_UNSUPPORTED.)  r3d_rgb_to_gray_u8: the rule alone, on [n][channels] 8-bit
 * R,G,B(,A) pixels already in memory. */
#define R3D_GRAY_OPENCV_PNG 0
#define R3D_GRAY_CVTCOLOR 1
int r3d_png_gray8_info(const char* path, int* height, int* width);
int r3d_png_gray8_decode_batch(const char* const* paths, int n_files, unsigned char* h_out, int height, int width, int rule);
int r3d_rgb_to_gray_u8(const unsigned char* pixels, int64_t n_pixels, int channels, int rule, unsigned char* gray_out);
/* The same for JPEG depth files (AirSim writes its depth images as 3-channel JPG, airsim/main.cpp:1369-1392): OpenCV's JPEG reader
 * asks libjpeg for GREY output, i.e. the luma component alone through libjpeg's default integer IDCT ("islow", jidctint.c), + 128,
 * clamped -- restated here, pinned byte for byte against libjpeg-turbo (PIL's draft('L') decode makes the same request).
 * Sequential Huffman JPEGs of 1 or 3 (YCbCr) components with full-resolution luma, restart intervals included; progressive,
 * arithmetic-coded, 12-bit, CMYK and RGB-tagged files: R3D_ERR_UNSUPPORTED.  n files into one [n][height][width] buffer. */
int r3d_jpeg_gray_info(const char* path, int* height, int* width);
int r3d_jpeg_gray_decode_batch(const char* const* paths, int n_files, unsigned char* h_out, int height, int width);
/* The colour images of the RGBD path (the `Image.open(imgpath)` of genply_noRGB, pixel_to_camera.py:58-60): non-interlaced
 * 8-bit PNGs -- RGB, RGBA (alpha dropped) or grey (replicated) -- as R,G,B bytes, n files into one [n][height][width][3]
 * buffer, which is what r3d_fuse_frames_rgb takes.  *channels = samples per pixel in the file. */
int r3d_png_rgb_info(const char* path, int* height, int* width, int* channels);
int r3d_png_rgb_decode_batch(const char* const* paths, int n_files, unsigned char* h_out, int height, int width);
/* The same for JPEG colour files (AirSim's scene images, airsim/main.cpp:1369-1392): the bytes PIL / libjpeg(-turbo) give by
 * default -- every component through the islow IDCT, chroma to full resolution by libjpeg's "fancy" triangle upsampling
 * (jdsample.c h2v1 / h2v2; replication when a chroma row has fewer than three samples), YCbCr -> RGB through jdcolor.c's
 * 16-bit fixed-point tables; a grey JPEG is replicated.  Pinned byte for byte against PIL over sizes, qualities and
 * 4:4:4 / 4:2:2 / 4:2:0.  (That is libjpeg-turbo's / libjpeg 6b's decoder, the one in current Pillow wheels and in OpenCV; IJG
 * libjpeg 7+ upsamples subsampled chroma in the DCT domain and gives slightly different COLOURS for 4:2:x files.)
 * Same refusals as the grey reader, plus any other chroma layout: R3D_ERR_UNSUPPORTED (the Python
 * host then lets PIL decode, which IS the reference's reader for colour).  *components = 1 or 3. */
int r3d_jpeg_rgb_info(const char* path, int* height, int* width, int* components);
int r3d_jpeg_rgb_decode_batch(const char* const* paths, int n_files, unsigned char* h_out, int height, int width);

/* ---- f2: occupied-voxel set + OctoMap binary export.  Replaces the per-point tree.updateNode(xyz, True) loop,
 * updateInnerOccupancy() and writeBinary() of octomap/txt_transfer_octomap.py:16-36 and
 * octomap/ply_transfer_octomap.py:16-48 (arithmetic in the un-vendored OctoMap library; restated from its
 * published semantics: float coordinates, key = (int)floor((1/res)*x) + 32768 per axis, depth 16, hits only).
 * The set lives in HBM as an open-addressing hash table of 48-bit Morton codes; `capacity` = slots
 * (rounded up to a power of two; >= 2x the expected number of distinct voxels keeps probing short). */
typedef struct r3d_voxelset r3d_voxelset;
struct r3d_comm; /* multi-GPU communicator, declared below */
int r3d_voxelset_create(r3d_ctx* ctx, double resolution, int64_t capacity, r3d_voxelset** vs_out);
int r3d_voxelset_destroy(r3d_voxelset* vs);
int r3d_voxelset_clear(r3d_voxelset* vs);
/* Insert float32 xyz points (on the ctx stream; may be called once per frame batch).  Two paths with the same result:
 *   1  per-workgroup LDS set in front of 64-bit CAS into the table: for clouds whose neighbouring points share voxels (scans);
 *   2  sort-merge: region-tagged keys, two radix passes, every table region updated in LDS and streamed back -- no random
 *      access to HBM: for clouds where nearly every point has a voxel of its own (2-3x faster there; needs a table of
 *      2^16..2^29 slots).
 * Tuning key "voxel_path": 0 (default) = inserts of >= 2^22 points into a table of <= 16 slots per point are SAMPLED first
 * (256 groups of 4096 neighbouring points: distinct voxels per point; path 2 when its cost -- per point and per table slot -- comes
 * out below path 1's, which on a 2-slots-per-point table is the case below ~7 points per voxel among neighbours) -- that sample
 * synchronises the stream once (16 bytes come back); smaller inserts take path 1 without asking.  1 / 2 force a path
 * (asynchronous).  "voxel_last_path" reads back which one the last insert took. */
int r3d_voxelset_insert(r3d_voxelset* vs, const float* d_xyz, int64_t n_points);
/* The cloud AND the map in one launch: r3d_fuse_frames_rgb (f32 xyz; d_pose NULL = camera frame; d_rgb and d_rgba_out both
 * NULL = no colour) followed by r3d_voxelset_insert of the points it wrote, without reading them back: the keys are taken
 * from the very floats the store writes.  Same cloud bytes, same set, same counters as the two calls.  (camera_to_world.py
 * :77-86 feeding txt_transfer_octomap.py:16-26 in the reference.)  The call picks the faster FORM itself ("voxel_path" 0): a
 * big batch is probed -- its first ~2^18 points are fused by the plain kernel and sampled as above -- and the rest goes
 * either through the one-launch kernel (scans) or through plain fuse + sort-merge insert of the whole cloud (no surfaces);
 * "voxel_path" 1 = always the one-launch kernel, 2 = always fuse + sort-merge. */
int r3d_fuse_frames_voxel(r3d_ctx* ctx, const r3d_camera* cam, const void* d_depth, int depth_dtype, int n_frames,
                          double depth_scale, const double* d_pose, const unsigned char* d_rgb, float* d_xyz_out,
                          uint32_t* d_rgba_out, r3d_voxelset* vs);
int r3d_voxelset_insert_host(r3d_voxelset* vs, const float* h_xyz, int64_t n_points);
/* synchronises; any pointer may be NULL.  n_ignored = points outside the 2^16 key range or non-finite
 * (OctoMap drops them); n_overflow > 0 means the table was too small and the set is incomplete. */
int r3d_voxelset_stats(r3d_voxelset* vs, int64_t* n_voxels, int64_t* n_ignored, int64_t* n_overflow);
/* distinct voxels as ascending 48-bit Morton codes (3 bits per level, x lowest: OctoMap's child index order).
 * h_codes_sorted == NULL only reports the count. */
int r3d_voxelset_codes(r3d_voxelset* vs, uint64_t* h_codes_sorted, int64_t cap, int64_t* n_out);
/* Insert ready-made 48-bit Morton codes (e.g. another rank's distinct voxels); codes with bits above 48 count as ignored. */
int r3d_voxelset_insert_codes(r3d_voxelset* vs, const uint64_t* d_codes, int64_t n_codes);
/* Config 5 (frames sharded over the GPUs, ONE map): collective over `comm`.  Every rank has voxelised its own shard of the
 * world cloud into its own set; the ranks all-gather only their DISTINCT codes (8 B/voxel, unequal shards -- the 12 B/point
 * of the clouds never leave their GPU) and fold them in.  Afterwards every rank's set is the union.  Synchronises.
 * `comm` must live on the set's context (one stream orders the set's kernels and the exchange).  If ANY rank's set has
 * overflowed, every rank takes part in the first exchange and then returns R3D_ERR_NOMEM: no rank is left waiting. */
int r3d_voxelset_union(r3d_voxelset* vs, struct r3d_comm* comm);

/* ---- voxel-grid downsampling: one output point per occupied voxel (Open3D's voxel_down_sample).  A device-resident
 * accumulator bound to one ctx: points are inserted, possibly over many calls, then extracted as one row per occupied voxel
 * in ascending 48-bit Morton order.  The voxel of a point is the voxel set's (same key rule, same ignored points), so the
 * extracted codes equal r3d_voxelset_codes of the same cloud and go straight to r3d_octree_write_bt.  Per voxel: the code, the
 * exact point count, the centroid (f32, from exact fixed-point sums: within ulp_f32 + res * 2^-28 of the exact mean) and,
 * with R3D_VOXELGRID_RGB, the mean colour word (r | g << 8 | b << 16, as r3d_fuse_frames_rgb writes; each channel
 * floor((2 S + n) / (2 n))).  Every output bit is independent of launch geometry and of how the points were split into
 * inserts and in which order.  `capacity` = table slots (rounded up to a power of two; >= 2x the expected voxels).  A full
 * table counts the points that found no slot (n_overflow) and extract then returns R3D_ERR_NOMEM until r3d_voxelgrid_clear.
 * A voxel of more than 2^32 - 1 points makes extract return R3D_ERR_INVALID with nothing written. */
typedef struct r3d_voxelgrid r3d_voxelgrid;
#define R3D_VOXELGRID_RGB 1 /* the grid also accumulates colour words */
int r3d_voxelgrid_create(r3d_ctx* ctx, double resolution, int64_t capacity, int flags, r3d_voxelgrid** vg_out);
int r3d_voxelgrid_destroy(r3d_voxelgrid* vg);
int r3d_voxelgrid_clear(r3d_voxelgrid* vg);
/* asynchronous on the ctx stream; d_rgba NULL = no colour (must be NULL iff the grid was created without R3D_VOXELGRID_RGB);
 * the alpha byte of an input word is not read */
int r3d_voxelgrid_insert(r3d_voxelgrid* vg, const float* d_xyz, const uint32_t* d_rgba, int64_t n_points);
int r3d_voxelgrid_insert_host(r3d_voxelgrid* vg, const float* h_xyz, const uint32_t* h_rgba, int64_t n_points);
/* synchronises; any pointer may be NULL.  n_ignored as r3d_voxelset_stats; n_overflow = points that found no slot */
int r3d_voxelgrid_stats(r3d_voxelgrid* vg, int64_t* n_voxels, int64_t* n_ignored, int64_t* n_overflow);
/* synchronises; device outputs ([cap][3] f32, [cap] u32, [cap] u32, [cap] u64), any of them may be NULL; all NULL = only
 * report *n_out.  cap < voxels -> R3D_ERR_INVALID, nothing written, *n_out set; overlapping output ranges -> R3D_ERR_INVALID. */
int r3d_voxelgrid_extract(r3d_voxelgrid* vg, float* d_xyz_out, uint32_t* d_rgba_out, uint32_t* d_count_out,
                          uint64_t* d_codes_out, int64_t cap, int64_t* n_out);
/* ---- k nearest neighbours of an index's own points, and outlier removal over them.  P = the cloud the index was built from
 * (n rows, original order); d2(i,j) = fmaf(dz,dz, fmaf(dy,dy, dx*dx)), dx = x_i - x_j ..., the index's NN expression.  A pair is a
 * candidate iff j != i and d2(i,j) is finite: a point with a NaN / inf coordinate has no candidates and is nobody's.  Every
 * call is deterministic (fixed-order fp64 reductions, no float atomics); invalid arguments return R3D_ERR_INVALID with nothing
 * written.
 * r3d_nn_index_knn_self (1 <= k <= 32; asynchronous): row i of d_idx_out [n][k] (u32) / d_d2_out [n][k] (f32, may be NULL)
 * holds the k candidates j with the smallest (d2(i,j), j), ascending; fewer than k candidates -> the tail is (UINT32_MAX, +inf). */
int r3d_nn_index_knn_self(r3d_nn_index* index, int k, uint32_t* d_idx_out, float* d_d2_out);
/* Statistical outlier removal (1 <= k <= 32, std_ratio finite and > 0; synchronises).  Point i is scored iff it has k
 * candidates; m_i = (sum over its k-list of sqrt((double) d2), ascending, in fp64) / k, unscored: +inf.  Over the V scored
 * points mu = sum m / V, sigma = sqrt(sum (m - mu)^2 / (V - 1)) (0 when V <= 1), T = mu + std_ratio sigma; d_keep_out[i]
 * (u8) = m_i <= T.  m_i depends only on the k smallest d2 values: bit-identical under any row permutation.  Optional:
 * d_score_out [n] f64 = m_i, h_stats_out (host, 4 doubles) = V, mu, sigma, T; h_n_kept = points kept. */
int r3d_outlier_statistical(r3d_nn_index* index, int k, double std_ratio, uint8_t* d_keep_out, double* d_score_out,
                            double* h_stats_out, int64_t* h_n_kept);
/* Radius outlier removal (radius finite and > 0, min_points >= 1; synchronises): r2 = (float)((double) radius * radius),
 * c_i = #{candidates j : d2(i,j) <= r2}, d_keep_out[i] = c_i >= min_points; d_count_out [n] u32 (may be NULL) =
 * min(c_i, min_points) (saturated: the search stops early). */
int r3d_outlier_radius(r3d_nn_index* index, double radius, int64_t min_points, uint8_t* d_keep_out, uint32_t* d_count_out,
                       int64_t* h_n_kept);
/* Normals of the index's own cloud P (n rows, original order) from the covariance of each point's neighbourhood (3 <= k <= 32).
 * Asynchronous on the ctx stream; deterministic (the same bits on every run and for every launch geometry).
 * Neighbourhood: N_i = row i of r3d_nn_index_knn_self(index, k) -- the exact (d2, j) order, ties by row, tails dropped -- cut,
 *   when radius > 0, at the first entry with d2 > (float)((double) radius * radius) (radius <= 0: no cut).  c_i = |N_i| goes to
 *   d_count_out [n] u32.
 * Covariance (fp64, no fused multiply-add, fixed order): e_j = (double) p_j - (double) p_i per component; S1 = sum e_j and
 *   S2_ab = sum e_j,a * e_j,b for ab in xx, xy, xz, yy, yz, zz, both over N_i in list order starting from 0.0.  The point itself
 *   is a member with e = 0, so m = c_i + 1 and C_ab = (S2_ab - S1_a * S1_b / m) / m, evaluated as written.  d_cov_out [n][6]
 *   f64 = the six C_ab in that order.  Differences about the query point keep the sums small whatever the cloud's offset.
 * Normal: the unit eigenvector of the smallest eigenvalue l0 <= l1 <= l2 of C (cyclic Jacobi rotations in fp64; of equal
 *   eigenvalues the lowest axis), rounded once to f32 into d_normals_out [n][3].  d_curvature_out [n] f32 =
 *   (float)(l0 / (l0 + l1 + l2)) with a rounding-negative l0 taken as 0 (surface variation; 0 when the sum is 0).
 * Sign: with n_views > 0, row i belongs to view v = min(i / points_per_view, n_views - 1) (n_views = 1: one camera for the
 *   whole cloud; n_views = F, points_per_view = H*W: an r3d_fuse_frames cloud and the frames' camera centres) and the normal is
 *   negated iff n . (h_viewpoints[v] - p_i) < 0, in fp64 from the fp64 eigenvector.  n_views = 0: negated iff its component of
 *   largest magnitude (lowest axis on ties) is negative.  The table (host, [n_views][3] f64) is copied before the call returns;
 *   n_views > 1 with points_per_view < n needs n <= 2^31.
 * No plane: the zero vector, curvature 0 and a zero covariance are written when p_i has a non-finite coordinate, when c_i < 2,
 *   or when l1 <= 0 (all members on one line to the last bit, e.g. a cluster of identical points); c_i is written as it is.
 * d_curvature_out, d_cov_out, d_count_out may be NULL.  k out of range, radius NaN, n_views < 0, n_views > 0 with a NULL table
 *   or points_per_view < 1, NULL normals, outputs overlapping each other or the index's cloud -> R3D_ERR_INVALID, nothing written. */
int r3d_normals_knn(r3d_nn_index* index, int k, double radius, const double* h_viewpoints, int64_t n_views,
                    int64_t points_per_view, float* d_normals_out, float* d_curvature_out, double* d_cov_out,
                    uint32_t* d_count_out);
/* Order-preserving row selection (synchronises): the xyz rows i with d_keep[i] != 0, in their original order, into d_xyz_out
 * and (optional) their row numbers i into d_rows_out (u32); *h_n_out = rows kept.  The outputs need room for the kept rows
 * only; an output that overlaps an input or the other output -> R3D_ERR_INVALID. */
int r3d_select_rows(r3d_ctx* ctx, const float* d_xyz, int64_t n_points, const uint8_t* d_keep, float* d_xyz_out,
                    uint32_t* d_rows_out, int64_t* h_n_out);
/* ---- RANSAC plane segmentation (csrc/r3d_ransac.hip; NOT IN THE REFERENCE -- what users of this kind of pipeline call Open3D's
 * segment_plane for; no parity with Open3D is claimed, this text is the specification).  d_xyz [n][3] f32, 3 <= n < 2^32;
 * thr = distance_threshold, finite and > 0; 1 <= H = n_hypotheses <= 65536; seed: any u64.  Synchronises.  Every output bit is
 * the same on every run; the counts are integer sums and do not depend on the launch geometry.
 * Sampler (counter-based; r3d_ransac_rows is the same function on the host, no GPU needed): the rows of hypothesis h are
 *   r_j(h) = mulhi64(splitmix64(seed + (3h + j + 1) * 0x9E3779B97F4A7C15 mod 2^64), n), j = 0, 1, 2, with
 *   splitmix64(z): z = (z ^ z >> 30) * 0xBF58476D1CE4E5B9; z = (z ^ z >> 27) * 0x94D049BB133111EB; return z ^ z >> 31  (mod 2^64)
 *   and mulhi64(a, n) = (a * n) >> 64.
 * Hypothesis: a, b, c = the three rows in fp64; u = b - a, v = c - a, N = u x v = (uy vz - uz vy, uz vx - ux vz, ux vy - uy vx),
 *   l2 = (Nx Nx + Ny Ny) + Nz Nz, all in fp64 as written, no fused multiply-add.  Valid iff the three rows are pairwise different
 *   and l2 is finite and > 0 (duplicates, collinear triples and non-finite points are out).  n^ = (float)(N / sqrt(l2)) per
 *   component; the anchor a^ is the f32 point of row r_0.
 * Count: e = p_i - a^ per component in f32, s = (n^x ex + n^y ey) + n^z ez in f32, no fused multiply-add;
 *   c_h = #{i : |s| <= (float) thr}.  NaN compares false: a non-finite point is nobody's inlier.  Invalid hypothesis: c_h = 0.
 *   d_counts_out [H] u32 (may be NULL) = c_h.
 * Best hypothesis: the lowest h among those with maximal c_h.  Maximum < 3: there is no plane -- R3D_OK, *n_inliers_out = 0, the
 *   mask all zero, plane, centroid and eigenvalues NaN (best h, c_best, its rows and the valid count are still reported).
 * Refit: I0 = the best hypothesis' inliers by the same f32 test, m = |I0|.  With e = (double) p - (double) a^: S1 = sum e and
 *   S2 = the six sums e_a e_b (xx, xy, xz, yy, yz, zz), fp64, reduced in two fixed-order stages (shuffle tree -> LDS -> one row per
 *   workgroup -> one fold; no float atomics).  Centroid c = a^ + S1 / m, C = (S2 - S1 S1^T / m) / m evaluated as written.
 *   n = the unit eigenvector of the smallest eigenvalue l0 <= l1 <= l2 of C (cyclic Jacobi in fp64 on the host; of equal
 *   eigenvalues the lowest axis), negated iff its component of largest magnitude (lowest axis on ties) is negative;
 *   d = -((nx cx + ny cy) + nz cz).  l1 <= 0 (the inliers are collinear to the last bit): the hypothesis' own fp64 plane,
 *   n = N / sqrt(l2) with the same sign rule, c = a, eigenvalues as computed.
 * Final mask: t = (nx (x - cx) + ny (y - cy)) + nz (z - cz) in fp64 from the f32 point, no fused multiply-add;
 *   d_inlier_out[i] (u8) = |t| <= thr; *n_inliers_out = their number.
 * h_result (host, 16 doubles): [0..3] plane a b c d, [4..6] centroid, [7..9] l0 l1 l2, [10] best h, [11] c_best,
 *   [12..14] the best hypothesis' rows, [15] the number of valid hypotheses.
 * NULL ctx / d_xyz / d_inlier_out / h_result / n_inliers_out, n < 3 or >= 2^32, H out of range, thr not finite or not > 0,
 *   outputs overlapping the cloud or each other -> R3D_ERR_INVALID, nothing written to any output. */
int r3d_segment_plane(r3d_ctx* ctx, const float* d_xyz, int64_t n, double distance_threshold, int n_hypotheses, uint64_t seed,
                      uint8_t* d_inlier_out, uint32_t* d_counts_out, double* h_result, int64_t* n_inliers_out);
/* The sampler alone (host): rows[j] = r_j(h) for a cloud of n rows.  NULL rows, n < 1 or n >= 2^32 -> R3D_ERR_INVALID. */
int r3d_ransac_rows(uint64_t seed, uint64_t h, int64_t n, uint32_t* rows);
/* ---- Global registration: FPFH features, feature matching, RANSAC over correspondences (csrc/r3d_fpfh.hip,
 * csrc/r3d_register.hip; NOT IN THE REFERENCE -- what users of this kind of pipeline call Open3D's compute_fpfh_feature and
 * registration_ransac_based_on_feature_matching for, in front of ICP; no parity with Open3D or PCL is claimed, this text is the
 * specification).  Every output bit is the same on every run and for every launch geometry; all f32 / f64 arithmetic below is
 * evaluated as written, one rounding per operation, no fused multiply-add, IEEE division and square root.
 * dot(a, b) = (ax bx + ay by) + az bz and a x b = (ay bz - az by, az bx - ax bz, ax by - ay bx) throughout.
 *
 * r3d_fpfh_knn: FPFH of the index's own cloud P (n rows, original order); 3 <= k <= 32; asynchronous on the ctx stream.
 * d_normals [n][3] f32 as r3d_normals_knn writes them; a row is "no normal" when a component is non-finite or all three are 0.
 * Neighbourhood: N_i = row i of r3d_nn_index_knn_self(index, k) with its d2 values, in list order, tails dropped, cut when
 *   radius > 0 at the first entry with d2 > (float)((double) radius * radius) (radius <= 0: no cut).
 * Pair feature of (i, j), j in N_i, in f32: d = p_j - p_i per component, L = sqrt((dx dx + dy dy) + dz dz).  The pair is skipped
 *   when L is 0 or non-finite or when i or j has no normal.  a_i = dot(n_i, d), a_j = dot(n_j, d).  If |a_j| > |a_i| the roles
 *   swap: u = n_j, n_t = n_i, d := -d; otherwise (ties included) u = n_i, n_t = n_j.  d^ = d / L per component; v = d^ x u;
 *   l_v = sqrt((vx vx + vy vy) + vz vz), the pair is skipped when l_v is 0 or non-finite; v^ = v / l_v; w = u x v^;
 *   alpha = dot(v^, n_t), phi = dot(u, d^), x = dot(u, n_t), y = dot(w, n_t).  The pair is skipped when one of alpha, phi, x, y
 *   is non-finite or when x = y = 0.
 * Bins: 11 per feature, stored in the order theta, alpha, phi (R3D_FPFH_DIM = 33 values per point).  For f = alpha, phi:
 *   t = (f + 1.0f) * 5.5f, b = 0 when t < 1, 10 when t >= 10, else (int) t.  theta = the direction of (x, y), binned without a
 *   transcendental: with (c_m, s_m) = R3D_FPFH_THETA_COS / _SIN [m - 1], the f32 roundings of cos / sin of
 *   beta_m = -pi + 2 pi m / 11, m = 1..10, and cr_m = c_m * y - s_m * x, b_theta = the number of m with
 *   (y >= 0 || cr_m >= 0) for m <= 5 (beta_m < 0), (y >= 0 && cr_m >= 0) for m >= 6 (beta_m > 0).
 * SPFH: spfh_i[3][11] = the pairs of point i counted per bin (<= 32: u8) -> d_spfh_out [n][33] u8; c_i = the pairs counted ->
 *   d_count_out [n] u32.
 * FPFH (f32): P_j[e] = (float) spfh_j[e] * (100.0f / (float) c_j), all zero when c_j = 0.  A[e] = sum over j in N_i, in list
 *   order, with d2_ij finite and > 0 (the list's value), of P_j[e] / d2_ij, from 0.0f.  T[s] = sum_b A[s][b], b ascending, from
 *   0.0f.  d_fpfh_out[i][s][b] = P_i[s][b] + (T[s] > 0 ? A[s][b] * (100.0f / T[s]) : 0.0f).  A point with a non-finite
 *   coordinate has an empty list and gets 33 zeros.
 * d_spfh_out, d_count_out may be NULL.  NULL index / d_normals / d_fpfh_out, k out of range, radius NaN, outputs overlapping each
 *   other, the normals or the index's cloud -> R3D_ERR_INVALID, nothing written. */
#define R3D_FPFH_DIM 33
#define R3D_FPFH_THETA_COS \
  { -0.841253519f, -0.415415019f, 0.142314836f, 0.654860735f, 0.959492981f, 0.959492981f, 0.654860735f, 0.142314836f, -0.415415019f, -0.841253519f }
#define R3D_FPFH_THETA_SIN \
  { -0.540640831f, -0.909631968f, -0.989821434f, -0.755749583f, -0.281732559f, 0.281732559f, 0.755749583f, 0.989821434f, 0.909631968f, 0.540640831f }
int r3d_fpfh_knn(r3d_nn_index* index, int k, double radius, const float* d_normals, float* d_fpfh_out, uint8_t* d_spfh_out,
                 uint32_t* d_count_out);
/* r3d_feature_match: d_a [na][33], d_b [nb][33] f32, 1 <= na, nb < 2^32.  dist(i, j) = sum_{b = 0..32} e_b * e_b, e_b = a_ib - b_jb,
 *   every product and sum its own f32 operation, b ascending, from 0.0f.  d_idx_out [na] u32 = the j with the smallest
 *   (dist, j) among finite dist, d_dist_out [na] f32 (may be NULL) = that dist; no finite dist: (UINT32_MAX, +inf).
 * Correspondences (d_corr_out != NULL; this part synchronises): row i is kept iff idx_a[i] != UINT32_MAX and, with mutual = 1,
 *   idx_b[idx_a[i]] == i, idx_b being the same search from b to a.  d_corr_out [*h_m_out][2] u32 = (i, idx_a[i]) of the kept rows,
 *   i ascending; the buffer holds [na][2].  d_corr_out == NULL: h_m_out must be NULL and mutual 0; the call is asynchronous.
 * NULL ctx / d_a / d_b / d_idx_out, sizes out of range, mutual not 0 / 1, one of d_corr_out and h_m_out without the other,
 *   outputs overlapping each other or an input -> R3D_ERR_INVALID, nothing written. */
int r3d_feature_match(r3d_ctx* ctx, const float* d_a, int64_t na, const float* d_b, int64_t nb, int mutual, uint32_t* d_idx_out,
                      float* d_dist_out, uint32_t* d_corr_out, int64_t* h_m_out);
/* r3d_register_ransac: the rigid motion T with q ~ T p for the most correspondences.  d_src [ns][3], d_tgt [nt][3] f32;
 *   d_corr [m][2] u32 (source row, target row), 3 <= m < 2^32; thr = distance_threshold, finite and > 0;
 *   1 <= H = n_hypotheses <= 65536; seed: any u64.  Synchronises.  Pair g is (p_g, q_g) = (src[corr[g][0]], tgt[corr[g][1]]);
 *   a row number outside its cloud makes that point NaN.
 * Sampling: hypothesis h takes the pairs r_j(h), j = 0, 1, 2, of r3d_ransac_rows(seed, h, m).
 * Pose (fp64 from the f32 points): with (a, b, c) the three source points, u = b - a, v = c - a, N = u x v,
 *   e1 = u / sqrt(|u|^2), e3 = N / sqrt(|N|^2), e2 = e3 x e1, |z|^2 = (zx zx + zy zy) + zz zz; the target points (a', b', c') give
 *   e1', e2', e3' the same way.  R_rc = (e1'_r e1_c + e2'_r e2_c) + e3'_r e3_c, t_r = a'_r - ((R_r0 ax + R_r1 ay) + R_r2 az).
 *   Valid iff the three source rows are pairwise different, the three target rows are pairwise different, |u|^2, |N|^2, |u'|^2,
 *   |N'|^2 are finite and > 0, and | sqrt(|z|^2) - sqrt(|z'|^2) | <= 2 thr for z = b - a, c - a, c - b.
 * Count: R^, t^ = R, t rounded once to f32; per pair, in f32, q^_r = ((R^_r0 px + R^_r1 py) + R^_r2 pz) + t^_r, e = q^ - q,
 *   s2 = (ex ex + ey ey) + ez ez; c_h = #{g : s2 <= (float)(thr * thr)} (thr * thr in fp64).  NaN compares false.  An invalid
 *   hypothesis has c_h = 0.  d_counts_out [H] u32 (may be NULL) = c_h.
 * Best hypothesis: the lowest h of maximal c_h.  Maximum < 3: R3D_OK, a zero mask, T and the rms NaN, 0 inliers (best h, c_best,
 *   its pairs and the valid count are still reported).
 * Refit: I0 = the best hypothesis' inliers by the same test.  With pc = (double) p - (double) a, qc = (double) q - (double) a'
 *   (a, a' the points of pair r_0), the 18 sums of r3d_icp_accumulate over (pc, qc), each pair adding, for axis = x, y, z in
 *   turn, pc_axis, qc_axis, pc_axis qc_b (b = x, y, z), pc_axis pc_axis and qc_axis qc_axis to its sum; one accumulator set per
 *   lane: lane L of G x 256 (G = min(ceil(m / 256), 1024)) takes the pairs L, L + 256 G, ... in order; the lanes of a workgroup
 *   are added by a halving tree inside each 64 (v_l += v_{l + off}, off = 32, 16, .. 1) and the four sixty-fours in order; the G
 *   rows are added by 256 lanes (lane t: rows t, t + 256, ... in order) and the same tree.  T_c = r3d_umeyama_from_sums(sums,
 *   with_scale = 0); R = R_c, t_r = (a'_r + t_c,r) - ((R_r0 ax + R_r1 ay) + R_r2 az).  An undefined fit keeps the hypothesis' own
 *   fp64 pose.
 * Final mask: the same f32 test with the refitted pose rounded to f32 -> d_inlier_out [m] u8.
 * h_result (host, R3D_REGISTER_RESULT_DOUBLES doubles): [0..15] T row-major 4x4, [16] best h, [17] c_best, [18..20] the pairs
 *   r_0 r_1 r_2 of the best hypothesis, [21] the number of valid hypotheses, [22] the final inlier count, [23] the inlier rms
 *   sqrt(sum (double) s2 / count) over the final inliers (the same two-stage order; NaN without inliers), [24] 1 when the refit
 *   was undefined, [25..31] 0.
 * NULL ctx / d_src / d_tgt / d_corr / d_inlier_out / h_result, sizes, H or thr out of range, outputs overlapping an input or each
 *   other -> R3D_ERR_INVALID, nothing written to any output. */
#define R3D_REGISTER_RESULT_DOUBLES 32
int r3d_register_ransac(r3d_ctx* ctx, const float* d_src, int64_t n_src, const float* d_tgt, int64_t n_tgt, const uint32_t* d_corr,
                        int64_t n_corr, double distance_threshold, int n_hypotheses, uint64_t seed, uint8_t* d_inlier_out,
                        uint32_t* d_counts_out, double* h_result);
/* In-place ascending sort of 64-bit keys in HBM by their low key_bits bits (stable LSD radix sort, 8-bit digits;
 * asynchronous on the ctx stream).  Building block of r3d_voxelset_codes, exported for tests and reuse. */
int r3d_sort_u64(r3d_ctx* ctx, uint64_t* d_keys, int64_t n_keys, int key_bits);
/* OctoMap ".bt" bytes (header + pruned maximum-likelihood tree, depth first) for ascending unique codes. */
int r3d_octree_format_bt(const uint64_t* h_codes_sorted, int64_t n_codes, double resolution, char* h_buf,
                         size_t buf_cap, size_t* n_bytes_out, int64_t* n_nodes_out);
int r3d_octree_write_bt(const char* path, const uint64_t* h_codes_sorted, int64_t n_codes, double resolution,
                        int64_t* n_nodes_out);
/* The same tree serialised ON THE DEVICE (csrc/r3d_octree.hip): the codes never visit host memory, only the finished records
 * (2 bytes per inner node) cross PCIe.  Byte-identical to the two host calls above, which stay as the path without a GPU.
 * r3d_octree_records_device: the uint16 records (depth-first pre-order; child c's field at bits 2c..2c+1: 00 absent, 10 leaf,
 * 11 inner) of the pruned tree over n_codes ascending unique codes in HBM; *n_nodes_out = the header's `size` (inner nodes +
 * the leaves the records name).  Two-call protocol (d_records_out == NULL: sizes only); synchronises the ctx stream once for
 * the sizes, the records themselves are enqueued.  cap_records < records, codes that do not strictly ascend or pass 48 bits,
 * output overlapping input -> R3D_ERR_INVALID, nothing written.  n_codes == 0 -> 0 records, 0 nodes.  No byte outside
 * d_records_out[0 .. records) is touched, whatever its alignment.
 * Tuning key "octree_timing" 1: HIP events around the four launches, read back (microseconds of the last call) through
 * "octree_count_us", "octree_scan_us", "octree_own_us", "octree_link_us"; such a call waits for its launches. */
int r3d_octree_records_device(r3d_ctx* ctx, const uint64_t* d_codes_sorted, int64_t n_codes, uint16_t* d_records_out,
                              int64_t cap_records, int64_t* n_records_out, int64_t* n_nodes_out);
/* The text header in front of the records, alone (host; h_buf == NULL only reports its length; it is not NUL-terminated).
 * n_nodes < 0, resolution <= 0 or a buffer that is too small -> R3D_ERR_INVALID. */
int r3d_octree_bt_header(int64_t n_nodes, double resolution, char* h_buf, size_t buf_cap, size_t* n_bytes_out);
/* The whole chain on the set's context: sorted codes (device) -> records (device) -> the .bt bytes in a host buffer (two-call
 * protocol like r3d_octree_format_bt) or, streamed by r3d_write_device_text_files, in a file.  An overflowed set is reported
 * exactly as r3d_voxelset_codes reports it (R3D_ERR_NOMEM; no file is created). */
int r3d_voxelset_format_bt(r3d_voxelset* vs, char* h_buf, size_t buf_cap, size_t* n_bytes_out, int64_t* n_nodes_out);
int r3d_voxelset_write_bt(r3d_voxelset* vs, const char* path, int64_t* n_nodes_out);

/* ---- TSDF volume (csrc/r3d_tsdf.hip; NOT IN THE REFERENCE -- what users of a depth + pose pipeline integrate their frames into
 * before meshing; no parity with Open3D's UniformTSDFVolume is claimed, this text is the specification).  Where r3d_fuse_frames
 * concatenates the frames' points, noise and all, the volume averages overlapping frames and yields the zero level set as
 * oriented points.  Every output bit is a chain of IEEE f32 operations in the order written here: no fused multiply-add,
 * correctly rounded division and square root, f32 denormals kept, independent of launch geometry and of how the frames are split
 * into calls.
 * Volume: origin[3], voxel_size, sdf_trunc are doubles rounded once to f32 (o, vs, tr; o finite, vs > 0, tr > 0), nx, ny, nz >= 1
 *   with nx ny nz < 2^31.  Storage: one float2 {tsdf, weight} per voxel at linear index (z ny + y) nx + x; a fresh or reset volume
 *   is all zero bytes.
 * Integration of frame f into voxel (x, y, z), frames in ascending f, all f32:
 *     c  = o + ((float) idx + 0.5f) * vs                                   per axis
 *     pc = ((R0 c.x + R1 c.y) + R2 c.z) + t                                per row of the pose, rounded to f32 on the host
 *     skip unless pc.z > 0
 *     u  = fx (pc.x / pc.z) + cx;  v = fy (pc.y / pc.z) + cy               the camera's intrinsics rounded to f32
 *     ui = floorf(u + 0.5f);  vi = floorf(v + 0.5f)                        skip unless 0 <= ui < W and 0 <= vi < H (as floats; NaN skips)
 *     d  = (float) depth[f][vi][ui] * (float) depth_scale                  skip unless d > 0 and d is finite
 *     sdf = d - pc.z                                                       skip if sdf < -tr
 *     tn = fminf(1.0f, sdf / tr);  w1 = w + 1.0f;  tsdf = (tsdf * w + tn) / w1;  w = w1
 *   h_pose_w2c: n_frames x 12 host doubles [R row-major (9), t (3)], WORLD -> CAMERA: p_cam = R p_w + t -- the quaternion's
 *   rotation and the pose file's t as they stand, BEFORE the inversion r3d_fuse_frames' table takes.  A depth of 0 is "no
 *   measurement" (the cloud path keeps its Z = 0 pixels).  Rasters of more than 2^24 pixels a side or 2^31 in all: R3D_ERR_INVALID.
 *   The frames of a call are applied R3D_TSDF_CHUNK per launch, inside the kernel: a batch costs one read and one write of the
 *   voxels it touches, not one per frame.  r3d_tsdf_integrate is asynchronous (the pose rows are copied before it returns);
 *   r3d_tsdf_integrate_host uploads the rasters itself and is synchronous.  NULL volume / camera, a camera of another ctx, an
 *   unknown dtype, n_frames < 0, NULL depth or poses with n_frames > 0 -> R3D_ERR_INVALID, nothing written; n_frames == 0 -> R3D_OK.
 * Surface points (synchronises): mw = (float) min_weight > 0; a voxel is valid iff w >= mw.  Voxels in linear index order, per
 *   voxel v the axes a = x, y, z in that order: n = v + e_a; if n is inside the volume, both are valid and (A < 0) != (B < 0) for
 *   A = tsdf(v), B = tsdf(n), one point: r = A / (A - B), position = the centre c of v with component a replaced by c_a + r * vs.
 *   Normal: g(q)_b = T(q + e_b) - T(q - e_b), T = that neighbour's tsdf if it is inside the volume and valid, else tsdf(q);
 *   m = g(v) + r * (g(n) - g(v)) per component, len = sqrtf((m0 m0 + m1 m1) + m2 m2), normal = m / len, or zeros unless len > 0.
 *   It points from behind the surface to in front of it, i.e. towards the cameras.
 *   d_xyz_out / d_normals_out: [cap][3] f32 (normals may be NULL; both may with cap == 0).  *n_out = the true number of points,
 *   always; at most cap rows are written and nothing beyond them; cap < *n_out is not an error.  Volumes of 2^32 / 3 voxels or
 *   more: R3D_ERR_UNSUPPORTED.
 * r3d_tsdf_volume: the device view of the float2 array ([n_voxels][2] f32), valid until destroy; work on the ctx stream. */
typedef struct r3d_tsdf r3d_tsdf;
#define R3D_TSDF_CHUNK 32 /* frames per integration launch */
int r3d_tsdf_create(r3d_ctx* ctx, const double* h_origin, double voxel_size, int nx, int ny, int nz, double sdf_trunc,
                    r3d_tsdf** out);
int r3d_tsdf_destroy(r3d_tsdf* vol);
int r3d_tsdf_reset(r3d_tsdf* vol);
int r3d_tsdf_integrate(r3d_tsdf* vol, const r3d_camera* cam, const void* d_depth, int depth_dtype, int n_frames,
                       double depth_scale, const double* h_pose_w2c);
int r3d_tsdf_integrate_host(r3d_tsdf* vol, const r3d_camera* cam, const void* h_depth, int depth_dtype, int n_frames,
                            double depth_scale, const double* h_pose_w2c);
int r3d_tsdf_volume(r3d_tsdf* vol, float** d_tsdf_weight_out, int64_t* n_voxels_out);
int r3d_tsdf_extract_points(r3d_tsdf* vol, double min_weight, float* d_xyz_out, float* d_normals_out, int64_t cap,
                            int64_t* n_out);

/* ---- TSDF mesh (csrc/r3d_tsdf_mesh.hip; marching cubes over the volume above; this text is the specification).  The result is
 * an INDEXED triangle mesh.  Its vertices are exactly the rows r3d_tsdf_extract_points writes for the same min_weight: same
 * count, same order, same bits for positions and normals.  The vertex of the volume edge "(voxel v, axis a)" is that edge's
 * surface point and its index is its rank in that order, so the mesh is welded by construction.  What is specified here is the
 * connectivity, which is integer-exact: the same bits whatever the launch geometry.
 * Cell: one per voxel (x, y, z) with x < nx-1, y < ny-1, z < nz-1.  Corner k = dx + 2 dy + 4 dz is voxel (x+dx, y+dy, z+dz).  A
 *   cell is active iff all 8 corners are valid (w >= mw, mw = (float) min_weight > 0); corner k is negative iff tsdf < 0 (the
 *   points' predicate (A < 0)); the case is m = sum of negative(k) << k.  Inactive cells emit nothing.  In an active cell a cell
 *   edge crosses iff its two corners differ in sign, which is exactly when the edge owns a surface point: every index a triangle
 *   names exists.
 * Cell edges: e = 4 a + j, a = the edge's axis, j = u + 2 v with (u, v) the offsets of the edge's lower corner along the two
 *   other axes in ascending axis order.  Edge e belongs to the voxel at that lower corner, on axis a.
 * Case table (built by construction -- tools/make_mc_table.py writes csrc/r3d_mc_table.h -- so that shared faces always agree):
 *   each of the 6 cell faces lists its 4 corners counter-clockwise as seen from outside the cell.  Walking that cycle, every
 *   maximal run of negative corners preceded by a non-negative corner gives one directed segment: from the cell edge where the
 *   walk enters the run (between the non-negative corner and the run's first corner) to the cell edge where it leaves the run.
 *   A face with two diagonal negative corners gives two segments, each cutting off one negative corner; the rule reads only the
 *   face's own four signs, so the two cells sharing a face draw the same segments in opposite directions.  Faces with 0 or 4
 *   negative corners give nothing.  The segments of a case form closed directed loops over its crossing edges.  Loops are taken
 *   in ascending order of their smallest edge id; each starts at that edge and follows the segments as l0, l1, ...; its
 *   triangles are the fan (l0, l_i, l_i+1), i = 1 .. len-2.  That is 820 triangles over the 256 cases, at most 5 per case
 *   (cases with 0..5 triangles: 2, 16, 50, 80, 76, 32).  With a single negative corner, (b - a) x (c - a) of the triangle
 *   (a, b, c) points away from that corner: towards the cameras, the side the vertex normals point to.
 * Order: cells in linear voxel order (z ny + y) nx + x of corner 0; within a cell the table's order.  Indices are int32.
 * r3d_tsdf_extract_mesh synchronises (for the counts; the rows are enqueued on the ctx stream).  *n_vertices_out and
 *   *n_triangles_out are the true counts, always; at most cap_vertices rows of d_xyz_out / d_normals_out ([cap_vertices][3] f32)
 *   and cap_triangles rows of d_tri_out ([cap_triangles][3] int32) are written and nothing beyond them; triangle rows are
 *   written as they are, even where an index is >= cap_vertices.  d_normals_out may be NULL; d_xyz_out may be NULL with
 *   cap_vertices == 0, d_tri_out with cap_triangles == 0.  Argument errors as for r3d_tsdf_extract_points (R3D_ERR_INVALID,
 *   nothing written).  5 n_voxels >= 2^32, or more than 2^31 - 1 vertices: R3D_ERR_UNSUPPORTED.  The volume is not modified. */
int r3d_tsdf_extract_mesh(r3d_tsdf* vol, double min_weight, float* d_xyz_out, float* d_normals_out, int64_t cap_vertices,
                          int32_t* d_tri_out, int64_t cap_triangles, int64_t* n_vertices_out, int64_t* n_triangles_out);

/* ---- Mesh components (csrc/r3d_mesh_cc.hip; NOT IN THE REFERENCE, this text is the specification).  A volume fused from noisy
 * depth leaves marching cubes as one large surface plus floaters of a few triangles each; these two calls label the connected
 * pieces of an indexed triangle mesh, count them, and keep the big ones or the biggest, on the device, between
 * r3d_tsdf_extract_mesh and the download.  Users of this kind of pipeline know the step as Open3D's cluster_connected_triangles
 * followed by remove_triangles_by_mask; NO parity with Open3D is claimed: connectivity here is by SHARED VERTEX, not by shared
 * edge (for a welded marching-cubes mesh the two separate the same floaters).  Everything is integer-exact: the same bits
 * whatever the launch geometry, the scheduling or the order of the triangles.  Not yet timed on a card.
 * The mesh: d_tri [n_triangles][3] int32 vertex indices into n_vertices vertices (their positions are never read).
 *
 * r3d_mesh_components
 *   Validity: a triangle is valid iff its three indices lie in [0, n_vertices); the indices are checked before any of them is used
 *     as an address.  An invalid triangle joins nothing, its triangle label is 0xFFFFFFFF, and it is counted in *n_invalid_out.
 *   A valid triangle with repeated indices ((a, a, b), (a, a, a)) joins what it names and counts like any other; a triangle that
 *     occurs twice counts twice.
 *   Connectivity: two vertices are connected iff a chain of valid triangles links them through shared vertex indices.
 *   d_vertex_label_out [n_vertices] u32: the smallest vertex index of the vertex's component.  A vertex no valid triangle names is
 *     its own label.
 *   d_tri_label_out [n_triangles] u32 (may be NULL): the label of the triangle's first index; 0xFFFFFFFF for an invalid triangle.
 *   d_comp_out [cap_components][3] u32 rows {label, n_vertices, n_triangles}: the components that have at least one valid
 *     triangle, in ascending label; n_vertices = the vertices that carry the label, n_triangles = the valid triangles whose label
 *     it is.  May be NULL with cap_components == 0.  *n_components_out is the true count, always; at most cap_components rows are
 *     written and nothing beyond them (call with cap 0 for the count, then with room).
 *   n_triangles == 0: every vertex is its own label, 0 components.  n_vertices == 0 (every triangle is then invalid) is fine too.
 *   R3D_ERR_INVALID, nothing written: a NULL ctx, n_components_out or n_invalid_out; a negative size or cap; a NULL d_tri with
 *     n_triangles > 0, d_vertex_label_out with n_vertices > 0 or d_comp_out with cap_components > 0; an output overlapping the
 *     triangles or another output.  n_vertices or n_triangles > 2^31 - 1: R3D_ERR_UNSUPPORTED.
 *   How: lock-free union-find in d_vertex_label_out itself (csrc/r3d_unionfind_dev.h): parent[v] <= v always, the larger of two
 *     roots is hooked under the smaller with atomicMin and a lost race is answered by finding again; no lane waits for another, and
 *     every loop walks a strictly decreasing sequence of vertex numbers.  The next launch flattens.  Counts are integer atomics,
 *     the rows are placed by a scan.  The call synchronises once, for the two counts.
 *
 * r3d_mesh_filter_components: d_vertex_label [n_vertices] u32 = the labels r3d_mesh_components wrote for this mesh.  The call
 *   recounts the valid triangles per label (the label of a triangle's first index) itself, in integers.  A label that is not in
 *   [0, n_vertices) is data, never an address: its triangles count as invalid.
 *   A triangle is kept iff it is valid and its component has at least min_triangles valid triangles (min_triangles >= 1), and,
 *     with keep_largest != 0, its component is also the one with the greatest triangle count, ties going to the smallest label;
 *     both conditions apply together (the largest component is dropped too when it is smaller than min_triangles).
 *   Kept triangles stay in their original order.  A vertex is kept iff a kept triangle names it; kept vertices stay in ascending
 *     old index.  d_kept_vertices_out [cap_vertices] u32: entry new = the old index -- the row list r3d_gather_rows takes, so
 *     positions and normals are compacted with that call.  d_tri_out [cap_triangles][3] int32: the kept triangles, naming the NEW
 *     indices.  *n_vertices_out and *n_triangles_out are the true counts, always; at most cap rows each are written and nothing
 *     beyond them; a cap smaller than a count is not an error, and triangle rows are written as they are even where a new index
 *     is >= cap_vertices.  Either output may be NULL with its cap 0.  The call synchronises once, for the two counts.
 *   R3D_ERR_INVALID, nothing written: a NULL ctx, n_vertices_out or n_triangles_out; a negative size or cap; min_triangles < 1; a
 *     NULL d_tri with n_triangles > 0, d_vertex_label with n_vertices > 0, or output with a cap > 0; an output overlapping an input
 *     or the other output.  n_vertices or n_triangles > 2^31 - 1: R3D_ERR_UNSUPPORTED.
 * Neither call modifies its inputs.  Both keep their workspace (8 bytes per vertex, and 4 per 4096 vertices or triangles) in the
 *   context, apart from the scratch other calls share: results do not depend on what ran before on the context. */
int r3d_mesh_components(r3d_ctx* ctx, const int32_t* d_tri, int64_t n_triangles, int64_t n_vertices, uint32_t* d_vertex_label_out,
                        uint32_t* d_tri_label_out, uint32_t* d_comp_out, int64_t cap_components, int64_t* n_components_out,
                        int64_t* n_invalid_out);
int r3d_mesh_filter_components(r3d_ctx* ctx, const int32_t* d_tri, int64_t n_triangles, int64_t n_vertices,
                               const uint32_t* d_vertex_label, int64_t min_triangles, int keep_largest,
                               uint32_t* d_kept_vertices_out, int64_t cap_vertices, int32_t* d_tri_out, int64_t cap_triangles,
                               int64_t* n_vertices_out, int64_t* n_triangles_out);

/* ---- Mesh smoothing (csrc/r3d_mesh_smooth.hip, csrc/r3d_mesh_smooth_host.cpp; NOT IN THE REFERENCE, this text is the
 * specification).  Component removal takes the floaters away; the surface that stays is bumpy and terraced where the depth was
 * noisy.  These three calls build the vertex adjacency of an indexed triangle mesh, move the vertices by a sequence of umbrella
 * steps (Laplacian and Taubin smoothing), and recompute the vertex normals of the moved mesh, on the device, between
 * r3d_tsdf_extract_mesh (or r3d_mesh_filter_components) and the download.  Users know the steps as Open3D's filter_smooth_taubin
 * and compute_vertex_normals; NO parity with Open3D or MeshLab is claimed.  tests/mesh_smooth_ref.py restates this text in NumPy and
 * the device matches it bit for bit: no result depends on the launch geometry, the scheduling or the order of the triangles.
 * Timed once, without a gate: DESIGN.md 4.5j''.
 * The mesh: d_tri [n_triangles][3] int32 vertex indices into n_vertices vertices; positions [n_vertices][3] f32, packed.
 * A triangle is VALID iff its three indices lie in [0, n_vertices) (the rule of "Mesh components"); an invalid triangle
 * contributes nothing anywhere below, and no index is used as an address before it is checked.
 *
 * r3d_mesh_adjacency: the one-ring of every vertex as a CSR, and the boundary flags.
 *   Sides: a valid triangle (a, b, c) has the sides (a, b), (b, c), (c, a).  A side with u == v is dropped; the other sides of a
 *     degenerate triangle still count.
 *   Neighbours: v is a neighbour of u iff some side joins them, in either direction.  Row u of the CSR holds its distinct
 *     neighbours in ASCENDING INDEX: d_neighbours_out[d_row_start_out[u] .. d_row_start_out[u + 1]).  d_row_start_out
 *     [n_vertices + 1] u32 is always written whole; row_start[u + 1] - row_start[u] is the degree and row_start[n_vertices] the
 *     total E.  The adjacency is symmetric by construction, so E is even.
 *   Boundary: d_boundary_out [n_vertices] u8 (may be NULL): 1 iff the vertex lies on an undirected edge {u, v} that exactly one
 *     side has, counted with multiplicity over all valid triangles and both directions; else 0.  A triangle listed twice
 *     therefore makes its edges non-boundary, and a vertex without neighbours is not boundary.
 *   Caps: *n_neighbours_out is the true E, always; at most cap_neighbours entries of d_neighbours_out are written and nothing
 *     beyond them (call with cap 0 for the count, then with room); d_neighbours_out may be NULL with cap_neighbours == 0.
 *   n_triangles == 0 gives an all-zero row_start and boundary; n_vertices == 0 (every triangle is then invalid) is legal and
 *     writes the one word row_start[0] = 0.
 *   R3D_ERR_INVALID, nothing written: a NULL ctx, d_row_start_out or n_neighbours_out; a negative size or cap; a NULL d_tri with
 *     n_triangles > 0 or d_neighbours_out with cap_neighbours > 0; any overlap between d_tri and an output or between two
 *     outputs.  6 * n_triangles >= 2^32 (the prefixes are 32-bit) or n_vertices > 2^31 - 1: R3D_ERR_UNSUPPORTED.
 *   How: both directions of every side as a key (u << vb | v), vb = the bits of a vertex index, radix-sorted over the 2 vb + 1
 *     bits in use; the run heads are the distinct neighbours, compacted in order; a run of length 1 is a boundary edge; row_start
 *     is a lower bound per vertex.  The call synchronises (twice: for E, and before it returns).
 *
 * r3d_mesh_smooth: n_factors umbrella steps, `factors` (host, fp64) one per step.  Laplacian smoothing with `it` iterations is
 *   [lambda] * it; Taubin smoothing is [lambda, mu] * it with mu < 0 and |mu| > lambda (e.g. 0.5 and -0.53).
 *   d_row_start, d_neighbours: what r3d_mesh_adjacency wrote for this mesh (all E entries).  d_locked [n_vertices] u8 or NULL.
 *   One step with factor f, for every vertex i with degree d > 0 and (d_locked == NULL or d_locked[i] == 0), per component, in
 *   fp64 from the f32 positions widened first, the neighbours j0, j1, ... in row order (ascending index):
 *       s  = (((double)p[j0] + (double)p[j1]) + (double)p[j2]) + ...
 *       m  = s / (double)d
 *       p' = (float)((double)p[i] + f * (m - (double)p[i]))          no fused multiply-add, correctly rounded division
 *   Every other vertex keeps its bits.  Positions are rounded to f32 once per step, and every vertex of a step reads the previous
 *   step's positions (Jacobi, never in place).  NaN and infinities propagate as the arithmetic says; there is no special case.
 *   n_factors == 0 copies d_xyz_in to d_xyz_out.  n_vertices == 0 does nothing.  d_neighbours is read only for vertices with a
 *   degree > 0 (it may be NULL for a mesh without edges).  d_xyz_in is not modified.
 *   R3D_ERR_INVALID, nothing written: a NULL ctx; n_vertices < 0; n_factors outside [0, 4096]; NULL factors with n_factors > 0; a
 *     factor that is not finite; a NULL position pointer with n_vertices > 0; a NULL d_row_start with steps to do; d_xyz_out
 *     overlapping d_xyz_in, d_row_start, d_neighbours or d_locked.  n_vertices > 2^31 - 1: R3D_ERR_UNSUPPORTED.
 *   How: one lane per vertex, one launch per step, no atomics, vector stores; the intermediate positions ping-pong between two
 *     arrays of the context's workspace: only the first step reads d_xyz_in and only the last writes d_xyz_out.  ASYNCHRONOUS on
 *     the context's stream (`factors` has been read when the call returns).
 *
 * r3d_mesh_vertex_normals: area-weighted vertex normals of the mesh as it stands.
 *   For vertex i, s starts at (+0, +0, +0); every valid triangle t in ASCENDING t, and in it every corner c = 0, 1, 2 that names
 *   i, adds the unnormalised face normal of t = (a, b, c) in fp64 from the f32 positions widened first, without fused multiply-add:
 *       e1 = p[b] - p[a],  e2 = p[c] - p[a]
 *       s.x += e1.y * e2.z - e1.z * e2.y;   s.y += e1.z * e2.x - e1.x * e2.z;   s.z += e1.x * e2.y - e1.y * e2.x
 *   (a triangle that names i twice adds twice; a degenerate triangle adds exactly zero).  len = sqrt((s.x^2 + s.y^2) + s.z^2),
 *   correctly rounded.  If 0 < len < inf the row is (float)(s / len) per component; otherwise it is row i of d_fallback, bits
 *   kept, or (0, 0, 0) with d_fallback == NULL.  The winding of r3d_tsdf_extract_mesh faces the cameras, so these normals agree
 *   in sign with the TSDF normals they replace.
 *   R3D_ERR_INVALID, nothing written: a NULL ctx; a negative size; a NULL d_tri with n_triangles > 0, d_xyz or d_normals_out with
 *     n_vertices > 0; d_normals_out overlapping an input.  The size limits of r3d_mesh_adjacency: R3D_ERR_UNSUPPORTED.
 *   How: the incidence list (v << 32 | 3 t + c), sorted on the v bits alone by the stable radix sort, keeps t ascending; a lane per
 *     vertex finds its run by lower bound.  No count comes back: ASYNCHRONOUS on the context's stream.
 * The three calls keep their workspace (16 bytes per side or corner key, 24 per vertex) in the context, apart from the scratch
 *   other calls share: results do not depend on what ran before on the context. */
int r3d_mesh_adjacency(r3d_ctx* ctx, const int32_t* d_tri, int64_t n_triangles, int64_t n_vertices, uint32_t* d_row_start_out,
                       uint32_t* d_neighbours_out, int64_t cap_neighbours, uint8_t* d_boundary_out, int64_t* n_neighbours_out);
int r3d_mesh_smooth(r3d_ctx* ctx, const float* d_xyz_in, float* d_xyz_out, int64_t n_vertices, const uint32_t* d_row_start,
                    const uint32_t* d_neighbours, const uint8_t* d_locked, const double* factors, int n_factors);
int r3d_mesh_vertex_normals(r3d_ctx* ctx, const float* d_xyz, int64_t n_vertices, const int32_t* d_tri, int64_t n_triangles,
                            const float* d_fallback, float* d_normals_out);

/* ---- TSDF ray casting (csrc/r3d_tsdf_raycast.hip; the volume above seen from a camera: the depth, surface-point and normal image
 * the model predicts for a pose -- the third leg of integrate / ray cast / register; this text is the specification).  A ray-cast
 * vertex and normal map is a target cloud with normals for r3d's point-to-plane ICP (frame-to-model registration), and the depth
 * map is a hole-filled raster that integrates back.  Every output bit is a chain of IEEE f32 operations in the order written
 * here: no fused multiply-add, correctly rounded division and square root, f32 denormals kept, independent of launch geometry and
 * of how the views are split into launches.
 * Pose, per view: h_pose_w2c holds the 12-double world -> camera rows r3d_tsdf_integrate takes (R row-major, t).  The host
 *   computes the camera centre in double, in this order: C_k = -((R[0][k] t0 + R[1][k] t1) + R[2][k] t2), then rounds R (9) and
 *   C (3) once to f32.  The intrinsics are the camera's, rounded to f32.
 * Ray of pixel (row vi, column ui):
 *     x = ((float) ui - cx) / fx;  y = ((float) vi - cy) / fy
 *     len = sqrtf((x x + y y) + 1.0f);  n = (x / len, y / len, 1.0f / len)      the unit direction in the camera frame
 *     dw_k = (R[0][k] n.x + R[1][k] n.y) + R[2][k] n.z                          the direction in the world
 *   t is Euclidean distance along the ray: p(t)_a = C_a + t * dw_a.
 * Sample domain: the box of voxel centres, lo_a = o_a + 0.5f * vs, hi_a = o_a + ((float) (n_a - 1) + 0.5f) * vs.  Slab test per
 *   axis a = x, y, z from tmin = (float) t_near, tmax = (float) t_far: if dw_a == 0 the ray misses unless lo_a <= C_a <= hi_a;
 *   otherwise q1 = (lo_a - C_a) / dw_a, q2 = (hi_a - C_a) / dw_a, tmin = fmaxf(tmin, fminf(q1, q2)),
 *   tmax = fminf(tmax, fmaxf(q1, q2)).  The ray misses unless tmin <= tmax.  A volume with any n_a == 1 has no cell: every
 *   pixel is a miss.
 * Sample at t: ivs = 1.0f / vs (once);  g_a = (p_a - o_a) * ivs - 0.5f;  i_a = floorf(g_a);  f_a = g_a - i_a.  The sample is
 *   invalid unless 0 <= i_a <= n_a - 2 for all axes (compared as floats; NaN fails; where (float) (n_a - 2) is inexact, n_a >
 *   2^24 + 2, the integer i_a <= n_a - 2 must hold too) and all eight voxels i + d, d in {0, 1}^3, have w >= mw = (float)
 *   min_weight.  Otherwise it is the trilinear value, x first, then y, then z, with T0 / T1 the tsdf of the x pair:
 *     c[jy][jz] = T0 + f_x * (T1 - T0);  b[jz] = c[0][jz] + f_y * (c[1][jz] - c[0][jz]);  S = b[0] + f_z * (b[1] - b[0])
 * March: s = (float) step.  For k = 0, 1, ..., 65536: t_k = tmin + (float) k * s; the loop stops, and the pixel is a miss, unless
 *   t_k <= tmax.  The first k >= 1 at which sample k-1 and sample k are both valid with A = S_(k-1) > 0 and B = S_k <= 0 is the
 *   hit; nothing else ends the march.  On the hit: r = A / (A - B);  t* = t_(k-1) + r * s.
 * Hit point: one more sample at t*; invalid -> miss.  The gradient is analytic, from that cell's eight corners: for axis a with
 *   the other two axes (b, c) in ascending order, D[jb][jc] = T(a=1, jb, jc) - T(a=0, jb, jc);
 *   e[jc] = D[0][jc] + f_b * (D[1][jc] - D[0][jc]);  G_a = e[0] + f_c * (e[1] - e[0]).
 *   L = sqrtf((G_x G_x + G_y G_y) + G_z G_z); the pixel is a miss unless L > 0.  On a hit:
 *     depth = t* * n.z  (z-depth, the quantity the integrated rasters hold);  vertex_a = C_a + t* * dw_a;  normal_a = G_a / L
 *   (towards the camera side, like the surface points' normals).
 * Miss: depth = 0.0f ("no measurement": a ray-cast raster integrates back without special cases); the vertex and the normal row
 *   are three words of 0x7FC00000 -- a NaN marks a missing row, a point at the world origin is a legitimate point.
 * d_depth_out: [n_views][H][W] f32; d_vertex_out, d_normal_out: [n_views][H][W][3] f32, world coordinates.  Any of the three may
 *   be NULL; with all three NULL the call is a valid no-op.  Asynchronous on the ctx stream (the pose rows are copied before it
 *   returns; R3D_TSDF_CHUNK views per launch).  The volume is not modified; no byte outside the three outputs' extents is written.
 * R3D_ERR_INVALID, nothing written: NULL volume or camera, a camera of another ctx, n_views < 0, NULL poses with n_views > 0,
 *   min_weight or step not > 0 and finite in f32, t_near not finite or < 0, t_far not > t_near (+inf is allowed), an output
 *   overlapping another output or the volume, a march that could pass the loop bound -- vs * sqrt((nx-1)^2 + (ny-1)^2 +
 *   (nz-1)^2) / s >= 65536, in double from the f32 values -- and the raster-size limits of r3d_tsdf_integrate.
 *   n_views == 0 -> R3D_OK. */
int r3d_tsdf_raycast(r3d_tsdf* vol, const r3d_camera* cam, int n_views, const double* h_pose_w2c, double min_weight, double step,
                     double t_near, double t_far, float* d_depth_out, float* d_vertex_out, float* d_normal_out);

/* ---- TSDF colour (csrc/r3d_tsdf_color.hip; the volume above fed from RGBD: colour images are integrated next to the depth rasters
 * and the surface points -- which are the mesh's vertices -- come back with a colour each; this text is the specification).  A
 * volume without colour is untouched by anything here: same storage, same kernels, same bits.
 * Storage: a volume made by r3d_tsdf_create_rgb (arguments, errors and R3D_ERR_NOMEM as r3d_tsdf_create) owns a second plane,
 *   separate from the float2 array, whose layout and device view (r3d_tsdf_volume) stay as they are: one uint32[4] {sum_r, sum_g,
 *   sum_b, n} per voxel at the same linear index, 16 bytes, 16-byte aligned.  Zero bytes = fresh; r3d_tsdf_reset clears both planes.
 * Integration: d_rgb is [n_frames][H][W][3] uint8 in R, G, B order (the layout r3d_fuse_frames_rgb takes).  Frame f touches a
 *   voxel exactly when the depth rule of "TSDF volume" accepts it -- the same tests at the same pixel (vi, ui) -- and then updates
 *   tsdf and w exactly as written there AND adds the three bytes rgb[f][vi][ui][0..2] to sum_r, sum_g, sum_b and 1 to n, in uint32
 *   arithmetic.  The tsdf / weight plane is bit-identical to what r3d_tsdf_integrate makes of the same depth and poses.  The
 *   plane holds integers, so it does not depend on the order of the frames or on how they are split into calls; n == w for fewer
 *   than 2^24 frames (w is an f32 and stops counting there; the sums and n wrap modulo 2^32, the sums from 2^24 frames of 255 on).
 *   r3d_tsdf_integrate_rgb is asynchronous (same pose ring, R3D_TSDF_CHUNK frames per launch); r3d_tsdf_integrate_rgb_host uploads
 *   rasters and images itself, in slabs of whole frames sized for both together, and is synchronous.
 * Colour of a surface point: row k of r3d_tsdf_extract_points lies on the edge from voxel v to its neighbour u with
 *   r = A / (A - B) as specified there.  Per channel, all f32, no fused multiply-add, correctly rounded division, uint32 -> f32
 *   conversions rounding to nearest even:
 *     mv = (float) sum_v / (float) n_v;  mu = (float) sum_u / (float) n_u      (a mean is 0.0f where n == 0: no division by zero is
 *                                                                              specified; a valid voxel has w >= 1, hence n >= 1)
 *     m  = mv + r * (mu - mv);  q = fminf(fmaxf(floorf(m + 0.5f), 0.0f), 255.0f)
 *   The row is the word r | g << 8 | b << 16 (what r3d_fuse_frames_rgb writes).  Colour row k belongs to point row k: same count,
 *   same order, same cap rule -- *n_out is the true count, always; at most cap words are written and nothing beyond them.  The
 *   mesh's vertices are those rows, so the same call colours the mesh.  r3d_tsdf_extract_colors synchronises.
 * r3d_tsdf_colors: the device view of the plane ([n_voxels][4] uint32), valid until destroy; either out-pointer may be NULL.
 * R3D_ERR_INVALID, nothing written: a colour call (r3d_tsdf_integrate_rgb, _rgb_host, r3d_tsdf_colors, r3d_tsdf_extract_colors) on
 *   a volume without the plane; r3d_tsdf_integrate / _host on a volume WITH the plane (n and w would part), whatever n_frames;
 *   NULL d_rgb / h_rgb with n_frames > 0; and the argument errors of r3d_tsdf_integrate and r3d_tsdf_extract_points.
 *   n_frames == 0 -> R3D_OK. */
int r3d_tsdf_create_rgb(r3d_ctx* ctx, const double* h_origin, double voxel_size, int nx, int ny, int nz, double sdf_trunc,
                        r3d_tsdf** out);
int r3d_tsdf_integrate_rgb(r3d_tsdf* vol, const r3d_camera* cam, const void* d_depth, int depth_dtype, int n_frames,
                           double depth_scale, const double* h_pose_w2c, const uint8_t* d_rgb);
int r3d_tsdf_integrate_rgb_host(r3d_tsdf* vol, const r3d_camera* cam, const void* h_depth, int depth_dtype, int n_frames,
                                double depth_scale, const double* h_pose_w2c, const uint8_t* h_rgb);
int r3d_tsdf_colors(r3d_tsdf* vol, uint32_t** d_sums_out, int64_t* n_voxels_out);
int r3d_tsdf_extract_colors(r3d_tsdf* vol, double min_weight, uint32_t* d_rgba_out, int64_t cap, int64_t* n_out);

/* ---- TSDF from an oriented cloud (csrc/r3d_tsdf_cloud.hip; NOT IN THE REFERENCE -- the way from a fused, cleaned cloud with
 * oriented normals (r3d_normals_knn) to a surface: the volume above is filled with the signed distance to the tangent plane of
 * the NEAREST cloud point (Hoppe et al. 1992), after which the mesh, the surface points, ray casting and colour work unchanged;
 * this text is the specification).  Every output bit is a chain of IEEE f32 operations in the order written here: no contraction
 * except where fmaf is written, correctly rounded division, f32 denormals kept.
 * Inputs: a volume; an r3d_nn_index built over the cloud's n points (same ctx as the volume); d_normals [n][3] f32 in the cloud's
 *   ORIGINAL row order; d_rgba [n] u32 words r | g << 8 | b << 16, for a volume created with colour and only for one.
 * For every voxel (x, y, z):
 *     c    = o + ((float) idx + 0.5f) * vs                                 per axis (the volume's own centre rule)
 *     j,d2 = the nearest cloud point of c under r3d_icp_nn's rule          d2 = fmaf(dz,dz, fmaf(dy,dy, dx*dx)) with dx = c.x - p.x ...;
 *                                                                          lowest index wins exact ties; non-finite pairs never win
 *     skip unless d2 <= tr * tr                                            (an f32 product; a voxel without a finite pair has d2 = +inf)
 *     n    = normals[j];  skip unless all three are finite and not all are zero
 *     s    = ((c.x - p.x) * n.x + (c.y - p.y) * n.y) + (c.z - p.z) * n.z   p = points[j]
 *     tn   = fmaxf(-1.0f, fminf(1.0f, s / tr))                             (fminf / fmaxf return the other operand of a NaN: an s that
 *                                                                          overflowed to NaN gives 1)
 *     w1   = w + 1.0f;  tsdf = (tsdf * w + tn) / w1;  w = w1               the update of "TSDF volume": a cloud counts as ONE frame
 *     colour (with d_rgba): r, g, b of rgba[j] are added to sum_r, sum_g, sum_b and 1 to n, as r3d_tsdf_integrate_rgb adds a pixel
 *   The normals are used as given: unit length is the caller's business (a longer normal clamps earlier).  The winner alone decides:
 *   a voxel whose nearest point has a zero or non-finite normal is skipped, not handed to the runner-up.  A skipped voxel keeps
 *   every bit it had.  The result is DEFINED by brute force over all voxels and all points: it does not depend on launch geometry,
 *   on how the implementation limits the work to the band of voxels within tr of the cloud, or on its chunking (tuning key
 *   "tsdf_cloud_chunk": blocks of 4 x 4 x 4 voxels per chunk, 0 = default).  Calls compose with each other and with
 *   r3d_tsdf_integrate*: a cloud on top of depth frames, or two clouds, are the running averages written above.
 * r3d_tsdf_integrate_cloud is asynchronous on the ctx stream unless n_touched_out != NULL: then it synchronises and reports the
 *   number of voxels updated.  (Sizing the band costs one small read-back either way.)  r3d_tsdf_integrate_cloud_host uploads
 *   h_xyz [n][3], h_normals [n][3] (and h_rgba [n]), builds and destroys an index of its own and is synchronous; n == 0 -> R3D_OK,
 *   nothing written.  The work buffers belong to the volume and go with r3d_tsdf_destroy.
 * R3D_ERR_INVALID, nothing written: NULL volume, index or normals (NULL h_xyz / h_normals with n > 0; n < 0); an index of another
 *   ctx than the volume's; d_rgba on a volume without colour; NO d_rgba on a volume WITH colour (n and w would part, as in "TSDF
 *   colour"). */
int r3d_tsdf_integrate_cloud(r3d_tsdf* vol, r3d_nn_index* index, const float* d_normals, const uint32_t* d_rgba,
                             int64_t* n_touched_out);
int r3d_tsdf_integrate_cloud_host(r3d_tsdf* vol, const float* h_xyz, const float* h_normals, const uint32_t* h_rgba, int64_t n,
                                  int64_t* n_touched_out);

/* ---- TSDF ray-cast colour (csrc/r3d_tsdf_raycast.hip; the colour image a volume with colour predicts for a pose, next to the three
 * maps of "TSDF ray casting"; this text is the specification).  r3d_tsdf_raycast_rgb is r3d_tsdf_raycast with a fourth output: the
 * ray, the slab test, the march, the hit and the hit-point sample are the ones specified there, word for word, and d_depth_out,
 * d_vertex_out and d_normal_out receive the same bits that call writes for the same arguments.  r3d_tsdf_raycast itself is as it
 * was, on volumes with colour too.
 * d_rgb_out: [n_views][H][W][3] uint8 in R, G, B order -- the layout r3d_tsdf_integrate_rgb takes, so a ray-cast image integrates
 *   back together with its ray-cast depth.  A miss writes 0, 0, 0: the depth of 0 is what marks a miss, black is a legitimate colour.
 * Colour of a hit: the cell i and the fractions f of the hit-point sample at t* (the sample the normal uses).  For each corner
 *   k = jx + 2 jy + 4 jz of the cell and each channel, all f32, no fused multiply-add, correctly rounded division, uint32 -> f32
 *   conversions rounding to nearest even:
 *     M_k = (float) sum_k / (float) n_k           (0.0f where n_k == 0, as for the surface points)
 *   interpolated in the order of the tsdf sample, x first, then y, then z, with M0 / M1 the means of the x pair:
 *     c[jy][jz] = M0 + f_x * (M1 - M0);  b[jz] = c[0][jz] + f_y * (c[1][jz] - c[0][jz]);  m = b[0] + f_z * (b[1] - b[0])
 *     q = fminf(fmaxf(floorf(m + 0.5f), 0.0f), 255.0f), stored as a byte.
 *   Like the maps, it does not depend on launch geometry or on how the views are split into launches.
 * Any of the four outputs may be NULL; with all four NULL the call is a valid no-op, and with d_rgb_out == NULL it does what
 *   r3d_tsdf_raycast does.  Asynchronous on the ctx stream (same pose ring, R3D_TSDF_CHUNK views per launch).  The volume and its
 *   colour plane are only read; no byte outside the outputs' extents is written.
 * R3D_ERR_INVALID, nothing written: every argument error of r3d_tsdf_raycast; a volume without the colour plane, whatever the
 *   pointers and n_views; d_rgb_out overlapping another output, the tsdf plane or the colour plane (and, when d_rgb_out is given,
 *   any other output overlapping the colour plane). */
int r3d_tsdf_raycast_rgb(r3d_tsdf* vol, const r3d_camera* cam, int n_views, const double* h_pose_w2c, double min_weight, double step,
                         double t_near, double t_far, float* d_depth_out, float* d_vertex_out, float* d_normal_out, uint8_t* d_rgb_out);

/* ---- TSDF tracking (csrc/r3d_track.hip; frame-to-model registration by PROJECTIVE point-to-plane ICP: the pose of a new depth
 * frame against the vertex and normal map the volume predicts -- the fourth leg of integrate / extract / ray cast / track; NOT IN
 * THE REFERENCE, this text is the specification).  The model maps are organised rasters, so the partner of a source point is one
 * projection and one gather away: no search structure is built.  All arithmetic is fp64 in the order written, no fused
 * multiply-add; the results are the same bits on every run, on every device and under every tuning.
 * Inputs: a camera (H, W and its intrinsics fx, fy, cx, cy as doubles); the new frame's maps in ITS camera frame, d_src_vertex
 *   [H][W][3] f32 (what r3d_unproject writes) and optionally d_src_normal [H][W][3] f32 (what r3d_normals_organized writes; a
 *   zero row = "no normal"; NULL = no normal gate); the model maps in WORLD coordinates, d_model_vertex and d_model_normal
 *   [H][W][3] f32, exactly what r3d_tsdf_raycast writes (a miss is three NaN words); h_model_pose_w2c, 12 doubles in
 *   r3d_tsdf_integrate's row layout: the pose the model maps were cast from (Rm row-major, tm); h_S, 16 doubles, a row-major 4x4,
 *   source camera -> world: the guess; dist_max > 0; cos_min in [-1, 1], used only when source normals are given.
 * Per source pixel i = vi W + ui with (x, y, z) its source vertex:
 *   1. reject with code -1 unless x, y, z are finite and z > 0
 *   2. M = T_total . S, every entry summed over m = 0..3 in ascending order starting from 0.0 (the loop that updates T_total in
 *      the solve); T_total is the device state's in r3d_track_iterate and the identity in r3d_track_accumulate
 *   3. p_a = ((M[a][0] x + M[a][1] y) + M[a][2] z) + M[a][3]                      the point in the world
 *   4. pm_a = ((Rm[a][0] p_0 + Rm[a][1] p_1) + Rm[a][2] p_2) + tm_a               ... in the model camera
 *   5. reject -2 unless pm_2 > 0;  u = fx (pm_0 / pm_2) + cx;  v = fy (pm_1 / pm_2) + cy;  uj = floor(u + 0.5);
 *      vj = floor(v + 0.5);  reject -2 unless 0 <= uj < W and 0 <= vj < H, compared as doubles (NaN fails)
 *   6. j = vj W + uj;  q = model vertex row j, n = model normal row j
 *   7. reject -3 unless all six are finite and n is not the zero vector
 *   8. d = p - q;  reject -4 unless (d_0 d_0 + d_1 d_1) + d_2 d_2 <= dist_max dist_max
 *   9. with source normals, ns = source normal row i: reject -5 unless ns is finite and non-zero; g_a = (M[a][0] ns_0 +
 *      M[a][1] ns_1) + M[a][2] ns_2; reject -5 unless (g_0 n_0 + g_1 n_1) + g_2 n_2 >= cos_min
 *  10. r = n_0 (p_0 - q_0) + n_1 (p_1 - q_1) + n_2 (p_2 - q_2), left to right; the pair enters the 29 sums of the point-to-plane
 *      step with weight 1: J = [p x n ; n], [0] += 1, [1] += r r, [2 + a] += J_a r, [8..28] += the upper triangle of J J^T
 *      (csrc/r3d_plane_sums.h: pair_accumulate)
 *   Per-pixel outputs, each may be NULL: d_match_out [H W] int32 = j on a match, else the reject code; d_residual_out [H W] f32 =
 *   (float) r on a match, else 0.
 * Sums: a 256-thread workgroup owns 1024 consecutive pixels; thread t takes pixels base + t + 256 k for k = 0..3 in that order;
 *   its 29 accumulators go through the 64-lane shuffle tree (offsets 32, 16, .., 1), then the workgroup's 4 waves are added in
 *   ascending order: one partial row per workgroup.  One workgroup then adds the rows -- thread t rows t, t + 256, .. in
 *   ascending order -- and reduces them the same way.  The launch shape is part of the specification.
 * r3d_track_accumulate: one pass with T_total = I; h_sums receives the 29 sums.  Synchronous.
 * r3d_track_iterate: n_iters passes enqueued back to back with no host round trip: the pass above reading T_total from d_state,
 *   then the reduction and the solve, which updates d_state exactly as r3d_icp_iterate_plane's solve does (the
 *   R3D_ICP_STATE_DOUBLES layout; r3d_icp_state_reset starts a loop).  A degenerate step (fewer than 6 pairs, or normal equations
 *   singular to working precision) sets status 1 and leaves T_total as it was.  Asynchronous.
 * r3d_tsdf_track: the whole step for one frame: r3d_tsdf_raycast of the vertex and normal map at the guess (min_weight, step,
 *   t_near, t_far as there); r3d_unproject of the depth raster (d_depth: [H][W] of depth_dtype, depth_scale) and, when
 *   cos_min > -1, its r3d_normals_organized (max_jump; the origin as viewpoint) -- with cos_min == -1 every angle passes, so no
 *   source normals are computed or asked for; a state reset; r3d_track_iterate with the guess as the model pose and S = its
 *   inverse, in double on the host: S[a][b] = R[b][a], S[a][3] = -((R[0][a] t_0 + R[1][a] t_1) + R[2][a] t_2); the state is read
 *   back (synchronises).  With M = T_total . S (the loop of step 2): R_out = the transpose of M's rotation block,
 *   t_out_a = -((R_out[a][0] M[0][3] + R_out[a][1] M[1][3]) + R_out[a][2] M[2][3]); h_pose_out = 12 doubles in
 *   r3d_tsdf_integrate's row layout, world -> camera: it feeds straight back into r3d_tsdf_integrate.  h_info_out = 4 doubles:
 *   pairs and rms of r seen by the last step, status, steps solved.  status 1 = some step was degenerate: h_pose_out is then the
 *   guess, bit for bit.  The maps and the state live in the context's scratch: nothing is allocated per call after the first.
 *   A volume with the colour plane is accepted (the volume is only read).
 * R3D_ERR_INVALID, nothing written: NULL ctx / volume / camera, a camera of another ctx, a NULL required pointer (every map but
 *   d_src_normal, the poses, h_sums, d_state, h_pose_out, h_info_out), dist_max not > 0 and finite, cos_min outside [-1, 1] or
 *   NaN, n_iters < 0 or > R3D_ICP_STATE_DOUBLES - R3D_ICP_STATE_HISTORY (what the history holds), a device output overlapping an
 *   input map or another output (r3d_tsdf_track: a host output overlapping the guess or the other output), a raster of
 *   2^31 - 1024 pixels or more; r3d_tsdf_track also: a non-finite guess, max_jump < 0, and the argument errors of
 *   r3d_tsdf_integrate (depth) and r3d_tsdf_raycast.  Coarse-to-fine passes over an image pyramid: r3d_tsdf_track_pyramid
 *   ("Depth pyramid", below).  Photometric (colour) terms: "TSDF colour tracking", further below (one level; not in the pyramid). */
int r3d_track_accumulate(r3d_ctx* ctx, const r3d_camera* cam, const float* d_src_vertex, const float* d_src_normal,
                         const float* d_model_vertex, const float* d_model_normal, const double* h_model_pose_w2c, const double* h_S,
                         double dist_max, double cos_min, double* h_sums, int32_t* d_match_out, float* d_residual_out);
int r3d_track_iterate(r3d_ctx* ctx, const r3d_camera* cam, const float* d_src_vertex, const float* d_src_normal,
                      const float* d_model_vertex, const float* d_model_normal, const double* h_model_pose_w2c, const double* h_S,
                      double dist_max, double cos_min, int n_iters, double* d_state);
int r3d_tsdf_track(r3d_tsdf* vol, const r3d_camera* cam, const void* d_depth, int depth_dtype, double depth_scale,
                   const double* h_pose_guess_w2c, double min_weight, double step, double t_near, double t_far, float max_jump,
                   double dist_max, double cos_min, int n_iters, double* h_pose_out, double* h_info_out);

/* ---- Depth pyramid (csrc/r3d_pyramid.hip, and the coarse-to-fine driver in csrc/r3d_track.hip; NOT IN THE REFERENCE, this text is
 * the specification).  Projective association pairs a source point with the model pixel it lands on, so a few pixels of image
 * motion already pair across surfaces; tracking therefore starts on a halved raster, where the same motion is fewer pixels, and
 * hands its pose down level by level.
 * The level camera.  Pixel ui of a camera looks along x = (ui - cx) / fx: pixel centres sit at integer coordinates.  A coarse
 *   pixel u' stands for the fine pixels 2 u' and 2 u' + 1, whose centre is 2 u' + 0.5.  r3d_camera_half: H' = H >> 1, W' = W >> 1
 *   (an odd last row or column is dropped); fx' = 0.5 fx, fy' = 0.5 fy, cx' = 0.5 (cx - 0.5), cy' = 0.5 (cy - 0.5), in double, in
 *   that order; the camera is created in cam's context as r3d_camera_create does (destroy it with r3d_camera_destroy).
 *   R3D_ERR_INVALID with *out untouched for a NULL argument, H < 2 or W < 2.
 * r3d_depth_half.  d_in holds the depth of pixel (v, u) at d_in[(v width + u) in_stride]: in_stride 1 is an f32 depth raster,
 *   in_stride 3 the z column of a vertex map (the caller passes vertex + 2).  d_out is [height >> 1][width >> 1] f32.  All of it is
 *   f32, in the order written, no fused multiply-add, correctly rounded division, f32 denormals kept:
 *   1. a depth is valid iff it is finite and > 0
 *   2. for output pixel (v', u') the block is the four inputs (2v', 2u'), (2v', 2u' + 1), (2v' + 1, 2u'), (2v' + 1, 2u' + 1), in that
 *      order
 *   3. m = the minimum of the block's valid depths; with no valid depth the output is 0.0f ("no measurement", as a ray-cast miss)
 *   4. a valid depth d is included iff d - m <= max_jump: foreground wins -- a block that straddles a depth edge averages the near
 *      side only and never invents a depth between two surfaces
 *   5. s = 0.0f, then s += d over the included depths in block order; the output is s / (float) count
 *   max_jump >= 0; +inf is allowed and includes every valid depth.  The result does not depend on the launch geometry.
 *   Asynchronous on the ctx stream; nothing outside d_out's extent is written.  One lane per output pixel, one launch per level.
 *   R3D_ERR_INVALID, nothing written: a NULL pointer, in_stride not 1 or 3, height < 2 or width < 2, max_jump NaN or negative, the
 *   input extent (((height width - 1) in_stride + 1) floats from d_in) overlapping the output, a raster of 2^31 - 1024 pixels or
 *   more.
 * r3d_tsdf_track_pyramid: r3d_tsdf_track coarse to fine.  cams[0] is the frame's camera; cams[l] must have the size
 *   r3d_camera_half gives from cams[l - 1], in the same context (its intrinsics are the caller's: normally r3d_camera_half's; they
 *   are not checked).  1 <= n_levels <= R3D_TRACK_MAX_LEVELS; h_iters[l] >= 0 iterations at level l, their sum at most
 *   R3D_ICP_STATE_DOUBLES - R3D_ICP_STATE_HISTORY.  Every other argument means what it means in r3d_tsdf_track.
 *   Source side: the level-0 vertex map is r3d_unproject of d_depth, as there.  The level-l depth, l >= 1, is r3d_depth_half of the
 *   level l - 1 depth with max_jump (level 0's is read from the z column of its vertex map, in_stride 3, whatever dtype the frame
 *   came in); the level-l vertex map is r3d_unproject of that f32 raster with cams[l] and scale 1; with cos_min > -1 each level's
 *   normals are r3d_normals_organized of its vertex map with max_jump.
 *   Model side: for every level with h_iters[l] > 0 the vertex and normal map are r3d_tsdf_raycast of the volume AT THE GUESS with
 *   cams[l] (min_weight, step, t_near, t_far as given): ray-cast, not down-sampled, so every level's maps are what "TSDF ray
 *   casting" specifies.  The model pose of every level is the guess, and S, its inverse, is the same for all levels.
 *   Loop: one state reset; then from l = n_levels - 1 down to 0, h_iters[l] passes of r3d_track_iterate's pass at that level's
 *   camera and maps ON THE SAME STATE: T_total, the iteration count and the rms history carry across levels.  A level with 0
 *   iterations is skipped.  Everything is enqueued back to back; the state is read once at the end (synchronises).  Status is
 *   sticky: a degenerate step at any level gives status 1 and h_pose_out = the guess, bit for bit.
 *   h_pose_out and h_info_out as in r3d_tsdf_track (the iteration count is the total over all levels).  h_rms_out may be NULL;
 *   otherwise it receives sum(h_iters) doubles: the state's rms history in execution order (coarsest level first).
 *   With n_levels == 1 the call returns the bytes r3d_tsdf_track returns with n_iters = h_iters[0] (the two share one body).
 *   All levels' maps, the depth rasters and the state live in the context's scratch (4/3 of the one-level footprint plus the
 *   depth rasters): nothing is allocated per call after the first.
 *   R3D_ERR_INVALID, nothing written, all checked before anything is enqueued: every argument error of r3d_tsdf_track; n_levels out
 *   of range; NULL cams, cams[l] or h_iters; a level camera of the wrong size or of another context; a negative iteration count;
 *   an iteration sum over the limit; h_rms_out overlapping another host argument. */
#define R3D_TRACK_MAX_LEVELS 8
int r3d_camera_half(const r3d_camera* cam, r3d_camera** out);
int r3d_depth_half(r3d_ctx* ctx, const float* d_in, int in_stride, int height, int width, float max_jump, float* d_out);
int r3d_tsdf_track_pyramid(r3d_tsdf* vol, const r3d_camera* const* cams, int n_levels, const int* h_iters, const void* d_depth,
                           int depth_dtype, double depth_scale, const double* h_pose_guess_w2c, double min_weight, double step,
                           double t_near, double t_far, float max_jump, double dist_max, double cos_min, double* h_pose_out,
                           double* h_info_out, double* h_rms_out);

/* ---- TSDF colour tracking (csrc/r3d_photo.hip and the sibling kernel and drivers in csrc/r3d_track.hip; NOT IN THE REFERENCE, this
 * text is the specification).  Point-to-plane ICP alone is blind wherever the geometry leaves a freedom open -- sliding along a
 * corridor, over one wall or a floor: r3d_tsdf_track then reports status 1.  A volume with colour predicts a colour image for the
 * guess (r3d_tsdf_raycast_rgb), and the frame brings its own: the difference of their intensities constrains what the planes do not.
 * The linearised photometric residual has the Jacobian shape of the geometric one -- with a the image gradient pulled back to a
 * world-space 3-vector, J = [p x a ; a] where the plane term has [p x n ; n] -- so a photometric pair enters the same 6 x 6 normal
 * equations through the same arithmetic; the reduction, the solve and the ICP state are the ones of "TSDF tracking".  Nothing of
 * "TSDF tracking" changes: r3d_track_accumulate, r3d_track_iterate, r3d_tsdf_track and r3d_tsdf_track_pyramid return the bits they
 * returned.  Not yet timed on a card.
 * r3d_intensity_map: one launch, one lane per pixel, asynchronous on the ctx stream.  d_rgb is [H][W][3] uint8 in R, G, B order (the
 *   layout of r3d_tsdf_integrate_rgb and r3d_tsdf_raycast_rgb).  d_valid is a float raster read as d_valid[(v W + u) valid_stride],
 *   valid_stride 1 or 3 as in r3d_depth_half: 1 reads a depth raster (the model side passes the ray-cast depth), 3 the z column of a
 *   camera-frame vertex map (the source side passes src_vertex + 2).  A pixel is valid iff its value is finite and > 0.
 *   max_jump >= 0; +inf is allowed.  Outputs, either may be NULL (both NULL: a valid no-op): d_intensity_out [H][W] f32;
 *   d_packed_out [H][W][4] f32 {I, gx, gy, 0}, 16-byte aligned so that one tap is one 16-byte load.  All f32, in the order written,
 *   no fused multiply-add:
 *     I  = (0.299f R + 0.587f G) + 0.114f B, in 0..255; NaN where the pixel is invalid
 *     gx = 0.5f (I(u + 1) - I(u - 1)); NaN if u is 0 or W - 1, if the pixel or either neighbour is invalid, or if
 *          |d(u +- 1) - d(u)| > max_jump for either neighbour (d = the validity raster's value): no gradient is taken across a depth
 *          edge
 *     gy   the same along v
 *   The neighbours' intensities are recomputed from their bytes (there is no second pass); the result does not depend on the launch
 *   geometry; nothing outside the outputs' extents is written.
 *   R3D_ERR_INVALID, nothing written: a NULL required pointer (ctx, d_rgb, d_valid), valid_stride not 1 or 3, H < 1 or W < 1,
 *   max_jump NaN or negative, d_packed_out not 16-byte aligned, an output overlapping an input (the validity extent is
 *   ((H W - 1) valid_stride + 1) floats) or the other output, a raster of 2^31 - 1024 pixels or more.
 * The association pass with a colour term has the tile of "TSDF tracking" (256 threads own 1024 consecutive pixels, thread t takes
 *   base + t + 256 k), so its launch shape is part of the specification in the same way.  Extra inputs: d_src_intensity [H][W] f32
 *   (r3d_intensity_map's first output for the frame), d_model_packed [H][W][4] f32, 16-byte aligned (its second output for the
 *   model's colour image), w_photo >= 0 finite (the weight of a photometric pair against a geometric pair's 1, in metres^2 per
 *   intensity^2), i_max > 0 finite.  Steps 1..10 are those of "TSDF tracking", word for word.  Then, for a pixel whose geometric
 *   pair was accepted (code >= 0), all in fp64, left to right, no fused multiply-add:
 *  11. with u, v, pm of step 5: u0 = floor(u), v0 = floor(v); no photometric pair unless 0 <= u0, u0 + 1 <= W - 1, 0 <= v0 and
 *      v0 + 1 <= H - 1, compared as doubles; fu = u - u0, fv = v - v0
 *  12. the four packed model taps t00 = (v0, u0), t01 = (v0, u0 + 1), t10 = (v0 + 1, u0), t11 = (v0 + 1, u0 + 1); for each of I, gx,
 *      gy: top = t00 + fu (t01 - t00); bot = t10 + fu (t11 - t10); val = top + fv (bot - top).  A NaN tap makes val NaN: that is
 *      the validity test, there is no separate mask
 *  13. rI = Im - Is, Is = the source intensity of pixel i
 *  14. b0 = (gx fx) / pm_2;  b1 = (gy fy) / pm_2;  b2 = -((gx fx) pm_0 + (gy fy) pm_1) / (pm_2 pm_2);
 *      a_c = (Rm[0][c] b0 + Rm[1][c] b1) + Rm[2][c] b2: Rm^T b, the gradient as a world-space vector
 *  15. no photometric pair unless rI, a_0, a_1, a_2 are all finite and |rI| <= i_max
 *  16. with w = w_photo and J = [p x a ; a]: [2 + k] += (w J_k) rI; [8..28] += the upper triangle of (w J_k) J_l (pair_accumulate's
 *      order); [29] += 1; [30] += rI rI
 *   Sums [0] and [1] stay purely geometric -- the pair count and sum r^2 in metres -- so the state's pairs, rms and rms history and
 *   the n >= 6 test of the solve mean what they mean in "TSDF tracking".  31 sums, reduced as the 29 are there; the step is solved
 *   from the first 29.  Per-pixel outputs: d_match_out and d_residual_out as r3d_track_accumulate's, the same bits; d_photo_out
 *   [H W] f32 = (float) rI where a photometric pair entered, NaN elsewhere.  Each may be NULL.
 * r3d_track_accumulate_rgb: r3d_track_accumulate with the colour term; h_sums receives 31 doubles.  With w_photo == 0 the first 29,
 *   the match and the residual are the bits r3d_track_accumulate gives (step 15 keeps non-finite terms out).  Synchronous.
 * r3d_track_iterate_rgb: r3d_track_iterate with the colour term, on the same R3D_ICP_STATE_DOUBLES state.  Asynchronous.
 * r3d_tsdf_track_rgb: the whole step for one frame, one level: r3d_tsdf_raycast_rgb at the guess (depth, vertex, normal, rgb);
 *   r3d_intensity_map of the model's image with the ray-cast depth as validity (stride 1, max_jump), packed output;
 *   r3d_unproject of the frame's depth; r3d_intensity_map of d_rgb ([H][W][3] uint8) with the z column of the source vertex map as
 *   validity (stride 3, max_jump), intensity output only; source normals when cos_min > -1; a state reset; n_iters passes; pose and
 *   info read back exactly as r3d_tsdf_track does (status 1 gives the guess back bit for bit).  h_info_out = 6 doubles: the four
 *   of r3d_tsdf_track, then the photometric pair count and the photometric rms sqrt([30] / [29]) the last step saw (0 with no pair
 *   or no step).  Everything lives in the context's scratch: nothing is allocated per call after the first.
 * R3D_ERR_INVALID, nothing written, all checked before anything is enqueued: every argument error of the call each extends; a NULL
 *   d_src_intensity, d_model_packed or d_rgb; a d_model_packed that is not 16-byte aligned; w_photo negative or not finite; i_max
 *   not > 0 and finite; a device output overlapping an input (the two new maps included) or another output; r3d_tsdf_track_rgb on
 *   a volume without the colour plane.
 * Deliberately not done here: a colour term in r3d_tsdf_track_pyramid (it needs a depth-consistent intensity half-sampler), and
 *   robust (Huber) weights. */
int r3d_intensity_map(r3d_ctx* ctx, const uint8_t* d_rgb, const float* d_valid, int valid_stride, int height, int width, float max_jump,
                      float* d_intensity_out, float* d_packed_out);
int r3d_track_accumulate_rgb(r3d_ctx* ctx, const r3d_camera* cam, const float* d_src_vertex, const float* d_src_normal,
                             const float* d_model_vertex, const float* d_model_normal, const double* h_model_pose_w2c, const double* h_S,
                             double dist_max, double cos_min, const float* d_src_intensity, const float* d_model_packed, double w_photo,
                             double i_max, double* h_sums, int32_t* d_match_out, float* d_residual_out, float* d_photo_out);
int r3d_track_iterate_rgb(r3d_ctx* ctx, const r3d_camera* cam, const float* d_src_vertex, const float* d_src_normal,
                          const float* d_model_vertex, const float* d_model_normal, const double* h_model_pose_w2c, const double* h_S,
                          double dist_max, double cos_min, const float* d_src_intensity, const float* d_model_packed, double w_photo,
                          double i_max, int n_iters, double* d_state);
int r3d_tsdf_track_rgb(r3d_tsdf* vol, const r3d_camera* cam, const void* d_depth, int depth_dtype, double depth_scale,
                       const uint8_t* d_rgb, const double* h_pose_guess_w2c, double min_weight, double step, double t_near, double t_far,
                       float max_jump, double dist_max, double cos_min, double w_photo, double i_max, int n_iters, double* h_pose_out,
                       double* h_info_out);

/* ---- Depth bilateral filter (csrc/r3d_bilateral.hip; NOT IN THE REFERENCE, this text is the specification).  A sensor's depth
 * carries millimetres of noise, and r3d_normals_organized differences neighbouring depths: the noise becomes degrees of normal
 * error, the cos_min gate of tracking throws pairs away and the residuals carry the rest.  The classic remedy is to track on an
 * edge-preserving smoothing of the raster and to integrate the raw one.  The weights are TABLES made once on the host, so the
 * kernel does no transcendental arithmetic and its output is reproducible bit for bit from those tables.
 * Weights (r3d_bilateral_weights; host only, no ctx, no GPU): host doubles, rounded once to f32.  r = radius.
 *   spatial[(dy + r)(2r + 1) + (dx + r)] = (float) exp(-(dx^2 + dy^2) / (2 sigma_s^2)), dx, dy in -r..r; sigma_s is in pixels
 *   range[k] = (float) exp(-0.5 t^2) with t = 3.0 k / 256.0, k in 0..255: the LEFT edge of bin k, so range[0] and the centre spatial
 *              entry are exactly 1.0f
 *   cut      = (float) (3.0 sigma_r); sigma_r is in metres
 *   inv_step = (float) (256.0 / (3.0 sigma_r))
 *   h_spatial receives (2r + 1)^2 floats, h_range R3D_BILATERAL_RANGE_BINS, h_cut and h_inv_step one each.  These are exactly the
 *   numbers r3d_depth_bilateral uses for the same (radius, sigma_s, sigma_r) (one function makes both): a restatement that takes
 *   them reproduces the device output bit for bit, whatever the last bit of a libm's exp.
 *   R3D_ERR_INVALID, nothing written: a NULL pointer, radius outside [0, R3D_BILATERAL_MAX_RADIUS], sigma_s or sigma_r not finite
 *   or not > 0 (for sigma_r: as a double, and cut and inv_step as f32 -- both must come out finite and > 0).
 * Filter (r3d_depth_bilateral).  d_in holds the depth of pixel (v, u) at d_in[(v width + u) in_stride], in_stride 1 or 3 as in
 *   r3d_depth_half: an f32 depth raster, or the z column of a vertex map (the caller passes vertex + 2).  d_out is [height][width]
 *   f32.  All arithmetic is f32, in the order written, no fused multiply-add, correctly rounded division, f32 denormals kept:
 *   1. a depth is valid iff it is finite and > 0
 *   2. output pixel (v, u) with an invalid centre depth dc is 0.0f: no holes are filled
 *   3. otherwise num = 0.0f, den = 0.0f; then for dy = -r..r (outer) and dx = -r..r (inner), in that order, with d the depth of
 *      pixel (v + dy, u + dx):
 *        skip a tap outside the raster; skip an invalid d;
 *        a = fabsf(d - dc); skip unless a <= cut;
 *        k = min(255, (int) (a * inv_step));
 *        w = spatial[dy][dx] * range[k];
 *        num = num + w * d;  den = den + w
 *   4. the output is num / den.  The centre tap always enters with w == 1, so den >= 1.
 *   Properties.  Radius 0 returns the valid inputs bit for bit (and 0.0f for the others).  Two surfaces more than cut apart never
 *   mix: no depth is invented between them.  The result depends on the pixel's own window only, not on the launch geometry or any
 *   tuning.  Asynchronous on the ctx stream; nothing outside d_out's extent is written.  The tables are uploaded through the
 *   context and kept per (radius, sigma_s, sigma_r): a repeated call uploads nothing.  One lane per output pixel, a 32 x 8 tile
 *   and its halo staged in LDS per workgroup.
 *   R3D_ERR_INVALID, nothing written: NULL ctx or pointer, in_stride not 1 or 3, height < 1 or width < 1, the argument errors of
 *   r3d_bilateral_weights, the input extent (((height width - 1) in_stride + 1) floats from d_in) overlapping the output, a raster
 *   of 2^31 - 1024 pixels or more. */
#define R3D_BILATERAL_MAX_RADIUS 8
#define R3D_BILATERAL_RANGE_BINS 256
int r3d_bilateral_weights(int radius, double sigma_s, double sigma_r, float* h_spatial, float* h_range, float* h_cut,
                          float* h_inv_step);
int r3d_depth_bilateral(r3d_ctx* ctx, const float* d_in, int in_stride, int height, int width, int radius, double sigma_s,
                        double sigma_r, float* d_out);

/* ---- Multiway registration: the information matrix and quality of a registered pair, and pose-graph optimisation
 * (csrc/r3d_reginfo.hip, csrc/r3d_posegraph.cpp; NOT IN THE REFERENCE -- the step between "register pairs" and "integrate
 * everything", for which users of this kind of pipeline call Open3D's get_information_matrix_from_point_clouds,
 * evaluate_registration, PoseGraph and global_optimization; no parity with Open3D is claimed, this text is the specification).
 *
 * r3d_registration_sums: the pair sums of a pose under test.  d_src [n_src][3] f32 is the source ALREADY MOVED by that pose
 *   (r3d_apply_T, f32); d_idx [n_src] u32 / d_d2 [n_src] f32 are what r3d_nn_index_query or r3d_icp_nn wrote for it against
 *   d_tgt [n_tgt][3] f32.  Pair k takes part iff d_idx[k] < n_tgt (the index array is data: nothing is read past the target
 *   cloud), all six coordinates of src[k] and q = tgt[d_idx[k]] are finite, and d_d2[k] <= max_d2 -- the pair AT max_d2 is in,
 *   as in r3d_icp_accumulate; a NaN d2 is out.  With q promoted to fp64, h_sums (host, R3D_REGISTRATION_SUMS doubles):
 *     [0] n = the pairs taking part, [1..3] sum q, [4..9] sum qx qx, qx qy, qx qz, qy qy, qy qz, qz qz, [10] sum (double) d2.
 *   One lane per source row, grid-stride, one accumulator set per lane, the fixed two-stage tree of r3d_icp_accumulate, no float
 *   atomics: the same input gives the same bits run to run.  Synchronous.  n_src == 0: eleven zeros, no launch.
 *   R3D_ERR_INVALID, nothing written: NULL ctx or h_sums, a NULL device pointer with n_src > 0, a negative count, n_tgt >= 2^32,
 *   max_d2 < 0 or NaN (an information matrix without a distance gate is meaningless).
 *
 * r3d_information_from_sums: pure host fp64 arithmetic, no GPU needed.  Parameter order (rotation, translation).  A small motion
 *   (w, v) moves a target point q by w x q + v = G (w, v) with G = [ -[q]x | I ]; h_info (36 doubles, row-major 6x6) =
 *     L = sum G^T G = [[ sum (|q|^2 I - q q^T),  [sum q]x ],
 *                      [ -[sum q]x,              n I      ]]
 *   with [a]x = [[0, -az, ay], [az, 0, -ax], [-ay, ax, 0]]; the diagonal of the first block is s[7] + s[9], s[4] + s[9],
 *   s[4] + s[7], every other entry one sum or its negative.  *h_fitness (may be NULL) = n / n_src, 0 when n_src == 0;
 *   *h_rmse (may be NULL) = sqrt(s[10] / n), 0 when n == 0.  NULL h_sums / h_info or n_src < 0 -> R3D_ERR_INVALID.
 *
 * r3d_posegraph_optimize: pure host fp64 arithmetic, no GPU needed.  All matrices are row-major 4x4 rigid motions [R t; 0 1];
 *   R is taken to be a rotation (the inverse used is [R^T, -R^T t]).
 *   Conventions.  The pose X_i of node i maps cloud i into the frame of cloud 0.  An edge (s, t, T) says p_t = T p_s -- the T
 *   that register_global and icp_point_to_plane(src = s, tgt = t) return -- so a consistent graph has X_s = X_t T.  The residual
 *   of an edge is xi = (w, v) of E = T^-1 X_t^-1 X_s: w the SO(3) logarithm of E's rotation (|w| <= pi), v E's translation;
 *   chi2_e = xi^T L_e xi with L_e = h_edge_info[e], symmetrised as (L + L^T) / 2.
 *   Weights.  Certain edges (h_edge_uncertain[e] == 0) have w_e = 1.  Uncertain edges have w_e = (mu / (mu + chi2_e))^2 (1 when
 *   mu + chi2_e == 0), recomputed from the current poses in every iteration -- the closed form of the line process of Choi, Zhou
 *   and Koltun (CVPR 2015) -- with mu = preference_loop_closure x max_correspondence_distance^2 x the mean of L_e[5][5] (the pair
 *   count of an information matrix made above) over the uncertain edges not yet pruned.  preference_loop_closure = +inf
 *   switches the robust weights off: every w_e = 1 and nothing is pruned.
 *   Cost.  C = sum_e w_e chi2_e, weights at the same poses: h_report[0] before the first step, h_report[1] at the end.  The
 *   step test below uses the line-process objective F = sum_e w_e chi2_e + mu (sqrt(w_e) - 1)^2 (uncertain edges: mu chi2_e /
 *   (mu + chi2_e)), which the weights minimise in closed form and which, unlike C, grows with every chi2_e; without uncertain
 *   edges, or with the robust weights off, F = C.
 *   Solver.  Levenberg-Marquardt over the 6 (n_nodes - 1) parameters of the nodes 1 .. n_nodes - 1; node 0 is fixed, its 16
 *   doubles keep their bits.  Per iteration: weights, H = sum w_e J_e^T L_e J_e and g = sum w_e J_e^T L_e xi_e (dense; J_e the
 *   derivative of xi_e by the left perturbations of X_s and X_t), (H + lambda I) d = -g by Cholesky (a failed factorisation
 *   multiplies lambda by 10 and counts as an iteration); X_i <- exp(d_i) X_i with the SE(3) exponential of d_i = (w, v); the step is
 *   kept when F falls, lambda then shrinks by max(1/3, 1 - (2 rho - 1)^3), otherwise it grows by 2, 4, 8, ... (Nielsen's rule; it
 *   starts at 1e-6 x the largest diagonal entry of H).  The loop stops when the largest |component| of d is below 1e-10 (that
 *   step is still applied when F does not rise), when a kept step changed F by less than 1e-14 F, when F is 0, or after max_iters
 *   iterations (h_report[4] = 1).  n_nodes <= R3D_POSEGRAPH_MAX_NODES = 512: the normal equations are dense (72 MB and some 1e10
 *   operations per iteration at the limit); more is R3D_ERR_INVALID.
 *   Pruning.  After the loop, uncertain edges with w_e < prune_threshold are pruned: they take no further part.  If any was
 *   pruned, the loop runs once more (again up to max_iters) over the other edges, the kept uncertain edges still weighted by
 *   the rule above; nothing is pruned after that second loop.  A node held by pruned edges alone stays where it is.
 *   Outputs.  h_poses [n_nodes][16] in / out.  h_edge_weight_out [n_edges] (may be NULL): the final w_e, 0 for pruned edges.
 *   h_report (may be NULL; R3D_POSEGRAPH_REPORT_DOUBLES doubles): [0] C at the start, [1] C at the end, [2] iterations (both
 *   loops), [3] edges pruned, [4] status: 0, or 1 when a loop ended because of max_iters, [5..7] 0.
 *   R3D_ERR_INVALID, nothing written (the poses keep their bits): n_nodes < 1 or > 512, n_edges < 0, max_iters < 0, a NULL
 *   h_poses (or edge array with n_edges > 0); a node index out of range or s == t; a non-finite value in a pose, a T, an L,
 *   max_correspondence_distance or prune_threshold; max_correspondence_distance <= 0; preference_loop_closure NaN or <= 0 (+inf
 *   is allowed); an L with |L_ab - L_ba| > 1e-9 x its largest |entry| or with a negative diagonal entry; a pose or T whose bottom
 *   row is not exactly 0 0 0 1; a node that no path of edges connects to node 0. */
#define R3D_REGISTRATION_SUMS 11
#define R3D_POSEGRAPH_MAX_NODES 512
#define R3D_POSEGRAPH_REPORT_DOUBLES 8
int r3d_registration_sums(r3d_ctx* ctx, const float* d_src, int64_t n_src, const float* d_tgt, int64_t n_tgt, const uint32_t* d_idx,
                          const float* d_d2, float max_d2, double* h_sums);
int r3d_information_from_sums(const double* h_sums, int64_t n_src, double* h_info, double* h_fitness, double* h_rmse);
int r3d_posegraph_optimize(int n_nodes, double* h_poses, int n_edges, const int32_t* h_edge_nodes, const double* h_edge_T,
                           const double* h_edge_info, const uint8_t* h_edge_uncertain, double max_correspondence_distance,
                           double preference_loop_closure, double prune_threshold, int max_iters, double* h_edge_weight_out,
                           double* h_report);

/* ---- Coloured ICP (csrc/r3d_color_icp.hip; NOT IN THE REFERENCE -- the colour-assisted cloud-to-cloud registration of Park, Zhou and
 * Koltun (ICCV 2017), which users of this kind of pipeline know as Open3D's registration_colored_icp; no parity with Open3D is claimed,
 * this text is the specification).  Point-to-plane ICP between two unorganised clouds is undefined where the overlap is one wall, a
 * floor, two parallel walls or a corridor.  Clouds that carry colour (r3d_fuse_frames_rgb, r3d_voxelgrid_extract,
 * r3d_tsdf_extract_colors: words r | g << 8 | b << 16) constrain the open freedoms: every target point gets the gradient of its
 * intensity over its tangent plane, and a matched pair then carries a photometric residual next to the geometric one.  Its Jacobian
 * has the plane term's shape, J = [p x a ; a] with a the tangent gradient, so it enters the 6 x 6 normal equations through the
 * arithmetic of the tracking calls' colour term (r3d_track_accumulate_rgb); the reduction, the solve and the ICP state are the ones of r3d_icp_iterate_plane.  Nothing
 * existing changes.  Not yet timed on a card.
 * All arithmetic below is fp64 unless it says f32, left to right as written, no fused multiply-add; each stored value is rounded once.
 *
 * r3d_color_gradient_knn: asynchronous; one lane per point i of the index's own cloud P (n rows, original order), 3 <= k <= 32.
 *   d_normals [n][3] f32 (r3d_normals_knn's output, or any unit normals), d_rgba [n] u32.
 *   Neighbourhood: N_i = row i of r3d_nn_index_knn_self(index, k) -- the exact (d2, j) order, ties by row, tails dropped -- cut, when
 *     radius > 0, at the first entry with d2 > (float)((double) radius * radius) (radius <= 0: no cut).  c_i = |N_i| goes to
 *     d_count_out [n] u32 (may be NULL).  The lists are stored in HBM by r3d_nn_index_knn_self (a grow-only buffer of the context) and read back.
 *   Intensity (f32): R = w & 255, G = (w >> 8) & 255, B = (w >> 16) & 255 of the colour word w, each converted to f32;
 *     I = (0.299f R + 0.587f G) + 0.114f B, in 0..255 -- r3d_intensity_map's rule.  The alpha byte is never read.  I_i goes to
 *     d_intensity_out [n] f32 for EVERY row, whatever becomes of its gradient.
 *   Gradient: with n = (double) d_normals[i], p_i = (double) P[i], and A_00, A_01, A_02, A_11, A_12, A_22, b_0, b_1, b_2 = 0.0, for each
 *     entry j of N_i in list order:
 *       e_a = (double) p_j,a - p_i,a;  h = (e_0 n_0 + e_1 n_1) + e_2 n_2;  t_a = e_a - h n_a;  dI = (double) I_j - (double) I_i
 *       A_ab += t_a t_b for ab in 00, 01, 02, 11, 12, 22;  b_a += t_a dI
 *     then the tangent-plane constraint with c = (double) c_i, c2 = c c:  A_ab += (c2 n_a) n_b for the same six ab.  Adjugate:
 *       C00 = A_11 A_22 - A_12 A_12;  C01 = A_02 A_12 - A_01 A_22;  C02 = A_01 A_12 - A_02 A_11
 *       C11 = A_00 A_22 - A_02 A_02;  C12 = A_01 A_02 - A_00 A_12;  C22 = A_00 A_11 - A_01 A_01
 *       det = (A_00 C00 + A_01 C01) + A_02 C02;  tr = (A_00 + A_11) + A_22
 *       g_0 = ((C00 b_0 + C01 b_1) + C02 b_2) / det;  g_1 = ((C01 b_0 + C11 b_1) + C12 b_2) / det;
 *       g_2 = ((C02 b_0 + C12 b_1) + C22 b_2) / det
 *     d_grad_out [n][3] f32 = (float) g, in intensity per length unit.  The constraint row pins g . n to 0 up to rounding.
 *   No gradient = a row of three NaN (validity needs no mask, as for r3d_intensity_map's gradients): a normal that is the zero vector or has a
 *     non-finite component; a point with a non-finite coordinate; c_i < 3; det not finite; det not above the conditioning floor,
 *     i.e. unless det > R3D_COLOR_GRADIENT_FLOOR ((tr tr) tr).  With collinear tangent offsets det is rounding noise, up to a few
 *     1e-16 tr^3 when the normal is oblique to the axes; the floor 1e-14 sits well above that.  The constraint row weighs c2 (a pure
 *     number) against offsets in length^2, so the ratio depends on the cloud's unit: a regular neighbourhood of spacing s has
 *     det / tr^3 of about s^4 / c2 once s^2 << c_i, and passes down to s of about a thousandth of the unit.
 *   R3D_ERR_INVALID, nothing written: a NULL index, d_normals, d_rgba, d_intensity_out or d_grad_out; k outside [3, 32]; radius NaN; an
 *     output overlapping another output, the normals, the colours or the index's cloud.
 *
 * r3d_icp_color_accumulate: the coloured sibling of r3d_icp_plane_accumulate without trimming; synchronous, h_sums (host) receives
 *   R3D_COLOR_ICP_SUMS = 31 doubles.  Inputs: d_src [n_src][3] f32 the MOVED source and d_src_intensity [n_src] f32 in the same order;
 *   d_tgt [n_tgt][3] f32 with d_tgt_normals [n_tgt][3] f32, d_tgt_intensity [n_tgt] f32 and d_tgt_grad [n_tgt][3] f32 (the two outputs
 *   above); d_idx [n_src] u32 / d_d2 [n_src] f32 from the NN index; max_d2 (f32; < 0: no gate, d_d2 may then be NULL); w_photo >= 0
 *   finite (the weight of a photometric pair against a geometric pair's 1, in length^2 per intensity^2); i_max > 0 finite.
 *   Geometric pair k = (p = src[k], q = tgt[idx[k]], n = tgt_normals[idx[k]]), exactly the untrimmed plane pair: out when idx[k] >=
 *     n_tgt (the index array is data), when max_d2 >= 0 and not (d2[k] <= max_d2) (the pair AT the gate is in, a NaN d2 is out), when
 *     n is the zero vector, when r = n_0 (p_0 - q_0) + n_1 (p_1 - q_1) + n_2 (p_2 - q_2) or (p_0 + p_1) + p_2 is not finite.  It adds,
 *     with J = [p x n ; n]: [0] += 1; [1] += r r; [2 + a] += J_a r; [8..28] += the upper triangle of J_a J_b, row-major.
 *   Photometric term of an accepted geometric pair, with I_p = d_src_intensity[k], I_q, g = the target's intensity and gradient at q:
 *       p'_a = p_a - r n_a;  d_a = p'_a - q_a;  rI = ((double) I_q + ((g_0 d_0 + g_1 d_1) + g_2 d_2)) - (double) I_p
 *       gn = (g_0 n_0 + g_1 n_1) + g_2 n_2;  a_c = g_c - gn n_c
 *     the pair enters iff rI, a_0, a_1, a_2 are all finite and |rI| <= i_max (the pair AT i_max is in); then with w = w_photo and
 *     J = [p x a ; a]: [2 + k] += (w J_k) rI; [8..28] += the upper triangle of (w J_k) J_l; [29] += 1; [30] += rI rI.
 *   Sums [0] and [1] stay purely geometric, so the state's pairs, rms and rms history and the n >= 6 test of the solve mean what they
 *     mean for r3d_icp_iterate_plane; r3d_plane_step_from_sums solves the step from the first 29.  Grid and reduction are
 *     r3d_icp_plane_accumulate's: min(ceil(n_src / 256), C) workgroups (C = the device's compute units), one row of 31 partials per
 *     workgroup, one finishing workgroup, no float atomics: bitwise repeatable, and with w_photo == 0 the first 29 sums are the bits
 *     of r3d_icp_plane_accumulate(..., trim_q 0, gate_scale 1).  d_photo_out [n_src] f32 (may be NULL) = (float) rI where a
 *     photometric pair entered, NaN elsewhere.  n_src == 0: 31 zeros, no launch.
 *   R3D_ERR_INVALID, nothing written: a NULL ctx or h_sums; negative sizes; with n_src > 0 a NULL d_src, d_src_intensity, d_tgt,
 *     d_tgt_normals, d_tgt_intensity, d_tgt_grad or d_idx; max_d2 >= 0 with a NULL d_d2; max_d2 NaN; w_photo negative or not finite;
 *     i_max not > 0 and finite; d_photo_out overlapping an input.
 *
 * r3d_icp_iterate_color: n_iters whole passes with NO host round trip on the R3D_ICP_STATE_DOUBLES state -- r3d_icp_iterate_plane
 *   without the direction classes and the rank trimming.  Each pass: culled exact NN (d_src in the index's order,
 *   r3d_nn_index_sort_cloud; warm-started exactly as the plane loop is) -> the pass above against the index's cloud -> finish, solve
 *   from the first 29 sums and state update on the device -> d_src = T_total . d_src_orig (d_src_orig NULL: d_src moved in place by
 *   the step).  d_src_intensity [n_src] f32 is constant and in the order of d_src.  d_tgt_normals, d_tgt_intensity, d_tgt_grad: of
 *   the index's cloud in its ORIGINAL order.  A singular solve sets the sticky status 1 and moves nothing.  d_sums_out (may be NULL):
 *   the 31 sums of the last pass, in HBM.  Asynchronous.
 *   R3D_ERR_INVALID, nothing written: a NULL ctx, index or required device pointer; an index of another context; n_iters < 0;
 *     n_src < 6; d_src_orig == d_src; max_d2 NaN; w_photo / i_max as above; d_src, d_idx, d_d2, d_state or d_sums_out overlapping one
 *     another or an input.
 * Deliberately not done here: colour in register_multiway and register_global; robust (Huber) weights; rank trimming in the coloured
 *   loop; exposure compensation; a bench.py workload; the multi-GPU path. */
#define R3D_COLOR_ICP_SUMS 31
#define R3D_COLOR_GRADIENT_FLOOR 1e-14
int r3d_color_gradient_knn(r3d_nn_index* index, int k, double radius, const float* d_normals, const uint32_t* d_rgba,
                           float* d_intensity_out, float* d_grad_out, uint32_t* d_count_out);
int r3d_icp_color_accumulate(r3d_ctx* ctx, const float* d_src, const float* d_src_intensity, int64_t n_src, const float* d_tgt,
                             const float* d_tgt_normals, const float* d_tgt_intensity, const float* d_tgt_grad, int64_t n_tgt,
                             const uint32_t* d_idx, const float* d_d2, float max_d2, double w_photo, double i_max, double* h_sums,
                             float* d_photo_out);
int r3d_icp_iterate_color(r3d_ctx* ctx, r3d_nn_index* index, const float* d_src_orig, float* d_src, const float* d_src_intensity,
                          int64_t n_src, const float* d_tgt_normals, const float* d_tgt_intensity, const float* d_tgt_grad,
                          uint32_t* d_idx, float* d_d2, int n_iters, float max_d2, double w_photo, double i_max, double* d_state,
                          double* d_sums_out);

/* ---- Reconstruction evaluation (csrc/r3d_meshdist.hip; NOT IN THE REFERENCE, whose readme leaves "the accuracy comparison of the
 * clouds" to CloudCompare; this text is the specification, tests/compare_ref.py restates it in NumPy).  Distance from every point
 * to a triangle mesh (CloudCompare's C2M, Open3D's RaycastingScene.compute_distance; NO parity with either is claimed), fixed-order
 * statistics of a distance field, the f32 root that turns r3d_nn_index_query's d2 into distances (cloud to cloud), and a colour
 * ramp.  None of these kernels has been timed on a card.
 *
 * r3d_mesh_index_create: d_xyz [n_vertices][3] f32, d_tri [n_triangles][3] int32.  The index keeps its own copy of what it needs:
 *   the mesh may be freed or rewritten when the call returns (it synchronises).  n_triangles == 0 and n_vertices == 0 are fine.
 *   Validity: a triangle is valid iff its three indices lie in [0, n_vertices) -- checked before any of them is used as an address --
 *     and its nine coordinates are finite.  An invalid triangle is never a winner.  A zero-area triangle (a repeated index,
 *     coincident or collinear vertices) is valid and is measured as the segment or point it is; a triangle listed twice is two
 *     triangles.
 *   R3D_ERR_INVALID, nothing written: a NULL ctx or index_out; a negative size; a NULL d_tri with n_triangles > 0 or d_xyz with
 *     n_vertices > 0.  n_vertices or n_triangles > 2^31 - 1: R3D_ERR_UNSUPPORTED.
 *
 * r3d_mesh_index_query: for every point p of d_points [n_points][3] f32 the nearest valid triangle, by this DEFINITION (brute
 *   force over all valid triangles; culling is an implementation matter and never changes a bit).  All arithmetic is IEEE fp64 on
 *   the f32 inputs converted exactly, products and sums in the order written, left to right, no fused multiply-add; x . y means
 *   (x0*y0 + x1*y1) + x2*y2.  For the triangle (a, b, c):
 *     ab = b - a, ac = c - a, bc = c - b, ap = p - a, bp = p - b, cp = p - c
 *     d1 = ab.ap, d2 = ac.ap, d3 = ab.bp, d4 = ac.bp, d5 = ab.cp, d6 = ac.cp
 *     vc = d1*d4 - d3*d2, vb = d5*d2 - d1*d6, va = d3*d6 - d5*d4, e43 = d4 - d3, e56 = d5 - d6
 *     den_ab = d1 - d3, den_ac = d2 - d6, den_bc = e43 + e56   (|ab|^2, |ac|^2, |bc|^2 but for rounding)
 *   The region is the FIRST of these that holds:
 *     A:  d1 <= 0 and d2 <= 0                      q = a
 *     B:  d3 >= 0 and d4 <= d3                     q = b
 *     AB: vc <= 0, d1 >= 0, d3 <= 0, den_ab > 0    r = d1 / den_ab,              q = (a + ab*r) + ac*0
 *     C:  d6 >= 0 and d5 <= d6                     q = c
 *     AC: vb <= 0, d2 >= 0, d6 <= 0, den_ac > 0    r = d2 / den_ac,              q = (a + ab*0) + ac*r
 *     BC: va <= 0, e43 >= 0, e56 >= 0, den_bc > 0  r = e43 / den_bc,             q = (b + bc*r) + ac*0
 *     face (otherwise)                             r = 1 / ((va + vb) + vc), or 0 where that sum is not > 0,
 *                                                  q = (a + ab*v) + ac*w  with
 *         v = vb*r, v = v > 0 ? v : 0, v = v < 1 ? v : 1;  w = vc*r, w = w > 0 ? w : 0, w = w < 1 - v ? w : 1 - v
 *   (q per coordinate; a vertex region returns the vertex itself).  Zero-area rule: an edge region is taken only where its
 *   denominator is > 0 -- an edge of no length is left to the regions of its end points and of the other edges --, the face's
 *   quotient is 0 where its denominator is not > 0, and the selects above turn a NaN into 0: no division by zero and no NaN arises
 *   for finite input.  A triangle with a repeated index or coincident vertices has an edge vector of exact zeros, its products
 *   are exact zeros, and it is measured exactly as its segment or point; so is a collinear triangle whose products are exact.
 *   For other collinear triangles rounding decides the region as it does for any sliver, and q is a point of the segment.
 *     dq = p - q,  d2(p, triangle) = (dq0*dq0 + dq1*dq1) + dq2*dq2
 *   The triangle with the smallest d2 wins; the LOWEST triangle index wins exact ties.
 *   d_dist_out [n_points] f32 = (float) sqrt(d2), rounded once from the correctly rounded fp64 root (+inf where d2 exceeds the f32
 *     range).  With R3D_MESHDIST_SIGNED in flags it is negated where n . dq < 0 for n = ab x ac = (ab1*ac2 - ab2*ac1,
 *     ab2*ac0 - ab0*ac2, ab0*ac1 - ab1*ac0) of the winning triangle; the sign is + where the product is 0.  This is the FACE-NORMAL
 *     sign of the tie-winning triangle, not an angle-weighted pseudonormal: next to an edge or a vertex of a closed surface, where
 *     the nearest point is shared by triangles facing differently, it may disagree with inside / outside.
 *   d_tri_out [n_points] u32 (may be NULL): the winner.  d_closest_out [n_points][3] f32 (may be NULL): (float) q, rounded once.
 *   A point with a non-finite coordinate, or an index without a valid triangle: distance +inf, triangle 0xFFFFFFFF, closest NaN.
 *   h_groups_evaluated (may be NULL; the call synchronises when it is given, and is asynchronous otherwise): the number of
 *     32-triangle groups whose triangles were measured, summed over the waves of 64 points -- waves * ceil(valid triangles / 32)
 *     without culling.  It depends on the order the points are met in, the results do not.
 *   n_points == 0 is fine.  R3D_ERR_INVALID, nothing written: a NULL index; a negative n_points; unknown flag bits; a NULL d_points
 *     or d_dist_out with n_points > 0; an output overlapping the points or another output.  n_points > 2^31 - 1:
 *     R3D_ERR_UNSUPPORTED.  Inputs are never modified.  Results do not depend on the launch geometry, on the order of the points
 *     or on what ran before on the context (the call sorts its keys in a workspace of the context that only the evaluation calls touch, in stream order).
 *   How: the valid triangles are sorted by the Morton code of their centroid and grouped by 32 with an f32 box per group; the
 *     points are sorted by the same code and a wave takes 64 of them, starts at the group of its own neighbourhood, walks outwards
 *     and skips a group only when a conservative lower bound of its box is STRICTLY above every lane's best.  No float atomics.
 *     There is no coarser level than the group yet: every wave tests every group's box.
 *
 * r3d_distance_stats: d_values [n] f32 -> x = (double) v, then x = sqrt(x) (correctly rounded) when squared_input != 0.  An x that
 *   is not finite is counted apart and takes no part in anything else.
 *   h_stats_out [6] f64 = {n_finite, n_nonfinite, sum x, sum x*x, min, max}.  Fixed order, the same bits run to run: row r holds
 *     elements [256 r, 256 r + 256), one per lane, a missing lane adding 0.0; a row is reduced per 64 lanes by the tree
 *     s[i] += s[i + 32], s[i + 16], ... s[i + 1], then the four waves are added in order to 0.0; the finish gives thread t of 256 the
 *     rows t, t + 256, ... added in order to 0.0, and reduces the 256 values the same way.  min and max have 0.0 added (a zero
 *     is reported as +0); with no finite element they are +inf and -inf and the sums are 0.
 *   h_count_le_out [n_thresholds] int64: the finite x with x <= h_thresholds[t]; n_thresholds <= 8.
 *   h_hist_out [n_bins] u64: finite x counts in bin min((int64) floor(x / bin_width), n_bins - 1), a negative x in bin 0;
 *     n_bins <= 4096 (0: no histogram, bin_width is ignored).  Integer atomics.
 *   Synchronises.  R3D_ERR_INVALID, nothing written: a NULL ctx or h_stats_out; a negative n; a NULL d_values with n > 0;
 *     n_thresholds outside [0, 8] or n_bins outside [0, 4096]; NULL h_thresholds or h_count_le_out with n_thresholds > 0; a NaN
 *     threshold; NULL h_hist_out, or a bin_width that is not finite and > 0, with n_bins > 0.  n > 2^31 - 1: R3D_ERR_UNSUPPORTED.
 * r3d_sqrt_f32_inplace: v = (float) sqrt((double) v), which is the correctly rounded f32 root (fp64 carries more than twice the
 *   bits): r3d_nn_index_query's d2 become distances.  A negative value becomes NaN, -0 stays -0.  Asynchronous.
 * r3d_distance_colors: CloudCompare's scalar-field view.  d_rgba_out [n] u32 = r | g << 8 | b << 16, the words r3d_write_ply_rgba
 *   takes.  A distance that is not finite: r = g = b = 128.  Otherwise, in fp64, t = |d| / d_max, t = t < 1 ? t : 1,
 *   q = (integer) floor(t * 765): q <= 255: (r, g, b) = (0, q, 255 - q), blue to green; q <= 510: (q - 255, 255, 0), green to
 *   yellow; else (255, 255 - (q - 510), 0), yellow to red.  d_max must be finite and > 0.  Asynchronous.
 *   R3D_ERR_INVALID for both, nothing written: a NULL ctx; a negative n; a NULL device pointer with n > 0; d_max as above; the
 *     output overlapping the distances.  n > 2^31 - 1: R3D_ERR_UNSUPPORTED. */
typedef struct r3d_mesh_index r3d_mesh_index;
#define R3D_MESHDIST_SIGNED 1
int r3d_mesh_index_create(r3d_ctx* ctx, const float* d_xyz, int64_t n_vertices, const int32_t* d_tri, int64_t n_triangles,
                          r3d_mesh_index** index_out);
int r3d_mesh_index_destroy(r3d_mesh_index* index);
int r3d_mesh_index_query(r3d_mesh_index* index, const float* d_points, int64_t n_points, int flags, float* d_dist_out,
                         uint32_t* d_tri_out, float* d_closest_out, int64_t* h_groups_evaluated);
int r3d_distance_stats(r3d_ctx* ctx, const float* d_values, int64_t n, int squared_input, const double* h_thresholds, int n_thresholds,
                       double bin_width, int n_bins, double* h_stats_out, int64_t* h_count_le_out, uint64_t* h_hist_out);
int r3d_sqrt_f32_inplace(r3d_ctx* ctx, float* d_values, int64_t n);
int r3d_distance_colors(r3d_ctx* ctx, const float* d_dist, int64_t n, double d_max, uint32_t* d_rgba_out);

/* ---- Depth consistency (csrc/r3d_consistency.hip; NOT IN THE REFERENCE -- the geometric consistency check that COLMAP's fusion and
 * MVSNet-style pipelines put between depth maps and fusion; no parity with either is claimed, this text is the specification).
 * r3d_fuse_frames concatenates every pixel of every frame and the TSDF volume carves with every depth; the cleaning tools work on
 * the cloud afterwards.  This filter asks the OTHER frames' depth maps: a pixel is kept when enough of them see a surface where it
 * says one is and none (few) sees through it.  All F frames of a batch are references; frame r asks up to S sources.
 * All device arithmetic is f32 in the order written: no fused multiply-add, correctly rounded division, f32 denormals kept.  The
 * result of a pixel is a function of that pixel, the rasters and the poses alone -- no LDS, no atomics, independent of launch
 * geometry.
 * Inputs.  The rasters [F][H][W] of depth_dtype and the camera, as r3d_tsdf_integrate takes them: scale = (float) depth_scale
 *   (finite), fx, fy, cx, cy rounded once to f32.  h_pose_w2c: F x 12 host doubles [R row-major (9), t (3)], WORLD -> CAMERA, the
 *   layout r3d_tsdf_integrate reads.  h_sources: [F][S] host int32, S = n_sources in [1, R3D_CONSISTENCY_MAX_SOURCES]; row r lists
 *   the sources of frame r: -1 is an empty slot, any other entry must be in [0, F), an entry equal to r is an argument error.
 *   Repeated entries are allowed and simply vote twice.  F H W < 2^31; H, W <= 2^24.
 * Relative pose (host, fp64, no fused multiply-add): for every filled slot (r, s = h_sources[r][k])
 *     Rsr[i][j] = (Rs[i][0] Rr[j][0] + Rs[i][1] Rr[j][1]) + Rs[i][2] Rr[j][2]                 (R_s R_r^T)
 *     tsr[i]    = ts[i] - ((Rsr[i][0] tr[0] + Rsr[i][1] tr[1]) + Rsr[i][2] tr[2])             (from the fp64 Rsr)
 *   each of the twelve numbers rounded once to f32: a camera-r point p maps to camera s as Rsr p + tsr.
 * Reference pixel (u, v) of frame r:  Z = (float) depth[r][v][u] * scale.  The pixel is valid iff Z > 0 and Z < inf.  An invalid
 *   pixel gets votes (0, 0), keep 0 and filtered 0.0f.  For a valid pixel
 *     x = (((float) u - cx) / fx) * Z;   y = (((float) v - cy) / fy) * Z;   z = Z
 *   and then, for every filled slot in slot order:
 *     1. p = ((R0 x + R1 y) + R2 z) + t  per row of the relative pose            (the parenthesisation of "TSDF volume")
 *     2. unseen unless p.z > 0
 *     3. u' = fx (p.x / p.z) + cx;  v' = fy (p.y / p.z) + cy;  ui = floorf(u' + 0.5f);  vi = floorf(v' + 0.5f);
 *        unseen unless 0 <= ui < W and 0 <= vi < H (as floats; NaN fails)       (the nearest-pixel rule of "TSDF volume")
 *     4. d = (float) depth[s][vi][ui] * scale;  unseen unless d > 0 and d < inf
 *     5. diff = d - p.z;  tol = (float) rel_tol * p.z
 *     6. fabsf(diff) <= tol: a CONSISTENT vote.  Otherwise diff > 0: a VIOLATION -- the source sees past the point, so the point
 *        floats in space that camera saw as free.  Anything else: the point is occluded in s and casts no vote.
 *   Decision: keep = consistent >= min_consistent && violations <= max_violations.
 * Outputs (each may be NULL, at least one must be given; none may overlap the rasters or another output):
 *     d_votes_out     [F][H][W][2] u8   {consistent, violations}; 2-byte aligned
 *     d_keep_out      [F][H][W]    u8   0 or 1
 *     d_filtered_out  [F][H][W]    f32  Z where kept, otherwise 0.0f: a raster r3d_tsdf_integrate takes as it stands (R3D_DEPTH_F32,
 *                                       depth_scale 1, 0 = no measurement)
 *   No byte outside the given outputs' extents is written.
 * What the nearest-pixel rule costs: the source depth is read at the centre of the pixel the point falls into, up to half a pixel
 *   away from where it falls.  On a surface slanted by an angle a to the source's image plane that is a depth difference of up to
 *   about Z tan(a) / (2 f) (f = the focal length in pixels): 0.3 % of Z at 60 degrees and f = 300.  rel_tol has to cover it next to
 *   the depth noise.  Bilinear sampling would not have this error on a plane, but it mixes the depths on both sides of an edge and
 *   invents surfaces between them -- exactly where floaters sit.
 * r3d_depth_consistency takes device rasters and is asynchronous on the ctx stream (poses and table are copied before it returns);
 *   r3d_depth_consistency_host takes host rasters and host outputs, uploads and downloads itself and is synchronous.  One lane per
 *   reference pixel with the source loop inside, one frame per blockIdx.y, a 32 x 2 pixel tile per wave.
 * R3D_ERR_INVALID, nothing written, checked in this order: an unknown depth dtype; n_frames < 0; n_sources outside
 *   [1, R3D_CONSISTENCY_MAX_SOURCES]; rel_tol not finite or not > 0 in f32; min_consistent or max_violations outside [0, 255];
 *   depth_scale not finite in f32; with n_frames > 0 a NULL h_pose_w2c or h_sources, then a table entry outside [-1, F), then a
 *   frame listing itself; a NULL ctx; a NULL camera; a camera of another ctx.  n_frames == 0: R3D_OK here.  Then: a raster too
 *   large (above); a NULL raster pointer; no output given; d_votes_out at an odd address (device call); an output overlapping the
 *   rasters or another output.
 * r3d_compact_rows_by_mask: the filtered cloud.  d_xyz [n][3] f32, d_rgba [n] u32 colour words or NULL, d_keep [n] u8: the rows i
 *   with d_keep[i] != 0 go, in input order and bit for bit, to d_xyz_out (and their words to d_rgba_out; given iff d_rgba is).  Fed
 *   with r3d_fuse_frames' cloud and d_keep_out above it yields the fused cloud without the rejected pixels.  *n_out = the TRUE number
 *   of kept rows, always; at most cap rows are written and nothing beyond them; cap < *n_out is not an error and cap == 0 with NULL
 *   outputs asks for the count alone (the two-phase manner of r3d_tsdf_extract_points).  r3d_select_rows is its sibling for the
 *   outlier masks: row numbers instead of colours, no cap.  Synchronises (the count is read back).
 *   R3D_ERR_INVALID, nothing written, in this order: NULL n_out; n outside [0, 2^32); cap < 0; a NULL ctx; with n > 0 a NULL d_xyz
 *   or d_keep; d_xyz_out NULL with cap > 0; d_rgba without d_rgba_out (cap > 0) or d_rgba_out without d_rgba; an output's written
 *   rows overlapping an input or the other output. */
#define R3D_CONSISTENCY_MAX_SOURCES 16
int r3d_depth_consistency(r3d_ctx* ctx, const r3d_camera* cam, const void* d_depth, int depth_dtype, int n_frames, double depth_scale,
                          const double* h_pose_w2c, const int32_t* h_sources, int n_sources, double rel_tol, int min_consistent,
                          int max_violations, uint8_t* d_votes_out, uint8_t* d_keep_out, float* d_filtered_out);
int r3d_depth_consistency_host(r3d_ctx* ctx, const r3d_camera* cam, const void* h_depth, int depth_dtype, int n_frames,
                               double depth_scale, const double* h_pose_w2c, const int32_t* h_sources, int n_sources, double rel_tol,
                               int min_consistent, int max_violations, uint8_t* h_votes_out, uint8_t* h_keep_out,
                               float* h_filtered_out);
int r3d_compact_rows_by_mask(r3d_ctx* ctx, const float* d_xyz, const uint32_t* d_rgba, int64_t n, const uint8_t* d_keep,
                             float* d_xyz_out, uint32_t* d_rgba_out, int64_t cap, int64_t* n_out);

#ifdef __cplusplus
}
#endif
#endif /* R3D_H */
