"""Multi-view depth consistency on the MI355X: before frames are fused into a cloud or integrated into a volume, every pixel is
checked against the depth maps of neighbouring frames -- kept when enough of them see a surface where the pixel says one is and
none (few) sees through it.  What COLMAP's fusion and MVSNet-style pipelines do between depth maps and fusion; no parity with
either is claimed.  Semantics: include/r3d.h ("Depth consistency") and DESIGN.md section 4.5z.

Inputs are what fuse_frames and TSDFVolume.integrate take: [F,H,W] depth, one pose-file row per frame (quats_xyzw, ts), a pinhole
camera.  The poses are used as they stand (world -> camera, poses_w2c); fuse_frames' pose_table is the inverse of the same pose,
so one (quats, ts) pair serves the filter and the fusion.
"""
import ctypes as C
import math

import numpy as np

from . import _lib as L
from .device import default_context, depth_code
from .fusion import REF_INTRINSICS, _as_batch, fuse_frames_device, fuse_frames_rgb_device
from .poses import pose_table
from .tsdf import _pose_rows, _rgb_batch, poses_w2c

MAX_SOURCES = 16   # R3D_CONSISTENCY_MAX_SOURCES


def window_sources(n_frames, radius):
    """[n_frames, 2*radius] int32: row r lists the frames r-radius .. r+radius without r, those outside the sequence dropped,
    in ascending order, the row padded with -1.  1 <= radius <= 8 (2*radius slots)."""
    n_frames, radius = int(n_frames), int(radius)
    if n_frames < 0:
        raise ValueError("n_frames must be >= 0, got %d" % n_frames)
    if not 1 <= 2 * radius <= MAX_SOURCES:
        raise ValueError("radius must be in [1, %d], got %d" % (MAX_SOURCES // 2, radius))
    table = np.full((n_frames, 2 * radius), -1, dtype=np.int32)
    for r in range(n_frames):
        near = [s for s in range(r - radius, r + radius + 1) if s != r and 0 <= s < n_frames]
        table[r, :len(near)] = near
    return table


def _source_table(sources, n_frames, radius):
    """the [F,S] int32 table of a call: `sources` as given, or the window of `radius`"""
    if sources is None:
        return window_sources(n_frames, radius)
    t = np.asarray(sources)
    if t.ndim != 2 or t.shape[0] != n_frames or not 1 <= t.shape[1] <= MAX_SOURCES or not np.issubdtype(t.dtype, np.integer):
        raise ValueError("sources must be an integer [%d, S] table with 1 <= S <= %d, got %s of shape %s"
                         % (n_frames, MAX_SOURCES, t.dtype, list(t.shape)))
    if ((t < -1) | (t >= n_frames)).any():
        raise ValueError("sources holds an entry that is not -1 and not in [0, %d)" % n_frames)
    if (t == np.arange(n_frames)[:, None]).any():
        raise ValueError("sources lists a frame as its own source")
    return np.ascontiguousarray(t, dtype=np.int32)


def _rule(rel_tol, min_consistent, max_violations):
    try:
        tol = float(rel_tol)
    except (TypeError, ValueError):
        raise ValueError("rel_tol must be a finite number > 0, got %r" % (rel_tol,))
    with np.errstate(over="ignore"):
        t32 = np.float32(tol)
    if isinstance(rel_tol, bool) or not (math.isfinite(tol) and t32 > 0 and np.isfinite(t32)):
        raise ValueError("rel_tol must be a finite number > 0 (in float32), got %r" % (rel_tol,))
    for name, v in (("min_consistent", min_consistent), ("max_violations", max_violations)):
        if isinstance(v, bool) or int(v) != v or not 0 <= int(v) <= 255:
            raise ValueError("%s must be an integer in [0, 255], got %r" % (name, v))
    return tol, int(min_consistent), int(max_violations)


def depth_consistency_device(ctx, cam, d_depth, depth_dtype, n_frames, poses_w2c, sources, d_votes=None, d_keep=None,
                             d_filtered=None, rel_tol=0.01, min_consistent=2, max_violations=0, depth_scale=1.0):
    """The filter from rasters in HBM (d_depth: [n_frames][H][W] of depth_dtype at a raw device address; cam: ctx.camera(...));
    poses_w2c: [n_frames,12] host rows; sources: the [n_frames,S] table (window_sources makes one).  Outputs at raw device
    addresses, any of them None but not all: d_votes [n_frames][H][W][2] uint8 {consistent, violations}, d_keep [n_frames][H][W]
    uint8, d_filtered [n_frames][H][W] float32 (the depth where kept, else 0: what integrate_device takes with float32 and
    depth_scale 1).  Asynchronous on the context's stream."""
    n_frames = int(n_frames)
    if n_frames < 0:
        raise ValueError("n_frames must be >= 0, got %d" % n_frames)
    table = _pose_rows(poses_w2c, n_frames)
    if sources is None:
        raise ValueError("sources must be given: the [n_frames, S] table (window_sources makes one)")
    src = _source_table(sources, n_frames, 1)
    tol, mc, mv = _rule(rel_tol, min_consistent, max_violations)
    L.check(ctx.lib.r3d_depth_consistency(ctx.handle, cam.handle, d_depth, depth_code(depth_dtype), n_frames, float(depth_scale),
                                          table.ctypes.data, src.ctypes.data, src.shape[1], tol, mc, mv, d_votes, d_keep, d_filtered))


def depth_consistency(depths, quats_xyzw, ts, intrinsics=REF_INTRINSICS, radius=2, sources=None, rel_tol=0.01, min_consistent=2,
                      max_violations=0, depth_scale=1.0, ctx=None):
    """(consistent [F,H,W] uint8, violations [F,H,W] uint8, keep [F,H,W] bool, filtered [F,H,W] float32) of host rasters [H,W] or
    [F,H,W] (uint8, uint16 or float32) seen from the pose-file rows (quats_xyzw, ts).  Every frame asks its sources -- the frames
    within `radius` of it in the sequence, or row r of `sources` ([F,S] integers, -1 = empty slot) -- where each of its pixels
    lies in them: a source whose depth there agrees within rel_tol (relative to the depth in the source) casts a consistent vote, one
    that sees farther a violation (the pixel floats in space that camera saw as free), one that sees something nearer none.
    keep = consistent >= min_consistent and violations <= max_violations; filtered = the depth (times depth_scale) where kept, else
    0 -- rasters TSDFVolume.integrate takes with depth_scale 1.  A pixel without a depth (0, negative, not finite) is never kept.
    rel_tol has to cover the half pixel of the nearest-pixel lookup on slanted surfaces next to the depth noise.  Synchronous."""
    d = _as_batch(depths)
    f, h, w = d.shape
    table = poses_w2c(quats_xyzw, ts)
    if table.shape[0] != f:
        raise ValueError("%d frames but %d poses" % (f, table.shape[0]))
    src = _source_table(sources, f, radius)
    tol, mc, mv = _rule(rel_tol, min_consistent, max_violations)
    votes = np.zeros((f, h, w, 2), dtype=np.uint8)
    keep = np.zeros((f, h, w), dtype=np.uint8)
    filtered = np.zeros((f, h, w), dtype=np.float32)
    if f * h * w:
        ctx = ctx or default_context()
        cam = ctx.camera(h, w, *intrinsics)
        L.check(ctx.lib.r3d_depth_consistency_host(ctx.handle, cam.handle, d.ctypes.data, depth_code(d.dtype), f, float(depth_scale),
                                                   table.ctypes.data, src.ctypes.data, src.shape[1], tol, mc, mv, votes.ctypes.data,
                                                   keep.ctypes.data, filtered.ctypes.data))
    return np.ascontiguousarray(votes[..., 0]), np.ascontiguousarray(votes[..., 1]), keep.astype(bool), filtered


def compact_rows_device(ctx, d_xyz, d_rgba, n, d_keep, d_xyz_out, d_rgba_out, cap):
    """The rows of the [n][3] float32 cloud d_xyz (and the words of d_rgba, [n] uint32 or None) whose d_keep byte is not 0, in
    input order, into d_xyz_out / d_rgba_out (raw device addresses with room for cap rows; None with cap == 0).  Returns the TRUE
    number of kept rows, of which at most cap were written (r3d_compact_rows_by_mask).  Synchronises."""
    m = C.c_int64()
    L.check(ctx.lib.r3d_compact_rows_by_mask(ctx.handle, d_xyz, d_rgba, int(n), d_keep, d_xyz_out, d_rgba_out, int(cap), C.byref(m)))
    return m.value


def fuse_frames_consistent(depths, quats_xyzw, ts, intrinsics=REF_INTRINSICS, radius=2, sources=None, rel_tol=0.01,
                           min_consistent=2, max_violations=0, depth_scale=1.0, rgb=None, ctx=None):
    """fuse_frames without the pixels the consistency filter rejects: (xyz [N,3] float32, keep [F,H,W] bool), or with rgb
    ([F,H,W,3] uint8) (xyz, rgba [N] uint32, keep) as fuse_frames_rgb returns them.  The rasters go up once; the filter, the fusion and
    an order-preserving compaction run on the device: xyz is fuse_frames(...)[keep.ravel()] bit for bit.  The other arguments: depth_consistency."""
    d = _as_batch(depths)
    f, h, w = d.shape
    w2c = poses_w2c(quats_xyzw, ts)
    if w2c.shape[0] != f:
        raise ValueError("%d frames but %d poses" % (f, w2c.shape[0]))
    src = _source_table(sources, f, radius)
    _rule(rel_tol, min_consistent, max_violations)
    n = f * h * w
    if rgb is not None:
        rgb = _rgb_batch(rgb, d.shape)
    if n == 0:
        empty = (np.zeros((0, 3), np.float32), np.zeros((f, h, w), bool))
        return empty if rgb is None else (empty[0], np.zeros(0, np.uint32), empty[1])
    ctx = ctx or default_context()
    cam = ctx.camera(h, w, *intrinsics)
    tab = pose_table(quats_xyzw, ts)
    with ctx.buffers() as B:
        d_depth, d_pose, d_keep, d_xyz = B.upload(d), B.upload(tab), B.alloc(n), B.alloc(n * 12)
        d_rgb = d_rgba = None
        if rgb is not None:
            d_rgb, d_rgba = B.upload(rgb), B.alloc(n * 4)
        depth_consistency_device(ctx, cam, d_depth.ptr, d.dtype, f, w2c, src, d_keep=d_keep.ptr, rel_tol=rel_tol,
                                 min_consistent=min_consistent, max_violations=max_violations, depth_scale=depth_scale)
        if rgb is None:
            fuse_frames_device(ctx, cam, d_depth.ptr, d.dtype, f, d_pose.ptr, d_xyz.ptr, np.float32, depth_scale)
        else:
            fuse_frames_rgb_device(ctx, cam, d_depth.ptr, d.dtype, f, d_pose.ptr, d_rgb.ptr, d_xyz.ptr, np.float32, d_rgba.ptr, depth_scale)
        keep = d_keep.download(np.uint8, n).reshape(f, h, w).astype(bool)
        m = int(keep.sum())
        out_xyz, out_rgba = np.zeros((m, 3), np.float32), np.zeros(m, np.uint32)
        if m:
            d_out = B.alloc(m * 12)
            d_out_rgba = None if rgb is None else B.alloc(m * 4)
            got = compact_rows_device(ctx, d_xyz.ptr, None if rgb is None else d_rgba.ptr, n, d_keep.ptr, d_out.ptr,
                                      None if rgb is None else d_out_rgba.ptr, m)
            assert got == m, (got, m)
            out_xyz = d_out.download_array(np.float32, (m, 3))
            if rgb is not None:
                out_rgba = d_out_rgba.download(np.uint32, m)
    return (out_xyz, keep) if rgb is None else (out_xyz, out_rgba, keep)
