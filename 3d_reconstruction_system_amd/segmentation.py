"""RANSAC plane segmentation on the MI355X: what users of Open3D call segment_plane for after outlier removal and normal
estimation -- strip the floor, find the walls, cut an indoor scene into structure and clutter (no parity with Open3D is
claimed).  Semantics: include/r3d.h (r3d_segment_plane, r3d_ransac_rows) and DESIGN.md section 4.5h.

segment_plane finds the one plane most points lie on; segment_planes peels plane after plane off the remaining points.  The
*_device function takes device pointers.
"""
import collections
import ctypes as C

import numpy as np

from . import _lib as L
from ._args import positive as _check_positive, whole as _check_count
from .device import default_context
from .outliers import _cloud, select_rows_device

MAX_HYPOTHESES = 65536

PlaneSegment = collections.namedtuple("PlaneSegment", ["plane", "rows", "centroid", "eigenvalues", "best_hypothesis", "best_count",
                                                       "n_valid"])
PlaneSegment.__doc__ = ("plane [4] float64 (a b c d, unit normal; NaN when there is no plane), rows [M] uint32 (the inliers of the "
                        "refined plane, ascending), centroid [3] and eigenvalues [3] (ascending) of the refit, the best hypothesis, "
                        "its inlier count and the number of valid hypotheses.")
DevicePlane = collections.namedtuple("DevicePlane", ["plane", "centroid", "eigenvalues", "best_hypothesis", "best_count", "best_rows",
                                                     "n_valid", "n_inliers"])
DevicePlane.__doc__ = "What r3d_segment_plane reports on the host; the mask (and the counts) stay in HBM."


def _check_hypotheses(h):
    if isinstance(h, bool) or not isinstance(h, (int, np.integer)) or not 1 <= int(h) <= MAX_HYPOTHESES:
        raise ValueError("num_hypotheses must be an integer in [1, %d], got %r" % (MAX_HYPOTHESES, h))
    return int(h)


def _check_seed(seed):
    if isinstance(seed, bool) or not isinstance(seed, (int, np.integer)) or not 0 <= int(seed) < 1 << 64:
        raise ValueError("seed must be an integer in [0, 2^64), got %r" % (seed,))
    return int(seed)


def ransac_rows(seed, h, n):
    """The three rows hypothesis h samples from a cloud of n rows (host only, no GPU)."""
    seed = _check_seed(seed)
    if not 0 <= int(h) < 1 << 64 or not 1 <= int(n) < 1 << 32:
        raise ValueError("h must be in [0, 2^64) and n in [1, 2^32), got %r, %r" % (h, n))
    rows = (C.c_uint32 * 3)()
    L.check(L.load().r3d_ransac_rows(seed, int(h), int(n), rows))
    return tuple(rows)


def segment_plane_device(ctx, d_xyz, n, distance_threshold, num_hypotheses, seed, d_inlier, d_counts=None):
    """d_inlier [n] uint8 (1 = within the threshold of the refined plane), d_counts [num_hypotheses] uint32 (optional);
    returns a DevicePlane.  Synchronous."""
    thr, hyp, seed = _check_positive(distance_threshold, "distance_threshold"), _check_hypotheses(num_hypotheses), _check_seed(seed)
    if int(n) < 3:
        raise ValueError("a plane needs at least 3 points, got %d" % n)
    res, m = (C.c_double * 16)(), C.c_int64()
    L.check(ctx.lib.r3d_segment_plane(ctx.handle, d_xyz, int(n), thr, hyp, seed, d_inlier, d_counts, res, C.byref(m)))
    r = np.array(res[:], np.float64)
    return DevicePlane(r[0:4].copy(), r[4:7].copy(), r[7:10].copy(), int(r[10]), int(r[11]), r[12:15].astype(np.uint32), int(r[15]),
                       m.value)


def _rows_of(ctx, d_xyz, n, d_keep, m, B):
    """Row numbers (uint32 [m]) and the device copy (in the buffer scope B) of the rows with d_keep != 0."""
    d_out, d_rows = B.alloc(m * 12), B.alloc(m * 4)
    if m == 0:
        return np.zeros(0, np.uint32), d_out
    got = select_rows_device(ctx, d_xyz.ptr, n, d_keep.ptr, d_out.ptr, d_rows.ptr)
    assert got == m, (got, m)
    return d_rows.download(np.uint32, m), d_out


def segment_plane(xyz, distance_threshold=0.01, num_hypotheses=1024, seed=0, ctx=None):
    """PlaneSegment: the plane with the most points within distance_threshold among num_hypotheses three-point samples, refitted
    to those points by least squares, and the rows within distance_threshold of the refitted plane."""
    xyz = _cloud(xyz)
    thr, hyp, seed = _check_positive(distance_threshold, "distance_threshold"), _check_hypotheses(num_hypotheses), _check_seed(seed)
    n = xyz.shape[0]
    if n < 3:
        raise ValueError("a plane needs at least 3 points, got %d" % n)
    ctx = ctx or default_context()
    with ctx.buffers() as B:
        d_xyz, d_keep = B.upload(xyz), B.alloc(n)
        p = segment_plane_device(ctx, d_xyz.ptr, n, thr, hyp, seed, d_keep.ptr)
        rows, _ = _rows_of(ctx, d_xyz, n, d_keep, p.n_inliers, B)
        return PlaneSegment(p.plane, rows, p.centroid, p.eigenvalues, p.best_hypothesis, p.best_count, p.n_valid)


def segment_planes(xyz, distance_threshold=0.01, num_hypotheses=1024, max_planes=6, min_inliers=100, seed=0, ctx=None):
    """(planes [P,4] float64, labels [N] int32 with -1 = no plane, counts [P] int64): round r segments the rows no earlier plane
    took with seed + r (mod 2^64); the peeling stops after max_planes planes, when a round finds fewer than min_inliers inliers
    or when fewer than 3 rows remain."""
    xyz = _cloud(xyz)
    thr, hyp, seed = _check_positive(distance_threshold, "distance_threshold"), _check_hypotheses(num_hypotheses), _check_seed(seed)
    max_planes, min_inliers = _check_count(max_planes, "max_planes", 0), _check_count(min_inliers, "min_inliers", 1)
    n = xyz.shape[0]
    labels = np.full(n, -1, np.int32)
    planes, counts = [], []
    if n < 3 or max_planes == 0:
        return np.zeros((0, 4)), labels, np.zeros(0, np.int64)
    ctx = ctx or default_context()
    with ctx.buffers() as B:
        d_cur, d_keep = B.upload(xyz), B.alloc(n)
        rows_cur, m = np.arange(n, dtype=np.int64), n       # original row of every remaining row
        for r in range(max_planes):
            if m < 3:
                break
            p = segment_plane_device(ctx, d_cur.ptr, m, thr, hyp, (seed + r) % (1 << 64), d_keep.ptr)
            if p.n_inliers < min_inliers or p.n_inliers == 0:
                break
            keep = d_keep.download(np.uint8, m) != 0
            labels[rows_cur[keep]] = len(planes)
            planes.append(p.plane)
            counts.append(p.n_inliers)
            # the rest, compacted on the device: flip the mask and select
            d_keep.upload((~keep).astype(np.uint8))
            rest = m - p.n_inliers
            _, d_next = _rows_of(ctx, d_cur, m, d_keep, rest, B)
            rows_cur, d_cur, m = rows_cur[~keep], d_next, rest
        return np.array(planes, np.float64).reshape(-1, 4), labels, np.array(counts, np.int64)
