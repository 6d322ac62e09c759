"""Reconstruction evaluation on the MI355X: how far a reconstructed cloud or mesh lies from the truth -- the comparison step the
reference's readme (section 4.1) leaves to CloudCompare.  Cloud to cloud is the exact nearest neighbour of the NN index, cloud to
mesh the exact nearest triangle (r3d_mesh_index_*), and every reported number comes from the device's fixed-order sums and integer
counts (r3d_distance_stats).  No parity with CloudCompare or Open3D is claimed.  Semantics: include/r3d.h ("Reconstruction
evaluation") and DESIGN.md section 4.5w.  There is no CPU path: without the library or a device every entry point raises.

The *_device functions take raw device addresses and leave their results in HBM.
"""
import ctypes as C
import math

import numpy as np

from . import _lib as L
from ._args import MAX_ITEMS, count as _count
from .device import default_context
from .icp import NNIndex

NO_TRIANGLE = 0xFFFFFFFF     # the winner of a point without a nearest triangle
SIGNED = 1                   # R3D_MESHDIST_SIGNED
MAX_THRESHOLDS, MAX_BINS = 8, 4096


def _points(xyz, what):
    p = np.asarray(xyz)
    if p.size == 0:
        p = np.zeros((0, 3), np.float32)
    if p.ndim != 2 or p.shape[1] != 3 or p.dtype.kind not in "fiu":
        raise ValueError("%s must be an [N,3] array of numbers, got %s of shape %s" % (what, p.dtype, list(p.shape)))
    _count(len(p), "the number of rows of %s" % what)
    return np.ascontiguousarray(p, dtype=np.float32)


def _triangles(triangles):
    t = np.asarray(triangles)
    if t.size == 0:
        t = np.zeros((0, 3), np.int32)
    if t.ndim != 2 or t.shape[1] != 3 or t.dtype.kind not in "iu":
        raise ValueError("triangles must be an [M,3] integer array, got %s of shape %s" % (t.dtype, list(t.shape)))
    if t.dtype != np.int32:
        if t.size and (t.min() < -2 ** 31 or t.max() > MAX_ITEMS):
            raise ValueError("triangle indices must fit int32")
        t = t.astype(np.int32)
    _count(len(t), "the number of triangles")
    return np.ascontiguousarray(t)


class MeshIndex:
    """r3d_mesh_index: the valid triangles of a device-resident mesh, sorted and boxed for exact nearest-triangle queries.  The
    index keeps its own copy: the mesh buffers may be freed once the constructor returns.  A context manager."""

    def __init__(self, ctx, d_xyz_ptr, n_vertices, d_tri_ptr, n_triangles):
        self.ctx, self.handle = ctx, None
        h = C.c_void_p()
        L.check(ctx.lib.r3d_mesh_index_create(ctx.handle, d_xyz_ptr, _count(n_vertices, "n_vertices"), d_tri_ptr,
                                              _count(n_triangles, "n_triangles"), C.byref(h)))
        self.handle = h.value
        ctx.adopt(self)

    def query(self, d_points_ptr, n_points, d_dist_ptr, d_tri_ptr=None, d_closest_ptr=None, signed=False, want_groups=False):
        """Distances [n] float32 (signed by the winning triangle's face normal with signed=True), winners [n] uint32 and closest
        points [n][3] float32 (both optional) for the points at d_points_ptr.  want_groups: returns the number of 32-triangle
        group evaluations (synchronises); otherwise None, and the call is asynchronous."""
        g = C.c_int64()
        L.check(self.ctx.lib.r3d_mesh_index_query(self.handle, d_points_ptr, _count(n_points, "n_points"), SIGNED if signed else 0,
                                                  d_dist_ptr, d_tri_ptr, d_closest_ptr, C.byref(g) if want_groups else None))
        return g.value if want_groups else None

    def close(self):
        if self.handle:
            self.ctx.lib.r3d_mesh_index_destroy(self.handle)
            self.handle = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def cloud_to_cloud_distance_device(ctx, d_src, n_src, d_tgt, n_tgt, d_dist, d_idx):
    """d_dist [n_src] float32 = the distance from every source point to its exact nearest target point, d_idx [n_src] uint32 =
    that point's row (r3d_nn_index_query, then r3d_sqrt_f32_inplace on its d2).  n_tgt >= 1.  Asynchronous."""
    index = NNIndex(ctx, d_tgt, _count(n_tgt, "n_tgt"))
    try:
        n = _count(n_src, "n_src")
        if n:
            index.query(d_src, n, d_idx, d_dist)
            L.check(ctx.lib.r3d_sqrt_f32_inplace(ctx.handle, d_dist, n))
    finally:
        index.close()


def distance_stats_device(ctx, d_values, n, thresholds=(), bin_width=None, n_bins=0, squared=False):
    """r3d_distance_stats of the [n] float32 values at d_values, as the dict distance_stats returns.  Synchronises."""
    thr = np.ascontiguousarray(np.asarray(thresholds, np.float64).reshape(-1))
    if len(thr) > MAX_THRESHOLDS:
        raise ValueError("at most %d thresholds, got %d" % (MAX_THRESHOLDS, len(thr)))
    if isinstance(n_bins, bool) or not isinstance(n_bins, (int, np.integer)) or not 0 <= int(n_bins) <= MAX_BINS:
        raise ValueError("n_bins must be an integer in [0, %d], got %r" % (MAX_BINS, n_bins))
    n_bins = int(n_bins)
    if n_bins and bin_width is None:
        raise ValueError("a histogram needs a bin_width")
    stats, counts, hist = np.zeros(6), np.zeros(max(len(thr), 1), np.int64), np.zeros(max(n_bins, 1), np.uint64)
    L.check(ctx.lib.r3d_distance_stats(ctx.handle, d_values, _count(n, "n"), 1 if squared else 0, thr.ctypes.data if len(thr) else None,
                                       len(thr), float(bin_width) if n_bins else 0.0, n_bins, stats.ctypes.data,
                                       counts.ctypes.data if len(thr) else None, hist.ctypes.data if n_bins else None))
    return stats_dict(stats, counts[:len(thr)], hist[:n_bins])


def stats_dict(stats, counts, hist):
    """The six device sums and the integer counts as a dict: n, n_nonfinite, sum, sum_sq, min, max, mean, rms, std (population;
    NaN without a finite element), counts [T] int64 and hist [n_bins] uint64."""
    n, bad, s, ss, lo, hi = (float(v) for v in stats)
    out = {"n": int(n), "n_nonfinite": int(bad), "sum": s, "sum_sq": ss, "min": lo, "max": hi, "counts": np.asarray(counts, np.int64),
           "hist": np.asarray(hist, np.uint64)}
    if n > 0:
        mean = s / n
        out.update(mean=mean, rms=math.sqrt(ss / n), std=math.sqrt(max(ss / n - mean * mean, 0.0)))
    else:
        out.update(mean=float("nan"), rms=float("nan"), std=float("nan"))
    return out


def distance_colors_device(ctx, d_dist, n, d_max, d_rgba):
    """d_rgba [n] uint32 = the blue-green-yellow-red ramp of min(|d| / d_max, 1) (grey where d is not finite).  Asynchronous."""
    L.check(ctx.lib.r3d_distance_colors(ctx.handle, d_dist, _count(n, "n"), float(d_max), d_rgba))


def cloud_to_cloud_distance(src, tgt, ctx=None):
    """(distances [N] float32, indices [N] uint32): from every point of src to its exact nearest point of tgt (at least one)."""
    src, tgt = _points(src, "src"), _points(tgt, "tgt")
    if len(tgt) == 0:
        raise ValueError("the target cloud is empty")
    ctx = ctx or default_context()
    with ctx.buffers() as B:
        d_src, d_tgt = B.upload(src), B.upload(tgt)
        d_dist, d_idx = B.alloc(len(src) * 4), B.alloc(len(src) * 4)
        cloud_to_cloud_distance_device(ctx, d_src.ptr, len(src), d_tgt.ptr, len(tgt), d_dist.ptr, d_idx.ptr)
        return d_dist.download_array(np.float32, (len(src),)), d_idx.download_array(np.uint32, (len(src),))


def cloud_to_mesh_distance(points, vertices, triangles, signed=False, return_closest=False, ctx=None):
    """(distances [N] float32, triangles [N] uint32[, closest [N,3] float32]): from every point to the nearest valid triangle of
    the mesh (vertices [V,3], triangles [M,3] integers), the lowest index winning ties.  signed: negative behind the winning
    triangle's face.  A point with a non-finite coordinate, or a mesh without a valid triangle: +inf, 0xFFFFFFFF, NaN."""
    pts, v, t = _points(points, "points"), _points(vertices, "vertices"), _triangles(triangles)
    ctx = ctx or default_context()
    with ctx.buffers() as B:
        d_pts, d_v, d_t = B.upload(pts), B.upload(v), B.upload(t)
        n = len(pts)
        d_dist, d_win = B.alloc(n * 4), B.alloc(n * 4)
        d_q = B.alloc(n * 12) if return_closest else None
        index = B.adopt(MeshIndex(ctx, d_v.ptr, len(v), d_t.ptr, len(t)))
        index.query(d_pts.ptr, n, d_dist.ptr, d_win.ptr, d_q.ptr if d_q else None, signed=signed)
        out = (d_dist.download_array(np.float32, (n,)), d_win.download_array(np.uint32, (n,)))
        return out + (d_q.download_array(np.float32, (n, 3)),) if return_closest else out


def distance_stats(d, thresholds=(), bin_width=None, n_bins=0, squared=False, ctx=None):
    """Statistics of the float32 distances d (their roots with squared=True): a dict with n, n_nonfinite, sum, sum_sq, min, max,
    mean, rms, std, counts (d <= threshold, per threshold) and hist (n_bins bins of bin_width, the last one open).  Non-finite
    values are counted apart.  Fixed-order device sums: the same bits run to run."""
    d = np.ascontiguousarray(np.asarray(d, np.float32).reshape(-1))
    ctx = ctx or default_context()
    with ctx.buffers() as B:
        return distance_stats_device(ctx, B.upload(d).ptr, len(d), thresholds, bin_width, n_bins, squared)


def distance_colors(d, d_max, ctx=None):
    """[N] uint32 colour words (r | g << 8 | b << 16, what cloud_io.write_ply_rgb takes) of the distances d."""
    d = np.ascontiguousarray(np.asarray(d, np.float32).reshape(-1))
    ctx = ctx or default_context()
    with ctx.buffers() as B:
        d_rgba = B.alloc(len(d) * 4)
        distance_colors_device(ctx, B.upload(d).ptr, len(d), d_max, d_rgba.ptr)
        return d_rgba.download_array(np.uint32, (len(d),))


def _side(x, what):
    """(points [N,3] float32, triangles [M,3] int32 or None)"""
    if isinstance(x, (tuple, list)) and len(x) == 2 and np.asarray(x[1]).dtype.kind in "iu" and np.asarray(x[0]).ndim == 2:
        return _points(x[0], what + " vertices"), _triangles(x[1])
    return _points(x, what), None


def directed_numbers(stats, threshold_count):
    """mean, rms, max and the share within the threshold of one direction, from a distance_stats dict"""
    n = stats["n"]
    return {"n": n, "mean": stats["mean"], "rms": stats["rms"], "max": stats["max"] if n else float("nan"),
            "within": threshold_count / n if n else float("nan")}


def combine(accuracy, completeness, threshold):
    """The report of evaluate_reconstruction from its two directions."""
    p, r = accuracy["within"], completeness["within"]
    f = 2.0 * p * r / (p + r) if p + r > 0 else 0.0
    return {"threshold": float(threshold), "accuracy": accuracy, "completeness": completeness, "precision": p, "recall": r, "f_score": f,
            "chamfer": accuracy["mean"] + completeness["mean"]}


def _directed(ctx, B, d_pts, n, other, d_other, threshold):
    """distances from the n points at d_pts to `other` (points, triangles or None) whose arrays sit in d_other; (numbers, d_dist)"""
    pts, tri = other
    d_dist = B.alloc(n * 4)
    if tri is None:
        if len(pts) == 0:
            raise ValueError("a cloud to compare with is empty")
        cloud_to_cloud_distance_device(ctx, d_pts, n, d_other[0].ptr, len(pts), d_dist.ptr, B.alloc(n * 4).ptr)
    else:
        with MeshIndex(ctx, d_other[0].ptr, len(pts), d_other[1].ptr, len(tri)) as index:
            index.query(d_pts, n, d_dist.ptr)
            ctx.sync()
    st = distance_stats_device(ctx, d_dist.ptr, n, (threshold,))
    return directed_numbers(st, int(st["counts"][0])), d_dist


def evaluate_reconstruction(recon, truth, threshold, ctx=None, return_distances=False):
    """Accuracy and completeness of a reconstruction against the truth.  Each side is an [N,3] cloud or a (vertices, triangles)
    mesh; the samples of a mesh are its vertices.  accuracy: from the reconstruction's samples to the truth (to its nearest
    triangle where the truth is a mesh, to its nearest point otherwise); completeness: from the truth's samples to the
    reconstruction.  Returns a dict: accuracy and completeness (n, mean, rms, max, within = the share of distances <= threshold),
    precision = accuracy's share, recall = completeness' share, f_score = their harmonic mean, chamfer = the sum of the two mean
    distances.  Samples whose distance is not finite (a NaN point) take no part.  return_distances: also the two [N] float32
    distance arrays."""
    threshold = float(threshold)
    if not threshold >= 0.0:
        raise ValueError("threshold must be >= 0, got %r" % threshold)
    rec, tru = _side(recon, "recon"), _side(truth, "truth")
    ctx = ctx or default_context()
    with ctx.buffers() as B:
        d_rec = [B.upload(rec[0])] + ([B.upload(rec[1])] if rec[1] is not None else [])
        d_tru = [B.upload(tru[0])] + ([B.upload(tru[1])] if tru[1] is not None else [])
        acc, d_acc = _directed(ctx, B, d_rec[0].ptr, len(rec[0]), tru, d_tru, threshold)
        com, d_com = _directed(ctx, B, d_tru[0].ptr, len(tru[0]), rec, d_rec, threshold)
        out = combine(acc, com, threshold)
        if return_distances:
            return out, d_acc.download_array(np.float32, (len(rec[0]),)), d_com.download_array(np.float32, (len(tru[0]),))
        return out
