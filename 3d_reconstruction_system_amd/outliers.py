"""Outlier removal over exact k nearest neighbours on the MI355X: the statistical and radius filters users of Open3D call
after fusion (remove_statistical_outlier / remove_radius_outlier; no parity with Open3D is claimed), built on an r3d_nn_index
of the cloud itself.  Semantics: include/r3d.h (r3d_nn_index_knn_self, r3d_outlier_statistical, r3d_outlier_radius,
r3d_select_rows) and DESIGN.md section 4.5e.

Host functions take an [N,3] cloud and return the kept rows, their original row numbers (to filter colour or other per-point
data with) and the per-point score or count.  The *_device functions take an NNIndex over a device cloud and device pointers.
"""
import collections
import ctypes as C

import numpy as np

from . import _lib as L
from ._args import positive as _check_positive
from .device import BufferScope, default_context
from .icp import NNIndex

SORStats = collections.namedtuple("SORStats", ["V", "mu", "sigma", "T"])
SORStats.__doc__ = "Scored points V, mean score mu, its sample deviation sigma (0 when V <= 1), threshold T = mu + ratio sigma."
StatisticalOutliers = collections.namedtuple("StatisticalOutliers", ["xyz", "rows", "score", "stats"])
StatisticalOutliers.__doc__ = ("Kept xyz [M,3] float32, their original rows [M] uint32, the score m_i of every input point [N] "
                               "float64 (+inf: fewer than k neighbours), SORStats.")
RadiusOutliers = collections.namedtuple("RadiusOutliers", ["xyz", "rows", "count"])
RadiusOutliers.__doc__ = ("Kept xyz [M,3] float32, their original rows [M] uint32, the neighbour count of every input point "
                          "[N] uint32, saturated at nb_points.")


def _cloud(xyz):
    xyz = np.ascontiguousarray(xyz, dtype=np.float32)
    if xyz.ndim != 2 or xyz.shape[1] != 3:
        raise ValueError("cloud must be [N,3]")
    if xyz.shape[0] >= 1 << 32:
        raise ValueError("cloud too large for uint32 row numbers")
    return xyz


def _check_k(k, what="k"):
    if isinstance(k, bool) or not isinstance(k, (int, np.integer)) or not 1 <= int(k) <= 32:
        raise ValueError("%s must be an integer in [1, 32], got %r" % (what, k))
    return int(k)


def _check_min_points(n):
    if isinstance(n, bool) or not isinstance(n, (int, np.integer)) or int(n) < 1:
        raise ValueError("nb_points must be an integer >= 1, got %r" % (n,))
    return int(n)


# ---- device pointers -----------------------------------------------------------------------------------------------------

def knn_device(index, k, d_idx, d_d2=None):
    """[n][k] neighbour rows (uint32) and d2 (float32, d_d2 may be None) of the index's own points; asynchronous."""
    index.knn_self(_check_k(k), d_idx, d_d2)


def statistical_outlier_device(index, nb_neighbors, std_ratio, d_keep, d_score=None):
    """d_keep [n] uint8 (1 = kept), d_score [n] float64 (optional); returns (kept, SORStats).  Synchronous."""
    k, ratio = _check_k(nb_neighbors, "nb_neighbors"), _check_positive(std_ratio, "std_ratio")
    stats, kept = (C.c_double * 4)(), C.c_int64()
    L.check(index.ctx.lib.r3d_outlier_statistical(index.handle, k, ratio, d_keep, d_score, stats, C.byref(kept)))
    return kept.value, SORStats(int(stats[0]), stats[1], stats[2], stats[3])


def radius_outlier_device(index, nb_points, radius, d_keep, d_count=None):
    """d_keep [n] uint8 (1 = kept), d_count [n] uint32 (optional, saturated at nb_points); returns the kept count.
    Synchronous."""
    m, r = _check_min_points(nb_points), _check_positive(radius, "radius")
    kept = C.c_int64()
    L.check(index.ctx.lib.r3d_outlier_radius(index.handle, r, m, d_keep, d_count, C.byref(kept)))
    return kept.value


def select_rows_device(ctx, d_xyz, n, d_keep, d_xyz_out, d_rows_out=None):
    """The rows with d_keep[i] != 0, in order, into d_xyz_out (and their row numbers into d_rows_out); returns how many."""
    m = C.c_int64()
    L.check(ctx.lib.r3d_select_rows(ctx.handle, d_xyz, int(n), d_keep, d_xyz_out, d_rows_out, C.byref(m)))
    return m.value


# ---- host arrays ---------------------------------------------------------------------------------------------------------

class Cloud(BufferScope):
    """The buffer scope of one call over a cloud: the cloud in HBM (d_xyz) and its NNIndex (index) are its first two members, the
    call's other buffers follow; everything goes at close()."""

    def __init__(self, ctx, xyz):
        super().__init__(ctx)
        self.n = xyz.shape[0]
        try:
            self.d_xyz = self.upload(xyz)
            self.index = self.adopt(NNIndex(ctx, self.d_xyz.ptr, self.n))
        except BaseException:
            self.close()
            raise

    def select(self, d_keep, m):
        """(xyz [m,3], rows [m]) of the kept rows."""
        if m == 0:
            return np.zeros((0, 3), np.float32), np.zeros(0, np.uint32)
        d_out, d_rows = self.alloc(m * 12), self.alloc(m * 4)
        got = select_rows_device(self.ctx, self.d_xyz.ptr, self.n, d_keep.ptr, d_out.ptr, d_rows.ptr)
        assert got == m, (got, m)
        return d_out.download_array(np.float32, (m, 3)), d_rows.download(np.uint32, m)


def knn(xyz, k, ctx=None):
    """(idx [N,k] uint32, d2 [N,k] float32): the k nearest OTHER points of every point, ascending (d2, row), with the
    library's fp32 distance; points with fewer than k finite neighbours get (0xffffffff, +inf) tails."""
    xyz, k = _cloud(xyz), _check_k(k)
    ctx = ctx or default_context()
    n = xyz.shape[0]
    if n == 0:
        return np.zeros((0, k), np.uint32), np.zeros((0, k), np.float32)
    with Cloud(ctx, xyz) as c:
        d_idx, d_d2 = c.alloc(n * k * 4), c.alloc(n * k * 4)
        knn_device(c.index, k, d_idx.ptr, d_d2.ptr)
        return d_idx.download_array(np.uint32, (n, k)), d_d2.download_array(np.float32, (n, k))


def remove_statistical_outlier(xyz, nb_neighbors=20, std_ratio=2.0, ctx=None):
    """StatisticalOutliers: keep point i iff it has nb_neighbors neighbours and its mean neighbour distance m_i is at most
    mu + std_ratio * sigma over all such points."""
    xyz, k, ratio = _cloud(xyz), _check_k(nb_neighbors, "nb_neighbors"), _check_positive(std_ratio, "std_ratio")
    ctx = ctx or default_context()
    n = xyz.shape[0]
    if n == 0:
        return StatisticalOutliers(np.zeros((0, 3), np.float32), np.zeros(0, np.uint32), np.zeros(0),
                                   SORStats(0, float("nan"), 0.0, float("nan")))
    with Cloud(ctx, xyz) as c:
        d_keep, d_score = c.alloc(n), c.alloc(n * 8)
        m, stats = statistical_outlier_device(c.index, k, ratio, d_keep.ptr, d_score.ptr)
        kept, rows = c.select(d_keep, m)
        return StatisticalOutliers(kept, rows, d_score.download(np.float64, n), stats)


def remove_radius_outlier(xyz, nb_points, radius, ctx=None):
    """RadiusOutliers: keep point i iff at least nb_points other points lie within `radius` (d2 <= (float) radius^2)."""
    xyz, m_pts, r = _cloud(xyz), _check_min_points(nb_points), _check_positive(radius, "radius")
    ctx = ctx or default_context()
    n = xyz.shape[0]
    if n == 0:
        return RadiusOutliers(np.zeros((0, 3), np.float32), np.zeros(0, np.uint32), np.zeros(0, np.uint32))
    with Cloud(ctx, xyz) as c:
        d_keep, d_count = c.alloc(n), c.alloc(n * 4)
        m = radius_outlier_device(c.index, m_pts, r, d_keep.ptr, d_count.ptr)
        kept, rows = c.select(d_keep, m)
        return RadiusOutliers(kept, rows, d_count.download(np.uint32, n))
