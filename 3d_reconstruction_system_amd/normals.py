"""Normals of an unorganised cloud on the MI355X: the smallest eigenvector of the covariance of every point's k nearest
neighbours, oriented towards the camera that saw the point (Open3D's estimate_normals /
orient_normals_towards_camera_location, in the same toolbox as the outlier filters; no parity with Open3D is claimed).  The
search, the covariance and the eigen-solve are one launch over an r3d_nn_index of the cloud itself: the neighbour lists never
leave registers.  Semantics: include/r3d.h (r3d_normals_knn) and DESIGN.md section 4.5g.

Host functions take an [N,3] cloud; estimate_normals_device takes an NNIndex over a device cloud and device pointers.  The
normals are what icp.icp_point_to_plane(..., tgt_normals=...) needs for a fused, downsampled or filtered target, and what
cloud_io.write_ply_normals stores for MeshLab.
"""
import collections
import math

import numpy as np

from . import _lib as L
from .device import default_context
from .outliers import Cloud, _cloud
from .poses import pose_table

Normals = collections.namedtuple("Normals", ["normals", "curvature", "count"])
Normals.__doc__ = ("Unit normals [N,3] float32 (zero rows: no plane), surface variation l0 / (l0 + l1 + l2) [N] float32, "
                   "neighbours used [N] uint32.")


def _check_k(k):
    if isinstance(k, bool) or not isinstance(k, (int, np.integer)) or not 3 <= int(k) <= 32:
        raise ValueError("k must be an integer in [3, 32], got %r" % (k,))
    return int(k)


def _check_radius(radius):
    """None (no radius) or a finite number > 0 -> the C ABI's double (0.0 = none)."""
    if radius is None:
        return 0.0
    try:
        r = float(radius)
    except (TypeError, ValueError):
        raise ValueError("radius must be None or a finite number > 0, got %r" % (radius,))
    if not (math.isfinite(r) and r > 0.0):
        raise ValueError("radius must be None or a finite number > 0, got %r" % (radius,))
    return r


def _check_views(viewpoint, viewpoints, points_per_view):
    """-> ([V,3] float64 or None, points_per_view)."""
    if viewpoint is not None and viewpoints is not None:
        raise ValueError("give viewpoint or viewpoints, not both")
    if viewpoint is not None:
        v = np.asarray(viewpoint, dtype=np.float64)
        if v.shape != (3,) or not np.isfinite(v).all():
            raise ValueError("viewpoint must be three finite numbers, got %r" % (viewpoint,))
        if points_per_view is not None:
            raise ValueError("points_per_view goes with viewpoints")
        return np.ascontiguousarray(v.reshape(1, 3)), 1
    if viewpoints is None:
        if points_per_view is not None:
            raise ValueError("points_per_view goes with viewpoints")
        return None, 1
    v = np.ascontiguousarray(viewpoints, dtype=np.float64)
    if v.ndim != 2 or v.shape[1] != 3 or v.shape[0] < 1 or not np.isfinite(v).all():
        raise ValueError("viewpoints must be [F,3] finite numbers with F >= 1")
    if isinstance(points_per_view, bool) or not isinstance(points_per_view, (int, np.integer)) or int(points_per_view) < 1:
        raise ValueError("viewpoints need points_per_view, an integer >= 1, got %r" % (points_per_view,))
    return v, int(points_per_view)


def fused_viewpoints(quats_xyzw, ts):
    """[F,3] float64 camera centres -Rinv t of the poses fuse_frames takes: the viewpoints of a fused cloud, frame by frame
    (estimate_normals(fuse_frames(depth, q, t), viewpoints=fused_viewpoints(q, t), points_per_view=H*W))."""
    tab = pose_table(quats_xyzw, ts)
    return np.ascontiguousarray(-np.einsum("fab,fb->fa", tab[:, :9].reshape(-1, 3, 3), tab[:, 9:]))


def estimate_normals_device(index, k, d_normals, d_curvature=None, d_cov=None, d_count=None, radius=None, viewpoint=None,
                            viewpoints=None, points_per_view=None):
    """Normals of the index's own cloud into d_normals [n][3] float32; optional d_curvature [n] float32, d_cov [n][6] float64
    (xx xy xz yy yz zz), d_count [n] uint32.  Asynchronous on the index's context."""
    k, r = _check_k(k), _check_radius(radius)
    views, ppv = _check_views(viewpoint, viewpoints, points_per_view)
    index.normals_knn(k, r, views, ppv, d_normals, d_curvature, d_cov, d_count)


def estimate_normals(xyz, k=20, radius=None, viewpoint=None, viewpoints=None, points_per_view=None, ctx=None):
    """Normals: for every point the unit normal of the plane through its k nearest neighbours (those within `radius` when
    given), its surface variation and the neighbours used.  viewpoint: one camera position for the whole cloud; viewpoints
    [F,3] + points_per_view: row i was seen from viewpoints[min(i // points_per_view, F - 1)]; neither: the largest component
    of every normal is positive.  Points without a plane (non-finite, fewer than two neighbours, all on one line) get zeros."""
    xyz, k, r = _cloud(xyz), _check_k(k), _check_radius(radius)
    views, ppv = _check_views(viewpoint, viewpoints, points_per_view)
    n = xyz.shape[0]
    if n == 0:
        return Normals(np.zeros((0, 3), np.float32), np.zeros(0, np.float32), np.zeros(0, np.uint32))
    with Cloud(ctx or default_context(), xyz) as c:
        d_n, d_c, d_m = c.alloc(n * 12), c.alloc(n * 4), c.alloc(n * 4)
        c.index.normals_knn(k, r, views, ppv, d_n.ptr, d_c.ptr, None, d_m.ptr)
        return Normals(d_n.download_array(np.float32, (n, 3)), d_c.download(np.float32, n), d_m.download(np.uint32, n))


def estimate_covariances(xyz, k, radius=None, ctx=None):
    """[N,6] float64: the neighbourhood covariance (xx xy xz yy yz zz) of every point, zero rows where there is no plane."""
    xyz, k, r = _cloud(xyz), _check_k(k), _check_radius(radius)
    n = xyz.shape[0]
    if n == 0:
        return np.zeros((0, 6))
    with Cloud(ctx or default_context(), xyz) as c:
        d_n, d_cov = c.alloc(n * 12), c.alloc(n * 48)
        c.index.normals_knn(k, r, None, 1, d_n.ptr, None, d_cov.ptr, None)
        return d_cov.download_array(np.float64, (n, 6))
