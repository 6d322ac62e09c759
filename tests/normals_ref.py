"""Reference computation for the normal-estimation tests: a NumPy restatement of include/r3d.h's r3d_normals_knn that takes the
k-lists (r3d_nn_index_knn_self's idx / d2) as input.  Counts and covariances follow the specified fp64 operation order, so they
are compared bit for bit; eigenvalues and eigenvectors come from numpy.linalg.eigh and are compared within the bounds the tests
derive."""
import numpy as np

NO_ROW = np.uint32(0xffffffff)
AXES = ((0, 0), (0, 1), (0, 2), (1, 1), (1, 2), (2, 2))          # xx xy xz yy yz zz


def r2_of(radius):
    return np.float32(np.float64(radius) * np.float64(radius))


def members(xyz, idx, d2, radius=None):
    """[N,k] bool: list entries that belong to the neighbourhood (real, within the radius, of a finite point)."""
    xyz = np.asarray(xyz, np.float32)
    m = (idx != NO_ROW) & np.isfinite(d2) & np.isfinite(xyz).all(axis=1)[:, None]
    if radius is not None and radius > 0:
        m &= d2 <= r2_of(radius)
    # the lists ascend, so "cut at the first entry beyond the radius" and "keep the entries within it" are the same set
    assert not (m[:, 1:] & ~m[:, :-1]).any()
    return m


def raw_covariance(xyz, idx, d2, radius=None):
    """(count [N] uint32, C [N,6] float64) in the specified order: e about the query point, S1 and S2 over the list from
    0.0, m = count + 1, C_ab = (S2_ab - S1_a * S1_b / m) / m.  No row is zeroed here."""
    xyz = np.asarray(xyz, np.float32)
    n, k = idx.shape
    mem = members(xyz, idx, d2, radius)
    p64 = xyz.astype(np.float64)
    s1 = np.zeros((n, 3))
    s2 = np.zeros((n, 6))
    with np.errstate(invalid="ignore", over="ignore"):
        for t in range(k):
            j = np.where(mem[:, t], idx[:, t], 0).astype(np.int64)
            e = np.where(mem[:, t, None], p64[j] - p64, 0.0)
            s1 = s1 + e
            for c, (a, b) in enumerate(AXES):
                s2[:, c] = s2[:, c] + e[:, a] * e[:, b]
        count = mem.sum(axis=1).astype(np.uint32)
        m = (count + 1).astype(np.float64)
        C = np.stack([(s2[:, c] - s1[:, a] * s1[:, b] / m) / m for c, (a, b) in enumerate(AXES)], axis=1)
    return count, C


def matrices(C6):
    M = np.empty((C6.shape[0], 3, 3))
    for c, (a, b) in enumerate(AXES):
        M[:, a, b] = C6[:, c]
        M[:, b, a] = C6[:, c]
    return M


class Result:
    """count, cov (zero where there is no plane), plane (bool), l [N,3] ascending eigenvalues, n [N,3] float64 unit
    eigenvector of l0 (unoriented), curvature float64, line (bool: l1 within rounding of 0 -- the plane decision is then
    not determined by the data and a test may accept either answer)."""


def normals(xyz, idx, d2, radius=None):
    xyz = np.asarray(xyz, np.float32)
    count, C = raw_covariance(xyz, idx, d2, radius)
    finite = np.isfinite(xyz).all(axis=1)
    can = finite & (count >= 2) & np.isfinite(C).all(axis=1)
    l = np.zeros((xyz.shape[0], 3))
    v = np.zeros((xyz.shape[0], 3))
    if can.any():
        w, V = np.linalg.eigh(matrices(C[can]))
        l[can] = w
        v[can] = V[:, :, 0]
    r = Result()
    r.line = can & (l[:, 1] <= 1e-13 * l[:, 2]) & (l[:, 2] > 0)
    r.plane = can & (l[:, 1] > 0)
    r.count = count
    r.raw_cov = C
    r.cov = np.where(r.plane[:, None], C, 0.0)
    r.l = np.where(r.plane[:, None], l, 0.0)
    r.n = np.where(r.plane[:, None], v, 0.0)
    s = np.maximum(r.l[:, 0], 0.0) + r.l[:, 1] + r.l[:, 2]
    with np.errstate(invalid="ignore", divide="ignore"):
        r.curvature = np.where(s > 0, np.maximum(r.l[:, 0], 0.0) / s, 0.0)
    return r


def orient(n, xyz, viewpoints=None, points_per_view=1):
    """The specification's sign rule applied to unit vectors n [N,3] float64."""
    n = np.array(n, dtype=np.float64)
    if viewpoints is None:
        big = np.argmax(np.abs(n), axis=1)                        # first maximum: the lowest axis on ties
        flip = n[np.arange(n.shape[0]), big] < 0
    else:
        viewpoints = np.asarray(viewpoints, np.float64).reshape(-1, 3)
        v = np.minimum(np.arange(n.shape[0]) // int(points_per_view), viewpoints.shape[0] - 1)
        with np.errstate(invalid="ignore"):
            flip = (n * (viewpoints[v] - np.asarray(xyz, np.float32).astype(np.float64))).sum(axis=1) < 0
    n[flip] = -n[flip]
    return n
