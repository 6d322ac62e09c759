"""Reference computation for the k-NN / outlier tests (include/r3d.h: r3d_nn_index_knn_self, r3d_outlier_statistical,
r3d_outlier_radius).  Pairs are ranked by the library's fp32 expression (oracle.icp_ref.pair_d2; its emulated fma may differ
from the device's on about 2^-29 of pairs), ties by row.  Small clouds: brute force.  Larger ones: a scipy cKDTree superset
over the DISTINCT rows (every row within the fp64 k-th distance x (1 + 1e-5)), re-ranked with pair_d2; identical rows are
grouped first, so a point with k identical others costs O(k) and not O(copies)."""
import numpy as np

from oracle.icp_ref import pair_d2 as _pair_d2


def pair_d2(a, b):
    with np.errstate(invalid="ignore", over="ignore"):
        return _pair_d2(a, b)


NO_ROW = np.uint32(0xffffffff)


def _finite_rows(xyz):
    return np.isfinite(xyz).all(axis=1)


def knn_brute(xyz, k, chunk=256):
    """(idx [N,k] uint32, d2 [N,k] float32), ascending (d2, row); missing tails (0xffffffff, +inf)."""
    xyz = np.asarray(xyz, np.float32)
    n = xyz.shape[0]
    ok = _finite_rows(xyz)
    idx = np.full((n, k), NO_ROW, np.uint32)
    d2 = np.full((n, k), np.inf, np.float32)
    for lo in range(0, n, chunk):
        d = pair_d2(xyz[lo:lo + chunk], xyz)
        d[~np.isfinite(d)] = np.inf
        r = np.arange(d.shape[0])
        d[r, lo + r] = np.inf
        d[:, ~ok] = np.inf
        o = np.argsort(d, axis=1, kind="stable")[:, :k]          # stable: lowest row first among equal d2
        dd = np.take_along_axis(d, o, axis=1)
        real = np.isfinite(dd)
        w = min(k, o.shape[1])
        idx[lo:lo + chunk, :w] = np.where(real, o, NO_ROW)
        d2[lo:lo + chunk, :w] = dd
    idx[~ok] = NO_ROW
    d2[~ok] = np.inf
    return idx, d2


class _Distinct:
    """The finite rows grouped by identical coordinates, with a cKDTree over the distinct points."""

    def __init__(self, xyz):
        from scipy.spatial import cKDTree
        self.xyz = np.asarray(xyz, np.float32)
        self.rows = np.flatnonzero(_finite_rows(self.xyz))
        self.u, inv, self.mult = np.unique(self.xyz[self.rows], axis=0, return_inverse=True, return_counts=True)
        inv = inv.reshape(-1)
        order = np.argsort(inv, kind="stable")
        self.members = np.split(self.rows[order], np.cumsum(self.mult)[:-1])   # ascending rows of each distinct point
        self.tree = cKDTree(self.u.astype(np.float64))

    def ball_rows(self, u, radius):
        """Rows of every distinct point within `radius` (fp64) of distinct point u, ascending."""
        nb = self.tree.query_ball_point(self.u[u].astype(np.float64), radius)
        return np.sort(np.concatenate([self.members[v] for v in nb]))

    def kth_distance(self, u, k):
        """fp64 distance to the k-th nearest OTHER row of distinct point u (inf if there are fewer)."""
        q = min(self.u.shape[0], k + 1)
        dist, nb = self.tree.query(self.u[u].astype(np.float64), k=q)
        dist, nb = np.atleast_1d(dist), np.atleast_1d(nb)
        have = 0
        for dv, v in zip(dist, nb):
            have += self.mult[v] - (1 if v == u else 0)
            if have >= k:
                return dv
        return np.inf


def knn_tree(xyz, k):
    """knn_brute's answer through the cKDTree superset."""
    xyz = np.asarray(xyz, np.float32)
    n = xyz.shape[0]
    idx = np.full((n, k), NO_ROW, np.uint32)
    d2 = np.full((n, k), np.inf, np.float32)
    if n == 0:
        return idx, d2
    D = _Distinct(xyz)
    for u in range(D.u.shape[0]):
        kth = D.kth_distance(u, k)
        cand = D.rows if not np.isfinite(kth) else D.ball_rows(u, kth * (1 + 1e-5))
        d = pair_d2(D.u[u][None, :], xyz[cand])[0]
        d[~np.isfinite(d)] = np.inf
        o = np.argsort(d, kind="stable")[:k + 1]                 # the k + 1 first: one of them may be the row itself
        top, topd = cand[o], d[o]
        mine = D.members[u]
        keep = top[None, :] != mine[:, None]                     # every copy drops itself, keeps the order of the rest
        pick = np.argsort(~keep, axis=1, kind="stable")[:, :k]
        rows_sel, d_sel = top[pick], topd[pick]
        valid = np.take_along_axis(keep, pick, axis=1) & np.isfinite(d_sel)
        w = pick.shape[1]
        idx[mine, :w] = np.where(valid, rows_sel, NO_ROW)
        d2[mine, :w] = np.where(valid, d_sel, np.inf)
    return idx, d2


def knn(xyz, k):
    return knn_brute(xyz, k) if len(xyz) <= 4200 else knn_tree(xyz, k)


def sor(xyz, k, std_ratio, lists=None):
    """(m [N] f64, keep [N] bool, (V, mu, sigma, T)) from the k-lists (computed when not given)."""
    _, d2 = lists if lists is not None else knn(xyz, k)
    d2 = d2[:, :k]
    scored = np.isfinite(d2).all(axis=1)
    m = np.full(d2.shape[0], np.inf)
    s = np.zeros(d2.shape[0])
    for t in range(k):                                           # fp64, in list order
        s = s + np.sqrt(d2[:, t].astype(np.float64))
    m[scored] = s[scored] / k
    V = int(scored.sum())
    mu = m[scored].sum() / V if V else float("nan")
    sigma = float(np.sqrt(((m[scored] - mu) ** 2).sum() / (V - 1))) if V > 1 else 0.0
    T = mu + std_ratio * sigma
    return m, scored & (m <= T), (V, mu, sigma, T)


def r2_of(radius):
    return np.float32(np.float64(radius) * np.float64(radius))


def ror_counts(xyz, radius):
    """c_i = #{j != i, finite d2(i,j) <= (float)(radius^2)} (exact, unsaturated)."""
    xyz = np.asarray(xyz, np.float32)
    r2 = r2_of(radius)
    c = np.zeros(xyz.shape[0], np.int64)
    if xyz.shape[0] == 0:
        return c
    D = _Distinct(xyz)
    for u in range(D.u.shape[0]):
        cand = D.ball_rows(u, np.sqrt(np.float64(r2)) * (1 + 1e-5))
        d = pair_d2(D.u[u][None, :], xyz[cand])[0]
        c[D.members[u]] = int((d <= r2).sum()) - 1               # the row itself is in the ball at d2 = 0
    return c


def ror(xyz, min_points, radius):
    """(saturated counts [N] int64, keep [N] bool)."""
    c = ror_counts(xyz, radius)
    return np.minimum(c, min_points), c >= min_points
