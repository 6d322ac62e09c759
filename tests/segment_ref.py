"""NumPy restatement of include/r3d.h's r3d_segment_plane: the counter-based sampler in Python ints, the hypotheses in fp64, the
count in f32 arrays (NumPy never fuses a multiply with an add), the refit and the final mask in fp64.  Test infrastructure; the
scene builders the host and the GPU tests share live here too."""
import collections

import numpy as np

M64 = (1 << 64) - 1
GOLDEN = 0x9E3779B97F4A7C15


def splitmix64(z):
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & M64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & M64
    return z ^ (z >> 31)


def rows_of(seed, h, n):
    return tuple((splitmix64((seed + (3 * h + j + 1) * GOLDEN) & M64) * n) >> 64 for j in range(3))


def all_rows(seed, H, n):
    return np.array([rows_of(seed, h, n) for h in range(H)], dtype=np.int64).reshape(H, 3)


Hypotheses = collections.namedtuple("Hypotheses", ["rows", "valid", "anchor", "normal", "normal64"])


def hypotheses(xyz, H, seed):
    """rows [H,3], valid [H], anchor [H,3] f32, normal [H,3] f32 (NaN where invalid), normal64 [H,3]."""
    xyz = np.ascontiguousarray(xyz, np.float32)
    rows = all_rows(seed, H, xyz.shape[0])
    with np.errstate(all="ignore"):
        a, b, c = (xyz[rows[:, j]].astype(np.float64) for j in range(3))
        u, v = b - a, c - a
        N = np.stack([u[:, 1] * v[:, 2] - u[:, 2] * v[:, 1], u[:, 2] * v[:, 0] - u[:, 0] * v[:, 2],
                      u[:, 0] * v[:, 1] - u[:, 1] * v[:, 0]], axis=1)
        l2 = (N[:, 0] * N[:, 0] + N[:, 1] * N[:, 1]) + N[:, 2] * N[:, 2]
        differ = (rows[:, 0] != rows[:, 1]) & (rows[:, 0] != rows[:, 2]) & (rows[:, 1] != rows[:, 2])
        valid = differ & np.isfinite(l2) & (l2 > 0)
        n64 = N / np.sqrt(l2)[:, None]
        n32 = n64.astype(np.float32)
    n32[~valid] = np.nan
    return Hypotheses(rows, valid, xyz[rows[:, 0]].copy(), n32, n64)


def inliers_f32(xyz, anchor, normal, thr):
    """[B, n] bool: the f32 test of B hypotheses against every point."""
    with np.errstate(all="ignore"):
        ex = xyz[None, :, 0] - anchor[:, 0, None]
        ey = xyz[None, :, 1] - anchor[:, 1, None]
        ez = xyz[None, :, 2] - anchor[:, 2, None]
        s = (normal[:, 0, None] * ex + normal[:, 1, None] * ey) + normal[:, 2, None] * ez
        assert s.dtype == np.float32
        return np.abs(s) <= np.float32(thr)


def counts(xyz, hyp, thr, block_pairs=4_000_000):
    xyz = np.ascontiguousarray(xyz, np.float32)
    H, n = hyp.rows.shape[0], xyz.shape[0]
    out = np.zeros(H, np.int64)
    step = max(1, block_pairs // n)
    for lo in range(0, H, step):
        hi = min(H, lo + step)
        out[lo:hi] = inliers_f32(xyz, hyp.anchor[lo:hi], hyp.normal[lo:hi], thr).sum(axis=1)
    out[~hyp.valid] = 0
    return out.astype(np.uint32)


def orient(n):
    k = int(np.argmax(np.abs(n)))            # the first of equal magnitudes
    return -n if n[k] < 0 else n


Result = collections.namedtuple("Result", ["counts", "best_h", "c_best", "rows", "n_valid", "plane", "centroid", "eigenvalues", "mask",
                                           "I0", "anchor"])


def final_mask(xyz, normal, centroid, thr):
    p = np.ascontiguousarray(xyz, np.float32).astype(np.float64)
    with np.errstate(all="ignore"):
        t = (normal[0] * (p[:, 0] - centroid[0]) + normal[1] * (p[:, 1] - centroid[1])) + normal[2] * (p[:, 2] - centroid[2])
        return np.abs(t) <= thr


def segment_plane(xyz, thr, H, seed):
    """The whole of r3d_segment_plane (the eigenvectors by numpy.linalg.eigh: equal to the library's Jacobi to rounding, which the
    tests bound; everything in front of the refit and the mask from a GIVEN plane are exact restatements)."""
    xyz = np.ascontiguousarray(xyz, np.float32)
    hyp = hypotheses(xyz, H, seed)
    c = counts(xyz, hyp, thr)
    best = int(np.argmax(c))                 # the first of equal counts
    rows, nan3 = hyp.rows[best], np.full(3, np.nan)
    if c[best] < 3:
        return Result(c, best, int(c[best]), rows, int(hyp.valid.sum()), np.full(4, np.nan), nan3, nan3, np.zeros(xyz.shape[0], bool),
                      np.zeros(xyz.shape[0], bool), hyp.anchor[best])
    I0 = inliers_f32(xyz, hyp.anchor[best:best + 1], hyp.normal[best:best + 1], thr)[0]
    a = hyp.anchor[best].astype(np.float64)
    e = xyz[I0].astype(np.float64) - a
    m = float(e.shape[0])
    S1 = e.sum(axis=0)
    S2 = e.T @ e
    centroid = a + S1 / m
    C = (S2 - np.outer(S1, S1) / m) / m
    l, V = np.linalg.eigh(C)
    normal = V[:, 0]
    if not l[1] > 0:
        normal, centroid = hyp.normal64[best], a
    normal = orient(normal)
    d = -((normal[0] * centroid[0] + normal[1] * centroid[1]) + normal[2] * centroid[2])
    return Result(c, best, int(c[best]), rows, int(hyp.valid.sum()), np.array([normal[0], normal[1], normal[2], d]), centroid, l,
                  final_mask(xyz, normal, centroid, thr), I0, hyp.anchor[best])


def refit_longdouble(xyz, I0, anchor):
    """The reference refit of the GPU test's case 3: covariance in np.longdouble about the centroid, then eigh.  Returns the
    centroid (longdouble), eigenvalues, eigenvectors (columns, ascending) and tr C."""
    p = xyz[I0].astype(np.longdouble)
    c = p.mean(axis=0)
    q = p - c
    C = (q.T @ q) / np.longdouble(p.shape[0])
    l, V = np.linalg.eigh(C.astype(np.float64))
    return c, l, V, float(np.trace(C))


def refit_bounds(xyz, I0, anchor):
    """(centroid in longdouble, normal, sin bound, centroid bound, gap ok) of the issue's case 3: sin(angle) <= m 2^-50 (tr C + |c - a|^2) /
    (l1 - l0) and |centroid error| <= m 2^-50 (|c - a| + sqrt(tr C)); gap ok = l1 - l0 >= 1e-6 l2."""
    c, l, V, tr = refit_longdouble(xyz, I0, anchor)
    m = float(I0.sum())
    off = float(np.sqrt(((c - anchor.astype(np.longdouble)) ** 2).sum()))
    gap = l[1] - l[0]
    sin_bound = m * 2.0 ** -50 * (tr + off * off) / gap if gap > 0 else np.inf
    return c, V[:, 0], sin_bound, m * 2.0 ** -50 * (off + np.sqrt(tr)), gap >= 1e-6 * l[2]


def segment_planes(xyz, thr, H, max_planes, min_inliers, seed):
    xyz = np.ascontiguousarray(xyz, np.float32)
    labels = np.full(xyz.shape[0], -1, np.int32)
    rows_cur, planes, cnts = np.arange(xyz.shape[0]), [], []
    for r in range(max_planes):
        if rows_cur.size < 3:
            break
        res = segment_plane(xyz[rows_cur], thr, H, (seed + r) & M64)
        k = int(res.mask.sum())
        if k < min_inliers or k == 0:
            break
        labels[rows_cur[res.mask]] = len(planes)
        planes.append(res.plane)
        cnts.append(k)
        rows_cur = rows_cur[~res.mask]
    return np.array(planes).reshape(-1, 4), labels, np.array(cnts, np.int64)


# ---- scenes ----------------------------------------------------------------------------------------------------------------------

def cube(n, seed):
    return np.random.default_rng(seed).random((n, 3)).astype(np.float32)


def lattice_plane(m=40, extra=300, seed=5):
    """m x m points at z = 0.5 on a 1/8 lattice (every coordinate and every difference exact in f32) plus `extra` points at
    z >= 1, shuffled."""
    g = np.stack(np.meshgrid(np.arange(m), np.arange(m), indexing="ij"), -1).reshape(-1, 2).astype(np.float32) * np.float32(0.125)
    plane = np.concatenate([g, np.full((g.shape[0], 1), 0.5, np.float32)], axis=1)
    rng = np.random.default_rng(seed)
    far = rng.random((extra, 3)).astype(np.float32) * np.float32(4.0) + np.float32([0, 0, 1.0])
    xyz = np.concatenate([plane, far])
    return xyz[rng.permutation(xyz.shape[0])]


def nonfinite(n=3000, seed=12):
    rng = np.random.default_rng(seed)
    xyz = cube(n, seed)
    xyz[:, 2] *= np.float32(0.02)                      # a slab: a real plane among the bad rows
    xyz[rng.choice(n, n // 10, replace=False), rng.integers(0, 3, n // 10)] = np.nan
    xyz[rng.choice(n, n // 20, replace=False), rng.integers(0, 3, n // 20)] = np.inf
    xyz[5, 0] = -np.inf
    return xyz


def hot(copies=2000, background=500, seed=4):
    rng = np.random.default_rng(seed)
    xyz = np.concatenate([np.tile(np.float32([[0.25, 0.5, 0.75]]), (copies, 1)), rng.random((background, 3)).astype(np.float32)])
    return xyz[rng.permutation(xyz.shape[0])]


def noisy_plane(n=20_000, sigma=0.002, outliers=0.3, seed=3):
    """(xyz, true unit normal): a tilted 2 x 2 plane patch with Gaussian noise along the normal plus uniform outliers in the
    patch's box."""
    rng = np.random.default_rng(seed)
    normal = np.array([0.3, -0.2, 0.9])
    normal /= np.linalg.norm(normal)
    u = np.cross(normal, [1.0, 0, 0])
    u /= np.linalg.norm(u)
    v = np.cross(normal, u)
    n_in = int(round(n * (1 - outliers)))
    st = rng.random((n_in, 2)) * 2 - 1
    pts = np.array([0.5, -0.3, 1.2]) + st[:, :1] * u + st[:, 1:] * v + rng.normal(0, sigma, (n_in, 1)) * normal
    lo, hi = pts.min(axis=0) - 0.2, pts.max(axis=0) + 0.2
    out = lo + rng.random((n - n_in, 3)) * (hi - lo)
    xyz = np.concatenate([pts, out]).astype(np.float32)
    return xyz[rng.permutation(n)], normal


def room_faces(planes, lo, hi):
    """For each plane (unit normal, d) the face (axis, side) of the box [lo, hi] it is, its 1 - |n_axis| and its offset error."""
    out = []
    for a, b, c, d in planes:
        nrm = np.array([a, b, c])
        axis = int(np.argmax(np.abs(nrm)))
        pos = -d / nrm[axis]                           # the plane's coordinate along its axis
        side = 0 if abs(pos - lo[axis]) < abs(pos - hi[axis]) else 1
        out.append((axis, side, 1.0 - abs(nrm[axis]), abs(pos - (lo, hi)[side][axis])))
    return out
