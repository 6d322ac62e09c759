"""NumPy restatement of include/r3d.h, "Reconstruction evaluation": brute-force point-to-mesh distance with the header's exact
fp64 expression (vectorised over points x triangles; NumPy neither fuses nor reorders), the distance statistics in the
reduction's fixed order, the f32 root and the colour ramp.  The GPU tests compare with this bit for bit."""
import numpy as np

NO_TRIANGLE = 0xFFFFFFFF
MAX_THRESHOLDS, MAX_BINS = 8, 4096


def _dot(a, b):
    return (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2]


def valid_triangles(vertices, triangles):
    """[M] bool: indices in [0, N) and nine finite coordinates"""
    v = np.asarray(vertices, np.float32).reshape(-1, 3)
    t = np.asarray(triangles, np.int64).reshape(-1, 3)
    ok = ((t >= 0) & (t < len(v))).all(axis=1)
    safe = np.where(ok[:, None], t, 0)
    if len(v):
        ok &= np.isfinite(v[safe].astype(np.float64)).all(axis=(1, 2))
    return ok


def closest_points(p, a, b, c):
    """The header's region form.  p: 3 arrays broadcastable against a, b, c (3 arrays each), float64.  Returns (d2, q0, q1, q2)."""
    ab = [b[k] - a[k] for k in range(3)]
    ac = [c[k] - a[k] for k in range(3)]
    bc = [c[k] - b[k] for k in range(3)]
    ap = [p[k] - a[k] for k in range(3)]
    bp = [p[k] - b[k] for k in range(3)]
    cp = [p[k] - c[k] for k in range(3)]
    d1, d2 = _dot(ab, ap), _dot(ac, ap)
    d3, d4 = _dot(ab, bp), _dot(ac, bp)
    d5, d6 = _dot(ab, cp), _dot(ac, cp)
    vc = d1 * d4 - d3 * d2
    vb = d5 * d2 - d1 * d6
    va = d3 * d6 - d5 * d4
    e43, e56 = d4 - d3, d5 - d6
    den_ab, den_ac, den_bc = d1 - d3, d2 - d6, e43 + e56
    in_a = (d1 <= 0) & (d2 <= 0)
    in_b = ~in_a & (d3 >= 0) & (d4 <= d3)
    in_ab = ~in_a & ~in_b & (vc <= 0) & (d1 >= 0) & (d3 <= 0) & (den_ab > 0)
    done3 = in_a | in_b | in_ab
    in_c = ~done3 & (d6 >= 0) & (d5 <= d6)
    in_ac = ~done3 & ~in_c & (vb <= 0) & (d2 >= 0) & (d6 <= 0) & (den_ac > 0)
    done5 = done3 | in_c | in_ac
    in_bc = ~done5 & (va <= 0) & (e43 >= 0) & (e56 >= 0) & (den_bc > 0)
    face = ~done5 & ~in_bc
    vertex = in_a | in_b | in_c
    one = np.ones_like(d1)
    num = np.where(in_ab, d1, np.where(in_ac, d2, np.where(in_bc, e43, one)))
    den = np.where(in_ab, den_ab, np.where(in_ac, den_ac, np.where(in_bc, den_bc, (va + vb) + vc)))
    with np.errstate(all="ignore"):
        r = np.where(den > 0, num / np.where(den > 0, den, one), 0.0)
        v = vb * r
        w = vc * r
    v = np.where(v > 0, v, 0.0)
    v = np.where(v < 1, v, 1.0)
    wmax = 1.0 - v
    w = np.where(w > 0, w, 0.0)
    w = np.where(w < wmax, w, wmax)
    t1 = np.where(face, v, np.where(in_ab | in_bc, r, 0.0))
    t2 = np.where(face, w, np.where(in_ac, r, 0.0))
    from_b = in_b | in_bc
    q = []
    for k in range(3):
        s = np.where(in_c, c[k], np.where(from_b, b[k], a[k]))
        e = np.where(in_bc, bc[k], ab[k])
        q.append(np.where(vertex, s, (s + e * t1) + ac[k] * t2))
    dq = [p[k] - q[k] for k in range(3)]
    return (dq[0] * dq[0] + dq[1] * dq[1]) + dq[2] * dq[2], q[0], q[1], q[2]


def mesh_distance(points, vertices, triangles, signed=False, chunk=128, with_d2=False):
    """(distance [P] float32, triangle [P] uint32, closest [P,3] float32[, d2 [P] float64, all d2 [P,M] or None]): brute force
    over the valid triangles, the lowest index winning exact ties."""
    pts = np.asarray(points, np.float32).reshape(-1, 3)
    v = np.asarray(vertices, np.float32).reshape(-1, 3)
    t = np.asarray(triangles, np.int64).reshape(-1, 3)
    ok = valid_triangles(v, t)
    keep = np.flatnonzero(ok)
    n = len(pts)
    dist = np.full(n, np.inf, np.float32)
    win = np.full(n, NO_TRIANGLE, np.uint32)
    closest = np.full((n, 3), np.nan, np.float32)
    best_d2 = np.full(n, np.inf)
    p_ok = np.isfinite(pts.astype(np.float64)).all(axis=1)
    if len(keep) == 0 or not p_ok.any():
        return (dist, win, closest, best_d2) if with_d2 else (dist, win, closest)
    tv = v[t[keep]].astype(np.float64)                           # [T, 3 corners, 3]
    a = [tv[None, :, 0, k] for k in range(3)]
    b = [tv[None, :, 1, k] for k in range(3)]
    c = [tv[None, :, 2, k] for k in range(3)]
    rows = np.flatnonzero(p_ok)
    for lo in range(0, len(rows), chunk):
        r = rows[lo:lo + chunk]
        p64 = pts[r].astype(np.float64)
        p = [p64[:, k:k + 1] for k in range(3)]
        d2, q0, q1, q2 = closest_points(p, a, b, c)
        j = np.argmin(d2, axis=1)                                # the first minimum: the lowest index (keep ascends)
        i = np.arange(len(r))
        m = d2[i, j]
        q = np.stack([q0[i, j], q1[i, j], q2[i, j]], axis=1)
        with np.errstate(over="ignore"):
            d = np.sqrt(m).astype(np.float32)
            if signed:
                ta = tv[j]
                ab, ac = ta[:, 1] - ta[:, 0], ta[:, 2] - ta[:, 0]
                nx = ab[:, 1] * ac[:, 2] - ab[:, 2] * ac[:, 1]
                ny = ab[:, 2] * ac[:, 0] - ab[:, 0] * ac[:, 2]
                nz = ab[:, 0] * ac[:, 1] - ab[:, 1] * ac[:, 0]
                dq = p64 - q
                s = (nx * dq[:, 0] + ny * dq[:, 1]) + nz * dq[:, 2]
                d = np.where(s < 0, -d, d).astype(np.float32)
            closest[r] = q.astype(np.float32)
        dist[r], win[r], best_d2[r] = d, keep[j].astype(np.uint32), m
    return (dist, win, closest, best_d2) if with_d2 else (dist, win, closest)


def all_d2(points, vertices, triangles):
    """[P, M] float64 d2 of every point to every triangle (NaN for an invalid triangle): what the host tests look ties up in"""
    pts = np.asarray(points, np.float32).reshape(-1, 3).astype(np.float64)
    v = np.asarray(vertices, np.float32).reshape(-1, 3)
    t = np.asarray(triangles, np.int64).reshape(-1, 3)
    ok = valid_triangles(v, t)
    tv = v[np.where(ok[:, None], t, 0)].astype(np.float64)
    out = closest_points([pts[:, k:k + 1] for k in range(3)], [tv[None, :, 0, k] for k in range(3)],
                         [tv[None, :, 1, k] for k in range(3)], [tv[None, :, 2, k] for k in range(3)])[0]
    return np.where(ok[None, :], out, np.nan)


# ---- statistics ------------------------------------------------------------------------------------------------------------
def _wave_sum(v):
    """the shuffle tree over the last axis of 64"""
    for off in (32, 16, 8, 4, 2, 1):
        v = v[..., :off] + v[..., off:2 * off]
    return v[..., 0]


def _block_sum(v):
    """[..., 256] -> [...]: the tree per 64 lanes, then the four waves added in order to 0.0"""
    w = _wave_sum(v.reshape(v.shape[:-1] + (4, 64)))
    out = np.zeros(w.shape[:-1])
    for k in range(4):
        out = out + w[..., k]
    return out


def fixed_order_sum(x):
    """sum of the float64 array x in the order of r3d_distance_stats (0 for an empty array)"""
    x = np.asarray(x, np.float64).reshape(-1)
    if x.size == 0:
        return 0.0
    rows = -(-x.size // 256)
    part = _block_sum(np.concatenate([x, np.zeros(rows * 256 - x.size)]).reshape(rows, 256))        # one partial per row
    folds = -(-rows // 256)
    part = np.concatenate([part, np.zeros(folds * 256 - rows)]).reshape(folds, 256)
    acc = np.zeros(256)
    for j in range(folds):                                       # thread t: rows t, t + 256, ... in order
        acc = acc + part[j]
    return float(_block_sum(acc))


def distance_stats(values, thresholds=(), bin_width=None, n_bins=0, squared=False):
    """(stats [6] float64 = n_finite, n_nonfinite, sum, sum of squares, min, max; count_le [T] int64; hist [n_bins] uint64)"""
    v = np.asarray(values, np.float32).reshape(-1)
    with np.errstate(invalid="ignore"):
        x = v.astype(np.float64)
        if squared:
            x = np.sqrt(x)
    fin = np.isfinite(x)
    z = np.where(fin, x, 0.0)                                     # a lane without a finite element adds 0.0
    stats = np.array([fixed_order_sum(fin.astype(np.float64)), fixed_order_sum((~fin).astype(np.float64)), fixed_order_sum(z),
                      fixed_order_sum(z * z), np.inf, -np.inf])
    xf = x[fin]
    if xf.size:
        stats[4], stats[5] = xf.min() + 0.0, xf.max() + 0.0
    counts = np.array([np.count_nonzero(xf <= t) for t in thresholds], np.int64)
    hist = np.zeros(n_bins, np.uint64)
    if n_bins:
        q = np.floor(xf / float(bin_width))
        top = n_bins - 1
        b = np.where(q >= top, top, np.where(q > 0, q, 0)).astype(np.int64)
        hist = np.bincount(b, minlength=n_bins).astype(np.uint64)
    return stats, counts, hist


def sqrt_f32(values):
    with np.errstate(invalid="ignore"):
        return np.sqrt(np.asarray(values, np.float32).astype(np.float64)).astype(np.float32)


def distance_colors(d, d_max):
    """[N] uint32 words r | g << 8 | b << 16 of the header's integer ramp; grey for a non-finite distance"""
    x = np.abs(np.asarray(d, np.float32).astype(np.float64))
    fin = np.isfinite(x)
    t = np.where(fin, x, 0.0) / float(d_max)
    t = np.where(t < 1, t, 1.0)
    q = np.floor(t * 765.0).astype(np.int64)
    r = np.where(q <= 255, 0, np.where(q <= 510, q - 255, 255))
    g = np.where(q <= 255, q, np.where(q <= 510, 255, 255 - (q - 510)))
    b = np.where(q <= 255, 255 - q, 0)
    r, g, b = (np.where(fin, c, 128).astype(np.uint32) for c in (r, g, b))
    return r | (g << 8) | (b << 16)


# ---- the numbers evaluate_reconstruction reports, from the device sums ---------------------------------------------------------
def side_numbers(stats, count_le):
    """mean, rms, max and the fraction within the threshold of one direction, from r3d_distance_stats' outputs"""
    n = stats[0]
    if n == 0:
        return {"n": 0, "mean": float("nan"), "rms": float("nan"), "max": float("nan"), "within": float("nan")}
    return {"n": int(n), "mean": stats[2] / n, "rms": float(np.sqrt(stats[3] / n)), "max": float(stats[5]), "within": count_le / n}


def f_score(precision, recall):
    return 2.0 * precision * recall / (precision + recall) if precision + recall > 0 else 0.0
