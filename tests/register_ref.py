"""NumPy restatement of include/r3d.h's global registration: r3d_fpfh_knn (the neighbour lists are an input), r3d_feature_match
and r3d_register_ransac.  f32 arrays with one operation per NumPy call (NumPy never fuses a multiply with an add), the sampler
in Python ints, the pose in fp64, the refit's sums in the device's two-stage order, the Umeyama solve by numpy.linalg.svd.
Test infrastructure; the scene builders the host and the GPU tests share live here too."""
import collections

import numpy as np

NONE = np.uint32(0xffffffff)
DIM, BINS = 33, 11
M64 = (1 << 64) - 1
GOLDEN = 0x9E3779B97F4A7C15
F = np.float32

# the f32 roundings of cos / sin(-pi + 2 pi m / 11), m = 1..10, as the header prints them
THETA_COS = np.array([-0.841253519, -0.415415019, 0.142314836, 0.654860735, 0.959492981, 0.959492981, 0.654860735, 0.142314836,
                      -0.415415019, -0.841253519], dtype=np.float32)
THETA_SIN = np.array([-0.540640831, -0.909631968, -0.989821434, -0.755749583, -0.281732559, 0.281732559, 0.755749583, 0.989821434,
                      0.909631968, 0.540640831], dtype=np.float32)


# ---- stage 1: FPFH ---------------------------------------------------------------------------------------------------------

def dot(a, b):
    return (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2]


def cross(a, b):
    return (a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0])


def theta_bin(x, y):
    x, y = np.asarray(x, F), np.asarray(y, F)
    b = np.zeros(x.shape, np.int64)
    for m in range(10):
        cr = THETA_COS[m] * y - THETA_SIN[m] * x
        assert cr.dtype == np.float32
        b += ((y >= 0) | (cr >= 0)) if m < 5 else ((y >= 0) & (cr >= 0))
    return b


def bin11(f):
    t = (np.asarray(f, F) + F(1.0)) * F(5.5)
    with np.errstate(invalid="ignore"):
        return np.where(t < 1, 0, np.where(t >= 10, 10, np.where(np.isfinite(t), t, 0).astype(np.int64)))


def members(idx, d2, radius):
    """[n,k] bool: the list entries that belong to N_i (tails dropped, cut at the radius)."""
    real = idx != NONE
    stop = ~real
    if radius is not None and radius > 0:
        stop = stop | (d2 > F(float(radius) * float(radius)))
    return np.cumsum(stop, axis=1) == 0


def has_normal(nrm):
    return np.isfinite(nrm).all(axis=1) & (nrm != 0).any(axis=1)


def spfh(xyz, normals, idx, d2, radius=None):
    """(spfh [n,33] uint8, count [n] uint32) of the pair features of every list."""
    xyz, nrm = np.ascontiguousarray(xyz, F), np.ascontiguousarray(normals, F)
    n, k = idx.shape
    mem = members(idx, d2, radius)
    j = np.where(mem, idx, 0).astype(np.int64)
    ok = mem & has_normal(nrm)[:, None] & has_normal(nrm)[j]
    hist = np.zeros((n, DIM), np.int64)
    with np.errstate(all="ignore"):
        pi = [xyz[:, a][:, None] for a in range(3)]
        ni = [np.broadcast_to(nrm[:, a][:, None], (n, k)) for a in range(3)]
        nj = [nrm[j, a] for a in range(3)]
        d = [xyz[j, a] - pi[a] for a in range(3)]
        Ln = np.sqrt((d[0] * d[0] + d[1] * d[1]) + d[2] * d[2])
        ok &= (Ln > 0) & np.isfinite(Ln)
        ai, aj = dot(ni, d), dot(nj, d)
        swap = np.abs(aj) > np.abs(ai)
        u = [np.where(swap, nj[a], ni[a]) for a in range(3)]
        nt = [np.where(swap, ni[a], nj[a]) for a in range(3)]
        d = [np.where(swap, -d[a], d[a]) for a in range(3)]
        dh = [d[a] / Ln for a in range(3)]
        v = cross(dh, u)
        lv = np.sqrt((v[0] * v[0] + v[1] * v[1]) + v[2] * v[2])
        ok &= (lv > 0) & np.isfinite(lv)
        vh = [v[a] / lv for a in range(3)]
        w = cross(u, vh)
        alpha, phi, x, y = dot(vh, nt), dot(u, dh), dot(u, nt), dot(w, nt)
        for q in (Ln, alpha, phi, x, y):
            assert q.dtype == np.float32
        ok &= np.isfinite(alpha) & np.isfinite(phi) & np.isfinite(x) & np.isfinite(y) & ~((x == 0) & (y == 0))
        bins = (theta_bin(x, y), BINS + bin11(alpha), 2 * BINS + bin11(phi))
    rows = np.broadcast_to(np.arange(n)[:, None], (n, k))
    for b in bins:
        np.add.at(hist, (rows[ok], b[ok]), 1)
    return hist.astype(np.uint8), ok.sum(axis=1).astype(np.uint32)


def fpfh_from_spfh(hist, count, idx, d2, radius=None):
    n, k = idx.shape
    mem = members(idx, d2, radius)
    with np.errstate(all="ignore"):
        scale = np.where(count > 0, F(100.0) / count.astype(F), F(0)).astype(F)
        P = hist.astype(F) * scale[:, None]
        A = np.zeros((n, DIM), F)
        for s in range(k):
            use = mem[:, s] & np.isfinite(d2[:, s]) & (d2[:, s] > 0)
            j = np.where(use, idx[:, s], 0).astype(np.int64)
            term = P[j] / np.where(use, d2[:, s], F(1))[:, None]
            A = np.where(use[:, None], A + term, A)
        out = np.zeros((n, DIM), F)
        for s3 in range(3):
            T = np.zeros(n, F)
            for b in range(BINS):
                T = T + A[:, s3 * BINS + b]
            some = T > 0
            f = np.where(some, F(100.0) / np.where(some, T, F(1)), F(0)).astype(F)
            sl = slice(s3 * BINS, (s3 + 1) * BINS)
            out[:, sl] = P[:, sl] + np.where(some[:, None], A[:, sl] * f[:, None], F(0))
        assert A.dtype == np.float32 and out.dtype == np.float32
    return out


def fpfh(xyz, normals, idx, d2, radius=None):
    """(fpfh [n,33] f32, spfh [n,33] u8, count [n] u32) from the lists idx / d2 [n,k] as r3d_nn_index_knn_self returns them."""
    hist, count = spfh(xyz, normals, idx, d2, radius)
    return fpfh_from_spfh(hist, count, idx, d2, radius), hist, count


# ---- stage 2: matching -------------------------------------------------------------------------------------------------------

def nearest_rows(fa, fb, block_pairs=262_144):
    """(idx [na] uint32, dist [na] f32): the smallest (dist, j) among finite dist; none: (NONE, +inf).  Blocks that stay in the
    cache, every operation in place: one f32 rounding per subtraction, product and sum, b ascending."""
    fa, fb = np.ascontiguousarray(fa, F), np.ascontiguousarray(fb, F)
    na, nb = fa.shape[0], fb.shape[0]
    idx, dist = np.full(na, NONE, np.uint32), np.full(na, np.inf, F)
    step = max(1, block_pairs // nb)
    fbt = np.ascontiguousarray(fb.T)
    with np.errstate(all="ignore"):
        for lo in range(0, na, step):
            a = fa[lo:lo + step]
            d, e = np.zeros((a.shape[0], nb), F), np.empty((a.shape[0], nb), F)
            for b in range(DIM):
                np.subtract(a[:, b][:, None], fbt[b][None, :], out=e)
                np.multiply(e, e, out=e)
                np.add(d, e, out=d)
            d[~np.isfinite(d)] = np.inf
            j = np.argmin(d, axis=1)                      # the first of equal distances
            best = d[np.arange(a.shape[0]), j]
            hit = np.isfinite(best)
            idx[lo:lo + step] = np.where(hit, j, NONE).astype(np.uint32)
            dist[lo:lo + step] = best
    return idx, dist


def match(fa, fb, mutual=True):
    """(corr [m,2] uint32, idx_a, dist_a)."""
    idx_a, dist_a = nearest_rows(fa, fb)
    keep = idx_a != NONE
    if mutual:
        idx_b, _ = nearest_rows(fb, fa)
        back = idx_b[np.where(keep, idx_a, 0).astype(np.int64)]
        keep &= back == np.arange(idx_a.shape[0], dtype=np.uint32)
    rows = np.flatnonzero(keep).astype(np.uint32)
    return np.stack([rows, idx_a[rows]], axis=1).reshape(-1, 2), idx_a, dist_a


# ---- stage 3: RANSAC ---------------------------------------------------------------------------------------------------------

def splitmix64(z):
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & M64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & M64
    return z ^ (z >> 31)


def rows_of(seed, h, n):
    return tuple((splitmix64((seed + (3 * h + j + 1) * GOLDEN) & M64) * n) >> 64 for j in range(3))


def all_rows(seed, H, n):
    return np.array([rows_of(seed, h, n) for h in range(H)], dtype=np.int64).reshape(H, 3)


def gather_pairs(src, tgt, corr):
    """(p [m,3] f32, q [m,3] f32): rows outside their cloud become NaN points."""
    src, tgt, corr = np.ascontiguousarray(src, F), np.ascontiguousarray(tgt, F), np.asarray(corr, np.int64)
    p, q = np.full((corr.shape[0], 3), np.nan, F), np.full((corr.shape[0], 3), np.nan, F)
    okp, okq = corr[:, 0] < src.shape[0], corr[:, 1] < tgt.shape[0]
    p[okp], q[okq] = src[corr[okp, 0]], tgt[corr[okq, 1]]
    return p, q


def sq3(v):
    return (v[..., 0] * v[..., 0] + v[..., 1] * v[..., 1]) + v[..., 2] * v[..., 2]


def cross_rows(a, b):
    return np.stack([a[..., 1] * b[..., 2] - a[..., 2] * b[..., 1], a[..., 2] * b[..., 0] - a[..., 0] * b[..., 2],
                     a[..., 0] * b[..., 1] - a[..., 1] * b[..., 0]], axis=-1)


def frame(a, b, c):
    """fp64 rows [...,3] -> (e1, e2, e3, lengths [...,3], ok)."""
    u, v, w = b - a, c - a, c - b
    N = cross_rows(u, v)
    lu2, ln2 = sq3(u), sq3(N)
    ok = (lu2 > 0) & np.isfinite(lu2) & (ln2 > 0) & np.isfinite(ln2)
    e1, e3 = u / np.sqrt(lu2)[..., None], N / np.sqrt(ln2)[..., None]
    e2 = cross_rows(e3, e1)
    return e1, e2, e3, np.stack([np.sqrt(lu2), np.sqrt(sq3(v)), np.sqrt(sq3(w))], axis=-1), ok


def pose_from_pairs(p3, q3, thr):
    """p3, q3 [...,3,3] (pair, axis) f32 or f64 -> (R [...,3,3], t [...,3], geometric validity) in fp64 as the header writes it."""
    p3, q3 = np.asarray(p3, np.float64), np.asarray(q3, np.float64)
    with np.errstate(all="ignore"):
        e1, e2, e3, ls, oks = frame(p3[..., 0, :], p3[..., 1, :], p3[..., 2, :])
        f1, f2, f3, lt, okt = frame(q3[..., 0, :], q3[..., 1, :], q3[..., 2, :])
        ok = oks & okt & (np.abs(ls - lt) <= 2.0 * thr).all(axis=-1)
        R = (f1[..., :, None] * e1[..., None, :] + f2[..., :, None] * e2[..., None, :]) + f3[..., :, None] * e3[..., None, :]
        a = p3[..., 0, :]
        t = q3[..., 0, :] - ((R[..., 0] * a[..., 0, None] + R[..., 1] * a[..., 1, None]) + R[..., 2] * a[..., 2, None])
    return R, t, ok


def dist2_f32(p, q, R32, t32):
    """[B, m] f32: the squared distance of the header's test for B poses."""
    with np.errstate(all="ignore"):
        e = []
        for r in range(3):
            x = ((R32[:, r, 0, None] * p[None, :, 0] + R32[:, r, 1, None] * p[None, :, 1]) + R32[:, r, 2, None] * p[None, :, 2]) \
                + t32[:, r, None]
            e.append(x - q[None, :, r])
        s2 = (e[0] * e[0] + e[1] * e[1]) + e[2] * e[2]
    assert s2.dtype == np.float32
    return s2


def device_sum(terms, mask):
    """The two-stage fixed-order fp64 reduction of the header.  terms: list over accumulator slots of lists of [m] addends, added
    in list order per pair; mask [m]: the pairs that take part.  Returns one double per slot."""
    m = mask.shape[0]
    G = min((m + 255) // 256, 1024)
    lanes = G * 256
    K = len(terms)
    acc = np.zeros((lanes, K))
    with np.errstate(all="ignore"):
        for start in range(0, m, lanes):
            sl = slice(start, min(m, start + lanes))
            w = sl.stop - sl.start
            mk = mask[sl]
            for k in range(K):
                for addend in terms[k]:
                    acc[:w, k] = np.where(mk, acc[:w, k] + addend[sl], acc[:w, k])

        def block(v):                      # [B, 256, K] -> [B, K]
            v = v.reshape(v.shape[0], 4, 64, K)
            width = 64
            while width > 1:
                width //= 2
                v = v[:, :, :width] + v[:, :, width:2 * width]
            v = v[:, :, 0]
            out = np.zeros((v.shape[0], K))
            for wv in range(4):
                out = out + v[:, wv]
            return out

        rows = block(acc.reshape(G, 256, K))
        fold = np.zeros((256, K))
        for b in range(0, G, 256):
            part = rows[b:b + 256]
            fold[:part.shape[0]] = fold[:part.shape[0]] + part
        return block(fold.reshape(1, 256, K))[0]


def umeyama_rigid(s):
    """T [4,4] from the 18 sums (no scale), or None when the fit is undefined."""
    n = s[0]
    if not n >= 3:
        return None
    mp, mq = s[1:4] / n, s[4:7] / n
    if not s[16] / n - mp @ mp > 0:
        return None
    M = (s[7:16].reshape(3, 3) / n - np.outer(mp, mq)).T            # Sigma_qp
    if not np.isfinite(M).all():
        return None
    U, D, Vt = np.linalg.svd(M)
    S = np.diag([1.0, 1.0, -1.0 if np.linalg.det(U) * np.linalg.det(Vt) < 0 else 1.0])
    R = U @ S @ Vt
    T = np.eye(4)
    T[:3, :3], T[:3, 3] = R, mq - R @ mp
    return T if np.isfinite(T).all() else None


Ransac = collections.namedtuple("Ransac", ["counts", "best_h", "c_best", "rows", "n_valid", "T", "mask", "n_inliers", "rms", "degenerate"])


def ransac(src, tgt, corr, thr, H, seed, block_pairs=4_000_000):
    corr = np.asarray(corr, np.int64)
    m = corr.shape[0]
    p, q = gather_pairs(src, tgt, corr)
    rows = all_rows(seed, H, m)
    cs, ct = corr[rows, 0], corr[rows, 1]
    differ = np.ones(H, bool)
    for c in (cs, ct):
        differ &= (c[:, 0] != c[:, 1]) & (c[:, 0] != c[:, 2]) & (c[:, 1] != c[:, 2])
    R, t, ok = pose_from_pairs(p[rows], q[rows], thr)
    valid = ok & differ
    with np.errstate(all="ignore"):
        R32, t32 = R.astype(F), t.astype(F)
    R32[~valid], t32[~valid] = np.nan, np.nan
    thr2 = F(thr * thr)
    counts = np.zeros(H, np.int64)
    step = max(1, block_pairs // m)
    for lo in range(0, H, step):
        with np.errstate(invalid="ignore"):
            counts[lo:lo + step] = (dist2_f32(p, q, R32[lo:lo + step], t32[lo:lo + step]) <= thr2).sum(axis=1)
    counts[~valid] = 0
    counts = counts.astype(np.uint32)
    best = int(np.argmax(counts))
    c_best, n_valid = int(counts[best]), int(valid.sum())
    if c_best < 3:
        return Ransac(counts, best, c_best, rows[best], n_valid, np.full((4, 4), np.nan), np.zeros(m, bool), 0, float("nan"), False)
    with np.errstate(invalid="ignore"):
        I0 = dist2_f32(p, q, R32[best:best + 1], t32[best:best + 1])[0] <= thr2
    a, b = p[rows[best, 0]].astype(np.float64), q[rows[best, 0]].astype(np.float64)
    pc, qc = p.astype(np.float64) - a, q.astype(np.float64) - b
    terms = [[] for _ in range(18)]
    terms[0].append(np.ones(m))
    for ax in range(3):
        terms[1 + ax].append(pc[:, ax])
        terms[4 + ax].append(qc[:, ax])
        for bx in range(3):
            terms[7 + 3 * ax + bx].append(pc[:, ax] * qc[:, bx])
        terms[16].append(pc[:, ax] * pc[:, ax])
        terms[17].append(qc[:, ax] * qc[:, ax])
    sums = device_sum(terms, I0)
    Tc = umeyama_rigid(sums)
    Rf, tf = R[best], t[best]
    if Tc is not None:
        Rf = Tc[:3, :3]
        tf = (b + Tc[:3, 3]) - ((Rf[:, 0] * a[0] + Rf[:, 1] * a[1]) + Rf[:, 2] * a[2])
    T = np.eye(4)
    T[:3, :3], T[:3, 3] = Rf, tf
    mask, n_in, rms = final_mask(p, q, T, thr)
    return Ransac(counts, best, c_best, rows[best], n_valid, T, mask, n_in, rms, Tc is None)


def final_mask(p, q, T, thr):
    """(mask [m] bool, count, rms) of the header's final test for a GIVEN fp64 pose."""
    R32, t32 = T[:3, :3].astype(F)[None], T[:3, 3].astype(F)[None]
    s2 = dist2_f32(p, q, R32, t32)[0]
    with np.errstate(invalid="ignore"):
        mask = s2 <= F(thr * thr)
    tot = device_sum([[np.ones(mask.shape[0])], [s2.astype(np.float64)]], mask)
    return mask, int(tot[0]), float(np.sqrt(tot[1] / tot[0])) if tot[0] > 0 else float("nan")


# ---- scenes ------------------------------------------------------------------------------------------------------------------

def cube(n, seed):
    return np.random.default_rng(seed).random((n, 3)).astype(F)


def unit_normals(n, seed):
    v = np.random.default_rng(seed).normal(size=(n, 3))
    return (v / np.linalg.norm(v, axis=1, keepdims=True)).astype(F)


def lattice(side=13):
    g = np.arange(side, dtype=F)
    return np.stack(np.meshgrid(g, g, g, indexing="ij"), axis=-1).reshape(-1, 3).copy()


def axis_normals(n, seed):
    """Unit normals along +-x, +-y, +-z and the diagonals: with lattice points every pair feature sits on a bin boundary."""
    rng = np.random.default_rng(seed)
    table = np.array([[1, 0, 0], [0, 1, 0], [0, 0, 1], [-1, 0, 0], [0, -1, 0], [0, 0, -1]], F)
    return table[rng.integers(0, 6, n)]


def rigid(angle_deg, axis, t):
    axis = np.asarray(axis, np.float64) / np.linalg.norm(axis)
    a = np.deg2rad(angle_deg)
    K = np.array([[0, -axis[2], axis[1]], [axis[2], 0, -axis[0]], [-axis[1], axis[0], 0]])
    T = np.eye(4)
    T[:3, :3] = np.eye(3) + np.sin(a) * K + (1 - np.cos(a)) * (K @ K)
    T[:3, 3] = t
    return T


def correspondences(kind, m, seed):
    """(src [n,3], tgt [n,3], corr [m,2], T_true) for the RANSAC tests."""
    rng = np.random.default_rng(seed)
    n = max(m, 3)
    T = rigid(110.0, (0.3, 1.0, -0.2), (2.0, -3.0, 4.0))
    src = (rng.random((n, 3)) * 4 - 2).astype(F)
    if kind == "collinear":
        src = np.outer(np.arange(n, dtype=F), F([1, 2, -1])).astype(F)
    tgt = (src.astype(np.float64) @ T[:3, :3].T + T[:3, 3]).astype(F)
    corr = np.stack([np.arange(m), np.arange(m)], axis=1).astype(np.uint32)
    if kind == "outliers":
        bad = rng.random(m) < 0.7
        bad[:3] = False
        corr[bad, 1] = rng.integers(0, n, int(bad.sum()))
    if kind == "repeated":
        corr = corr[rng.integers(0, max(3, m // 4), m)]
        corr[:3] = [[0, 0], [1, 1], [2, 2]]
    return src, tgt, corr, T


# ---- the end-to-end scene ------------------------------------------------------------------------------------------------------

ROOM_LO, ROOM_HI = np.array([-4.0, -1.5, -3.0]), np.array([4.0, 1.5, 3.0])     # synthetic.ROOM_LO / ROOM_HI


def cluttered_room(seed, step=0.05):
    """[n,3] float64 points on the floor and the walls of the synthetic room and on ten boxes standing on its floor, sampled on
    a jittered grid of spacing `step`."""
    rng = np.random.default_rng(seed)
    pts = []

    def quad(origin, eu, ev):
        nu, nv = int(np.linalg.norm(eu) / step), int(np.linalg.norm(ev) / step)
        u, v = np.meshgrid((np.arange(nu) + 0.5) / nu, (np.arange(nv) + 0.5) / nv, indexing="ij")
        p = np.asarray(origin, np.float64) + u.reshape(-1, 1) * np.asarray(eu, np.float64) + v.reshape(-1, 1) * np.asarray(ev, np.float64)
        return p + rng.uniform(-0.2, 0.2, p.shape) * step

    ext = ROOM_HI - ROOM_LO
    pts.append(quad(ROOM_LO, [ext[0], 0, 0], [0, 0, ext[2]]))
    pts.append(quad(ROOM_LO, [ext[0], 0, 0], [0, ext[1], 0]))
    pts.append(quad(ROOM_LO, [0, 0, ext[2]], [0, ext[1], 0]))
    pts.append(quad(ROOM_HI, [-ext[0], 0, 0], [0, -ext[1], 0]))
    pts.append(quad(ROOM_HI, [0, 0, -ext[2]], [0, -ext[1], 0]))
    for _ in range(10):
        size = rng.uniform(0.4, 1.3, 3)
        c = np.array([rng.uniform(-3.2, 3.2), ROOM_LO[1] + size[1] / 2, rng.uniform(-2.4, 2.4)])
        Rb = rigid(rng.uniform(0, 90), (0, 1, 0), (0, 0, 0))[:3, :3]
        for ax in range(3):
            a1, a2 = [(1, 2), (2, 0), (0, 1)][ax]
            for sgn in (-1.0, 1.0):
                n, e1, e2 = np.zeros(3), np.zeros(3), np.zeros(3)
                n[ax], e1[a1], e2[a2] = sgn, size[a1], size[a2]
                pts.append(quad(n * size[ax] / 2 - e1 / 2 - e2 / 2, e1, e2) @ Rb.T + c)
    return np.concatenate(pts)


def room_pair(seed=0):
    """Two overlapping parts of the cluttered room: dict(src, tgt [n,3] f32, T (tgt ~ T src: 130 degrees, 6.2 m), src_view,
    tgt_view).  The target is the part x < 1, the source the part x > -1.5 moved by inv(T); the views are one point inside the
    room in either frame."""
    P = cluttered_room(seed)
    T = rigid(130.0, (0.2, 1.0, 0.3), (3.0, -2.0, 5.0))
    Ti = np.linalg.inv(T)
    view = np.array([0.0, 0.3, 0.0])
    return {"tgt": P[P[:, 0] < 1.0].astype(F), "src": (P[P[:, 0] > -1.5] @ Ti[:3, :3].T + Ti[:3, 3]).astype(F), "T": T,
            "tgt_view": view, "src_view": Ti[:3, :3] @ view + Ti[:3, 3]}


def downsample_normals_lists(cloud, voxel, view, k, radius):
    """What the recipe does in front of FPFH, on the host and to rounding only: voxel centroids, k nearest neighbours (scipy),
    the smallest eigenvector of the neighbourhood covariance turned towards `view`.  Returns (xyz f32, normals f32, idx, d2)."""
    from scipy.spatial import cKDTree
    key = np.floor(cloud.astype(np.float64) / voxel).astype(np.int64)
    _, inv = np.unique(key, axis=0, return_inverse=True)
    inv = inv.reshape(-1)
    cnt = np.bincount(inv)
    d = np.stack([np.bincount(inv, cloud[:, a].astype(np.float64)) / cnt for a in range(3)], axis=1).astype(F)
    _, j = cKDTree(d.astype(np.float64)).query(d.astype(np.float64), k + 1)
    idx = j[:, 1:]
    e = d[idx] - d[:, None, :]
    d2 = ((e[..., 0] * e[..., 0] + e[..., 1] * e[..., 1]) + e[..., 2] * e[..., 2]).astype(F)
    mem = d2 <= F(radius * radius)
    nb = e.astype(np.float64) * mem[..., None]
    m = (mem.sum(axis=1) + 1)[:, None, None]
    S1 = nb.sum(axis=1)
    Cv = (np.einsum("nka,nkb->nab", nb, nb) - S1[:, :, None] * S1[:, None, :] / m) / m
    n = np.linalg.eigh(Cv)[1][:, :, 0]
    n[((view - d) * n).sum(axis=1) < 0] *= -1
    return d, n.astype(F), np.where(mem, idx, NONE).astype(np.uint32), d2


def recipe(src, tgt, voxel, src_view, tgt_view, H, seed, k=32, feature_radius=5.0):
    """The whole recipe with the restatements of the three stages: (T, source_down, correspondences, Ransac)."""
    a = downsample_normals_lists(src, voxel, src_view, k, feature_radius * voxel)
    b = downsample_normals_lists(tgt, voxel, tgt_view, k, feature_radius * voxel)
    fa, fb = fpfh(a[0], a[1], a[2], a[3])[0], fpfh(b[0], b[1], b[2], b[3])[0]
    corr = match(fa, fb, mutual=True)[0]
    r = ransac(a[0], b[0], corr, 1.5 * voxel, H, seed)
    return r.T, a[0], corr, r
