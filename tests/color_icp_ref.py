"""NumPy restatement of include/r3d.h, "Coloured ICP": the f32 intensity, the fp64 tangent-plane gradient in the written order,
the 31 sums as plain fp64 sums, and the loop over icp.plane_step_from_sums (the library's host solver; everything else here is
NumPy).  Written from the header text, not from the kernels.  Every elementwise expression keeps the header's order of operations,
so the intensity, the gradient and (float) rI are comparable bit for bit.  The neighbour lists and the NN matches are INPUTS: the
tests take them from knn_lists / nearest below, a brute-force (d2, j) search in f32 with the index's fmaf expression.  Also the
textured wall the tests register on.

The header's text, restated:

  Intensity (f32): R = w & 255, G = (w >> 8) & 255, B = (w >> 16) & 255 of the colour word w, each converted to f32;
    I = (0.299f R + 0.587f G) + 0.114f B.  The alpha byte is never read.
  Neighbourhood: N_i = row i of the k-lists, tails dropped, cut, when radius > 0, at the first entry with
    d2 > (float)((double) radius * radius).  c_i = |N_i|.
  Gradient: with n = (double) normals[i], p_i = (double) P[i], and A_00, A_01, A_02, A_11, A_12, A_22, b_0, b_1, b_2 = 0.0, for each
    entry j of N_i in list order:
      e_a = (double) p_j,a - p_i,a;  h = (e_0 n_0 + e_1 n_1) + e_2 n_2;  t_a = e_a - h n_a;  dI = (double) I_j - (double) I_i
      A_ab += t_a t_b for ab in 00, 01, 02, 11, 12, 22;  b_a += t_a dI
    then with c = (double) c_i, c2 = c c:  A_ab += (c2 n_a) n_b for the same six ab.  Adjugate:
      C00 = A_11 A_22 - A_12 A_12;  C01 = A_02 A_12 - A_01 A_22;  C02 = A_01 A_12 - A_02 A_11
      C11 = A_00 A_22 - A_02 A_02;  C12 = A_01 A_02 - A_00 A_12;  C22 = A_00 A_11 - A_01 A_01
      det = (A_00 C00 + A_01 C01) + A_02 C02;  tr = (A_00 + A_11) + A_22
      g_0 = ((C00 b_0 + C01 b_1) + C02 b_2) / det;  g_1 = ((C01 b_0 + C11 b_1) + C12 b_2) / det;
      g_2 = ((C02 b_0 + C12 b_1) + C22 b_2) / det
    grad = (float) g.
  No gradient = a row of three NaN: a zero or non-finite normal; a non-finite point; c_i < 3; det not finite; unless
    det > R3D_COLOR_GRADIENT_FLOOR ((tr tr) tr), R3D_COLOR_GRADIENT_FLOOR = 1e-14.
  Geometric pair k = (p = src[k], q = tgt[idx[k]], n = normals[idx[k]]): out when idx[k] >= n_tgt, when max_d2 >= 0 and not
    (d2[k] <= max_d2), when n is the zero vector, when r = n_0 (p_0 - q_0) + n_1 (p_1 - q_1) + n_2 (p_2 - q_2) or (p_0 + p_1) + p_2 is
    not finite.  With J = [p x n ; n]: [0] += 1; [1] += r r; [2 + a] += J_a r; [8..28] += the upper triangle of J_a J_b, row-major.
  Photometric term of an accepted geometric pair:
      p'_a = p_a - r n_a;  d_a = p'_a - q_a;  rI = ((double) I_q + ((g_0 d_0 + g_1 d_1) + g_2 d_2)) - (double) I_p
      gn = (g_0 n_0 + g_1 n_1) + g_2 n_2;  a_c = g_c - gn n_c
    the pair enters iff rI, a_0, a_1, a_2 are all finite and |rI| <= i_max; then with w = w_photo and J = [p x a ; a]:
    [2 + k] += (w J_k) rI; [8..28] += the upper triangle of (w J_k) J_l; [29] += 1; [30] += rI rI.
  Loop: NN -> the pass -> step from the first 29 sums -> state update -> src = (float)(T_total . src_orig).  A singular solve sets
    the sticky status 1 and moves nothing."""
import importlib

import numpy as np

import icp_state_ref as SR
from helpers import PKG
from outliers_ref import NO_ROW, knn_brute
from oracle.icp_ref import nearest_neighbours

F = np.float32
FLOOR = 1e-14          # R3D_COLOR_GRADIENT_FLOOR
SUMS = 31


def words(rgb, alpha=None):
    """[N,3] uint8 -> the colour words r | g << 8 | b << 16 (| alpha << 24)"""
    c = np.asarray(rgb, dtype=np.uint8).reshape(-1, 3).astype(np.uint32)
    w = c[:, 0] | (c[:, 1] << 8) | (c[:, 2] << 16)
    if alpha is not None:
        w = w | (np.asarray(alpha, dtype=np.uint32) << 24)
    return w.astype(np.uint32)


def intensity(rgba):
    """I = (0.299f R + 0.587f G) + 0.114f B, f32"""
    w = np.asarray(rgba, dtype=np.uint32)
    r, g, b = (w & 255).astype(F), ((w >> 8) & 255).astype(F), ((w >> 16) & 255).astype(F)
    out = (F(0.299) * r + F(0.587) * g) + F(0.114) * b
    assert out.dtype == F
    return out


def knn_lists(xyz, k):
    """(idx [N,k] uint32, d2 [N,k] float32): brute force, ascending (d2, row), tails (0xffffffff, +inf)"""
    return knn_brute(np.asarray(xyz, F), k)


def nearest(src, tgt):
    """(idx [N] uint32, d2 [N] float32): brute force, lowest row on ties; a source without a finite d2 gets (0, +inf)"""
    with np.errstate(all="ignore"):
        s, t = np.asarray(src, F), np.asarray(tgt, F)
        idx, d2 = nearest_neighbours(s, t)
    return idx, d2


def gradients(xyz, normals, rgba, idx, d2, radius=None, details=False):
    """(I [N] f32, grad [N,3] f32, count [N] uint32) from stored lists.  details: also det, tr [N] f64."""
    P = np.asarray(xyz, F).astype(np.float64)
    N = np.asarray(normals, F)
    n = N.astype(np.float64)
    I = intensity(rgba)
    npts, k = idx.shape
    r2 = F(np.inf) if radius is None or not radius > 0 else F(np.float64(radius) * np.float64(radius))
    A = {ab: np.zeros(npts) for ab in ("00", "01", "02", "11", "12", "22")}
    b = [np.zeros(npts) for _ in range(3)]
    count = np.zeros(npts, np.uint32)
    live = np.ones(npts, bool)
    with np.errstate(all="ignore"):
        for t in range(k):
            j = idx[:, t]
            live = live & (j != NO_ROW) & (j.astype(np.int64) < npts) & ~(d2[:, t] > r2)
            jj = np.where(live, j, 0).astype(np.int64)
            count += live.astype(np.uint32)
            e = [P[jj, a] - P[:, a] for a in range(3)]
            h = (e[0] * n[:, 0] + e[1] * n[:, 1]) + e[2] * n[:, 2]
            tt = [e[a] - h * n[:, a] for a in range(3)]
            dI = I[jj].astype(np.float64) - I.astype(np.float64)
            for ab in A:
                a_, b_ = int(ab[0]), int(ab[1])
                A[ab] = A[ab] + np.where(live, tt[a_] * tt[b_], 0.0)
            for a in range(3):
                b[a] = b[a] + np.where(live, tt[a] * dI, 0.0)
        c = count.astype(np.float64)
        c2 = c * c
        for ab in A:
            a_, b_ = int(ab[0]), int(ab[1])
            A[ab] = A[ab] + (c2 * n[:, a_]) * n[:, b_]
        C00 = A["11"] * A["22"] - A["12"] * A["12"]
        C01 = A["02"] * A["12"] - A["01"] * A["22"]
        C02 = A["01"] * A["12"] - A["02"] * A["11"]
        C11 = A["00"] * A["22"] - A["02"] * A["02"]
        C12 = A["01"] * A["02"] - A["00"] * A["12"]
        C22 = A["00"] * A["11"] - A["01"] * A["01"]
        det = (A["00"] * C00 + A["01"] * C01) + A["02"] * C02
        tr = (A["00"] + A["11"]) + A["22"]
        g = np.stack([((C00 * b[0] + C01 * b[1]) + C02 * b[2]) / det,
                      ((C01 * b[0] + C11 * b[1]) + C12 * b[2]) / det,
                      ((C02 * b[0] + C12 * b[1]) + C22 * b[2]) / det], axis=1)
        ok = np.isfinite(P).all(axis=1) & np.isfinite(N).all(axis=1) & (N != 0).any(axis=1) & (count >= 3)
        ok = ok & np.isfinite(det) & (det > FLOOR * ((tr * tr) * tr))
        grad = np.where(ok[:, None], g, np.nan).astype(F)
    if details:
        return I, grad, count, det, tr
    return I, grad, count


def photo_term(p, q, n, Iq, g, Ip):
    """(r, rI, a [..,3]) of pairs given as fp64 arrays [..,3] / [..]: the geometric residual, the photometric residual and the
    tangent gradient, in the header's order"""
    r = (n[..., 0] * (p[..., 0] - q[..., 0]) + n[..., 1] * (p[..., 1] - q[..., 1])) + n[..., 2] * (p[..., 2] - q[..., 2])
    d = [(p[..., a] - r * n[..., a]) - q[..., a] for a in range(3)]
    rI = (Iq + ((g[..., 0] * d[0] + g[..., 1] * d[1]) + g[..., 2] * d[2])) - Ip
    gn = (g[..., 0] * n[..., 0] + g[..., 1] * n[..., 1]) + g[..., 2] * n[..., 2]
    a = np.stack([g[..., c] - gn * n[..., c] for c in range(3)], axis=-1)
    return r, rI, a


def _jacobian(p, v):
    return np.concatenate([np.cross(p, v), v], axis=1)


def _normal_equations(sums, J, w, r):
    """[2..7] += sum (w J_a) r, [8..28] += the upper triangle of sum (w J_a) J_b, row-major"""
    wJ = w * J
    sums[2:8] += (wJ * r[:, None]).sum(axis=0)
    k = 8
    for a in range(6):
        for b in range(a, 6):
            sums[k] += (wJ[:, a] * J[:, b]).sum()
            k += 1


class Pass:
    pass


def accumulate(src, src_I, tgt, normals, tgt_I, tgt_grad, idx, d2, max_d2, w_photo, i_max):
    """Pass with sums [31], photo [N] f32 ((float) rI where a photometric pair entered, NaN elsewhere), geo / pho: the boolean
    masks of the pairs that entered, rI [N] f64 (NaN where there is no geometric pair)"""
    S, T, Nn = np.asarray(src, F), np.asarray(tgt, F), np.asarray(normals, F)
    idx = np.asarray(idx, np.uint32).astype(np.int64)
    n_src, n_tgt = S.shape[0], T.shape[0]
    out = Pass()
    with np.errstate(all="ignore"):
        inside = idx < n_tgt
        j = np.where(inside, idx, 0)
        ok = inside.copy()
        if max_d2 >= 0:
            ok &= np.asarray(d2, F) <= F(max_d2)
        p, q, n = S.astype(np.float64), T[j].astype(np.float64), Nn[j].astype(np.float64)
        g = np.asarray(tgt_grad, F)[j].astype(np.float64)
        Iq, Ip = np.asarray(tgt_I, F)[j].astype(np.float64), np.asarray(src_I, F).astype(np.float64)
        ok &= (Nn[j] != 0).any(axis=1)
        r, rI, a = photo_term(p, q, n, Iq, g, Ip)
        ok &= np.isfinite(r) & np.isfinite((p[:, 0] + p[:, 1]) + p[:, 2])
        pho = ok & np.isfinite(rI) & np.isfinite(a).all(axis=1) & (np.abs(rI) <= i_max)
    sums = np.zeros(SUMS)
    sums[0] = float(ok.sum())
    sums[1] = (r[ok] * r[ok]).sum()
    _normal_equations(sums, _jacobian(p[ok], n[ok]), 1.0, r[ok])
    _normal_equations(sums, _jacobian(p[pho], a[pho]), float(w_photo), rI[pho])
    sums[29] = float(pho.sum())
    sums[30] = (rI[pho] * rI[pho]).sum()
    out.sums, out.geo, out.pho = sums, ok, pho
    out.photo = np.where(pho, rI, np.nan).astype(F)
    out.rI = np.where(ok, rI, np.nan)
    return out


def apply_T(T, xyz):
    """(float)(row . [x y z 1]) of a row-major 4x4 on an f32 cloud, in fp64"""
    T = np.asarray(T, np.float64).reshape(4, 4)
    P = np.asarray(xyz, F).astype(np.float64)
    return np.stack([((T[a, 0] * P[:, 0] + T[a, 1] * P[:, 1]) + T[a, 2] * P[:, 2]) + T[a, 3] for a in range(3)], axis=1).astype(F)


def loop(src, src_I, tgt, normals, tgt_I, tgt_grad, n_iters, max_d2, w_photo, i_max):
    """(state [512], last Pass): n_iters passes from a reset state on the source as given"""
    icp = importlib.import_module(PKG + ".icp")
    st = SR.reset()
    src0 = np.asarray(src, F)
    moved, last = src0, None
    for _ in range(n_iters):
        idx, d2 = nearest(moved, tgt)
        last = accumulate(moved, src_I, tgt, normals, tgt_I, tgt_grad, idx, d2, max_d2, w_photo, i_max)
        s = last.sums
        rms = float(np.sqrt(max(s[1], 0.0) / s[0])) if s[0] > 0 else 0.0
        try:
            T, _ = icp.plane_step_from_sums(s[:29])
            bad = 0
        except ValueError:
            T, bad = np.eye(4), 1
        st = SR.advance(st, T.reshape(16), rms, bad, s[0])
        moved = apply_T(st[SR.T_TOTAL:SR.T_TOTAL + 16], src0)
    return st, last


# ---- the scene: one textured wall ------------------------------------------------------------------------------------------------
SPACING = 0.02
WALL_W, WALL_H = 64, 48


def wall_colour(x, y):
    """[N,3] uint8: per channel a sum of sinusoids of wavelengths between 8 and 31 spacings, over wall coordinates in metres"""
    u, v = np.asarray(x, np.float64) / SPACING, np.asarray(y, np.float64) / SPACING
    out = []
    for (l1, l2, l3, ph) in ((8.0, 13.0, 31.0, 0.3), (9.0, 17.0, 23.0, 1.1), (11.0, 19.0, 29.0, 2.0)):
        s = (np.sin(2 * np.pi * u / l1 + ph) * np.cos(2 * np.pi * v / l2) + np.sin(2 * np.pi * (u + v) / l3 + 2 * ph)
             + np.cos(2 * np.pi * (u - 2 * v) / (l2 + 5.0) - ph))
        out.append(np.clip(np.rint(127.5 + 40.0 * s), 0, 255).astype(np.uint8))
    return np.stack(out, axis=1)


def wall_scene(seed=0, shift=(0.031, -0.027), angle_deg=1.0):
    """The issue's scene.  Target: a 64 x 48 grid at z = 1.5, spacing 0.02 m, jittered by up to 0.3 spacings in the plane.
    Source: the same wall sampled at other jittered positions (inset by four spacings so that it stays on the target after the
    move), then moved in the plane by `shift` (about two spacings) and angle_deg about the normal through the wall's centre.
    Returns a dict: tgt, tgt_rgba, normals (0, 0, 1), src, src_rgba, T_true (src -> tgt)."""
    rng = np.random.default_rng(seed)
    gx, gy = np.meshgrid(np.arange(WALL_W), np.arange(WALL_H), indexing="xy")
    base = np.stack([gx.ravel(), gy.ravel()], axis=1).astype(np.float64) * SPACING

    def sample(pts):
        q = pts + rng.uniform(-0.3, 0.3, pts.shape) * SPACING
        xyz = np.concatenate([q, np.full((q.shape[0], 1), 1.5)], axis=1).astype(F)
        return xyz, words(wall_colour(xyz[:, 0].astype(np.float64), xyz[:, 1].astype(np.float64)))

    tgt, tgt_rgba = sample(base)
    inner = (gx.ravel() >= 4) & (gx.ravel() < WALL_W - 4) & (gy.ravel() >= 4) & (gy.ravel() < WALL_H - 4)
    on_wall, src_rgba = sample(base[inner] + 0.5 * SPACING * np.array([0.37, -0.21]))
    a = np.deg2rad(angle_deg)
    c = np.array([0.5 * (WALL_W - 1) * SPACING, 0.5 * (WALL_H - 1) * SPACING, 1.5])
    R = np.array([[np.cos(a), -np.sin(a), 0.0], [np.sin(a), np.cos(a), 0.0], [0.0, 0.0, 1.0]])
    M = np.eye(4)                       # wall -> where the source is handed over
    M[:3, :3] = R
    M[:3, 3] = c - R @ c + np.array([shift[0], shift[1], 0.0])
    src = apply_T(M, on_wall)
    normals = np.tile(F([0, 0, 1]), (tgt.shape[0], 1))
    return {"tgt": tgt, "tgt_rgba": tgt_rgba, "normals": normals, "src": src, "src_rgba": src_rgba, "T_true": np.linalg.inv(M)}


def in_plane_error(T, scene):
    """RMS distance in metres, over the source points, between where T puts them and where T_true does"""
    a, b = apply_T(T, scene["src"]).astype(np.float64), apply_T(scene["T_true"], scene["src"]).astype(np.float64)
    return float(np.sqrt(((a - b)[:, :2] ** 2).sum(axis=1).mean()))


# what the tests run on the wall, and the figure the restatement loop reaches there (tests/test_color_icp_host.py prints it):
# k = 8, i_max = 40, lambda_geometric = 0.968
WALL_ITERS = 20
WALL_MAX_DIST = 3 * SPACING
WALL_MAX_D2 = WALL_MAX_DIST ** 2
WALL_ERROR_AFTER = 1.84e-4   # metres, in-plane RMS after WALL_ITERS passes (1.8315e-04, rounded up); before: 4.1675e-02
