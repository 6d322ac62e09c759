"""NumPy restatement of the multiway-registration text of include/r3d.h: the 11 pair sums (r3d_registration_sums, as plain fp64
sums -- the reduction tree is not restated, the tests bound the difference), the information matrix, fitness and rmse
(r3d_information_from_sums, the same handful of fp64 operations) and a plain dense Levenberg-Marquardt pose-graph optimiser with
the same residual, cost, weights, damping rule, stopping rule and pruning (r3d_posegraph_optimize).  Test infrastructure only."""
import math

import numpy as np


# ---- pair sums ----------------------------------------------------------------------------------------------------------------

def registration_sums(src, tgt, idx, d2, max_d2):
    """(sums [11] float64, magnitudes [11] float64 = the sums of the terms' absolute values, for the summation bound)."""
    src, tgt = np.asarray(src, np.float32), np.asarray(tgt, np.float32)
    idx, d2 = np.asarray(idx, np.uint32).astype(np.int64), np.asarray(d2, np.float32)
    with np.errstate(invalid="ignore"):
        keep = (idx < tgt.shape[0]) & (d2 <= np.float32(max_d2))
    keep &= np.isfinite(src).all(axis=1)
    q = tgt[np.where(keep, idx, 0)].astype(np.float64)
    keep &= np.isfinite(q).all(axis=1)
    q, d = q[keep], d2[keep].astype(np.float64)
    terms = np.stack([np.ones(len(q)), q[:, 0], q[:, 1], q[:, 2], q[:, 0] * q[:, 0], q[:, 0] * q[:, 1], q[:, 0] * q[:, 2],
                      q[:, 1] * q[:, 1], q[:, 1] * q[:, 2], q[:, 2] * q[:, 2], d], axis=1)
    return np.array([math.fsum(c) for c in terms.T]), np.abs(terms).sum(axis=0)


def information_from_sums(s, n_src):
    """(info [6,6], fitness, rmse)"""
    s = np.asarray(s, np.float64)
    n = s[0]
    info = np.array([[s[7] + s[9], -s[5], -s[6], 0.0, -s[3], s[2]],
                     [-s[5], s[4] + s[9], -s[8], s[3], 0.0, -s[1]],
                     [-s[6], -s[8], s[4] + s[7], -s[2], s[1], 0.0],
                     [0.0, s[3], -s[2], n, 0.0, 0.0],
                     [-s[3], 0.0, s[1], 0.0, n, 0.0],
                     [s[2], -s[1], 0.0, 0.0, 0.0, n]])
    return info, (n / n_src if n_src > 0 else 0.0), (math.sqrt(s[10] / n) if n > 0 else 0.0)


def information_direct(q):
    """sum G^T G with G = [-[q]x | I] over the rows of q, built pair by pair"""
    lam = np.zeros((6, 6))
    for p in np.asarray(q, np.float64):
        G = np.hstack([-hat(p), np.eye(3)])
        lam += G.T @ G
    return lam


# ---- SO(3) / SE(3) --------------------------------------------------------------------------------------------------------------

def hat(w):
    return np.array([[0.0, -w[2], w[1]], [w[2], 0.0, -w[0]], [-w[1], w[0], 0.0]])


def so3_exp(w):
    th = float(np.linalg.norm(w))
    W = hat(w)
    if th < 1e-8:
        return np.eye(3) + W + 0.5 * W @ W
    return np.eye(3) + math.sin(th) / th * W + (1.0 - math.cos(th)) / th ** 2 * W @ W


def se3_exp(d):
    w, v = np.asarray(d[:3], np.float64), np.asarray(d[3:], np.float64)
    th = float(np.linalg.norm(w))
    W = hat(w)
    if th < 1e-4:
        V = np.eye(3) + 0.5 * W + W @ W / 6.0
    else:
        V = np.eye(3) + (1.0 - math.cos(th)) / th ** 2 * W + (th - math.sin(th)) / th ** 3 * W @ W
    T = np.eye(4)
    T[:3, :3], T[:3, 3] = so3_exp(w), V @ v
    return T


def so3_log(R):
    """rotation vector, |w| <= pi, through the eigenvector of the symmetric part near pi and the skew part elsewhere"""
    c = min(1.0, max(-1.0, (np.trace(R) - 1.0) / 2.0))
    axis = np.array([R[2, 1] - R[1, 2], R[0, 2] - R[2, 0], R[1, 0] - R[0, 1]])
    s = float(np.linalg.norm(axis)) / 2.0
    th = math.atan2(s, c)
    if s > 1e-6:
        return axis / (2.0 * s) * th
    if c > 0.0:
        return axis / 2.0
    vals, vecs = np.linalg.eigh((R + R.T) / 2.0)          # th ~ pi: the axis is the eigenvector of eigenvalue 1
    a = vecs[:, np.argmax(vals)]
    if axis @ a < 0:
        a = -a
    return a * th


def inverse(T):
    out = np.eye(4)
    out[:3, :3] = T[:3, :3].T
    out[:3, 3] = -T[:3, :3].T @ T[:3, 3]
    return out


def pose(w, t):
    T = np.eye(4)
    T[:3, :3], T[:3, 3] = so3_exp(np.asarray(w, np.float64)), t
    return T


def random_pose(rng, max_angle, max_shift):
    w = rng.normal(size=3)
    w *= rng.uniform(0.0, max_angle) / np.linalg.norm(w)
    return pose(w, rng.uniform(-1.0, 1.0, 3) * max_shift / math.sqrt(3.0))


def pose_distance(A, B):
    """(angle in rad, distance) between two poses"""
    D = inverse(A) @ B
    return float(np.linalg.norm(so3_log(D[:3, :3]))), float(np.linalg.norm(A[:3, 3] - B[:3, 3]))


def left_jacobian_inverse(w):
    th = float(np.linalg.norm(w))
    W = hat(w)
    k = 1.0 / 12.0 + th * th / 720.0 if th < 1e-3 else (1.0 - 0.5 * th / math.tan(0.5 * th)) / th ** 2
    return np.eye(3) - 0.5 * W + k * W @ W


def edge_residual(Xs, Xt, T, jacobian=False):
    """xi = (w, v) of E = T^-1 Xt^-1 Xs, and its derivative by the left perturbation of Xs (that by Xt's is its negative)"""
    A = inverse(Xt @ T)
    E = A @ Xs
    xi = np.concatenate([so3_log(E[:3, :3]), E[:3, 3]])
    if not jacobian:
        return xi
    J = np.zeros((6, 6))
    J[:3, :3] = left_jacobian_inverse(xi[:3]) @ A[:3, :3]
    J[3:, :3] = hat(A[:3, 3] - E[:3, 3]) @ A[:3, :3]
    J[3:, 3:] = A[:3, :3]
    return xi, J


# ---- pose-graph optimisation ------------------------------------------------------------------------------------------------------

class _Graph:
    def __init__(self, n, nodes, Ts, infos, uncertain, pref, dist):
        self.n, self.nodes, self.Ts, self.unc = n, nodes, Ts, uncertain
        self.L = [(L + L.T) / 2.0 for L in infos]
        self.active = [True] * len(nodes)
        self.robust, self.pref, self.dist, self.mu = math.isfinite(pref), pref, dist, 0.0
        self.update_mu()

    def update_mu(self):
        counts = [self.L[e][5, 5] for e in range(len(self.nodes)) if self.active[e] and self.unc[e]]
        self.mu = self.pref * self.dist ** 2 * float(np.mean(counts)) if counts and self.robust else 0.0

    def weight(self, e, chi2):
        if not self.robust or not self.unc[e] or not self.mu + chi2 > 0.0:
            return 1.0
        return (self.mu / (self.mu + chi2)) ** 2

    def evaluate(self, poses):
        """(C, F, weights)"""
        C = F = 0.0
        w = np.zeros(len(self.nodes))
        for e, (s, t) in enumerate(self.nodes):
            if not self.active[e]:
                continue
            xi = edge_residual(poses[s], poses[t], self.Ts[e])
            chi2 = float(xi @ self.L[e] @ xi)
            w[e] = self.weight(e, chi2)
            C += w[e] * chi2
            F += self.mu * chi2 / (self.mu + chi2) if self.robust and self.unc[e] and self.mu + chi2 > 0.0 else w[e] * chi2
        return C, F, w

    def normal_equations(self, poses):
        dim = 6 * (self.n - 1)
        H, g = np.zeros((dim, dim)), np.zeros(dim)
        for e, (s, t) in enumerate(self.nodes):
            if not self.active[e]:
                continue
            xi, Js = edge_residual(poses[s], poses[t], self.Ts[e], jacobian=True)
            w = self.weight(e, float(xi @ self.L[e] @ xi))
            J = np.zeros((6, dim))
            if s:
                J[:, 6 * (s - 1):6 * s] = Js
            if t:
                J[:, 6 * (t - 1):6 * t] = -Js
            H += w * J.T @ self.L[e] @ J
            g += w * J.T @ self.L[e] @ xi
        return H, g

    def loop(self, poses, max_iters):
        """(poses, iterations, status)"""
        dim = 6 * (self.n - 1)
        F = self.evaluate(poses)[1]
        if dim == 0:
            return poses, 0, 0
        lam, nu, fresh, iters = -1.0, 2.0, False, 0
        for _ in range(max_iters):
            if F == 0.0:
                return poses, iters, 0
            if not fresh:
                H, g = self.normal_equations(poses)
                fresh = True
            if lam < 0.0:
                top = float(np.diag(H).max())
                if not top > 0.0:
                    return poses, iters, 0
                lam = 1e-6 * top
            iters += 1
            try:
                np.linalg.cholesky(H + lam * np.eye(dim))
            except np.linalg.LinAlgError:
                lam *= 10.0
                continue
            d = -np.linalg.solve(H + lam * np.eye(dim), g)
            pred = float(d @ (lam * d - g))
            trial = poses.copy()
            for i in range(1, self.n):
                trial[i] = se3_exp(d[6 * (i - 1):6 * i]) @ poses[i]
            Fn = self.evaluate(trial)[1]
            if np.abs(d).max() < 1e-10:
                return (trial if Fn <= F else poses), iters, 0
            if Fn < F:
                drop = F - Fn
                rho = drop / pred if pred > 0.0 else 1.0
                poses, fresh = trial, False
                lam *= max(1.0 / 3.0, 1.0 - (2.0 * rho - 1.0) ** 3)
                nu = 2.0
                flat = drop < 1e-14 * F
                F = Fn
                if flat:
                    return poses, iters, 0
            else:
                lam *= nu
                nu *= 2.0
                if not math.isfinite(lam):
                    return poses, iters, 0
        return poses, iters, 0 if F == 0.0 else 1


def posegraph_optimize(poses, nodes, Ts, infos, uncertain, max_correspondence_distance, preference_loop_closure=1.0,
                       prune_threshold=0.25, max_iters=100):
    """(poses [N,4,4], weights [M], report dict) as r3d_posegraph_optimize defines them"""
    poses = np.array(poses, np.float64)
    G = _Graph(poses.shape[0], [tuple(int(v) for v in e) for e in nodes], [np.asarray(T, np.float64) for T in Ts],
               [np.asarray(L, np.float64) for L in infos], [bool(u) for u in uncertain], float(preference_loop_closure),
               float(max_correspondence_distance))
    c0 = G.evaluate(poses)[0]
    poses, iters, status = G.loop(poses, max_iters)
    c1, _, w = G.evaluate(poses)
    pruned = 0
    if G.robust:
        for e in range(len(G.nodes)):
            if G.unc[e] and w[e] < prune_threshold:
                G.active[e] = False
                pruned += 1
        if pruned:
            G.update_mu()
            poses, more, status2 = G.loop(poses, max_iters)
            iters, status = iters + more, status | status2
            c1, _, w = G.evaluate(poses)
    return poses, w, {"initial_cost": c0, "final_cost": c1, "iterations": iters, "pruned": pruned, "max_iters_reached": bool(status)}
