"""NumPy fp64 restatement of include/r3d.h, "TSDF tracking": the projective association with its reject codes, the residuals, the
29 sums (as plain fp64 sums: the reduction tree is not restated), the step through icp.plane_step_from_sums (the library's host
code), the loop and the pose composition.  Written from the header text, not from the kernel.  Every elementwise expression keeps
the header's order of operations, so match codes and (float) r are comparable bit for bit."""
import importlib

import numpy as np

from helpers import PKG


def matmul4(A, B):
    """every entry summed over m = 0..3 in ascending order starting from 0.0"""
    out = np.zeros((4, 4))
    for r in range(4):
        for c in range(4):
            v = 0.0
            for m in range(4):
                v += A[r, m] * B[m, c]
            out[r, c] = v
    return out


def inverse_pose(row):
    """S of r3d_tsdf_track: S[a][b] = R[b][a], S[a][3] = -((R[0][a] t0 + R[1][a] t1) + R[2][a] t2)"""
    row = np.asarray(row, dtype=np.float64).reshape(12)
    R, t = row[:9].reshape(3, 3), row[9:]
    S = np.zeros((4, 4))
    for a in range(3):
        S[a, :3] = R[:, a]
        S[a, 3] = -((R[0, a] * t[0] + R[1, a] * t[1]) + R[2, a] * t[2])
    S[3, 3] = 1.0
    return S


def pose_from(T_total, S):
    """R_out = M[:3,:3]^T, t_out_a = -((R_out[a][0] M[0][3] + R_out[a][1] M[1][3]) + R_out[a][2] M[2][3]), M = T_total . S"""
    M = matmul4(np.asarray(T_total, dtype=np.float64), np.asarray(S, dtype=np.float64))
    out = np.zeros(12)
    Ro = M[:3, :3].T
    out[:9] = Ro.reshape(9)
    for a in range(3):
        out[9 + a] = -((Ro[a, 0] * M[0, 3] + Ro[a, 1] * M[1, 3]) + Ro[a, 2] * M[2, 3])
    return out


def pose_matrix(row):
    row = np.asarray(row, dtype=np.float64).reshape(12)
    T = np.eye(4)
    T[:3, :3], T[:3, 3] = row[:9].reshape(3, 3), row[9:]
    return T


def pose_error(row_a, row_b):
    """(rotation angle in degrees, distance of the camera centres) between two world -> camera rows"""
    Ta, Tb = pose_matrix(row_a), pose_matrix(row_b)
    Rd = Ta[:3, :3] @ Tb[:3, :3].T
    ang = np.degrees(np.arccos(np.clip((np.trace(Rd) - 1.0) / 2.0, -1.0, 1.0)))
    ca, cb = -Ta[:3, :3].T @ Ta[:3, 3], -Tb[:3, :3].T @ Tb[:3, 3]
    return float(ang), float(np.linalg.norm(ca - cb))


class Pass:
    """One association pass: match [H*W] int32, residual [H*W] float32, sums [29] float64, and upv = the u + 0.5 and v + 0.5 of
    every pixel that reached the rounding (for the callers' distance-to-an-integer check)."""


def associate(src_vertex, src_normal, model_vertex, model_normal, model_pose, S, K, dist_max, cos_min, T_total=None):
    sv = np.asarray(src_vertex, dtype=np.float32)
    H, W = sv.shape[:2]
    n_px = H * W
    sv = sv.reshape(n_px, 3)
    mv = np.asarray(model_vertex, dtype=np.float32).reshape(n_px, 3)
    mn = np.asarray(model_normal, dtype=np.float32).reshape(n_px, 3)
    sn = None if src_normal is None else np.asarray(src_normal, dtype=np.float32).reshape(n_px, 3)
    pose = np.asarray(model_pose, dtype=np.float64).reshape(12)
    Rm, tm = pose[:9].reshape(3, 3), pose[9:]
    fx, fy, cx, cy = [float(v) for v in K]
    M = matmul4(np.eye(4) if T_total is None else np.asarray(T_total, dtype=np.float64), np.asarray(S, dtype=np.float64))
    match = np.full(n_px, -1, dtype=np.int32)
    with np.errstate(all="ignore"):
        x, y, z = [sv[:, a].astype(np.float64) for a in range(3)]
        live = np.isfinite(x) & np.isfinite(y) & np.isfinite(z) & (z > 0)                                     # 1
        p = np.stack([((M[a, 0] * x + M[a, 1] * y) + M[a, 2] * z) + M[a, 3] for a in range(3)], axis=1)       # 3
        pm = np.stack([((Rm[a, 0] * p[:, 0] + Rm[a, 1] * p[:, 1]) + Rm[a, 2] * p[:, 2]) + tm[a] for a in range(3)], axis=1)   # 4
        front = pm[:, 2] > 0                                                                                  # 5
        u = fx * (pm[:, 0] / pm[:, 2]) + cx
        v = fy * (pm[:, 1] / pm[:, 2]) + cy
        uj, vj = np.floor(u + 0.5), np.floor(v + 0.5)
        inside = front & (uj >= 0) & (uj < W) & (vj >= 0) & (vj < H)
        match[live & ~inside] = -2
        live &= inside
        j = np.where(live, vj * W + uj, 0).astype(np.int64)                                                   # 6
        q, n = mv[j].astype(np.float64), mn[j].astype(np.float64)
        surf = np.isfinite(q).all(axis=1) & np.isfinite(n).all(axis=1) & (n != 0).any(axis=1)                 # 7
        match[live & ~surf] = -3
        live &= surf
        d = p - q
        near = (d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2] <= dist_max * dist_max             # 8
        match[live & ~near] = -4
        live &= near
        if sn is not None:                                                                                    # 9
            ns = sn.astype(np.float64)
            ok = np.isfinite(ns).all(axis=1) & (ns != 0).any(axis=1)
            g = np.stack([(M[a, 0] * ns[:, 0] + M[a, 1] * ns[:, 1]) + M[a, 2] * ns[:, 2] for a in range(3)], axis=1)
            ok &= (g[:, 0] * n[:, 0] + g[:, 1] * n[:, 1]) + g[:, 2] * n[:, 2] >= cos_min
            match[live & ~ok] = -5
            live &= ok
        r = n[:, 0] * (p[:, 0] - q[:, 0]) + n[:, 1] * (p[:, 1] - q[:, 1]) + n[:, 2] * (p[:, 2] - q[:, 2])      # 10
    match[live] = j[live].astype(np.int32)
    out = Pass()
    out.match = match
    out.residual = np.where(live, r, 0.0).astype(np.float32)
    pl, nl, rl = p[live], n[live], r[live]
    J = np.concatenate([np.cross(pl, nl), nl], axis=1) if len(pl) else np.zeros((0, 6))
    sums = np.zeros(29)
    sums[0] = float(len(pl))
    sums[1] = np.sum(rl * rl)
    sums[2:8] = (J * rl[:, None]).sum(axis=0)
    k = 8
    for a in range(6):
        for b in range(a, 6):
            sums[k] = np.sum(J[:, a] * J[:, b])
            k += 1
    out.sums = sums
    reached = front & np.isfinite(x) & np.isfinite(y) & np.isfinite(z) & (z > 0)
    out.upv = np.concatenate([(u + 0.5)[reached], (v + 0.5)[reached]])
    return out


def rounding_margin(upv):
    """the smallest distance of a finite u + 0.5 / v + 0.5 to an integer"""
    f = upv[np.isfinite(upv)]
    f = f[np.abs(f) < 1e15]
    return float(np.abs(f - np.round(f)).min()) if f.size else 1.0


def loop(src_vertex, src_normal, model_vertex, model_normal, model_pose, S, K, dist_max, cos_min, n_iters):
    """(T_total, info): n_iters iterations of associate -> sums -> step; a degenerate step sets status 1 and leaves T_total"""
    icp = importlib.import_module(PKG + ".icp")
    T_total = np.eye(4)
    info = {"status": 0, "pairs": 0.0, "rms": 0.0, "iterations": 0, "matched": 0}
    for _ in range(n_iters):
        a = associate(src_vertex, src_normal, model_vertex, model_normal, model_pose, S, K, dist_max, cos_min, T_total)
        info["pairs"] = float(a.sums[0])
        info["matched"] = int((a.match >= 0).sum())
        info["rms"] = float(np.sqrt(max(a.sums[1], 0.0) / a.sums[0])) if a.sums[0] > 0 else 0.0
        try:
            T, _ = icp.plane_step_from_sums(a.sums)
            T_total = matmul4(T, T_total)
        except ValueError:
            info["status"] = 1
        info["iterations"] += 1
    return T_total, info


def track(src_vertex, src_normal, model_vertex, model_normal, guess_row, K, dist_max, cos_min, n_iters):
    """r3d_tsdf_track from ready-made maps: (pose row, info); status 1 gives the guess back"""
    S = inverse_pose(guess_row)
    T_total, info = loop(src_vertex, src_normal, model_vertex, model_normal, guess_row, S, K, dist_max, cos_min, n_iters)
    if info["status"]:
        return np.asarray(guess_row, dtype=np.float64).reshape(12).copy(), info
    return pose_from(T_total, S), info


# ---- analytic maps of the box room ----------------------------------------------------------------------------------------------
def pose_row(q_xyzw, t):
    syn = importlib.import_module(PKG + ".synthetic")
    T = syn.pose_matrix(q_xyzw, t)
    return np.concatenate([T[:3, :3].reshape(9), T[:3, 3]])


def camera_points(z, K):
    """[H,W,3] float64 camera-frame points of a z-depth raster"""
    fx, fy, cx, cy = K
    H, W = z.shape
    u, v = np.meshgrid(np.arange(W), np.arange(H))
    return np.stack([(u - cx) / fx * z, (v - cy) / fy * z, z], axis=-1)


def room_maps(h, w, yaw, centre, pitch):
    """(world vertex map f32, inward axis normal of the nearest wall f32, camera-frame vertex map f32, pose row, K) of
    synthetic.room_view"""
    syn = importlib.import_module(PKG + ".synthetic")
    z, q, t, K = syn.room_view(h, w, yaw, centre, pitch=pitch)
    row = pose_row(q, t)
    T = pose_matrix(row)
    cam = camera_points(z, K)
    world = (cam.reshape(-1, 3) - T[:3, 3]) @ T[:3, :3]
    dist = np.concatenate([np.abs(world - syn.ROOM_LO), np.abs(syn.ROOM_HI - world)], axis=1)   # lo x y z, hi x y z
    face = dist.argmin(axis=1)
    normal = np.zeros_like(world)
    normal[np.arange(len(world)), face % 3] = np.where(face < 3, 1.0, -1.0)
    return (world.reshape(h, w, 3).astype(np.float32), normal.reshape(h, w, 3).astype(np.float32), cam.astype(np.float32), row, K)


def analytic_case(h, w, dyaw_deg, dpitch_deg, dcentre):
    """model at room_view(yaw 0.9, centre (0.3, -0.1, 0.4), pitch 0.2); source turned and moved by the given amounts"""
    yaw, centre, pitch = 0.9, np.array([0.3, -0.1, 0.4]), 0.2
    mv, mn, _, model_row, K = room_maps(h, w, yaw, centre, pitch)
    _, _, sv, true_row, _ = room_maps(h, w, yaw + np.radians(dyaw_deg), centre + np.asarray(dcentre), pitch + np.radians(dpitch_deg))
    return {"model_vertex": mv, "model_normal": mn, "src_vertex": sv, "model_row": model_row, "true_row": true_row, "K": K}
