"""NumPy restatement of include/r3d.h, "Depth pyramid": the half-sampler (every operation on np.float32 in the written order, so
its output is comparable bit for bit), the level camera rule, and the coarse-to-fine loop over ready-made per-level maps.  Written
from the header text, not from the kernel.  The association, the 4x4 products and the pose composition are track_ref's, the step
is icp.plane_step_from_sums (the library's host code).  Test infrastructure only."""
import importlib

import numpy as np

import track_ref as TR
from helpers import PKG

F = np.float32
MAX_LEVELS = 8


def depth_half(depth, max_jump):
    """[H >> 1, W >> 1] f32 of an [H, W] f32 raster (for in_stride 3 pass vertex[..., 2]: the same numbers)"""
    d = np.asarray(depth)
    assert d.dtype == F and d.ndim == 2 and d.shape[0] >= 2 and d.shape[1] >= 2
    oh, ow = d.shape[0] >> 1, d.shape[1] >> 1
    mj = F(max_jump)
    block = [d[0:2 * oh:2, 0:2 * ow:2], d[0:2 * oh:2, 1:2 * ow:2], d[1:2 * oh:2, 0:2 * ow:2], d[1:2 * oh:2, 1:2 * ow:2]]   # 2
    with np.errstate(all="ignore"):
        valid = [np.isfinite(b) & (b > 0) for b in block]                                                               # 1
        m = np.full((oh, ow), np.inf, F)
        for b, ok in zip(block, valid):                                                                                 # 3
            m = np.where(ok & (b < m), b, m)
        s = np.zeros((oh, ow), F)
        count = np.zeros((oh, ow), F)
        for b, ok in zip(block, valid):
            take = ok & (b - m <= mj)                                                                                   # 4
            s = np.where(take, s + b, s)                                                                                # 5
            count = np.where(take, count + F(1.0), count)
        out = np.where(count > 0, s / count, F(0.0))
    assert out.dtype == F and s.dtype == F and m.dtype == F
    return out


def pyramid_intrinsics(K, level):
    fx, fy, cx, cy = [float(v) for v in K]
    for _ in range(level):
        fx, fy, cx, cy = 0.5 * fx, 0.5 * fy, 0.5 * (cx - 0.5), 0.5 * (cy - 0.5)
    return fx, fy, cx, cy


def pyramid_shape(h, w, level):
    return h >> level, w >> level


def depth_levels(depth0, n_levels, max_jump):
    """[level 0 .. n_levels - 1] f32 rasters; depth0 is the z column of the level-0 vertex map"""
    out = [np.asarray(depth0, dtype=F)]
    for _ in range(1, n_levels):
        out.append(depth_half(out[-1], max_jump))
    return out


def loop(levels, iters, guess_row, dist_max, cos_min):
    """levels[l] = dict(src_vertex, src_normal (or None), model_vertex, model_normal, K), fine (0) to coarse; iters[l] passes at
    level l, from the coarsest down, on ONE state.  (T_total, info): info has status (sticky), pairs and rms of the last step,
    iterations, rms_history in execution order and margin = the smallest track_ref.rounding_margin of any pass."""
    icp = importlib.import_module(PKG + ".icp")
    S = TR.inverse_pose(guess_row)
    T_total = np.eye(4)
    info = {"status": 0, "pairs": 0.0, "rms": 0.0, "iterations": 0, "rms_history": [], "margin": 1.0, "matched": []}
    for l in range(len(levels) - 1, -1, -1):
        lv = levels[l]
        for _ in range(iters[l]):
            a = TR.associate(lv["src_vertex"], lv.get("src_normal"), lv["model_vertex"], lv["model_normal"], guess_row, S, lv["K"],
                             dist_max, cos_min, T_total)
            info["margin"] = min(info["margin"], TR.rounding_margin(a.upv))
            info["pairs"] = float(a.sums[0])
            info["rms"] = float(np.sqrt(max(a.sums[1], 0.0) / a.sums[0])) if a.sums[0] > 0 else 0.0
            info["rms_history"].append(info["rms"])
            info["matched"].append(int((a.match >= 0).sum()))
            try:
                T, _ = icp.plane_step_from_sums(a.sums)
                T_total = TR.matmul4(T, T_total)
            except ValueError:
                info["status"] = 1
            info["iterations"] += 1
    return T_total, info


def track(levels, iters, guess_row, dist_max, cos_min):
    """r3d_tsdf_track_pyramid from ready-made maps: (pose row, info); status 1 gives the guess back"""
    T_total, info = loop(levels, iters, guess_row, dist_max, cos_min)
    if info["status"]:
        return np.asarray(guess_row, dtype=np.float64).reshape(12).copy(), info
    return TR.pose_from(T_total, TR.inverse_pose(guess_row)), info


def unproject(depth, K):
    """[H,W,3] f32: r3d_unproject of an f32 raster with scale 1 -- X = (u - cx) / fx Z in double, one rounding"""
    return TR.camera_points(np.asarray(depth, dtype=F).astype(np.float64), K).astype(F)


def cpu_levels(vol, frame, guess_row, K, n_levels, max_jump, min_weight=1.0):
    """The maps of every level with no device: the source side from `frame` ([H,W] f32), the model side from raycast_ref over a
    tsdf_ref volume at the guess."""
    RC = importlib.import_module("raycast_ref")
    H, W = frame.shape
    sv0 = unproject(frame, K)
    depths = depth_levels(sv0[..., 2], n_levels, max_jump)
    levels = []
    for l in range(n_levels):
        Kl, shape = pyramid_intrinsics(K, l), pyramid_shape(H, W, l)
        _, vertex, normal = RC.raycast(vol, np.asarray(guess_row).reshape(1, 12), Kl, shape, min_weight=min_weight)
        levels.append({"src_vertex": sv0 if l == 0 else unproject(depths[l], Kl), "src_normal": None, "model_vertex": vertex[0],
                       "model_normal": normal[0], "K": Kl})
    return levels
