#!/usr/bin/env python3
"""RANSAC plane segmentation (r3d_segment_plane), one process, one JSON line per cloud and hypothesis count:
  (a) C3's 500k target: uniform in a 20 m cube (seed 0);
  (b) 20 fused synthetic.room_views frames at 384x1280 (9.8 M points) plus 1 % uniform outliers in the scene's box;
  (c) (b) after voxel_down_sample at 0.02;
  (d) the hot cluster: 100k copies of one point plus 20k uniform background points, shuffled
-- the four clouds of tools/outliers_once.py.  Per cloud and H in {256, 1024, 4096}: the hipEvent median of `reps` whole calls
(hypotheses, count, fold, refit, host eigen-solve, mask: the call synchronises twice) after two warm-ups, H n pair evaluations per
second, and the fp32 rate at 10 flop per pair against 157.3 TFLOP/s.  Beside it, measured in the same process: the brute-force
r3d_icp_nn with four sources per lane (nn_kernel<4>) on 100k x 100k points, in pairs per second at its 8 flop per pair.  CPU leg,
as reported and not optimised against: the same counts in NumPy on one thread for H = 256, timed once on at most 500k points of
the cloud and scaled to its size.
usage: segment_once.py [reps] [out.json]   (default out: profiles/segment_lines.json)"""
import importlib
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
r3d = importlib.import_module("3d_reconstruction_system_amd")
L = importlib.import_module("3d_reconstruction_system_amd._lib")
SEG = importlib.import_module("3d_reconstruction_system_amd.segmentation")
S = importlib.import_module("3d_reconstruction_system_amd.synthetic")
reps = int(sys.argv[1]) if len(sys.argv) > 1 else 20
out_path = sys.argv[2] if len(sys.argv) > 2 else os.path.join(ROOT, "profiles", "segment_lines.json")
PEAK = 157.3e12
THR = 0.01
ctx = r3d.Context(0)


def timed(fn):
    ts = []
    for k in range(reps + 2):
        ctx.sync()
        ctx.timer_start()
        fn()
        t = ctx.timer_stop()
        if k >= 2:
            ts.append(t)
    return float(np.median(ts))


def nn4_pairs_per_s(n=100_000):
    rng = np.random.default_rng(7)
    src, tgt = ((rng.random((n, 3)) * 20).astype(np.float32) for _ in range(2))
    d_src, d_tgt = ctx.alloc(src.nbytes).upload(src), ctx.alloc(tgt.nbytes).upload(tgt)
    d_idx, d_d2 = ctx.alloc(n * 4), ctx.alloc(n * 4)
    ctx.set_tuning("nn_variant", 4)
    ms = timed(lambda: L.check(ctx.lib.r3d_icp_nn(ctx.handle, d_src.ptr, n, d_tgt.ptr, n, d_idx.ptr, d_d2.ptr)))
    ctx.set_tuning("nn_variant", 0)
    for b in (d_src, d_tgt, d_idx, d_d2):
        b.free()
    return n * n / (ms * 1e-3)


def cpu_counts_seconds(xyz, H=256):
    """The count of H hypotheses against the cloud in NumPy (one thread), on at most 500k points, scaled to the cloud."""
    sub = xyz[:500_000]
    rng = np.random.default_rng(0)
    rows = rng.integers(0, sub.shape[0], (H, 3))
    a, b, c = (sub[rows[:, j]].astype(np.float64) for j in range(3))
    nrm = np.cross(b - a, c - a)
    with np.errstate(all="ignore"):
        nrm = (nrm / np.linalg.norm(nrm, axis=1)[:, None]).astype(np.float32)
    anchor = sub[rows[:, 0]]
    t = time.perf_counter()
    for h in range(H):
        e = sub - anchor[h]
        s = (nrm[h, 0] * e[:, 0] + nrm[h, 1] * e[:, 1]) + nrm[h, 2] * e[:, 2]
        int((np.abs(s) <= np.float32(THR)).sum())
    return (time.perf_counter() - t) * xyz.shape[0] / sub.shape[0]


def measure(name, xyz, nn_rate):
    xyz = np.ascontiguousarray(xyz, np.float32)
    n = xyz.shape[0]
    d_xyz, d_mask, d_counts = ctx.alloc(n * 12).upload(xyz), ctx.alloc(n), ctx.alloc(4096 * 4)
    lines = []
    for H in (256, 1024, 4096):
        ms = timed(lambda: SEG.segment_plane_device(ctx, d_xyz.ptr, n, THR, H, 0, d_mask.ptr, d_counts.ptr))
        p = SEG.segment_plane_device(ctx, d_xyz.ptr, n, THR, H, 0, d_mask.ptr, d_counts.ptr)
        rate = H * n / (ms * 1e-3)
        line = {"cloud": name, "points": n, "hypotheses": H, "reps": reps, "segment_plane_ms": round(ms, 4),
                "pairs_per_s": round(rate, 1), "fp32_frac_at_10_flop": round(rate * 10 / PEAK, 4),
                "nn_kernel4_pairs_per_s": round(nn_rate, 1), "rate_over_nn_kernel4": round(rate / nn_rate, 4),
                "best_count": p.best_count, "n_valid": p.n_valid, "inliers": p.n_inliers, "plane": [float(v) for v in p.plane]}
        if H == 256:
            line["cpu_numpy_1thread_counts_s"] = round(cpu_counts_seconds(xyz), 3)
        print(json.dumps(line), flush=True)
        lines.append(line)
    for b in (d_xyz, d_mask, d_counts):
        b.free()
    return lines


def room_with_outliers():
    depth, q, t, K = S.room_views(20, 384, 1280, seed=0)
    xyz = r3d.fuse_frames(depth, q, t, intrinsics=K, ctx=ctx)
    xyz = xyz[np.isfinite(xyz).all(axis=1)]
    rng = np.random.default_rng(1)
    lo, hi = xyz.min(axis=0), xyz.max(axis=0)
    noise = (lo + rng.random((xyz.shape[0] // 100, 3)) * (hi - lo)).astype(np.float32)
    return np.concatenate([xyz, noise])


nn_rate = nn4_pairs_per_s()
lines = []
rng = np.random.default_rng(0)
lines += measure("a_c3_500k_uniform", (rng.random((500000, 3)) * 20).astype(np.float32), nn_rate)
room = room_with_outliers()
lines += measure("b_room_20x384x1280_plus_1pct", room, nn_rate)
lines += measure("c_room_voxel_0.02", r3d.voxel_down_sample(room, 0.02, ctx=ctx).xyz, nn_rate)
del room
rng = np.random.default_rng(7)
hot = np.concatenate([np.tile(np.float32([[0.25, 0.5, 0.75]]), (100000, 1)), rng.random((20000, 3)).astype(np.float32)])
lines += measure("d_hot_100k_copies_20k_background", hot[rng.permutation(hot.shape[0])], nn_rate)
os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
with open(out_path, "w") as f:
    for line in lines:
        f.write(json.dumps(line) + "\n")
