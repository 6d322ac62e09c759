#!/usr/bin/env python3
"""k-NN of an index's own points and the two outlier filters (r3d_nn_index_knn_self, r3d_outlier_statistical,
r3d_outlier_radius, r3d_select_rows), one process, one JSON line per cloud:
  (a) C3's 500k target: uniform in a 20 m cube (tools/nn_probe.py, seed 0);
  (b) 20 fused synthetic.room_views frames at 384x1280 (9.8 M points) plus 1 % uniform outliers in the scene's box;
  (c) (b) after voxel_down_sample at 0.02;
  (d) the hot cluster: 100k copies of one point plus 20k uniform background points, shuffled.
Per cloud, hipEvent medians of `reps` runs after two warm-ups: index build, knn_self at k = 20, SOR (20, 2.0), ROR (16, 0.05),
select_rows of SOR's mask; pair evaluations per point of each search (32-target groups x 32 x 64 lanes / n) and the fp32 rate
at 8 flop per pair against 157.3 TFLOP/s.  CPU leg, as reported and not optimised against: scipy cKDTree(xyz) built and
queried with k=21, workers=1, once.
usage: outliers_once.py [reps] [out.json]"""
import importlib
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
r3d = importlib.import_module("3d_reconstruction_system_amd")
icp = importlib.import_module("3d_reconstruction_system_amd.icp")
O = importlib.import_module("3d_reconstruction_system_amd.outliers")
S = importlib.import_module("3d_reconstruction_system_amd.synthetic")
reps = int(sys.argv[1]) if len(sys.argv) > 1 else 20
out_path = sys.argv[2] if len(sys.argv) > 2 else None
PEAK = 157.3e12
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
    return round(float(np.median(ts)), 4)


def measure(name, xyz):
    xyz = np.ascontiguousarray(xyz, np.float32)
    n = xyz.shape[0]
    d_xyz = ctx.alloc(n * 12).upload(xyz)
    ix = icp.NNIndex(ctx, d_xyz.ptr, n)
    d_idx, d_d2 = ctx.alloc(n * 20 * 4), ctx.alloc(n * 20 * 4)
    d_keep, d_score, d_cnt = ctx.alloc(n), ctx.alloc(n * 8), ctx.alloc(n * 4)
    d_out, d_rows = ctx.alloc(n * 12), ctx.alloc(n * 4)
    line = {"cloud": name, "points": n, "reps": reps}
    line["index_build_ms"] = timed(lambda: ix.rebuild(d_xyz.ptr, n))
    runs = {"knn20": lambda: ix.knn_self(20, d_idx.ptr, d_d2.ptr),
            "sor_20_2": lambda: O.statistical_outlier_device(ix, 20, 2.0, d_keep.ptr, d_score.ptr),
            "ror_16_005": lambda: O.radius_outlier_device(ix, 16, 0.05, d_keep.ptr, d_cnt.ptr)}
    for key, fn in runs.items():
        ms = timed(fn)
        pairs = ix.knn_pairs()
        line[key + "_ms"] = ms
        line[key + "_pairs_per_point"] = round(pairs / n, 1)
        line[key + "_fp32_frac"] = round(pairs * 8 / (ms * 1e-3) / PEAK, 4)
    kept, stats = O.statistical_outlier_device(ix, 20, 2.0, d_keep.ptr, d_score.ptr)
    line["sor_kept"] = kept
    line["sor_stats"] = [stats.V, stats.mu, stats.sigma, stats.T]
    line["ror_kept"] = O.radius_outlier_device(ix, 16, 0.05, d_keep.ptr, d_cnt.ptr)
    O.statistical_outlier_device(ix, 20, 2.0, d_keep.ptr, d_score.ptr)
    line["select_rows_ms"] = timed(lambda: O.select_rows_device(ctx, d_xyz.ptr, n, d_keep.ptr, d_out.ptr, d_rows.ptr))
    for b in (d_idx, d_d2, d_keep, d_score, d_cnt, d_out, d_rows):
        b.free()
    ix.close()
    d_xyz.free()
    from scipy.spatial import cKDTree
    t = time.perf_counter()
    cKDTree(xyz).query(xyz, k=21, workers=1)
    line["cpu_ckdtree_build_query_k21_workers1_s"] = round(time.perf_counter() - t, 3)
    print(json.dumps(line), flush=True)
    return line


def room_with_outliers():
    depth, q, t, K = S.room_views(20, 384, 1280, seed=0)
    xyz = r3d.fuse_frames(depth, q, t, intrinsics=K, ctx=ctx)
    xyz = xyz[np.isfinite(xyz).all(axis=1)]
    rng = np.random.default_rng(1)
    lo, hi = xyz.min(axis=0), xyz.max(axis=0)
    noise = (lo + rng.random((xyz.shape[0] // 100, 3)) * (hi - lo)).astype(np.float32)
    return np.concatenate([xyz, noise])


lines = []
rng = np.random.default_rng(0)
lines.append(measure("a_c3_500k_uniform", (rng.random((500000, 3)) * 20).astype(np.float32)))
room = room_with_outliers()
lines.append(measure("b_room_20x384x1280_plus_1pct", room))
lines.append(measure("c_room_voxel_0.02", r3d.voxel_down_sample(room, 0.02, ctx=ctx).xyz))
del room
rng = np.random.default_rng(7)
hot = np.concatenate([np.tile(np.float32([[0.25, 0.5, 0.75]]), (100000, 1)), rng.random((20000, 3)).astype(np.float32)])
lines.append(measure("d_hot_100k_copies_20k_background", hot[rng.permutation(hot.shape[0])]))
if out_path:
    with open(out_path, "w") as f:
        for line in lines:
            f.write(json.dumps(line) + "\n")
