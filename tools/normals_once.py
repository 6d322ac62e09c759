#!/usr/bin/env python3
"""Normals of an unorganised cloud (r3d_normals_knn) next to the search it is fused behind (r3d_nn_index_knn_self at the same k
on the same index), one process, one JSON line per cloud:
  (a) C3's 500k target: uniform in a 20 m cube (tools/nn_probe.py, seed 0);
  (b) 20 fused synthetic.room_views frames at 384x1280 (9.8 M points) plus 1 % uniform outliers in the scene's box;
  (c) (b) after voxel_down_sample at 0.02;
  (d) the hot cluster: 100k copies of one point plus 20k uniform background points, shuffled.
Per cloud and k in (8, 20, 32): hipEvent medians of `reps` runs after two warm-ups, the two calls alternating run by run;
normals with all four outputs, with the normals alone, and (k = 20) with one viewpoint and with a 0.1 radius.  ratio = normals /
knn_self: an unfused composition runs knn_self and then reads its 8 k bytes per point back.  CPU leg, as reported and not
optimised against: scipy cKDTree(xyz) built and queried with k=21, workers=1, neighbour covariances and numpy.linalg.eigh in
batches, one thread, once.
usage: normals_once.py [reps] [out.json] [cpu: 1|0]"""
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
S = importlib.import_module("3d_reconstruction_system_amd.synthetic")
reps = int(sys.argv[1]) if len(sys.argv) > 1 else 20
out_path = sys.argv[2] if len(sys.argv) > 2 else None
cpu_leg = (sys.argv[3] != "0") if len(sys.argv) > 3 else True
ctx = r3d.Context(0)


def timed_alternating(fns):
    """Medians (ms) of the calls in `fns`, run in turn `reps` times after two warm-up turns."""
    ts = [[] for _ in fns]
    for k in range(reps + 2):
        for i, fn in enumerate(fns):
            ctx.sync()
            ctx.timer_start()
            fn()
            t = ctx.timer_stop()
            if k >= 2:
                ts[i].append(t)
    return [round(float(np.median(t)), 4) for t in ts]


def cpu_normals(xyz):
    from scipy.spatial import cKDTree
    t = time.perf_counter()
    _, nb = cKDTree(xyz).query(xyz, k=21, workers=1)
    t_tree = time.perf_counter() - t
    t = time.perf_counter()
    p = xyz.astype(np.float64)
    for lo in range(0, xyz.shape[0], 1 << 18):
        e = p[nb[lo:lo + (1 << 18)]] - p[lo:lo + (1 << 18), None, :]
        m = e.mean(axis=1, keepdims=True)
        np.linalg.eigh(np.einsum("nka,nkb->nab", e - m, e - m))
    return round(t_tree, 3), round(time.perf_counter() - t, 3)


def measure(name, xyz):
    xyz = np.ascontiguousarray(xyz, np.float32)
    n = xyz.shape[0]
    d_xyz = ctx.alloc(n * 12).upload(xyz)
    ix = icp.NNIndex(ctx, d_xyz.ptr, n)
    d_idx, d_d2 = ctx.alloc(n * 32 * 4), ctx.alloc(n * 32 * 4)
    d_n, d_c, d_cov, d_m = ctx.alloc(n * 12), ctx.alloc(n * 4), ctx.alloc(n * 48), ctx.alloc(n * 4)
    view = np.ascontiguousarray(xyz[np.isfinite(xyz).all(axis=1)].mean(axis=0, dtype=np.float64).reshape(1, 3))
    line = {"cloud": name, "points": n, "reps": reps}
    for k in (8, 20, 32):
        knn, full, lean = timed_alternating([lambda: ix.knn_self(k, d_idx.ptr, d_d2.ptr),
                                             lambda: ix.normals_knn(k, 0.0, None, 1, d_n.ptr, d_c.ptr, d_cov.ptr, d_m.ptr),
                                             lambda: ix.normals_knn(k, 0.0, None, 1, d_n.ptr)])
        line["knn%d_ms" % k], line["normals%d_all_outputs_ms" % k], line["normals%d_ms" % k] = knn, full, lean
        line["normals%d_over_knn" % k] = round(lean / knn, 3)
        line["normals%d_all_outputs_over_knn" % k] = round(full / knn, 3)
    seen, hybrid = timed_alternating([lambda: ix.normals_knn(20, 0.0, view, 1, d_n.ptr),
                                      lambda: ix.normals_knn(20, 0.1, None, 1, d_n.ptr)])
    line["normals20_viewpoint_ms"], line["normals20_radius_0.1_ms"] = seen, hybrid
    ix.normals_knn(20, 0.0, None, 1, d_n.ptr)
    line["without_a_normal"] = int((d_n.download(np.float32, 3 * n).reshape(n, 3) == 0).all(axis=1).sum())
    for b in (d_idx, d_d2, d_n, d_c, d_cov, d_m):
        b.free()
    ix.close()
    d_xyz.free()
    if cpu_leg:
        line["cpu_ckdtree_build_query_k21_workers1_s"], line["cpu_covariance_eigh_k20_s"] = cpu_normals(xyz)
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
