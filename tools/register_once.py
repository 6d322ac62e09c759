#!/usr/bin/env python3
"""Global registration (r3d_fpfh_knn, r3d_feature_match, r3d_register_ransac, registration.register_global), one process, one
JSON line per size.  The scene is tests/register_ref.py's cluttered room in two overlapping parts, sampled so that each part
has about 10 k and about 50 k points after downsampling (voxel 0.1 and 0.045).  Per size, hipEvent medians of `reps` whole calls
after two warm-ups:
  fpfh    r3d_fpfh_knn on the downsampled source (k = 32, radius 5 voxels): the k-NN lists, the SPFH and the FPFH launch
  match   r3d_feature_match, mutual, with the compaction (synchronises); the feature sets alternate between two copies in HBM so
          that no call finds the other call's rows in the L2; beside it the fraction of the f32 vector peak (157.3 TFLOP/s) at
          the specified 99 operations per pair of rows and direction
  ransac  r3d_register_ransac, 65536 hypotheses, one seed
  whole   registration.register_global from host arrays (wall clock: uploads, downsampling, normals, four RANSAC rounds)
and, at the small size only, the NumPy restatement of the three stages on one thread, timed once.
usage: register_once.py [reps] [out.json]   (default out: profiles/register_lines.json)"""
import importlib
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import register_ref as REF  # noqa: E402

r3d = importlib.import_module("3d_reconstruction_system_amd")
L = importlib.import_module("3d_reconstruction_system_amd._lib")
G = importlib.import_module("3d_reconstruction_system_amd.registration")
ICP = importlib.import_module("3d_reconstruction_system_amd.icp")
NRM = importlib.import_module("3d_reconstruction_system_amd.normals")
reps = int(sys.argv[1]) if len(sys.argv) > 1 else 10
out_path = sys.argv[2] if len(sys.argv) > 2 else os.path.join(ROOT, "profiles", "register_lines.json")
PEAK, K, H = 157.3e12, 32, 65536
ctx = r3d.Context(0)


def timed(fn):
    ts = []
    for k in range(reps + 2):
        ctx.sync()
        ctx.timer_start()
        fn(k)
        t = ctx.timer_stop()
        if k >= 2:
            ts.append(t)
    return float(np.median(ts))


def features(xyz, view, voxel):
    """(downsampled cloud, normals, fpfh, fpfh ms)"""
    d = np.ascontiguousarray(r3d.voxel_down_sample(xyz, voxel, ctx=ctx).xyz, np.float32)
    n = d.shape[0]
    nrm = NRM.estimate_normals(d, K, radius=5 * voxel, viewpoint=view, ctx=ctx).normals
    d_xyz, d_n, d_f = ctx.alloc(n * 12).upload(d), ctx.alloc(n * 12).upload(nrm), ctx.alloc(n * 132)
    index = ICP.NNIndex(ctx, d_xyz.ptr, n)
    ms = timed(lambda k: G.compute_fpfh_device(index, K, d_n.ptr, d_f.ptr, radius=5 * voxel))
    f = d_f.download(np.float32, n * 33).reshape(n, 33)
    index.close()
    for b in (d_xyz, d_n, d_f):
        b.free()
    return d, nrm, f, ms


def measure(name, step, voxel, cpu_leg):
    P = REF.cluttered_room(0, step)
    s = REF.room_pair(0)
    Ti = np.linalg.inv(s["T"])
    tgt = P[P[:, 0] < 1.0].astype(np.float32)
    src = (P[P[:, 0] > -1.5] @ Ti[:3, :3].T + Ti[:3, 3]).astype(np.float32)
    a, na_nrm, fa, fpfh_ms = features(src, s["src_view"], voxel)
    b, nb_nrm, fb, _ = features(tgt, s["tgt_view"], voxel)
    na, nb = fa.shape[0], fb.shape[0]
    copies = [(ctx.alloc(fa.nbytes).upload(fa), ctx.alloc(fb.nbytes).upload(fb)) for _ in range(2)]
    d_idx, d_dist, d_corr = ctx.alloc(na * 4), ctx.alloc(na * 4), ctx.alloc(na * 8)
    match_ms = timed(lambda k: G.match_features_device(ctx, copies[k & 1][0].ptr, na, copies[k & 1][1].ptr, nb, d_idx.ptr, d_dist.ptr,
                                                       d_corr.ptr, True))
    m = G.match_features_device(ctx, copies[0][0].ptr, na, copies[0][1].ptr, nb, d_idx.ptr, d_dist.ptr, d_corr.ptr, True)
    d_a, d_b, d_in = ctx.alloc(a.nbytes).upload(a), ctx.alloc(b.nbytes).upload(b), ctx.alloc(max(m, 16))
    thr = 1.5 * voxel
    ransac_ms = timed(lambda k: G.registration_ransac_device(ctx, d_a.ptr, na, d_b.ptr, nb, d_corr.ptr, m, thr, H, 0, d_in.ptr))
    res = G.registration_ransac_device(ctx, d_a.ptr, na, d_b.ptr, nb, d_corr.ptr, m, thr, H, 0, d_in.ptr)
    for buf in [d_idx, d_dist, d_corr, d_a, d_b, d_in] + [x for c in copies for x in c]:
        buf.free()
    whole = []
    for k in range(3):
        t = time.perf_counter()
        T, info = G.register_global(src, tgt, voxel, src_viewpoint=s["src_view"], tgt_viewpoint=s["tgt_view"], ctx=ctx)
        whole.append(time.perf_counter() - t)
    full = src.astype(np.float64)
    err = float(np.linalg.norm((full @ T[:3, :3].T + T[:3, 3]) - (full @ s["T"][:3, :3].T + s["T"][:3, 3]), axis=1).max())
    ops = 2.0 * na * nb * 99
    line = {"size": name, "source_points": int(src.shape[0]), "target_points": int(tgt.shape[0]), "source_down": na, "target_down": nb,
            "voxel": voxel, "reps": reps, "fpfh_ms": round(fpfh_ms, 4), "match_mutual_ms": round(match_ms, 4),
            "match_f32_frac_at_99_ops": round(ops / (match_ms * 1e-3) / PEAK, 4), "correspondences": int(m),
            "ransac_65536_ms": round(ransac_ms, 4), "ransac_inliers": int(res[22]),
            "register_global_wall_s_median_of_3": round(float(np.median(whole)), 4), "worst_point_error": round(err, 5),
            "distance_threshold": thr}
    if cpu_leg:
        t = time.perf_counter()
        host = REF.downsample_normals_lists(src, voxel, s["src_view"], K, 5 * voxel)   # the restatement's input: cloud, normals, lists
        t_lists = time.perf_counter() - t
        t = time.perf_counter()
        REF.fpfh(*host, radius=5 * voxel)
        line["cpu_numpy_1thread_fpfh_s"] = round(time.perf_counter() - t, 3)
        t = time.perf_counter()
        corr = REF.match(fa, fb, mutual=True)[0]
        line["cpu_numpy_1thread_match_s"] = round(time.perf_counter() - t, 3)
        t = time.perf_counter()
        REF.ransac(a, b, corr, thr, H, 0)
        line["cpu_numpy_1thread_ransac_s"] = round(time.perf_counter() - t, 3)
        line["cpu_lists_s_not_part_of_the_restatement"] = round(t_lists, 3)
    print(json.dumps(line), flush=True)
    return line


lines = [measure("10k", 0.05, 0.1, True), measure("50k", 0.022, 0.045, False)]
os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
with open(out_path, "w") as f:
    for line in lines:
        f.write(json.dumps(line) + "\n")
