#!/usr/bin/env python3
"""Voxel-grid downsampling (r3d_voxelgrid) against the occupied-voxel set (r3d_voxelset) on the same clouds, one process:
  (a) surfaces: tools/voxel_path_crossover.py's 100 frames of slanted planes (49 M points), res 0.1;
  (b) C2's synthetic fused cloud (100 x 384 x 1280 random u8 depth, seed 1234): nearly every point its own voxel;
  (c) hot points: 4 M points in 16 voxels plus 300 k uniform background points, shuffled.
Per cloud, medians of `reps` hipEvent-timed repetitions after two warm-ups: grid insert, grid insert + extract into device
buffers (with and without colour), set insert, set insert + codes() (sorted codes to the host).  One JSON line per cloud.
usage: voxel_downsample_once.py [reps] [out.json]"""
import importlib
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
r3d = importlib.import_module("3d_reconstruction_system_amd")
V = importlib.import_module("3d_reconstruction_system_amd.voxelmap")
reps = int(sys.argv[1]) if len(sys.argv) > 1 else 20
out_path = sys.argv[2] if len(sys.argv) > 2 else None
HBM = 8e12
ctx = r3d.Context(0)


def fused(depth, tab, K):
    F, H, W = depth.shape
    n = F * H * W
    cam = ctx.camera(H, W, *K)
    d_pose, d_depth, d_xyz = ctx.alloc(tab.nbytes).upload(tab), ctx.alloc(depth.nbytes).upload(depth), ctx.alloc(n * 12)
    r3d.fuse_frames_device(ctx, cam, d_depth.ptr, depth.dtype.type, F, d_pose.ptr, d_xyz.ptr, np.float32)
    d_pose.free()
    d_depth.free()
    return d_xyz, n


def timed(fn, reps):
    ts = []
    for k in range(reps + 2):
        ctx.sync()
        ctx.timer_start()
        fn()
        t = ctx.timer_stop()
        if k >= 2:
            ts.append(t)
    return float(np.median(ts)), float(np.min(ts))


def measure(name, d_xyz, n, res):
    rng = np.random.default_rng(1)
    d_rgba = ctx.alloc(n * 4).upload(rng.integers(0, 1 << 24, size=n, dtype=np.uint32))
    cap = 1 << int(np.ceil(np.log2(2 * n)))
    line = {"cloud": name, "points": n, "res": res, "table_slots": cap, "reps": reps}
    for colour in (False, True):
        vg = V.VoxelGrid(res, cap, colour, ctx)
        rgba = d_rgba.ptr if colour else None
        vg.insert_device(d_xyz.ptr, n, rgba)
        m = vg.extract_device()
        bufs = [ctx.alloc(m * b) for b in (12, 4, 4, 8)]
        outs = (bufs[0].ptr, bufs[1].ptr if colour else None, bufs[2].ptr, bufs[3].ptr)

        def ins():
            vg.clear()
            vg.insert_device(d_xyz.ptr, n, rgba)

        def ins_ext():
            ins()
            vg.extract_device(*outs, cap=m)
        t_clear = timed(vg.clear, reps)[0]
        t_ins = timed(ins, reps)[0] - t_clear
        t_all = timed(ins_ext, reps)[0] - t_clear
        key = "grid_rgb" if colour else "grid"
        read = n * (16 if colour else 12)
        written = m * (28 if colour else 24)
        line.update({"voxels": m, key + "_insert_ms": round(t_ins, 4), key + "_insert_extract_ms": round(t_all, 4),
                     key + "_algorithmic_bytes": read + written,
                     key + "_hbm_frac": round((read + written) / (t_all * 1e-3) / HBM, 4)})
        if not colour:
            # the insert's global atomics when no two points of a workgroup run share a voxel: one CAS + 4 adds per voxel entry
            line["grid_global_atomics_if_no_lds_merge"] = 5 * n
        for b in bufs:
            b.free()
        vg.close()
    vs = V.VoxelSet(res, cap, ctx)

    def s_ins():
        vs.clear()
        vs.insert_device(d_xyz.ptr, n)

    def s_all():
        s_ins()
        vs.codes()
    t_clear = timed(vs.clear, reps)[0]
    line["set_insert_ms"] = round(timed(s_ins, reps)[0] - t_clear, 4)
    line["set_insert_codes_ms"] = round(timed(s_all, reps)[0] - t_clear, 4)
    line["set_voxels"] = vs.stats()["voxels"]
    vs.close()
    line["grid_over_set_insert"] = round(line["grid_insert_ms"] / line["set_insert_ms"], 3)
    d_rgba.free()
    print(json.dumps(line), flush=True)
    return line


lines = []
rng = np.random.default_rng(7)
F, H, W = 100, 384, 1280
tab = r3d.pose_table(rng.normal(size=(F, 4)), rng.normal(size=(F, 3)))
yy, xx = np.mgrid[0:H, 0:W]
depth = np.stack([np.clip(40 + (xx // 8 + yy // 6 + 3 * f) % 200, 1, 255) for f in range(F)]).astype(np.uint8)
d_xyz, n = fused(depth, tab, r3d.REF_INTRINSICS)
lines.append(measure("a_surfaces_49M", d_xyz, n, 0.1))
d_xyz.free()

rng = np.random.default_rng(1234)
depth = rng.integers(1, 256, (F, H, W), dtype=np.uint8)
tab = r3d.pose_table(rng.normal(size=(F, 4)), rng.normal(size=(F, 3)) * 10)
d_xyz, n = fused(depth, tab, r3d.REF_INTRINSICS)
lines.append(measure("b_c2_random_49M", d_xyz, n, 0.1))
d_xyz.free()

rng = np.random.default_rng(5)
centres = np.floor(rng.uniform(-20, 20, size=(16, 3)) / 0.1) * 0.1
hot = centres[rng.integers(0, 16, size=4_000_000)] + rng.uniform(0.001, 0.099, size=(4_000_000, 3))
xyz = np.concatenate([hot, rng.uniform(-50, 50, size=(300_000, 3))]).astype(np.float32)
xyz = xyz[rng.permutation(len(xyz))]
d_xyz = ctx.alloc(xyz.nbytes).upload(xyz)
lines.append(measure("c_hot_16_voxels", d_xyz, len(xyz), 0.1))
d_xyz.free()
ctx.close()
if out_path:
    with open(out_path, "w") as f:
        for line in lines:
            f.write(json.dumps(line) + "\n")
