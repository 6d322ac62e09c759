#!/usr/bin/env python3
"""r3d_tsdf_integrate_cloud timed once, one process, one JSON line: a synthetic room cloud of 1 M points (uniform over the six faces
of a 4.8 x 2.8 x 4.8 m box, the normals pointing into the room) into a 256^3 volume of 2 cm voxels, truncation 4 voxels.  Two legs,
alternating run by run: `device` (the index over the cloud is built once outside the window; one timed window is CALLS back-to-back
calls between two HIP events, divided by CALLS -- every call sizes its band with one 4-byte read-back, so the window includes that
wait) and `host` (r3d_tsdf_integrate_cloud_host: upload, index build, integration, index destroy; a host clock around the
synchronous call).  The figure is the median of `reps` windows after two warm-ups.  Next to it: the voxels one call updates and their
share of the volume (the band the work is limited to is a superset of them, in blocks of 4 x 4 x 4 voxels).  A record, not a gate.
usage: cloud_tsdf_once.py [reps] [out.json]"""
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

CALLS = 3
DIM, VS, TRUNC_VOXELS, POINTS = 256, 0.02, 4, 1000000
HALF = np.array([2.4, 1.4, 2.4])
reps = int(sys.argv[1]) if len(sys.argv) > 1 else 5
out_path = sys.argv[2] if len(sys.argv) > 2 else None


def room_cloud(n, seed=0):
    """(xyz, normals) float32: n points uniform over the faces of the box |x| <= 2.4, |y| <= 1.4, |z| <= 2.4, normals inwards"""
    rng = np.random.default_rng(seed)
    area = np.array([HALF[1] * HALF[2], HALF[0] * HALF[2], HALF[0] * HALF[1]])
    axis = rng.choice(3, size=n, p=area / area.sum())
    side = rng.integers(0, 2, n) * 2 - 1
    xyz = rng.uniform(-1.0, 1.0, (n, 3)) * HALF
    rows = np.arange(n)
    xyz[rows, axis] = side * HALF[axis]
    normals = np.zeros((n, 3))
    normals[rows, axis] = -side
    return xyz.astype(np.float32), normals.astype(np.float32)


xyz, normals = room_cloud(POINTS)
ctx = r3d.Context(0)
vol = r3d.TSDFVolume((-0.5 * DIM * VS,) * 3, VS, (DIM,) * 3, TRUNC_VOXELS * VS, ctx=ctx)
d_xyz, d_nrm = ctx.alloc(xyz.nbytes).upload(xyz), ctx.alloc(normals.nbytes).upload(normals)
index = icp.NNIndex(ctx, d_xyz.ptr, POINTS)
touched = vol.integrate_cloud_device(index, d_nrm.ptr, want_count=True)
times = {"device": [], "host": []}
for k in range(reps + 2):
    ctx.timer_start()
    for _ in range(CALLS):
        vol.integrate_cloud_device(index, d_nrm.ptr)
    ms = ctx.timer_stop() / CALLS
    t0 = time.perf_counter()
    assert vol.integrate_cloud(xyz, normals) == touched
    host_ms = (time.perf_counter() - t0) * 1e3
    if k >= 2:
        times["device"].append(ms)
        times["host"].append(host_ms)
result = {"workload": "cloud_tsdf", "points": POINTS, "volume": [DIM] * 3, "voxel_size": VS, "trunc_voxels": TRUNC_VOXELS,
          "voxels_touched": touched, "touched_share_of_volume": round(touched / DIM ** 3, 4), "calls_per_window": CALLS, "reps": reps}
for name, t in times.items():
    result[name] = {"ms_median": round(float(np.median(t)), 3), "ms_min": round(min(t), 3), "ms_max": round(max(t), 3)}
line = json.dumps(result)
print(line)
if out_path:
    with open(out_path, "w") as f:
        f.write(line + "\n")
index.close()
vol.close()
ctx.close()
