#!/usr/bin/env python3
"""The mesh smoothing entry points (r3d_mesh_adjacency, r3d_mesh_smooth, r3d_mesh_vertex_normals) timed on the mesh of a 256^3
volume, one process, one JSON line: a sphere of radius 100 voxels written straight into the volume (tsdf = distance - radius, all
weights 1), extracted on the device, so the vertices come in marching-cubes (voxel-linear) order.  Three legs, alternating run by
run: `adjacency` (the build with room for every neighbour; it synchronises twice per call), `step` (one umbrella step: a call with one
factor) and `normals`.  One timed window is CALLS back-to-back device calls between two HIP events; the figure is the median window of
`reps` after two warm-ups, divided by CALLS.  Next to it, from shapes and not measured: the minimum bytes and the share of the HBM
rate they amount to at the measured time -- adjacency: the triangles read once, row_start, neighbours and flags written once (its
sort passes come on top); step: per vertex 12 B own + 4 B row_start + degree x (4 B index + 12 B gather) + 12 B store; normals:
positions and triangles read once, normals written once.  A record, not a gate.
usage: mesh_smooth_once.py [reps] [out.json]"""
import importlib
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
r3d = importlib.import_module("3d_reconstruction_system_amd")
M = importlib.import_module("3d_reconstruction_system_amd.mesh")
L = importlib.import_module("3d_reconstruction_system_amd._lib")

HBM_SPEC, HBM_COPY = 8.0e12, 6.29e12   # bytes per second: the data sheet's rate and the measured float4 copy
CALLS = 10
DIM, RADIUS = 256, 100.0
reps = int(sys.argv[1]) if len(sys.argv) > 1 else 9
out_path = sys.argv[2] if len(sys.argv) > 2 else None

ctx = r3d.Context(0)
vol = r3d.TSDFVolume((0.0, 0.0, 0.0), 1.0, (DIM, DIM, DIM), 3.0, ctx=ctx)
c = np.arange(DIM, dtype=np.float32) + np.float32(0.5 - DIM / 2)
dist = np.sqrt(c[None, None, :] ** 2 + c[None, :, None] ** 2 + c[:, None, None] ** 2) - np.float32(RADIUS)
raw = np.ascontiguousarray(np.stack([dist.reshape(-1), np.ones(DIM ** 3, np.float32)], axis=1), dtype=np.float32)
p, n_voxels = vol.device_view()
assert raw.shape == (n_voxels, 2)
L.check(ctx.lib.r3d_memcpy_h2d(ctx.handle, p, raw.ctypes.data, raw.nbytes))
ctx.sync()
nv, nt = vol.extract_mesh_device(1.0, None, None, 0, None, 0)
d_xyz, d_nrm, d_tri = ctx.alloc(nv * 12), ctx.alloc(nv * 12), ctx.alloc(nt * 12)
assert vol.extract_mesh_device(1.0, d_xyz.ptr, d_nrm.ptr, nv, d_tri.ptr, nt) == (nv, nt)
d_rs, d_nb, d_bd, e = M.adjacency_buffers(ctx, d_tri.ptr, nt, nv, ctx.buffers())
d_out, d_n = ctx.alloc(nv * 12), ctx.alloc(nv * 12)


def adjacency():
    M.mesh_adjacency_device(ctx, d_tri.ptr, nt, nv, d_rs.ptr, d_nb.ptr, e, d_bd.ptr)


def step():
    M.smooth_mesh_device(ctx, d_xyz.ptr, d_out.ptr, nv, d_rs.ptr, d_nb.ptr, None, [0.5])


def normals():
    M.vertex_normals_device(ctx, d_out.ptr, nv, d_tri.ptr, nt, d_nrm.ptr, d_n.ptr)


legs = {"adjacency": adjacency, "step": step, "normals": normals}
min_bytes = {"adjacency": nt * 12 + (nv + 1) * 4 + e * 4 + nv, "step": nv * (12 + 4 + 12) + e * (4 + 12), "normals": nv * 12 + nt * 12 + nv * 12}
times = {name: [] for name in legs}
for k in range(reps + 2):
    for name, call in legs.items():
        ctx.timer_start()
        for _ in range(CALLS):
            call()
        ms = ctx.timer_stop() / CALLS
        if k >= 2:
            times[name].append(ms)
result = {"workload": "mesh_smooth", "volume": [DIM] * 3, "vertices": nv, "triangles": nt, "neighbour_entries": e,
          "boundary_vertices": int(np.count_nonzero(d_bd.download(np.uint8, nv))), "calls_per_window": CALLS, "reps": reps}
for name in legs:
    med = float(np.median(times[name]))
    result[name] = {"ms_median": round(med, 4), "ms_min": round(min(times[name]), 4), "ms_max": round(max(times[name]), 4),
                    "min_bytes": min_bytes[name], "share_of_8.0TBps": round(min_bytes[name] / (med * 1e-3) / HBM_SPEC, 4),
                    "share_of_6.29TBps_copy": round(min_bytes[name] / (med * 1e-3) / HBM_COPY, 4)}
line = json.dumps(result)
print(line)
if out_path:
    with open(out_path, "w") as f:
        f.write(line + "\n")
ctx.close()
