#!/usr/bin/env python3
"""The depth consistency filter (r3d_depth_consistency) timed at the workload's own shape, one process, one JSON line:
100 synthetic.room_views frames at 384x1280, quantised to uint8 at 1/32 m (BASELINE config 2's batch), in HBM; radius 2 (four
sources), rel_tol 0.03, min_consistent 2, max_violations 0.  Two legs, alternating run by run: `all` writes votes, keep and filtered,
`keep` the mask alone.  One timed window is CALLS back-to-back device calls between two HIP events (a call includes the host's
relative poses and their upload); the figure is the median window of `reps` after two warm-ups, divided by CALLS.  Next to it,
from shapes and not measured: the minimum bytes (each raster read once, each requested output written once) and the share of the
HBM rate they amount to at the measured time.  A record, not a gate.
usage: consistency_once.py [reps] [out.json]"""
import importlib
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
r3d = importlib.import_module("3d_reconstruction_system_amd")
S = importlib.import_module("3d_reconstruction_system_amd.synthetic")

HBM_SPEC, HBM_COPY = 8.0e12, 6.29e12   # bytes per second: the data sheet's rate and the measured float4 copy
CALLS = 10
F, H, W = 100, 384, 1280
reps = int(sys.argv[1]) if len(sys.argv) > 1 else 9
out_path = sys.argv[2] if len(sys.argv) > 2 else None

z, q, t, K = S.room_views(F, H, W)
depth = np.clip(np.rint(z * 32.0), 0, 255).astype(np.uint8)
poses, src = r3d.poses_w2c(q, t), r3d.window_sources(F, 2)
n = F * H * W
ctx = r3d.Context(0)
cam = ctx.camera(H, W, *K)
d_depth, d_votes, d_keep, d_filtered = ctx.alloc(n).upload(depth), ctx.alloc(2 * n), ctx.alloc(n), ctx.alloc(4 * n)
legs = {"all": dict(d_votes=d_votes.ptr, d_keep=d_keep.ptr, d_filtered=d_filtered.ptr), "keep": dict(d_keep=d_keep.ptr)}
min_bytes = {"all": n * (1 + 2 + 1 + 4), "keep": n * (1 + 1)}
times = {name: [] for name in legs}
for k in range(reps + 2):
    for name, outs in legs.items():
        ctx.timer_start()
        for _ in range(CALLS):
            r3d.depth_consistency_device(ctx, cam, d_depth.ptr, np.uint8, F, poses, src, rel_tol=0.03, depth_scale=1.0 / 32.0, **outs)
        ms = ctx.timer_stop() / CALLS
        if k >= 2:
            times[name].append(ms)
keep = d_keep.download(np.uint8, n)
result = {"workload": "depth_consistency", "frames": F, "height": H, "width": W, "dtype": "uint8", "sources": int(src.shape[1]),
          "calls_per_window": CALLS, "reps": reps, "kept_share": round(float(keep.mean()), 4)}
for name in legs:
    med = float(np.median(times[name]))
    result[name] = {"ms_median": round(med, 4), "ms_min": round(min(times[name]), 4), "ms_max": round(max(times[name]), 4),
                    "min_bytes": min_bytes[name], "share_of_8.0TBps": round(min_bytes[name] / (med * 1e-3) / HBM_SPEC, 3),
                    "share_of_6.29TBps_copy": round(min_bytes[name] / (med * 1e-3) / HBM_COPY, 3)}
line = json.dumps(result)
print(line)
if out_path:
    with open(out_path, "w") as f:
        f.write(line + "\n")
ctx.close()
