#!/usr/bin/env python3
"""TSDF integration and surface extraction (r3d_tsdf_*), one process, one JSON line per volume:
100 synthetic.room_views frames at 384x1280, quantised to uint8 at 1/32 m (BASELINE config 2's batch), into a 256^3 and a 512^3
volume around the room.  hipEvent medians of `reps` runs after two warm-ups, the legs alternating run by run, the volume reset
outside the timed window before every run:
  batched      one r3d_tsdf_integrate call of all frames (the frame loop inside the kernel, R3D_TSDF_CHUNK frames per launch);
  per_frame    the same kernel launched one frame at a time (one call per frame);
  extract      r3d_tsdf_extract_points (count + scan + emit, with normals) of the integrated volume;
  mesh         r3d_tsdf_extract_mesh (count + scan + vertices + triangles) of the same volume, alternating with extract;
  rgb          a second volume with the colour plane: one r3d_tsdf_integrate_rgb call of all frames (seeded noise images in HBM),
               alternating with the depth-only batched call on the first volume, both volumes reset outside the window;
  colors       r3d_tsdf_extract_colors of the integrated colour volume, alternating with r3d_tsdf_extract_points on it.
Roofs are printed from shapes, not measured: algorithmic bytes of the batched form (16 B per voxel and launch + the rasters once)
against 8 TB/s, and voxel-frames x the per-voxel-frame instruction count of the disassembly against the VALU rate.
CPU leg, as reported and not optimised against: tests/tsdf_ref.py (NumPy, one thread) on a 64^3 volume and 10 frames.
usage: tsdf_once.py [reps] [out.json] [cpu: 1|0]
       tsdf_once.py bilateral [reps] [out.json]     the depth bilateral filter alone (bilateral_leg below)"""
import importlib
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
r3d = importlib.import_module("3d_reconstruction_system_amd")
S = importlib.import_module("3d_reconstruction_system_amd.synthetic")
T = importlib.import_module("3d_reconstruction_system_amd.tsdf")
bilateral_only = len(sys.argv) > 1 and sys.argv[1] == "bilateral"
if bilateral_only:
    del sys.argv[1]
reps = int(sys.argv[1]) if len(sys.argv) > 1 else 20
out_path = sys.argv[2] if len(sys.argv) > 2 else None
cpu_leg = (sys.argv[3] != "0") if len(sys.argv) > 3 else True
ctx = r3d.Context(0)


def bilateral_leg():
    """r3d_depth_bilateral alone: a noisy room_view raster of 1080 x 1920 and of 480 x 640 in HBM, radius 3 and 6
    (sigma_s = radius / 1.5 pixels, sigma_r 0.05 m), in_stride 1.  One timed window is CALLS back-to-back calls between two HIP
    events (a single launch of this size is shorter than the events' own resolution); the figure is the median window of `reps`
    after two warm-ups, divided by CALLS, the four legs alternating run by run; one untimed call of the leg's parameters goes in
    front of every window, so the window holds kernels only (the tables are cached by then).  Next to it: one read plus one write of the raster
    at the HBM rate.  No gate: there is no earlier kernel to compare with."""
    L = importlib.import_module("3d_reconstruction_system_amd._lib")
    CALLS = 20
    legs = []
    for h, w in ((1080, 1920), (480, 640)):
        z = S.room_view(h, w, 0.9, np.array([0.3, -0.1, 0.4]), pitch=0.2)[0]
        z = (z * (1.0 + np.random.default_rng(7).normal(size=z.shape) * 0.005)).astype(np.float32)
        d_in, d_out = ctx.alloc(z.nbytes).upload(z), ctx.alloc(z.nbytes)
        for radius in (3, 6):
            legs.append((h, w, radius, d_in, d_out))
    times = [[] for _ in legs]
    for k in range(reps + 2):
        for i, (h, w, radius, d_in, d_out) in enumerate(legs):
            # one call of this leg's parameters outside the window: the table build and upload of a changed radius stay out of it
            L.check(ctx.lib.r3d_depth_bilateral(ctx.handle, d_in.ptr, 1, h, w, radius, radius / 1.5, 0.05, d_out.ptr))
            ctx.sync()
            ctx.timer_start()
            for _ in range(CALLS):
                L.check(ctx.lib.r3d_depth_bilateral(ctx.handle, d_in.ptr, 1, h, w, radius, radius / 1.5, 0.05, d_out.ptr))
            t = ctx.timer_stop()
            if k >= 2:
                times[i].append(t / CALLS)
    out = []
    for (h, w, radius, _, _), t in zip(legs, times):
        out.append({"kernel": "depth_bilateral", "raster": [h, w], "radius": radius, "reps": reps, "calls_per_window": CALLS,
                    "ms_per_call_median": round(float(np.median(t)), 5), "ms_per_call_min": round(float(np.min(t)), 5),
                    "ms_per_call_max": round(float(np.max(t)), 5),
                    "read_plus_write_at_8TBps_ms": round(2.0 * 4 * h * w / 8.0e12 * 1e3, 5)})
        print(json.dumps(out[-1]), flush=True)
    return out


if bilateral_only:
    lines = bilateral_leg()
    if out_path:
        with open(out_path, "w") as f:
            for line in lines:
                f.write(json.dumps(line) + "\n")
    ctx.close()
    sys.exit(0)

FRAMES, H, W = 100, 384, 1280
INSTR_PER_VOXEL_FRAME = 125          # from the disassembly of tsdf_integrate_kernel<uint8_t, true>'s frame loop
HBM_BYTES_PER_S = 8.0e12
VALU_LANE_INSTR_PER_S = 256 * 4 * 32 * 2.4e9     # CUs x SIMDs x lanes per clock x clock


def timed_alternating(fns, before):
    ts = [[] for _ in fns]
    for k in range(reps + 2):
        for i, fn in enumerate(fns):
            before()
            ctx.sync()
            ctx.timer_start()
            fn()
            t = ctx.timer_stop()
            if k >= 2:
                ts[i].append(t)
    return [round(float(np.median(t)), 4) for t in ts]


depth, quats, ts, K = S.room_views(FRAMES, H, W, seed=0)
depth_u8 = np.clip(np.round(depth * 32.0), 0, 255).astype(np.uint8)
del depth
poses = T.poses_w2c(quats, ts)
cam = ctx.camera(H, W, *K)
d_depth = ctx.alloc(depth_u8.nbytes).upload(depth_u8)
rgb = np.random.default_rng(0).integers(0, 256, (FRAMES, H, W, 3), dtype=np.uint8)
d_rgb = ctx.alloc(rgb.nbytes).upload(rgb)
del rgb
lo, hi = S.ROOM_LO - 0.3, S.ROOM_HI + 0.3
lines = []
for n in (256, 512):
    vs = float((hi - lo).max() / n)
    vol = T.TSDFVolume(lo, vs, (n, n, n), 4 * vs, ctx=ctx)

    def batched():
        vol.integrate_device(cam, d_depth.ptr, np.uint8, FRAMES, poses, 1.0 / 32)

    def per_frame():
        for f in range(FRAMES):
            vol.integrate_device(cam, d_depth.ptr + f * H * W, np.uint8, 1, poses[f:f + 1], 1.0 / 32)

    b_ms, p_ms = timed_alternating([batched, per_frame], vol.reset)
    vol.reset()
    batched()
    count = vol.extract_points_device(1.0, None, None, 0)
    d_xyz, d_nrm = ctx.alloc(max(count, 1) * 12), ctx.alloc(max(count, 1) * 12)
    n_v, n_t = vol.extract_mesh_device(1.0, None, None, 0, None, 0)
    assert n_v == count
    d_tri = ctx.alloc(max(n_t, 1) * 12)
    e_ms, m_ms = timed_alternating([lambda: vol.extract_points_device(1.0, d_xyz.ptr, d_nrm.ptr, count),
                                    lambda: vol.extract_mesh_device(1.0, d_xyz.ptr, d_nrm.ptr, count, d_tri.ptr, n_t)], lambda: None)
    # the colour legs
    cvol = T.TSDFVolume(lo, vs, (n, n, n), 4 * vs, ctx=ctx, color=True)

    def batched_rgb():
        cvol.integrate_device(cam, d_depth.ptr, np.uint8, FRAMES, poses, 1.0 / 32, d_rgb=d_rgb.ptr)

    def reset_both():
        vol.reset()
        cvol.reset()

    d_ms, c_ms = timed_alternating([batched, batched_rgb], reset_both)
    reset_both()
    batched()
    batched_rgb()
    assert cvol.extract_colors_device(1.0, None, 0) == count
    d_rgba = ctx.alloc(max(count, 1) * 4)
    ec_ms, ep_ms = timed_alternating([lambda: cvol.extract_colors_device(1.0, d_rgba.ptr, count),
                                      lambda: cvol.extract_points_device(1.0, d_xyz.ptr, d_nrm.ptr, count)], lambda: None)
    d_rgba.free()
    cvol.close()
    _, w = vol.volume()
    pairs = float(w.sum())                               # (voxel, frame) pairs that passed every test
    launches = -(-FRAMES // T.CHUNK)
    voxels = n ** 3
    roof_bytes_ms = (16.0 * voxels * launches + depth_u8.nbytes) / HBM_BYTES_PER_S * 1e3
    roof_valu_ms = voxels * FRAMES * INSTR_PER_VOXEL_FRAME / VALU_LANE_INSTR_PER_S * 1e3
    line = {"volume": "%d^3" % n, "voxel_size": round(vs, 6), "frames": FRAMES, "raster": [H, W], "dtype": "uint8", "reps": reps,
            "integrate_batched_ms": b_ms, "integrate_per_frame_ms": p_ms, "per_frame_over_batched": round(p_ms / b_ms, 3),
            "extract_ms": e_ms, "mesh_ms": m_ms, "integrate_rgb_batched_ms": c_ms, "integrate_depth_only_same_legs_ms": d_ms,
            "rgb_over_depth_only": round(c_ms / d_ms, 3), "extract_colors_ms": ec_ms, "extract_points_color_volume_ms": ep_ms, "surface_points": int(count), "triangles": int(n_t), "voxel_frame_pairs_accepted": pairs,
            "voxel_frames_per_s_batched": round(voxels * FRAMES / (b_ms * 1e-3), 1),
            "roof_hbm_ms_8TBps": round(roof_bytes_ms, 4), "roof_valu_ms_at_%d_instr" % INSTR_PER_VOXEL_FRAME: round(roof_valu_ms, 4)}
    print(json.dumps(line), flush=True)
    lines.append(line)
    for b in (d_xyz, d_nrm, d_tri):
        b.free()
    vol.close()
if cpu_leg:
    import tsdf_ref as REF
    vs = float((hi - lo).max() / 64)
    ref = REF.Volume(lo, vs, (64, 64, 64), 4 * vs)
    t0 = time.perf_counter()
    REF.integrate(ref, depth_u8[:10], poses[:10], K, 1.0 / 32)
    t1 = time.perf_counter()
    xyz, _ = REF.extract(ref)
    line = {"volume": "64^3", "frames": 10, "cpu_numpy_one_thread_integrate_s": round(t1 - t0, 3),
            "cpu_numpy_one_thread_extract_s": round(time.perf_counter() - t1, 3), "surface_points": int(len(xyz))}
    print(json.dumps(line), flush=True)
    lines.append(line)
if out_path:
    with open(out_path, "w") as f:
        for line in lines:
            f.write(json.dumps(line) + "\n")
