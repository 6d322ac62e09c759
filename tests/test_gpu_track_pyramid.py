"""GPU: the depth pyramid (csrc/r3d_pyramid.hip) bit for bit against tests/pyramid_ref.py, the NumPy restatement of include/r3d.h
"Depth pyramid", and the coarse-to-fine driver r3d_tsdf_track_pyramid: its one-level case against r3d_tsdf_track byte for byte,
its pose against the reference loop over the device's own maps, whole sequences, an empty volume, the invalid calls and the
command line."""
import ctypes as C
import importlib
import os
import subprocess
import sys

import numpy as np
import pytest

import pyramid_ref as PR
import track_ref as TR
from helpers import PKG, ROOT, r3d as _r3d
from test_gpu_bounds import Guarded
from test_gpu_track import room_volume, small_motion_sequence, surface_count

pytestmark = pytest.mark.gpu

F = np.float32
# 2 x 2: one output; 2 x 3, 3 x 5: an odd row / column dropped; 5 x 258: 258 outputs, two workgroups, the second partial; 64 x 66
# and 96 x 128: even widths (both rows of a block pair-aligned from an aligned base); 17 x 65: odd width (the rows alternate)
RASTERS = [(2, 2), (2, 3), (3, 5), (5, 258), (64, 66), (17, 65), (96, 128)]
MAX_JUMP = 0.25


@pytest.fixture(scope="module")
def R():
    return _r3d()


@pytest.fixture(scope="module")
def L(R):
    return importlib.import_module(PKG + "._lib")


@pytest.fixture(scope="module")
def tracking(R):
    return importlib.import_module(PKG + ".tracking")


@pytest.fixture(scope="module")
def ctx(R):
    c = R.Context(0)
    yield c
    c.close()


def bits(a):
    return np.ascontiguousarray(a, dtype=F).view(np.uint32)


def dirty_depth(h, w, seed):
    """random depths with 20 % invalid of every kind (0, negative, NaN, +inf, -inf), some blocks wholly invalid, and, in a fifth of the
    blocks, an edge planted around MAX_JUMP: the block's minimum 1.0 and a partner exactly MAX_JUMP behind it, one ulp more, one ulp less or far behind"""
    rng = np.random.default_rng([seed, h, w])
    d = rng.uniform(0.5, 4.0, size=(h, w)).astype(F)
    step = F(1.0) + F(MAX_JUMP)
    partners = [step, np.nextafter(step, F(np.inf)), np.nextafter(step, F(0.0)), F(3.0)]
    for v in range(h >> 1):
        for u in range(w >> 1):
            if rng.random() < 0.2:
                block = np.array([1.0] + [partners[k] for k in rng.integers(0, 4, size=3)], dtype=F)
                d[2 * v:2 * v + 2, 2 * u:2 * u + 2] = rng.permutation(block).reshape(2, 2)
    kind = rng.random((h, w))
    for k, bad in enumerate([0.0, -1.5, np.nan, np.inf, -np.inf]):
        d[(kind >= 0.04 * k) & (kind < 0.04 * (k + 1))] = bad
    for v in range(h >> 1):                                           # ... and one block in twenty has no valid depth at all
        for u in range(w >> 1):
            if rng.random() < 0.05:
                d[2 * v:2 * v + 2, 2 * u:2 * u + 2] = rng.permutation(np.array([0.0, np.nan, -2.0, np.inf], dtype=F)).reshape(2, 2)
    return d


@pytest.mark.parametrize("h,w", RASTERS)
def test_depth_half_against_reference(L, ctx, tracking, h, w):
    d = dirty_depth(h, w, 1)
    oh, ow = h >> 1, w >> 1
    rng = np.random.default_rng([2, h, w])
    vertex = rng.normal(size=(h, w, 3)).astype(F)
    vertex[..., 2] = d
    made = []
    try:
        seen = set()
        for k, (stride, in_off, out_off, mj) in enumerate([(1, 0, 0, MAX_JUMP), (1, 4, 4, MAX_JUMP), (3, 0, 4, MAX_JUMP), (3, 4, 0, MAX_JUMP),
                                                           (1, 0, 4, 0.0), (1, 4, 0, np.inf), (3, 0, 0, np.inf)]):
            want = PR.depth_half(d, mj)
            g_in = Guarded(ctx, h * w * 4 * stride, in_off, d if stride == 1 else vertex, seed=k)
            g_out = Guarded(ctx, oh * ow * 4, out_off, seed=20 + k)
            made += [g_in, g_out]
            L.check(ctx.lib.r3d_depth_half(ctx.handle, g_in.ptr + (8 if stride == 3 else 0), stride, h, w, mj, g_out.ptr))
            got = g_out.read(np.uint32)
            assert np.array_equal(got, bits(want).reshape(-1)), (stride, in_off, out_off, mj, np.flatnonzero(got != bits(want).reshape(-1))[:5])
            g_in.unchanged()
            L.check(ctx.lib.r3d_depth_half(ctx.handle, g_in.ptr + (8 if stride == 3 else 0), stride, h, w, mj, g_out.ptr))
            assert np.array_equal(g_out.read(np.uint32), got)                      # the same bytes on a repeat
            seen.add(want.tobytes())
        if h * w >= 1000:
            # the cases are not all alike: the edges and the invalid entries decide something
            assert len(seen) == 3
            ref, near, far = PR.depth_half(d, MAX_JUMP), PR.depth_half(d, 0.0), PR.depth_half(d, np.inf)
            assert (ref == 0).any() and (ref != near).any() and (ref != far).any()
        if (h, w) == (17, 65):
            assert np.array_equal(bits(tracking.depth_half(d, MAX_JUMP, ctx=ctx)), bits(PR.depth_half(d, MAX_JUMP)))
    finally:
        for g in made:
            g.free()


def test_depth_half_invalid_calls_write_nothing(L, ctx):
    h, w = 5, 8
    d = dirty_depth(h, w, 3)
    g_in, g_out = Guarded(ctx, h * w * 4, 0, d), Guarded(ctx, 2 * 4 * 4, 0, seed=4)
    g_vertex = Guarded(ctx, h * w * 12, 0, seed=5)
    try:
        good = dict(ctx=ctx.handle, din=g_in.ptr, stride=1, h=h, w=w, mj=0.05, out=g_out.ptr)
        order = ["ctx", "din", "stride", "h", "w", "mj", "out"]
        bad = [dict(ctx=None), dict(din=None), dict(out=None), dict(stride=2), dict(stride=0), dict(stride=-1), dict(stride=4), dict(h=1),
               dict(w=1), dict(h=0), dict(w=-2), dict(mj=float("nan")), dict(mj=-0.5), dict(mj=-float("inf")),
               dict(out=g_in.ptr), dict(out=g_in.ptr + h * w * 4 - 4), dict(din=g_out.ptr, h=2, w=2),
               dict(h=1 << 16, w=1 << 15),                                                                # 2^31 pixels
               # stride 3 reaches ((h w - 1) 3 + 1) floats: an output behind the stride-1 extent but inside that one
               dict(din=g_vertex.ptr + 8, stride=3, out=g_vertex.ptr + h * w * 4 + 64),
               dict(din=g_vertex.ptr + 8, stride=3, out=g_vertex.ptr + 8 + ((h * w - 1) * 3) * 4)]
        for b in bad:
            a = {**good, **b}
            assert ctx.lib.r3d_depth_half(*[a[k] for k in order]) == L.ERR_INVALID, b
        for g in (g_in, g_out, g_vertex):
            g.unchanged()
        # ... and the first byte behind the stride-3 extent is a valid output
        a = {**good, **dict(din=g_vertex.ptr + 8, stride=3, h=2, w=2, out=g_vertex.ptr + 8 + (3 * 3 + 1) * 4)}
        assert ctx.lib.r3d_depth_half(*[a[k] for k in order]) == L.OK
        ctx.sync()
    finally:
        for g in (g_in, g_out, g_vertex):
            g.free()


def test_camera_half(L, ctx):
    cam = ctx.camera(17, 65, 102.4, 99.7, 31.5, 8.25)
    out = C.c_void_p(0x1234)
    assert ctx.lib.r3d_camera_half(cam.handle, None) == L.ERR_INVALID
    tiny = ctx.camera(1, 65, 102.4, 99.7, 31.5, 0.0)
    assert ctx.lib.r3d_camera_half(tiny.handle, C.byref(out)) == L.ERR_INVALID and out.value == 0x1234
    L.check(ctx.lib.r3d_camera_half(cam.handle, C.byref(out)))
    try:
        # the new camera is of this context, 8 x 32, and unprojects as ctx.camera(8, 32, pyramid_intrinsics(K, 1)) does
        depth = np.random.default_rng(6).uniform(0.5, 4.0, size=(8, 32)).astype(F)
        want_cam = ctx.camera(8, 32, *PR.pyramid_intrinsics((102.4, 99.7, 31.5, 8.25), 1))
        d_depth, d_a, d_b = ctx.alloc(depth.nbytes).upload(depth), ctx.alloc(8 * 32 * 12), ctx.alloc(8 * 32 * 12)
        L.check(ctx.lib.r3d_unproject(ctx.handle, out.value, d_depth.ptr, L.DEPTH_F32, 1, 1.0, d_a.ptr, L.F32))
        L.check(ctx.lib.r3d_unproject(ctx.handle, want_cam.handle, d_depth.ptr, L.DEPTH_F32, 1, 1.0, d_b.ptr, L.F32))
        assert d_a.download(np.uint32, 8 * 32 * 3).tobytes() == d_b.download(np.uint32, 8 * 32 * 3).tobytes()
        for b in (d_depth, d_a, d_b):
            b.free()
    finally:
        ctx.lib.r3d_camera_destroy(out.value)


# ---- the driver ----------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def scene(R, ctx):
    """The setup of test_gpu_track.test_frame_to_model_on_a_real_volume: 16 room_views of 96 x 128 in a volume of 0.05 m voxels,
    pose 2 as the guess."""
    syn = importlib.import_module(PKG + ".synthetic")
    H, W, n_frames, i = 96, 128, 16, 2
    depths, quats, ts, K = syn.room_views(n_frames, H, W, seed=0)
    poses = R.poses_w2c(quats, ts)
    V = room_volume(R, ctx, 0.05, 0.2)
    V.integrate(depths, quats, ts, intrinsics=K)
    T_i = TR.pose_matrix(poses[i])
    c_i = -T_i[:3, :3].T @ T_i[:3, 3]

    def frame(yaw_deg, dcentre):
        z, q, t, _ = syn.room_view(H, W, 2 * np.pi * i / n_frames + 0.1 + np.radians(yaw_deg), c_i + np.asarray(dcentre))
        return z.astype(F), TR.pose_row(q, t)
    s = {"V": V, "H": H, "W": W, "K": K, "guess": poses[i].copy(), "quat": quats[i:i + 1], "t": ts[i:i + 1], "frame": frame}
    yield s
    V.close()


def device_levels(R, V, s, sv0, n_levels, max_jump):
    """every level's maps as the device makes them, from the level-0 source vertex map: ray casts at the level intrinsics,
    unproject of depth_half rasters"""
    tracking = importlib.import_module(PKG + ".tracking")
    depth = np.ascontiguousarray(sv0[..., 2])
    levels = []
    for l in range(n_levels):
        Kl, (h, w) = tracking.pyramid_intrinsics(s["K"], l), tracking.pyramid_shape(s["H"], s["W"], l)
        if l > 0:
            depth = tracking.depth_half(depth, max_jump, ctx=V.ctx)
        _, vertex, normal = V.raycast(s["quat"], s["t"], (h, w), intrinsics=Kl)
        levels.append({"src_vertex": sv0 if l == 0 else R.unproject(depth, intrinsics=Kl).reshape(h, w, 3), "src_normal": None,
                       "model_vertex": vertex[0], "model_normal": normal[0], "K": Kl})
    return levels


def test_one_level_equals_tsdf_track(R, scene):
    V, frame = scene["V"], scene["frame"](2.0, (0.03, 0.0, 0.04))[0]
    for kwargs in (dict(), dict(max_angle_deg=30.0)):
        row, info = V.track(frame, scene["guess"], intrinsics=scene["K"], **kwargs)
        for n in (10, 0, 3):
            if n != 10:
                row, info = V.track(frame, scene["guess"], intrinsics=scene["K"], n_iters=n, **kwargs)
            row1, info1 = V.track(frame, scene["guess"], intrinsics=scene["K"], pyramid_iters=(n,), **kwargs)
            assert row1.tobytes() == row.tobytes(), (kwargs, n)
            assert len(info1.pop("rms_history")) == n and info1 == info and info["iterations"] == n
    assert info["status"] == 0 and info["pairs"] > 0


def test_pyramid_pose_against_reference_loop_over_device_maps(R, scene):
    V, K = scene["V"], scene["K"]
    frame, true_row = scene["frame"](2.0, (0.03, 0.0, 0.04))
    iters = (10, 5, 4)
    row, info = V.track(frame, scene["guess"], intrinsics=K, pyramid_iters=iters)
    assert info["status"] == 0 and info["iterations"] == 19 and len(info["rms_history"]) == 19
    levels = device_levels(R, V, scene, R.unproject(frame, intrinsics=K).reshape(scene["H"], scene["W"], 3), 3, 0.05)
    want, winfo = PR.track(levels, iters, scene["guess"], 2 * 0.2, -1.0)
    assert winfo["status"] == 0 and winfo["margin"] >= 1e-9, winfo["margin"]
    print("pyramid (10, 5, 4): %s -> %s; matched per pass %s" % (TR.pose_error(scene["guess"], true_row), TR.pose_error(row, true_row),
                                                                 winfo["matched"]))
    np.testing.assert_allclose(row, want, atol=2e-6, rtol=0)
    np.testing.assert_allclose(info["rms_history"], winfo["rms_history"], atol=2e-6, rtol=0)
    assert info["pairs"] == winfo["pairs"] and abs(info["rms"] - winfo["rms"]) <= 2e-6
    # every level was used: the coarse passes see a quarter / a sixteenth of the pixels
    assert max(winfo["matched"][:4]) <= 24 * 32 and max(winfo["matched"][4:9]) <= 48 * 64 < max(winfo["matched"][9:])
    # a level with 0 iterations is skipped, whichever it is; a repeat gives the same bytes
    for it in ((0, 5, 4), (10, 0, 4), (10, 5, 0), (0, 0, 6)):
        r2, i2 = V.track(frame, scene["guess"], intrinsics=K, pyramid_iters=it)
        w2, wi2 = PR.track(levels, it, scene["guess"], 2 * 0.2, -1.0)
        assert i2["status"] == 0 and i2["iterations"] == sum(it) == len(i2["rms_history"])
        np.testing.assert_allclose(r2, w2, atol=2e-6, rtol=0)
    r3, i3 = V.track(frame, scene["guess"], intrinsics=K, pyramid_iters=iters)
    assert r3.tobytes() == row.tobytes() and i3 == info
    # u16 input goes the same way: level 0's depth is the z column of its vertex map, whatever dtype the frame came in
    mm = np.round(frame * 1000.0).astype(np.uint16)
    r4, i4 = V.track(mm, scene["guess"], intrinsics=K, pyramid_iters=iters, depth_scale=0.001)
    lv = device_levels(R, V, scene, R.unproject(mm, intrinsics=K, depth_scale=0.001).reshape(scene["H"], scene["W"], 3), 3, 0.05)
    w4, wi4 = PR.track(lv, iters, scene["guess"], 2 * 0.2, -1.0)
    assert i4["status"] == 0 and wi4["margin"] >= 1e-9
    np.testing.assert_allclose(r4, w4, atol=2e-6, rtol=0)


def test_pyramid_on_a_large_motion(R, scene):
    """12 degrees of yaw and 0.30 m along (0.6, 0, 0.8) from the guess.  Measured on the CPU first (tsdf_ref + raycast_ref +
    track_ref + pyramid_ref, no device), yaw a degrees and 0.025 a m for a in 4, 6, 8, 10, 12, one level with 19 iterations
    against levels (10, 5, 4):
        a = 4: 0.00748 deg / 0.000537 m   against 0.00748 deg / 0.000537 m
        a = 6: 0.02180 deg / 0.001022 m   against 0.02180 deg / 0.001022 m
        a = 8: 0.02417 deg / 0.001032 m   against 0.02418 deg / 0.001031 m
        a = 10: 0.02974 deg / 0.001145 m  against 0.02974 deg / 0.001145 m
        a = 12: 0.04021 deg / 0.002189 m  against 0.04021 deg / 0.002189 m
    No a separates the two: in this room of six flat walls the point-to-plane step is right even for a pair that is wrong along
    its wall, so the one-level loop follows every motion of the list and ends where the pyramid ends.  The assertion "the
    pyramid beats the one-level loop" is therefore not made.  What stays: at the largest motion of the list the
    pyramid's status is 0 and its error is under 4 x the pyramid reference's figures, the margin DESIGN 4.5m uses because the
    device's maps are not raycast_ref's bit for bit.  The smallest rounding margin of a reference pass at a = 12 is 7.8e-7."""
    V, K, a = scene["V"], scene["K"], 12.0
    frame, true_row = scene["frame"](a, 0.025 * a * np.array([0.6, 0.0, 0.8]))
    before = TR.pose_error(scene["guess"], true_row)
    assert abs(before[0] - 12.0) < 1e-6 and abs(before[1] - 0.3) < 1e-9
    row, info = V.track(frame, scene["guess"], intrinsics=K, pyramid_iters=(10, 5, 4))
    one, info1 = V.track(frame, scene["guess"], intrinsics=K, n_iters=19)
    after, after1 = TR.pose_error(row, true_row), TR.pose_error(one, true_row)
    print("a = 12: pyramid %.5f deg / %.6f m (status %d), one level x 19 %.5f deg / %.6f m (status %d)"
          % (after[0], after[1], info["status"], after1[0], after1[1], info1["status"]))
    assert info["status"] == 0 and info["iterations"] == 19
    assert after[0] < 4 * 0.04021 and after[1] < 4 * 0.002189


def test_track_and_integrate_with_a_pyramid(R, ctx):
    """test_gpu_track.test_track_and_integrate_small_motions with pyramid_iters=(10, 5, 4).  The reference pyramid loop on the CPU
    (raycast_ref + tsdf_ref + pyramid_ref) keeps every centre within 0.00465 m and ends with 2128 surface points against 2129
    with the true poses: inside the existing test's bounds, one voxel and 5 %."""
    depths, truth, K, quats, ts = small_motion_sequence(8, 48, 64)
    V = room_volume(R, ctx, 0.1, 0.3)
    rows = V.track_and_integrate(depths, truth[0], intrinsics=K, pyramid_iters=(10, 5, 4))
    n_tracked = surface_count(V)
    V.reset()
    V.integrate(depths, np.array(quats), np.array(ts), intrinsics=K)
    n_true = surface_count(V)
    assert rows.shape == (8, 12) and rows[0].tobytes() == truth[0].tobytes()
    errs = [TR.pose_error(rows[k], truth[k]) for k in range(8)]
    print("track_and_integrate, pyramid: worst centre error %.5f m, worst rotation %.4f degrees, %d / %d points" %
          (max(e[1] for e in errs), max(e[0] for e in errs), n_tracked, n_true))
    assert max(e[1] for e in errs) <= 0.1
    assert abs(n_tracked - n_true) <= 0.05 * n_true
    V.reset()
    blank = depths.copy()
    blank[3] = 0.0
    with pytest.raises(RuntimeError, match="frame 3"):
        V.track_and_integrate(blank, truth[0], intrinsics=K, pyramid_iters=(10, 5, 4))
    V.close()


def test_empty_volume_gives_the_guess_back(R, ctx, scene):
    V = room_volume(R, ctx, 0.1, 0.3)
    frame = scene["frame"](2.0, (0.03, 0.0, 0.04))[0]
    row, info = V.track(frame, scene["guess"], intrinsics=scene["K"], pyramid_iters=(3, 2, 2))
    assert info["status"] == 1 and info["pairs"] == 0 and info["iterations"] == 7 and row.tobytes() == scene["guess"].tobytes()
    assert info["rms_history"] == [0.0] * 7
    V.close()


def test_invalid_driver_calls_write_nothing(R, L, ctx, tracking):
    h, w = 9, 13
    K = (10.0, 10.0, 6.0, 4.0)
    cams = [ctx.camera(*tracking.pyramid_shape(h, w, l), *tracking.pyramid_intrinsics(K, l)) for l in range(3)]     # 9 x 13, 4 x 6, 2 x 3
    other = R.Context(0)
    V = room_volume(R, ctx, 0.5, 1.0)
    d_depth = Guarded(ctx, h * w * 4, 0, np.ones((h, w), F))
    try:
        wrong = ctx.camera(4, 7, *tracking.pyramid_intrinsics(K, 1))
        foreign = other.camera(4, 6, *tracking.pyramid_intrinsics(K, 1))
        pose = np.concatenate([np.eye(3).reshape(9), np.zeros(3)])
        out, info, rms = np.full(12, 7.0), np.full(4, 7.0), np.full(464, 7.0)
        inf = float("inf")

        def arr(*handles):
            return (C.c_void_p * len(handles))(*handles)

        def cnt(*n):
            return (C.c_int * len(n))(*n)
        h0, h1, h2 = [c.handle for c in cams]
        good = dict(vol=V.handle, cams=arr(h0, h1, h2), n=3, it=cnt(2, 1, 1), depth=d_depth.ptr, dt=L.DEPTH_F32, scale=1.0,
                    guess=pose.ctypes.data, mw=1.0, step=0.5, tn=0.0, tf=inf, mj=0.05, dist=0.5, cos=-1.0, out=out.ctypes.data,
                    info=info.ctypes.data, rms=rms.ctypes.data)
        order = ["vol", "cams", "n", "it", "depth", "dt", "scale", "guess", "mw", "step", "tn", "tf", "mj", "dist", "cos", "out", "info", "rms"]
        nan_guess = np.full(12, np.nan)
        bad = [dict(cams=arr(h0, wrong.handle, h2)), dict(cams=arr(h0, h2, h2)), dict(cams=arr(h0, h0, h1)),              # a wrong level size
               dict(cams=arr(h0, foreign.handle, h2)),                                                                  # another context
               dict(n=0), dict(n=9), dict(n=-1), dict(it=cnt(2, -1, 1)), dict(it=cnt(-1, 0, 0)),
               dict(it=cnt(400, 60, 5)), dict(it=cnt(2**31 - 1, 2**31 - 1, 2)),                                         # a sum over the limit
               dict(cams=arr(h0, None, h2)), dict(cams=arr(None, h1, h2)), dict(cams=arr(h0, h1, None)), dict(cams=None), dict(it=None),
               # every argument error of r3d_tsdf_track
               dict(vol=None), dict(depth=None), dict(dt=9), dict(guess=None), dict(guess=nan_guess.ctypes.data), dict(mw=0.0), dict(step=0.0),
               dict(tn=-1.0), dict(tn=2.0, tf=1.0), dict(mj=-1.0), dict(mj=float("nan")), dict(dist=0.0), dict(dist=inf), dict(cos=2.0),
               dict(cos=float("nan")), dict(out=None), dict(info=None), dict(out=info.ctypes.data), dict(out=pose.ctypes.data),
               # h_rms_out over another host argument
               dict(rms=out.ctypes.data), dict(rms=info.ctypes.data + 8), dict(rms=pose.ctypes.data + 88)]
        for b in bad:
            a = {**good, **b}
            assert ctx.lib.r3d_tsdf_track_pyramid(*[a[k] for k in order]) == L.ERR_INVALID, b
        its = cnt(2, 1, 1)
        a = {**good, "it": its, "rms": C.addressof(its) - 8}                       # 4 doubles that end inside h_iters
        assert ctx.lib.r3d_tsdf_track_pyramid(*[a[k] for k in order]) == L.ERR_INVALID
        assert np.all(out == 7.0) and np.all(info == 7.0) and np.all(rms == 7.0)
        d_depth.unchanged()
        # the limit itself is valid, and h_rms_out may be NULL
        a = {**good, "it": cnt(460, 2, 2), "rms": None}
        assert ctx.lib.r3d_tsdf_track_pyramid(*[a[k] for k in order]) == L.OK
        assert info[3] == 464.0 and np.all(rms == 7.0)
    finally:
        d_depth.free()
        V.close()
        other.close()


def test_command_line_with_track_pyramid(R, ctx, tmp_path):
    """--track --track-pyramid 10,5,4 reconstructs from 8-bit depth maps and the first pose, as test_command_line_with_track_flag
    does without the pyramid; every other output is what --track writes."""
    from PIL import Image
    syn = importlib.import_module(PKG + ".synthetic")
    H, W, n, scale = 48, 64, 5, 40.0            # the room in units of 2.5 cm, so that an 8-bit raster holds its depths
    lo, hi = syn.ROOM_LO * scale, syn.ROOM_HI * scale
    frames = [syn.room_view(H, W, 0.9 + np.radians(2.0) * k, (np.array([0.3, -0.1, 0.4]) + k * np.array([0.03, 0.01, -0.04])) * scale,
                            lo=lo, hi=hi) for k in range(n)]
    K = frames[0][3]
    work = tmp_path / "work"
    os.makedirs(str(work / "depth"))
    os.makedirs(str(work / "camera_pose"))
    rows = ["id,tx,ty,tz,qx,qy,qz,qw,name,tail"]
    for k, (z, q, t, _) in enumerate(frames):
        Image.fromarray(np.clip(np.round(z), 0, 255).astype(np.uint8), mode="L").save(str(work / "depth" / ("%03d.png" % k)))
        rows.append(",".join([str(k + 1)] + [repr(float(v)) for v in t] + [repr(float(v)) for v in q] + ["%03d.png" % k, "x"]))
    (work / "camera_pose" / "image_colmap_simi_2.txt").write_text("\n".join(rows) + "\n")
    tool = os.path.join(ROOT, PKG, "other_tools", "integrate_tsdf.py")
    origin = [str(v) for v in lo - 12.0]
    dims = [str(int(np.ceil((hi[a] - lo[a] + 24.0) / 4.0))) for a in range(3)]
    args = ["--voxel-size", "4", "--trunc", "12", "--origin"] + origin + ["--dims"] + dims
    env = dict(os.environ, PYTHONPATH=ROOT, R3D_FX=repr(K[0]), R3D_FY=repr(K[1]), R3D_CX=repr(K[2]), R3D_CY=repr(K[3]))
    r = subprocess.run([sys.executable, tool] + args + ["--track", "--track-pyramid", "10,5,4"], cwd=str(work), env=env, capture_output=True,
                       text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-1000:] + r.stderr[-2000:]
    assert r.stdout.strip().split("\n")[-1] == "tracked %d frames -> ./camera_pose/image_colmap_simi_2_tracked.txt" % n
    assert sorted(os.listdir(str(work / "ply"))) == ["tsdf_surface.ply"]
    names, quats, ts = R.read_pose_file(str(work / "camera_pose" / "image_colmap_simi_2.txt"))
    names2, quats2, ts2 = R.read_pose_file(str(work / "camera_pose" / "image_colmap_simi_2_tracked.txt"))
    assert names2 == names
    got, want = R.poses_w2c(quats2, ts2), R.poses_w2c(quats, ts)
    np.testing.assert_allclose(got[0], want[0], atol=1e-12)
    errs = [TR.pose_error(got[k], want[k]) for k in range(n)]
    print("--track-pyramid: worst centre error %.3f units (voxel 4), worst rotation %.4f degrees" % (max(e[1] for e in errs), max(e[0] for e in errs)))
    assert max(e[1] for e in errs) <= 4.0 and max(e[0] for e in errs) <= 1.0
    # the tool's poses are the library's for the same call
    depths = R.cloud_io.read_depth_batch([str(work / "depth" / nm) for nm in names])
    V = R.TSDFVolume([float(v) for v in origin], 4.0, [int(d) for d in dims], 12.0, ctx=ctx)
    lib_rows = V.track_and_integrate(depths, want[0], intrinsics=K, pyramid_iters=(10, 5, 4))
    V.close()
    assert max(TR.pose_error(got[k], lib_rows[k])[1] for k in range(n)) <= 1e-6
    # the flag needs --track
    r2 = subprocess.run([sys.executable, tool] + args + ["--track-pyramid", "10,5,4"], cwd=str(work), env=env, capture_output=True, text=True,
                        timeout=300)
    assert r2.returncode == 2 and "--track-pyramid needs --track" in r2.stderr
