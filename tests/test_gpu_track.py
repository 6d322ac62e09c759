"""GPU: frame-to-model tracking (csrc/r3d_track.hip) against tests/track_ref.py, the NumPy restatement of include/r3d.h "TSDF
tracking": per-pixel match codes and residuals bit for bit, the 29 sums at the tolerance test_gpu_plane_icp.py uses for the same
sums, the device-resident loop against the one-pass form and against the reference loop, and the whole step on real volumes."""
import ctypes as C
import importlib
import itertools
import os
import shutil
import subprocess
import sys

import numpy as np
import pytest

import track_ref as TR
from helpers import PKG, ROOT, r3d as _r3d
from test_gpu_bounds import Guarded

pytestmark = pytest.mark.gpu

RASTERS = [(1, 1), (5, 7), (32, 32), (33, 31), (17, 65)]   # 32 x 32: exactly one workgroup; 1023 px; 1105 px: two, the second partial
OFFSETS = [0, 4, 8]


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
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def rot_y(a):
    T = np.eye(4)
    T[0, 0] = T[2, 2] = np.cos(a)
    T[0, 2], T[2, 0] = np.sin(a), -np.sin(a)
    return T


def dirty_case(h, w, seed):
    """analytic room maps with what real maps carry: ~10 % missing model rows (NaN), some zero model normals; source rows with
    Z = 0, NaN, +-inf and negative z; random unit source normals near the model's, some zero"""
    rng = np.random.default_rng([seed, h, w])
    case = TR.analytic_case(h, w, 2.0, 1.0, (0.03, 0.02, -0.04))
    n = h * w
    mv, mn, sv = [case[k].reshape(n, 3).copy() for k in ("model_vertex", "model_normal", "src_vertex")]
    miss = rng.random(n) < 0.1
    mv[miss] = np.nan
    mn[miss] = np.nan
    mn[rng.random(n) < 0.03] = 0.0
    mn[rng.random(n) < 0.01, 1] = np.inf
    kind = rng.random(n)
    sv[kind < 0.04] = 0.0
    sv[(kind >= 0.04) & (kind < 0.06), 0] = np.nan
    sv[(kind >= 0.06) & (kind < 0.08), 1] = np.inf
    sv[(kind >= 0.08) & (kind < 0.10), 2] = -np.inf
    sv[(kind >= 0.10) & (kind < 0.12), 2] *= -1.0
    # source normals in the source camera frame: the world axis normal of the source's own wall would need the true pose; a
    # perturbed copy of the model normal of the same pixel, turned into the camera frame by the model pose, is as good a test
    Rm = case["model_row"][:9].reshape(3, 3)
    base = np.nan_to_num(case["model_normal"].reshape(n, 3).astype(np.float64), nan=0.0, posinf=0.0) @ Rm.T
    sn = base + rng.normal(size=(n, 3)) * 0.25
    with np.errstate(invalid="ignore", divide="ignore"):
        sn = sn / np.linalg.norm(sn, axis=1, keepdims=True)
    sn = sn.astype(np.float32)
    sn[rng.random(n) < 0.05] = 0.0
    sn[rng.random(n) < 0.02, 2] = np.nan
    case.update(model_vertex=mv.reshape(h, w, 3), model_normal=mn.reshape(h, w, 3), src_vertex=sv.reshape(h, w, 3),
                src_normal=sn.reshape(h, w, 3))
    c2w_model = TR.inverse_pose(case["model_row"])
    shift = np.eye(4)
    shift[0, 3] = 3.0
    case["S"] = {"truth": TR.inverse_pose(case["true_row"]), "offset": c2w_model, "behind": c2w_model @ rot_y(np.pi),
                 "shifted": c2w_model @ shift}
    return case


def run_accumulate(ctx, L, case, S, src_normal, dist_max, cos_min, d_src, d_mv, d_mn, d_sn, d_match, d_res):
    h, w = case["src_vertex"].shape[:2]
    cam = ctx.camera(h, w, *case["K"])
    sums = np.zeros(29)
    pose, S = np.ascontiguousarray(case["model_row"]), np.ascontiguousarray(S)
    L.check(ctx.lib.r3d_track_accumulate(ctx.handle, cam.handle, d_src, d_sn if src_normal else None, d_mv, d_mn, pose.ctypes.data,
                                         S.ctypes.data, dist_max, cos_min, sums.ctypes.data, d_match, d_res))
    return sums


def assert_sums(got, want):
    np.testing.assert_allclose(got, want, rtol=1e-11, atol=1e-11 * max(np.abs(want).max(), 1e-300))


@pytest.mark.parametrize("h,w", RASTERS)
def test_match_residual_and_sums_against_reference(R, L, ctx, h, w):
    case = dirty_case(h, w, 1)
    n = h * w
    ins = {k: Guarded(ctx, n * 12, off, case[k], seed=s) for s, (k, off) in
           enumerate([("src_vertex", 0), ("src_normal", 4), ("model_vertex", 8), ("model_normal", 4)])}
    made = list(ins.values())
    codes = set()
    try:
        combos = list(itertools.product(["truth", "offset", "behind", "shifted"], [None, -1.0, 0.9, 1.0]))
        for k, (which, cos_min) in enumerate(combos):
            S = case["S"][which]
            with_n = cos_min is not None
            cm = -1.0 if cos_min is None else cos_min
            ref = TR.associate(case["src_vertex"], case["src_normal"] if with_n else None, case["model_vertex"], case["model_normal"],
                               case["model_row"], S, case["K"], 0.5, cm)
            assert TR.rounding_margin(ref.upv) >= 1e-9, (which, TR.rounding_margin(ref.upv))
            codes |= set(ref.match[ref.match < 0].tolist())
            g_match, g_res = Guarded(ctx, n * 4, OFFSETS[k % 3], seed=10 + k), Guarded(ctx, n * 4, OFFSETS[(k + 1) % 3], seed=40 + k)
            made += [g_match, g_res]
            sums = run_accumulate(ctx, L, case, S, with_n, 0.5, cm, ins["src_vertex"].ptr, ins["model_vertex"].ptr,
                                  ins["model_normal"].ptr, ins["src_normal"].ptr, g_match.ptr, g_res.ptr)
            got_match, got_res = g_match.read(np.int32), g_res.read(np.uint32)
            assert np.array_equal(got_match, ref.match), (which, cos_min, np.flatnonzero(got_match != ref.match)[:5])
            assert np.array_equal(got_res, bits(ref.residual)), (which, cos_min)
            assert_sums(sums, ref.sums)
            if which == "truth" and cos_min is None:
                if n >= 1023:
                    assert (ref.match >= 0).sum() >= 0.4 * n
                # all subsets of the optional outputs: the sums are the same bits, a present output the same bits
                for use_m, use_r in [(False, False), (True, False), (False, True)]:
                    gm, gr = Guarded(ctx, n * 4, 8, seed=70), Guarded(ctx, n * 4, 0, seed=71)
                    made += [gm, gr]
                    s2 = run_accumulate(ctx, L, case, S, False, 0.5, cm, ins["src_vertex"].ptr, ins["model_vertex"].ptr,
                                        ins["model_normal"].ptr, None, gm.ptr if use_m else None, gr.ptr if use_r else None)
                    assert s2.tobytes() == sums.tobytes()
                    if use_m:
                        assert np.array_equal(gm.read(np.int32), ref.match)
                    else:
                        gm.unchanged()
                    if use_r:
                        assert np.array_equal(gr.read(np.uint32), bits(ref.residual))
                    else:
                        gr.unchanged()
                # two runs, and a run under other tuning values: the same bits
                for key, value in [(None, 0), ("apply_blocks", 7), ("fuse_blocks", 3), ("nn_variant", 2)]:
                    if key:
                        ctx.set_tuning(key, value)
                    try:
                        s3 = run_accumulate(ctx, L, case, S, False, 0.5, cm, ins["src_vertex"].ptr, ins["model_vertex"].ptr,
                                            ins["model_normal"].ptr, None, None, None)
                    finally:
                        if key:
                            ctx.set_tuning(key, 0)
                    assert s3.tobytes() == sums.tobytes(), key
        if n >= 1023:
            assert codes == {-1, -2, -3, -4, -5}, codes
        for g in ins.values():
            g.unchanged()
    finally:
        for g in made:
            g.free()


@pytest.fixture(scope="module")
def analytic48():
    case = TR.analytic_case(48, 64, 2.0, 1.0, (0.03, 0.02, -0.04))
    case["S"] = TR.inverse_pose(case["model_row"])
    case["ref_T"], case["ref_info"] = TR.loop(case["src_vertex"], None, case["model_vertex"], case["model_normal"], case["model_row"],
                                              case["S"], case["K"], 0.5, -1.0, 10)
    return case


def test_iterate_against_accumulate_and_reference_loop(R, L, ctx, tracking, analytic48):
    icp = importlib.import_module(PKG + ".icp")
    case = analytic48
    dev = tracking.TrackDevice(case["src_vertex"], case["model_vertex"], case["model_normal"], case["model_row"], case["S"], case["K"],
                               ctx=ctx)
    try:
        sums, match, _ = dev.sums(0.5)
        T_want, rms_want = icp.plane_step_from_sums(sums)
        dev.iterate(1, 0.5)
        st = dev.state()
        assert st["iterations"] == 1 and not st["degenerate"] and st["pairs"] == sums[0]
        np.testing.assert_allclose(st["T_step"], T_want, atol=1e-10, rtol=0)
        np.testing.assert_allclose(st["T_total"], T_want, atol=1e-10, rtol=0)
        assert abs(st["rms"] - rms_want) <= 1e-10
        dev.state_reset()
        dev.iterate(10, 0.5)
        st = dev.state()
        assert st["iterations"] == 10 and not st["degenerate"] and len(st["rms_history"]) == 10
        np.testing.assert_allclose(st["T_total"], case["ref_T"], atol=2e-6, rtol=0)
        after = TR.pose_error(dev.pose(), case["true_row"])
        print("device loop 48x64: %.5f deg / %.6f m, %d pairs" % (after[0], after[1], st["pairs"]))
        assert after[0] < 0.05 and after[1] < 0.002 and st["pairs"] >= 0.8 * 48 * 64
        # the same loop in two calls continues from the state; a second device run gives the same bits
        first = dev.d_state.download(np.float64, 512).tobytes()
        # ... and so does a run whose state lies in a guard-banded buffer at offset 8: all 512 doubles written, nothing else
        g_state = Guarded(ctx, 512 * 8, 8, seed=90)
        try:
            L.check(ctx.lib.r3d_icp_state_reset(ctx.handle, g_state.ptr))
            pose, S = np.ascontiguousarray(case["model_row"]), np.ascontiguousarray(case["S"])
            L.check(ctx.lib.r3d_track_iterate(ctx.handle, dev.cam.handle, dev.d_src_vertex.ptr, None, dev.d_model_vertex.ptr,
                                              dev.d_model_normal.ptr, pose.ctypes.data, S.ctypes.data, 0.5, -1.0, 10, g_state.ptr))
            assert g_state.bytes().tobytes() == first
        finally:
            g_state.free()
        dev.state_reset()
        dev.iterate(4, 0.5)
        dev.iterate(6, 0.5)
        assert dev.d_state.download(np.float64, 512).tobytes() == first
    finally:
        dev.free()


def room_volume(R, ctx, vs, tr, **kw):
    syn = importlib.import_module(PKG + ".synthetic")
    lo, hi = syn.ROOM_LO - 0.3, syn.ROOM_HI + 0.3
    dims = tuple(int(np.ceil((hi[a] - lo[a]) / vs - 1e-9)) for a in range(3))
    return R.TSDFVolume(tuple(lo), vs, dims, tr, ctx=ctx, **kw)


@pytest.mark.parametrize("color", [False, True])
def test_frame_to_model_on_a_real_volume(R, ctx, color):
    """The setup of test_gpu_raycast.test_frame_to_model_registration.  The reference loop over raycast_ref maps of this scene
    (CPU, 96 x 128, vs 0.05) goes from 2.0000 degrees / 0.05000 m to 0.02496 degrees / 0.000771 m in 10 iterations (DESIGN
    4.5m): the device is gated at 4 x that, and its pose must equal the reference loop's over the device's own maps."""
    syn = importlib.import_module(PKG + ".synthetic")
    H, W, n_frames, i = 96, 128, 16, 2
    depths, quats, ts, K = syn.room_views(n_frames, H, W, seed=0)
    poses = R.poses_w2c(quats, ts)
    V = room_volume(R, ctx, 0.05, 0.2, color=color)
    if color:
        V.integrate(depths, quats, ts, intrinsics=K, rgb=np.full(depths.shape + (3,), 128, np.uint8))
    else:
        V.integrate(depths, quats, ts, intrinsics=K)
    T_i = TR.pose_matrix(poses[i])
    c_i = -T_i[:3, :3].T @ T_i[:3, 3]
    z, q_new, t_new, _ = syn.room_view(H, W, 2 * np.pi * i / n_frames + 0.1 + np.radians(2.0), c_i + np.array([0.03, 0.0, 0.04]))
    true_row = TR.pose_row(q_new, t_new)
    frame = z.astype(np.float32)
    before = TR.pose_error(poses[i], true_row)
    assert abs(before[0] - 2.0) < 1e-6 and abs(before[1] - 0.05) < 1e-9
    row, info = V.track(frame, poses[i], intrinsics=K)
    after = TR.pose_error(row, true_row)
    print("frame-to-model: rotation %.4f -> %.5f degrees, centre %.4f -> %.6f m, %d pairs" % (before[0], after[0], before[1], after[1], info["pairs"]))
    assert info["status"] == 0 and info["iterations"] == 10
    assert after[0] < before[0] and after[1] < before[1]
    assert after[0] < 4 * 0.02496 and after[1] < 4 * 0.000771
    # the reference loop over the maps the device itself made
    _, vertex, normal = V.raycast(quats[i:i + 1], ts[i:i + 1], (H, W), intrinsics=K)
    sv = R.unproject(frame, intrinsics=K).reshape(H, W, 3)
    want, winfo = TR.track(sv, None, vertex[0], normal[0], poses[i], K, 2 * 0.2, -1.0, 10)
    assert winfo["status"] == 0
    np.testing.assert_allclose(row, want, atol=2e-6, rtol=0)
    if not color:
        # with the normal gate: still converges, fewer pairs
        row2, info2 = V.track(frame, poses[i], intrinsics=K, max_angle_deg=30.0)
        after2 = TR.pose_error(row2, true_row)
        assert info2["status"] == 0 and 0 < info2["pairs"] <= info["pairs"]
        assert after2[0] < before[0] and after2[1] < before[1]
        # an empty volume: nothing to track against -> status 1, the guess comes back bit for bit
        V.reset()
        row3, info3 = V.track(frame, poses[i], intrinsics=K)
        assert info3["status"] == 1 and info3["pairs"] == 0 and row3.tobytes() == poses[i].tobytes()
    V.close()


def small_motion_sequence(n, h, w):
    syn = importlib.import_module(PKG + ".synthetic")
    frames = [syn.room_view(h, w, 0.9 + np.radians(2.0) * k, np.array([0.3, -0.1, 0.4]) + k * np.array([0.03, 0.01, -0.04])) for k in range(n)]
    return (np.stack([f[0].astype(np.float32) for f in frames]), np.stack([TR.pose_row(f[1], f[2]) for f in frames]), frames[0][3],
            [f[1] for f in frames], [f[2] for f in frames])


def surface_count(V):
    return V.extract_points_device(1.0, None, None, 0)


def test_track_and_integrate_small_motions(R, ctx):
    """8 frames of 48 x 64, 2 degrees of yaw and 0.051 m apart, vs 0.1, tr 0.3.  The reference loop on the CPU (raycast_ref +
    tsdf_ref + track_ref) keeps every centre within 0.0047 m and ends with 2128 surface points against 2129 with the true poses:
    the bounds are one voxel and 5 %."""
    depths, truth, K, quats, ts = small_motion_sequence(8, 48, 64)
    V = room_volume(R, ctx, 0.1, 0.3)
    rows = V.track_and_integrate(depths, truth[0], intrinsics=K)
    n_tracked = surface_count(V)
    V.reset()
    V.integrate(depths, np.array(quats), np.array(ts), intrinsics=K)
    n_true = surface_count(V)
    assert rows.shape == (8, 12) and rows[0].tobytes() == truth[0].tobytes()
    errs = [TR.pose_error(rows[k], truth[k]) for k in range(8)]
    print("track_and_integrate: worst centre error %.5f m, worst rotation %.4f degrees, %d / %d points" %
          (max(e[1] for e in errs), max(e[0] for e in errs), n_tracked, n_true))
    assert max(e[1] for e in errs) <= 0.1
    assert abs(n_tracked - n_true) <= 0.05 * n_true
    # a frame that cannot be tracked stops the loop with a clear exception
    V.reset()
    blank = depths.copy()
    blank[3] = 0.0
    with pytest.raises(RuntimeError, match="frame 3"):
        V.track_and_integrate(blank, truth[0], intrinsics=K)
    V.close()


def test_track_and_integrate_room_views(R, ctx):
    """8 synthetic.room_views frames of 48 x 64 from the true first pose, vs 0.1, tr 0.3.  Consecutive frames of that sequence
    are 45 degrees of yaw and up to 2 m apart -- far outside what projective association without a pyramid can follow.  The
    reference loop on the CPU (raycast_ref + tsdf_ref + track_ref) finishes all 8 frames with status 0, its worst centre error
    is 2.645 m (frame 7; one voxel is 0.1 m) and it ends with 4504 surface points against 10748 with the true poses (58 %
    fewer).  One voxel and 5 % are out of reach for the method on this sequence, so the bounds are what the reference achieves
    plus a margin: 3.0 m and 65 %.  The loop must complete: any exception fails the test."""
    syn = importlib.import_module(PKG + ".synthetic")
    depths, quats, ts, K = syn.room_views(8, 48, 64, seed=0)
    truth = R.poses_w2c(quats, ts)
    V = room_volume(R, ctx, 0.1, 0.3)
    rows = V.track_and_integrate(depths, truth[0], intrinsics=K)
    n_tracked = surface_count(V)
    V.reset()
    V.integrate(depths, quats, ts, intrinsics=K)
    n_true = surface_count(V)
    V.close()
    worst = max(TR.pose_error(rows[k], truth[k])[1] for k in range(8))
    print("room_views: worst centre error %.4f m, %d / %d points" % (worst, n_tracked, n_true))
    assert rows.shape == (8, 12) and rows[0].tobytes() == truth[0].tobytes()
    assert worst <= 3.0 and abs(n_tracked - n_true) <= 0.65 * n_true


def test_invalid_calls_write_nothing(R, L, ctx, tracking):
    h, w = 5, 7
    case = dirty_case(h, w, 2)
    n = h * w
    cam = ctx.camera(h, w, *case["K"])
    other = R.Context(0)
    cam_other = other.camera(h, w, *case["K"])
    made = []
    try:
        g = {k: Guarded(ctx, n * 12, 0, case[k]) for k in ("src_vertex", "src_normal", "model_vertex", "model_normal")}
        gm, gr, gs = Guarded(ctx, n * 4, 0, seed=5), Guarded(ctx, n * 4, 4, seed=6), Guarded(ctx, 512 * 8, 8, seed=7)
        made = list(g.values()) + [gm, gr, gs]
        pose, S = np.ascontiguousarray(case["model_row"]), np.ascontiguousarray(case["S"]["offset"])
        sums = np.full(29, 7.0)
        good = dict(ctx=ctx.handle, cam=cam.handle, sv=g["src_vertex"].ptr, sn=g["src_normal"].ptr, mv=g["model_vertex"].ptr,
                    mn=g["model_normal"].ptr, pose=pose.ctypes.data, S=S.ctypes.data, dist=0.5, cos=0.5)
        order = ["ctx", "cam", "sv", "sn", "mv", "mn", "pose", "S", "dist", "cos"]
        bad = [dict(ctx=None), dict(cam=None), dict(cam=cam_other.handle), dict(sv=None), dict(mv=None), dict(mn=None), dict(pose=None),
               dict(S=None), dict(dist=0.0), dict(dist=-1.0), dict(dist=float("inf")), dict(dist=float("nan")), dict(cos=1.5),
               dict(cos=-1.5), dict(cos=float("nan"))]
        for b in bad:
            a = {**good, **b}
            args = [a[k] for k in order]
            assert ctx.lib.r3d_track_accumulate(*args, sums.ctypes.data, gm.ptr, gr.ptr) == L.ERR_INVALID, b
            assert ctx.lib.r3d_track_iterate(*args, 1, gs.ptr) == L.ERR_INVALID, b
        args = [good[k] for k in order]
        assert ctx.lib.r3d_track_accumulate(*args, None, gm.ptr, gr.ptr) == L.ERR_INVALID
        assert ctx.lib.r3d_track_accumulate(*args, sums.ctypes.data, g["src_vertex"].ptr, gr.ptr) == L.ERR_INVALID      # output over an input
        assert ctx.lib.r3d_track_accumulate(*args, sums.ctypes.data, gm.ptr, g["model_normal"].ptr + 8) == L.ERR_INVALID
        assert ctx.lib.r3d_track_accumulate(*args, sums.ctypes.data, gm.ptr, gm.ptr + 4) == L.ERR_INVALID               # outputs overlap
        assert ctx.lib.r3d_track_iterate(*args, 1, None) == L.ERR_INVALID
        assert ctx.lib.r3d_track_iterate(*args, -1, gs.ptr) == L.ERR_INVALID
        assert ctx.lib.r3d_track_iterate(*args, 512 - 48 + 1, gs.ptr) == L.ERR_INVALID
        assert ctx.lib.r3d_track_iterate(*args, 1, g["model_vertex"].ptr) == L.ERR_INVALID
        assert np.all(sums == 7.0)
        for x in made:
            x.unchanged()
        assert ctx.lib.r3d_track_iterate(*args, 0, gs.ptr) == L.OK                                                      # a valid no-op
        gs.unchanged()
        # r3d_tsdf_track
        V = room_volume(R, ctx, 0.5, 1.0)
        d_depth = Guarded(ctx, n * 4, 0, np.ones((h, w), np.float32))
        made.append(d_depth)
        out, info = np.full(12, 7.0), np.full(4, 7.0)
        inf = float("inf")
        tgood = dict(vol=V.handle, cam=cam.handle, depth=d_depth.ptr, dt=L.DEPTH_F32, scale=1.0, guess=pose.ctypes.data, mw=1.0, step=0.5,
                     tn=0.0, tf=inf, mj=0.05, dist=0.5, cos=-1.0, it=2, out=out.ctypes.data, info=info.ctypes.data)
        torder = ["vol", "cam", "depth", "dt", "scale", "guess", "mw", "step", "tn", "tf", "mj", "dist", "cos", "it", "out", "info"]
        nan_guess = np.full(12, np.nan)
        tbad = [dict(vol=None), dict(cam=None), dict(cam=cam_other.handle), dict(depth=None), dict(dt=9), dict(guess=None),
                dict(guess=nan_guess.ctypes.data), dict(mw=0.0), dict(step=0.0), dict(tn=-1.0), dict(tn=2.0, tf=1.0), dict(mj=-1.0),
                dict(dist=0.0), dict(dist=inf), dict(cos=2.0), dict(cos=float("nan")), dict(it=-1), dict(it=465), dict(out=None),
                dict(info=None), dict(out=info.ctypes.data), dict(out=pose.ctypes.data)]
        for b in tbad:
            a = {**tgood, **b}
            assert ctx.lib.r3d_tsdf_track(*[a[k] for k in torder]) == L.ERR_INVALID, b
        assert np.all(out == 7.0) and np.all(info == 7.0)
        d_depth.unchanged()
        V.close()
    finally:
        for x in made:
            x.free()
        other.close()


def test_command_line_with_track_flag(R, ctx, tmp_path):
    """--track reconstructs from 8-bit depth maps and the first pose; without the flag the tool's output is what it was."""
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
    plain = subprocess.run([sys.executable, tool] + args, cwd=str(work), env=env, capture_output=True, text=True, timeout=300)
    assert plain.returncode == 0, plain.stdout[-1000:] + plain.stderr[-2000:]
    plain_ply = (work / "ply" / "tsdf_surface.ply").read_bytes()
    assert sorted(os.listdir(str(work / "camera_pose"))) == ["image_colmap_simi_2.txt"] and "tracked" not in plain.stdout
    # the same call through the library: the tool without the flag writes what it always wrote
    names, quats, ts = R.read_pose_file(str(work / "camera_pose" / "image_colmap_simi_2.txt"))
    depths = R.cloud_io.read_depth_batch([str(work / "depth" / nm) for nm in names])
    V = R.TSDFVolume([float(v) for v in origin], 4.0, [int(d) for d in dims], 12.0, ctx=ctx)
    V.integrate(depths, quats, ts, intrinsics=K)
    xyz, nrm = V.extract_point_cloud(1.0)
    V.close()
    R.cloud_io.write_ply_normals(str(tmp_path / "want.ply"), xyz, nrm)
    assert plain_ply == (tmp_path / "want.ply").read_bytes()
    shutil.rmtree(str(work / "ply"))
    r = subprocess.run([sys.executable, tool] + args + ["--track"], cwd=str(work), env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-1000:] + r.stderr[-2000:]
    assert r.stdout.strip().split("\n")[-1] == "tracked %d frames -> ./camera_pose/image_colmap_simi_2_tracked.txt" % n
    assert sorted(os.listdir(str(work / "ply"))) == ["tsdf_surface.ply"]
    names2, quats2, ts2 = R.read_pose_file(str(work / "camera_pose" / "image_colmap_simi_2_tracked.txt"))
    assert names2 == names
    got, want = R.poses_w2c(quats2, ts2), R.poses_w2c(quats, ts)
    np.testing.assert_allclose(got[0], want[0], atol=1e-12)
    errs = [TR.pose_error(got[k], want[k]) for k in range(n)]
    print("--track: worst centre error %.3f units (voxel 4), worst rotation %.4f degrees" % (max(e[1] for e in errs), max(e[0] for e in errs)))
    assert max(e[1] for e in errs) <= 4.0 and max(e[0] for e in errs) <= 1.0
    # a pose file without rows: the identity is the first pose and ./depth/ lists the frames; the poses found are the true ones
    # relative to frame 0 (a volume around a camera at the origin)
    bare = tmp_path / "bare"
    shutil.copytree(str(work / "depth"), str(bare / "depth"))
    os.makedirs(str(bare / "camera_pose"))
    (bare / "camera_pose" / "image_colmap_simi_2.txt").write_text(rows[0] + "\n")
    args0 = ["--voxel-size", "4", "--trunc", "12", "--origin", "-280", "-280", "-280", "--dims", "140", "140", "140", "--track"]
    r0 = subprocess.run([sys.executable, tool] + args0, cwd=str(bare), env=env, capture_output=True, text=True, timeout=300)
    assert r0.returncode == 0, r0.stdout[-1000:] + r0.stderr[-2000:]
    names0, quats0, ts0 = R.read_pose_file(str(bare / "camera_pose" / "image_colmap_simi_2_tracked.txt"))
    assert names0 == names
    got0 = R.poses_w2c(quats0, ts0)
    np.testing.assert_allclose(got0[0], np.concatenate([np.eye(3).reshape(9), np.zeros(3)]), atol=1e-12)
    T0 = TR.pose_matrix(want[0])
    for k in range(n):
        rel = TR.pose_matrix(want[k]) @ np.linalg.inv(T0)          # frame-0 camera -> frame-k camera
        e = TR.pose_error(got0[k], np.concatenate([rel[:3, :3].reshape(9), rel[:3, 3]]))
        assert e[1] <= 4.0 and e[0] <= 1.0, (k, e)
