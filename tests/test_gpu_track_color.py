"""GPU: tracking with a photometric term (csrc/r3d_photo.hip, track_kernel<true> and its drivers in csrc/r3d_track.hip) against
tests/photo_ref.py, the NumPy restatement of include/r3d.h "TSDF colour tracking": the intensity maps and the per-pixel intensity
differences bit for bit, match and residual against r3d_track_accumulate itself, the 31 sums at the tolerance of the 29, the
device-resident loop against the reference loop, and the whole step in a textured corridor where depth alone cannot see along
the axis."""
import importlib
import itertools
import os
import subprocess
import sys

import numpy as np
import pytest

import photo_ref as PR
import track_ref as TR
from helpers import PKG, ROOT, r3d as _r3d
from test_gpu_bounds import Guarded

pytestmark = pytest.mark.gpu

F = np.float32
RASTERS = [(1, 1), (3, 5), (31, 33), (32, 32), (25, 41), (48, 64)]   # 1023, 1024 and 1025 px: the tile edge; 48 x 64: three tiles
W_PHOTO = 1e-4
CORRIDOR_MAX_JUMP = 0.3      # at 48 x 64 neighbouring pixels of the far walls are up to 0.2 m apart in depth
# the NumPy reference's own result on the CPU (test_photo_host.py's corridor: ray cast, maps and loop all by the references):
# the along-axis error goes from -0.10000 m to -0.00502 m.  The device's bound is 2 x that: f32 ray-cast differences only.
REF_ALONG_AXIS = 0.00502


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


def assert_sums(got, want):
    np.testing.assert_allclose(got, want, rtol=1e-11, atol=1e-11 * max(np.abs(want).max(), 1e-300))


def map_inputs(h, w, seed):
    """a colour image and a validity raster with everything a raster carries: zeros, negatives, NaN, +-inf, steps in depth"""
    rng = np.random.default_rng([seed, h, w, 9])
    rgb = rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
    d = (1.0 + 0.02 * rng.random((h, w)) + 0.3 * (rng.random((h, w)) < 0.15)).astype(F)
    kind = rng.random((h, w))
    for lo, val in [(0.00, 0.0), (0.03, -1.0), (0.05, np.nan), (0.07, np.inf), (0.09, -np.inf)]:
        d[(kind >= lo) & (kind < lo + 0.02)] = val
    return rgb, d


@pytest.mark.parametrize("h,w", RASTERS)
def test_intensity_map_bit_for_bit(L, ctx, h, w):
    rgb, d = map_inputs(h, w, 3)
    n = h * w
    vertex = np.full((h, w, 3), 7.0, F)
    vertex[..., 2] = d
    g_rgb, g_d, g_v = Guarded(ctx, n * 3, 1, rgb, seed=1), Guarded(ctx, n * 4, 4, d, seed=2), Guarded(ctx, n * 12, 8, vertex, seed=3)
    made = [g_rgb, g_d, g_v]
    try:
        for k, (stride, mj) in enumerate(itertools.product([1, 3], [0.0, 0.05, float("inf")])):
            want_I, want_P = PR.intensity_map(rgb, d, mj)
            if n >= 1023 and mj == 0.05:
                assert np.isfinite(want_P[..., 1]).sum() >= 0.2 * n and np.isnan(want_P[..., 1]).sum() >= 0.2 * n
            valid = g_d.ptr if stride == 1 else g_v.ptr + 8
            for use_i, use_p in [(True, True), (True, False), (False, True), (False, False)]:
                g_i, g_p = Guarded(ctx, n * 4, 4 * (k % 3), seed=10 + k), Guarded(ctx, n * 16, 16 * (k % 2), seed=20 + k)
                made += [g_i, g_p]
                L.check(ctx.lib.r3d_intensity_map(ctx.handle, g_rgb.ptr, valid, stride, h, w, mj, g_i.ptr if use_i else None,
                                                  g_p.ptr if use_p else None))
                if use_i:
                    assert np.array_equal(g_i.read(np.uint32), bits(want_I).reshape(-1)), (stride, mj)
                else:
                    g_i.unchanged()
                if use_p:
                    assert np.array_equal(g_p.read(np.uint32), bits(want_P).reshape(-1)), (stride, mj)
                else:
                    g_p.unchanged()
        for g in (g_rgb, g_d, g_v):
            g.unchanged()
    finally:
        for g in made:
            g.free()


@pytest.mark.parametrize("h,w", RASTERS)
def test_accumulate_rgb_against_reference_and_depth_only_call(L, ctx, h, w):
    case = PR.dirty_case(h, w, 1)
    n = h * w
    ins = {k: Guarded(ctx, n * size, off, case[k], seed=s) for s, (k, size, off) in
           enumerate([("src_vertex", 12, 0), ("src_normal", 12, 4), ("model_vertex", 12, 8), ("model_normal", 12, 4),
                      ("src_intensity", 4, 4), ("model_packed", 16, 16)])}
    made = list(ins.values())
    cam = ctx.camera(h, w, *case["K"])
    pose = np.ascontiguousarray(case["model_row"])
    reasons = {k: 0 for k in PR.REASONS}

    def run(S, with_n, cm, w_photo, outs):
        S = np.ascontiguousarray(S)
        maps = (ins["src_vertex"].ptr, ins["src_normal"].ptr if with_n else None, ins["model_vertex"].ptr, ins["model_normal"].ptr,
                pose.ctypes.data, S.ctypes.data, 0.5, cm)
        sums = np.zeros(31)
        L.check(ctx.lib.r3d_track_accumulate_rgb(ctx.handle, cam.handle, *maps, ins["src_intensity"].ptr, ins["model_packed"].ptr, w_photo,
                                                 PR.DIRTY_I_MAX, sums.ctypes.data, *outs))
        return sums, maps

    try:
        combos = list(itertools.product(["truth", "offset", "behind", "shifted"], [None, -1.0, 0.9, 1.0]))
        for k, (which, cos_min) in enumerate(combos):
            S = case["S"][which]
            with_n = cos_min is not None
            cm = -1.0 if cos_min is None else cos_min
            ref = PR.associate(case["src_vertex"], case["src_normal"] if with_n else None, case["model_vertex"], case["model_normal"],
                               case["model_row"], S, case["K"], 0.5, cm, case["src_intensity"], case["model_packed"], W_PHOTO,
                               PR.DIRTY_I_MAX)
            assert TR.rounding_margin(ref.upv) >= 1e-9 and ref.floor_margin >= 1e-9 and ref.i_max_margin >= 1e-9, (which, cos_min)
            for name in reasons:
                reasons[name] += ref.reasons[name]
            outs = [Guarded(ctx, n * 4, 4 * ((k + a) % 3), seed=10 * a + k) for a in range(3)]
            made += outs
            sums, maps = run(S, with_n, cm, W_PHOTO, [g.ptr for g in outs])
            # match and residual: the bits of the depth-only call on the same inputs
            gm, gr = Guarded(ctx, n * 4, 0, seed=50 + k), Guarded(ctx, n * 4, 8, seed=60 + k)
            made += [gm, gr]
            sums29 = np.zeros(29)
            L.check(ctx.lib.r3d_track_accumulate(ctx.handle, cam.handle, *maps, sums29.ctypes.data, gm.ptr, gr.ptr))
            assert outs[0].bytes().tobytes() == gm.bytes().tobytes() and outs[1].bytes().tobytes() == gr.bytes().tobytes()
            assert np.array_equal(outs[0].read(np.int32), ref.match)
            assert np.array_equal(outs[2].read(np.uint32), bits(ref.photo)), (which, cos_min)
            assert_sums(sums, ref.sums)
            # w_photo = 0: the first 29 sums are the depth-only call's bits; the photometric count and sum stay
            sums0, _ = run(S, with_n, cm, 0.0, [None, None, None])
            assert sums0[:29].tobytes() == sums29.tobytes(), (which, cos_min)
            assert sums0[29:].tobytes() == sums[29:].tobytes()
            if which == "truth" and cos_min is None:
                if n >= 1023:
                    assert ref.sums[29] >= 0.25 * n
                # every subset of the optional outputs: the same sums, a present output the same bits, an absent one untouched
                for use in itertools.product([False, True], repeat=3):
                    sub = [Guarded(ctx, n * 4, 4 * a, seed=70 + a) for a in range(3)]
                    made += sub
                    s2, _ = run(S, with_n, cm, W_PHOTO, [g.ptr if u else None for g, u in zip(sub, use)])
                    assert s2.tobytes() == sums.tobytes()
                    for g, u, o in zip(sub, use, outs):
                        if u:
                            assert g.bytes().tobytes() == o.bytes().tobytes()
                        else:
                            g.unchanged()
                # a second run, and runs under other tuning values: the same bytes
                for key, value in [(None, 0), ("apply_blocks", 7), ("fuse_blocks", 3), ("nn_variant", 2)]:
                    if key:
                        ctx.set_tuning(key, value)
                    try:
                        s3, _ = run(S, with_n, cm, W_PHOTO, [None, None, None])
                    finally:
                        if key:
                            ctx.set_tuning(key, 0)
                    assert s3.tobytes() == sums.tobytes(), key
        if n >= 1023:
            assert all(v > 0 for v in reasons.values()), reasons
        for g in ins.values():
            g.unchanged()
    finally:
        for g in made:
            g.free()


def test_iterate_rgb_against_reference_loop(ctx, tracking):
    """48 x 64 analytic room maps with a smooth colour pattern on both sides.  atol 2e-6 on T_total: the bound of the depth-only
    iterate test (the tree-ordered device sums against plain fp64 sums, through 10 solves)."""
    h, w = 48, 64
    case = TR.analytic_case(h, w, 2.0, 1.0, (0.03, 0.02, -0.04))
    dirty = PR.dirty_case(h, w, 4)
    Rm, tm = case["model_row"][:9].reshape(3, 3), case["model_row"][9:]
    model_depth = (case["model_vertex"].reshape(-1, 3).astype(np.float64) @ Rm[2] + tm[2]).astype(F).reshape(h, w)
    Is, _ = PR.intensity_map(dirty["src_rgb"], case["src_vertex"][..., 2], PR.DIRTY_MAX_JUMP)
    _, packed = PR.intensity_map(dirty["model_rgb"], model_depth, PR.DIRTY_MAX_JUMP)
    S = TR.inverse_pose(case["model_row"])
    want, winfo = PR.loop(case["src_vertex"], None, case["model_vertex"], case["model_normal"], case["model_row"], S, case["K"], 0.5, -1.0,
                          10, Is, packed, W_PHOTO, PR.DIRTY_I_MAX)
    assert winfo["status"] == 0 and winfo["photo_pairs"] >= 0.25 * h * w
    dev = tracking.TrackDevice(case["src_vertex"], case["model_vertex"], case["model_normal"], case["model_row"], S, case["K"], ctx=ctx,
                               src_intensity=Is, model_packed=packed)
    try:
        dev.iterate_rgb(10, 0.5, photo_weight=W_PHOTO, i_max=PR.DIRTY_I_MAX)
        st = dev.state()
        assert st["iterations"] == 10 and not st["degenerate"] and len(st["rms_history"]) == 10 and st["pairs"] == winfo["pairs"]
        np.testing.assert_allclose(st["T_total"], want[0:16].reshape(4, 4), atol=2e-6, rtol=0)
        first = dev.d_state.download(np.float64, 512).tobytes()
        dev.state_reset()
        dev.iterate_rgb(4, 0.5, photo_weight=W_PHOTO, i_max=PR.DIRTY_I_MAX)
        dev.iterate_rgb(6, 0.5, photo_weight=W_PHOTO, i_max=PR.DIRTY_I_MAX)
        assert dev.d_state.download(np.float64, 512).tobytes() == first
        # one pass of the loop is the one-pass form's sums, solved
        dev.state_reset()
        sums, _, _, photo = dev.sums_rgb(0.5, photo_weight=W_PHOTO, i_max=PR.DIRTY_I_MAX)
        assert np.isfinite(photo).sum() == sums[29]
        icp = importlib.import_module(PKG + ".icp")
        T1, _ = icp.plane_step_from_sums(sums[:29])
        dev.iterate_rgb(1, 0.5, photo_weight=W_PHOTO, i_max=PR.DIRTY_I_MAX)
        np.testing.assert_allclose(dev.state()["T_total"], T1, atol=1e-10, rtol=0)
        # a device without the two maps has no colour term
        plain = tracking.TrackDevice(case["src_vertex"], case["model_vertex"], case["model_normal"], case["model_row"], S, case["K"], ctx=ctx)
        with pytest.raises(ValueError):
            plain.iterate_rgb(1, 0.5)
        plain.free()
    finally:
        dev.free()


def corridor_volume(R, ctx, color):
    return R.TSDFVolume(PR.CORRIDOR_ORIGIN, PR.CORRIDOR_VS, PR.CORRIDOR_DIMS, PR.CORRIDOR_TR, ctx=ctx, color=color)


def quats_ts(R, rows):
    tool = importlib.import_module(PKG + ".other_tools.integrate_tsdf")
    return np.array([tool.quat_xyzw(r[:9].reshape(3, 3)) for r in rows]), np.array([r[9:] for r in rows])


def test_corridor_end_to_end(R, ctx, tracking):
    depths, rgbs, rows, K = PR.corridor_frames([0.0, 0.1, 0.2, 0.3])
    d_new, rgb_new, true_row, _ = PR.corridor_view(0.4)
    guess = rows[-1]
    H, W = PR.CORRIDOR_SHAPE
    quats, ts = quats_ts(R, rows)
    np.testing.assert_allclose(R.poses_w2c(quats, ts), rows, atol=1e-12)
    V = corridor_volume(R, ctx, True)
    V.integrate(depths, quats, ts, intrinsics=K, rgb=rgbs)
    before = PR.along_axis_error(guess, true_row)
    # depth alone: singular, or solved and nowhere nearer along the axis
    row_d, info_d = V.track(d_new, guess, intrinsics=K, max_jump=CORRIDOR_MAX_JUMP)
    after_d = PR.along_axis_error(row_d, true_row)
    assert info_d["status"] == 1 or abs(after_d) >= 0.9 * abs(before), (info_d, after_d)
    # with the colour term
    row_c, info_c = V.track(d_new, guess, intrinsics=K, max_jump=CORRIDOR_MAX_JUMP, rgb=rgb_new)
    after_c = PR.along_axis_error(row_c, true_row)
    print("corridor on the device: along-axis error %.5f -> depth only %.5f (status %d), with colour %.5f; %d photometric pairs, rms %.2f"
          % (before, after_d, info_d["status"], after_c, info_c["photo_pairs"], info_c["photo_rms"]))
    assert info_c["status"] == 0 and info_c["iterations"] == 10 and info_c["photo_pairs"] > 0
    assert abs(after_c) <= 2 * REF_ALONG_AXIS, after_c
    # the reference loop over the maps the device itself made
    depth, vertex, normal, rgb = V.raycast(quats[-1:], ts[-1:], (H, W), intrinsics=K, with_colors=True)
    sv = R.unproject(d_new, intrinsics=K).reshape(H, W, 3)
    Is, _ = PR.intensity_map(rgb_new, sv[..., 2], CORRIDOR_MAX_JUMP)
    _, packed = PR.intensity_map(rgb[0], depth[0], CORRIDOR_MAX_JUMP)
    want, winfo = PR.track(sv, None, vertex[0], normal[0], guess, K, 2 * PR.CORRIDOR_TR, -1.0, 10, Is, packed, tracking.PHOTO_WEIGHT,
                           tracking.I_MAX)
    assert winfo["status"] == 0 and winfo["photo_pairs"] == info_c["photo_pairs"] and winfo["pairs"] == info_c["pairs"]
    np.testing.assert_allclose(row_c, want, atol=2e-6, rtol=0)
    assert abs(info_c["photo_rms"] - winfo["photo_rms"]) <= 1e-6
    # the Python layer's refusals
    with pytest.raises(ValueError, match="pyramid"):
        V.track(d_new, guess, intrinsics=K, rgb=rgb_new, pyramid_iters=(4, 2))
    with pytest.raises(ValueError):
        V.track(d_new, guess, intrinsics=K, rgb=rgb_new[:-1])
    plain = corridor_volume(R, ctx, False)
    with pytest.raises(ValueError, match="colour"):
        plain.track(d_new, guess, intrinsics=K, rgb=rgb_new)
    plain.close()
    V.close()


def test_track_and_integrate_slides_along_the_corridor(R, ctx):
    zs = [0.06 * k for k in range(5)]
    depths, rgbs, rows, K = PR.corridor_frames(zs)
    V = corridor_volume(R, ctx, True)
    got = V.track_and_integrate(depths, rows[0], intrinsics=K, rgbs=rgbs, max_jump=CORRIDOR_MAX_JUMP)
    assert got.shape == (5, 12) and got[0].tobytes() == rows[0].tobytes()
    errs = [abs(PR.along_axis_error(got[k], rows[k])) for k in range(5)]
    print("track_and_integrate(rgbs=): along-axis errors %s" % ["%.4f" % e for e in errs])
    assert V.extract_points_device(1.0, None, None, 0) > 0
    V.close()
    # depth only: a frame is refused, or the poses stay where the first was along the axis
    P = corridor_volume(R, ctx, False)
    try:
        flat = P.track_and_integrate(depths, rows[0], intrinsics=K, max_jump=CORRIDOR_MAX_JUMP)
        assert abs(PR.along_axis_error(flat[-1], rows[-1])) >= 0.9 * zs[-1]
    except RuntimeError as e:
        assert "cannot be tracked" in str(e)
    P.close()
    with pytest.raises(ValueError):
        P2 = corridor_volume(R, ctx, False)
        try:
            P2.track_and_integrate(depths, rows[0], intrinsics=K, rgbs=rgbs)
        finally:
            P2.close()


def test_invalid_calls_write_nothing(R, L, ctx):
    h, w = 5, 7
    case = PR.dirty_case(h, w, 2)
    n = h * w
    cam = ctx.camera(h, w, *case["K"])
    other = R.Context(0)
    cam_other = other.camera(h, w, *case["K"])
    made = []
    try:
        g = {k: Guarded(ctx, n * size, 0, case[k]) for k, size in [("src_vertex", 12), ("src_normal", 12), ("model_vertex", 12),
                                                                    ("model_normal", 12), ("src_intensity", 4), ("model_packed", 16)]}
        g_rgb, g_d = Guarded(ctx, n * 3, 0, case["src_rgb"]), Guarded(ctx, n * 4, 0, case["model_depth"])
        gm, gr, gp, gs = [Guarded(ctx, nb, off, seed=s) for nb, off, s in [(n * 4, 0, 5), (n * 4, 4, 6), (n * 4, 8, 7), (512 * 8, 8, 8)]]
        gi, gk = Guarded(ctx, n * 4, 0, seed=9), Guarded(ctx, n * 16, 0, seed=10)
        made = list(g.values()) + [g_rgb, g_d, gm, gr, gp, gs, gi, gk]
        nan, inf = float("nan"), float("inf")
        # r3d_intensity_map
        mgood = dict(ctx=ctx.handle, rgb=g_rgb.ptr, valid=g_d.ptr, stride=1, h=h, w=w, mj=0.05, i=gi.ptr, p=gk.ptr)
        morder = ["ctx", "rgb", "valid", "stride", "h", "w", "mj", "i", "p"]
        for b in [dict(ctx=None), dict(rgb=None), dict(valid=None), dict(stride=0), dict(stride=2), dict(stride=4), dict(mj=-1.0),
                  dict(mj=nan), dict(h=0), dict(w=-1), dict(p=gk.ptr + 4), dict(p=gk.ptr + 8), dict(i=g_rgb.ptr), dict(i=g_d.ptr + 8),
                  dict(p=g_d.ptr - 16), dict(i=gk.ptr + 16), dict(h=1 << 16, w=1 << 15)]:
            a = {**mgood, **b}
            assert ctx.lib.r3d_intensity_map(*[a[k] for k in morder]) == L.ERR_INVALID, b
        # the two association calls
        pose, S = np.ascontiguousarray(case["model_row"]), np.ascontiguousarray(case["S"]["offset"])
        sums = np.full(31, 7.0)
        good = dict(ctx=ctx.handle, cam=cam.handle, sv=g["src_vertex"].ptr, sn=g["src_normal"].ptr, mv=g["model_vertex"].ptr,
                    mn=g["model_normal"].ptr, pose=pose.ctypes.data, S=S.ctypes.data, dist=0.5, cos=0.5, si=g["src_intensity"].ptr,
                    mp=g["model_packed"].ptr, wp=1e-4, im=20.0)
        order = ["ctx", "cam", "sv", "sn", "mv", "mn", "pose", "S", "dist", "cos", "si", "mp", "wp", "im"]
        bad = [dict(ctx=None), dict(cam=None), dict(cam=cam_other.handle), dict(sv=None), dict(mv=None), dict(mn=None), dict(pose=None),
               dict(S=None), dict(dist=0.0), dict(dist=inf), dict(dist=nan), dict(cos=1.5), dict(cos=nan), dict(si=None), dict(mp=None),
               dict(mp=g["model_packed"].ptr + 4), dict(wp=-1.0), dict(wp=inf), dict(wp=nan), dict(im=0.0), dict(im=-1.0), dict(im=inf),
               dict(im=nan)]
        for b in bad:
            a = {**good, **b}
            args = [a[k] for k in order]
            assert ctx.lib.r3d_track_accumulate_rgb(*args, sums.ctypes.data, gm.ptr, gr.ptr, gp.ptr) == L.ERR_INVALID, b
            assert ctx.lib.r3d_track_iterate_rgb(*args, 1, gs.ptr) == L.ERR_INVALID, b
        args = [good[k] for k in order]
        acc = ctx.lib.r3d_track_accumulate_rgb
        assert acc(*args, None, gm.ptr, gr.ptr, gp.ptr) == L.ERR_INVALID
        assert acc(*args, sums.ctypes.data, g["src_intensity"].ptr, gr.ptr, gp.ptr) == L.ERR_INVALID        # an output over a new input
        assert acc(*args, sums.ctypes.data, gm.ptr, gr.ptr, g["model_packed"].ptr + 32) == L.ERR_INVALID
        assert acc(*args, sums.ctypes.data, gm.ptr, gr.ptr, g["src_vertex"].ptr) == L.ERR_INVALID
        assert acc(*args, sums.ctypes.data, gm.ptr, gp.ptr + 4, gp.ptr) == L.ERR_INVALID                    # outputs overlap
        it = ctx.lib.r3d_track_iterate_rgb
        assert it(*args, 1, None) == L.ERR_INVALID and it(*args, -1, gs.ptr) == L.ERR_INVALID
        assert it(*args, 512 - 48 + 1, gs.ptr) == L.ERR_INVALID and it(*args, 1, g["model_packed"].ptr) == L.ERR_INVALID
        assert np.all(sums == 7.0)
        assert it(*args, 0, gs.ptr) == L.OK                                                                  # a valid no-op
        # r3d_tsdf_track_rgb
        V = R.TSDFVolume((-1.0, -1.0, 0.0), 0.5, (4, 4, 8), 1.0, ctx=ctx, color=True)
        P = R.TSDFVolume((-1.0, -1.0, 0.0), 0.5, (4, 4, 8), 1.0, ctx=ctx)
        g_depth = Guarded(ctx, n * 4, 0, np.ones((h, w), F))
        made.append(g_depth)
        out, info = np.full(12, 7.0), np.full(6, 7.0)
        tgood = dict(vol=V.handle, cam=cam.handle, depth=g_depth.ptr, dt=L.DEPTH_F32, scale=1.0, rgb=g_rgb.ptr, guess=pose.ctypes.data, mw=1.0,
                     step=0.5, tn=0.0, tf=inf, mj=0.05, dist=0.5, cos=-1.0, wp=1e-4, im=20.0, it=2, out=out.ctypes.data, info=info.ctypes.data)
        torder = ["vol", "cam", "depth", "dt", "scale", "rgb", "guess", "mw", "step", "tn", "tf", "mj", "dist", "cos", "wp", "im", "it", "out",
                  "info"]
        nan_guess = np.full(12, np.nan)
        tbad = [dict(vol=None), dict(vol=P.handle), dict(cam=None), dict(cam=cam_other.handle), dict(depth=None), dict(dt=9), dict(rgb=None),
                dict(guess=None), dict(guess=nan_guess.ctypes.data), dict(mw=0.0), dict(step=0.0), dict(tn=-1.0), dict(tn=2.0, tf=1.0),
                dict(mj=-1.0), dict(dist=0.0), dict(cos=2.0), dict(wp=-1.0), dict(wp=nan), dict(im=0.0), dict(im=inf), dict(it=-1),
                dict(it=465), dict(out=None), dict(info=None), dict(out=info.ctypes.data), dict(out=pose.ctypes.data)]
        for b in tbad:
            a = {**tgood, **b}
            assert ctx.lib.r3d_tsdf_track_rgb(*[a[k] for k in torder]) == L.ERR_INVALID, b
        assert np.all(out == 7.0) and np.all(info == 7.0)
        for x in made:
            x.unchanged()
        V.close()
        P.close()
    finally:
        for x in made:
            x.free()
        other.close()


def test_command_line_with_track_color(R, tmp_path):
    """--track --track-color reconstructs the corridor from 8-bit depth maps, colour images and the first pose; --track-color
    alone is refused.  The corridor in units of 2.5 cm, so that an 8-bit raster holds its depths."""
    from PIL import Image
    scale = 40.0
    zs = [0.06 * k for k in range(4)]
    depths, rgbs, rows, K = PR.corridor_frames(zs)
    quats, ts = quats_ts(R, rows)
    work = tmp_path / "work"
    for sub in ("depth", "camera_pose", "color"):
        os.makedirs(str(work / sub))
    lines = ["id,tx,ty,tz,qx,qy,qz,qw,name,tail"]
    for k in range(len(zs)):
        Image.fromarray(np.clip(np.round(depths[k] * scale), 0, 255).astype(np.uint8), mode="L").save(str(work / "depth" / ("%03d.png" % k)))
        Image.fromarray(rgbs[k], mode="RGB").save(str(work / "color" / ("%03d.png" % k)))
        lines.append(",".join([str(k + 1)] + [repr(float(v) * scale) for v in ts[k]] + [repr(float(v)) for v in quats[k]] + ["%03d.png" % k, "x"]))
    (work / "camera_pose" / "image_colmap_simi_2.txt").write_text("\n".join(lines) + "\n")
    tool = os.path.join(ROOT, PKG, "other_tools", "integrate_tsdf.py")
    args = ["--voxel-size", "2", "--trunc", "6", "--origin"] + [str(v * scale) for v in PR.CORRIDOR_ORIGIN] + \
           ["--dims"] + [str(d) for d in PR.CORRIDOR_DIMS]
    env = dict(os.environ, PYTHONPATH=ROOT, R3D_FX=repr(K[0]), R3D_FY=repr(K[1]), R3D_CX=repr(K[2]), R3D_CY=repr(K[3]))
    refused = subprocess.run([sys.executable, tool] + args + ["--track-color"], cwd=str(work), env=env, capture_output=True, text=True,
                             timeout=300)
    assert refused.returncode == 2 and "--track-color needs --track" in refused.stderr
    extra = ["--photo-weight", repr(1e-5 * scale * scale), "--track-max-jump", repr(CORRIDOR_MAX_JUMP * scale)]   # metres -> units
    r = subprocess.run([sys.executable, tool] + args + ["--track", "--track-color", "--color-dir", "./color/"] + extra, cwd=str(work), env=env,
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-1000:] + r.stderr[-2000:]
    assert r.stdout.strip().split("\n")[-1] == "tracked %d frames -> ./camera_pose/image_colmap_simi_2_tracked.txt" % len(zs)
    assert b"property uchar red" in (work / "ply" / "tsdf_surface.ply").read_bytes()[:400]
