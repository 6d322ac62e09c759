"""GPU: the depth bilateral filter (csrc/r3d_bilateral.hip) bit for bit against tests/bilateral_ref.py, the NumPy restatement of
include/r3d.h "Depth bilateral filter", fed with the library's own weight tables; its guard bands, invalid calls and repeatability;
and bilateral= of TSDFVolume.track / track_and_integrate: radius 0 against the plain call byte for byte, the pose against the
reference loop over the device's own maps (one level, a pyramid, the colour term), the volume against integrating the raw frames,
and the command line."""
import importlib
import os
import subprocess
import sys

import numpy as np
import pytest

import bilateral_ref as BR
import photo_ref as PH
import pyramid_ref as PR
import track_ref as TR
from helpers import PKG, ROOT, r3d as _r3d
from test_gpu_bounds import Guarded
from test_gpu_track import room_volume, small_motion_sequence
from test_gpu_track_color import CORRIDOR_MAX_JUMP, corridor_volume, quats_ts
from test_gpu_track_pyramid import device_levels

pytestmark = pytest.mark.gpu

F = np.float32
# every tile edge (32 x 8) and one more / one less: 1 x 1; one row; 5 x 3; 7 x 31 and 9 x 33 either side of one tile, 8 x 32 the tile
# itself; 17 x 65: three tiles each way, the last one pixel wide / tall; 48 x 64: whole tiles only, 12 workgroups
RASTERS = [(1, 1), (1, 7), (5, 3), (7, 31), (8, 32), (9, 33), (17, 65), (48, 64)]
# radius -> (sigma_s, sigma_r): depths lie in 0.5 .. 4 m, so every cut (3 sigma_r) keeps some taps and rejects others; radius 8 has a
# halo (16 rows) taller than a tile
PARAMS = {0: (1.0, 1.0), 1: (0.8, 0.2), 3: (2.0, 0.4), 8: (4.0, 0.7)}


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
    """random depths in 0.5 .. 4 m, a tenth of them invalid in every way: 0, negative, NaN, +inf, -inf"""
    rng = np.random.default_rng([seed, h, w])
    d = rng.uniform(0.5, 4.0, size=(h, w)).astype(F)
    kind = rng.random((h, w))
    for k, bad in enumerate([0.0, -1.5, np.nan, np.inf, -np.inf]):
        d[(kind >= 0.02 * k) & (kind < 0.02 * (k + 1))] = bad
    return d


def step_raster(h, w):
    return (np.where(np.arange(w)[None, :] < (w + 1) // 3, F(1.0), F(2.0)) * np.ones((h, 1), F)).astype(F)


@pytest.mark.parametrize("h,w", RASTERS)
def test_filter_against_reference(L, ctx, tracking, h, w):
    d = dirty_depth(h, w, 1)
    ok = BR.valid(d)
    vertex = np.random.default_rng([2, h, w]).normal(size=(h, w, 3)).astype(F)
    vertex[..., 2] = d
    made = []
    try:
        for radius, (ss, sr) in PARAMS.items():
            tables = tracking.bilateral_weights(radius, ss, sr)
            want = bits(BR.depth_bilateral(d, radius, *tables)).reshape(-1)
            for k, (stride, in_off, out_off) in enumerate([(1, 0, 0), (1, 4, 4), (3, 0, 4), (3, 4, 0)]):
                g_in = Guarded(ctx, h * w * 4 * stride, in_off, d if stride == 1 else vertex, seed=k)
                g_out = Guarded(ctx, h * w * 4, out_off, seed=20 + k)
                made += [g_in, g_out]
                call = (ctx.handle, g_in.ptr + (8 if stride == 3 else 0), stride, h, w, radius, ss, sr, g_out.ptr)
                L.check(ctx.lib.r3d_depth_bilateral(*call))
                got = g_out.read(np.uint32)                                    # ... and both guard bands are untouched
                assert np.array_equal(got, want), (radius, stride, in_off, out_off, np.flatnonzero(got != want)[:5])
                g_in.unchanged()
                L.check(ctx.lib.r3d_depth_bilateral(*call))
                assert np.array_equal(g_out.read(np.uint32), got)                  # the same bytes on a repeat
            out = want.view(F).reshape(h, w)
            assert np.all(want.reshape(h, w)[~ok] == 0)
            if radius == 0:
                assert np.array_equal(bits(out[ok]), bits(d[ok]))
            elif h * w >= 200:
                assert (out[ok] != d[ok]).any()                                # the filter did something
        if (h, w) == (17, 65):
            ss, sr = PARAMS[3]
            assert np.array_equal(bits(tracking.depth_bilateral(d, 3, ss, sr, ctx=ctx)), bits(BR.depth_bilateral(d, 3, *tracking.bilateral_weights(3, ss, sr))))
    finally:
        for g in made:
            g.free()


@pytest.mark.parametrize("h,w", [(9, 33), (48, 64)])
def test_radius_zero_and_the_step_raster(ctx, tracking, h, w):
    d = dirty_depth(h, w, 3)
    ok = BR.valid(d)
    out = tracking.depth_bilateral(d, 0, 1.0, 1.0, ctx=ctx)
    assert np.array_equal(bits(out[ok]), bits(d[ok])) and np.all(bits(out[~ok]) == 0)
    # depths 1.0 | 2.0 with cut = 0.3 m: the two sides never mix, and powers of two make every weighted mean exact
    step = step_raster(h, w)
    for radius in (0, 1, 3, 8):
        assert np.array_equal(bits(tracking.depth_bilateral(step, radius, 1.7, 0.1, ctx=ctx)), bits(step)), radius
    assert (tracking.depth_bilateral(step, 3, 1.7, 0.5, ctx=ctx) != step).any()   # ... and with cut = 1.5 m they do


def test_invalid_calls_write_nothing(R, L, ctx):
    h, w = 5, 8
    d = dirty_depth(h, w, 4)
    g_in, g_out = Guarded(ctx, h * w * 4, 0, d), Guarded(ctx, h * w * 4, 0, seed=4)
    g_vertex = Guarded(ctx, h * w * 12 + h * w * 4 + 64, 0, seed=5)
    fresh = R.Context(0)
    try:
        good = dict(ctx=ctx.handle, din=g_in.ptr, stride=1, h=h, w=w, r=2, ss=1.5, sr=0.3, out=g_out.ptr)
        order = ["ctx", "din", "stride", "h", "w", "r", "ss", "sr", "out"]
        inf, nan = float("inf"), float("nan")
        # a context that has filtered nothing yet holds no tables: the values that mark that state (radius -1, both sigmas 0) are
        # invalid arguments like any others, on it and on a context that has tables
        for c in (fresh, ctx):
            for b in (dict(r=-1, ss=0.0, sr=0.0), dict(r=-1), dict(ss=0.0, sr=0.0), dict(r=0, ss=0.0, sr=0.0)):
                a = {**good, **b, "ctx": c.handle}
                assert c.lib.r3d_depth_bilateral(*[a[k] for k in order]) == L.ERR_INVALID, b
            c.sync()
        g_out.unchanged()
        bad = [dict(ctx=None), dict(din=None), dict(out=None), dict(stride=2), dict(stride=0), dict(stride=-1), dict(stride=4), dict(h=0),
               dict(w=0), dict(h=-3), dict(w=-1), dict(r=-1), dict(r=9), dict(r=1 << 20), dict(ss=0.0), dict(ss=-1.0), dict(ss=inf),
               dict(ss=nan), dict(sr=0.0), dict(sr=-0.3), dict(sr=inf), dict(sr=nan), dict(sr=1e-40), dict(sr=1e39),
               dict(out=g_in.ptr), dict(out=g_in.ptr + h * w * 4 - 4), dict(out=g_in.ptr - h * w * 4 + 4), dict(din=g_out.ptr + 12, h=2, w=2),
               dict(h=1 << 16, w=1 << 15),                                                                # 2^31 pixels
               dict(h=1, w=(1 << 31) - 1024), dict(h=(1 << 31) - 1024, w=1), dict(h=1 << 10, w=(1 << 21) - 1),   # the limit itself
               # stride 3 reaches ((h w - 1) 3 + 1) floats: an output behind the stride-1 extent but inside that one
               dict(din=g_vertex.ptr + 8, stride=3, out=g_vertex.ptr + h * w * 4 + 64),
               dict(din=g_vertex.ptr + 8, stride=3, out=g_vertex.ptr + 8 + ((h * w - 1) * 3) * 4)]
        for b in bad:
            a = {**good, **b}
            assert ctx.lib.r3d_depth_bilateral(*[a[k] for k in order]) == L.ERR_INVALID, b
        for g in (g_in, g_out, g_vertex):
            g.unchanged()
        # ... and the first byte behind the stride-3 extent is a valid output
        a = {**good, **dict(din=g_vertex.ptr + 8, stride=3, out=g_vertex.ptr + 8 + ((h * w - 1) * 3 + 1) * 4)}
        assert ctx.lib.r3d_depth_bilateral(*[a[k] for k in order]) == L.OK
        ctx.sync()
        # the fresh context's first valid call is served from tables it uploads itself
        assert fresh.lib.r3d_depth_bilateral(*[{**good, "ctx": fresh.handle}[k] for k in order]) == L.OK
        want = BR.depth_bilateral(d, 2, *importlib.import_module(PKG + ".tracking").bilateral_weights(2, 1.5, 0.3))
        fresh.sync()
        assert np.array_equal(g_out.read(np.uint32), bits(want).reshape(-1))
    finally:
        for g in (g_in, g_out, g_vertex):
            g.free()
        fresh.close()


def test_tables_follow_the_parameters(ctx, tracking):
    """the context keeps the tables of the last (radius, sigma_s, sigma_r): alternating parameters must not serve stale ones"""
    d = dirty_depth(17, 65, 5)
    cases = [(3, 2.0, 0.4), (3, 2.0, 0.7), (3, 1.0, 0.7), (8, 1.0, 0.7), (1, 1.0, 0.7), (3, 2.0, 0.4)]
    want = [bits(BR.depth_bilateral(d, c[0], *tracking.bilateral_weights(*c))) for c in cases]
    assert len({w.tobytes() for w in want}) == 5
    for _ in range(2):
        for c, w in zip(cases, want):
            assert np.array_equal(bits(tracking.depth_bilateral(d, *c, ctx=ctx)), w), c
            assert np.array_equal(bits(tracking.depth_bilateral(d, *c, ctx=ctx)), w), c


# ---- bilateral= of the tracking calls ------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def scene(R, ctx):
    """bilateral_ref.room_frame: the volume of test_gpu_track.test_frame_to_model_on_a_real_volume, a clean and a noisy new frame"""
    s = BR.room_frame()
    V = room_volume(R, ctx, 0.05, 0.2)
    V.integrate(s["depths"], s["quats"], s["ts"], intrinsics=s["K"])
    i = s["i"]
    s.update(V=V, guess=R.poses_w2c(s["quats"], s["ts"])[i].copy(), quat=s["quats"][i:i + 1], t=s["ts"][i:i + 1])
    yield s
    V.close()


def filtered_vertex_map(R, tracking, s, frame, bilateral, depth_scale=1.0):
    """the source vertex map track(bilateral=) works on, from the device's own calls: unproject, filter the z column, unproject"""
    sv0 = R.unproject(frame, intrinsics=s["K"], depth_scale=depth_scale).reshape(s["H"], s["W"], 3)
    filtered = tracking.depth_bilateral(np.ascontiguousarray(sv0[..., 2]), *bilateral, ctx=s["V"].ctx)
    return R.unproject(filtered, intrinsics=s["K"]).reshape(s["H"], s["W"], 3), filtered


def test_radius_zero_tracks_as_the_plain_call(scene):
    """an f32 frame at scale 1 only: other dtypes pass through an f32 rounding of z before x and y are formed"""
    V, K = scene["V"], scene["K"]
    for frame in (scene["clean"], scene["noisy"]):
        for kwargs in (dict(), dict(max_angle_deg=30.0), dict(pyramid_iters=(4, 3))):
            row, info = V.track(frame, scene["guess"], intrinsics=K, **kwargs)
            row0, info0 = V.track(frame, scene["guess"], intrinsics=K, bilateral=(0, 1, 1), **kwargs)
            assert info["status"] == 0 and row0.tobytes() == row.tobytes() and info0 == info, kwargs


def test_track_on_the_noisy_frame_against_reference_loop(R, tracking, scene):
    """in this room the filter does not improve the pose (the noise is zero-mean over 12 000 pairs; the filter's bias at
    the room's edges costs about a millimetre), so no pose gain is asserted: the pose must be the reference loop's over the
    device's own maps, and the loop must still converge.  What the filter is for -- the normals -- is gated on the CPU
    (test_bilateral_host) and seen here as the pairs that pass a 30 degree gate."""
    V, K, frame = scene["V"], scene["K"], scene["noisy"]
    before = TR.pose_error(scene["guess"], scene["true_row"])
    row, info = V.track(frame, scene["guess"], intrinsics=K, bilateral=BR.FILTER)
    after = TR.pose_error(row, scene["true_row"])
    assert info["status"] == 0 and info["iterations"] == 10
    assert after[0] < before[0] and after[1] < before[1]
    sv, filtered = filtered_vertex_map(R, tracking, scene, frame, BR.FILTER)
    assert np.array_equal(bits(filtered), bits(BR.depth_bilateral(frame, BR.FILTER[0], *tracking.bilateral_weights(*BR.FILTER))))
    _, vertex, normal = V.raycast(scene["quat"], scene["t"], (scene["H"], scene["W"]), intrinsics=K)
    want, winfo = TR.track(sv, None, vertex[0], normal[0], scene["guess"], K, 2 * 0.2, -1.0, 10)
    assert winfo["status"] == 0 and winfo["pairs"] == info["pairs"]
    np.testing.assert_allclose(row, want, atol=2e-6, rtol=0)
    assert abs(info["rms"] - winfo["rms"]) <= 2e-6
    # the raw frame, for the record, and the 30 degree normal gate on both
    raw, raw_info = V.track(frame, scene["guess"], intrinsics=K)
    gated, gated_info = V.track(frame, scene["guess"], intrinsics=K, max_angle_deg=30.0)
    gated_f, gated_f_info = V.track(frame, scene["guess"], intrinsics=K, max_angle_deg=30.0, bilateral=BR.FILTER)
    print("noisy frame: raw %s rms %.5f | filtered %s rms %.5f | 30 degree gate: raw %d pairs %s, filtered %d pairs %s"
          % (TR.pose_error(raw, scene["true_row"]), raw_info["rms"], after, info["rms"], gated_info["pairs"],
             TR.pose_error(gated, scene["true_row"]), gated_f_info["pairs"], TR.pose_error(gated_f, scene["true_row"])))
    assert gated_info["status"] == 0 and gated_f_info["status"] == 0
    # a u16 frame in millimetres goes the same way: unprojected with its scale, z filtered, the loop on f32 metres
    mm = np.round(frame * 1000.0).astype(np.uint16)
    row_mm, info_mm = V.track(mm, scene["guess"], intrinsics=K, depth_scale=0.001, bilateral=BR.FILTER)
    sv_mm, _ = filtered_vertex_map(R, tracking, scene, mm, BR.FILTER, depth_scale=0.001)
    want_mm, winfo_mm = TR.track(sv_mm, None, vertex[0], normal[0], scene["guess"], K, 2 * 0.2, -1.0, 10)
    assert info_mm["status"] == 0 and winfo_mm["pairs"] == info_mm["pairs"]
    np.testing.assert_allclose(row_mm, want_mm, atol=2e-6, rtol=0)
    # the Python layer's refusals
    for bad in [(9, 1.0, 1.0), (-1, 1.0, 1.0), (1.5, 1.0, 1.0), (1, 0.0, 1.0), (1, 1.0, float("nan")), (1, 1.0), 3]:
        with pytest.raises(ValueError):
            V.track(frame, scene["guess"], intrinsics=K, bilateral=bad)


def test_bilateral_with_a_pyramid(R, tracking, scene):
    V, K, frame, iters = scene["V"], scene["K"], scene["noisy"], (6, 4, 3)
    row, info = V.track(frame, scene["guess"], intrinsics=K, pyramid_iters=iters, bilateral=BR.FILTER)
    assert info["status"] == 0 and info["iterations"] == 13 and len(info["rms_history"]) == 13
    sv, _ = filtered_vertex_map(R, tracking, scene, frame, BR.FILTER)
    levels = device_levels(R, V, scene, sv, 3, 0.05)
    want, winfo = PR.track(levels, iters, scene["guess"], 2 * 0.2, -1.0)
    assert winfo["status"] == 0 and winfo["margin"] >= 1e-9, winfo["margin"]
    np.testing.assert_allclose(row, want, atol=2e-6, rtol=0)
    np.testing.assert_allclose(info["rms_history"], winfo["rms_history"], atol=2e-6, rtol=0)
    plain, _ = V.track(frame, scene["guess"], intrinsics=K, pyramid_iters=iters)
    assert plain.tobytes() != row.tobytes()                                     # the filter took part


def test_bilateral_with_the_colour_term(R, ctx, tracking):
    """the corridor of test_gpu_track_color.test_corridor_end_to_end, tracked with rgb= on a filtered frame"""
    bilateral = (2, 1.5, 0.1)
    depths, rgbs, rows, K = PH.corridor_frames([0.0, 0.1, 0.2, 0.3])
    d_new, rgb_new, true_row, _ = PH.corridor_view(0.4)
    guess = rows[-1]
    H, W = PH.CORRIDOR_SHAPE
    quats, ts = quats_ts(R, rows)
    V = corridor_volume(R, ctx, True)
    try:
        V.integrate(depths, quats, ts, intrinsics=K, rgb=rgbs)
        row, info = V.track(d_new, guess, intrinsics=K, max_jump=CORRIDOR_MAX_JUMP, rgb=rgb_new, bilateral=bilateral)
        assert info["status"] == 0 and info["iterations"] == 10 and info["photo_pairs"] > 0
        depth, vertex, normal, rgb = V.raycast(quats[-1:], ts[-1:], (H, W), intrinsics=K, with_colors=True)
        sv0 = R.unproject(d_new, intrinsics=K).reshape(H, W, 3)
        filtered = tracking.depth_bilateral(np.ascontiguousarray(sv0[..., 2]), *bilateral, ctx=ctx)
        assert (filtered != sv0[..., 2]).any()
        sv = R.unproject(filtered, intrinsics=K).reshape(H, W, 3)
        Is, _ = PH.intensity_map(rgb_new, sv[..., 2], CORRIDOR_MAX_JUMP)
        _, packed = PH.intensity_map(rgb[0], depth[0], CORRIDOR_MAX_JUMP)
        want, winfo = PH.track(sv, None, vertex[0], normal[0], guess, K, 2 * PH.CORRIDOR_TR, -1.0, 10, Is, packed, tracking.PHOTO_WEIGHT,
                               tracking.I_MAX)
        assert winfo["status"] == 0 and winfo["photo_pairs"] == info["photo_pairs"] and winfo["pairs"] == info["pairs"]
        np.testing.assert_allclose(row, want, atol=2e-6, rtol=0)
    finally:
        V.close()


def test_track_and_integrate_integrates_the_raw_frames(R, ctx):
    depths, truth, K, _, _ = small_motion_sequence(5, 48, 64)
    noisy = np.stack([BR.noisy(depths[k], 0.003, 10 + k) for k in range(5)])
    bilateral = (2, 1.5, 0.05)
    V = room_volume(R, ctx, 0.1, 0.3)
    try:
        rows = V.track_and_integrate(noisy, truth[0], intrinsics=K, bilateral=bilateral)
        tsdf, weight = V.volume()
        assert rows.shape == (5, 12) and rows[0].tobytes() == truth[0].tobytes()
        assert max(TR.pose_error(rows[k], truth[k])[1] for k in range(5)) <= 0.1       # one voxel, as test_gpu_track asks
        # the raw frames at the poses it returned: the same volume, byte for byte
        V.reset()
        cam = ctx.camera(48, 64, *K)
        buf = ctx.alloc(noisy.nbytes).upload(noisy)
        V.integrate_device(cam, buf.ptr, np.float32, 5, rows)
        tsdf_raw, weight_raw = V.volume()
        buf.free()
        assert tsdf.tobytes() == tsdf_raw.tobytes() and weight.tobytes() == weight_raw.tobytes() and weight.max() > 1
        # ... and the filter did take part in the tracking
        V.reset()
        plain = V.track_and_integrate(noisy, truth[0], intrinsics=K)
        assert plain[1:].tobytes() != rows[1:].tobytes()
        with pytest.raises(ValueError):
            V.track_and_integrate(noisy, truth[0], intrinsics=K, bilateral=(9, 1.0, 1.0))
    finally:
        V.close()


def test_command_line_with_track_bilateral(R, ctx, tmp_path):
    """--track --track-bilateral R,SIGMA_S,SIGMA_R on 8-bit depth maps (the room in units of 2.5 cm, as
    test_gpu_track_pyramid.test_command_line_with_track_pyramid): the tool's poses are the library's for the same call."""
    from PIL import Image
    syn = importlib.import_module(PKG + ".synthetic")
    H, W, n, scale = 48, 64, 4, 40.0
    lo, hi = syn.ROOM_LO * scale, syn.ROOM_HI * scale
    frames = [syn.room_view(H, W, 0.9 + np.radians(2.0) * k, (np.array([0.3, -0.1, 0.4]) + k * np.array([0.03, 0.01, -0.04])) * scale,
                            lo=lo, hi=hi) for k in range(n)]
    K = frames[0][3]
    work = tmp_path / "work"
    os.makedirs(str(work / "depth"))
    os.makedirs(str(work / "camera_pose"))
    lines = ["id,tx,ty,tz,qx,qy,qz,qw,name,tail"]
    for k, (z, q, t, _) in enumerate(frames):
        Image.fromarray(np.clip(np.round(z), 0, 255).astype(np.uint8), mode="L").save(str(work / "depth" / ("%03d.png" % k)))
        lines.append(",".join([str(k + 1)] + [repr(float(v)) for v in t] + [repr(float(v)) for v in q] + ["%03d.png" % k, "x"]))
    (work / "camera_pose" / "image_colmap_simi_2.txt").write_text("\n".join(lines) + "\n")
    tool = os.path.join(ROOT, PKG, "other_tools", "integrate_tsdf.py")
    origin = [str(v) for v in lo - 12.0]
    dims = [str(int(np.ceil((hi[a] - lo[a] + 24.0) / 4.0))) for a in range(3)]
    args = ["--voxel-size", "4", "--trunc", "12", "--origin"] + origin + ["--dims"] + dims
    env = dict(os.environ, PYTHONPATH=ROOT, R3D_FX=repr(K[0]), R3D_FY=repr(K[1]), R3D_CX=repr(K[2]), R3D_CY=repr(K[3]))
    r = subprocess.run([sys.executable, tool] + args + ["--track", "--track-bilateral", "2,1.5,2.0"], cwd=str(work), env=env,
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-1000:] + r.stderr[-2000:]
    assert r.stdout.strip().split("\n")[-1] == "tracked %d frames -> ./camera_pose/image_colmap_simi_2_tracked.txt" % n
    names, quats, ts = R.read_pose_file(str(work / "camera_pose" / "image_colmap_simi_2.txt"))
    names2, quats2, ts2 = R.read_pose_file(str(work / "camera_pose" / "image_colmap_simi_2_tracked.txt"))
    assert names2 == names
    got, want = R.poses_w2c(quats2, ts2), R.poses_w2c(quats, ts)
    errs = [TR.pose_error(got[k], want[k]) for k in range(n)]
    assert max(e[1] for e in errs) <= 4.0 and max(e[0] for e in errs) <= 1.0             # one voxel, one degree
    depths = R.cloud_io.read_depth_batch([str(work / "depth" / nm) for nm in names])
    V = R.TSDFVolume([float(v) for v in origin], 4.0, [int(d) for d in dims], 12.0, ctx=ctx)
    lib_rows = V.track_and_integrate(depths, want[0], intrinsics=K, bilateral=(2, 1.5, 2.0))
    V.reset()
    plain_rows = V.track_and_integrate(depths, want[0], intrinsics=K)
    V.close()
    assert max(TR.pose_error(got[k], lib_rows[k])[1] for k in range(n)) <= 1e-6
    assert plain_rows[1:].tobytes() != lib_rows[1:].tobytes()
    # the flag needs --track, and a well-formed value
    for extra, message in ((["--track-bilateral", "2,1.5,2.0"], "--track-bilateral needs --track"),
                           (["--track", "--track-bilateral", "2,1.5"], "--track-bilateral takes"),
                           (["--track", "--track-bilateral", "9,1.5,2.0"], "--track-bilateral takes")):
        r2 = subprocess.run([sys.executable, tool] + args + extra, cwd=str(work), env=env, capture_output=True, text=True, timeout=300)
        assert r2.returncode == 2 and message in r2.stderr, r2.stderr[-500:]
