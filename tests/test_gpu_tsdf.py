"""GPU: the TSDF volume against its NumPy reference (tests/tsdf_ref.py), BIT FOR BIT: tsdf, weight, point count, point order,
positions and normals.  The scenes are those of tests/test_tsdf_host.py, which asserts their conditions of the reference first.
Volume shapes put lane, pair, wave and workgroup tails on both sides of their limits; frame counts straddle the pose table's chunk.
No f32 denormal arises with these inputs (tsdf_ref.random_scene says why), so flush modes cannot show."""
import ctypes as C
import importlib
import os
import subprocess
import sys

import numpy as np
import pytest

import tsdf_ref as REF
from helpers import PKG, ROOT, r3d as _r3d
from test_gpu_bounds import Guarded

pytestmark = pytest.mark.gpu

DIMS = [(1, 1, 1), (3, 5, 7), (63, 2, 2), (64, 4, 4), (65, 3, 2), (129, 9, 5), (130, 9, 5)]
DTYPES = [np.uint8, np.uint16, np.float32]
RASTERS = [(24, 32), (48, 64)]


@pytest.fixture(scope="module")
def R():
    return _r3d()


@pytest.fixture(scope="module")
def L(R):
    return importlib.import_module(PKG + "._lib")


@pytest.fixture(scope="module")
def T(R):
    return importlib.import_module(PKG + ".tsdf")


@pytest.fixture(scope="module")
def ctx(R):
    c = R.Context(0)
    yield c
    c.close()


FRAMES = [1, 2, 17, 32, 33]          # 32 = the pose table's chunk (asserted against the package below)


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def device_volume(T, ctx, s):
    return T.TSDFVolume(s["origin"], s["vs"], s["dims"], s["tr"], ctx=ctx)


def integrate_device(ctx, V, s, lo=0, hi=None):
    """frames [lo, hi) of the scene through r3d_tsdf_integrate (rasters uploaded first)"""
    depths = s["depths"][lo:hi]
    f, h, w = depths.shape
    cam = ctx.camera(h, w, *s["K"])
    buf = ctx.alloc(max(depths.nbytes, 16)).upload(depths)
    V.integrate_device(cam, buf.ptr, depths.dtype, f, s["poses"][lo:hi], s["scale"])
    ctx.sync()
    buf.free()


def assert_volume(V, ref):
    tsdf, w = V.volume()
    assert tsdf.shape == ref.tsdf.shape
    assert np.array_equal(w, ref.w)
    assert np.array_equal(bits(tsdf), bits(ref.tsdf))


def assert_points(V, ref, min_weight=1.0):
    xyz, nrm = V.extract_point_cloud(min_weight)
    want_xyz, want_nrm = REF.extract(ref, min_weight)
    assert xyz.shape == want_xyz.shape, (xyz.shape, want_xyz.shape)
    assert np.array_equal(bits(xyz), bits(want_xyz)) and np.array_equal(bits(nrm), bits(want_nrm))
    return len(xyz)


def test_chunk_is_what_the_cases_assume(T):
    assert T.CHUNK == 32 and T.CHUNK in FRAMES and T.CHUNK + 1 in FRAMES


@pytest.mark.parametrize("n_frames", FRAMES)
@pytest.mark.parametrize("dims", DIMS)
def test_integration_and_extraction_match_the_reference(T, ctx, dims, n_frames):
    k = DIMS.index(dims) + FRAMES.index(n_frames)
    dtype, hw = DTYPES[k % 3], RASTERS[(k // 3) % 2]
    s = REF.random_scene(dims, n_frames, dtype, hw, seed=k)
    ref, passed, _, _ = REF.run(s)
    if dims != (1, 1, 1) and n_frames >= 17:
        assert 0 < passed < n_frames * ref.w.size             # some (voxel, frame) pairs pass, some are rejected
    V = device_volume(T, ctx, s)
    integrate_device(ctx, V, s)
    assert_volume(V, ref)
    for mw in sorted({1, 2, n_frames}):
        assert_points(V, ref, mw)
    V.close()


@pytest.mark.parametrize("hw", RASTERS)
@pytest.mark.parametrize("dtype", DTYPES)
def test_every_dtype_on_every_raster(T, ctx, dtype, hw):
    for dims in ((65, 3, 2), (130, 9, 5)):
        s = REF.random_scene(dims, 5, dtype, hw, seed=11)
        ref, passed, want_xyz, _ = REF.run(s)
        assert passed > 0
        if np.dtype(dtype) == np.float32:
            d = s["depths"]
            assert np.isnan(d).any() and (d == np.inf).any() and (d == -np.inf).any() and (d < 0).any() and (d == 0).any()
        else:
            assert (s["depths"] == 0).any()
        V = device_volume(T, ctx, s)
        integrate_device(ctx, V, s)
        assert_volume(V, ref)
        n = assert_points(V, ref)
        assert n > 0 or dims == (65, 3, 2)
        V.close()


def test_scene_covers_the_rejections():
    """the random scenes do exercise every early-out: behind the camera, outside the image, no measurement, behind the band"""
    F = np.float32
    s = REF.random_scene((130, 9, 5), 17, np.float32, (24, 32), seed=5)
    vol = REF.Volume(s["origin"], s["vs"], s["dims"], s["tr"])
    gx, gy, gz = vol.centres()
    X, Y, Z = gx[None, None, :], gy[None, :, None], gz[:, None, None]
    behind = outside = 0
    for p in s["poses"].astype(F):
        pz = ((p[6] * X + p[7] * Y) + p[8] * Z) + p[11]
        px = ((p[0] * X + p[1] * Y) + p[2] * Z) + p[9]
        behind += int((pz <= 0).sum())
        with np.errstate(all="ignore"):
            u = F(s["K"][0]) * (px / pz) + F(s["K"][2])
        outside += int(((pz > 0) & ((u + F(0.5) < 0) | (u + F(0.5) >= 32))).sum())
    assert behind > 0 and outside > 0
    assert REF.integrate(vol, s["depths"], s["poses"], s["K"], s["scale"]) > 0


def test_origin_offset_by_1e3(T, ctx):
    s = REF.random_scene((65, 3, 2), 6, np.float32, (24, 32), seed=21, offset=1e3)
    ref, passed, xyz, _ = REF.run(s)
    assert passed > 0 and len(xyz) > 0 and xyz[:, 0].min() > 990
    V = device_volume(T, ctx, s)
    integrate_device(ctx, V, s)
    assert_volume(V, ref)
    assert_points(V, ref)
    V.close()


def test_boundary_pixels(T, ctx):
    s = REF.boundary_scene()
    ref, _, _, _ = REF.run(s)
    V = device_volume(T, ctx, s)
    integrate_device(ctx, V, s)
    assert_volume(V, ref)
    assert_points(V, ref)
    V.close()


def test_unseen_volume_stays_zero_and_reset_restores_zero_bytes(T, ctx):
    s = REF.random_scene((17, 4, 3), 5, np.uint16, (24, 32), seed=3, unseen=True)
    V = device_volume(T, ctx, s)
    integrate_device(ctx, V, s)
    p, n = V.device_view()
    assert n == 17 * 4 * 3

    def raw():
        out = np.empty(n * 8, np.uint8)
        ctx.lib.r3d_download(ctx.handle, out.ctypes.data, p, out.nbytes)
        return out
    assert not raw().any()
    xyz, nrm = V.extract_point_cloud()
    assert xyz.shape == (0, 3) and nrm.shape == (0, 3)
    seen = REF.random_scene((17, 4, 3), 5, np.uint16, (24, 32), seed=3)
    integrate_device(ctx, V, seen)
    assert raw().any()
    V.reset()
    ctx.sync()
    assert not raw().any()
    # and the volume is as good as new
    integrate_device(ctx, V, seen)
    assert_volume(V, REF.run(seen)[0])
    V.close()


@pytest.mark.parametrize("dims,n_frames", [((65, 3, 2), 33), ((130, 9, 5), 17), ((64, 4, 4), 40)])
def test_split_invariance_and_repeatability(T, ctx, dims, n_frames):
    s = REF.random_scene(dims, n_frames, np.uint8, (24, 32), seed=31)
    ref = REF.run(s)[0]
    whole = device_volume(T, ctx, s)
    integrate_device(ctx, whole, s)
    assert_volume(whole, ref)
    again = device_volume(T, ctx, s)                      # a second run gives the same bits
    integrate_device(ctx, again, s)
    assert_volume(again, ref)
    single = device_volume(T, ctx, s)                     # F calls of one frame
    for f in range(n_frames):
        integrate_device(ctx, single, s, f, f + 1)
    assert_volume(single, ref)
    for cut in (1, n_frames // 2, n_frames - 1, 32 if n_frames > 32 else 3):   # two calls split anywhere
        two = device_volume(T, ctx, s)
        integrate_device(ctx, two, s, 0, cut)
        integrate_device(ctx, two, s, cut, n_frames)
        assert_volume(two, ref)
        two.close()
    host = device_volume(T, ctx, s)                       # the *_host entry point: the same launches behind an upload
    cam = ctx.camera(24, 32, *s["K"])
    L_ = importlib.import_module(PKG + "._lib")
    L_.check(ctx.lib.r3d_tsdf_integrate_host(host.handle, cam.handle, s["depths"].ctypes.data, L_.DEPTH_U8, n_frames, s["scale"],
                                             np.ascontiguousarray(s["poses"]).ctypes.data))
    assert_volume(host, ref)
    for v in (whole, again, single, host):
        v.close()


def test_extraction_caps_and_guard_bands(T, L, ctx):
    s = REF.random_scene((129, 9, 5), 6, np.float32, (24, 32), seed=41)
    ref, _, want_xyz, want_nrm = REF.run(s)
    n = len(want_xyz)
    assert n > 10
    V = device_volume(T, ctx, s)
    integrate_device(ctx, V, s)
    for cap in (0, n - 1, n, n + 1):
        room = n + 3
        gx, gn = Guarded(ctx, room * 12, seed=cap), Guarded(ctx, room * 12, off=4, seed=cap + 1)
        before_x, before_n = gx.bytes().copy(), gn.bytes().copy()
        got = V.extract_points_device(1.0, gx.ptr, gn.ptr, cap)
        assert got == n                                   # always the true count
        after_x, after_n = gx.bytes(), gn.bytes()         # (asserts the guard bands)
        rows = min(cap, n)
        assert np.array_equal(after_x[:rows * 12].view(np.uint32).reshape(-1, 3), bits(want_xyz[:rows]))
        assert np.array_equal(after_n[:rows * 12].view(np.uint32).reshape(-1, 3), bits(want_nrm[:rows]))
        assert np.array_equal(after_x[rows * 12:], before_x[rows * 12:]) and np.array_equal(after_n[rows * 12:], before_n[rows * 12:])
    # positions alone
    gx = Guarded(ctx, n * 12, seed=9)
    assert V.extract_points_device(1.0, gx.ptr, None, n) == n
    assert np.array_equal(gx.bytes().view(np.uint32).reshape(-1, 3), bits(want_xyz))
    V.close()


def test_crossings_on_the_last_voxel_of_each_axis(T, ctx):
    """the last voxel of an axis has no neighbour beyond: no point along that axis from it, and its gradient takes its own tsdf
    on that side"""
    s = REF.random_scene((8, 6, 5), 9, np.float32, (24, 32), seed=51)
    ref, _, xyz, _ = REF.run(s)
    valid = ref.w >= 1
    last = (valid[:, :, -1] & valid[:, :, -2] & ((ref.tsdf[:, :, -1] < 0) != (ref.tsdf[:, :, -2] < 0))).any() and \
           (valid[:, -1] & valid[:, -2] & ((ref.tsdf[:, -1] < 0) != (ref.tsdf[:, -2] < 0))).any() and \
           (valid[-1] & valid[-2] & ((ref.tsdf[-1] < 0) != (ref.tsdf[-2] < 0))).any()
    assert last and len(xyz) > 0                           # crossings do end on the last layer of every axis
    V = device_volume(T, ctx, s)
    integrate_device(ctx, V, s)
    assert_volume(V, ref)
    assert_points(V, ref)
    V.close()


def test_invalid_calls_write_nothing(R, T, L, ctx):
    s = REF.random_scene((65, 3, 2), 3, np.uint8, (24, 32), seed=61)
    ref = REF.run(s)[0]
    V = device_volume(T, ctx, s)
    integrate_device(ctx, V, s)
    cam = ctx.camera(24, 32, *s["K"])
    other = R.Context(0)
    foreign = other.camera(24, 32, *s["K"])
    buf = ctx.alloc(s["depths"].nbytes).upload(s["depths"])
    poses = np.ascontiguousarray(s["poses"])
    lib = ctx.lib
    for fn in (lib.r3d_tsdf_integrate, lib.r3d_tsdf_integrate_host):
        src = buf.ptr if fn is lib.r3d_tsdf_integrate else s["depths"].ctypes.data
        assert fn(V.handle, foreign.handle, src, L.DEPTH_U8, 3, s["scale"], poses.ctypes.data) == L.ERR_INVALID
        assert fn(V.handle, cam.handle, src, 7, 3, s["scale"], poses.ctypes.data) == L.ERR_INVALID
        assert fn(V.handle, cam.handle, src, L.DEPTH_U8, -1, s["scale"], poses.ctypes.data) == L.ERR_INVALID
        assert fn(V.handle, None, src, L.DEPTH_U8, 3, s["scale"], poses.ctypes.data) == L.ERR_INVALID
        assert fn(V.handle, cam.handle, None, L.DEPTH_U8, 3, s["scale"], poses.ctypes.data) == L.ERR_INVALID
        assert fn(V.handle, cam.handle, src, L.DEPTH_U8, 3, s["scale"], None) == L.ERR_INVALID
        assert fn(V.handle, cam.handle, None, L.DEPTH_U8, 0, s["scale"], None) == L.OK
    n = C.c_int64(-7)
    g = Guarded(ctx, 1200, seed=3)
    before = g.bytes().copy()
    assert lib.r3d_tsdf_extract_points(V.handle, 0.0, g.ptr, None, 100, C.byref(n)) == L.ERR_INVALID
    assert lib.r3d_tsdf_extract_points(V.handle, float("nan"), g.ptr, None, 100, C.byref(n)) == L.ERR_INVALID
    assert lib.r3d_tsdf_extract_points(V.handle, 1.0, g.ptr, None, -1, C.byref(n)) == L.ERR_INVALID
    assert lib.r3d_tsdf_extract_points(V.handle, 1.0, None, None, 100, C.byref(n)) == L.ERR_INVALID
    assert lib.r3d_tsdf_extract_points(V.handle, 1.0, g.ptr, None, 100, None) == L.ERR_INVALID
    assert n.value == -7 and np.array_equal(g.bytes(), before)
    h = C.c_void_p(7)
    origin = (C.c_double * 3)(0.0, 0.0, 0.0)
    for vs, dims, tr in ((0.0, (4, 4, 4), 0.3), (0.1, (0, 4, 4), 0.3), (0.1, (4, 4, 4), -1.0), (0.1, (2048, 2048, 512), 0.3),
                         (float("nan"), (4, 4, 4), 0.3)):
        assert lib.r3d_tsdf_create(ctx.handle, origin, vs, dims[0], dims[1], dims[2], tr, C.byref(h)) == L.ERR_INVALID and h.value is None
    assert_volume(V, ref)                                  # nothing of the above touched the volume
    buf.free()
    V.close()
    other.close()


@pytest.mark.parametrize("wide", [False, True])
def test_wall_on_the_device(T, ctx, wide):
    s = REF.wall_scene(wide)
    V = device_volume(T, ctx, s)
    integrate_device(ctx, V, s)
    xyz, nrm = V.extract_point_cloud()
    REF.check_wall(s, xyz, nrm)
    assert_volume(V, REF.run(s)[0])
    V.close()


def test_room_through_the_python_api(R, T, ctx):
    """the host-array API end to end: pose-file rows in, surface points out"""
    s = REF.room_scene()
    ref, _, want_xyz, want_nrm = REF.run(s)
    V = R.TSDFVolume(s["origin"], s["vs"], s["dims"], s["tr"], ctx=ctx)
    V.integrate(s["depths"], s["quats"], s["ts"], intrinsics=s["K"], depth_scale=s["scale"])
    assert_volume(V, ref)
    xyz, nrm = V.extract_point_cloud(min_weight=1.0)
    REF.check_room(s, xyz)
    assert np.array_equal(bits(xyz), bits(want_xyz)) and np.array_equal(bits(nrm), bits(want_nrm))
    # (test_tsdf_host.py asserts of the reference that two frames leave some of the points and that no voxel pair has four)
    few, _ = V.extract_point_cloud(min_weight=2)
    assert 0 < len(few) < len(xyz) and np.array_equal(bits(few), bits(REF.extract(ref, 2)[0]))
    assert V.extract_point_cloud(min_weight=4)[0].shape == (0, 3)
    V.reset()
    assert V.extract_point_cloud()[0].shape == (0, 3)
    with pytest.raises(ValueError):
        V.integrate(s["depths"], s["quats"][:3], s["ts"][:3])
    with pytest.raises(ValueError):
        V.extract_point_cloud(min_weight=0)
    V.close()


def test_command_line_on_scene3(R, T, ctx, golden_dir, tmp_path):
    """other_tools/integrate_tsdf.py from a drop-in working directory: its PLY holds the rows of the API call with its arguments"""
    import shutil
    work = tmp_path / "work"
    shutil.copytree(os.path.join(golden_dir, "scene3", "depth"), work / "depth")
    shutil.copytree(os.path.join(golden_dir, "scene3", "camera_pose"), work / "camera_pose")
    tool = os.path.join(ROOT, PKG, "other_tools", "integrate_tsdf.py")
    args = ["--voxel-size", "8", "--trunc", "24", "--origin", "-300", "-300", "-300", "--dims", "75", "75", "75", "--min-weight", "1"]
    # the fixture's 24 x 32 rasters under the reference's 640 x 480 intrinsics see a sliver; a wide-angle camera fills the volume
    K = (20.0, 20.0, 15.5, 11.5)
    env = dict(os.environ, PYTHONPATH=ROOT, R3D_FX="20", R3D_FY="20", R3D_CX="15.5", R3D_CY="11.5")
    r = subprocess.run([sys.executable, tool] + args, cwd=str(work), env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-1000:] + r.stderr[-2000:]
    xyz, nrm = R.cloud_io.read_ply_normals(str(work / "ply" / "tsdf_surface.ply"))
    names, quats, ts = R.read_pose_file(str(work / "camera_pose" / "image_colmap_simi_2.txt"))
    depths = R.cloud_io.read_depth_batch([str(work / "depth" / n) for n in names])
    V = R.TSDFVolume((-300, -300, -300), 8, (75, 75, 75), 24, ctx=ctx)
    V.integrate(depths, quats, ts, intrinsics=K)
    want_xyz, want_nrm = V.extract_point_cloud(1.0)
    V.close()
    assert len(want_xyz) > 1000 and np.array_equal(bits(xyz), bits(want_xyz)) and np.array_equal(bits(nrm), bits(want_nrm))
    # defaults: origin and dims from the camera centres' bounding box
    r = subprocess.run([sys.executable, tool, "--voxel-size", "8", "--trunc", "24"], cwd=str(work), env=env, capture_output=True, text=True,
                       timeout=300)
    assert r.returncode == 0, r.stdout[-1000:] + r.stderr[-2000:]
    assert "origin" in r.stdout and "dims" in r.stdout
