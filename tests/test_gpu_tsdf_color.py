"""GPU: the TSDF volume's colour against its NumPy reference (tests/tsdf_color_ref.py on top of tests/tsdf_ref.py), BIT FOR BIT:
tsdf, weight, the colour sums and counts, the surface points' colours, their count and order.  tests/test_tsdf_color_host.py
asserts the closed forms of the reference first.  Volume shapes sit around the pair / wave / workgroup limits of the integration
kernel, frame counts around the pose ring's chunk; rasters are tiny (24 x 32, 5 x 7)."""
import ctypes as C
import functools
import importlib
import os
import shutil
import subprocess
import sys

import numpy as np
import pytest

import tsdf_color_ref as CREF
import tsdf_ref as REF
from helpers import PKG, ROOT, r3d as _r3d
from test_gpu_bounds import Guarded

pytestmark = pytest.mark.gpu

DIMS = [(1, 1, 1), (2, 3, 1), (3, 5, 4), (33, 9, 5), (64, 4, 3), (130, 3, 2), (129, 2, 2)]
FRAMES = [1, 32, 33]                  # 32 = the pose ring's chunk (asserted against the package below)
DTYPES = [np.uint8, np.uint16, np.float32]


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


@functools.lru_cache(maxsize=None)
def scene(dims, n_frames, dtype, hw=(24, 32), seed=0):
    """(scene dict, colour images, reference volume, accepted pairs): computed once per case, never modified"""
    s = REF.random_scene(dims, n_frames, dtype, hw, seed=seed)
    rgb = CREF.random_colors(s, seed)
    ref, passed, _ = CREF.run(s, rgb)
    return s, rgb, ref, passed


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def color_volume(T, ctx, s):
    return T.TSDFVolume(s["origin"], s["vs"], s["dims"], s["tr"], ctx=ctx, color=True)


def integrate_rgb(ctx, V, s, rgb, lo=0, hi=None):
    """frames [lo, hi) of the scene through r3d_tsdf_integrate_rgb (rasters and images uploaded first)"""
    depths, images = s["depths"][lo:hi], np.ascontiguousarray(rgb[lo:hi])
    f, h, w = depths.shape
    cam = ctx.camera(h, w, *s["K"])
    d_depth, d_rgb = ctx.alloc(max(depths.nbytes, 16)).upload(depths), ctx.alloc(max(images.nbytes, 16)).upload(images)
    V.integrate_device(cam, d_depth.ptr, depths.dtype, f, s["poses"][lo:hi], s["scale"], d_rgb=d_rgb.ptr)
    ctx.sync()
    d_depth.free()
    d_rgb.free()


def raw_planes(ctx, V):
    """the bytes of the tsdf / weight plane and of the colour plane (None for a volume without)"""
    ctx.sync()
    p, n = V.device_view()
    a = np.empty(n * 8, np.uint8)
    ctx.lib.r3d_download(ctx.handle, a.ctypes.data, p, a.nbytes)
    if not V.color:
        return a, None
    q, m = V.colors_device_view()
    assert m == n
    b = np.empty(n * 16, np.uint8)
    ctx.lib.r3d_download(ctx.handle, b.ctypes.data, q, b.nbytes)
    return a, b


def assert_planes(V, ref):
    tsdf, w = V.volume()
    assert tsdf.shape == ref.tsdf.shape and np.array_equal(w, ref.w) and np.array_equal(bits(tsdf), bits(ref.tsdf))
    sums, n = V.colors()
    assert sums.dtype == np.uint32 and n.dtype == np.uint32 and sums.shape == ref.sums.shape
    assert np.array_equal(n, ref.n) and np.array_equal(sums, ref.sums)


def assert_colors(V, ref, min_weight=1.0):
    xyz, nrm, colors = V.extract_point_cloud(min_weight, with_colors=True)
    want_xyz, want_nrm = REF.extract(ref, min_weight)
    assert xyz.shape == want_xyz.shape and np.array_equal(bits(xyz), bits(want_xyz)) and np.array_equal(bits(nrm), bits(want_nrm))
    want = CREF.extract_colors(ref, min_weight)
    assert colors.dtype == np.uint8 and colors.shape == want.shape and np.array_equal(colors, want)
    assert V.extract_colors_device(min_weight, None, 0) == V.extract_points_device(min_weight, None, None, 0) == len(want)
    return len(want)


def test_chunk_is_what_the_cases_assume(T):
    assert T.CHUNK == 32 and T.CHUNK in FRAMES and T.CHUNK + 1 in FRAMES


@pytest.mark.parametrize("n_frames", FRAMES)
@pytest.mark.parametrize("dims", DIMS)
def test_integration_and_colours_match_the_reference(T, ctx, dims, n_frames):
    k = DIMS.index(dims) + FRAMES.index(n_frames)
    s, rgb, ref, passed = scene(dims, n_frames, DTYPES[k % 3], seed=k)
    if dims[0] >= 33 and n_frames >= 32:
        assert 0 < passed < n_frames * ref.w.size             # some (voxel, frame) pairs pass, some are rejected
        assert ref.n.max() > 1
    V = color_volume(T, ctx, s)
    integrate_rgb(ctx, V, s, rgb)
    assert_planes(V, ref)
    for mw in sorted({1, 2, n_frames}):
        assert_colors(V, ref, mw)
    V.close()


@pytest.mark.parametrize("dtype", DTYPES)
def test_every_depth_type(T, ctx, dtype):
    s, rgb, ref, passed = scene((33, 9, 5), 5, dtype, seed=11)
    assert passed > 0
    if np.dtype(dtype) == np.float32:
        d = s["depths"]
        assert np.isnan(d).any() and (d == np.inf).any() and (d == -np.inf).any() and (d < 0).any() and (d == 0).any()
    else:
        assert (s["depths"] == 0).any()
    V = color_volume(T, ctx, s)
    integrate_rgb(ctx, V, s, rgb)
    assert_planes(V, ref)
    assert assert_colors(V, ref) > 0
    V.close()


@pytest.mark.parametrize("dtype", [np.uint8, np.float32])
def test_raster_whose_colour_rows_are_not_word_aligned(T, ctx, dtype):
    """5 x 7: a colour row is 21 bytes, a frame 105"""
    s, rgb, ref, passed = scene((33, 9, 5), 6, dtype, hw=(5, 7), seed=13)
    assert passed > 0 and ref.n.max() > 1
    V = color_volume(T, ctx, s)
    integrate_rgb(ctx, V, s, rgb)
    assert_planes(V, ref)
    assert_colors(V, ref)
    V.close()


def test_volume_partly_behind_the_camera_and_outside_the_image(T, ctx):
    """the scene tests/test_gpu_tsdf.py::test_scene_covers_the_rejections counts the early-outs of"""
    s, rgb, ref, passed = scene((130, 9, 5), 17, np.float32, seed=5)
    F32 = np.float32
    gx, gy, gz = ref.centres()
    X, Y, Z = gx[None, None, :], gy[None, :, None], gz[:, None, None]
    behind = outside = 0
    for p in s["poses"].astype(F32):
        pz = ((p[6] * X + p[7] * Y) + p[8] * Z) + p[11]
        px = ((p[0] * X + p[1] * Y) + p[2] * Z) + p[9]
        behind += int((pz <= 0).sum())
        with np.errstate(all="ignore"):
            u = F32(s["K"][0]) * (px / pz) + F32(s["K"][2])
        outside += int(((pz > 0) & ((u + F32(0.5) < 0) | (u + F32(0.5) >= 32))).sum())
    assert behind > 0 and outside > 0 and passed > 0
    V = color_volume(T, ctx, s)
    integrate_rgb(ctx, V, s, rgb)
    assert_planes(V, ref)
    assert assert_colors(V, ref) > 0
    V.close()


@pytest.mark.parametrize("dims,n_frames", [((33, 9, 5), 33), ((64, 4, 3), 34)])
def test_call_forms_agree(T, L, ctx, dims, n_frames):
    s, rgb, ref, _ = scene(dims, n_frames, np.uint8, seed=31)
    plain = T.TSDFVolume(s["origin"], s["vs"], s["dims"], s["tr"], ctx=ctx)      # the depth-only kernels on the same input
    cam = ctx.camera(24, 32, *s["K"])
    d_depth = ctx.alloc(s["depths"].nbytes).upload(s["depths"])
    plain.integrate_device(cam, d_depth.ptr, np.uint8, n_frames, s["poses"], s["scale"])
    want_tsdf, _ = raw_planes(ctx, plain)
    d_depth.free()
    plain.close()
    whole = color_volume(T, ctx, s)
    integrate_rgb(ctx, whole, s, rgb)
    assert_planes(whole, ref)
    got_tsdf, want_col = raw_planes(ctx, whole)
    assert np.array_equal(got_tsdf, want_tsdf)               # tsdf / weight: the bits of the depth-only call
    again = color_volume(T, ctx, s)                          # a second run gives the same bits
    integrate_rgb(ctx, again, s, rgb)
    single = color_volume(T, ctx, s)                         # F calls of one frame
    for f in range(n_frames):
        integrate_rgb(ctx, single, s, rgb, f, f + 1)
    host = color_volume(T, ctx, s)                           # the *_host entry point: the same launches behind an upload
    L.check(ctx.lib.r3d_tsdf_integrate_rgb_host(host.handle, cam.handle, s["depths"].ctypes.data, L.DEPTH_U8, n_frames, s["scale"],
                                                np.ascontiguousarray(s["poses"]).ctypes.data, rgb.ctypes.data))
    for v in (again, single, host):
        a, b = raw_planes(ctx, v)
        assert np.array_equal(a, want_tsdf) and np.array_equal(b, want_col)
    for cut in (1, n_frames // 2, 32, n_frames - 1):         # two calls split anywhere
        two = color_volume(T, ctx, s)
        integrate_rgb(ctx, two, s, rgb, 0, cut)
        integrate_rgb(ctx, two, s, rgb, cut, n_frames)
        a, b = raw_planes(ctx, two)
        assert np.array_equal(a, want_tsdf) and np.array_equal(b, want_col)
        two.close()
    for v in (whole, again, single, host):
        v.close()


def test_two_volumes_and_ray_casts_take_turns_on_one_context(T, ctx):
    """The same 33 frames into a plain and a colour volume of one context in chunks of 17 and 16 -- plain, colour, plain, colour,
    nothing waited for in between -- and one ray cast of the colour volume behind each pair: every integrate call and every ray
    cast takes the next slot of its volume's pose ring (four slots: the colour volume uses them all), through the one driver both
    kinds of volume share."""
    import raycast_ref as RC
    from test_gpu_raycast import assert_maps, cast, poses_around, raster_K
    cut, shape = 17, (24, 32)
    s, rgb, ref, _ = scene((33, 9, 5), 33, np.uint8, seed=31)
    head = dict(s, depths=s["depths"][:cut], poses=s["poses"][:cut])
    ref_head = CREF.run(head, rgb[:cut])[0]                  # the colour volume's state at the first ray cast
    K, view = raster_K(shape), poses_around(ref, 1, 31)
    plain = T.TSDFVolume(s["origin"], s["vs"], s["dims"], s["tr"], ctx=ctx)
    V = color_volume(T, ctx, s)
    cam = ctx.camera(*shape, *s["K"])
    d_depth, d_rgb = ctx.alloc(s["depths"].nbytes).upload(s["depths"]), ctx.alloc(rgb.nbytes).upload(rgb)
    px = shape[0] * shape[1]
    for lo, hi, state in ((0, cut, ref_head), (cut, 33, ref)):
        plain.integrate_device(cam, d_depth.ptr + lo * px, np.uint8, hi - lo, s["poses"][lo:hi], s["scale"])
        V.integrate_device(cam, d_depth.ptr + lo * px, np.uint8, hi - lo, s["poses"][lo:hi], s["scale"], d_rgb=d_rgb.ptr + lo * px * 3)
        want = RC.raycast(state, view, K, shape)
        assert RC.hits(want[1]).any()
        assert_maps(cast(ctx, V, view, K, shape), want)
    assert_planes(V, ref)
    tsdf, w = plain.volume()
    assert np.array_equal(w, ref.w) and np.array_equal(bits(tsdf), bits(ref.tsdf))
    for b in (d_depth, d_rgb):
        b.free()
    for v in (plain, V):
        v.close()


def test_reset_clears_both_planes(T, ctx):
    s, rgb, ref, passed = scene((33, 9, 5), 5, np.uint16, seed=11)
    V = color_volume(T, ctx, s)
    a, b = raw_planes(ctx, V)
    assert not a.any() and not b.any()                       # fresh: zero bytes
    integrate_rgb(ctx, V, s, rgb)
    a, b = raw_planes(ctx, V)
    assert a.any() and b.any()
    V.reset()
    a, b = raw_planes(ctx, V)
    assert not a.any() and not b.any()
    assert [x.shape for x in V.extract_point_cloud(with_colors=True)] == [(0, 3)] * 3
    integrate_rgb(ctx, V, s, rgb)                            # and the volume is as good as new
    assert_planes(V, ref)
    V.close()


def test_unseen_volume_keeps_zero_sums(T, ctx):
    s = REF.random_scene((17, 4, 3), 5, np.uint16, (24, 32), seed=3, unseen=True)
    V = color_volume(T, ctx, s)
    integrate_rgb(ctx, V, s, CREF.random_colors(s))
    a, b = raw_planes(ctx, V)
    assert not a.any() and not b.any()
    assert [x.shape for x in V.extract_triangle_mesh(with_colors=True)] == [(0, 3)] * 4
    V.close()


def test_extraction_caps_and_guard_bands(T, ctx):
    s, rgb, ref, _ = scene((129, 9, 5), 6, np.float32, seed=41)
    want = CREF.pack(CREF.extract_colors(ref))
    n = len(want)
    assert n > 10 and len(set(want.tolist())) > 10
    V = color_volume(T, ctx, s)
    integrate_rgb(ctx, V, s, rgb)
    for cap in (0, n - 1, n, n + 1):
        g = Guarded(ctx, (n + 3) * 4, seed=cap)
        before = g.bytes().copy()
        assert V.extract_colors_device(1.0, g.ptr, cap) == n  # always the true count
        after = g.bytes()                                      # (asserts the guard bands)
        rows = min(cap, n)
        assert np.array_equal(after[:rows * 4].view(np.uint32), want[:rows])
        assert np.array_equal(after[rows * 4:], before[rows * 4:])
        g.free()
    V.close()


def test_mesh_with_colours(T, ctx):
    s, rgb, ref, _ = scene((33, 9, 5), 32, np.uint16, seed=DIMS.index((33, 9, 5)) + 1)
    V = color_volume(T, ctx, s)
    integrate_rgb(ctx, V, s, rgb)
    for mw in (1, 2):
        xyz, nrm, tri = V.extract_triangle_mesh(mw)
        cx, cn, ct, colors = V.extract_triangle_mesh(mw, with_colors=True)
        assert np.array_equal(bits(cx), bits(xyz)) and np.array_equal(bits(cn), bits(nrm)) and np.array_equal(ct, tri)
        assert np.array_equal(bits(xyz), bits(REF.extract(ref, mw)[0]))
        assert np.array_equal(colors, CREF.extract_colors(ref, mw))
    assert len(tri) > 0
    V.close()


def test_invalid_calls_write_nothing(R, T, L, ctx):
    s, rgb, ref, _ = scene((33, 9, 5), 5, np.uint8, seed=11)
    plain = T.TSDFVolume(s["origin"], s["vs"], s["dims"], s["tr"], ctx=ctx)
    cam = ctx.camera(24, 32, *s["K"])
    d_depth, d_rgb = ctx.alloc(s["depths"].nbytes).upload(s["depths"]), ctx.alloc(rgb.nbytes).upload(rgb)
    plain.integrate_device(cam, d_depth.ptr, np.uint8, 5, s["poses"], s["scale"])
    V = color_volume(T, ctx, s)
    integrate_rgb(ctx, V, s, rgb)
    plain_before, (tsdf_before, col_before) = raw_planes(ctx, plain)[0], raw_planes(ctx, V)
    poses = np.ascontiguousarray(s["poses"])
    lib = ctx.lib
    other = R.Context(0)
    foreign = other.camera(24, 32, *s["K"])
    g = Guarded(ctx, 1200, seed=3)
    guard_before = g.bytes().copy()
    n, p = C.c_int64(-7), C.c_void_p(5)
    colour_calls = ((lib.r3d_tsdf_integrate_rgb, d_depth.ptr, d_rgb.ptr), (lib.r3d_tsdf_integrate_rgb_host, s["depths"].ctypes.data, rgb.ctypes.data))
    # a colour call on a volume without the plane
    for fn, src, img in colour_calls:
        assert fn(plain.handle, cam.handle, src, L.DEPTH_U8, 5, s["scale"], poses.ctypes.data, img) == L.ERR_INVALID
        assert fn(plain.handle, cam.handle, src, L.DEPTH_U8, 0, s["scale"], poses.ctypes.data, img) == L.ERR_INVALID
    assert "colour" in L.last_error()
    assert lib.r3d_tsdf_colors(plain.handle, C.byref(p), C.byref(n)) == L.ERR_INVALID and n.value == -7 and p.value == 5
    assert lib.r3d_tsdf_extract_colors(plain.handle, 1.0, g.ptr, 100, C.byref(n)) == L.ERR_INVALID and n.value == -7
    # the depth-only entry points on a volume with the plane
    for fn, src in ((lib.r3d_tsdf_integrate, d_depth.ptr), (lib.r3d_tsdf_integrate_host, s["depths"].ctypes.data)):
        assert fn(V.handle, cam.handle, src, L.DEPTH_U8, 5, s["scale"], poses.ctypes.data) == L.ERR_INVALID
    assert "colour" in L.last_error()
    # the colour entry points' own argument errors
    for fn, src, img in colour_calls:
        assert fn(V.handle, cam.handle, src, L.DEPTH_U8, 5, s["scale"], poses.ctypes.data, None) == L.ERR_INVALID   # NULL rgb
        assert fn(V.handle, foreign.handle, src, L.DEPTH_U8, 5, s["scale"], poses.ctypes.data, img) == L.ERR_INVALID
        assert fn(V.handle, cam.handle, src, 7, 5, s["scale"], poses.ctypes.data, img) == L.ERR_INVALID
        assert fn(V.handle, cam.handle, src, L.DEPTH_U8, -1, s["scale"], poses.ctypes.data, img) == L.ERR_INVALID
        assert fn(V.handle, None, src, L.DEPTH_U8, 5, s["scale"], poses.ctypes.data, img) == L.ERR_INVALID
        assert fn(V.handle, cam.handle, None, L.DEPTH_U8, 5, s["scale"], poses.ctypes.data, img) == L.ERR_INVALID
        assert fn(V.handle, cam.handle, src, L.DEPTH_U8, 5, s["scale"], None, img) == L.ERR_INVALID
        assert fn(V.handle, cam.handle, src, L.DEPTH_U8, 5, float("inf"), poses.ctypes.data, img) == L.ERR_INVALID
        assert fn(V.handle, cam.handle, None, L.DEPTH_U8, 0, s["scale"], None, None) == L.OK
    for mw, out, cap, n_out in ((0.0, g.ptr, 100, C.byref(n)), (float("nan"), g.ptr, 100, C.byref(n)), (-1.0, g.ptr, 100, C.byref(n)),
                                (1.0, g.ptr, -1, C.byref(n)), (1.0, None, 100, C.byref(n)), (1.0, g.ptr, 100, None)):
        assert lib.r3d_tsdf_extract_colors(V.handle, mw, out, cap, n_out) == L.ERR_INVALID
    h = C.c_void_p(7)
    origin = (C.c_double * 3)(0.0, 0.0, 0.0)
    for vs, dims, tr in ((0.0, (4, 4, 4), 0.3), (0.1, (0, 4, 4), 0.3), (0.1, (4, 4, 4), -1.0), (0.1, (2048, 2048, 512), 0.3)):
        assert lib.r3d_tsdf_create_rgb(ctx.handle, origin, vs, dims[0], dims[1], dims[2], tr, C.byref(h)) == L.ERR_INVALID and h.value is None
    # nothing of the above wrote anything
    assert n.value == -7 and np.array_equal(g.bytes(), guard_before)
    assert np.array_equal(raw_planes(ctx, plain)[0], plain_before)
    a, b = raw_planes(ctx, V)
    assert np.array_equal(a, tsdf_before) and np.array_equal(b, col_before)
    assert_planes(V, ref)
    # the views' out-pointers are optional
    assert lib.r3d_tsdf_colors(V.handle, None, None) == L.OK
    for b_ in (d_depth, d_rgb):
        b_.free()
    g.free()
    for v in (plain, V):
        v.close()
    other.close()


def test_python_api_end_to_end(R, T, ctx):
    """host arrays in ([F,H,W] + [F,H,W,3], then one [H,W] + [H,W,3] frame), coloured points and mesh out"""
    quats, ts = np.tile([0.0, 0.0, 0.0, 1.0], (2, 1)), np.zeros((2, 3))
    w = REF.wall_scene()
    wall = CREF.repeated(w, 2)
    c = (200, 17, 255)
    V = R.TSDFVolume(w["origin"], w["vs"], w["dims"], w["tr"], ctx=ctx, color=True)
    V.integrate(wall["depths"][:1], quats[:1], ts[:1], intrinsics=w["K"], depth_scale=w["scale"], rgb=CREF.uniform_colors(w, [c]))
    V.integrate(wall["depths"][1], quats[1:], ts[1:], intrinsics=w["K"], depth_scale=w["scale"], rgb=CREF.uniform_colors(w, [c])[0])
    want, _, want_colors = CREF.run(wall, CREF.uniform_colors(wall, [c, c]))
    assert_planes(V, want)
    xyz, nrm, colors = V.extract_point_cloud(2.0, with_colors=True)
    REF.check_wall(w, xyz, nrm)
    assert np.array_equal(colors, want_colors) and (colors == np.array(c, np.uint8)).all()
    assert len(V.extract_point_cloud()) == 2 and len(V.extract_triangle_mesh()) == 3      # the default returns are unchanged
    with pytest.raises(ValueError):
        V.integrate(wall["depths"], quats, ts, intrinsics=w["K"])                          # colour volume, no rgb
    with pytest.raises(ValueError):
        V.integrate(wall["depths"], quats, ts, intrinsics=w["K"], rgb=np.zeros((2, 24, 32, 4), np.uint8))
    assert_planes(V, want)
    V.close()
    P = R.TSDFVolume(w["origin"], w["vs"], w["dims"], w["tr"], ctx=ctx)
    with pytest.raises(ValueError):
        P.integrate(wall["depths"], quats, ts, intrinsics=w["K"], rgb=CREF.uniform_colors(wall, [c, c]))
    with pytest.raises(ValueError):
        P.extract_point_cloud(with_colors=True)
    with pytest.raises(ValueError):
        P.colors()
    P.close()


def _ply_vertex_colours(path):
    """the uchar red green blue columns of a binary PLY whose vertex rows are float x y z nx ny nz + those three"""
    data = open(path, "rb").read()
    end = data.index(b"end_header\n")
    head = data[:end].decode().split("\n")
    assert head[9:12] == ["property uchar red", "property uchar green", "property uchar blue"], head
    n = int(head[2].split()[2])
    rows = np.frombuffer(data, dtype=np.dtype([("f", "<f4", (6,)), ("c", "u1", (3,))]), count=n, offset=end + 11)
    return np.ascontiguousarray(rows["c"])


def test_command_line_with_colour_directory(R, ctx, golden_dir, tmp_path):
    from PIL import Image
    work = tmp_path / "work"
    shutil.copytree(os.path.join(golden_dir, "scene3", "depth"), work / "depth")
    shutil.copytree(os.path.join(golden_dir, "scene3", "camera_pose"), work / "camera_pose")
    names, quats, ts = R.read_pose_file(str(work / "camera_pose" / "image_colmap_simi_2.txt"))
    depths = R.cloud_io.read_depth_batch([str(work / "depth" / n) for n in names])
    rng = np.random.default_rng(5)
    os.makedirs(work / "rgb")
    images = rng.integers(0, 256, depths.shape + (3,), dtype=np.uint8)
    for name, image in zip(names, images):
        Image.fromarray(image).save(str(work / "rgb" / name))
    tool = os.path.join(ROOT, PKG, "other_tools", "integrate_tsdf.py")
    args = ["--voxel-size", "8", "--trunc", "24", "--origin", "-300", "-300", "-300", "--dims", "75", "75", "75", "--min-weight", "1"]
    K = (20.0, 20.0, 15.5, 11.5)
    env = dict(os.environ, PYTHONPATH=ROOT, R3D_FX="20", R3D_FY="20", R3D_CX="15.5", R3D_CY="11.5")
    r = subprocess.run([sys.executable, tool] + args + ["--color-dir", "rgb", "--mesh", "--raycast"], cwd=str(work), env=env,
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-1000:] + r.stderr[-2000:]
    V = R.TSDFVolume((-300, -300, -300), 8, (75, 75, 75), 24, ctx=ctx, color=True)
    V.integrate(depths, quats, ts, intrinsics=K, rgb=images)
    want_xyz, want_nrm, want_tri, want_colors = V.extract_triangle_mesh(1.0, with_colors=True)
    V.close()
    assert len(want_xyz) > 1000 and len(np.unique(want_colors, axis=0)) > 100
    xyz, nrm = R.cloud_io.read_ply_normals(str(work / "ply" / "tsdf_surface.ply"))
    assert np.array_equal(bits(xyz), bits(want_xyz)) and np.array_equal(bits(nrm), bits(want_nrm))
    assert np.array_equal(_ply_vertex_colours(str(work / "ply" / "tsdf_surface.ply")), want_colors)
    mx, mn, mt, mc = R.cloud_io.read_ply_mesh(str(work / "ply" / "tsdf_mesh.ply"), with_colors=True)
    assert np.array_equal(bits(mx), bits(want_xyz)) and np.array_equal(bits(mn), bits(want_nrm)) and np.array_equal(mt, want_tri)
    assert np.array_equal(mc, want_colors)
    assert "raycast %d frames" % len(names) in r.stdout and os.path.exists(str(work / "raycast" / (names[0] + ".npy")))
    # an image of another size, then a missing one: a message, no traceback, before the device is touched
    Image.fromarray(images[0][:, :16]).save(str(work / "rgb" / names[0]))
    for what in ("the colour images", "not found"):
        r = subprocess.run([sys.executable, tool] + args + ["--color-dir", "rgb"], cwd=str(work), env=env, capture_output=True, text=True,
                           timeout=300)
        assert r.returncode != 0 and what in r.stderr and "Traceback" not in r.stderr, r.stderr[-2000:]
        if what == "the colour images":
            os.remove(str(work / "rgb" / names[0]))
