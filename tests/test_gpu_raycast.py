"""GPU: r3d_tsdf_raycast against tests/raycast_ref.py, BIT FOR BIT (uint32 views) on all three maps: depth, vertex, normal.  The
scenes are those of tests/test_raycast_host.py, which asserts their conditions of the reference first, plus tsdf_ref.random_scene
volumes integrated on the device and mesh_ref.random_volume arrays uploaded through device_view.  Volume shapes have one cell,
odd rows, more rows than a wave and flat volumes without a cell; rasters leave partial 8 x 8 and 16 x 16 tiles on both edges; view
counts straddle the pose ring's chunk.  Every cast writes into test_gpu_bounds.Guarded buffers at offsets 0, 4 and 8."""
import ctypes as C
import importlib
import os
import shutil
import subprocess
import sys

import numpy as np
import pytest

import mesh_ref as MREF
import raycast_ref as RC
import tsdf_ref as REF
from helpers import PKG, ROOT, r3d as _r3d
from test_gpu_bounds import Guarded

pytestmark = pytest.mark.gpu

INF = float("inf")


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


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def integrated(T, ctx, s):
    V = T.TSDFVolume(s["origin"], s["vs"], s["dims"], s["tr"], ctx=ctx)
    depths = s["depths"]
    f, h, w = depths.shape
    cam = ctx.camera(h, w, *s["K"])
    buf = ctx.alloc(max(depths.nbytes, 16)).upload(depths)
    V.integrate_device(cam, buf.ptr, depths.dtype, f, s["poses"] if "poses" in s else REF.poses_w2c(s["quats"], s["ts"]), s["scale"])
    ctx.sync()
    buf.free()
    return V


def uploaded(T, ctx, ref):
    """a device volume holding the reference volume's arrays (through device_view)"""
    V = T.TSDFVolume(ref.o.astype(np.float64), float(ref.vs), (ref.nx, ref.ny, ref.nz), float(ref.tr), ctx=ctx)
    p, n = V.device_view()
    raw = np.ascontiguousarray(np.stack([ref.tsdf.reshape(-1), ref.w.reshape(-1)], axis=1), dtype=np.float32)
    assert raw.shape == (n, 2)
    importlib.import_module(PKG + "._lib").check(ctx.lib.r3d_memcpy_h2d(ctx.handle, p, raw.ctypes.data, raw.nbytes))
    ctx.sync()
    return V


def raw_volume(ctx, V):
    p, n = V.device_view()
    out = np.empty(n * 8, np.uint8)
    ctx.lib.r3d_download(ctx.handle, out.ctypes.data, p, out.nbytes)
    return out


def cast(ctx, V, poses, K, shape, want=(True, True, True), seed=0, **kw):
    """raycast_device into guarded buffers at offsets 0, 4, 8, rotated by the seed (asserting the guard bands); the maps asked
    for, else None"""
    H, W = shape
    poses = np.ascontiguousarray(poses, dtype=np.float64).reshape(-1, 12)
    nv = len(poses)
    n = nv * H * W
    cam = ctx.camera(H, W, *K)
    offs = [(0, 4, 8)[(j + seed) % 3] for j in range(3)]        # the seed rotates the offsets: every output sees 0, 4 and 8
    g = [Guarded(ctx, n * size, off=off, seed=seed + off) if on else None for on, size, off in zip(want, (4, 12, 12), offs)]
    V.raycast_device(cam, nv, poses, *[b.ptr if b else None for b in g], **kw)
    out = []
    for b, tail in zip(g, ((), (3,), (3,))):
        out.append(b.bytes().view(np.float32).reshape((nv, H, W) + tail) if b else None)
        if b:
            b.free()
    return out


def assert_maps(got, want):
    for g, w, name in zip(got, want, ("depth", "vertex", "normal")):
        assert g.shape == w.shape, (name, g.shape, w.shape)
        bad = np.flatnonzero(bits(g).reshape(-1) != bits(w).reshape(-1))
        assert bad.size == 0, "%s: %d words differ, first at %d: %r != %r" % (name, bad.size, bad[0], g.reshape(-1)[bad[0]], w.reshape(-1)[bad[0]])


def raster_K(shape):
    """an integer principal point: an axis-aligned camera has rays with exactly zero direction components"""
    H, W = shape
    f = 1.2 * max(H, W, 4)
    return (f, f, float(W // 2), float(H // 2))


def poses_around(ref, n, seed):
    """n world -> camera rows in a cycle of four kinds: outside looking in, inside the volume, looking away, axis-parallel"""
    rng = np.random.default_rng([seed, n])
    dims = np.array([ref.nx, ref.ny, ref.nz], dtype=np.float64)
    lo, ext = ref.o.astype(np.float64), dims * float(ref.vs)
    c, r = lo + ext / 2, float(np.linalg.norm(ext)) / 2 + 2 * float(ref.vs)
    rows = []
    for v in range(n):
        d = rng.normal(size=3)
        d /= np.linalg.norm(d)
        if v % 4 == 0:
            rows.append(RC.look_at(c + d * r * rng.uniform(1.2, 2.0), c + rng.uniform(-0.2, 0.2, 3) * ext))
        elif v % 4 == 1:
            rows.append(RC.look_at(c + rng.uniform(-0.3, 0.3, 3) * ext, c + d * r))
        elif v % 4 == 2:
            eye = c + d * r * 1.5
            rows.append(RC.look_at(eye, eye + (eye - c)))
        else:
            row = np.zeros(12)
            row[0] = row[4] = row[8] = 1.0                        # identity rotation, looking down +z from in front of the volume
            eye = c + np.array([rng.integers(-1, 2) * 0.25 * ext[0], 0.0, -(ext[2] / 2 + r * rng.uniform(0.3, 1.0))])
            row[9:] = -eye
            rows.append(row)
    return np.stack(rows)


CHUNK = 32                               # R3D_TSDF_CHUNK (asserted against the package below)
# (kind, dims, seed, raster, n_views): kind "scene" = tsdf_ref.random_scene integrated on the device, "dense" / "holes" =
# mesh_ref.random_volume(invalid = 0.0 / 0.1) uploaded.  The seeds are ones for which the reference has hits and misses (asserted).
CASES = [
    ("dense", (2, 2, 2), 1, (24, 32), 3),
    ("holes", (3, 2, 2), 102, (24, 32), 3),
    ("scene", (17, 3, 2), 72, (24, 32), 3),
    ("scene", (16, 16, 17), 86, (24, 32), 3),
    ("dense", (16, 16, 17), 5, (17, 65), 3),
    ("holes", (16, 16, 17), 5, (24, 32), 1),
    ("scene", (130, 9, 5), 109, (17, 65), 1),
    ("holes", (130, 9, 5), 5, (5, 7), CHUNK + 1),
    ("dense", (17, 3, 2), 7, (1, 1), CHUNK + 1),
    ("dense", (130, 9, 5), 5, (24, 32), 3),
    ("dense", (1, 5, 5), 3, (5, 7), 3),
    ("holes", (7, 6, 1), 4, (24, 32), 1),
    ("scene", (1, 5, 5), 79, (17, 65), 1),
]


def case_volume(kind, dims, seed):
    """(reference volume, scene or None)"""
    if kind == "scene":
        s = REF.random_scene(dims, 9, np.float32, (24, 32), seed=seed)
        return REF.run(s)[0], s
    return MREF.random_volume(dims, seed, invalid=0.1 if kind == "holes" else 0.0), None


def case_step(ref):
    return float(ref.vs) * 0.5


def test_chunk_is_what_the_cases_assume(T):
    assert T.CHUNK == CHUNK


@pytest.mark.parametrize("case", CASES, ids=lambda c: "%s-%dx%dx%d-%dx%d-%d" % ((c[0],) + c[1] + c[3] + (c[4],)))
def test_matches_the_reference(T, ctx, case):
    kind, dims, seed, shape, nv = case
    ref, s = case_volume(kind, dims, seed)
    K, poses = raster_K(shape), poses_around(ref, nv, seed)
    want = RC.raycast(ref, poses, K, shape, step=case_step(ref))
    h = RC.hits(want[1])
    if min(dims) == 1:
        assert not h.any()                                        # no cell: all misses by construction
    else:
        assert h.any() and (~h).any(), (h.sum(), h.size)          # the reference has hits and misses
    V = integrated(T, ctx, s) if s is not None else uploaded(T, ctx, ref)
    before = raw_volume(ctx, V)
    got = cast(ctx, V, poses, K, shape, seed=CASES.index(case), step=case_step(ref))
    assert_maps(got, want)
    assert np.array_equal(raw_volume(ctx, V), before)             # the call does not modify the volume
    V.close()


def test_pose_kinds_each_do_their_part():
    """of the reference: the four kinds of poses_around give hits from outside and from inside, none looking away, and rays with
    exactly zero direction components"""
    ref = MREF.random_volume((16, 16, 17), 5)
    poses = poses_around(ref, 4, 5)
    K = raster_K((24, 32))
    per = [RC.cast_view(ref, p, K, (24, 32), step=0.5)[3] for p in poses]
    assert per[0].any() and per[1].any() and not per[2].any() and per[3].any()
    c = np.array([8.0, 8.0, 8.5])
    _, C1 = RC.prepare_pose(poses[1])
    assert (np.abs(C1 - c) < np.array([8.0, 8.0, 8.5])).all()    # that camera is inside the volume
    assert per[3][12, 16] or per[3][:, 16].any()                  # the column ui = cx: dw_x == 0


@pytest.fixture(scope="module")
def dense(T, ctx):
    """one uploaded volume shared by the tests that do not vary the shape: (V, ref, poses, K, shape, step, want)"""
    ref = MREF.random_volume((16, 16, 17), 5, invalid=0.1)
    shape = (17, 33)
    K, poses = raster_K(shape), poses_around(ref, 3, 11)
    want = RC.raycast(ref, poses, K, shape, step=0.5)
    h = RC.hits(want[1])
    assert h.any() and (~h).any()
    V = uploaded(T, ctx, ref)
    yield V, ref, poses, K, shape, 0.5, want
    V.close()


def test_any_subset_of_outputs(dense, ctx):
    V, ref, poses, K, shape, step, want = dense
    for mask in range(8):
        on = tuple(bool(mask >> j & 1) for j in range(3))
        got = cast(ctx, V, poses, K, shape, want=on, seed=mask, step=step)
        for j in range(3):
            if on[j]:
                assert np.array_equal(bits(got[j]), bits(want[j])), (mask, j)
            else:
                assert got[j] is None


def test_repeatability_and_order_of_calls(dense, ctx):
    V, ref, poses, K, shape, step, want = dense
    before = raw_volume(ctx, V)
    assert_maps(cast(ctx, V, poses, K, shape, step=step), want)
    assert_maps(cast(ctx, V, poses, K, shape, seed=5, step=step), want)      # a second run gives the same bytes
    V.extract_triangle_mesh()
    assert_maps(cast(ctx, V, poses, K, shape, seed=6, step=step), want)      # and one after extract_triangle_mesh
    one = [cast(ctx, V, poses[v:v + 1], K, shape, seed=7 + v, step=step) for v in range(len(poses))]   # one call per view
    assert_maps([np.concatenate([o[j] for o in one]) for j in range(3)], want)
    assert np.array_equal(raw_volume(ctx, V), before)


def test_march_parameters(dense, ctx):
    """min_weight, step, t_near and t_far reach the kernel as the reference takes them"""
    V, ref, poses, K, shape, step, want = dense
    for kw in (dict(step=0.25), dict(step=1.0, t_near=3.0), dict(step=0.5, t_far=22.0), dict(step=0.5, t_near=2.6, t_far=1e30),
               dict(step=0.5, min_weight=0.5), dict(step=0.5, min_weight=2.0)):
        other = RC.raycast(ref, poses, K, shape, **kw)
        assert_maps(cast(ctx, V, poses, K, shape, **kw), other)
        if kw.get("min_weight") == 2.0:
            assert not RC.hits(other[1]).any()
        elif kw != dict(step=0.5, min_weight=0.5):
            assert not np.array_equal(bits(other[0]), bits(want[0]))          # the parameter does change the result


def test_invalid_calls_write_nothing(R, dense, L, ctx):
    V, ref, poses, K, shape, step, want = dense
    lib = ctx.lib
    H, W = shape
    nv = len(poses)
    n = nv * H * W
    cam = ctx.camera(H, W, *K)
    other = R.Context(0)
    foreign = other.camera(H, W, *K)
    gd, gv, gn = Guarded(ctx, n * 4, seed=1), Guarded(ctx, n * 12, off=4, seed=2), Guarded(ctx, n * 12, off=8, seed=3)
    before = [g.bytes().copy() for g in (gd, gv, gn)]
    vol_before = raw_volume(ctx, V)
    p = np.ascontiguousarray(poses).ctypes.data
    vol_ptr, n_vox = V.device_view()
    nan = float("nan")
    good = (V.handle, cam.handle, nv, p, 1.0, step, 0.0, INF, gd.ptr, gv.ptr, gn.ptr)

    def call(**kw):
        names = ("vol", "cam", "n_views", "poses", "mw", "step", "t_near", "t_far", "depth", "vertex", "normal")
        args = list(good)
        for k, v in kw.items():
            args[names.index(k)] = v
        return lib.r3d_tsdf_raycast(*args)

    bad = [dict(vol=None), dict(cam=None), dict(cam=foreign.handle), dict(n_views=-1), dict(poses=None),
           dict(mw=0.0), dict(mw=-1.0), dict(mw=nan), dict(mw=INF), dict(mw=1e-60),
           dict(step=0.0), dict(step=-0.5), dict(step=nan), dict(step=INF), dict(step=1e-60),
           dict(t_near=-0.1), dict(t_near=nan), dict(t_near=INF), dict(t_far=0.0), dict(t_near=2.0, t_far=2.0), dict(t_near=2.0, t_far=1.0),
           dict(t_far=nan),
           dict(vertex=gd.ptr), dict(normal=gv.ptr + 12), dict(depth=gv.ptr + 4 * 3), dict(depth=vol_ptr), dict(normal=vol_ptr + n_vox * 8 - 4),
           dict(step=float(np.sqrt(15.0 ** 2 * 2 + 16.0 ** 2)) / 65537.0)]     # the march could take more than 65536 samples
    for kw in bad:
        assert call(**kw) == L.ERR_INVALID, kw
    big = ctx.camera((1 << 24) + 1, 1, *K)
    assert call(cam=big.handle) == L.ERR_INVALID
    assert call(n_views=0, poses=None) == L.OK
    assert call(depth=None, vertex=None, normal=None) == L.OK     # a valid no-op
    assert call(step=float(np.sqrt(15.0 ** 2 * 2 + 16.0 ** 2)) / 65000.0, depth=None, vertex=None, normal=None) == L.OK
    after = [g.bytes() for g in (gd, gv, gn)]
    for a, b in zip(after, before):
        assert np.array_equal(a, b)
    assert np.array_equal(raw_volume(ctx, V), vol_before)
    assert call() == L.OK                                         # and the good call is good
    got = [g.bytes().view(np.float32) for g in (gd, gv, gn)]
    assert_maps([got[0].reshape(nv, H, W), got[1].reshape(nv, H, W, 3), got[2].reshape(nv, H, W, 3)], want)
    for g in (gd, gv, gn):
        g.free()
    other.close()


def test_wall_on_the_device(T, ctx):
    s = REF.wall_scene()
    ref = REF.run(s)[0]
    V = integrated(T, ctx, s)
    got = cast(ctx, V, s["poses"], s["K"], (24, 32), step=RC.WALL_STEP)
    zero_K = (40.0, 40.0, 16.0, 12.0)                            # the column ui = cx and the row vi = cy: zero direction components
    axis = cast(ctx, V, s["poses"], zero_K, (24, 32), step=RC.WALL_STEP)
    V.close()
    RC.check_wall(s, got[0][0], got[1][0], got[2][0])
    assert RC.hits(axis[1])[0, 12, 16] and axis[1][0, 12, 16, 0] == 0.0
    assert_maps(axis, RC.raycast(ref, s["poses"], zero_K, (24, 32), step=RC.WALL_STEP))
    assert_maps(got, RC.raycast(ref, s["poses"], s["K"], (24, 32), step=RC.WALL_STEP))


def test_sphere_on_the_device(T, ctx):
    ref = MREF.sphere_volume()
    V = uploaded(T, ctx, ref)
    got = cast(ctx, V, RC.sphere_poses(), RC.SPHERE_K, (24, 32), step=0.5)
    inside = cast(ctx, V, RC.look_at((1.5, 2.0, 1.5), (10.0, 10.0, 10.0)), RC.SPHERE_K, (24, 32), step=0.5)
    cut = cast(ctx, V, RC.sphere_poses()[:1], RC.SPHERE_K, (24, 32), step=0.5, t_far=17.0)
    beyond = cast(ctx, V, RC.sphere_poses()[:1], RC.SPHERE_K, (24, 32), step=0.5, t_near=24.0)
    V.close()
    RC.check_sphere(got[1], got[2])
    assert_maps(got, RC.raycast(ref, RC.sphere_poses(), RC.SPHERE_K, (24, 32), step=0.5))
    assert_maps(inside, RC.raycast(ref, RC.look_at((1.5, 2.0, 1.5), (10.0, 10.0, 10.0)), RC.SPHERE_K, (24, 32), step=0.5))
    assert_maps(cut, RC.raycast(ref, RC.sphere_poses()[:1], RC.SPHERE_K, (24, 32), step=0.5, t_far=17.0))
    assert 0 < RC.hits(cut[1]).sum() < RC.hits(got[1][0]).sum()
    assert not RC.hits(beyond[1]).any() and not beyond[0].any()


def test_room_round_trip_through_the_python_api(R, ctx):
    s = REF.room_scene()
    ref = REF.run(s)[0]
    V = R.TSDFVolume(s["origin"], s["vs"], s["dims"], s["tr"], ctx=ctx)
    V.integrate(s["depths"], s["quats"], s["ts"], intrinsics=s["K"], depth_scale=s["scale"])
    got = V.raycast(s["quats"], s["ts"], (96, 128), intrinsics=s["K"])
    assert [a.shape for a in got] == [(8, 96, 128), (8, 96, 128, 3), (8, 96, 128, 3)] and all(a.dtype == np.float32 for a in got)
    RC.check_round_trip(s, got[0], got[1])
    assert_maps(got, RC.raycast(ref, REF.poses_w2c(s["quats"], s["ts"]), s["K"], (96, 128)))
    # a ray-cast raster integrates back: the misses are "no measurement"
    V2 = R.TSDFVolume(s["origin"], s["vs"], s["dims"], s["tr"], ctx=ctx)
    V2.integrate(got[0], s["quats"], s["ts"], intrinsics=s["K"])
    assert len(V2.extract_point_cloud()[0]) > 1000
    V2.close()
    empty = V.raycast(s["quats"][:0], s["ts"][:0], (4, 5))
    assert [a.shape for a in empty] == [(0, 4, 5), (0, 4, 5, 3), (0, 4, 5, 3)]
    for kw in (dict(step=0), dict(step=-1.0), dict(min_weight=0), dict(t_near=-1.0), dict(t_near=3.0, t_far=3.0), dict(t_far=float("nan")),
               dict(step=float("inf"))):
        with pytest.raises(ValueError):
            V.raycast(s["quats"], s["ts"], (96, 128), **kw)
    for shape in ((0, 5), (4,), (4.5, 5), "ab"):
        with pytest.raises(ValueError):
            V.raycast(s["quats"], s["ts"], shape)
    with pytest.raises(ValueError):
        V.raycast(s["quats"], s["ts"][:3], (4, 5))
    with pytest.raises(ValueError):
        V.raycast_device(ctx.camera(4, 5, *s["K"]), 2, np.zeros((3, 12)), None, None, None)
    with pytest.raises(ValueError):
        V.raycast_device(ctx.camera(4, 5, *s["K"]), -1, np.zeros((0, 12)), None, None, None)
    V.close()


def test_command_line_with_raycast_flag(R, ctx, golden_dir, tmp_path):
    work = tmp_path / "work"
    shutil.copytree(os.path.join(golden_dir, "scene3", "depth"), work / "depth")
    shutil.copytree(os.path.join(golden_dir, "scene3", "camera_pose"), work / "camera_pose")
    tool = os.path.join(ROOT, PKG, "other_tools", "integrate_tsdf.py")
    args = ["--voxel-size", "8", "--trunc", "24", "--origin", "-300", "-300", "-300", "--dims", "75", "75", "75", "--min-weight", "1"]
    K = (20.0, 20.0, 15.5, 11.5)
    env = dict(os.environ, PYTHONPATH=ROOT, R3D_FX="20", R3D_FY="20", R3D_CX="15.5", R3D_CY="11.5")
    r = subprocess.run([sys.executable, tool] + args + ["--raycast"], cwd=str(work), env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-1000:] + r.stderr[-2000:]
    names, quats, ts = R.read_pose_file(str(work / "camera_pose" / "image_colmap_simi_2.txt"))
    depths = R.cloud_io.read_depth_batch([str(work / "depth" / n) for n in names])
    lines = [l for l in r.stdout.split("\n") if l.startswith(("origin", "raycast"))]
    assert len(lines) == 2 and lines[1] == "raycast %d frames -> ./raycast/" % len(names)
    V = R.TSDFVolume((-300, -300, -300), 8, (75, 75, 75), 24, ctx=ctx)
    V.integrate(depths, quats, ts, intrinsics=K)
    want = V.raycast(quats, ts, depths.shape[1:], intrinsics=K)[0]
    V.close()
    assert (want > 0).sum() > 100
    for k, name in enumerate(names):
        got = np.load(str(work / "raycast" / (name + ".npy")))
        assert got.dtype == np.float32 and np.array_equal(bits(got), bits(want[k]))
    # without the flag, from a fresh copy of the inputs: no directory, and the one line the tool prints today
    plain = tmp_path / "plain"
    shutil.copytree(os.path.join(golden_dir, "scene3", "depth"), plain / "depth")
    shutil.copytree(os.path.join(golden_dir, "scene3", "camera_pose"), plain / "camera_pose")
    r2 = subprocess.run([sys.executable, tool] + args, cwd=str(plain), env=env, capture_output=True, text=True, timeout=300)
    assert r2.returncode == 0, r2.stdout[-1000:] + r2.stderr[-2000:]
    assert not (plain / "raycast").exists()
    assert r2.stdout == r.stdout.replace(lines[1] + "\n", "") and "raycast" not in r2.stdout      # exactly today's lines
    assert sorted(os.listdir(str(plain / "ply"))) == ["tsdf_surface.ply"]


def _pose_error(Ta, Tb):
    """(rotation angle in degrees, distance of the camera centres) between two world -> camera matrices"""
    Rd = Ta[:3, :3] @ Tb[:3, :3].T
    ang = np.degrees(np.arccos(np.clip((np.trace(Rd) - 1.0) / 2.0, -1.0, 1.0)))
    ca, cb = -Ta[:3, :3].T @ Ta[:3, 3], -Tb[:3, :3].T @ Tb[:3, 3]
    return float(ang), float(np.linalg.norm(ca - cb))


def test_frame_to_model_registration(R, ctx):
    """A new frame, taken 2 degrees of yaw and 0.05 m from pose i, is registered against the model's ray-cast vertex and normal
    map at pose i: rotation and translation error after registration are each strictly smaller than before."""
    syn = importlib.import_module(PKG + ".synthetic")
    icp = importlib.import_module(PKG + ".icp")
    # pose 2 looks along yaw 0.885 rad, into the room's corner at atan2(4, 3) = 0.927 rad: two walls, floor and ceiling are in
    # sight, so the planes' normals span all three directions and no sliding along a single wall is left unconstrained
    H, W, n_frames, i = 96, 128, 16, 2
    depths, quats, ts, K = syn.room_views(n_frames, H, W, seed=0)
    vs, margin = 0.05, 0.3
    lo, hi = syn.ROOM_LO - margin, syn.ROOM_HI + margin
    dims = tuple(int(np.ceil((hi[a] - lo[a]) / vs - 1e-9)) for a in range(3))
    V = R.TSDFVolume(tuple(lo), vs, dims, 0.2, ctx=ctx)
    V.integrate(depths, quats, ts, intrinsics=K)
    depth, vertex, normal = V.raycast(quats[i:i + 1], ts[i:i + 1], (H, W), intrinsics=K)
    V.close()
    h = RC.hits(vertex[0])
    assert h.mean() >= 0.5 and np.array_equal(h, depth[0] > 0)
    assert np.abs(depth[0][h] - depths[i][h]).max() <= np.sqrt(3.0) * vs
    assert np.abs(np.linalg.norm(normal[0][h].astype(np.float64), axis=1) - 1.0).max() <= 1e-6
    # the new frame: pose i turned by 2 degrees of yaw and moved by 0.05 m
    T_i = syn.pose_matrix(quats[i], ts[i])
    c_i = -T_i[:3, :3].T @ T_i[:3, 3]
    yaw_i = 2 * np.pi * i / n_frames + 0.1
    z, q_new, t_new, _ = syn.room_view(H, W, yaw_i + np.radians(2.0), c_i + np.array([0.03, 0.0, 0.04]))
    T_true = syn.pose_matrix(q_new, t_new)
    fx, fy, cx, cy = K
    u, v = np.meshgrid(np.arange(W), np.arange(H))
    cam_pts = np.stack([(u - cx) / fx * z, (v - cy) / fy * z, z], axis=-1).reshape(-1, 3)
    src = (cam_pts - T_i[:3, 3]) @ T_i[:3, :3]                 # back-projected with the unperturbed guess: R_i^T (p - t_i)
    before = _pose_error(T_i, T_true)
    assert abs(before[0] - 2.0) < 1e-6 and abs(before[1] - 0.05) < 1e-9
    T_found, info = icp.icp_point_to_plane(src.astype(np.float32), vertex[0][h], tgt_normals=normal[0][h], ctx=ctx)
    T_est = T_i @ np.linalg.inv(T_found)                       # T_found moves the guessed world points onto the model
    after = _pose_error(T_est, T_true)
    print("frame-to-model: rotation %.4f -> %.4f degrees, translation %.4f -> %.4f m, %d iterations" %
          (before[0], after[0], before[1], after[1], info["iterations"]))
    assert after[0] < before[0] and after[1] < before[1], (before, after)
