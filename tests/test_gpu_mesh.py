"""GPU: r3d_tsdf_extract_mesh against tests/mesh_ref.py, BIT FOR BIT: vertices (count, order, positions, normals -- the rows of
r3d_tsdf_extract_points) and triangles (count, order, indices).  The scenes are tsdf_ref.random_scene's (crossings everywhere,
alternating signs, holes) and the shapes of tests/test_mesh_host.py, which asserts their conditions of the reference first.
Volume shapes put the 16-voxel groups and the 4096-voxel tiles on both sides of rows, slabs and the volume's end."""
import ctypes as C
import importlib
import os
import shutil
import subprocess
import sys

import numpy as np
import pytest

import mesh_ref as MREF
import tsdf_ref as REF
from helpers import PKG, ROOT, r3d as _r3d
from test_gpu_bounds import Guarded

pytestmark = pytest.mark.gpu

DIMS = [(2, 2, 2), (3, 2, 2), (17, 3, 2), (65, 3, 2), (16, 16, 16), (16, 16, 17), (130, 9, 5), (64, 4, 4), (40, 1, 3), (1, 5, 5), (7, 6, 1)]
SEEDS = [81, 71, 72, 73, 85, 86, 109, 110, 78, 79, 91]     # scenes in which every shape with cells has triangles at min_weight 1 (asserted below)
DTYPES = [np.uint8, np.uint16, np.float32]
N_FRAMES = 9


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
    V.integrate_device(cam, buf.ptr, depths.dtype, f, s["poses"], s["scale"])
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


def assert_mesh(got, want):
    for g, w in zip(got, want):
        assert g.shape == w.shape, (g.shape, w.shape)
    assert np.array_equal(bits(got[0]), bits(want[0])) and np.array_equal(bits(got[1]), bits(want[1]))
    assert got[2].dtype == np.int32 and np.array_equal(got[2], want[2])


@pytest.fixture(scope="module")
def scene129(T, ctx):
    """one integrated scene with a few thousand vertices, shared by the tests that do not vary the shape"""
    s = REF.random_scene((129, 9, 5), 12, np.float32, (24, 32), seed=41)
    ref = REF.run(s)[0]
    want = MREF.extract_mesh(ref)
    assert len(want[0]) > 10 and len(want[2]) > 10
    V = integrated(T, ctx, s)
    yield V, ref, want
    V.close()


@pytest.mark.parametrize("dims", DIMS)
def test_mesh_matches_the_reference(T, ctx, dims):
    k = DIMS.index(dims)
    s = REF.random_scene(dims, N_FRAMES, DTYPES[k % 3], (24, 32), seed=SEEDS[k])
    ref = REF.run(s)[0]
    V = integrated(T, ctx, s)
    before = raw_volume(ctx, V)
    any_triangle = False
    for mw in (1, 2, N_FRAMES):
        want = MREF.extract_mesh(ref, mw)
        got = V.extract_triangle_mesh(mw)
        assert_mesh(got, want)
        pts = V.extract_point_cloud(mw)                      # the vertices are the points' bytes
        assert np.array_equal(bits(got[0]), bits(pts[0])) and np.array_equal(bits(got[1]), bits(pts[1]))
        any_triangle |= len(want[2]) > 0
        if min(dims) == 1:
            assert got[2].shape == (0, 3)
    assert any_triangle == (min(dims) > 1)
    assert np.array_equal(raw_volume(ctx, V), before)        # the call does not modify the volume
    V.close()


def test_inactive_cells_appear_with_min_weight(scene129):
    V, ref, want = scene129
    counts = [len(MREF.extract_mesh(ref, mw)[2]) for mw in (1, 2, 12)]
    assert counts[0] > counts[1] > counts[2] >= 0
    for mw in (2, 12):
        assert_mesh(V.extract_triangle_mesh(mw), MREF.extract_mesh(ref, mw))


def test_caps_and_guard_bands(scene129, ctx):
    V, ref, (want_xyz, want_nrm, want_tri) = scene129
    n, m = len(want_xyz), len(want_tri)
    assert V.extract_mesh_device(1.0, None, None, 0, None, 0) == (n, m)
    for cv in (0, n - 1, n, n + 1):
        for ct in (0, m - 1, m, m + 1):
            gx, gn = Guarded(ctx, (n + 3) * 12, seed=cv), Guarded(ctx, (n + 3) * 12, off=4, seed=cv + 1)
            gt = Guarded(ctx, (m + 3) * 12, off=8, seed=ct + 2)
            before = [g.bytes().copy() for g in (gx, gn, gt)]
            assert V.extract_mesh_device(1.0, gx.ptr, gn.ptr, cv, gt.ptr, ct) == (n, m)      # always the true counts
            after = [g.bytes() for g in (gx, gn, gt)]         # (asserts the guard bands)
            vr, tr = min(cv, n), min(ct, m)
            assert np.array_equal(after[0][:vr * 12].view(np.uint32).reshape(-1, 3), bits(want_xyz[:vr]))
            assert np.array_equal(after[1][:vr * 12].view(np.uint32).reshape(-1, 3), bits(want_nrm[:vr]))
            assert np.array_equal(after[2][:tr * 12].view(np.int32).reshape(-1, 3), want_tri[:tr])   # rows as they are
            for a, b, rows in zip(after, before, (vr, vr, tr)):
                assert np.array_equal(a[rows * 12:], b[rows * 12:])
            for g in (gx, gn, gt):
                g.free()
    # positions and triangles alone
    gx, gt = Guarded(ctx, n * 12, seed=9), Guarded(ctx, m * 12, seed=10)
    assert V.extract_mesh_device(1.0, gx.ptr, None, n, gt.ptr, m) == (n, m)
    assert np.array_equal(gx.bytes().view(np.uint32).reshape(-1, 3), bits(want_xyz))
    assert np.array_equal(gt.bytes().view(np.int32).reshape(-1, 3), want_tri)
    # triangles alone
    gt2 = Guarded(ctx, m * 12, seed=11)
    assert V.extract_mesh_device(1.0, None, None, 0, gt2.ptr, m) == (n, m)
    assert np.array_equal(gt2.bytes().view(np.int32).reshape(-1, 3), want_tri)
    for g in (gx, gt, gt2):
        g.free()


def test_repeatability_and_order_of_calls(scene129):
    V, ref, want = scene129
    first = V.extract_triangle_mesh()
    assert_mesh(first, want)
    assert_mesh(V.extract_triangle_mesh(), first)            # a second run gives the same bytes
    pts = V.extract_point_cloud()
    assert_mesh(V.extract_triangle_mesh(), first)            # after extract_points
    again = V.extract_point_cloud()                          # and the points after the mesh
    assert np.array_equal(bits(pts[0]), bits(again[0])) and np.array_equal(bits(pts[1]), bits(again[1]))
    assert np.array_equal(bits(pts[0]), bits(first[0]))


def test_invalid_calls_write_nothing(scene129, L, ctx):
    V, ref, want = scene129
    lib = ctx.lib
    gx, gt = Guarded(ctx, 1200, seed=3), Guarded(ctx, 1200, seed=4)
    bx, bt = gx.bytes().copy(), gt.bytes().copy()
    vol_before = raw_volume(ctx, V)
    nv, nt = C.c_int64(-7), C.c_int64(-9)
    calls = [(None, 1.0, gx.ptr, None, 100, gt.ptr, 100, C.byref(nv), C.byref(nt)),
             (V.handle, 0.0, gx.ptr, None, 100, gt.ptr, 100, C.byref(nv), C.byref(nt)),
             (V.handle, float("nan"), gx.ptr, None, 100, gt.ptr, 100, C.byref(nv), C.byref(nt)),
             (V.handle, -1.0, gx.ptr, None, 100, gt.ptr, 100, C.byref(nv), C.byref(nt)),
             (V.handle, 1.0, gx.ptr, None, -1, gt.ptr, 100, C.byref(nv), C.byref(nt)),
             (V.handle, 1.0, gx.ptr, None, 100, gt.ptr, -1, C.byref(nv), C.byref(nt)),
             (V.handle, 1.0, None, None, 100, gt.ptr, 100, C.byref(nv), C.byref(nt)),
             (V.handle, 1.0, gx.ptr, None, 100, None, 100, C.byref(nv), C.byref(nt)),
             (V.handle, 1.0, gx.ptr, None, 100, gt.ptr, 100, None, C.byref(nt)),
             (V.handle, 1.0, gx.ptr, None, 100, gt.ptr, 100, C.byref(nv), None)]
    for args in calls:
        assert lib.r3d_tsdf_extract_mesh(*args) == L.ERR_INVALID, args
    assert (nv.value, nt.value) == (-7, -9)
    assert np.array_equal(gx.bytes(), bx) and np.array_equal(gt.bytes(), bt)
    assert np.array_equal(raw_volume(ctx, V), vol_before)
    with pytest.raises(ValueError):
        V.extract_triangle_mesh(min_weight=0)
    gx.free()
    gt.free()


def test_sphere_uploaded_into_the_volume_is_closed(T, ctx):
    ref = MREF.sphere_volume()
    want = MREF.extract_mesh(ref)
    V = uploaded(T, ctx, ref)
    got = V.extract_triangle_mesh()
    V.close()
    MREF.check_sphere(got[0], got[2])                        # closed, Euler characteristic 2, outward
    assert_mesh(got, want)


@pytest.mark.parametrize("invalid", [0.0, 0.1])
@pytest.mark.parametrize("dims", [(9, 8, 7), (16, 16, 17), (130, 9, 5)])
def test_random_volume_uploaded(T, ctx, dims, invalid):
    """ambiguous faces everywhere (and holes), dense across rows, slabs and tiles: against the reference"""
    ref = MREF.random_volume(dims, 5, invalid=invalid)
    want = MREF.extract_mesh(ref)
    assert len(want[2]) > 50
    V = uploaded(T, ctx, ref)
    assert_mesh(V.extract_triangle_mesh(), want)
    V.close()


def test_wall_on_the_device(T, ctx):
    s = REF.wall_scene(False)
    V = integrated(T, ctx, s)
    xyz, nrm, tri = V.extract_triangle_mesh()
    V.close()
    REF.check_wall(s, xyz, nrm)
    assert MREF.check_wall_mesh(s, xyz, tri) == 2 * (s["dims"][0] - 1) * (s["dims"][1] - 1)


def test_room_through_the_python_api_and_ply(R, ctx, tmp_path):
    s = REF.room_scene()
    ref = REF.run(s)[0]
    want = MREF.extract_mesh(ref)
    V = R.TSDFVolume(s["origin"], s["vs"], s["dims"], s["tr"], ctx=ctx)
    V.integrate(s["depths"], s["quats"], s["ts"], intrinsics=s["K"], depth_scale=s["scale"])
    got = V.extract_triangle_mesh(min_weight=1.0)
    assert_mesh(got, want)
    REF.check_room(s, got[0][got[2].reshape(-1)])
    assert_mesh(V.extract_triangle_mesh(min_weight=2), MREF.extract_mesh(ref, 2))
    assert [a.shape for a in V.extract_triangle_mesh(min_weight=4)] == [(0, 3)] * 3
    V.reset()
    assert [a.shape for a in V.extract_triangle_mesh()] == [(0, 3)] * 3
    V.close()
    path = str(tmp_path / "room.ply")
    R.cloud_io.write_ply_mesh(path, *got)
    assert_mesh(R.cloud_io.read_ply_mesh(path), want)


def test_command_line_with_mesh_flag(R, golden_dir, tmp_path):
    work = tmp_path / "work"
    shutil.copytree(os.path.join(golden_dir, "scene3", "depth"), work / "depth")
    shutil.copytree(os.path.join(golden_dir, "scene3", "camera_pose"), work / "camera_pose")
    tool = os.path.join(ROOT, PKG, "other_tools", "integrate_tsdf.py")
    args = ["--voxel-size", "8", "--trunc", "24", "--origin", "-300", "-300", "-300", "--dims", "75", "75", "75", "--min-weight", "1"]
    env = dict(os.environ, PYTHONPATH=ROOT, R3D_FX="20", R3D_FY="20", R3D_CX="15.5", R3D_CY="11.5")
    r = subprocess.run([sys.executable, tool] + args + ["--mesh"], cwd=str(work), env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-1000:] + r.stderr[-2000:]
    xyz, nrm, tri = R.cloud_io.read_ply_mesh(str(work / "ply" / "tsdf_mesh.ply"))
    pxyz, pnrm = R.cloud_io.read_ply_normals(str(work / "ply" / "tsdf_surface.ply"))
    assert len(xyz) > 1000 and len(tri) > 1000
    assert np.array_equal(bits(xyz), bits(pxyz)) and np.array_equal(bits(nrm), bits(pnrm))
    lines = [l for l in r.stdout.split("\n") if l.startswith(("origin", "triangles"))]
    assert len(lines) == 2 and lines[1] == "triangles %d -> ./ply/tsdf_mesh.ply" % len(tri)
