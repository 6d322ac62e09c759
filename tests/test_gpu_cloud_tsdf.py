"""GPU: r3d_tsdf_integrate_cloud against its restatement (tests/cloud_tsdf_ref.py), the whole {tsdf, weight} plane (and the colour
plane) bit for bit and the count of updated voxels equal.  The cloud, the normals and the colours sit inside guarded allocations
(test_gpu_bounds.Guarded) that must come back untouched; the planes are the volume's own allocations and are compared whole, so a
stray write inside them shows as a difference.  Shapes are the smallest at which the band scheme can go wrong: blocks of 4 x 4 x 4
voxels that hang over the volume's faces, more than one 1024-point tile of the index, more than one chunk of blocks."""
import ctypes as C
import importlib

import numpy as np
import pytest

import cloud_tsdf_ref as CT
import tsdf_color_ref as TC
import tsdf_ref as REF
from helpers import PKG, r3d as _r3d
from test_cloud_tsdf_host import RMS_BOUND, radial_rms, sphere_volume
from test_gpu_bounds import Guarded

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def R():
    return _r3d()


@pytest.fixture(scope="module")
def L():
    return importlib.import_module(PKG + "._lib")


@pytest.fixture(scope="module")
def ctx(R):
    c = R.Context(0)
    yield c
    c.close()


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def planes(V):
    """(vol [n,2] float32, col [n,4] uint32 or None) of a device volume"""
    t, w = V.volume()
    vol = np.stack([t.reshape(-1), w.reshape(-1)], axis=1)
    if not V.color:
        return vol, None
    s, n = V.colors()
    return vol, np.concatenate([s.reshape(-1, 3), n.reshape(-1, 1)], axis=1)


def put(V, vol):
    """vol [n,2] float32 into the device volume"""
    raw = np.ascontiguousarray(vol, np.float32)
    p, n = V.device_view()
    assert raw.shape == (n, 2)
    V.ctx.lib.r3d_memcpy_h2d(V.ctx.handle, p, raw.ctypes.data, raw.nbytes)
    V.ctx.sync()


def cloud_into(R, V, xyz, normals, rgba=None):
    """the device entry point on V: an index over the guarded cloud, guarded normals and colours; returns the touched count"""
    icp = importlib.import_module(PKG + ".icp")
    xyz, normals = np.ascontiguousarray(xyz, np.float32), np.ascontiguousarray(normals, np.float32)
    ctx = V.ctx
    bufs = [Guarded(ctx, xyz.nbytes, 0, xyz, seed=1), Guarded(ctx, normals.nbytes, 0, normals, seed=2)]
    if rgba is not None:
        bufs.append(Guarded(ctx, 4 * len(xyz), 0, np.ascontiguousarray(rgba, np.uint32), seed=3))
    index = icp.NNIndex(ctx, bufs[0].ptr, len(xyz))
    try:
        touched = V.integrate_cloud_device(index, bufs[1].ptr, None if rgba is None else bufs[2].ptr, want_count=True)
        for b in bufs:
            b.unchanged()
        return touched
    finally:
        index.close()
        for b in bufs:
            b.free()


def check(R, ctx, geo, clouds, start=None, color=False):
    """clouds: (xyz, normals[, rgba]) tuples applied in order to a fresh volume of geo = (origin, vs, dims, tr) (or to `start`, a
    [n,2] plane); after each, planes and count against the restatement.  Returns the final planes."""
    origin, vs, dims, tr = geo
    n = dims[0] * dims[1] * dims[2]
    want = np.zeros((n, 2), np.float32) if start is None else np.array(start, np.float32)
    want_col = np.zeros((n, 4), np.uint32) if color else None
    V = R.TSDFVolume(origin, vs, dims, tr, ctx=ctx, color=color)
    try:
        if start is not None:
            put(V, start)
        for cloud in clouds:
            xyz, normals = cloud[:2]
            rgba = cloud[2] if color else None
            if color:
                want, want_col, want_touched = CT.integrate_cloud(want, origin, vs, dims, tr, xyz, normals, want_col, rgba)
            else:
                want, want_touched = CT.integrate_cloud(want, origin, vs, dims, tr, xyz, normals)
            touched = cloud_into(R, V, xyz, normals, rgba)
            vol, col = planes(V)
            bad = np.flatnonzero((bits(vol) != bits(want)).any(axis=1))
            assert bad.size == 0, "%d voxels differ, first %d: got %s want %s" % (bad.size, bad[0], vol[bad[0]], want[bad[0]])
            assert touched == want_touched, (touched, want_touched)
            if color:
                assert np.array_equal(col, want_col)
        return vol, col
    finally:
        V.close()


def random_cloud(n, lo, hi, seed, unit=True):
    rng = np.random.default_rng(seed)
    xyz = rng.uniform(lo, hi, size=(n, 3)).astype(np.float32)
    nrm = rng.normal(size=(n, 3))
    if unit:
        nrm /= np.linalg.norm(nrm, axis=1, keepdims=True)
    return xyz, nrm.astype(np.float32)


GEO = ((-1.0, -0.85, -0.65), 0.1, (20, 17, 13), 0.3)     # odd sizes: blocks hang over two faces


def test_sphere(R, ctx):
    want, want_touched, (origin, vs, dims, tr, xyz, normals) = sphere_volume(4)
    vol, _ = check(R, ctx, (origin, vs, dims, tr), [(xyz, normals)])
    assert np.array_equal(bits(vol), bits(want)) and want_touched == 9582


def test_more_than_one_index_tile(R, ctx):
    xyz, nrm = random_cloud(2500, (-1.0, -0.85, -0.65), (1.0, 0.85, 0.65), 5)
    check(R, ctx, GEO, [(xyz, nrm)])


@pytest.mark.parametrize("dims,n", [((5, 7, 3), 40), ((1, 1, 1), 5), ((9, 9, 9), 1), ((4, 4, 4), 3), ((8, 5, 4), 64)], ids=str)
def test_small_volumes_and_clouds(R, ctx, dims, n):
    hi = np.array(dims) * 0.25
    xyz, nrm = random_cloud(n, (0, 0, 0), hi, 11)
    vol, _ = check(R, ctx, ((0.0, 0.0, 0.0), 0.25, dims, 0.6), [(xyz, nrm)])
    assert vol[:, 1].sum() > 0


def test_empty_cloud(R, ctx, L):
    start = np.random.default_rng(3).normal(size=(5 * 7 * 3, 2)).astype(np.float32)
    V = R.TSDFVolume((0.0, 0.0, 0.0), 0.25, (5, 7, 3), 0.6, ctx=ctx)
    try:
        put(V, start)
        assert V.integrate_cloud(np.zeros((0, 3), np.float32), np.zeros((0, 3), np.float32)) == 0
        assert np.array_equal(bits(planes(V)[0]), bits(start))
    finally:
        V.close()


LINE = ((0.0, 0.0, 0.0), 0.125, (8, 1, 1), 0.5)          # vs and tr are representable: centres at 0.0625 + 0.125 k
Y = np.float32(0.0625)


def edge_clouds():
    cx = CT.centres(*LINE[:3])[0]
    at = np.float32(cx[0] + np.float32(0.5))
    a, b = [cx[3] - np.float32(0.25), Y, Y], [cx[3] + np.float32(0.25), Y, Y]
    near, nearer = [cx[3] + np.float32(0.01), Y, Y], [cx[3], Y, Y]
    return {
        "exactly_tr": ([[at, Y, Y]], [[1, 0, 0]]),
        "just_past_tr": ([[np.nextafter(at, np.float32(2)), Y, Y]], [[1, 0, 0]]),
        "tie_ab": ([a, b], [[1, 0, 0], [1, 0, 0]]),
        "tie_ba": ([b, a], [[1, 0, 0], [1, 0, 0]]),
        "nan_inf_rows": ([[np.nan, Y, Y], nearer, [np.inf, Y, Y], [0.3, -np.inf, Y], [0.2, Y, np.nan]], [[1, 0, 0]] * 5),
        "zero_normal_wins": ([nearer, near], [[0, 0, 0], [1, 0, 0]]),
        "nan_normal_wins": ([nearer, near], [[0, np.nan, 1], [1, 0, 0]]),
        "inf_normal_wins": ([nearer, near], [[np.inf, 0, 0], [1, 0, 0]]),
        "outside_reaching_in": ([[-0.3, Y, Y], [1.2, 0.3, -0.2], [0.5, 0.5, Y]], [[1, 0, 0], [0, 1, 0], [0, 0, 1]]),
        "far_outside": ([[-5.0, Y, Y], [0.5, 40.0, Y], [1e30, Y, Y], [0.5, Y, -1e20]], [[1, 0, 0]] * 4),
        "long_normals": ([nearer, [0.9, Y, Y]], [[100, 0, 0], [-1e30, 1e30, 1e30]]),
        "huge_normals": ([[cx[3], Y + np.float32(0.3), Y - np.float32(0.3)]], [[3.4e38, -3.4e38, 3.4e38]]),
    }


@pytest.mark.parametrize("name", list(edge_clouds()))
def test_edges_of_the_rule(R, ctx, name):
    xyz, nrm = (np.array(a, np.float32) for a in edge_clouds()[name])
    start = np.zeros((8, 2), np.float32)
    start[:, 0], start[:, 1] = 0.25, np.arange(8) % 3      # voxels with and without history
    vol, _ = check(R, ctx, LINE, [(xyz, nrm)], start=start)
    w = vol[:, 1] - start[:, 1]
    if name == "exactly_tr":
        assert w[0] == 1
    if name == "just_past_tr":
        assert w[0] == 0 and w[1] == 1
    if name in ("tie_ab", "tie_ba"):
        fresh, _ = check(R, ctx, LINE, [(xyz, nrm)])
        assert fresh[3, 0] == (0.5 if name == "tie_ab" else -0.5)               # the lowest index wins
    if name in ("zero_normal_wins", "nan_normal_wins", "inf_normal_wins"):
        assert w[3] == 0 and w[4] == 1                                          # skipped, not given to the runner-up
    if name == "far_outside":
        assert not w.any() and np.array_equal(bits(vol), bits(start))
    if name == "outside_reaching_in":
        assert w[0] == 1 and w[7] == 1 and w[4] == 1


def test_compose_with_a_depth_frame(R, ctx):
    from test_gpu_tsdf import device_volume, integrate_device
    T = importlib.import_module(PKG + ".tsdf")
    s = REF.wall_scene()
    V = device_volume(T, ctx, s)
    try:
        integrate_device(ctx, V, s)
        after_frame = planes(V)[0]
    finally:
        V.close()
    assert after_frame[:, 1].sum() > 0
    lo = np.array(s["origin"])
    # five points: their balls of radius tr hold at most 5 x 0.0142 of the volume's 0.192 m^3, so voxels without the cloud remain
    xyz, nrm = random_cloud(5, lo, lo + np.array(s["dims"]) * s["vs"], 21)
    vol, _ = check(R, ctx, (s["origin"], s["vs"], s["dims"], s["tr"]), [(xyz, nrm)], start=after_frame)
    added = vol[:, 1] - after_frame[:, 1]
    assert set(np.unique(added)) == {0.0, 1.0} and vol[:, 1].max() == 2
    assert np.array_equal(bits(vol[added == 0]), bits(after_frame[added == 0]))


def test_compose_clouds(R, ctx):
    a = random_cloud(400, (-1.0, -0.85, -0.65), (0.6, 0.85, 0.65), 31)
    b = random_cloud(300, (-0.4, -0.85, -0.65), (1.0, 0.85, 0.65), 32)
    twice, _ = check(R, ctx, GEO, [a, a])
    once, _ = check(R, ctx, GEO, [a])
    assert np.array_equal(twice[:, 1], 2 * once[:, 1])
    assert np.array_equal(bits(twice[:, 0]), bits(once[:, 0]))                 # (t * 1 + t) / 2 is t: every step is exact
    ab, _ = check(R, ctx, GEO, [a, b])
    ba, _ = check(R, ctx, GEO, [b, a])
    assert np.array_equal(ab[:, 1], ba[:, 1]) and ab[:, 1].max() == 2
    assert np.array_equal(bits(ab[:, 0]), bits(ba[:, 0]))                      # (a * 1 + b) / 2: the f32 sum is commutative


def test_colour_volume(R, ctx):
    rng = np.random.default_rng(41)
    a = random_cloud(500, (-1.0, -0.85, -0.65), (1.0, 0.85, 0.65), 41) + (rng.integers(0, 1 << 24, 500).astype(np.uint32),)
    b = random_cloud(200, (-1.0, -0.85, -0.65), (1.0, 0.85, 0.65), 42) + (rng.integers(0, 1 << 32, 200, dtype=np.uint64).astype(np.uint32),)
    vol, col = check(R, ctx, GEO, [a, b], color=True)
    assert np.array_equal(col[:, 3], vol[:, 1].astype(np.uint32)) and col[:, 3].max() == 2
    plain, _ = check(R, ctx, GEO, [a[:2], b[:2]])
    assert np.array_equal(bits(plain), bits(vol))                              # the colour changes no bit of the tsdf plane


def test_argument_errors_leave_the_volume_untouched(R, L, ctx):
    icp = importlib.import_module(PKG + ".icp")
    xyz, nrm = random_cloud(50, (0, 0, 0), (1, 1, 1), 51)
    start = np.random.default_rng(52).normal(size=(64, 2)).astype(np.float32)
    other = R.Context(0)
    d_xyz, d_nrm, d_rgba = ctx.alloc(xyz.nbytes).upload(xyz), ctx.alloc(nrm.nbytes).upload(nrm), ctx.alloc(200).upload(np.zeros(50, np.uint32))
    o_xyz = other.alloc(xyz.nbytes).upload(xyz)
    index, foreign = icp.NNIndex(ctx, d_xyz.ptr, 50), icp.NNIndex(other, o_xyz.ptr, 50)
    V, VC = R.TSDFVolume((0, 0, 0), 0.25, (4, 4, 4), 0.5, ctx=ctx), R.TSDFVolume((0, 0, 0), 0.25, (4, 4, 4), 0.5, ctx=ctx, color=True)
    try:
        put(V, start)
        put(VC, start)
        n = C.c_int64(-7)
        lib = ctx.lib
        calls = [(lib.r3d_tsdf_integrate_cloud, (V.handle, index.handle, d_nrm.ptr, d_rgba.ptr, C.byref(n))),     # colours, no plane
                 (lib.r3d_tsdf_integrate_cloud, (VC.handle, index.handle, d_nrm.ptr, None, C.byref(n))),          # a plane, no colours
                 (lib.r3d_tsdf_integrate_cloud, (V.handle, foreign.handle, d_nrm.ptr, None, C.byref(n))),         # another context's index
                 (lib.r3d_tsdf_integrate_cloud, (V.handle, None, d_nrm.ptr, None, C.byref(n))),
                 (lib.r3d_tsdf_integrate_cloud, (V.handle, index.handle, None, None, C.byref(n))),
                 (lib.r3d_tsdf_integrate_cloud, (None, index.handle, d_nrm.ptr, None, C.byref(n))),
                 (lib.r3d_tsdf_integrate_cloud_host, (V.handle, xyz.ctypes.data, nrm.ctypes.data, xyz.ctypes.data, 50, C.byref(n))),
                 (lib.r3d_tsdf_integrate_cloud_host, (VC.handle, xyz.ctypes.data, nrm.ctypes.data, None, 50, C.byref(n))),
                 (lib.r3d_tsdf_integrate_cloud_host, (V.handle, None, nrm.ctypes.data, None, 50, C.byref(n))),
                 (lib.r3d_tsdf_integrate_cloud_host, (V.handle, xyz.ctypes.data, nrm.ctypes.data, None, -1, C.byref(n)))]
        for fn, args in calls:
            assert fn(*args) == L.ERR_INVALID, args
            assert L.last_error()
        assert n.value == -7
        for vol in (V, VC):
            got, col = planes(vol)
            assert np.array_equal(bits(got), bits(start)) and (col is None or not col.any())
        with pytest.raises(ValueError):
            V.integrate_cloud(xyz, nrm, rgb=np.zeros((50, 3), np.uint8))
        with pytest.raises(ValueError):
            VC.integrate_cloud(xyz, nrm)
        with pytest.raises(ValueError):
            V.integrate_cloud(xyz, nrm[:49])
        with pytest.raises(ValueError):
            VC.integrate_cloud(xyz, nrm, rgb=np.zeros((50, 3), np.float32))
    finally:
        for obj in (V, VC, index, foreign):
            obj.close()
        for b in (d_xyz, d_nrm, d_rgba):
            b.free()
        o_xyz.free()
        other.close()


def test_asynchronous_call_without_a_count(R, ctx):
    """n_touched_out == NULL: the call returns with its launches enqueued; two of them back to back, then one synchronise"""
    icp = importlib.import_module(PKG + ".icp")
    a = random_cloud(400, (-1.0, -0.85, -0.65), (1.0, 0.85, 0.65), 81)
    b = random_cloud(150, (-1.0, -0.85, -0.65), (1.0, 0.85, 0.65), 82)
    want, _ = check(R, ctx, GEO, [a, b])
    V = R.TSDFVolume(*GEO, ctx=ctx)
    made = []
    try:
        for xyz, nrm in (a, b):
            d_xyz, d_nrm = ctx.alloc(xyz.nbytes).upload(xyz), ctx.alloc(nrm.nbytes).upload(nrm)
            index = icp.NNIndex(ctx, d_xyz.ptr, len(xyz))
            made += [index, d_xyz, d_nrm]
            assert V.integrate_cloud_device(index, d_nrm.ptr) is None
        ctx.sync()
        assert np.array_equal(bits(planes(V)[0]), bits(want))
    finally:
        ctx.sync()
        for obj in made:
            obj.close() if hasattr(obj, "close") else obj.free()
        V.close()


@pytest.mark.parametrize("chunk", [1, 7])
def test_result_does_not_depend_on_the_chunk(R, ctx, chunk):
    xyz, nrm = random_cloud(300, (-1.0, -0.85, -0.65), (1.0, 0.85, 0.65), 61)
    assert ctx.get_tuning("tsdf_cloud_chunk") == 0
    ctx.set_tuning("tsdf_cloud_chunk", chunk)                                  # 5 x 5 x 4 blocks: many chunks
    try:
        check(R, ctx, GEO, [(xyz, nrm), (xyz[:100], nrm[:100])])
    finally:
        ctx.set_tuning("tsdf_cloud_chunk", 0)


def test_host_call_is_the_device_call_and_point_order_does_not_matter(R, ctx):
    xyz, nrm = random_cloud(700, (-1.0, -0.85, -0.65), (1.0, 0.85, 0.65), 71)      # random floats: no exact ties
    rgb = np.random.default_rng(72).integers(0, 256, (700, 3), dtype=np.uint8)
    want, want_col = check(R, ctx, GEO, [(xyz, nrm, TC.pack(rgb))], color=True)
    perm = np.random.default_rng(73).permutation(700)
    for order in (np.arange(700), perm):
        V = R.TSDFVolume(*GEO[:3], GEO[3], ctx=ctx, color=True)
        try:
            touched = V.integrate_cloud(xyz[order], nrm[order], rgb[order])
            vol, col = planes(V)
            assert np.array_equal(bits(vol), bits(want)) and np.array_equal(col, want_col) and touched == int(vol[:, 1].sum())
            assert V.integrate_cloud(xyz[order], nrm[order], rgb[order]) == touched          # the volume's buffers serve a second call
            assert np.array_equal(planes(V)[0][:, 1], 2 * want[:, 1])
        finally:
            V.close()


def test_reconstruct_surface_end_to_end(R, ctx, tmp_path):
    _, _, (origin, vs, dims, tr, xyz, normals) = sphere_volume(4)
    rgb = CT.sphere_colors(normals)
    n = dims[0] * dims[1] * dims[2]
    want, want_col, _ = CT.integrate_cloud(np.zeros((n, 2), np.float32), origin, vs, dims, tr, xyz, normals, np.zeros((n, 4), np.uint32),
                                           TC.pack(rgb))
    ref = TC.ColorVolume(origin, vs, dims, tr)
    ref.tsdf, ref.w = want[:, 0].reshape(dims[::-1]).copy(), want[:, 1].reshape(dims[::-1]).copy()
    ref.sums, ref.n = want_col[:, :3].reshape(dims[::-1] + (3,)).copy(), want_col[:, 3].reshape(dims[::-1]).copy()
    got = R.reconstruct_surface(xyz, normals, 0.1, rgb=rgb, trunc_voxels=4, margin_voxels=2, ctx=ctx)
    v, vn, tri, colours = got
    want_xyz, want_nrm = REF.extract(ref, 1.0)
    assert np.array_equal(bits(v), bits(want_xyz)) and np.array_equal(bits(vn), bits(want_nrm))     # volume_for_cloud made the 24^3 case
    assert np.array_equal(colours, TC.extract_colors(ref, 1.0))                # the nearest samples' colours, interpolated
    # ... and so close to the colour of the sample nearest to the vertex itself: a voxel of the vertex's edge is within a voxel (0.1)
    # of it and within 0.1 + 0.07 of its own nearest sample (0.07: half the samples' spacing), the vertex within 0.07 of its: the two
    # samples are at most 0.34 apart, and the colour moves by 127.5 per unit length and is rounded once
    samples = rgb[nearest_sample(xyz, v)].astype(np.int32)
    assert np.abs(colours.astype(np.int32) - samples).max() <= 0.34 * 127.5 + 1
    _, _, boundary = R.mesh_adjacency(tri, len(v), ctx=ctx)
    assert len(tri) > 3000 and not boundary.any()                              # a closed surface
    comps = R.mesh_components(tri, len(v), ctx=ctx)
    assert len(comps.components) == 1 and comps.n_invalid == 0 and comps.components[0, 2] == len(tri)
    rms, worst = radial_rms(v)
    print("mesh: %d vertices, %d triangles, rms %.4e max %.4e (bound %.4e)" % (len(v), len(tri), rms, worst, RMS_BOUND))
    assert rms <= RMS_BOUND
    assert (np.einsum("ij,ij->i", vn, v) > 0).all()                            # the normals point out of the sphere
    # the tool: the same mesh from a PLY with normals and colours, read back equal
    tool = importlib.import_module(PKG + ".other_tools.reconstruct_surface")
    src, out = str(tmp_path / "sphere.ply"), str(tmp_path / "mesh.ply")
    R.cloud_io.write_ply_normals(src, xyz, normals, rgb=rgb)
    tool.main([src, out, "--voxel-size", "0.1", "--trunc-voxels", "4"])
    back = R.cloud_io.read_ply_mesh(out, with_colors=True)
    wide = R.reconstruct_surface(xyz, normals, 0.1, rgb=rgb, ctx=ctx)          # the tool's volume: the default margin
    assert len(back) == len(wide) == 4
    for a, b in zip(back, wide):
        assert a.dtype == b.dtype and a.shape == b.shape and np.array_equal(a.view(np.uint8), b.view(np.uint8))
    assert radial_rms(back[0])[0] <= RMS_BOUND and len(back[2]) > 3000


def nearest_sample(samples, points):
    """the index of the nearest sample of every point (float64, brute force)"""
    d = ((np.asarray(points, np.float64)[:, None, :] - np.asarray(samples, np.float64)[None, :, :]) ** 2).sum(axis=2)
    return np.argmin(d, axis=1)
