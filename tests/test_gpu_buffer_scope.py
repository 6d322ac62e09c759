"""GPU: every host-array form releases the device buffers it made, on return and when the device call under it raises.
Context.alloc is wrapped here (nothing in the package knows), so every DeviceBuffer a call creates is recorded; afterwards each
must have ptr None.  The shapes are the smallest that still reach every allocation of a form: 64-point clouds (and 0 points
where a form takes them), a tetrahedron, 2 frames of 8 x 8 depth, a 16^3 volume holding a sphere.  The exception path swaps the
device-level callee of one form per module for a function that raises: the GPU is never asked to fail."""
import importlib

import numpy as np
import pytest

from helpers import PKG, r3d as _r3d

pytestmark = pytest.mark.gpu

K8 = (8.0, 8.0, 3.5, 3.5)                       # intrinsics of the 8 x 8 camera
POSE = np.array([1, 0, 0, 0, 1, 0, 0, 0, 1, -8, -8, 12], np.float64)   # world -> camera: at (8, 8, -12), looking along +z
QUAT, TS = np.array([[0.0, 0.0, 0.0, 1.0]]), POSE[9:].reshape(1, 3)
TET_XYZ = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0], [0, 0, 1]], np.float32)
TET_TRI = np.array([[0, 2, 1], [0, 1, 3], [0, 3, 2], [1, 2, 3]], np.int32)


@pytest.fixture(scope="module")
def R():
    return _r3d()


def sub(name):
    return importlib.import_module(PKG + "." + name)


@pytest.fixture(scope="module")
def ctx(R):
    c = R.Context(0)
    yield c
    c.close()


@pytest.fixture
def made(R, monkeypatch):
    """the DeviceBuffers created while the test runs"""
    out, real = [], R.Context.alloc

    def alloc(self, nbytes):
        out.append(real(self, nbytes))
        return out[-1]
    monkeypatch.setattr(R.Context, "alloc", alloc)
    return out


def all_freed(made, at_least=1):
    assert len(made) >= at_least, "the call made %d buffers, expected at least %d" % (len(made), at_least)
    held = [(i, b.nbytes) for i, b in enumerate(made) if b.ptr is not None]
    assert not held, "buffers (creation order, bytes) still held: %s of %d" % (held, len(made))
    del made[:]


def boom(*args, **kwargs):
    raise RuntimeError("boom")


def cloud(seed=0, n=64):
    return np.random.default_rng(seed).uniform(-1.0, 1.0, (n, 3)).astype(np.float32)


def two_planes():
    """40 points of z = 0 and 24 of x = 2"""
    p = cloud(3)
    p[:40, 2] = 0.0
    p[40:, 0] = 2.0
    return p


def words(n, seed=1):
    return np.random.default_rng(seed).integers(0, 1 << 24, n).astype(np.uint32)


EMPTY = np.zeros((0, 3), np.float32)
NO_TRI = np.zeros((0, 3), np.int32)
IDENTITY = np.float64([1, 0, 0, 0, 1, 0, 0, 0, 1, 0, 0, 0])      # a world -> camera row
MAPS = (np.ones((8, 8, 3), np.float32),) * 3                    # source vertex, model vertex and model normal maps


def test_download_array_of_zero_extent_shapes(ctx):
    buf = ctx.alloc(0)
    try:
        for dtype, shape in ((np.float32, (0, 3)), (np.uint32, (0,)), (np.uint8, (2, 0, 8, 3)), (np.float64, (0, 6))):
            a = buf.download_array(dtype, shape)
            assert a.shape == shape and a.dtype == dtype
        data = np.arange(12, dtype=np.int32)
        full = ctx.alloc(data.nbytes).upload(data)
        try:
            got = full.download_array(np.int32, (2, 2, 3))
            assert got.shape == (2, 2, 3) and got.dtype == np.int32 and np.array_equal(got.reshape(-1), data)
            assert full.download_array(np.int32, (0, 3)).shape == (0, 3)
        finally:
            full.free()
    finally:
        buf.free()


def test_evaluation_forms(R, ctx, made):
    E = sub("evaluation")
    for src in (cloud(), EMPTY):
        d, i = E.cloud_to_cloud_distance(src, cloud(1), ctx=ctx)
        assert d.shape == i.shape == (len(src),)
        all_freed(made, 4)
        out = E.cloud_to_mesh_distance(src, TET_XYZ, TET_TRI, signed=True, return_closest=True, ctx=ctx)
        assert out[2].shape == (len(src), 3)
        all_freed(made, 6)
        E.distance_stats(d, thresholds=(0.1,), bin_width=0.1, n_bins=4, ctx=ctx)
        all_freed(made)
        assert E.distance_colors(d, 1.0, ctx=ctx).shape == d.shape
        all_freed(made, 2)
    E.cloud_to_mesh_distance(cloud(), EMPTY, NO_TRI, ctx=ctx)
    all_freed(made, 5)
    E.evaluate_reconstruction(cloud(), cloud(1), 0.2, ctx=ctx, return_distances=True)
    all_freed(made, 6)
    E.evaluate_reconstruction((TET_XYZ, TET_TRI), cloud(1), 0.2, ctx=ctx)
    all_freed(made, 6)


def test_outlier_and_normal_forms(R, ctx, made):
    O, N = sub("outliers"), sub("normals")
    assert O.knn(cloud(), 4, ctx=ctx)[0].shape == (64, 4)
    all_freed(made, 3)
    assert len(O.remove_statistical_outlier(cloud(), 4, 2.0, ctx=ctx).rows) > 0       # the kept rows' two buffers are reached
    all_freed(made, 5)
    assert len(O.remove_radius_outlier(cloud(), 1, 10.0, ctx=ctx).rows) == 64
    all_freed(made, 5)
    N.estimate_normals(cloud(), 8, ctx=ctx)
    all_freed(made, 4)
    N.estimate_covariances(cloud(), 8, ctx=ctx)
    all_freed(made, 3)
    assert sub("icp").organized_normals(cloud(), 8, 8, ctx=ctx).shape == (64, 3)
    all_freed(made, 2)
    for form in (lambda: O.knn(EMPTY, 4, ctx=ctx), lambda: O.remove_statistical_outlier(EMPTY, 4, ctx=ctx),
                 lambda: O.remove_radius_outlier(EMPTY, 1, 1.0, ctx=ctx), lambda: N.estimate_normals(EMPTY, 8, ctx=ctx)):
        form()
        all_freed(made, 0)


def test_colour_and_registration_forms(R, ctx, made):
    CI, REG, N, PG = sub("colored_icp"), sub("registration"), sub("normals"), sub("posegraph")
    tgt, src = cloud(), cloud()[:48] + np.float32(0.01)
    nrm = N.estimate_normals(tgt, 8, ctx=ctx).normals
    all_freed(made)
    CI.colour_gradients(tgt, words(64), nrm, ctx=ctx)
    all_freed(made, 6)
    CI.icp_colored(src, words(48, 2), tgt, words(64), tgt_normals=nrm, init=np.eye(4), max_iter=2, ctx=ctx)
    all_freed(made, 13)
    f = REG.compute_fpfh(tgt, k=8, ctx=ctx)
    all_freed(made, 5)
    REG.compute_fpfh(tgt, nrm, k=8, ctx=ctx)
    all_freed(made, 5)
    REG.match_features(f.fpfh, f.fpfh[::-1], mutual=False, ctx=ctx)
    all_freed(made, 5)
    corr = np.stack([np.arange(48), np.arange(48)], axis=1)
    assert REG.registration_ransac(src, tgt, corr, 0.1, num_hypotheses=16, want_counts=True, ctx=ctx).counts.shape == (16,)
    all_freed(made, 5)
    PG.evaluate_registration(src, tgt, np.eye(4), 0.1, ctx=ctx)
    all_freed(made, 4)
    PG.registration_information(src, tgt, np.eye(4), 0.1, ctx=ctx)
    all_freed(made, 4)


def test_mesh_forms(R, ctx, made):
    M = sub("mesh")
    for xyz, tri in ((TET_XYZ, TET_TRI), (EMPTY, NO_TRI)):
        nv = len(xyz)
        assert len(M.mesh_components(tri, nv, ctx=ctx).components) == (1 if nv else 0)      # 1: the component rows' buffer is reached
        all_freed(made, 4 if nv else 3)
        M.remove_small_components(xyz, xyz, tri, colors=np.arange(nv), ctx=ctx)
        all_freed(made, 8)
        M.mesh_adjacency(tri, nv, ctx=ctx)
        all_freed(made, 4)
        M.smooth_mesh(xyz, tri, iterations=1, normals=xyz, lock_boundary=False, ctx=ctx)
        all_freed(made, 8)
        M.compute_vertex_normals(xyz, tri, fallback=xyz, ctx=ctx)
        all_freed(made, 4)


def test_segmentation_forms(R, ctx, made):
    S = sub("segmentation")
    assert len(S.segment_plane(two_planes(), 0.01, 64, ctx=ctx).rows) >= 24
    all_freed(made, 4)
    planes, _, _ = S.segment_planes(two_planes(), 0.01, 64, max_planes=2, min_inliers=3, ctx=ctx)
    assert len(planes) == 2                                                              # the second round runs on compacted rows
    all_freed(made, 6)


def frames():
    return np.full((2, 8, 8), 2.0, np.float32), np.tile(QUAT, (2, 1)), np.zeros((2, 3))


def test_consistency_and_tracking_forms(R, ctx, made):
    CO, TR = sub("consistency"), sub("tracking")
    d, q, t = frames()
    rgb = np.random.default_rng(5).integers(0, 256, (2, 8, 8, 3)).astype(np.uint8)
    xyz, keep = CO.fuse_frames_consistent(d, q, t, K8, radius=1, min_consistent=1, ctx=ctx)
    assert keep.any() and len(xyz) == keep.sum()                                         # the compacted rows' buffer is reached
    all_freed(made, 5)
    xyz, rgba, keep = CO.fuse_frames_consistent(d, q, t, K8, radius=1, min_consistent=1, rgb=rgb, ctx=ctx)
    assert keep.any() and len(rgba) == keep.sum()
    all_freed(made, 8)
    assert TR.depth_half(d[0], 0.05, ctx=ctx).shape == (4, 4)
    all_freed(made, 2)
    TR.depth_bilateral(d[0], 1, 1.0, 0.05, ctx=ctx)
    all_freed(made, 2)
    intensity, packed = TR.intensity_map(rgb[0], d[0], 0.05, ctx=ctx)
    all_freed(made, 4)
    vertex = R.unproject(d[0], K8, ctx=ctx).reshape(8, 8, 3)
    del made[:]
    TR.track_sums(vertex, vertex, np.tile(np.float32([0, 0, -1]), (8, 8, 1)), IDENTITY, np.eye(4), K8, 0.1, src_normal=vertex, ctx=ctx)
    all_freed(made, 7)
    dev = TR.TrackDevice(vertex, vertex, vertex, IDENTITY, np.eye(4), K8, ctx=ctx, src_intensity=intensity, model_packed=packed)
    dev.sums_rgb(0.1)
    assert all(b.ptr is not None for b in made) and len(made) == 9                      # a long-lived owner: held until free()
    dev.free()
    all_freed(made, 9)


def sphere_volume(R, ctx, color):
    """a 16^3 volume (voxel 1, truncation 3) holding a sphere of radius 5, every voxel seen once"""
    L = sub("_lib")
    vol = R.TSDFVolume((0.0, 0.0, 0.0), 1.0, (16, 16, 16), 3.0, ctx=ctx, color=color)
    c = np.arange(16, dtype=np.float32) - np.float32(7.5)
    dist = np.sqrt(c[None, None, :] ** 2 + c[None, :, None] ** 2 + c[:, None, None] ** 2) - np.float32(5.0)
    raw = np.ascontiguousarray(np.stack([dist.reshape(-1), np.ones(16 ** 3, np.float32)], axis=1), dtype=np.float32)
    p, n = vol.device_view()
    assert raw.shape == (n, 2)
    L.check(ctx.lib.r3d_memcpy_h2d(ctx.handle, p, raw.ctypes.data, raw.nbytes))
    ctx.sync()
    return vol


def test_tsdf_forms(R, ctx, made):
    vol = sphere_volume(R, ctx, color=True)
    try:
        xyz, _, rgb = vol.extract_point_cloud(with_colors=True)
        assert len(xyz) > 0 and rgb.shape == xyz.shape
        all_freed(made, 3)
        assert len(vol.extract_triangle_mesh(with_colors=True)[2]) > 0
        all_freed(made, 4)
        vol.extract_triangle_mesh(smooth={"iterations": 1})
        all_freed(made, 8)
        out = vol.extract_triangle_mesh(with_colors=True, min_component_triangles=2, keep_largest=True, with_stats=True, smooth=("laplacian", 1))
        assert out[-1]["components_kept"] == 1
        all_freed(made, 15)
        depth, vertex, normal, image = vol.raycast(QUAT, TS, (8, 8), K8, with_colors=True)
        assert (depth > 0).any()
        all_freed(made, 4)
        vol.track(depth[0], POSE, K8, n_iters=2, rgb=image[0], bilateral=(1, 1.0, 0.05))
        assert sum(b.ptr is not None for b in made) == 2 and len(made) == 4           # the volume keeps its bilateral pair
        vol.track(depth[0], POSE, K8, pyramid_iters=(1, 1), bilateral=(1, 1.0, 0.05))
        assert sum(b.ptr is not None for b in made) == 2 and len(made) == 5           # and uses it again
        TOOL = sub("other_tools.integrate_tsdf")
        assert TOOL.raycast_depth(R, vol, QUAT, TS, (8, 8), 1.0).shape == (1, 8, 8)
        assert TOOL.raycast_color(R, vol, QUAT, TS, (8, 8), 1.0).shape == (1, 8, 8, 3)
    finally:
        vol.close()
    all_freed(made, 7)
    plain = sphere_volume(R, ctx, color=False)
    try:
        try:
            plain.track_and_integrate(np.stack([depth[0], depth[0]]), POSE, K8, n_iters=1)
        except RuntimeError:      # "cannot be tracked" is a result here, not a failure: the buffers still go
            pass
    finally:
        plain.close()
    all_freed(made, 1)


def test_voxel_and_surface_forms(R, ctx, made):
    V, S = sub("voxelmap"), sub("surface")
    assert len(V.voxel_down_sample(cloud(), 0.25, rgba=words(64), ctx=ctx).xyz) > 0
    all_freed(made, 4)
    assert len(V.voxel_down_sample(cloud(), 0.25, ctx=ctx).xyz) > 0
    all_freed(made, 3)
    codes = V.voxelize(cloud(), 0.25, ctx=ctx)[0]
    d_codes = ctx.alloc(codes.nbytes).upload(codes)
    del made[:]
    try:
        assert len(V.octree_records_device(d_codes.ptr, len(codes), ctx=ctx)[0]) > 0
    finally:
        d_codes.free()
    all_freed(made, 1)
    p = cloud(7)
    p /= np.linalg.norm(p, axis=1, keepdims=True)
    S.reconstruct_surface(p * np.float32(4.0), p, 1.0, rgb=np.full((64, 3), 200, np.uint8), min_component_triangles=1, smooth={"iterations": 1},
                          ctx=ctx)
    all_freed(made, 0)


FAILING = [  # (module, the callee that raises, the host form over it, the fewest buffers made before it raises)
    ("evaluation", "cloud_to_cloud_distance_device", lambda m, c: m.cloud_to_cloud_distance(cloud(), cloud(1), ctx=c), 4),
    ("outliers", "statistical_outlier_device", lambda m, c: m.remove_statistical_outlier(cloud(), 4, ctx=c), 3),
    ("outliers", "select_rows_device", lambda m, c: m.remove_radius_outlier(cloud(), 1, 10.0, ctx=c), 5),
    ("colored_icp", "intensity", lambda m, c: m.icp_colored(cloud()[:48], words(48), cloud(), words(64), tgt_normals=cloud(9), ctx=c), 8),
    ("registration", "match_features_device", lambda m, c: m.match_features(np.ones((8, 33), np.float32), np.ones((8, 33), np.float32), ctx=c), 5),
    ("registration", "registration_ransac_device",
     lambda m, c: m.registration_ransac(cloud(), cloud(), np.stack([np.arange(8), np.arange(8)], axis=1), 0.1, 16, ctx=c), 4),
    ("mesh", "mesh_components_device", lambda m, c: m.mesh_components(TET_TRI, 4, ctx=c), 3),
    ("mesh", "remove_small_components_device", lambda m, c: m.remove_small_components(TET_XYZ, TET_XYZ, TET_TRI, ctx=c), 6),
    ("mesh", "vertex_normals_device", lambda m, c: m.smooth_mesh(TET_XYZ, TET_TRI, iterations=1, ctx=c), 7),
    ("segmentation", "segment_plane_device", lambda m, c: m.segment_planes(two_planes(), 0.01, 64, ctx=c), 2),
    ("segmentation", "select_rows_device", lambda m, c: m.segment_plane(two_planes(), 0.01, 64, ctx=c), 4),
    ("posegraph", "registration_sums_device", lambda m, c: m.evaluate_registration(cloud()[:48], cloud(), np.eye(4), 0.1, ctx=c), 4),
    ("consistency", "depth_consistency_device", lambda m, c: m.fuse_frames_consistent(*frames(), K8, radius=1, ctx=c), 4),
    ("consistency", "compact_rows_device", lambda m, c: m.fuse_frames_consistent(*frames(), K8, radius=1, min_consistent=1, ctx=c), 5),
    ("tracking", "TrackDevice.sums", lambda m, c: m.track_sums(*MAPS, IDENTITY, np.eye(4), K8, 0.1, ctx=c), 6),
    ("tracking", "TrackDevice.state_reset", lambda m, c: m.TrackDevice(*MAPS, IDENTITY, np.eye(4), K8, ctx=c), 6),
    ("icp", "NNIndex.normals_knn", lambda m, c: sub("normals").estimate_normals(cloud(), 8, ctx=c), 4),
    ("icp", "NNIndex.normals_knn", lambda m, c: sub("registration").compute_fpfh(cloud(), k=8, ctx=c), 2),
]


@pytest.mark.parametrize("module,callee,form,fewest", FAILING, ids=["%s-%s-%d" % (f[0], f[1], i) for i, f in enumerate(FAILING)])
def test_buffers_go_when_the_device_call_raises(R, ctx, made, monkeypatch, module, callee, form, fewest):
    m = owner = sub(module)
    *path, name = callee.split(".")
    for part in path:
        owner = getattr(owner, part)
    monkeypatch.setattr(owner, name, boom)
    with pytest.raises(RuntimeError, match="boom"):
        form(m, ctx)
    all_freed(made, fewest)


def test_buffers_go_when_a_volume_or_grid_call_raises(R, ctx, made, monkeypatch):
    T, M, V = sub("tsdf"), sub("mesh"), sub("voxelmap")
    vol = sphere_volume(R, ctx, color=False)
    try:
        with monkeypatch.context() as mp:
            mp.setattr(T.TSDFVolume, "raycast_device", boom)
            with pytest.raises(RuntimeError, match="boom"):
                vol.raycast(QUAT, TS, (8, 8), K8)
            all_freed(made, 3)
            with pytest.raises(RuntimeError, match="boom"):
                sub("other_tools.integrate_tsdf").raycast_depth(R, vol, QUAT, TS, (8, 8), 1.0)
            all_freed(made, 1)
        with monkeypatch.context() as mp:
            mp.setattr(M, "gather_rows_device", boom)
            with pytest.raises(RuntimeError, match="boom"):
                vol.extract_triangle_mesh(keep_largest=True)
            all_freed(made, 8)
        with monkeypatch.context() as mp:
            mp.setattr(T.TSDFVolume, "track_device", boom)
            with pytest.raises(RuntimeError, match="boom"):
                vol.track(np.full((8, 8), 2.0, np.float32), POSE, K8)
            all_freed(made, 1)
    finally:
        vol.close()
    real = V.VoxelGrid.extract_device

    def extract(self, d_xyz_out=None, *args, **kwargs):
        if d_xyz_out is not None:
            boom()
        return real(self, d_xyz_out, *args, **kwargs)
    monkeypatch.setattr(V.VoxelGrid, "extract_device", extract)
    with pytest.raises(RuntimeError, match="boom"):
        V.voxel_down_sample(cloud(), 0.25, ctx=ctx)
    all_freed(made, 3)
