"""The catalogue of tests/test_gpu_call_order.py: one small case per entry point (or the shortest chain that gives an output),
each a function run(ctx, scale=1) -> bytes that builds its inputs from a fixed seed, runs on the context it is given, checks
the result against the restatement that pins its module (with that module's own generators, helpers and bounds: nothing new
is derived here) and returns every output concatenated as raw bytes.  scale = 4 gives the larger instance
test_small_behind_large runs first so that every workspace of the context has grown and holds foreign data.

Device objects that belong to a context (NN index, voxel set, voxel grid, TSDF volume) are made inside run on that context and
closed there.  COVERS maps each case to the csrc/*.hip files whose entry points it calls; tests/test_call_order_host.py keeps
it complete.

The tracking cases use the room volume of test_gpu_track.py at 0.1 m voxels (larger than the 33 x 17 x 9 the other volume
cases keep to): the room is the only scene the tracking restatements have a converging loop for."""
import importlib

import numpy as np

from helpers import PKG, r3d as _r3d


def _m(name):
    _r3d()
    return importlib.import_module(PKG + "." + name)


_MEMO = {}


def _memo(module, *names):
    """The restatements are pure functions of their arguments and a case runs hundreds of times on the same inputs: each is
    computed once per distinct argument list (keyed by the pickled arguments) and handed out again, unchanged."""
    import hashlib
    import pickle
    for name in names:
        fn = getattr(module, name)
        if getattr(fn, "_call_order_memo", False):
            continue

        def cached(*a, _fn=fn, _key=(module.__name__, name), **kw):
            key = _key + (hashlib.sha1(pickle.dumps((a, sorted(kw.items())), protocol=4)).hexdigest(),)
            if key not in _MEMO:
                _MEMO[key] = _fn(*a, **kw)
            return _MEMO[key]
        cached._call_order_memo = True
        setattr(module, name, cached)


def _memo_all():
    import bilateral_ref, mesh_ref, normals_ref, outliers_ref, photo_ref, project_ref, pyramid_ref, raycast_color_ref, raycast_ref
    import color_icp_ref, compare_ref, mesh_cc_ref, posegraph_ref
    import register_ref, segment_ref, sort_ref, track_ref, tsdf_color_ref, tsdf_ref
    from oracle import fusion_ref, icp_ref, octomap_ref, plane_ref
    _memo(register_ref, "ransac", "match", "nearest_rows", "fpfh")
    _memo(segment_ref, "segment_plane", "refit_bounds")
    _memo(outliers_ref, "knn", "sor", "ror_counts")
    _memo(normals_ref, "normals")
    _memo(track_ref, "track")
    _memo(pyramid_ref, "track", "depth_half")
    _memo(photo_ref, "track", "intensity_map")
    _memo(plane_ref, "icp_point_to_plane", "organized_normals", "quantile_lower")
    _memo(icp_ref, "nearest_neighbours", "synthetic_pair")
    _memo(tsdf_ref, "run", "random_scene", "extract")
    _memo(tsdf_color_ref, "extract_colors")
    _memo(raycast_ref, "raycast")
    _memo(raycast_color_ref, "raycast")
    _memo(mesh_ref, "extract_mesh")
    _memo(octomap_ref, "occupied_set", "write_bt_bytes")
    _memo(bilateral_ref, "depth_bilateral")
    _memo(project_ref, "grad_points_f32", "grad_P_f64", "grad_P_bound", "dense_inputs")
    _memo(fusion_ref, "fuse_frames", "apply_T")
    _memo(sort_ref, "stable_sort_by_bits", "few_values")
    _memo(posegraph_ref, "registration_sums")
    _memo(color_icp_ref, "knn_lists", "nearest", "gradients", "accumulate", "loop")
    _memo(mesh_cc_ref, "components", "filter_components")
    _memo(compare_ref, "mesh_distance", "distance_stats")


def _cat(*arrays):
    return b"".join(a if isinstance(a, bytes) else np.ascontiguousarray(a).tobytes() for a in arrays)


def _n(base, scale, cap=80_000):
    return min(base * scale, cap)


def _side(scale):
    return 2 if scale > 1 else 1


# ---- fusion and moves -----------------------------------------------------------------------------------------------------------
def fuse_host(ctx, scale=1):
    from oracle import fusion_ref as O
    from test_gpu_fusion import check, make_depth
    R, s = _r3d(), _side(scale)
    rng = np.random.default_rng(101)
    out = []
    for dt in (np.uint8, np.uint16):
        d = make_depth(rng, (3, 37 * s, 52 * s), dt)
        q, t = rng.normal(size=(3, 4)), rng.normal(size=(3, 3)) * 10
        want = O.fuse_frames(d, q, t)
        for odt in (np.float32, np.float64):
            got = R.fuse_frames(d, q, t, out_dtype=odt, ctx=ctx)
            check(got, want, odt)
            out.append(got)
    return _cat(*out)


def fuse_rgb_host(ctx, scale=1):
    from oracle import fusion_ref as O
    from test_gpu_fusion import _rgba_words, check, make_depth
    R, s = _r3d(), _side(scale)
    rng = np.random.default_rng(102)
    out = []
    for dt in (np.uint8, np.uint16):
        shape = (3, 37 * s, 52 * s)
        d = make_depth(rng, shape, dt)
        rgb = rng.integers(0, 256, size=shape + (3,), dtype=np.uint8)
        q, t = rng.normal(size=(3, 4)), rng.normal(size=(3, 3)) * 10
        xyz, rgba = R.fuse_frames_rgb(d, rgb, q, t, ctx=ctx)
        check(xyz, O.fuse_frames(d, q, t), np.float32)
        assert np.array_equal(rgba, _rgba_words(rgb))
        out += [xyz, rgba]
    return _cat(*out)


def apply_host(ctx, scale=1):
    import icp_parts_ref as REF
    from oracle import fusion_ref as O
    from test_gpu_fusion import check
    from test_gpu_icp_parts import apply_many
    R, L = _r3d(), _m("_lib")
    n = _n(5001, scale)
    rng = np.random.default_rng(103)
    p = (rng.normal(size=(n, 3)) * 50).astype(np.float32)
    T = REF.transforms(1, 7)[0]
    got = R.apply_T(p, T, ctx=ctx)
    check(got, O.apply_T(p, T).astype(np.float32), np.float32)
    Ts = REF.transforms(5, n)
    d_in, d_out = ctx.alloc(p.nbytes).upload(p), ctx.alloc(5 * p.nbytes)
    try:
        L.check(apply_many(ctx, L, d_in.ptr, np.float32, n, Ts, d_out.ptr, np.float32))
        many = d_out.download(np.float32, 5 * n * 3).reshape(5, n, 3)
    finally:
        d_in.free()
        d_out.free()
    want = REF.apply_many(p, Ts)
    for j in range(5):
        check(many[j], want[j].astype(np.float32), np.float32)
    return _cat(got, many)


def sort(ctx, scale=1):
    import sort_ref as REF
    from test_gpu_sort import check_sort
    keys = REF.few_values(_n(5000, scale), 11, 40, 257)
    return _cat(check_sort(ctx, _m("_lib"), keys, 0, 40, "public", "catalogue"))


# ---- the NN index and the ICP loops ----------------------------------------------------------------------------------------------
def nn_build_query(ctx, scale=1):
    from oracle import icp_ref as OI
    icp = _m("icp")
    rng = np.random.default_rng(104)
    m, n = _n(4000, scale), _n(3000, scale)
    tgt, src = (rng.random((m, 3)) * 10).astype(np.float32), (rng.random((n, 3)) * 10).astype(np.float32)
    oi, od = OI.nearest_neighbours(src, tgt)
    d_tgt, d_src = ctx.alloc(tgt.nbytes).upload(tgt), ctx.alloc(src.nbytes).upload(src)
    d_idx, d_d2, d_perm = ctx.alloc(n * 4), ctx.alloc(n * 4), ctx.alloc(n * 4)
    ix = icp.NNIndex(ctx, d_tgt.ptr, m)
    try:
        ix.query(d_src.ptr, n, d_idx.ptr, d_d2.ptr)
        i0, d0 = d_idx.download(np.uint32, n), d_d2.download(np.float32, n)
        np.testing.assert_array_equal(i0, oi)
        np.testing.assert_allclose(d0, od, rtol=2e-7)
        ix.sort_cloud(d_src.ptr, n, d_perm.ptr)
        perm = d_perm.download(np.uint32, n)
        moved = d_src.download(np.float32, n * 3).reshape(n, 3)
        assert sorted(perm.tolist()) == list(range(n))
        np.testing.assert_array_equal(moved, src[perm])
        ix.query(d_src.ptr, n, d_idx.ptr, d_d2.ptr, presorted=True)
        i1, d1 = d_idx.download(np.uint32, n), d_d2.download(np.float32, n)
        np.testing.assert_array_equal(i1, oi[perm])
        np.testing.assert_array_equal(d1.view(np.uint32), d0[perm].view(np.uint32))
    finally:
        ix.close()
        for b in (d_tgt, d_src, d_idx, d_d2, d_perm):
            b.free()
    return _cat(i0, d0, perm, moved, i1, d1)


def icp_pair(scale=1):
    from oracle import icp_ref as OI
    return OI.synthetic_pair(n_tgt=_n(4000, scale), n_src=_n(3000, scale), s=1.01, angle_deg=0.5, t_norm=0.02, noise=0.005, seed=5)[:2]


def icp_loop_reference(ctx, src, tgt, iters=4):
    """the host-stepped loop test_gpu_icp_state.py holds the device loop to (1e-9 on T_total); once per cloud size"""
    if src.shape[0] in _ICP_REF:
        return _ICP_REF[src.shape[0]]
    _ICP_REF[src.shape[0]] = T = _icp_loop_reference(ctx, src, tgt, iters)
    return T


_ICP_REF, _PLANE = {}, {}


def _icp_loop_reference(ctx, src, tgt, iters):
    icp = _m("icp")
    b = icp.IcpDevice(src, tgt, ctx, True)
    T_total = np.eye(4)
    for _ in range(iters):
        b.nn()
        T = icp.umeyama_from_sums(b.sums(), with_scale=True)
        b.move_source(T)
        T_total = T @ T_total
    b.free()
    return T_total


def icp_loop(ctx, scale=1):
    icp = _m("icp")
    src, tgt = icp_pair(scale)
    dev = icp.IcpDevice(src, tgt, ctx, True)
    try:
        dev.state_reset()
        dev.iterate(4)
        st = dev.d_state.download(np.float64, 512)
        cloud = dev.source()
    finally:
        dev.free()
    assert st[32] == 4.0 and st[33] == 0.0
    np.testing.assert_allclose(st[:16].reshape(4, 4), icp_loop_reference(ctx, src, tgt), rtol=0, atol=1e-9)
    return _cat(st, cloud)


def plane_scene(scale=1):
    """(source rows, organised target, (h, w), rough start, the oracle loop's (T, rms history) over 4 iterations)"""
    if scale in _PLANE:
        return _PLANE[scale]
    from oracle import plane_ref as PR
    from test_gpu_plane_icp import rough, scene
    h, w = 48 * _side(scale), 64 * _side(scale)
    v, pa, pb = scene(_m("synthetic"), h, w, 15.0, (0.35, 0.05, -0.2), noise=0.002)
    T0 = rough(v["T_ab"])
    keep = np.any(pb != 0, axis=1)
    ref = PR.icp_point_to_plane(pb[keep], pa, PR.organized_normals(pa, h, w, 0.05), T0=T0, max_iter=4, trim_q=0.5, gate_scale=20.0, tol=0.0)
    _PLANE[scale] = pb[keep], pa, (h, w), T0, ref
    return _PLANE[scale]


def plane_icp_loop(ctx, scale=1):
    icp = _m("icp")
    src, tgt, shape, T0, (T_ref, hist) = plane_scene(scale)
    dev = icp.PlaneIcpDevice(src, tgt, shape, ctx=ctx)
    try:
        dev.move_source(T0)
        dev.state_reset()
        dev.iterate(4)                                              # trim_q = 0.5: the selection over the 24 direction classes
        st = dev.d_state.download(np.float64, 512)
        cloud = dev.d_src.download(np.float32, dev.n * 3)
    finally:
        dev.free()
    assert st[32] == 4.0
    for k in range(4):
        assert abs(st[48 + k] - hist[k]) <= 1e-6 * hist[0], (k, st[48 + k], hist[k])
    np.testing.assert_allclose(st[:16].reshape(4, 4) @ T0, T_ref, atol=2e-6)
    return _cat(st, cloud)


def select(ctx, scale=1):
    import icp_parts_ref as REF
    from oracle import plane_ref as PR
    from test_gpu_icp_parts import assert_trimmed, quantile_host, trimmed
    L = _m("_lib")
    v = REF.mixed_values(_n(5001, scale), 7)
    vt, _ = REF.trimmed_case(24, _n(257, scale), 1)
    dv, dt = ctx.alloc(v.nbytes).upload(v), ctx.alloc(vt.nbytes).upload(vt)
    out = []
    try:
        for q in (0.0, 0.5, 0.9, 1.0):
            val, cnt = quantile_host(ctx, L, dv.ptr, v.shape[0], q)
            want = PR.quantile_lower(v, q)
            assert cnt == want[1] and REF.same_selection([val], [want[0]])
            out += [np.float32(val), np.int64(cnt)]
        for keep in (0.5, 0.8):
            got = trimmed(ctx, L, dt.ptr, 24, vt.shape[0] // 24, keep)
            assert_trimmed(got, vt, 24, vt.shape[0] // 24, keep, "catalogue")
            out.append(got)
    finally:
        dv.free()
        dt.free()
    return _cat(*out)


def knn_sor_ror_select(ctx, scale=1):
    import outliers_ref as REF
    from test_gpu_outliers import _cube, assert_lists, device_knn
    R, O = _r3d(), _m("outliers")
    xyz = _cube(_n(3000, scale), 1)
    lists = REF.knn(xyz, 9)
    idx, d2 = device_knn(R, ctx, xyz, 9)
    assert_lists((idx, d2), lists, 9)
    got = O.remove_statistical_outlier(xyz, 9, 2.0, ctx=ctx)
    m, keep, (V, mu, sigma, T) = REF.sor(xyz, 9, 2.0, lists)
    assert np.array_equal(got.score.view(np.uint64), m.view(np.uint64)) and got.stats.V == V
    for a, b in ((got.stats.mu, mu), (got.stats.sigma, sigma), (got.stats.T, T)):
        assert abs(a - b) <= 1e-12 * max(abs(b), 1e-300), (a, b)
    mask = got.score <= got.stats.T
    assert np.array_equal(got.rows, np.flatnonzero(mask)) and np.array_equal(mask, keep)
    assert np.array_equal(got.xyz.view(np.uint32), xyz[mask].view(np.uint32))
    radius = 0.05 / (scale ** (1.0 / 3.0))
    ror = O.remove_radius_outlier(xyz, 2, radius, ctx=ctx)
    counts = REF.ror_counts(xyz, radius)
    assert np.array_equal(ror.count.astype(np.int64), np.minimum(counts, 2))
    assert np.array_equal(ror.rows, np.flatnonzero(counts >= 2))
    assert np.array_equal(ror.xyz.view(np.uint32), xyz[counts >= 2].view(np.uint32))
    return _cat(idx, d2, got.score, got.rows, got.xyz, ror.count, ror.rows, ror.xyz)


def normals_knn(ctx, scale=1):
    import normals_ref as REF
    from test_gpu_normals import _cube, bits, check_normals, device_run
    xyz = _cube(_n(2000, scale), 1)
    n = xyz.shape[0]
    views = np.array([[3.0, -2.0, 0.5], [-1.0, 0.5, 4.0]])
    got = device_run(ctx, xyz, 9, None, views=views, ppv=n // 2)
    want = REF.normals(xyz, got.idx, got.d2, None)
    assert np.array_equal(got.count, want.count)
    sure = ~want.line
    assert not ((bits(got.cov) != bits(want.cov)).any(axis=1) & sure).any()
    check_normals(got.normals, want, None, "catalogue")
    view_of = views[np.minimum(np.arange(n) // (n // 2), 1)]
    dot = (got.normals.astype(np.float64) * (view_of - xyz.astype(np.float64))).sum(axis=1)
    assert (dot[(got.normals != 0).any(axis=1)] >= 0).all()
    return _cat(got.idx, got.d2, got.normals, got.curvature, got.cov, got.count)


# ---- voxels, text, planes --------------------------------------------------------------------------------------------------------
def voxelset(ctx, scale=1):
    from oracle import octomap_ref as OM
    from test_gpu_octree_device import check_codes
    V, L = _m("voxelmap"), _m("_lib")
    rng = np.random.default_rng(105)
    pts = (rng.normal(size=(_n(20_000, scale), 3)) * 5).astype(np.float32)
    pts[11] = (np.nan, 0, 0)
    pts[13] = (5000.0, 0, 0)
    want, dropped = OM.occupied_set(pts)
    out = []
    try:
        for path in (1, 2):
            ctx.set_tuning("voxel_path", path)
            vs = V.VoxelSet(0.1, 1 << 17, ctx)
            try:
                vs.insert(pts)
                assert ctx.get_tuning("voxel_last_path") == path
                assert vs.stats() == {"voxels": len(want), "ignored_points": dropped, "overflow": 0}
                codes = vs.codes()
                np.testing.assert_array_equal(codes, want)
                bt, nodes = vs.format_bt()
                assert (bt, nodes) == V.format_bt(codes, 0.1)
                out += [codes, bt]
            finally:
                vs.close()
    finally:
        ctx.set_tuning("voxel_path", 0)
    out.append(check_codes(V, L, ctx, want)[0])
    return _cat(*out)


def voxelgrid(ctx, scale=1):
    from test_gpu_voxel_downsample import assert_matches, colours, run_grid, with_junk
    rng = np.random.default_rng(106)
    n = _n(20_000, scale)
    xyz = with_junk(rng, (rng.normal(size=(n, 3)) * 3).astype(np.float32), 0.2)
    rgba = colours(rng, n)
    got, stats = run_grid(_m("voxelmap"), ctx, xyz, 0.2, rgba)
    assert_matches(got, stats, xyz, 0.2, rgba)
    return _cat(got.codes, got.counts, got.xyz, got.rgba)


def textfmt(ctx, scale=1):
    from test_gpu_textfmt import device_text, first_difference, host_ply_rows
    R = _r3d()
    rng = np.random.default_rng(107)
    n = _n(1000, scale)
    xyz = (rng.normal(size=(n, 3)) * np.array([1e-3, 1.0, 1e5])).astype(np.float64)
    txt, offs = device_text(R, ctx, R.device_text.TEXT_XYZ_TXT, xyz, segment_points=256)
    want = R.cloud_io.format_xyz_txt(xyz)
    assert txt == want, first_difference(txt, want)
    assert len(offs) == (n + 255) // 256 + 1 and offs[0] == 0 and offs[-1] == len(want)
    rows, _ = device_text(R, ctx, R.device_text.TEXT_PLY_ROWS, xyz, segment_points=256)
    assert rows == host_ply_rows(R, xyz), first_difference(rows, host_ply_rows(R, xyz))
    return _cat(txt, np.asarray(offs, np.int64), rows)


def segment_plane(ctx, scale=1):
    import segment_ref as REF
    from test_gpu_segment import check_all
    xyz = REF.cube(_n(2000, scale), 1)
    p, mask, _ = check_all(_m("segmentation"), ctx, xyz, 0.02, 512, 0)
    return _cat(p.plane, p.centroid, np.int64([p.best_hypothesis, p.best_count, p.n_valid, p.n_inliers]), p.best_rows, mask)


# ---- the TSDF volume ------------------------------------------------------------------------------------------------------------
def _dims(scale):
    return (65, 33, 17) if scale > 1 else (33, 17, 9)


def _hw(scale):
    return (24 * _side(scale), 32 * _side(scale))


def tsdf(ctx, scale=1):
    import mesh_ref as MREF
    import raycast_ref as RC
    import tsdf_ref as REF
    from test_gpu_mesh import assert_mesh
    from test_gpu_raycast import assert_maps, cast, poses_around, raster_K
    from test_gpu_tsdf import assert_points, assert_volume, device_volume
    T = _m("tsdf")
    s = REF.random_scene(_dims(scale), 9, np.float32, _hw(scale), seed=86)
    ref = REF.run(s)[0]
    V = device_volume(T, ctx, s)
    try:
        _integrate_host(ctx, V, s)
        assert_volume(V, ref)
        assert_points(V, ref)
        pts = V.extract_point_cloud(1.0)
        mesh = V.extract_triangle_mesh(1.0)
        assert_mesh(mesh, MREF.extract_mesh(ref, 1.0))
        shape = _hw(scale)
        K, poses = raster_K(shape), poses_around(ref, 3, 86)
        maps = cast(ctx, V, poses, K, shape, step=float(ref.vs) * 0.5)
        assert_maps(maps, RC.raycast(ref, poses, K, shape, step=float(ref.vs) * 0.5))
        tsdf_w = V.volume()
    finally:
        V.close()
    return _cat(*tsdf_w, *pts, *mesh, *maps)


def _integrate_host(ctx, V, s, rgb=None):
    """the scene's frames from host memory (r3d_tsdf_integrate_host / _rgb_host) with its pose rows as they are"""
    dev, L = _m("device"), _m("_lib")
    d = np.ascontiguousarray(s["depths"])
    f, h, w = d.shape
    cam = ctx.camera(h, w, *s["K"])
    table = np.ascontiguousarray(s["poses"], np.float64).reshape(f, 12)
    if rgb is None:
        L.check(ctx.lib.r3d_tsdf_integrate_host(V.handle, cam.handle, d.ctypes.data, dev.depth_code(d.dtype), f, float(s["scale"]),
                                                table.ctypes.data))
    else:
        rgb = np.ascontiguousarray(rgb, np.uint8)
        L.check(ctx.lib.r3d_tsdf_integrate_rgb_host(V.handle, cam.handle, d.ctypes.data, dev.depth_code(d.dtype), f, float(s["scale"]),
                                                    table.ctypes.data, rgb.ctypes.data))


def tsdf_rgb(ctx, scale=1):
    import raycast_color_ref as RCC
    from test_gpu_raycast import poses_around, raster_K
    from test_gpu_raycast_color import assert_same, cast
    from test_gpu_tsdf_color import assert_colors, assert_planes, color_volume, scene
    T, L = _m("tsdf"), _m("_lib")
    s, rgb, ref, passed = scene(_dims(scale), 9, np.uint8, hw=_hw(scale), seed=11)
    assert passed > 0
    V = color_volume(T, ctx, s)
    try:
        _integrate_host(ctx, V, s, rgb)
        assert_planes(V, ref)
        assert_colors(V, ref)
        cloud = V.extract_point_cloud(1.0, with_colors=True)
        shape = _hw(scale)
        K, poses = raster_K(shape), poses_around(ref, 2, 11)
        maps = cast(L, ctx, V, poses, K, shape, step=float(ref.vs) * 0.5)
        assert_same(maps, RCC.raycast(ref, poses, K, shape, step=float(ref.vs) * 0.5))
        planes = V.volume() + V.colors()
    finally:
        V.close()
    return _cat(*planes, *cloud, *[m for m in maps if m is not None])


_TRACK = {}


def track_scene(scale=1):
    """eight room views and a frame 2 degrees / 0.05 m from view 2 (the setup of test_gpu_track.py at 48 x 64, 0.1 m voxels)"""
    if scale not in _TRACK:
        import track_ref as TR
        R, syn = _r3d(), _m("synthetic")
        H, W, n_frames, i = 48 * _side(scale), 64 * _side(scale), 8, 2
        depths, quats, ts, K = syn.room_views(n_frames, H, W, seed=0)
        poses = R.poses_w2c(quats, ts)
        T_i = TR.pose_matrix(poses[i])
        c_i = -T_i[:3, :3].T @ T_i[:3, 3]
        z, _q, _t, _ = syn.room_view(H, W, 2 * np.pi * i / n_frames + 0.1 + np.radians(2.0), c_i + np.array([0.03, 0.0, 0.04]))
        rgbs = np.random.default_rng(108).integers(0, 256, size=depths.shape + (3,), dtype=np.uint8)
        _TRACK[scale] = dict(H=H, W=W, K=K, depths=depths, quats=quats, ts=ts, guess=poses[i].copy(), quat=quats[i:i + 1], t=ts[i:i + 1],
                             frame=z.astype(np.float32), rgbs=rgbs, rgb_new=rgbs[i])
    return _TRACK[scale]


def _room_volume(ctx, s, color=False):
    from test_gpu_track import room_volume
    V = room_volume(_r3d(), ctx, 0.1, 0.3, color=color)
    if color:
        V.integrate(s["depths"], s["quats"], s["ts"], intrinsics=s["K"], rgb=s["rgbs"])
    else:
        V.integrate(s["depths"], s["quats"], s["ts"], intrinsics=s["K"])
    return V


def _info_bytes(info):
    return _cat(*[np.float64(info[k]) for k in sorted(info) if np.ndim(info[k]) == 0 or isinstance(info[k], list)])


def track(ctx, scale=1):
    import track_ref as TR
    R, s = _r3d(), track_scene(scale)
    V = _room_volume(ctx, s)
    try:
        row, info = V.track(s["frame"], s["guess"], intrinsics=s["K"])
        assert info["status"] == 0 and info["iterations"] == 10
        _, vertex, normal = V.raycast(s["quat"], s["t"], (s["H"], s["W"]), intrinsics=s["K"])
        sv = R.unproject(s["frame"], intrinsics=s["K"], ctx=ctx).reshape(s["H"], s["W"], 3)
        want, winfo = TR.track(sv, None, vertex[0], normal[0], s["guess"], s["K"], 2 * 0.3, -1.0, 10)
        assert winfo["status"] == 0
        np.testing.assert_allclose(row, want, atol=2e-6, rtol=0)
    finally:
        V.close()
    return _cat(row, _info_bytes(info), vertex, normal)


def track_pyramid_rgb(ctx, scale=1):
    import photo_ref as PH
    import pyramid_ref as PR
    from test_gpu_track_pyramid import device_levels
    R, tracking, s = _r3d(), _m("tracking"), track_scene(scale)
    V = _room_volume(ctx, s, color=True)
    try:
        iters = (4, 3, 3)
        row, info = V.track(s["frame"], s["guess"], intrinsics=s["K"], pyramid_iters=iters)
        assert info["status"] == 0 and info["iterations"] == 10
        sv = R.unproject(s["frame"], intrinsics=s["K"], ctx=ctx).reshape(s["H"], s["W"], 3)
        levels = device_levels(R, V, s, sv, 3, 0.05)
        want, winfo = PR.track(levels, iters, s["guess"], 2 * 0.3, -1.0)
        assert winfo["status"] == 0 and winfo["margin"] >= 1e-9, winfo["margin"]
        np.testing.assert_allclose(row, want, atol=2e-6, rtol=0)
        np.testing.assert_allclose(info["rms_history"], winfo["rms_history"], atol=2e-6, rtol=0)
        # the photometric term on the finest level alone
        row_c, info_c = V.track(s["frame"], s["guess"], intrinsics=s["K"], rgb=s["rgb_new"])
        assert info_c["status"] == 0 and info_c["photo_pairs"] > 0
        depth, vertex, normal, rgb = V.raycast(s["quat"], s["t"], (s["H"], s["W"]), intrinsics=s["K"], with_colors=True)
        Is, _ = PH.intensity_map(s["rgb_new"], sv[..., 2], 0.05)
        _, packed = PH.intensity_map(rgb[0], depth[0], 0.05)
        want_c, winfo_c = PH.track(sv, None, vertex[0], normal[0], s["guess"], s["K"], 2 * 0.3, -1.0, 10, Is, packed, tracking.PHOTO_WEIGHT,
                                   tracking.I_MAX)
        assert winfo_c["status"] == 0 and winfo_c["photo_pairs"] == info_c["photo_pairs"] and winfo_c["pairs"] == info_c["pairs"]
        np.testing.assert_allclose(row_c, want_c, atol=2e-6, rtol=0)
        assert abs(info_c["photo_rms"] - winfo_c["photo_rms"]) <= 1e-6
    finally:
        V.close()
    return _cat(row, _info_bytes(info), row_c, _info_bytes(info_c))


def bilateral(ctx, scale=1):
    import bilateral_ref as BR
    from test_gpu_bilateral import bits, dirty_depth
    tracking = _m("tracking")
    h, w = 17 * _side(scale) * _side(scale), 65 * _side(scale)
    d = dirty_depth(h, w, 1)
    out = []
    for radius, (ss, sr) in ((2, (1.5, 0.3)), (4, (2.5, 0.5)), (2, (1.5, 0.3))):
        got = tracking.depth_bilateral(d, radius, ss, sr, ctx=ctx)
        want = BR.depth_bilateral(d, radius, *tracking.bilateral_weights(radius, ss, sr))
        assert np.array_equal(bits(got), bits(want)), radius
        out.append(got)
    assert out[0].tobytes() == out[2].tobytes()
    return _cat(*out)


def project_grad(ctx, scale=1):
    import ctypes as C
    import project_ref as PR
    from test_gpu_torch_ops import _bits, _check_grad_P
    L = _m("_lib")
    shape = B, H, W = 2, 24 * _side(scale) * _side(scale), 80 * _side(scale)
    inp = PR.dense_inputs(*shape)
    hw = H * W
    d = {k: ctx.alloc(inp[k].nbytes).upload(inp[k]) for k in ("points", "P", "gpix")}
    gpts, gP = ctx.alloc(B * 4 * hw * 4), ctx.alloc(B * 48)
    try:
        L.check(ctx.lib.r3d_project3d_grad_f32(ctx.handle, d["gpix"].ptr, d["points"].ptr, d["P"].ptr, B, H, W, C.c_float(PR.EPS), gpts.ptr,
                                               gP.ptr))
        g_points, g_P = gpts.download(np.float32, B * 4 * hw).reshape(B, 4, hw), gP.download(np.float32, B * 12).reshape(B, 3, 4)
    finally:
        for b in list(d.values()) + [gpts, gP]:
            b.free()
    _bits(g_points, PR.grad_points_f32(inp["gpix"], inp["points"], inp["P"], H, W), "grad_points")
    _check_grad_P(inp, shape, g_P)
    return _cat(g_points, g_P)


# ---- global registration ---------------------------------------------------------------------------------------------------------
def fpfh(ctx, scale=1):
    import register_ref as REF
    from test_gpu_fpfh import check
    n = _n(2000, scale)
    f, s, c = check(_r3d(), _m("registration"), ctx, REF.cube(n, 1), REF.unit_normals(n, 2), 8, 0.1)
    return _cat(f, s, c)


def feature_match(ctx, scale=1):
    import register_ref as REF
    from test_gpu_feature_match import device_run, features
    fa, fb = features("ties", _n(1000, scale), 257 * scale, 0)
    want, wi, wd = REF.match(fa, fb, mutual=True)
    idx, dist, corr = device_run(_m("registration"), ctx, fa, fb, True)
    assert np.array_equal(idx, wi) and np.array_equal(dist.view(np.uint32), wd.view(np.uint32)) and np.array_equal(corr, want)
    return _cat(idx, dist, corr)


def register_ransac(ctx, scale=1):
    import register_ref as REF
    from test_gpu_register import check_all
    src, tgt, corr, _ = REF.correspondences("outliers", _n(1025, scale), 3)
    r, mask, _ = check_all(_m("registration"), ctx, src, tgt, corr, 0.02, 513, 1)
    return _cat(r, mask)


# ---- the entry points with workspaces of their own --------------------------------------------------------------------------------
def registration_sums(ctx, scale=1):
    """r3d_registration_sums on the pairs an index query returns (the setup of test_gpu_posegraph.py, its bound)"""
    import posegraph_ref as REF
    from test_gpu_posegraph import N_TGT, check, sums_call
    icp, L = _m("icp"), _m("_lib")
    n = _n(1000, scale)
    rng = np.random.default_rng(0)
    tgt = (rng.uniform(-2.0, 2.0, (N_TGT, 3)) + (0.5, -1.0, 3.0)).astype(np.float32)
    rng = np.random.default_rng(n)
    src = (tgt[rng.integers(8, 4000, n)].astype(np.float64) + rng.normal(size=(n, 3)) * 0.02).astype(np.float32)
    d_tgt, d_src, d_idx, d_d2 = ctx.alloc(tgt.nbytes).upload(tgt), ctx.alloc(src.nbytes).upload(src), ctx.alloc(n * 4), ctx.alloc(n * 4)
    ix = icp.NNIndex(ctx, d_tgt.ptr, N_TGT)
    try:
        ix.query(d_src.ptr, n, d_idx.ptr, d_d2.ptr)
        idx, d2 = d_idx.download(np.uint32, n), d_d2.download(np.float32, n)
        out = []
        for gate in (np.inf, float(np.sort(d2)[n // 2])):
            rc, got = sums_call(ctx, d_src.ptr, n, d_tgt.ptr, N_TGT, d_idx.ptr, d_d2.ptr, gate)
            assert rc == 0, L.last_error()
            want = check(got, src, tgt, idx, d2, gate)
            assert want[0] == (d2 <= gate).sum()
            out.append(got)
    finally:
        ix.close()
        for b in (d_tgt, d_src, d_idx, d_d2):
            b.free()
    return _cat(idx, d2, *out)


_WALL = {}


def _wall():
    """the colour wall of test_gpu_color_icp.py with the restatement's intensities and gradients (its `wall` fixture)"""
    if not _WALL:
        import color_icp_ref as REF
        sc = REF.wall_scene()
        idx, d2 = REF.knn_lists(sc["tgt"], 8)
        sc["I"], sc["grad"], _ = REF.gradients(sc["tgt"], sc["normals"], sc["tgt_rgba"], idx, d2)
        sc["src_I"] = REF.intensity(sc["src_rgba"])
        _WALL.update(sc)
    return _WALL


def color_icp(ctx, scale=1):
    """the wall's gradients, one 31-sums pass and a two-iteration loop on 257 of its sources"""
    import color_icp_ref as REF
    from test_gpu_bounds import Guarded
    from test_gpu_color_icp import ColourLoop, assert_sums, clouds, device_pass, nan_bits, pass_inputs
    icp, L, CI = _m("icp"), _m("_lib"), _m("colored_icp")
    wall, w = _wall(), _m("colored_icp").photo_weight(0.968)
    made = []

    def guard(nbytes, off=0, data=None, seed=0):
        made.append(Guarded(ctx, nbytes, off, data, seed))
        return made[-1]

    loop = None
    xyz, nrm, rgba, radius = clouds()["wall"]
    k, rad = (32, radius) if scale > 1 else (8, None)
    m = xyz.shape[0]
    bufs = [ctx.alloc(a.nbytes).upload(np.ascontiguousarray(a)) for a in (xyz, nrm, rgba)] + [ctx.alloc(m * 4), ctx.alloc(m * 12), ctx.alloc(m * 4)]
    ix = icp.NNIndex(ctx, bufs[0].ptr, m)
    try:
        L.check(ctx.lib.r3d_color_gradient_knn(ix.handle, k, 0.0 if rad is None else rad, bufs[1].ptr, bufs[2].ptr, bufs[3].ptr, bufs[4].ptr,
                                               bufs[5].ptr))
        got_I, got_g, got_c = bufs[3].download(np.float32, m), bufs[4].download(np.float32, m * 3).reshape(m, 3), bufs[5].download(np.uint32, m)
    finally:
        ix.close()
        for b in bufs:
            b.free()
    try:
        want_I, want_g, want_c = REF.gradients(xyz, nrm, rgba, *REF.knn_lists(xyz, k), radius=rad)
        assert np.array_equal(got_c, want_c) and np.array_equal(got_I.view(np.uint32), want_I.view(np.uint32))
        assert np.array_equal(nan_bits(got_g), nan_bits(want_g))
        n = _n(257, scale)
        src, src_I, pn, idx, d2 = pass_inputs(wall, n, 40 + n)
        want = REF.accumulate(src, src_I, wall["tgt"], pn, wall["I"], wall["grad"], idx, d2, float(REF.WALL_MAX_D2), w, 6.0)
        sums, photo, _ = device_pass(ctx, L, guard, wall, src, src_I, pn, idx, d2, float(REF.WALL_MAX_D2), w, 6.0)
        assert_sums(sums, want.sums)
        assert np.array_equal(nan_bits(photo), nan_bits(want.photo))
        rows = np.linspace(0, wall["src"].shape[0] - 1, n).astype(np.int64)
        lsrc, lsrc_I = np.ascontiguousarray(wall["src"][rows]), np.ascontiguousarray(wall["src_I"][rows])
        ln = wall["normals"].copy()
        ln[::7] = 0
        st_want, last = REF.loop(lsrc, lsrc_I, wall["tgt"], ln, wall["I"], wall["grad"], 2, -1.0, w, 40.0)
        loop = ColourLoop(ctx, L, CI, wall, lsrc, lsrc_I, ln, True)
        st = loop.iterate(2, w, 40.0)
        lsums, cloud = loop.d_sums.download(np.float64, 31), loop.d_src.download(np.float32, n * 3)
        assert st[32] == 2.0 and st[33] == 0.0 and lsums[0] == last.sums[0] and lsums[29] == last.sums[29]
        np.testing.assert_allclose(st[:16].reshape(4, 4), st_want[:16].reshape(4, 4), atol=2e-6, rtol=0)
    finally:
        if loop is not None:
            loop.c.close()
        for g in made:
            g.free()
    return _cat(got_I, got_g, got_c, sums, photo, st, lsums, cloud)


def mesh_components(ctx, scale=1):
    """label and filter a marching-cubes mesh with floaters and one triangle that names no vertex"""
    import mesh_cc_ref as CC
    from test_gpu_mesh_cc import assert_components, components, filtered
    from test_mesh_cc_host import volume_mesh
    L = _m("_lib")
    xyz, _, tri = volume_mesh(((16, 16, 17), 86, 0.0) if scale > 1 else ((40, 9, 5), 3, 0.2))
    nv = len(xyz)
    tri = np.concatenate([tri[:len(tri) // 2], np.array([[-1, 0, 1]], np.int32), tri[len(tri) // 2:]])
    want = CC.components(tri, nv)
    assert want[3] == 1 and len(want[2]) > 1
    got = components(ctx, L, tri, nv, seed=1)
    assert_components(got, want)
    out = [got[0], got[1], got[2]]
    for mt, largest in ((2, False), (1, True)):
        kept, kept_tri, n, m = filtered(ctx, L, tri, nv, got[0], mt, largest, seed=mt)
        want_kept, want_tri = CC.filter_components(tri, nv, got[0], mt, largest)
        assert (n, m) == (len(want_kept), len(want_tri)) and np.array_equal(kept, want_kept) and np.array_equal(kept_tri, want_tri)
        out += [kept, kept_tri]
    return _cat(*out)


def mesh_distance(ctx, scale=1):
    """index build, point-to-mesh query and the statistics of its distances"""
    import compare_ref as CR
    from test_gpu_compare import assert_stats, query, same_floats, sized_case, stats
    L = _m("_lib")
    pts, v, tri, want = sized_case(3000 if scale > 1 else 300)
    got = query(ctx, L, pts, v, tri)
    assert same_floats(got[0], want[0]) and np.array_equal(got[1], want[1]) and same_floats(got[2], want[2])
    thr = (0.5, 1.0, -1.0)
    st = stats(ctx, L, got[0], thr, 0.25, 16)
    assert_stats(st, CR.distance_stats(got[0], thr, 0.25, 16))
    return _cat(got[0], got[1], got[2], *st)


def _with_memo(f):
    def run(ctx, scale=1):
        _memo_all()
        return f(ctx, scale)
    run.__name__ = f.__name__
    return run


CASES = {f.__name__: _with_memo(f) for f in (
    fuse_host, fuse_rgb_host, apply_host, sort, nn_build_query, icp_loop, plane_icp_loop, select, knn_sor_ror_select, normals_knn, voxelset,
    voxelgrid, textfmt, segment_plane, tsdf, tsdf_rgb, track, track_pyramid_rgb, bilateral, project_grad, fpfh, feature_match,
    register_ransac, registration_sums, color_icp, mesh_components, mesh_distance)}

_NN = ["r3d_nnindex.hip", "r3d_sort.hip"]
_TSDF = ["r3d_tsdf.hip", "r3d_tsdf_raycast.hip"]
COVERS = {
    "fuse_host": ["r3d_fuse.hip", "r3d_hostpipe.hip"],
    "fuse_rgb_host": ["r3d_fuse.hip", "r3d_hostpipe.hip"],
    "apply_host": ["r3d_apply.hip"],
    "sort": ["r3d_sort.hip", "r3d_ctx.hip"],
    "nn_build_query": _NN,
    "icp_loop": _NN + ["r3d_icp.hip", "r3d_apply.hip"],
    "plane_icp_loop": _NN + ["r3d_plane.hip", "r3d_icp.hip", "r3d_apply.hip"],
    "select": ["r3d_plane.hip"],
    "knn_sor_ror_select": _NN + ["r3d_knn.hip"],
    "normals_knn": _NN + ["r3d_knn.hip"],
    "voxelset": ["r3d_voxel.hip", "r3d_voxel_merge.hip", "r3d_octree.hip", "r3d_sort.hip"],
    "voxelgrid": ["r3d_voxelgrid.hip", "r3d_sort.hip"],
    "textfmt": ["r3d_textfmt.hip"],
    "segment_plane": ["r3d_ransac.hip"],
    "tsdf": _TSDF + ["r3d_tsdf_mesh.hip"],
    "tsdf_rgb": _TSDF + ["r3d_tsdf_color.hip"],
    "track": _TSDF + ["r3d_track.hip", "r3d_backproject.hip"],
    "track_pyramid_rgb": _TSDF + ["r3d_track.hip", "r3d_pyramid.hip", "r3d_photo.hip"],
    "bilateral": ["r3d_bilateral.hip"],
    "project_grad": ["r3d_backproject.hip"],
    "fpfh": _NN + ["r3d_knn.hip", "r3d_fpfh.hip"],
    "feature_match": ["r3d_fpfh.hip", "r3d_register.hip"],
    "register_ransac": ["r3d_register.hip"],
    "registration_sums": _NN + ["r3d_reginfo.hip"],
    "color_icp": _NN + ["r3d_knn.hip", "r3d_color_icp.hip", "r3d_icp.hip", "r3d_plane.hip", "r3d_apply.hip"],
    "mesh_components": ["r3d_mesh_cc.hip"],
    "mesh_distance": ["r3d_meshdist.hip", "r3d_sort.hip"],
    "not_covered_multi_device": ["r3d_comm.hip"],
}
