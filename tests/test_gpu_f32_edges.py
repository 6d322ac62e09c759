"""GPU: the f32 kernels where values go subnormal, overflow or hit -0, BIT FOR BIT against the restatements, on the cases of
tests/f32_edge_cases.py (tests/test_f32_edges_host.py proves of the restatements alone that every case bites: its expected bits are
not what flush-to-zero arithmetic gives).  include/r3d.h promises IEEE f32 chains with "f32 denormals kept"; the rest of the suite
keeps its inputs away from subnormals on purpose, so a flush-to-zero or fast-math flag on one object, a reciprocal-based division,
a conversion or a v_med3 that drops subnormals would pass it.

  1  r3d_icp_nn, r3d_nn_index_query (cold and warm, nn_variant 1 / 2 / 4), r3d_nn_index_knn_self (k = 1, 8, 32): integer lattices
     times 2^-70 (every d2 subnormal and exact), 2^64 (every non-zero d2 overflows) and 2^60 (finite near the top)
  2  r3d_tsdf_integrate / _host and the extraction after it, every length of the scene times 2^-127
  3  r3d_tsdf_extract_points, _extract_mesh, r3d_tsdf_raycast and (geometry) _raycast_rgb from uploaded volumes of subnormals, signed
     zeros, +-2^-126, +-FLT_MAX / 2 and +-0.75 FLT_MAX
  4  r3d_depth_half and r3d_depth_bilateral; the filter's subnormal weights are entries of the SPATIAL table (the range table is
     exp(-t^2 / 2), t < 3, whatever sigma_r: it has no entry below 0.011)
  5  the four per-pixel torch-facing projection kernels
  6  r3d_apply_T, r3d_se3_apply, r3d_unproject, f32 in and f32 out: the f32 -> f64 conversion of subnormals, results in the
     subnormal range, exact ties, the tie that rounds up to 2^-126, overflow to inf

A NaN's sign and payload belong to the unit that made it (inf - inf is 0xffc00000 on x86, 0x7fc00000 on the device): where the
restatement has a NaN the device must have one, and every other word is compared exactly (f32_edge_cases.same_bits, the rule of
project_ref.eq_bits).  The missing-row word of the ray-cast maps is compared exactly.

Left out: colour sums (uint32 / weight), the intensity map (0 .. 255 times fixed coefficients), the twelve grad_P sums (an order
that is not specified) and the fp64 tracking and ICP sums cannot produce f32 subnormals from valid inputs."""
import ctypes as C
import importlib

import numpy as np
import pytest

import f32_edge_cases as E
import tsdf_color_ref as CREF
from helpers import PKG, r3d as _r3d
from test_gpu_bounds import Guarded

pytestmark = pytest.mark.gpu

F = np.float32


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
def icp(R):
    return importlib.import_module(PKG + ".icp")


@pytest.fixture(scope="module")
def ctx(R):
    c = R.Context(0)
    yield c
    c.close()


@pytest.fixture
def guard(ctx):
    made = []

    def make(nbytes, off=0, data=None, seed=0):
        g = Guarded(ctx, nbytes, off, data, seed)
        made.append(g)
        return g
    yield make
    for g in made:
        g.free()


def assert_bits(got, want, what):
    assert E.same_bits(got, want), "%s: (mismatches, first index, got, want, got bits, want bits) = %s" % (what, E.first_mismatch(got, want))


def assert_nn(got, case, what):
    idx, d2 = got
    bad = np.flatnonzero((idx != case["idx"]) | (E.bits(d2) != E.bits(case["d2"])))
    assert bad.size == 0, "%s: %d rows differ, first %d: got (%d, %r) want (%d, %r)" % (
        what, bad.size, bad[0], idx[bad[0]], d2[bad[0]], case["idx"][bad[0]], case["d2"][bad[0]])


# ---- case 1 ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(E.NN_SCALES))
def test_nn_brute_force(icp, ctx, L, guard, name):
    c = E.nn_case(name)
    n, m = E.NN_SHAPE
    assert_nn(icp.nearest_neighbours(c["src"], c["tgt"], ctx=ctx, culled=False), c, "r3d_icp_nn_host")
    s, t = guard(n * 12, 0, c["src"], seed=1), guard(m * 12, 4, c["tgt"], seed=2)
    for S in (1, 2, 4):
        gi, gd = guard(n * 4, 4, seed=3 + S), guard(n * 4, 0, seed=8 + S)
        ctx.set_tuning("nn_variant", S)
        try:
            L.check(ctx.lib.r3d_icp_nn(ctx.handle, s.ptr, n, t.ptr, m, gi.ptr, gd.ptr))
            got = gi.read(np.uint32), gd.read(F)
        finally:
            ctx.set_tuning("nn_variant", 0)
        assert_nn(got, c, "r3d_icp_nn, nn_variant %d" % S)


@pytest.mark.parametrize("S", [1, 2, 4])
@pytest.mark.parametrize("name", list(E.NN_SCALES))
def test_nn_index_cold_and_warm(icp, ctx, name, S):
    """the culled index at extents of 2^-64 and 2^70: the brute-force answer, on the first (cold) query and on the repeated (warm) one,
    which starts from the first one's matches as bounds"""
    c = E.nn_case(name)
    ctx.set_tuning("nn_variant", S)
    dev = icp.IcpDevice(c["src"], c["tgt"], ctx, culled=True)
    try:
        dev.nn()
        assert_nn(dev.download(), c, "cold query")
        dev.nn()
        assert_nn(dev.download(), c, "warm query")
        ctx.set_tuning("nn_warm", 1)
        dev.nn()
        assert_nn(dev.download(), c, "query with nn_warm off")
    finally:
        ctx.set_tuning("nn_warm", 0)
        ctx.set_tuning("nn_variant", 0)
        dev.free()


@pytest.mark.parametrize("name", list(E.NN_SCALES))
def test_nn_index_unsorted_query(icp, ctx, guard, name):
    """presorted = 0: the query sorts a copy of the sources into the index's quantisation frame itself"""
    c = E.nn_case(name)
    n, m = E.NN_SHAPE
    s, t = guard(n * 12, 0, c["src"], seed=1), guard(m * 12, 0, c["tgt"], seed=2)
    gi, gd = guard(n * 4, 0, seed=3), guard(n * 4, 4, seed=4)
    ix = icp.NNIndex(ctx, t.ptr, m)
    try:
        ix.query(s.ptr, n, gi.ptr, gd.ptr, presorted=False)
        assert_nn((gi.read(np.uint32), gd.read(F)), c, "unsorted query")
        s.unchanged()
    finally:
        ix.close()


@pytest.mark.parametrize("k", E.KNN_KS)
@pytest.mark.parametrize("name", list(E.NN_SCALES))
def test_knn_self(icp, ctx, guard, name, k):
    c = E.knn_case(name, k)
    n = len(c["xyz"])
    x = guard(n * 12, 0, c["xyz"], seed=1)
    gi, gd = guard(n * k * 4, 4, seed=2), guard(n * k * 4, 4, seed=3)
    ix = icp.NNIndex(ctx, x.ptr, n)
    try:
        ix.knn_self(k, gi.ptr, gd.ptr)
        idx, d2 = gi.read(np.uint32, (n, k)), gd.read(F, (n, k))
    finally:
        ix.close()
    bad = np.flatnonzero((idx != c["idx"]).any(1) | (E.bits(d2) != E.bits(c["d2"])).any(1))
    assert bad.size == 0, "%d rows differ, first %d: got %s %s want %s %s" % (bad.size, bad[0], idx[bad[0]], d2[bad[0]], c["idx"][bad[0]],
                                                                               c["d2"][bad[0]])


# ---- case 2 ---------------------------------------------------------------------------------------------------------------------
def _assert_volume(V, ref, what):
    tsdf, w = V.volume()
    assert tsdf.shape == ref.tsdf.shape and np.array_equal(w, ref.w), what
    assert_bits(tsdf, ref.tsdf, what + ": tsdf")


@pytest.mark.parametrize("dims,dtype", E.TSDF_CASES, ids=lambda v: "x".join(map(str, v)) if isinstance(v, tuple) else v.__name__)
def test_tsdf_at_2_to_the_minus_127(T, L, ctx, dims, dtype):
    c = E.tsdf_case(dims, dtype)
    s, ref = c["scene"], c["ref"]
    assert c["passed"] > 0 and len(c["xyz"]) > 0
    depths, poses = s["depths"], np.ascontiguousarray(s["poses"])
    f, h, w = depths.shape
    cam = ctx.camera(h, w, *s["K"])
    V = T.TSDFVolume(s["origin"], s["vs"], s["dims"], s["tr"], ctx=ctx)
    H = T.TSDFVolume(s["origin"], s["vs"], s["dims"], s["tr"], ctx=ctx)
    buf = ctx.alloc(depths.nbytes).upload(depths)
    try:
        V.integrate_device(cam, buf.ptr, depths.dtype, f, poses, s["scale"])
        ctx.sync()
        _assert_volume(V, ref, "r3d_tsdf_integrate")
        code = L.DEPTH_U16 if np.dtype(dtype) == np.uint16 else L.DEPTH_F32
        L.check(ctx.lib.r3d_tsdf_integrate_host(H.handle, cam.handle, depths.ctypes.data, code, f, s["scale"], poses.ctypes.data))
        _assert_volume(H, ref, "r3d_tsdf_integrate_host")
        xyz, nrm = V.extract_point_cloud(1.0)
        assert xyz.shape == c["xyz"].shape, (xyz.shape, c["xyz"].shape)
        assert_bits(xyz, c["xyz"], "positions")
        assert_bits(nrm, c["nrm"], "normals")
    finally:
        buf.free()
        V.close()
        H.close()


# ---- case 3 ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dims", E.VOLUME_DIMS, ids=lambda d: "x".join(map(str, d)))
def test_extraction_and_mesh_of_uploaded_edge_volumes(T, ctx, dims):
    from test_gpu_mesh import uploaded
    c = E.volume_case(dims)
    V = uploaded(T, ctx, c["vol"])
    try:
        xyz, nrm = V.extract_point_cloud(1.0)
        assert xyz.shape == c["xyz"].shape, (xyz.shape, c["xyz"].shape)             # the count: signed zeros and subnormals cross
        assert_bits(xyz, c["xyz"], "points: positions")
        assert_bits(nrm, c["nrm"], "points: normals")
        mx, mn, tri = V.extract_triangle_mesh(1.0)
        assert mx.shape == c["xyz"].shape and tri.shape == c["tri"].shape, (mx.shape, tri.shape, c["tri"].shape)
        assert_bits(mx, c["xyz"], "mesh: positions")
        assert_bits(mn, c["nrm"], "mesh: normals")
        assert tri.dtype == np.int32 and np.array_equal(tri, c["tri"])
    finally:
        V.close()


def _assert_maps(got, want, what):
    for g, w, name in zip(got, want, ("depth", "vertex", "normal")):
        assert g.shape == w.shape, (what, name, g.shape, w.shape)
        assert_bits(g, w, "%s: %s" % (what, name))
        none = E.bits(w) == 0x7FC00000
        assert np.array_equal(E.bits(g)[none], E.bits(w)[none]), (what, name, "the missing-row word")


@pytest.mark.parametrize("dims", E.VOLUME_DIMS, ids=lambda d: "x".join(map(str, d)))
def test_raycast_of_uploaded_edge_volumes(T, L, ctx, dims):
    import test_gpu_raycast as TR
    import test_gpu_raycast_color as TRC
    c = E.raycast_case(dims)
    vol = c["vol"]
    V = TR.uploaded(T, ctx, vol)
    try:
        _assert_maps(TR.cast(ctx, V, c["poses"], c["K"], c["shape"], seed=1, step=c["step"]), c["want"], "r3d_tsdf_raycast")
    finally:
        V.close()
    cv = CREF.ColorVolume(vol.o.astype(np.float64), float(vol.vs), dims, float(vol.tr))
    cv.tsdf, cv.w = vol.tsdf, vol.w
    V = TRC.uploaded(T, ctx, cv)
    try:
        got = TRC.cast(L, ctx, V, c["poses"], c["K"], c["shape"], want=(True, True, True, False), seed=2, step=c["step"])
        _assert_maps(got[:3], c["want"], "r3d_tsdf_raycast_rgb")
    finally:
        V.close()


# ---- case 4 ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("h,w", E.RASTERS)
def test_depth_half(L, ctx, guard, h, w):
    c = E.half_case(h, w)
    d, want = c["depth"], c["want"]
    vertex = np.random.default_rng([4, h, w]).normal(size=(h, w, 3)).astype(F)
    vertex[..., 2] = d
    for stride, src, off in ((1, d, 0), (3, vertex, 4)):
        g_in, g_out = guard(src.nbytes, off, src, seed=stride), guard(want.nbytes, 4 - off, seed=5 + stride)
        L.check(ctx.lib.r3d_depth_half(ctx.handle, g_in.ptr + (8 if stride == 3 else 0), stride, h, w, c["max_jump"], g_out.ptr))
        assert_bits(g_out.read(F, want.shape), want, "r3d_depth_half, in_stride %d" % stride)
        g_in.unchanged()


@pytest.mark.parametrize("h,w", E.RASTERS)
def test_depth_bilateral(L, ctx, guard, h, w):
    tracking = importlib.import_module(PKG + ".tracking")
    radius, ss, sr = E.BILATERAL
    tables = tracking.bilateral_weights(radius, ss, sr)                 # the library's own table: the filter must use these numbers
    assert E.is_sub(tables[0]).sum() > 0
    d = E.edge_depth(h, w)
    with np.errstate(over="ignore"):
        want = E.bilateral_expect(d, tables)
    vertex = np.random.default_rng([5, h, w]).normal(size=(h, w, 3)).astype(F)
    vertex[..., 2] = d
    cases = [(1, d, 0), (3, vertex, 4)] if (h, w) == E.RASTERS[1] else [(1, d, 4)]
    for stride, src, off in cases:
        g_in, g_out = guard(src.nbytes, off, src, seed=stride), guard(want.nbytes, 4 - off, seed=5 + stride)
        L.check(ctx.lib.r3d_depth_bilateral(ctx.handle, g_in.ptr + (8 if stride == 3 else 0), stride, h, w, radius, ss, sr, g_out.ptr))
        assert_bits(g_out.read(F, want.shape), want, "r3d_depth_bilateral, in_stride %d" % stride)
        g_in.unchanged()


# ---- case 5 ---------------------------------------------------------------------------------------------------------------------
def test_projection_kernels(L, ctx, guard):
    c = E.project_case()
    inp, want = c["inp"], c["want"]
    B, H, W = E.PROJECT_SHAPE
    hw = H * W
    d = {n: guard(inp[n].nbytes, 0, inp[n], seed=1 + i) for i, n in enumerate(("depth", "inv_K", "gcam", "points", "P", "gpix"))}
    cam, gdep = guard(B * 4 * hw * 4, seed=10), guard(B * hw * 4, seed=11)
    pix, gpts = guard(B * hw * 8, seed=12), guard(B * 4 * hw * 4, seed=13)
    eps = C.c_float(float(E.PROJECT_EPS))
    L.check(ctx.lib.r3d_backproject_depth_f32(ctx.handle, d["depth"].ptr, d["inv_K"].ptr, B, H, W, cam.ptr))
    L.check(ctx.lib.r3d_backproject_depth_grad_f32(ctx.handle, d["gcam"].ptr, d["inv_K"].ptr, B, H, W, gdep.ptr))
    L.check(ctx.lib.r3d_project3d_f32(ctx.handle, d["points"].ptr, d["P"].ptr, B, H, W, eps, pix.ptr))
    L.check(ctx.lib.r3d_project3d_grad_f32(ctx.handle, d["gpix"].ptr, d["points"].ptr, d["P"].ptr, B, H, W, eps, gpts.ptr, None))
    assert_bits(cam.read(F, (B, 4, hw)), want["cam"], "cam_points")
    assert_bits(gdep.read(F, (B, hw)), want["gdep"], "grad_depth")
    assert_bits(pix.read(F, (B, H, W, 2)), want["pix"], "pix")
    assert_bits(gpts.read(F, (B, 4, hw)), want["gpts"], "grad_points")
    for b in d.values():
        b.unchanged()


# ---- case 6 ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", E.APPLY_KS)
def test_apply_T_and_se3_apply_round_once(L, ctx, guard, k):
    x = E.apply_points()
    n = len(x)
    want = E.apply_expect(x, k)
    g_in = guard(x.nbytes, 4, x, seed=1)
    T4, pose = np.ascontiguousarray(E.apply_T(k)), np.ascontiguousarray(E.apply_pose(k))
    out = guard(x.nbytes, 0, seed=2)
    L.check(ctx.lib.r3d_apply_T(ctx.handle, g_in.ptr, L.F32, n, T4.ctypes.data, out.ptr, L.F32))
    assert_bits(out.read(F, (n, 3)), want, "r3d_apply_T, T = 2^%d P" % -k)
    out = guard(x.nbytes, 4, seed=3)
    L.check(ctx.lib.r3d_se3_apply(ctx.handle, g_in.ptr, L.F32, n, pose.ctypes.data, out.ptr, L.F32))
    assert_bits(out.read(F, (n, 3)), want, "r3d_se3_apply, Rinv = 2^%d P" % -k)
    g_in.unchanged()


@pytest.mark.parametrize("k", E.APPLY_KS)
def test_unproject_rounds_once(L, ctx, guard, k):
    d = E.unproject_depth()
    h, w = d.shape
    want = E.unproject_expect(d, k)
    cam = ctx.camera(h, w, 1.0, 1.0, 0.0, 0.0)
    g_in, out = guard(d.nbytes, 0, d, seed=1), guard(want.nbytes, 4, seed=2)
    L.check(ctx.lib.r3d_unproject(ctx.handle, cam.handle, g_in.ptr, L.DEPTH_F32, 1, 2.0 ** -k, out.ptr, L.F32))
    assert_bits(out.read(F, want.shape), want, "r3d_unproject, depth_scale = 2^%d" % -k)
    g_in.unchanged()
