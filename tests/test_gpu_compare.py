"""GPU: r3d_mesh_index_*, r3d_distance_stats, r3d_sqrt_f32_inplace and r3d_distance_colors against tests/compare_ref.py, BIT FOR
BIT: distance, winning triangle and closest point.  Every output sits in a test_gpu_bounds.Guarded buffer, so a stray write shows;
every input is checked to be unchanged.  The cases are those of tests/test_compare_host.py, which asserts their conditions and
checks the restatement against an independent formulation first."""
import ctypes as C
import importlib
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import compare_ref as CR
import test_compare_host as H
from helpers import PKG, ROOT, r3d as _r3d
from test_gpu_bounds import Guarded

pytestmark = pytest.mark.gpu

INT32_MAX = 2 ** 31 - 1


@pytest.fixture(scope="module")
def R():
    return _r3d()


@pytest.fixture(scope="module")
def L(R):
    return importlib.import_module(PKG + "._lib")


@pytest.fixture(scope="module")
def E(R):
    return importlib.import_module(PKG + ".evaluation")


@pytest.fixture(scope="module")
def ctx(R):
    c = R.Context(0)
    yield c
    c.close()


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def same_floats(got, want):
    """bit for bit, any NaN standing for any NaN"""
    got, want = np.asarray(got, np.float32), np.asarray(want, np.float32)
    nan = np.isnan(want)
    return got.shape == want.shape and np.array_equal(np.isnan(got), nan) and np.array_equal(bits(got)[~nan], bits(want)[~nan])


def query(ctx, L, pts, v, tri, signed=False, tri_out=True, closest_out=True, groups=False, seed=0, between=None):
    """(distance, triangle or None, closest or None, groups or None) through guarded buffers; the inputs are checked afterwards"""
    pts = np.ascontiguousarray(pts, np.float32).reshape(-1, 3)
    v = np.ascontiguousarray(v, np.float32).reshape(-1, 3)
    tri = np.ascontiguousarray(tri, np.int32).reshape(-1, 3)
    n = len(pts)
    g_v, g_t = Guarded(ctx, v.nbytes, data=v, seed=seed), Guarded(ctx, tri.nbytes, off=4, data=tri, seed=seed + 1)
    g_p = Guarded(ctx, pts.nbytes, off=8, data=pts, seed=seed + 2)
    g_d, g_w, g_q = Guarded(ctx, n * 4, off=4, seed=seed + 3), Guarded(ctx, n * 4, off=12, seed=seed + 4), Guarded(ctx, n * 12, off=8, seed=seed + 5)
    made = [g_v, g_t, g_p, g_d, g_w, g_q]
    h = C.c_void_p()
    try:
        L.check(ctx.lib.r3d_mesh_index_create(ctx.handle, g_v.ptr if len(v) else None, len(v), g_t.ptr if len(tri) else None, len(tri),
                                              C.byref(h)))
        if between:
            between()
        k = C.c_int64(-1)
        L.check(ctx.lib.r3d_mesh_index_query(h.value, g_p.ptr if n else None, n, 1 if signed else 0, g_d.ptr if n else None,
                                             g_w.ptr if tri_out and n else None, g_q.ptr if closest_out and n else None,
                                             C.byref(k) if groups else None))
        ctx.sync()
        for g in (g_v, g_t, g_p):
            g.unchanged()
        if not tri_out:
            g_w.unchanged()
        if not closest_out:
            g_q.unchanged()
        return (g_d.read(np.float32), g_w.read(np.uint32) if tri_out else None, g_q.read(np.float32, (-1, 3)) if closest_out else None,
                k.value if groups else None)
    finally:
        if h.value:
            ctx.lib.r3d_mesh_index_destroy(h.value)
        for g in made:
            g.free()


def assert_matches(got, pts, v, tri, signed=False):
    want = CR.mesh_distance(pts, v, tri, signed=signed)
    assert same_floats(got[0], want[0])
    if got[1] is not None:
        assert np.array_equal(got[1], want[1])
    if got[2] is not None:
        assert same_floats(got[2], want[2])
    return want


_SIZED = {}


def sized_case(nt):
    """(points, vertices, triangles, reference): the first nt triangles of a marching-cubes mesh, with own vertices, jittered
    copies and far-away points; the reference is computed once"""
    if nt not in _SIZED:
        v, tri = H.volume_case(H.KEY_BIG if nt > 1025 else H.KEY_SMALL, nt)
        own = H.own_vertices(v, tri, 150)
        pts = np.concatenate([own, H.jittered(own[:80], 0.3), H.far_points(v[np.unique(tri)], 27)])
        _SIZED[nt] = (pts, v, tri, CR.mesh_distance(pts, v, tri))
    return _SIZED[nt]


@pytest.mark.parametrize("nt", H.TRIANGLE_SIZES)
def test_marching_cubes_meshes_at_the_group_boundaries(ctx, L, nt):
    pts, v, tri, want = sized_case(nt)
    assert len(tri) == nt
    got = query(ctx, L, pts, v, tri)
    assert same_floats(got[0], want[0]) and np.array_equal(got[1], want[1]) and same_floats(got[2], want[2])
    n_own = min(150, len(np.unique(tri)))
    assert (got[0][:n_own] == 0).all()                            # own vertices: exactly 0, the lowest triangle at the vertex


@pytest.mark.parametrize("n_points", H.POINT_SIZES)
def test_point_counts_at_the_wave_boundaries(ctx, L, n_points):
    v, tri = H.volume_case("sphere")
    own = H.own_vertices(v, tri, n_points, seed=3)
    k = len(own)
    pts = np.concatenate([own[:k // 2], H.jittered(own[k // 2:], 0.5, seed=4)]) if n_points > 1 else own
    pts = np.concatenate([pts, H.far_points(v, n_points - len(pts))]) if len(pts) < n_points else pts
    assert len(pts) == n_points
    assert_matches(query(ctx, L, pts, v, tri, signed=True), pts, v, tri, signed=True)


@pytest.mark.parametrize("name", list(H.HAND_CASES))
def test_hand_made_cases(ctx, L, name):
    """exact ties on the grid, points on shared edges and in the plane of coplanar triangles, degenerate triangles of every kind, a
    triangle listed twice, invalid indices, NaN / inf vertices and points, 1e30 and subnormal coordinates"""
    pts, v, tri = H.hand_case(name)
    for signed in (False, True):
        assert_matches(query(ctx, L, pts, v, tri, signed=signed), pts, v, tri, signed=signed)


def test_signed_on_both_sides_of_the_room_box(ctx, L):
    v, tri = H.room_box()
    pts = np.array([[0, 0, 0], [3, 0, 0], [0, 1, 2.5], [5, 0, 0], [5, 2.5, 4], [0, -2, 0], [4, 1.5, 3], [-4, 0, 0], [3.5, 1.25, 2.75]], np.float32)
    got = query(ctx, L, pts, v, tri, signed=True)
    assert_matches(got, pts, v, tri, signed=True)
    assert (got[0][[0, 1, 2, 8]] < 0).all() and (got[0][[3, 4, 5]] > 0).all() and not np.signbit(got[0][[6, 7]]).any()
    assert np.array_equal(np.abs(got[0]), query(ctx, L, pts, v, tri)[0])


def test_optional_outputs_and_empty_sizes(ctx, L):
    pts, v, tri = H.hand_case("grid")
    want = CR.mesh_distance(pts, v, tri)
    for tri_out, closest_out in ((False, True), (True, False), (False, False)):
        got = query(ctx, L, pts, v, tri, tri_out=tri_out, closest_out=closest_out)
        assert same_floats(got[0], want[0])
        assert got[1] is None or np.array_equal(got[1], want[1])
        assert got[2] is None or same_floats(got[2], want[2])
    none = query(ctx, L, pts, v, tri[:0], groups=True)                      # no triangle at all
    assert np.isinf(none[0]).all() and (none[1] == CR.NO_TRIANGLE).all() and np.isnan(none[2]).all() and none[3] == 0
    none = query(ctx, L, pts, v[:0], tri)                                   # no vertex: every triangle is invalid
    assert np.isinf(none[0]).all() and (none[1] == CR.NO_TRIANGLE).all() and np.isnan(none[2]).all()
    empty = query(ctx, L, pts[:0], v, tri, groups=True)                     # no point: nothing is written
    assert len(empty[0]) == 0 and empty[3] == 0


def test_shuffled_points_and_triangles_give_the_same_bits(ctx, L):
    pts, v, tri, want = sized_case(3000)
    rng = np.random.default_rng(11)
    pp, pt = rng.permutation(len(pts)), rng.permutation(len(tri))
    got = query(ctx, L, pts[pp], v, tri)
    assert same_floats(got[0], want[0][pp]) and np.array_equal(got[1], want[1][pp]) and same_floats(got[2], want[2][pp])
    got = query(ctx, L, pts, v, tri[pt])
    assert same_floats(got[0], want[0])
    # the winner is the tying triangle that comes first in the shuffled list
    d2 = CR.all_d2(pts[:150], v, tri)
    tie = d2 == d2.min(axis=1, keepdims=True)
    first = np.array([min(np.flatnonzero(tie[i][pt])) for i in range(150)])
    assert np.array_equal(got[1][:150], first.astype(np.uint32)) and (tie.sum(axis=1) > 1).sum() > 100
    assert np.array_equal(got[1], CR.mesh_distance(pts, v, tri[pt])[1])


def test_two_calls_with_other_library_calls_between(ctx, L, E, R):
    pts, v, tri, want = sized_case(1025)

    def between():
        cloud = np.random.default_rng(5).normal(size=(5000, 3)).astype(np.float32)
        R.knn(cloud, 4, ctx=ctx)
        E.distance_stats(cloud[:, 0], thresholds=(0.0,), bin_width=0.1, n_bins=64, ctx=ctx)

    for _ in range(2):
        got = query(ctx, L, pts, v, tri, between=between)
        assert same_floats(got[0], want[0]) and np.array_equal(got[1], want[1]) and same_floats(got[2], want[2])
        between()


def test_culling_evaluates_fewer_groups_than_brute_force(ctx, L):
    v, tri = H.volume_case(H.KEY_BIG, 3000)
    own = H.own_vertices(v, tri, 2000, seed=9)
    pts = H.jittered(own, 0.05, seed=10)
    got = query(ctx, L, pts, v, tri, groups=True)
    assert_matches(got, pts, v, tri)
    waves, groups = -(-len(pts) // 64), -(-len(tri) // 32)
    print("groups evaluated: %d of %d (%d waves x %d groups), ratio %.4f" % (got[3], waves * groups, waves, groups, got[3] / (waves * groups)))
    assert 0 < got[3] < waves * groups


# ---- statistics, root, colours ---------------------------------------------------------------------------------------------------
def stats(ctx, L, values, thresholds=(), bin_width=0.0, n_bins=0, squared=False):
    values = np.ascontiguousarray(values, np.float32)
    g = Guarded(ctx, values.nbytes, off=4, data=values, seed=len(values))
    try:
        thr = np.asarray(thresholds, np.float64)
        out, cnt, hist = np.full(6, -7.0), np.full(max(len(thr), 1), -7, np.int64), np.full(max(n_bins, 1), 7, np.uint64)
        L.check(ctx.lib.r3d_distance_stats(ctx.handle, g.ptr if len(values) else None, len(values), int(squared),
                                           thr.ctypes.data if len(thr) else None, len(thr), bin_width, n_bins, out.ctypes.data,
                                           cnt.ctypes.data if len(thr) else None, hist.ctypes.data if n_bins else None))
        g.unchanged()
        return out, cnt[:len(thr)], hist[:n_bins]
    finally:
        g.free()


def assert_stats(got, want):
    assert np.array_equal(got[0].view(np.uint64), want[0].view(np.uint64)), (got[0], want[0])
    assert np.array_equal(got[1], want[1]) and np.array_equal(got[2], want[2])


@pytest.mark.parametrize("n", [0, 1, 255, 256, 257, 65537])
def test_stats_at_the_row_and_finish_boundaries(ctx, L, n):
    rng = np.random.default_rng(n)
    d = (rng.uniform(0, 3, size=n) ** 2).astype(np.float32)
    if n > 2:
        d[rng.integers(0, n, size=max(n // 50, 1))] = [np.nan, np.inf, -np.inf][n % 3]
        d[n // 2] = 1.0
        d[n // 3] = 0.5                                           # on a bin edge, and equal to a threshold
    thr = (0.5, 1.0, 2.25, -1.0, 100.0)
    want = CR.distance_stats(d, thr, 0.25, 16)
    for _ in range(2):                                            # the same bits from run to run
        assert_stats(stats(ctx, L, d, thr, 0.25, 16), want)
    assert_stats(stats(ctx, L, d, (1.5,), 0.5, 4096, squared=True), CR.distance_stats(d, (1.5,), 0.5, 4096, squared=True))
    assert_stats(stats(ctx, L, d), CR.distance_stats(d))


def test_stats_edges_by_hand(ctx, L):
    d = np.array([0.0, 0.5, 1.0, 1.5, 2.0, 7.0, np.nan, np.inf, -np.inf, -0.0, 0.25, -1.0], np.float32)
    got = stats(ctx, L, d, (0.5, 1.0, -5.0, 100.0), 0.5, 4)
    assert_stats(got, CR.distance_stats(d, (0.5, 1.0, -5.0, 100.0), 0.5, 4))
    assert got[1].tolist() == [5, 6, 0, 9] and got[2].tolist() == [4, 1, 1, 3]
    for bad in (np.array([np.nan, np.inf], np.float32), np.full(300, np.nan, np.float32)):          # all non-finite
        got = stats(ctx, L, bad, (1.0,), 1.0, 2)
        assert_stats(got, CR.distance_stats(bad, (1.0,), 1.0, 2))
        assert got[0].tolist() == [0.0, len(bad), 0.0, 0.0, np.inf, -np.inf]
    zero = stats(ctx, L, np.array([-0.0], np.float32))[0]
    assert not np.signbit(zero[4]) and not np.signbit(zero[5])


def test_root_on_every_binade_edge(ctx, L):
    x = H.binade_edges()
    g = Guarded(ctx, x.nbytes, off=4, data=x)
    try:
        L.check(ctx.lib.r3d_sqrt_f32_inplace(ctx.handle, g.ptr, len(x)))
        got = g.read(np.float32)
    finally:
        g.free()
    assert np.array_equal(bits(got), bits(np.sqrt(x))) and np.array_equal(bits(got), bits(CR.sqrt_f32(x)))
    L.check(ctx.lib.r3d_sqrt_f32_inplace(ctx.handle, None, 0))


@pytest.mark.parametrize("n", [1, 257, 5000])
def test_colours(ctx, L, n):
    rng = np.random.default_rng(n)
    d = rng.normal(size=n).astype(np.float32) * 2
    d[::7] = [np.nan, np.inf, -np.inf, 0.0, 3.0, -3.0, 1.0][n % 7]
    d[:min(n, 766)] = (np.arange(min(n, 766)) / 765.0 * 3.0).astype(np.float32)      # every step of the ramp
    g_d, g_o = Guarded(ctx, d.nbytes, data=d), Guarded(ctx, n * 4, off=4, seed=1)
    try:
        L.check(ctx.lib.r3d_distance_colors(ctx.handle, g_d.ptr, n, 3.0, g_o.ptr))
        got = g_o.read(np.uint32)
        g_d.unchanged()
    finally:
        g_d.free()
        g_o.free()
    assert np.array_equal(got, CR.distance_colors(d, 3.0))


# ---- errors ------------------------------------------------------------------------------------------------------------------------
def test_argument_errors_write_nothing(ctx, L):
    lib, INV = ctx.lib, L.ERR_INVALID
    pts, v, tri = H.hand_case("grid")
    n = len(pts)
    g_v, g_t, g_p = Guarded(ctx, v.nbytes, data=v), Guarded(ctx, tri.nbytes, data=tri), Guarded(ctx, pts.nbytes, data=pts)
    g_d, g_w, g_q, g_c = Guarded(ctx, n * 4, seed=1), Guarded(ctx, n * 4, seed=2), Guarded(ctx, n * 12, seed=3), Guarded(ctx, n * 4, seed=4)
    h = C.c_void_p()
    try:
        sentinel = C.c_void_p(1)
        assert lib.r3d_mesh_index_create(None, g_v.ptr, len(v), g_t.ptr, len(tri), C.byref(sentinel)) == INV
        assert lib.r3d_mesh_index_create(ctx.handle, g_v.ptr, len(v), g_t.ptr, len(tri), None) == INV
        for args in ((g_v.ptr, -1, g_t.ptr, len(tri)), (g_v.ptr, len(v), g_t.ptr, -1), (None, len(v), g_t.ptr, len(tri)),
                     (g_v.ptr, len(v), None, len(tri))):
            assert lib.r3d_mesh_index_create(ctx.handle, *args, C.byref(h)) == INV and not h.value
        assert lib.r3d_mesh_index_create(ctx.handle, g_v.ptr, 2 ** 31, g_t.ptr, len(tri), C.byref(h)) == L.ERR_UNSUPPORTED and not h.value
        assert lib.r3d_mesh_index_destroy(None) == 0
        L.check(lib.r3d_mesh_index_create(ctx.handle, g_v.ptr, len(v), g_t.ptr, len(tri), C.byref(h)))
        k = C.c_int64(-5)
        bad = [(None, g_p.ptr, n, 0, g_d.ptr, g_w.ptr, g_q.ptr), (h.value, g_p.ptr, -1, 0, g_d.ptr, g_w.ptr, g_q.ptr),
               (h.value, None, n, 0, g_d.ptr, g_w.ptr, g_q.ptr), (h.value, g_p.ptr, n, 0, None, g_w.ptr, g_q.ptr),
               (h.value, g_p.ptr, n, 2, g_d.ptr, g_w.ptr, g_q.ptr), (h.value, g_p.ptr, n, -1, g_d.ptr, g_w.ptr, g_q.ptr),
               (h.value, g_p.ptr, n, 0, g_d.ptr, g_d.ptr, g_q.ptr), (h.value, g_p.ptr, n, 0, g_d.ptr, g_w.ptr, g_w.ptr),
               (h.value, g_p.ptr, n, 0, g_p.ptr + 8, g_w.ptr, g_q.ptr), (h.value, g_p.ptr, n, 0, g_d.ptr, g_w.ptr, g_p.ptr)]
        for args in bad:
            assert lib.r3d_mesh_index_query(*args, C.byref(k)) == INV, args
            assert k.value == -5
        out, cnt, hist, thr = np.full(6, -7.0), np.full(8, -7, np.int64), np.full(8, 7, np.uint64), np.array([1.0, np.nan])
        sbad = [(None, g_d.ptr, n, 0, thr.ctypes.data, 1, 1.0, 4, out.ctypes.data, cnt.ctypes.data, hist.ctypes.data),
                (ctx.handle, g_d.ptr, -1, 0, thr.ctypes.data, 1, 1.0, 4, out.ctypes.data, cnt.ctypes.data, hist.ctypes.data),
                (ctx.handle, None, n, 0, thr.ctypes.data, 1, 1.0, 4, out.ctypes.data, cnt.ctypes.data, hist.ctypes.data),
                (ctx.handle, g_d.ptr, n, 0, thr.ctypes.data, 1, 1.0, 4, None, cnt.ctypes.data, hist.ctypes.data),
                (ctx.handle, g_d.ptr, n, 0, thr.ctypes.data, 9, 1.0, 4, out.ctypes.data, cnt.ctypes.data, hist.ctypes.data),
                (ctx.handle, g_d.ptr, n, 0, thr.ctypes.data, -1, 1.0, 4, out.ctypes.data, cnt.ctypes.data, hist.ctypes.data),
                (ctx.handle, g_d.ptr, n, 0, None, 1, 1.0, 4, out.ctypes.data, cnt.ctypes.data, hist.ctypes.data),
                (ctx.handle, g_d.ptr, n, 0, thr.ctypes.data, 1, 1.0, 4, out.ctypes.data, None, hist.ctypes.data),
                (ctx.handle, g_d.ptr, n, 0, thr.ctypes.data, 2, 1.0, 4, out.ctypes.data, cnt.ctypes.data, hist.ctypes.data),   # NaN threshold
                (ctx.handle, g_d.ptr, n, 0, thr.ctypes.data, 1, 1.0, 4097, out.ctypes.data, cnt.ctypes.data, hist.ctypes.data),
                (ctx.handle, g_d.ptr, n, 0, thr.ctypes.data, 1, 1.0, -1, out.ctypes.data, cnt.ctypes.data, hist.ctypes.data),
                (ctx.handle, g_d.ptr, n, 0, thr.ctypes.data, 1, 1.0, 4, out.ctypes.data, cnt.ctypes.data, None),
                (ctx.handle, g_d.ptr, n, 0, thr.ctypes.data, 1, 0.0, 4, out.ctypes.data, cnt.ctypes.data, hist.ctypes.data),
                (ctx.handle, g_d.ptr, n, 0, thr.ctypes.data, 1, -1.0, 4, out.ctypes.data, cnt.ctypes.data, hist.ctypes.data),
                (ctx.handle, g_d.ptr, n, 0, thr.ctypes.data, 1, float("nan"), 4, out.ctypes.data, cnt.ctypes.data, hist.ctypes.data),
                (ctx.handle, g_d.ptr, n, 0, thr.ctypes.data, 1, float("inf"), 4, out.ctypes.data, cnt.ctypes.data, hist.ctypes.data)]
        for args in sbad:
            assert lib.r3d_distance_stats(*args) == INV, args
        assert (out == -7.0).all() and (cnt == -7).all() and (hist == 7).all()
        assert lib.r3d_distance_stats(ctx.handle, g_d.ptr, 2 ** 31, 0, None, 0, 0.0, 0, out.ctypes.data, None, None) == L.ERR_UNSUPPORTED
        for args in ((None, g_d.ptr, n), (ctx.handle, g_d.ptr, -1), (ctx.handle, None, n)):
            assert lib.r3d_sqrt_f32_inplace(*args) == INV
        for args in ((None, g_d.ptr, n, 1.0, g_c.ptr), (ctx.handle, g_d.ptr, -1, 1.0, g_c.ptr), (ctx.handle, None, n, 1.0, g_c.ptr),
                     (ctx.handle, g_d.ptr, n, 1.0, None), (ctx.handle, g_d.ptr, n, 0.0, g_c.ptr), (ctx.handle, g_d.ptr, n, -2.0, g_c.ptr),
                     (ctx.handle, g_d.ptr, n, float("nan"), g_c.ptr), (ctx.handle, g_d.ptr, n, float("inf"), g_c.ptr),
                     (ctx.handle, g_d.ptr, n, 1.0, g_d.ptr)):
            assert lib.r3d_distance_colors(*args) == INV, args
        for g in (g_v, g_t, g_p, g_d, g_w, g_q, g_c):
            g.unchanged()
    finally:
        if h.value:
            lib.r3d_mesh_index_destroy(h.value)
        for g in (g_v, g_t, g_p, g_d, g_w, g_q, g_c):
            g.free()


# ---- the Python layer and the tool, end to end -----------------------------------------------------------------------------------
def test_python_layer(ctx, E):
    pts, v, tri = H.hand_case("grid")
    want = CR.mesh_distance(pts, v, tri, signed=True)
    d, w, q = E.cloud_to_mesh_distance(pts, v, tri.astype(np.int64), signed=True, return_closest=True, ctx=ctx)
    assert same_floats(d, want[0]) and np.array_equal(w, want[1]) and same_floats(q, want[2])
    assert len(E.cloud_to_mesh_distance(pts, v, tri, ctx=ctx)) == 2
    rng = np.random.default_rng(3)
    a, b = rng.normal(size=(700, 3)).astype(np.float32), rng.normal(size=(900, 3)).astype(np.float32)
    d, i = E.cloud_to_cloud_distance(a, b, ctx=ctx)
    diff = a[:, None, :].astype(np.float64) - b[None].astype(np.float64)
    d2 = (diff * diff).sum(axis=2)
    assert np.array_equal(i, np.argmin(d2, axis=1)) and np.abs(d - np.sqrt(d2.min(axis=1))).max() <= 1e-6
    st = E.distance_stats(d, thresholds=(0.3,), bin_width=0.1, n_bins=8, ctx=ctx)
    ref = CR.distance_stats(d, (0.3,), 0.1, 8)
    assert st["n"] == 700 and st["sum"] == ref[0][2] and np.array_equal(st["counts"], ref[1]) and np.array_equal(st["hist"], ref[2])
    assert np.array_equal(E.distance_colors(d, 0.5, ctx=ctx), CR.distance_colors(d, 0.5))
    with E.MeshIndex(ctx, None, 0, None, 0) as index:
        assert index.handle
    assert index.handle is None


def test_room_reconstruction_end_to_end(ctx, R, E, tmp_path):
    """synthetic.room_views into the smallest room volume the TSDF tests use (tsdf_ref.room_scene: 0.2 m voxels), its mesh against
    the true room box at threshold = one voxel: every distance equals the restatement's, the numbers come from the restated sums,
    the tool prints the in-process numbers, and the median accuracy distance is at most one voxel (checked with the restatement
    on the CPU in tests/test_compare_host.py: 0.2 m voxels give a median well below 0.2 m)."""
    import tsdf_ref as REF
    IO = importlib.import_module(PKG + ".cloud_io")
    s = REF.room_scene()
    V = R.TSDFVolume(s["origin"], s["vs"], s["dims"], s["tr"], ctx=ctx)
    V.integrate(s["depths"], s["quats"], s["ts"], intrinsics=s["K"], depth_scale=s["scale"])
    xyz, nrm, tri = V.extract_triangle_mesh()
    V.close()
    box_v, box_t = H.room_box()
    thr = s["vs"]
    out, d_acc, d_com = E.evaluate_reconstruction((xyz, tri), (box_v, box_t), thr, ctx=ctx, return_distances=True)
    assert same_floats(d_acc, CR.mesh_distance(xyz, box_v, box_t)[0]) and same_floats(d_com, CR.mesh_distance(box_v, xyz, tri)[0])
    for side, d in (("accuracy", d_acc), ("completeness", d_com)):
        st, cnt, _ = CR.distance_stats(d, (thr,))
        assert out[side] == CR.side_numbers(st, int(cnt[0])), side
    assert out["precision"] == out["accuracy"]["within"] and out["recall"] == out["completeness"]["within"]
    assert out["f_score"] == CR.f_score(out["precision"], out["recall"])
    assert out["chamfer"] == out["accuracy"]["mean"] + out["completeness"]["mean"]
    med = float(np.median(d_acc))
    print("room: %d vertices, %d triangles, median accuracy %.4f m, report %s" % (len(xyz), len(tri), med, json.dumps(out, sort_keys=True)))
    assert len(xyz) > 1000 and med <= thr
    recon, truth, ply = str(tmp_path / "recon.ply"), str(tmp_path / "truth.ply"), str(tmp_path / "coloured.ply")
    IO.write_ply_mesh(recon, xyz, nrm, tri)
    IO.write_ply_mesh(truth, box_v, np.zeros_like(box_v), box_t)
    tool = os.path.join(ROOT, PKG, "other_tools", "compare_clouds.py")
    run = subprocess.run([sys.executable, tool, recon, truth, "--threshold", repr(thr), "--signed", "--hist", "8,0.05", "--ply", ply,
                          "--ply-max", "0.4"], capture_output=True, text=True, timeout=300)
    assert run.returncode == 0, run.stderr
    lines = [ln for ln in run.stdout.splitlines() if ln.strip()]
    assert len(lines) == 1
    printed = json.loads(lines[0])
    for key in ("accuracy", "completeness", "precision", "recall", "f_score", "chamfer", "threshold"):
        assert printed[key] == json.loads(json.dumps(out[key])), key
    signed = CR.mesh_distance(xyz, box_v, box_t, signed=True)[0]
    assert printed["signed_accuracy"]["min"] == float(signed.min()) and printed["signed_accuracy"]["max"] == float(signed.max())
    assert printed["hist"]["counts"] == [int(c) for c in CR.distance_stats(d_acc, (), 0.05, 8)[2]]
    got_xyz, got_rgba = IO.read_ply_rgb(ply)
    assert len(got_xyz) == len(xyz) and np.array_equal(got_rgba & 0xFFFFFF, CR.distance_colors(d_acc, 0.4))
