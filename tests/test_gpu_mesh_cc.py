"""GPU: r3d_mesh_components and r3d_mesh_filter_components against tests/mesh_cc_ref.py, BIT FOR BIT: vertex labels, triangle
labels, component rows, counts, kept vertices and renumbered triangles.  Every output sits in a test_gpu_bounds.Guarded buffer, so
a stray write shows; every input is checked to be unchanged.  The meshes are those of tests/test_mesh_cc_host.py, which asserts
their conditions of the restatement first: the project's marching-cubes meshes (floaters, vertices no triangle names), strips
where a label travels 5000 vertices and hooks race, thousands of tiny components, fans that meet in one hub, invalid indices."""
import ctypes as C
import importlib
import os
import shutil
import subprocess
import sys

import numpy as np
import pytest

import mesh_cc_ref as CC
import mesh_ref as MREF
from helpers import PKG, ROOT, r3d as _r3d
from test_gpu_bounds import Guarded
from test_gpu_mesh import assert_mesh, bits, uploaded
from test_mesh_cc_host import VOLUMES, volume_mesh

pytestmark = pytest.mark.gpu

KEYS = list(VOLUMES) + ["sphere"]
INT32_MAX = 2 ** 31 - 1


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


_REF = {}


def reference(name, tri, nv):
    """mesh_cc_ref.components of a named mesh, computed once and shared"""
    if name not in _REF:
        _REF[name] = CC.components(tri, nv)
    return _REF[name]


def components(ctx, L, tri, nv, cap=None, tri_labels=True, seed=0):
    """(labels, triangle labels or None, rows written, n_components, n_invalid) through guarded buffers; cap None: two calls, the
    first with cap 0 for the count"""
    tri = np.ascontiguousarray(tri, np.int32).reshape(-1, 3)
    nt = len(tri)
    g_tri = Guarded(ctx, tri.nbytes, data=tri, seed=seed)
    g_vl, g_tl = Guarded(ctx, nv * 4, off=4, seed=seed + 1), Guarded(ctx, nt * 4, off=8, seed=seed + 2)
    k, bad = C.c_int64(-1), C.c_int64(-1)
    made = [g_tri, g_vl, g_tl]
    try:
        if cap is None:
            L.check(ctx.lib.r3d_mesh_components(ctx.handle, g_tri.ptr, nt, nv, g_vl.ptr, g_tl.ptr if tri_labels else None, None, 0,
                                                C.byref(k), C.byref(bad)))
            cap = k.value
        g_rows = Guarded(ctx, cap * 12, off=12, seed=seed + 3)
        made.append(g_rows)
        before = g_rows.bytes().copy()
        L.check(ctx.lib.r3d_mesh_components(ctx.handle, g_tri.ptr, nt, nv, g_vl.ptr, g_tl.ptr if tri_labels else None,
                                            g_rows.ptr if cap else None, cap, C.byref(k), C.byref(bad)))
        g_tri.unchanged()
        written = min(cap, k.value)
        raw = g_rows.bytes()
        assert np.array_equal(raw[written * 12:], before[written * 12:])          # nothing beyond the rows that exist
        if not tri_labels:
            g_tl.unchanged()
        return (g_vl.read(np.uint32), g_tl.read(np.uint32) if tri_labels else None, raw[:written * 12].view(np.uint32).reshape(-1, 3),
                k.value, bad.value)
    finally:
        for g in made:
            g.free()


def filtered(ctx, L, tri, nv, labels, min_triangles, largest, cap_v=None, cap_t=None, seed=0):
    """(kept vertices written, triangles written, n, m) through guarded buffers; caps None: room for everything"""
    tri = np.ascontiguousarray(tri, np.int32).reshape(-1, 3)
    nt = len(tri)
    cap_v, cap_t = nv if cap_v is None else cap_v, nt if cap_t is None else cap_t
    g_tri, g_lab = Guarded(ctx, tri.nbytes, data=tri, seed=seed), Guarded(ctx, nv * 4, off=4, data=np.asarray(labels, np.uint32), seed=seed + 1)
    g_kept, g_out = Guarded(ctx, cap_v * 4, off=8, seed=seed + 2), Guarded(ctx, cap_t * 12, off=12, seed=seed + 3)
    try:
        before = [g_kept.bytes().copy(), g_out.bytes().copy()]
        n, m = C.c_int64(-1), C.c_int64(-1)
        L.check(ctx.lib.r3d_mesh_filter_components(ctx.handle, g_tri.ptr, nt, nv, g_lab.ptr, min_triangles, int(largest),
                                                   g_kept.ptr if cap_v else None, cap_v, g_out.ptr if cap_t else None, cap_t,
                                                   C.byref(n), C.byref(m)))
        g_tri.unchanged()
        g_lab.unchanged()
        wv, wt = min(cap_v, n.value), min(cap_t, m.value)
        kept, out = g_kept.bytes(), g_out.bytes()
        assert np.array_equal(kept[wv * 4:], before[0][wv * 4:]) and np.array_equal(out[wt * 12:], before[1][wt * 12:])
        return kept[:wv * 4].view(np.uint32), out[:wt * 12].view(np.int32).reshape(-1, 3), n.value, m.value
    finally:
        for g in (g_tri, g_lab, g_kept, g_out):
            g.free()


def assert_components(got, want):
    labels, tl, rows, k, bad = got
    assert np.array_equal(labels, want[0])
    if tl is not None:
        assert np.array_equal(tl, want[1])
    assert k == len(want[2]) and bad == want[3]
    assert rows.dtype == np.uint32 and np.array_equal(rows, want[2][:len(rows)])


def assert_filter(ctx, L, tri, nv, labels, mt, largest, seed=0):
    kept, out, n, m = filtered(ctx, L, tri, nv, labels, mt, largest, seed=seed)
    want_kept, want_out = CC.filter_components(tri, nv, labels, mt, largest)
    assert (n, m) == (len(want_kept), len(want_out))
    assert np.array_equal(kept, want_kept) and np.array_equal(out, want_out)
    return n, m


# ---- the project's own meshes ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("key", KEYS, ids=[str(k) for k in KEYS])
def test_reference_meshes(ctx, L, key):
    xyz, _, tri = volume_mesh(key)
    nv = len(xyz)
    want = reference(key, tri, nv)
    assert_components(components(ctx, L, tri, nv, seed=1), want)                   # the two-call protocol
    k = len(want[2])
    for cap in (0, k - 1, k, k + 3):
        got = components(ctx, L, tri, nv, cap=cap, tri_labels=cap != 0, seed=cap)
        assert_components(got, want)
        assert len(got[2]) == min(cap, k)


@pytest.mark.parametrize("key", KEYS, ids=[str(k) for k in KEYS])
def test_triangle_order_does_not_change_the_labels(ctx, L, key):
    xyz, _, tri = volume_mesh(key)
    nv = len(xyz)
    want = reference(key, tri, nv)
    perm = np.random.default_rng(3).permutation(len(tri))
    labels, tl, rows, k, bad = components(ctx, L, tri[perm], nv)
    assert np.array_equal(labels, want[0]) and np.array_equal(tl, want[1][perm]) and np.array_equal(rows, want[2])


# ---- strips: a label travels far, hooks race ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("ids", ["in order", "reversed", "permuted"])
def test_strip(ctx, L, ids):
    rng = np.random.default_rng(11)
    n = 5000
    names = {"in order": None, "reversed": np.arange(n + 2)[::-1], "permuted": rng.permutation(n + 2)}[ids]
    tri = CC.strip(n, names)
    if ids != "in order":
        tri = tri[rng.permutation(n)]
    labels, tl, rows, k, bad = components(ctx, L, tri, n + 2)
    assert (labels == 0).all() and (tl == 0).all() and rows.tolist() == [[0, n + 2, n]] and (k, bad) == (1, 0)
    assert assert_filter(ctx, L, tri, n + 2, labels, n, True) == (n + 2, n)
    assert assert_filter(ctx, L, tri, n + 2, labels, n + 1, False) == (0, 0)


# ---- thousands of tiny components, duplicates, degenerates, one hub ---------------------------------------------------------------
def test_tiny_components(ctx, L):
    n = 4096
    tri = CC.disjoint(n)
    want = CC.components(tri, 3 * n)
    assert len(want[2]) == n and (want[2][:, 1:] == [3, 1]).all()
    assert_components(components(ctx, L, tri, 3 * n), want)
    dup = np.repeat(tri, 2, axis=0)
    want = CC.components(dup, 3 * n)
    assert len(want[2]) == n and (want[2][:, 1:] == [3, 2]).all()                  # a duplicate counts once each
    got = components(ctx, L, dup, 3 * n)
    assert_components(got, want)
    assert assert_filter(ctx, L, dup, 3 * n, got[0], 2, False) == (3 * n, 2 * n)
    assert assert_filter(ctx, L, dup, 3 * n, got[0], 3, False) == (0, 0)
    assert assert_filter(ctx, L, dup, 3 * n, got[0], 1, True) == (3, 2)            # all tie: label 0 wins
    mixed = tri.copy()
    mixed[1::4, 1] = mixed[1::4, 0]                                                # (a, a, b): joins a and b, the middle vertex is left alone
    mixed[2::4, 1:] = mixed[2::4, :1]                                              # (a, a, a)
    mixed[3::8, 2] = mixed[2::8, 0]                                                # ... and some reach into the neighbouring triangle
    want = CC.components(mixed, 3 * n)
    assert want[3] == 0 and n // 2 < len(want[2]) < n and len(np.unique(want[0])) > n
    got = components(ctx, L, mixed, 3 * n)
    assert_components(got, want)
    for mt in (1, 2):
        assert_filter(ctx, L, mixed, 3 * n, got[0], mt, False)


def test_fans_that_share_one_hub(ctx, L):
    tri, nv = CC.fans(64, 5)
    tri = tri[np.random.default_rng(5).permutation(len(tri))]
    labels, tl, rows, k, bad = components(ctx, L, tri, nv)
    assert (labels == 0).all() and rows.tolist() == [[0, nv, 320]]
    tri2, nv2 = tri + 1, nv + 1                                                    # the hub is vertex 1, vertex 0 is named by nobody
    got = components(ctx, L, tri2, nv2)
    assert_components(got, CC.components(tri2, nv2))
    assert got[0][0] == 0 and (got[0][1:] == 1).all()


# ---- invalid triangles -------------------------------------------------------------------------------------------------------------
def test_invalid_triangles_join_nothing_and_are_never_kept(ctx, L):
    xyz, _, tri = volume_mesh(((9, 8, 7), 5, 0.0))
    nv = len(xyz)
    rng = np.random.default_rng(17)
    bad_rows = []
    for value in (-1, nv, INT32_MAX, -2 ** 31, nv + 7):
        for col in range(3):
            row = tri[rng.integers(len(tri))].copy()
            row[col] = value
            bad_rows.append(row)
    bad_rows.append(np.array([-1, nv, INT32_MAX], np.int32))
    mixed = np.concatenate([tri, np.array(bad_rows, np.int32)])
    mixed = mixed[rng.permutation(len(mixed))]
    is_bad = ~CC.valid_mask(mixed, nv)
    assert is_bad.sum() == len(bad_rows)
    want = CC.components(mixed, nv)
    clean = reference(((9, 8, 7), 5, 0.0), tri, nv)
    assert np.array_equal(want[0], clean[0]) and np.array_equal(want[2], clean[2])  # they join nothing and count nowhere
    got = components(ctx, L, mixed, nv)
    assert_components(got, want)
    assert got[4] == len(bad_rows) and (got[1][is_bad] == 0xFFFFFFFF).all() and (got[1][~is_bad] != 0xFFFFFFFF).all()
    for mt, largest in ((1, False), (5, False), (1, True)):
        n, m = assert_filter(ctx, L, mixed, nv, got[0], mt, largest)
        assert m <= len(tri)
    assert assert_filter(ctx, L, mixed, nv, got[0], 1, False)[1] == len(tri)       # exactly the valid ones
    # every triangle invalid, and a mesh without vertices
    only = np.array(bad_rows, np.int32)
    assert_components(components(ctx, L, only, nv), CC.components(only, nv))
    got = components(ctx, L, only, 0)
    assert got[3:] == (0, len(only)) and (got[1] == 0xFFFFFFFF).all() and got[0].size == 0
    assert filtered(ctx, L, only, 0, np.zeros(0, np.uint32), 1, False)[2:] == (0, 0)
    # labels are data for the filter: one outside the mesh is never an address, its triangles count as invalid
    wild = clean[0].copy()
    wild[wild == 0] = 0xFFFFFFF0
    assert assert_filter(ctx, L, tri, nv, wild, 1, False)[1] == len(tri) - int(clean[2][0, 2])


# ---- sizes -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nt", [0, 1, 63, 64, 65, 255, 256, 257, 4097])
def test_sizes(ctx, L, nt):
    rng = np.random.default_rng(nt)
    nv = max(3, (nt * 3) // 2)
    tri = rng.integers(0, nv, (nt, 3)).astype(np.int32)                            # sparse random triangles: a handful of components
    tri[: nt // 2] = np.sort(rng.integers(0, nv, nt // 2))[:, None] + np.array([0, 1, 2]) % nv
    tri %= nv
    want = CC.components(tri, nv)
    got = components(ctx, L, tri, nv)
    assert_components(got, want)
    for mt, largest in ((1, False), (2, False), (1, True)):
        assert_filter(ctx, L, tri, nv, got[0], mt, largest, seed=nt)
    one = np.zeros((nt, 3), np.int32)                                              # n_vertices = 1: every triangle is (0, 0, 0)
    got = components(ctx, L, one, 1)
    assert_components(got, CC.components(one, 1))
    assert got[0].tolist() == [0] and got[3] == (1 if nt else 0)
    assert assert_filter(ctx, L, one, 1, got[0], 1, True) == ((1, nt) if nt else (0, 0))


# ---- the filter --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("key", KEYS, ids=[str(k) for k in KEYS])
def test_filter_thresholds(ctx, L, key):
    xyz, _, tri = volume_mesh(key)
    nv = len(xyz)
    labels, _, rows, _ = reference(key, tri, nv)
    big = int(rows[:, 2].max())
    seen = set()
    for mt in (1, 2, 5, 99, big, big + 1):
        for largest in (False, True):
            seen.add(assert_filter(ctx, L, tri, nv, labels, mt, largest, seed=mt))
    assert assert_filter(ctx, L, tri, nv, labels, big + 1, False) == (0, 0)        # the last threshold empties the mesh
    assert assert_filter(ctx, L, tri, nv, labels, 1, True)[1] == big
    assert len(seen) >= (2 if key == "sphere" else 4)


def test_filter_caps(ctx, L):
    key = ((16, 16, 16), 85, 0.3)
    xyz, _, tri = volume_mesh(key)
    nv = len(xyz)
    labels = reference(key, tri, nv)[0]
    want_kept, want_out = CC.filter_components(tri, nv, labels, 5, False)
    n, m = len(want_kept), len(want_out)
    assert 0 < n < nv and 0 < m < len(tri)
    for cv in (0, n - 1, n):
        for ct in (0, m - 1, m):
            kept, out, gn, gm = filtered(ctx, L, tri, nv, labels, 5, False, cv, ct, seed=cv + ct)
            assert (gn, gm) == (n, m)                                              # always the true counts
            assert np.array_equal(kept, want_kept[:cv]) and np.array_equal(out, want_out[:ct])   # rows as they are


def test_tie_goes_to_the_smaller_label(ctx, L):
    a, b = CC.strip(300), CC.strip(300) + 400
    small = np.array([[350, 351, 352]], np.int32)
    for tri in (np.concatenate([a, small, b]), np.concatenate([b, small, a])):     # whichever comes first in the array
        labels, _, rows, k, _ = components(ctx, L, tri, 702)
        assert rows.tolist() == [[0, 302, 300], [350, 3, 1], [400, 302, 300]]
        kept, out, n, m = filtered(ctx, L, tri, 702, labels, 1, True)
        assert (n, m) == (302, 300) and kept.tolist() == list(range(302))
        assert_filter(ctx, L, tri, 702, labels, 1, True)
        assert_filter(ctx, L, tri, 702, labels, 2, False)


# ---- argument errors on a live context ---------------------------------------------------------------------------------------------
def test_invalid_calls_write_nothing(ctx, L):
    tri = CC.strip(10)
    g_tri, g_a, g_b = Guarded(ctx, tri.nbytes, data=tri), Guarded(ctx, 480, seed=1), Guarded(ctx, 480, seed=2)
    ba, bb = g_a.bytes().copy(), g_b.bytes().copy()
    x, y = C.c_int64(-7), C.c_int64(-9)
    px, py = C.byref(x), C.byref(y)
    h, t, a, b = ctx.handle, g_tri.ptr, g_a.ptr, g_b.ptr
    comp = [(None, t, 10, 12, a, None, None, 0, px, py), (h, t, 10, 12, a, None, None, 0, None, py), (h, t, -1, 12, a, None, None, 0, px, py),
            (h, t, 10, -1, a, None, None, 0, px, py), (h, None, 10, 12, a, None, None, 0, px, py), (h, t, 10, 12, None, None, None, 0, px, py),
            (h, t, 10, 12, a, None, None, 5, px, py), (h, t, 10, 12, a, a + 44, None, 0, px, py), (h, t, 10, 12, a, None, a + 40, 5, px, py),
            (h, t, 10, 12, t + 100, None, None, 0, px, py), (h, t, 10, 12, a, b, b + 36, 1, px, py)]
    for args in comp:
        assert ctx.lib.r3d_mesh_components(*args) == L.ERR_INVALID, args
    filt = [(None, t, 10, 12, a, 1, 0, b, 12, None, 0, px, py), (h, t, 10, 12, a, 0, 0, b, 12, None, 0, px, py),
            (h, t, 10, 12, a, 1, 0, b, -1, None, 0, px, py), (h, t, 10, 12, a, 1, 0, None, 12, None, 0, px, py),
            (h, t, 10, 12, a, 1, 0, None, 0, None, 10, px, py), (h, t, 10, 12, a, 1, 0, a + 44, 12, None, 0, px, py),
            (h, t, 10, 12, a, 1, 0, b, 12, b + 44, 10, px, py), (h, t, 10, 12, a, 1, 0, b, 12, t + 8, 10, px, py),
            (h, t, 10, 12, a, 1, 0, b, 12, None, 0, None, py)]
    for args in filt:
        assert ctx.lib.r3d_mesh_filter_components(*args) == L.ERR_INVALID, args
    assert (x.value, y.value) == (-7, -9)
    assert np.array_equal(g_a.bytes(), ba) and np.array_equal(g_b.bytes(), bb)
    g_tri.unchanged()
    for g in (g_tri, g_a, g_b):
        g.free()


# ---- call order on one context -----------------------------------------------------------------------------------------------------
def test_call_order_on_one_context(R, T, L):
    import call_order_cases as CAT
    key = ((16, 16, 16), 85, 0.3)
    ref = MREF.random_volume(*key)
    xyz, _, tri = volume_mesh(key)
    nv = len(xyz)

    def cc(c):
        got = components(c, L, tri, nv)
        return b"".join(np.ascontiguousarray(a).tobytes() for a in got[:3]) + np.array(got[3:], np.int64).tobytes(), got[0]

    def filt(c, labels, mt, largest):
        return b"".join(np.ascontiguousarray(a).tobytes() for a in filtered(c, L, tri, nv, labels, mt, largest)[:2])

    def mesh(c):
        V = uploaded(T, c, ref)
        try:
            return b"".join(np.ascontiguousarray(a).tobytes() for a in V.extract_triangle_mesh())
        finally:
            V.close()

    def alone(f, *args):
        c = R.Context(0)
        try:
            return f(c, *args)
        finally:
            c.close()

    base_cc, labels = alone(cc)
    base = {"f5": alone(filt, labels, 5, False), "fl": alone(filt, labels, 1, True), "mesh": alone(mesh),
            "sort": alone(CAT.CASES["sort"]), "grid": alone(CAT.CASES["voxelgrid"])}
    assert np.array_equal(labels, reference(key, tri, nv)[0])
    large_sort = alone(CAT.CASES["sort"], 4)
    c = R.Context(0)
    try:
        for step in range(2):
            assert mesh(c) == base["mesh"]
            assert cc(c)[0] == base_cc
            assert CAT.CASES["sort"](c) == base["sort"]
            assert filt(c, labels, 5, False) == base["f5"]
            assert CAT.CASES["voxelgrid"](c) == base["grid"]
            assert filt(c, labels, 1, True) == base["fl"]
            assert mesh(c) == base["mesh"]
            assert CAT.CASES["sort"](c, 4) == large_sort                           # a larger instance in between
            assert cc(c)[0] == base_cc
            # a larger mesh grows the workspace between two runs of the smaller one
            big = volume_mesh(((16, 16, 17), 86, 0.0))
            assert_components(components(c, L, big[2], len(big[0])), reference(((16, 16, 17), 86, 0.0), big[2], len(big[0])))
            assert filt(c, labels, 5, False) == base["f5"]
    finally:
        c.close()


# ---- end to end --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("key", [((16, 16, 17), 86, 0.0), ((40, 9, 5), 3, 0.2)], ids=str)
def test_extract_triangle_mesh_filters_on_the_device(T, ctx, key):
    ref = MREF.random_volume(*key)
    mesh = volume_mesh(key)
    V = uploaded(T, ctx, ref)
    try:
        assert_mesh(V.extract_triangle_mesh(), mesh)                               # the default call is unchanged
        assert_mesh(V.extract_triangle_mesh(min_component_triangles=5), CC.remove_small(*mesh, 5, False))
        assert_mesh(V.extract_triangle_mesh(keep_largest=True), CC.remove_small(*mesh, 1, True))
        assert_mesh(V.extract_triangle_mesh(min_component_triangles=3, keep_largest=True), CC.remove_small(*mesh, 3, True))
        got = V.extract_triangle_mesh(min_component_triangles=5, with_stats=True)
        rows = reference(key, mesh[2], len(mesh[0]))[2]
        kept = rows[rows[:, 2] >= 5]
        assert got[-1] == {"components": len(rows), "components_kept": len(kept), "triangles": len(mesh[2]),
                           "triangles_kept": int(kept[:, 2].sum())}
        assert [a.shape for a in V.extract_triangle_mesh(min_component_triangles=10 ** 6)] == [(0, 3)] * 3
        assert_mesh(V.extract_triangle_mesh(), mesh)
        for bad in (0, -3, 2.5, True):
            with pytest.raises(ValueError):
                V.extract_triangle_mesh(min_component_triangles=bad)
    finally:
        V.close()


def test_module_functions(R, ctx):
    key = ((9, 8, 7), 5, 0.0)
    xyz, nrm, tri = volume_mesh(key)
    want = reference(key, tri, len(xyz))
    got = R.mesh_components(tri, len(xyz), ctx=ctx)
    assert np.array_equal(got.vertex_labels, want[0]) and np.array_equal(got.triangle_labels, want[1])
    assert got.components.dtype == np.uint32 and np.array_equal(got.components, want[2]) and got.n_invalid == 0
    colors = np.random.default_rng(2).integers(0, 256, (len(xyz), 3), dtype=np.uint8)
    for mt, largest in ((5, False), (1, True), (10 ** 6, False)):
        res = R.remove_small_components(xyz, nrm, tri.astype(np.int64), mt, largest, colors=colors, ctx=ctx)
        ref = CC.remove_small(xyz, nrm, tri, mt, largest, colors=colors)
        assert np.array_equal(bits(res[0]), bits(ref[0])) and np.array_equal(bits(res[1]), bits(ref[1]))
        assert res[2].dtype == np.int64 and np.array_equal(res[2], ref[2])
        assert res[3].dtype == np.uint8 and np.array_equal(res[3], ref[3])
    empty = R.mesh_components(np.zeros((0, 3), np.int32), 4, ctx=ctx)
    assert empty.vertex_labels.tolist() == [0, 1, 2, 3] and empty.components.shape == (0, 3) and empty.triangle_labels.shape == (0,)


def test_colour_volume_end_to_end(T, ctx):
    import test_gpu_tsdf_color as TC
    import tsdf_color_ref as CREF
    s, rgb, ref, _ = TC.scene((33, 9, 5), 32, np.uint16, seed=TC.DIMS.index((33, 9, 5)) + 1)
    V = TC.color_volume(T, ctx, s)
    try:
        TC.integrate_rgb(ctx, V, s, rgb)
        mesh = MREF.extract_mesh(ref)
        colors = CREF.extract_colors(ref)
        rows = CC.components(mesh[2], len(mesh[0]))[2]
        assert len(rows) > 3 and rows[:, 2].min() < 5 <= rows[:, 2].max()          # both filters drop something and keep something
        plain = V.extract_triangle_mesh(with_colors=True)
        assert_mesh(plain[:3], mesh)
        assert np.array_equal(plain[3], colors)
        for kw, args in (({"min_component_triangles": 5}, (5, False)), ({"keep_largest": True}, (1, True))):
            want = CC.remove_small(*mesh, *args, colors=colors)
            got = V.extract_triangle_mesh(with_colors=True, **kw)
            assert 0 < len(want[2]) < len(mesh[2])
            assert_mesh(got[:3], want[:3])
            assert got[3].dtype == np.uint8 and np.array_equal(got[3], want[3])
    finally:
        V.close()


def test_command_line_keeps_the_largest_component(R, golden_dir, tmp_path):
    work = tmp_path / "work"
    shutil.copytree(os.path.join(golden_dir, "scene3", "depth"), work / "depth")
    shutil.copytree(os.path.join(golden_dir, "scene3", "camera_pose"), work / "camera_pose")
    tool = os.path.join(ROOT, PKG, "other_tools", "integrate_tsdf.py")
    args = ["--voxel-size", "8", "--trunc", "24", "--origin", "-300", "-300", "-300", "--dims", "75", "75", "75", "--min-weight", "1"]
    env = dict(os.environ, PYTHONPATH=ROOT, R3D_FX="20", R3D_FY="20", R3D_CX="15.5", R3D_CY="11.5")
    script = ("import runpy, shutil, sys\n"
              "tool, base = sys.argv[1], sys.argv[2:]\n"
              "for extra, keep in ((['--mesh'], 'plain.ply'), (['--mesh', '--mesh-largest'], 'largest.ply'),\n"
              "                    (['--mesh', '--mesh-min-component', '5'], 'min5.ply')):\n"
              "    sys.argv = [tool] + base + extra\n"
              "    runpy.run_path(tool, run_name='__main__')\n"
              "    shutil.copy('./ply/tsdf_mesh.ply', keep)\n")
    r = subprocess.run([sys.executable, "-c", script, tool] + args, cwd=str(work), env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-1000:] + r.stderr[-2000:]
    plain = R.cloud_io.read_ply_mesh(str(work / "plain.ply"))
    rows = CC.components(plain[2], len(plain[0]))[2]
    lines = [l for l in r.stdout.split("\n") if l.startswith("components")]
    assert len(lines) == 2
    for name, mt, largest, line in (("largest.ply", 1, True, lines[0]), ("min5.ply", 5, False, lines[1])):
        want = CC.remove_small(*plain, mt, largest)
        got = R.cloud_io.read_ply_mesh(str(work / name))
        assert (len(got[0]), len(got[2])) == (len(want[0]), len(want[2]))          # vertex and face counts
        assert_mesh(got, want)
        kept = 1 if largest else int((rows[:, 2] >= mt).sum())
        assert line == "components %d kept %d triangles kept %d dropped %d" % (len(rows), kept, len(want[2]), len(plain[2]) - len(want[2]))
    pts = R.cloud_io.read_ply_normals(str(work / "ply" / "tsdf_surface.ply"))
    assert len(pts[0]) == len(plain[0]) and len(plain[2]) > 1000
