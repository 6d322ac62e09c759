"""GPU: r3d_mesh_adjacency, r3d_mesh_smooth and r3d_mesh_vertex_normals against tests/mesh_smooth_ref.py, BIT FOR BIT.  Every output
sits in a test_gpu_bounds.Guarded buffer, so a stray write shows; every input is checked to be unchanged.  The meshes are those of
tests/test_mesh_smooth_host.py, which asserts their conditions of the restatement first, plus a fan whose hub has 5001 neighbours
(one lane looping long), a strip, disjoint triangles, and the sizes where the sort's tile and pass counts change."""
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
import mesh_smooth_ref as MS
from f32_edge_cases import first_mismatch, same_bits
from helpers import PKG, ROOT, r3d as _r3d
from test_gpu_bounds import Guarded
from test_gpu_mesh import assert_mesh, bits, uploaded
from test_mesh_cc_host import volume_mesh
from test_mesh_smooth_host import MESHES, adjacency_of

pytestmark = pytest.mark.gpu

KEYS = list(MESHES)
INT32_MIN = -2 ** 31


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


def adjacency(ctx, L, tri, nv, cap=None, with_boundary=True, seed=0):
    """(row_start, the neighbour entries written, boundary or None, E) through guarded buffers; cap None: two calls, the first with
    cap 0 and no neighbour array for the count"""
    tri = np.ascontiguousarray(tri, np.int32).reshape(-1, 3)
    nt = len(tri)
    g_tri = Guarded(ctx, tri.nbytes, data=tri, seed=seed)
    g_rs, g_bd = Guarded(ctx, (nv + 1) * 4, off=4, seed=seed + 1), Guarded(ctx, nv, off=1, seed=seed + 2)
    made = [g_tri, g_rs, g_bd]
    e = C.c_int64(-1)
    bd = g_bd.ptr if with_boundary else None
    try:
        if cap is None:
            L.check(ctx.lib.r3d_mesh_adjacency(ctx.handle, g_tri.ptr, nt, nv, g_rs.ptr, None, 0, bd, C.byref(e)))
            cap = e.value
        g_nb = Guarded(ctx, cap * 4, off=12, seed=seed + 3)
        made.append(g_nb)
        before = g_nb.bytes().copy()
        L.check(ctx.lib.r3d_mesh_adjacency(ctx.handle, g_tri.ptr, nt, nv, g_rs.ptr, g_nb.ptr if cap else None, cap, bd, C.byref(e)))
        g_tri.unchanged()
        written = min(cap, e.value)
        raw = g_nb.bytes()
        assert np.array_equal(raw[written * 4:], before[written * 4:])              # nothing beyond the entries that exist
        if not with_boundary:
            g_bd.unchanged()
        return g_rs.read(np.uint32), raw[:written * 4].view(np.uint32), g_bd.read(np.uint8) if with_boundary else None, e.value
    finally:
        for g in made:
            g.free()


def assert_adjacency(ctx, L, tri, nv, want=None, seed=0):
    want = want or MS.adjacency(tri, nv)
    rs, nb, bd, e = adjacency(ctx, L, tri, nv, seed=seed)
    assert e == len(want[1]) == int(want[0][-1])
    assert np.array_equal(rs, want[0]) and np.array_equal(nb, want[1]) and np.array_equal(bd, want[2])
    return want


def smooth(ctx, L, xyz, rs, nb, locked, factors, seed=0):
    """the smoothed positions through guarded buffers; every input is checked to be unchanged"""
    xyz = np.ascontiguousarray(xyz, np.float32).reshape(-1, 3)
    nv = len(xyz)
    g_in, g_out = Guarded(ctx, xyz.nbytes, off=4, data=xyz, seed=seed), Guarded(ctx, xyz.nbytes, off=8, seed=seed + 1)
    g_rs = Guarded(ctx, (nv + 1) * 4, data=np.asarray(rs, np.uint32), seed=seed + 2)
    g_nb = Guarded(ctx, len(nb) * 4, off=4, data=np.asarray(nb, np.uint32), seed=seed + 3)
    g_lk = Guarded(ctx, nv, off=3, data=np.asarray(locked, np.uint8), seed=seed + 4) if locked is not None else None
    f = np.asarray(factors, np.float64)
    try:
        L.check(ctx.lib.r3d_mesh_smooth(ctx.handle, g_in.ptr, g_out.ptr, nv, g_rs.ptr, g_nb.ptr, g_lk.ptr if g_lk else None,
                                        f.ctypes.data if len(f) else None, len(f)))
        out = g_out.read(np.float32, (-1, 3))
        for g in (g_in, g_rs, g_nb) + ((g_lk,) if g_lk else ()):
            g.unchanged()
        return out
    finally:
        for g in (g_in, g_out, g_rs, g_nb) + ((g_lk,) if g_lk else ()):
            g.free()


def normals(ctx, L, xyz, tri, fallback=None, seed=0):
    xyz, tri = np.ascontiguousarray(xyz, np.float32).reshape(-1, 3), np.ascontiguousarray(tri, np.int32).reshape(-1, 3)
    nv = len(xyz)
    g_xyz, g_tri = Guarded(ctx, xyz.nbytes, off=4, data=xyz, seed=seed), Guarded(ctx, tri.nbytes, off=8, data=tri, seed=seed + 1)
    g_fb = Guarded(ctx, xyz.nbytes, off=12, data=np.ascontiguousarray(fallback, np.float32), seed=seed + 2) if fallback is not None else None
    g_out = Guarded(ctx, xyz.nbytes, off=4, seed=seed + 3)
    try:
        L.check(ctx.lib.r3d_mesh_vertex_normals(ctx.handle, g_xyz.ptr, nv, g_tri.ptr, len(tri), g_fb.ptr if g_fb else None, g_out.ptr))
        out = g_out.read(np.float32, (-1, 3))
        for g in (g_xyz, g_tri) + ((g_fb,) if g_fb else ()):
            g.unchanged()
        return out
    finally:
        for g in (g_xyz, g_tri, g_out) + ((g_fb,) if g_fb else ()):
            g.free()


def assert_bits(got, want):
    assert same_bits(got, want), first_mismatch(got, want)


def random_triangles(nv, nt, seed):
    return np.random.default_rng([seed, nv, nt]).integers(0, nv, (nt, 3)).astype(np.int32)


# ---- adjacency ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("key", KEYS, ids=str)
def test_adjacency_of_the_reference_meshes(ctx, L, key):
    xyz, _, tri = volume_mesh(key)
    assert_adjacency(ctx, L, tri, len(xyz), adjacency_of(key))
    perm = np.random.default_rng(9).permutation(len(tri))
    assert_adjacency(ctx, L, tri[perm][:, [1, 2, 0]], len(xyz), adjacency_of(key), seed=5)     # triangle order and corner rotation


def test_adjacency_of_empty_and_tiny_meshes(ctx, L):
    none = np.zeros((0, 3), np.int32)
    rs, nb, bd, e = adjacency(ctx, L, none, 0)
    assert rs.tolist() == [0] and len(nb) == 0 and len(bd) == 0 and e == 0
    rs, nb, bd, e = adjacency(ctx, L, none, 5)
    assert rs.tolist() == [0] * 6 and bd.tolist() == [0] * 5 and e == 0
    rs, nb, bd, e = adjacency(ctx, L, [[0, 1, 2]], 0)                                 # every triangle is invalid
    assert rs.tolist() == [0] and e == 0
    rs, nb, bd, e = adjacency(ctx, L, [[2, 0, 1]], 3)
    assert rs.tolist() == [0, 2, 4, 6] and nb.tolist() == [1, 2, 0, 2, 0, 1] and bd.tolist() == [1, 1, 1] and e == 6


@pytest.mark.parametrize("nt", [682, 683, 1365, 1366])
def test_adjacency_where_the_keys_cross_a_sort_tile(ctx, L, nt):
    assert (6 * 682 <= 4096 < 6 * 683) and (6 * 1365 <= 8192 < 6 * 1366)
    assert_adjacency(ctx, L, random_triangles(300, nt, 1), 300, seed=nt)


@pytest.mark.parametrize("nv", [63, 64, 65, 255, 256, 257])
def test_adjacency_vertex_counts(ctx, L, nv):
    assert_adjacency(ctx, L, random_triangles(nv, 2 * nv, 2), nv, seed=nv)


def test_adjacency_of_fan_strip_and_disjoint_triangles(ctx, L):
    rng = np.random.default_rng(4)
    want = assert_adjacency(ctx, L, MS.fan(5000)[rng.permutation(5000)], 5002)
    assert want[0][1] == 5001                                                        # the hub's row
    assert_adjacency(ctx, L, CC.strip(5000, rng.permutation(5002)), 5002, seed=1)
    want = assert_adjacency(ctx, L, CC.disjoint(2000), 6000, seed=2)
    assert want[2].all() and (np.diff(want[0].astype(np.int64)) == 2).all()


@pytest.mark.parametrize("nv", [2, 200, 300, 70000], ids=["1 bit", "8 bits", "9 bits", "17 bits"])
def test_adjacency_index_content(ctx, L, nv):
    """invalid indices, degenerate and repeated triangles mixed in; vertex counts whose indices need 1, 8, 9 and 17 bits, so the
    sort takes 1, 3, 3 and 5 passes"""
    rng = np.random.default_rng(nv)
    tri = random_triangles(nv, 900, 3)
    tri[rng.integers(0, 900, 60), rng.integers(0, 3, 60)] = rng.choice([-1, nv, INT32_MIN, 2 ** 31 - 1], 60)
    dup = rng.integers(0, 900, 80)
    tri[dup, 1] = tri[dup, 0]                                                        # (a, a, c)
    tri[rng.integers(0, 900, 20)] = nv - 1                                           # (a, a, a)
    tri = np.concatenate([tri, tri[rng.integers(0, 900, 100)], [[nv - 1, 0, nv - 2 if nv > 2 else 1]]]).astype(np.int32)
    want = assert_adjacency(ctx, L, tri, nv, seed=7)
    assert want[2].any() or nv == 2                                                  # (two vertices: the one edge has many sides)
    assert (~CC.valid_mask(tri, nv)).sum() > 20


def test_adjacency_caps_and_absent_outputs(ctx, L):
    key = ((9, 8, 7), 5, 0.0)
    xyz, _, tri = volume_mesh(key)
    nv, want = len(xyz), adjacency_of(key)
    total = len(want[1])
    for cap in (0, total - 1, total, total + 1):
        rs, nb, bd, e = adjacency(ctx, L, tri, nv, cap=cap, seed=cap)
        assert e == total and np.array_equal(rs, want[0]) and np.array_equal(bd, want[2])
        assert len(nb) == min(cap, total) and np.array_equal(nb, want[1][:len(nb)])
    rs, nb, bd, e = adjacency(ctx, L, tri, nv, with_boundary=False)
    assert bd is None and e == total and np.array_equal(rs, want[0]) and np.array_equal(nb, want[1])


def test_adjacency_refusals_write_nothing(ctx, L):
    tri = CC.strip(10)
    e = C.c_int64(-5)
    g = Guarded(ctx, 4096, data=np.resize(tri.view(np.uint8), 4096))
    try:
        p = g.ptr
        for args in ((p, 10, 12, p + 116, None, 0, None), (p, 10, 12, p + 1024, p + 60, 60, None), (p, 10, 12, p + 1024, None, 0, p + 119),
                     (p, 10, 12, p + 1024, p + 1072, 60, None), (p, 10, 12, p + 1024, p + 2048, 60, p + 2050), (p, 10, 12, None, None, 0, None),
                     (p, 10, 12, p + 1024, None, 5, None)):
            assert ctx.lib.r3d_mesh_adjacency(ctx.handle, *args, C.byref(e)) == L.ERR_INVALID, args
        assert ctx.lib.r3d_mesh_adjacency(ctx.handle, p, (2 ** 32 + 5) // 6, 12, p + 1024, None, 0, None, C.byref(e)) == L.ERR_UNSUPPORTED
        assert e.value == -5
        g.unchanged()
    finally:
        g.free()


# ---- smoothing -------------------------------------------------------------------------------------------------------------------------
FACTORS = [0.5, -0.53, 0.0, 1.0, 1.75]


@pytest.mark.parametrize("n_factors", [0, 1, 2, 3, 20, 21])
def test_smooth_step_counts(ctx, L, n_factors):
    """both parities of the ping-pong land in the output; 0 steps copy"""
    key = ((9, 8, 7), 5, 0.0)
    xyz, _, _ = volume_mesh(key)
    rs, nb, bd = adjacency_of(key)
    factors = (FACTORS * 5)[:n_factors]
    assert_bits(smooth(ctx, L, xyz, rs, nb, bd, factors), MS.smooth(xyz, rs, nb, bd, factors))


@pytest.mark.parametrize("key", KEYS, ids=str)
@pytest.mark.parametrize("locked", ["none", "all", "boundary"])
def test_smooth_reference_meshes(ctx, L, key, locked):
    xyz, _, _ = volume_mesh(key)
    rs, nb, bd = adjacency_of(key)
    lk = {"none": None, "all": np.ones(len(xyz), np.uint8), "boundary": bd}[locked]
    want = MS.smooth(xyz, rs, nb, lk, FACTORS)
    got = smooth(ctx, L, xyz, rs, nb, lk, FACTORS)
    assert_bits(got, want)
    if locked == "all":
        assert np.array_equal(bits(got), bits(xyz))
    assert np.array_equal(bits(smooth(ctx, L, xyz, rs, nb, lk, FACTORS, seed=11)), bits(got))   # a second run: the same bits
    alone = np.diff(rs.astype(np.int64)) == 0
    assert np.array_equal(bits(got[alone]), bits(xyz[alone]))                       # isolated vertices never move


def test_smooth_special_values(ctx, L):
    """NaN, infinities, -0, subnormals and 1e30 in a few rows travel as the arithmetic says; rows that do not move keep their bits,
    NaN payloads included"""
    key = ((9, 8, 7), 5, 0.0)
    xyz, _, _ = volume_mesh(key)
    rs, nb, bd = adjacency_of(key)
    p = xyz.copy()
    rng = np.random.default_rng(6)
    special = np.array([0x7fc00001, 0xffc12345, 0x7f800000, 0xff800000, 0x80000000, 0x00000001, 0x807fffff, 0x00400000], np.uint32).view(np.float32)
    rows = rng.choice(len(p), 40, replace=False)
    p[rows[:24], rng.integers(0, 3, 24)] = np.tile(special, 3)
    p[rows[24:32]] = np.float32(1e30) * rng.choice([-1, 1], (8, 3)).astype(np.float32)
    p[rows[32:]] = special[5:8][rng.integers(0, 3, (8, 3))]                          # whole rows of subnormals
    for factors in ([0.5], [0.5, -0.53, 1.0]):
        want = MS.smooth(p, rs, nb, bd, factors)
        got = smooth(ctx, L, p, rs, nb, bd, factors)
        assert_bits(got, want)
        assert np.isnan(want).any() and np.isinf(want).any() and np.array_equal(bits(got[bd == 1]), bits(p[bd == 1]))
    assert np.array_equal(bits(smooth(ctx, L, p, rs, nb, None, [])), bits(p))       # the copy keeps every bit


def test_smooth_fan_hub_and_small_behind_large(ctx, L):
    tri = MS.fan(5000)
    rs, nb, bd = MS.adjacency(tri, 5002)
    big = MS.positions(5002, 1)
    assert_bits(smooth(ctx, L, big, rs, nb, None, [0.5, -0.53, 0.5]), MS.smooth(big, rs, nb, None, [0.5, -0.53, 0.5]))
    # the workspace has grown and holds the fan's positions: a small mesh behind it, three steps through both halves
    xyz, tri = MS.grid(5, 4)
    rs, nb, bd = MS.adjacency(tri, len(xyz))
    assert_bits(smooth(ctx, L, xyz, rs, nb, bd, FACTORS), MS.smooth(xyz, rs, nb, bd, FACTORS))
    rs1, nb1, bd1, _ = adjacency(ctx, L, tri, len(xyz))                             # ... and the adjacency behind the steps
    assert np.array_equal(rs1, rs) and np.array_equal(nb1, nb) and np.array_equal(bd1, bd)


def test_smooth_refusals_write_nothing(ctx, L):
    xyz, tri = MS.grid(5, 4)
    rs, nb, _ = MS.adjacency(tri, 20)
    g = Guarded(ctx, 4096, seed=3)
    g_rs, g_nb = Guarded(ctx, 84, data=rs, seed=1), Guarded(ctx, len(nb) * 4, data=nb, seed=2)
    f = (C.c_double * 2)(0.5, -0.53)
    bad = (C.c_double * 2)(0.5, float("inf"))
    try:
        p = g.ptr
        for args in ((p, p, 20, g_rs.ptr, g_nb.ptr, None, f, 2), (p, p + 236, 20, g_rs.ptr, g_nb.ptr, None, f, 2),
                     (p + 8, p, 20, g_rs.ptr, g_nb.ptr, None, f, 0), (p, p + 1024, 20, g_rs.ptr, g_nb.ptr, p + 1100, f, 2),
                     (p, g_rs.ptr - 200, 20, g_rs.ptr, g_nb.ptr, None, f, 2), (p, p + 1024, 20, g_rs.ptr, g_nb.ptr, None, bad, 2),
                     (p, p + 1024, 20, g_rs.ptr, g_nb.ptr, None, f, 4097), (p, p + 1024, 20, None, g_nb.ptr, None, f, 2)):
            assert ctx.lib.r3d_mesh_smooth(ctx.handle, *args) == L.ERR_INVALID, args
        for x in (g, g_rs, g_nb):
            x.unchanged()
    finally:
        for x in (g, g_rs, g_nb):
            x.free()


# ---- vertex normals --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("key", KEYS, ids=str)
def test_normals_of_the_reference_meshes(ctx, L, key):
    xyz, nrm, tri = volume_mesh(key)
    assert_bits(normals(ctx, L, xyz, tri, nrm), MS.vertex_normals(xyz, tri, nrm))
    assert_bits(normals(ctx, L, xyz, tri, None, seed=4), MS.vertex_normals(xyz, tri, None))
    rs, nb, bd = adjacency_of(key)
    moved = MS.smooth(xyz, rs, nb, bd, [0.5, -0.53] * 3)
    assert_bits(normals(ctx, L, moved, tri, nrm, seed=8), MS.vertex_normals(moved, tri, nrm))


def test_normals_of_degenerate_and_fan_meshes(ctx, L):
    p = MS.positions(50, 2)
    fb = MS.positions(50, 3, 1.0)
    flat = np.array([[0, 0, 1], [2, 2, 2], [3, 4, 3], [-1, 0, 1], [7, 8, 50]], np.int32)   # no triangle with area
    assert np.array_equal(bits(normals(ctx, L, p, flat, fb)), bits(fb)) and not normals(ctx, L, p, flat, None).any()
    assert not normals(ctx, L, p, np.zeros((0, 3), np.int32), None).any()
    tri = MS.fan(5000)
    big = MS.positions(5002, 5)
    assert_bits(normals(ctx, L, big, tri, None), MS.vertex_normals(big, tri, None))  # the hub: 5000 contributions in triangle order
    perm = np.random.default_rng(1).permutation(5000)
    assert_bits(normals(ctx, L, big, tri[perm], None), MS.vertex_normals(big, tri[perm], None))
    huge = big.copy()
    huge[:40] *= np.float32(1e30)
    huge[40:60] *= np.float32(1e-30)
    huge[60:64] = np.float32(np.inf)                                                 # inf - inf: the NaN sums fall back
    want = MS.vertex_normals(huge, tri, big)
    assert_bits(normals(ctx, L, huge, tri, big), want)


@pytest.mark.parametrize("nv,nt", [(63, 682), (64, 683), (65, 1365), (255, 1366), (256, 2730), (257, 2731), (70000, 900), (2, 9)])
def test_normals_sizes(ctx, L, nv, nt):
    """3 M crosses one and two sort tiles at 1365 / 1366 and 2730 / 2731 triangles"""
    tri = random_triangles(nv, nt, 6)
    tri[::17, 1] = -1
    tri[5::29, 2] = tri[5::29, 0]
    p = MS.positions(nv, nt)
    assert_bits(normals(ctx, L, p, tri, None, seed=nt), MS.vertex_normals(p, tri, None))


def test_normals_refusals_write_nothing(ctx, L):
    g = Guarded(ctx, 4096, seed=5)
    try:
        p = g.ptr
        for args in ((p, 20, p + 1024, 10, None, p + 200), (p, 20, p + 1024, 10, None, p + 1100), (p, 20, p + 1024, 10, p + 2048, p + 2100),
                     (p, 20, None, 10, None, p + 2048), (p, 20, p + 1024, 10, None, None), (p, -1, p + 1024, 10, None, p + 2048)):
            assert ctx.lib.r3d_mesh_vertex_normals(ctx.handle, *args) == L.ERR_INVALID, args
        g.unchanged()
    finally:
        g.free()


# ---- the pipeline ----------------------------------------------------------------------------------------------------------------------
def test_smooth_mesh_is_the_three_calls_chained(R, ctx, L):
    key = ((16, 16, 16), 85, 0.3)
    xyz, nrm, tri = volume_mesh(key)
    rs, nb, bd = adjacency_of(key)
    got_rs, got_nb, got_bd = R.mesh_adjacency(tri.astype(np.int64), len(xyz), ctx=ctx)
    assert np.array_equal(got_rs, rs) and np.array_equal(got_nb, nb) and got_bd.dtype == bool and np.array_equal(got_bd, bd.astype(bool))
    for kw in ({}, {"method": "laplacian", "iterations": 3, "lam": 0.25}, {"lock_boundary": False, "iterations": 2, "normals": nrm}):
        got = R.smooth_mesh(xyz, tri, ctx=ctx, **kw)
        args = dict({"method": "taubin", "iterations": 10, "lam": 0.5, "mu": -0.53, "lock_boundary": True, "normals": None}, **kw)
        factors = R.smooth_factors(args["method"], args["iterations"], args["lam"], args["mu"])
        moved = smooth(ctx, L, xyz, rs, nb, bd if args["lock_boundary"] else None, factors)
        assert np.array_equal(bits(got[0]), bits(moved))
        assert np.array_equal(bits(got[1]), bits(normals(ctx, L, moved, tri, args["normals"])))
        want = MS.smooth_mesh(xyz, tri, **args)
        assert_bits(got[0], want[0])
        assert_bits(got[1], want[1])
    assert_bits(R.compute_vertex_normals(xyz, tri, fallback=nrm, ctx=ctx), MS.vertex_normals(xyz, tri, nrm))
    empty = R.smooth_mesh(np.zeros((0, 3), np.float32), [], ctx=ctx)
    assert empty[0].shape == (0, 3) and empty[1].shape == (0, 3)


@pytest.mark.parametrize("key", [((16, 16, 17), 86, 0.0), ((40, 9, 5), 3, 0.2)], ids=str)
def test_extract_triangle_mesh_smooths_on_the_device(R, T, ctx, key):
    mesh = MREF.extract_mesh(MREF.random_volume(*key))
    V = uploaded(T, ctx, MREF.random_volume(*key))
    try:
        assert_mesh(V.extract_triangle_mesh(), mesh)                                  # smooth=None: today's bytes
        assert_mesh(V.extract_triangle_mesh(smooth=None), mesh)
        for smooth_arg, kw in ((("taubin", 3), {"method": "taubin", "iterations": 3}),
                               ({"method": "laplacian", "iterations": 2, "lock_boundary": False}, None)):
            kw = kw or smooth_arg
            got = V.extract_triangle_mesh(smooth=smooth_arg)
            want = R.smooth_mesh(mesh[0], mesh[2], normals=mesh[1], ctx=ctx, **kw)
            assert_mesh(got, (want[0], want[1], mesh[2]))
            assert (bits(got[0]) != bits(mesh[0])).any()
            rs, nb, bd = MS.adjacency(mesh[2], len(mesh[0]))
            assert V.last_smooth == {"vertices": len(mesh[0]), "edges": len(nb) // 2, "boundary_vertices": int(bd.sum()),
                                     "steps": len(R.smooth_factors(**{k: v for k, v in kw.items() if k != "lock_boundary"}))}
            plain = V.extract_triangle_mesh(min_component_triangles=5, with_stats=True)
            got = V.extract_triangle_mesh(min_component_triangles=5, with_stats=True, smooth=smooth_arg)
            want = R.smooth_mesh(plain[0], plain[2], normals=plain[1], ctx=ctx, **kw)
            assert_mesh(got[:3], (want[0], want[1], plain[2]))
            assert got[3] == plain[3]
        assert_mesh(V.extract_triangle_mesh(), mesh)
        for bad in ("taubin", {"iters": 3}, ("taubin", -1)):
            with pytest.raises(ValueError):
                V.extract_triangle_mesh(smooth=bad)
    finally:
        V.close()


def test_colour_volume_smoothed_end_to_end(R, T, ctx):
    import test_gpu_tsdf_color as TC
    s, rgb, ref, _ = TC.scene((33, 9, 5), 32, np.uint16, seed=TC.DIMS.index((33, 9, 5)) + 1)
    V = TC.color_volume(T, ctx, s)
    try:
        TC.integrate_rgb(ctx, V, s, rgb)
        for kw in ({}, {"keep_largest": True}):
            plain = V.extract_triangle_mesh(with_colors=True, **kw)
            got = V.extract_triangle_mesh(with_colors=True, smooth={"iterations": 2}, **kw)
            want = R.smooth_mesh(plain[0], plain[2], iterations=2, normals=plain[1], ctx=ctx)
            assert len(plain[2]) > 0
            assert_mesh(got[:3], (want[0], want[1], plain[2]))
            assert got[3].dtype == np.uint8 and np.array_equal(got[3], plain[3])
    finally:
        V.close()


def test_command_line_smooths_the_mesh(R, golden_dir, tmp_path):
    work = tmp_path / "work"
    shutil.copytree(os.path.join(golden_dir, "scene3", "depth"), work / "depth")
    shutil.copytree(os.path.join(golden_dir, "scene3", "camera_pose"), work / "camera_pose")
    tool = os.path.join(ROOT, PKG, "other_tools", "integrate_tsdf.py")
    args = ["--voxel-size", "8", "--trunc", "24", "--origin", "-300", "-300", "-300", "--dims", "75", "75", "75", "--min-weight", "1"]
    env = dict(os.environ, PYTHONPATH=ROOT, R3D_FX="20", R3D_FY="20", R3D_CX="15.5", R3D_CY="11.5")
    script = ("import runpy, shutil, sys\n"
              "tool, base = sys.argv[1], sys.argv[2:]\n"
              "for extra, keep in ((['--mesh'], 'plain.ply'), (['--mesh', '--mesh-smooth', 'taubin,5'], 'smooth.ply')):\n"
              "    sys.argv = [tool] + base + extra\n"
              "    runpy.run_path(tool, run_name='__main__')\n"
              "    shutil.copy('./ply/tsdf_mesh.ply', keep)\n")
    r = subprocess.run([sys.executable, "-c", script, tool] + args, cwd=str(work), env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-1000:] + r.stderr[-2000:]
    plain, got = R.cloud_io.read_ply_mesh(str(work / "plain.ply")), R.cloud_io.read_ply_mesh(str(work / "smooth.ply"))
    assert len(got[0]) == len(plain[0]) and np.array_equal(got[2], plain[2]) and len(plain[2]) > 1000
    assert (bits(got[0]) != bits(plain[0])).any()
    want = MS.smooth_mesh(plain[0], plain[2], "taubin", 5, normals=plain[1])
    assert_bits(got[0], want[0])
    assert_bits(got[1], want[1])
    rs, nb, bd = MS.adjacency(plain[2], len(plain[0]))
    lines = [l for l in r.stdout.split("\n") if l.startswith("smoothed")]
    assert lines == ["smoothed vertices %d edges %d boundary %d steps 10" % (len(plain[0]), len(nb) // 2, int(bd.sum()))]
