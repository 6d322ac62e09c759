"""CPU: the evaluation restatement (tests/compare_ref.py) on the cases the GPU tests use -- their conditions are asserted here
first --, against an INDEPENDENT fp64 formulation of the point-to-triangle distance, on the analytic room box, and what the Python
layer and the tool do without a GPU."""
import importlib
import json
import math
import os

import numpy as np
import pytest

import compare_ref as CR
from helpers import PKG, ROOT
from test_mesh_cc_host import VOLUMES, volume_mesh

INT32_MAX = 2 ** 31 - 1
KEY_SMALL, KEY_BIG = ((9, 8, 7), 5, 0.0), ((16, 16, 17), 86, 0.0)
TRIANGLE_SIZES = (1, 31, 32, 33, 1023, 1025, 3000)      # group (32) and 1024 boundaries, and ~3000: 94 groups
POINT_SIZES = (1, 63, 64, 65, 257, 2000)                # wave (64) and workgroup (256) boundaries


def syn():
    return importlib.import_module(PKG + ".synthetic")


def room_box():
    """The room of synthetic.py as 8 vertices and 12 triangles, wound so that the face normals point OUT of the room"""
    lo, hi = syn().ROOM_LO, syn().ROOM_HI
    v = np.array([[(lo, hi)[i][0], (lo, hi)[j][1], (lo, hi)[k][2]] for i in (0, 1) for j in (0, 1) for k in (0, 1)], np.float32)
    # vertex number = 4 i + 2 j + k
    quads = [(0, 1, 3, 2), (4, 6, 7, 5), (0, 4, 5, 1), (2, 3, 7, 6), (0, 2, 6, 4), (1, 5, 7, 3)]   # -x +x -y +y -z +z
    tri = np.array([t for a, b, c, d in quads for t in ((a, b, c), (a, c, d))], np.int32)
    return v, tri


def grid_mesh(nx=9, ny=7):
    """unit squares in the plane z = 0, two triangles each: integer coordinates, so distances from lattice points are exact"""
    xs, ys = np.meshgrid(np.arange(nx + 1), np.arange(ny + 1), indexing="ij")
    v = np.stack([xs.ravel(), ys.ravel(), np.zeros(xs.size)], axis=1).astype(np.float32)
    idx = lambda i, j: i * (ny + 1) + j
    tri = [t for i in range(nx) for j in range(ny)
           for t in ((idx(i, j), idx(i + 1, j), idx(i + 1, j + 1)), (idx(i, j), idx(i + 1, j + 1), idx(i, j + 1)))]
    return v, np.array(tri, np.int32)


def grid_points():
    """above, below and beside the grid, on lattice points and cell centres: every distance is shared by several triangles"""
    p = [(i, j, h) for i in range(0, 10, 3) for j in range(0, 8, 2) for h in (0.0, 2.0, -3.0)]
    p += [(i + 0.5, j + 0.5, 1.0) for i in range(3) for j in range(3)]
    p += [(-2.0, 3.0, 0.0), (12.0, 7.0, 4.0), (4.0, -1.0, 0.0), (4.5, 3.0, 0.0)]
    return np.array(p, np.float32)


def degenerate_mesh():
    """zero-area triangles of every kind, small integers so that every product is exact; one proper triangle listed twice"""
    v = np.array([[0, 0, 0], [4, 0, 0], [0, 4, 0], [2, 0, 0], [4, 0, 0], [1, 1, 1], [2, 2, 2], [3, 3, 3], [8, 8, 8], [0, 0, 5],
                  [4, 0, 5], [0, 4, 5]], np.float32)
    tri = np.array([[0, 0, 1],      # repeated index: the segment 0-1
                    [5, 5, 5],      # one index three times: a point
                    [1, 4, 2],      # coincident vertices under different indices: the segment 1-2
                    [1, 4, 4],      # ... a point
                    [0, 3, 1],      # collinear, the middle vertex second
                    [5, 7, 6],      # collinear on a skew line, the middle vertex last
                    [3, 0, 1],      # collinear, the middle vertex first
                    [9, 10, 11], [9, 10, 11],   # listed twice
                    [8, 8, 8]], np.int32)
    return v, tri


def degenerate_points():
    p = [(2, 0, 0), (2, 3, 0), (-1, -1, 0), (5, 0, 0), (1, 1, 1), (2, 2, 2), (2.5, 2.5, 2.5), (4, 4, 4), (8, 8, 9), (1, 1, 5), (1, 1, 7),
         (2, 2, 5), (0, 2, 0), (3, 1, 0), (2, 0, 3), (10, 10, 10), (1, 2, 3)]
    return np.array(p, np.float32)


def edge_mesh():
    """two coplanar triangles sharing the edge (0,0,0)-(2,2,0), and a third folded up along the same edge"""
    v = np.array([[0, 0, 0], [2, 0, 0], [2, 2, 0], [0, 2, 0], [0, 0, 2]], np.float32)
    return v, np.array([[0, 1, 2], [0, 2, 3], [2, 0, 4]], np.int32)


def edge_points():
    p = [(1, 1, 0), (0.5, 0.5, 0), (2, 2, 0), (0, 0, 0), (3, 3, 0), (-1, -1, 0), (1, 0.5, 0), (0.5, 1, 0), (5, 1, 0), (-3, 1, 0),
         (1, 1, 1), (1, 1, -1), (0.25, 0.25, 0.5)]
    return np.array(p, np.float32)


def invalid_mesh():
    """invalid indices and non-finite vertices between valid triangles"""
    v = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0], [np.nan, 0, 0], [0, np.inf, 0], [0, 0, 1], [5, 5, 5], [-np.inf, 0, 0]], np.float32)
    tri = np.array([[0, 1, -1], [0, 1, 8], [0, 1, INT32_MAX], [0, 1, 3], [4, 1, 2], [0, 1, 2], [-2 ** 31, 0, 1], [7, 7, 7], [0, 1, 5],
                    [6, 6, 6]], np.int32)
    return v, tri


def invalid_points():
    return np.array([[0.25, 0.25, -1], [np.nan, 0, 0], [0, np.inf, 0], [0, 0, -np.inf], [5, 5, 6], [0.5, -1, 0.5], [np.nan, np.nan, np.nan]],
                    np.float32)


def extreme_mesh():
    """coordinates of 1e30 and subnormal ones"""
    s = np.float32(1e-42)
    v = np.array([[1e30, 0, 0], [0, 1e30, 0], [0, 0, 1e30], [-1e30, -1e30, -1e30], [0, 0, 0], [s, 0, 0], [0, s, 0], [s, s, s],
                  [3 * s, 0, 0]], np.float32)
    return v, np.array([[0, 1, 2], [3, 0, 1], [4, 5, 6], [5, 6, 7], [4, 5, 8]], np.int32)


def extreme_points():
    s = np.float32(1e-42)
    return np.array([[0, 0, 0], [1e30, 1e30, 1e30], [s, s, 0], [2 * s, 0, 0], [-1e30, 0, 5e29], [3e38, 3e38, -3e38], [s / 4, s / 4, 5 * s],
                     [1, 1, 1]], np.float32)


def volume_case(key, n_triangles=None):
    xyz, _, tri = volume_mesh(key)
    return xyz, (tri if n_triangles is None else tri[:n_triangles])


def own_vertices(v, tri, n, seed=0):
    """n of the vertices the triangles name (all of them in order when there are fewer)"""
    named = np.unique(tri)
    if len(named) > n:
        named = np.sort(np.random.default_rng(seed).choice(named, n, replace=False))
    return v[named]


def jittered(points, scale, seed=1):
    rng = np.random.default_rng(seed)
    return (points.astype(np.float64) + rng.normal(size=points.shape) * scale).astype(np.float32)


def far_points(v, n, seed=2):
    rng = np.random.default_rng(seed)
    c, ext = v.mean(axis=0), np.ptp(v, axis=0).max()
    d = rng.normal(size=(n, 3))
    return (c + d / np.linalg.norm(d, axis=1, keepdims=True) * ext * rng.uniform(3, 50, size=(n, 1))).astype(np.float32)


HAND_CASES = {"grid": (grid_points, grid_mesh), "degenerate": (degenerate_points, degenerate_mesh), "edges": (edge_points, edge_mesh),
              "invalid": (invalid_points, invalid_mesh), "extreme": (extreme_points, extreme_mesh)}


def hand_case(name):
    pts, mesh = HAND_CASES[name]
    v, tri = mesh()
    return pts(), v, tri


# ---- the independent formulation: plane distance inside, clamped segments outside ----------------------------------------------
def _seg_d2(p, a, b):
    e = b - a
    ee = (e * e).sum(-1)
    with np.errstate(all="ignore"):
        t = np.where(ee > 0, ((p - a) * e).sum(-1) / np.where(ee > 0, ee, 1.0), 0.0)
    t = np.clip(t, 0.0, 1.0)
    d = p - (a + t[..., None] * e)
    return (d * d).sum(-1)


def independent_d2(points, v, tri):
    """[P, M] float64: the distance to the triangle's plane where the projection's barycentric coordinates are all in [0, 1],
    otherwise the minimum over the three edges as clamped segments"""
    p = np.asarray(points, np.float64)[:, None, :]
    t = v[tri].astype(np.float64)
    a, b, c = t[None, :, 0], t[None, :, 1], t[None, :, 2]
    n = np.cross(b - a, c - a)
    nn = (n * n).sum(-1)
    ap = p - a
    with np.errstate(all="ignore"):
        safe = np.where(nn > 0, nn, 1.0)
        bw = (np.cross(b - a, ap) * n).sum(-1) / safe           # weight of c
        bv = (np.cross(ap, c - a) * n).sum(-1) / safe           # weight of b
        bu = 1.0 - bv - bw
        plane = (ap * n).sum(-1) ** 2 / safe
    inside = (nn > 0) & (bu >= 0) & (bu <= 1) & (bv >= 0) & (bv <= 1) & (bw >= 0) & (bw <= 1)
    edges = np.minimum(np.minimum(_seg_d2(p, a, b), _seg_d2(p, b, c)), _seg_d2(p, c, a))
    return np.where(inside, plane, edges)


def check_against_independent(points, v, tri):
    ok = CR.valid_triangles(v, tri)
    fin = np.isfinite(points.astype(np.float64)).all(axis=1)
    pts, t = points[fin], np.asarray(tri)[ok]
    if len(pts) == 0 or len(t) == 0:
        return
    both = np.concatenate([pts.astype(np.float64), v[np.unique(t)].astype(np.float64)])
    diag2 = float(((both.max(axis=0) - both.min(axis=0)) ** 2).sum())
    tol = 1e-13 * diag2
    got = CR.all_d2(pts, v, t)
    want = independent_d2(pts, v, t)
    assert np.isfinite(got).all()
    assert np.abs(got - want).max() <= tol, (np.abs(got - want).max(), tol)
    # the winner agrees wherever the runner-up is farther than the margin
    _, win, _ = CR.mesh_distance(pts, v, t)
    order = np.sort(want, axis=1)
    clear = np.ones(len(pts), bool) if want.shape[1] == 1 else order[:, 1] - order[:, 0] > 2 * tol
    assert np.array_equal(win[clear], np.argmin(want, axis=1)[clear].astype(np.uint32))


# ---- the cases' own conditions -------------------------------------------------------------------------------------------------
def test_conditions_of_the_hand_made_cases():
    pts, v, tri = hand_case("grid")
    d2 = CR.all_d2(pts, v, tri)
    ties = (d2 == d2.min(axis=1, keepdims=True)).sum(axis=1)
    assert (ties >= 2).sum() >= 40 and ties.max() >= 6          # exact ties, up to the six triangles round a lattice point
    dist, win, _ = CR.mesh_distance(pts, v, tri)
    assert np.array_equal(win, np.argmax(d2 == d2.min(axis=1, keepdims=True), axis=1))       # the lowest index among them
    assert np.array_equal(dist[:3], np.array([0.0, 2.0, 3.0], np.float32))

    pts, v, tri = hand_case("degenerate")
    t = v[tri].astype(np.float64)
    area = np.cross(t[:, 1] - t[:, 0], t[:, 2] - t[:, 0])
    assert (area[[0, 1, 2, 3, 4, 5, 6, 9]] == 0).all() and (area[[7, 8]] != 0).any(axis=1).all()   # zero area, exactly
    assert np.array_equal(tri[7], tri[8])
    d2 = CR.all_d2(pts, v, tri)
    assert np.isfinite(d2).all()                                  # no NaN from a zero denominator
    assert np.array_equal(d2[:, 7], d2[:, 8])
    dist, win, q = CR.mesh_distance(pts, v, tri)
    assert dist[0] == 0 and win[0] == 0                           # (2,0,0) lies on the segments of triangles 0, 4, 6: the lowest wins
    assert win[9] == 7 and dist[9] == 0 and win[10] == 7 and dist[10] == 2    # the twice-listed triangle: the first copy
    assert win[4] == 1 and dist[4] == 0                           # the point triangle (5,5,5) at (1,1,1)
    assert np.array_equal(q[6], np.array([2.5, 2.5, 2.5], np.float32)) and win[6] == 5    # inside the skew collinear triangle

    pts, v, tri = hand_case("edges")
    d2 = CR.all_d2(pts, v, tri)
    assert (d2[:5] == d2[:5, :1]).all()                           # on the shared edge (or beyond its ends): all three tie exactly
    assert (pts[:10, 2] == 0).all() and (d2[:10, :2].min(axis=1) == 0).sum() == 6    # in the plane of the two coplanar triangles:
    #                                                               six of the ten inside one of them, four beside them
    assert np.array_equal(CR.mesh_distance(pts, v, tri)[1][:5], np.zeros(5, np.uint32))

    pts, v, tri = hand_case("invalid")
    assert CR.valid_triangles(v, tri).tolist() == [False, False, False, False, False, True, False, False, True, True]
    dist, win, q = CR.mesh_distance(pts, v, tri)
    assert win.tolist() == [5, CR.NO_TRIANGLE, CR.NO_TRIANGLE, CR.NO_TRIANGLE, 9, 8, CR.NO_TRIANGLE]
    assert np.isinf(dist[[1, 2, 3, 6]]).all() and np.isnan(q[[1, 2, 3, 6]]).all() and dist[4] == 1
    none = CR.mesh_distance(pts, v, tri[:5])
    assert np.isinf(none[0]).all() and (none[1] == CR.NO_TRIANGLE).all() and np.isnan(none[2]).all()

    pts, v, tri = hand_case("extreme")
    dist, win, q = CR.mesh_distance(pts, v, tri)
    assert np.isfinite(CR.all_d2(pts, v, tri)).all() and (win != CR.NO_TRIANGLE).all()
    assert (v[5:] != 0).any() and (np.abs(v[5:]) < np.finfo(np.float32).tiny).all()          # subnormal coordinates
    assert dist[0] == 0 and win[0] == 2 and np.isinf(dist[5])     # 3e38 away: d2 is finite in fp64, its root is not an f32


@pytest.mark.parametrize("name", list(HAND_CASES))
def test_restatement_against_the_independent_form_by_hand(name):
    check_against_independent(*hand_case(name))


@pytest.mark.parametrize("key", [KEY_SMALL, "sphere"])
def test_restatement_against_the_independent_form_on_marching_cubes(key):
    v, tri = volume_case(key)
    own = own_vertices(v, tri, 257)
    dist, win, q = CR.mesh_distance(own, v, tri)
    assert (dist == 0).all() and np.array_equal(q, own)          # a mesh queried with its own vertices
    first = np.array([np.flatnonzero((v[tri] == p).all(axis=2).any(axis=1))[0] for p in own])
    assert np.array_equal(win, first.astype(np.uint32))           # ... ties between all triangles at the vertex: the lowest index
    pts = np.concatenate([own[:65], jittered(own[:129], 0.3), far_points(v, 33)])
    check_against_independent(pts, v, tri)


def test_big_marching_cubes_mesh_has_the_sizes_the_gpu_tests_cut():
    v, tri = volume_case(KEY_BIG)
    assert len(tri) >= max(TRIANGLE_SIZES) and len(volume_case(KEY_SMALL)[1]) >= 1025
    assert len(np.unique(tri[:3000])) >= 1500


def test_room_box_at_known_distances():
    v, tri = room_box()
    t = v[tri].astype(np.float64)
    n = np.cross(t[:, 1] - t[:, 0], t[:, 2] - t[:, 0])
    centre = t.mean(axis=1)
    assert ((n * centre).sum(axis=1) > 0).all()                   # outward normals (the room is centred on the origin)
    pts = np.array([[0, 0, 0], [3, 0, 0], [0, 1, 2.5], [5, 0, 0], [5, 2.5, 4], [0, -2, 0], [4, 1.5, 3], [-4, 0, 0], [3.5, 1.25, 2.75]],
                   np.float32)
    want = np.array([1.5, 1.0, 0.5, 1.0, math.sqrt(3.0), 0.5, 0.0, 0.0, 0.25])
    dist, win, q = CR.mesh_distance(pts, v, tri)
    assert np.array_equal(dist, want.astype(np.float32))
    signed = CR.mesh_distance(pts, v, tri, signed=True)[0]
    inside = np.array([1, 1, 1, 0, 0, 0, 0, 0, 1], bool)
    assert np.array_equal(np.abs(signed), dist) and (signed[inside] < 0).all() and (signed[~inside] >= 0).all()
    assert not np.signbit(signed[[6, 7]]).any()                   # distance 0: the sign is +
    check_against_independent(pts, v, tri)


# ---- statistics, root, colours ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [0, 1, 255, 256, 257, 65537])
def test_fixed_order_sum_is_a_sum(n):
    x = np.random.default_rng(n).uniform(0, 3, size=n).astype(np.float32).astype(np.float64)
    s = CR.fixed_order_sum(x)
    assert abs(s - math.fsum(x)) <= 2.0 ** -50 * max(n, 1) * 3 and (n > 0 or s == 0.0)
    stats, counts, hist = CR.distance_stats(x.astype(np.float32), thresholds=(1.0, 5.0), bin_width=0.5, n_bins=4)
    assert stats[0] == n and stats[1] == 0 and counts[1] == n and hist.sum() == n
    if n:
        assert stats[4] == x.min() and stats[5] == x.max() and hist[3] == np.count_nonzero(x >= 1.5)
    else:
        assert stats[4] == np.inf and stats[5] == -np.inf


def test_stats_edges_by_hand():
    d = np.array([0.0, 0.5, 1.0, 1.5, 2.0, 7.0, np.nan, np.inf, -np.inf, -0.0, 0.25, -1.0], np.float32)
    stats, counts, hist = CR.distance_stats(d, thresholds=(0.5, 1.0, -5.0, 100.0), bin_width=0.5, n_bins=4)
    assert stats[:2].tolist() == [9.0, 3.0] and stats[2] == 11.25 and stats[4] == -1.0 and stats[5] == 7.0
    assert counts.tolist() == [5, 6, 0, 9]                        # a threshold equal to a value counts it
    assert hist.tolist() == [4, 1, 1, 3]                          # values on bin edges go up, the last bin is open, negatives in bin 0
    sq = CR.distance_stats(np.array([4.0, 9.0, -1.0, 0.0], np.float32), squared=True)[0]
    assert sq.tolist() == [3.0, 1.0, 5.0, 13.0, 0.0, 3.0]
    only_bad = CR.distance_stats(np.array([np.nan, np.inf], np.float32), thresholds=(1.0,), bin_width=1.0, n_bins=2)
    assert only_bad[0].tolist() == [0.0, 2.0, 0.0, 0.0, np.inf, -np.inf] and only_bad[1].tolist() == [0] and only_bad[2].tolist() == [0, 0]
    zero = CR.distance_stats(np.array([-0.0], np.float32))[0]
    assert not np.signbit(zero[4]) and not np.signbit(zero[5])    # a zero is reported as +0


def binade_edges():
    """every f32 binade edge with its neighbours, subnormals, 0 and +inf"""
    e = np.arange(1, 255, dtype=np.uint32) << 23
    bits = np.concatenate([e, e - 1, e + 1, np.array([0, 1, 2, 3, 0x7FFFFF, 0x7F7FFFFF, 0x7F800000, 0x80000000], np.uint32)])
    return bits.view(np.float32)


def test_root_is_the_correctly_rounded_f32_root():
    x = binade_edges()
    got = CR.sqrt_f32(x)
    assert np.array_equal(got.view(np.uint32), np.sqrt(x).view(np.uint32))       # NumPy's float32 root is correctly rounded
    assert np.signbit(got[-1]) and got[-1] == 0


def test_colour_ramp_by_hand():
    d = np.array([0.0, 1.0, -1.0, 2.0, 3.0, 9.0, np.nan, np.inf, 0.5, 1.0 / 3.0], np.float32)
    w = CR.distance_colors(d, 3.0)
    rgb = np.stack([w & 255, (w >> 8) & 255, (w >> 16) & 255], axis=1).tolist()
    assert rgb[0] == [0, 0, 255] and rgb[1] == [0, 255, 0] and rgb[2] == [0, 255, 0] and rgb[3] == [255, 255, 0]
    assert rgb[4] == [255, 0, 0] and rgb[5] == [255, 0, 0] and rgb[6] == [128, 128, 128] and rgb[7] == [128, 128, 128]
    assert rgb[8] == [0, 127, 128] and (w >> 24 == 0).all()


# ---- the Python layer without a GPU ---------------------------------------------------------------------------------------------
def test_report_formulas_on_hand_made_distances():
    E = importlib.import_module(PKG + ".evaluation")
    acc = np.array([0.0, 0.1, 0.2, 0.4, np.nan], np.float32)
    com = np.array([0.05, 0.3, 0.3], np.float32)
    thr = 0.25
    sides = []
    for d in (acc, com):
        stats, counts, hist = CR.distance_stats(d, thresholds=(thr,))
        st = E.stats_dict(stats, counts, hist)
        sides.append(E.directed_numbers(st, int(st["counts"][0])))
        ref = CR.side_numbers(stats, int(counts[0]))
        assert sides[-1] == ref
    out = E.combine(sides[0], sides[1], thr)
    assert out["accuracy"]["n"] == 4 and out["completeness"]["n"] == 3
    assert out["precision"] == 0.75 and out["recall"] == 1.0 / 3.0
    assert out["f_score"] == CR.f_score(0.75, 1.0 / 3.0) == 2 * 0.75 / 3.0 / (0.75 + 1.0 / 3.0)
    a64, c64 = acc[:4].astype(np.float64), com.astype(np.float64)
    assert abs(out["chamfer"] - (a64.mean() + c64.mean())) <= 1e-15
    assert abs(out["accuracy"]["rms"] - math.sqrt((a64 ** 2).mean())) <= 1e-15 and out["accuracy"]["max"] == float(acc[3])
    st = E.stats_dict(*CR.distance_stats(acc))
    assert abs(st["std"] - a64.std()) <= 1e-15 and st["n_nonfinite"] == 1
    empty = E.stats_dict(*CR.distance_stats(np.zeros(0, np.float32)))
    assert empty["n"] == 0 and math.isnan(empty["mean"]) and math.isnan(empty["rms"])
    nothing = E.directed_numbers(empty, 0)
    assert math.isnan(nothing["within"]) and E.combine(nothing, nothing, 1.0)["f_score"] == 0.0


def test_python_layer_checks_its_arguments_and_has_no_cpu_path():
    r3d = importlib.import_module(PKG)
    E = importlib.import_module(PKG + ".evaluation")
    for name in ("MeshIndex", "cloud_to_cloud_distance", "cloud_to_mesh_distance", "distance_stats", "distance_colors",
                 "evaluate_reconstruction", "cloud_to_cloud_distance_device", "distance_stats_device", "distance_colors_device"):
        assert getattr(r3d, name) is getattr(E, name)
    with pytest.raises(ValueError):
        E.cloud_to_mesh_distance(np.zeros((2, 2)), np.zeros((3, 3)), np.zeros((1, 3), np.int32))
    with pytest.raises(ValueError):
        E.cloud_to_mesh_distance(np.zeros((2, 3)), np.zeros((3, 3)), np.zeros((1, 3), np.float32))
    with pytest.raises(ValueError):
        E.evaluate_reconstruction(np.zeros((2, 3)), np.zeros((2, 3)), -1.0)
    with pytest.raises(ValueError):
        E.cloud_to_cloud_distance(np.zeros((2, 3)), np.zeros((0, 3)))
    side = E._side((np.zeros((4, 3)), np.zeros((2, 3), np.int64)), "x")
    assert side[0].dtype == np.float32 and side[1].dtype == np.int32 and E._side(np.zeros((4, 3)), "x")[1] is None
    L = importlib.import_module(PKG + "._lib")
    n = importlib.import_module("ctypes").c_int(-1)
    if L.load().r3d_device_count(n) == 0 and n.value > 0:
        return                                                    # a GPU is visible: the no-device behaviour is covered on the CPU box
    with pytest.raises(r3d.R3DError):
        E.distance_stats(np.zeros(3, np.float32))


def test_tool_arguments_and_file_kinds(tmp_path):
    tool = importlib.import_module(PKG + ".other_tools.compare_clouds")
    IO = importlib.import_module(PKG + ".cloud_io")
    v, tri = room_box()
    mesh, cloud, binary, txt, empty = (str(tmp_path / n) for n in ("m.ply", "c.ply", "b.ply", "c.txt", "e.ply"))
    IO.write_ply_mesh(mesh, v, np.zeros_like(v), tri)
    IO.write_ply_mesh(empty, v, np.zeros_like(v), np.zeros((0, 3), np.int32))
    IO.write_ply(cloud, v)
    IO.write_ply_binary(binary, v)
    IO.write_xyz_txt(txt, v)
    assert [tool.file_kind(p) for p in (mesh, cloud, binary, txt, empty)] == ["ply_mesh", "ply", "ply", "txt", "ply"]
    r3d = importlib.import_module(PKG)
    got = tool.load(r3d, mesh)
    assert isinstance(got, tuple) and np.array_equal(got[0], v) and np.array_equal(got[1], tri)
    for p in (cloud, binary, txt):
        assert np.array_equal(tool.load(r3d, p), v.astype(np.float64))
    a = tool.parse_args([mesh, txt, "--threshold", "0.5", "--hist", "16,0.25", "--ply", "out.ply"])
    assert a.threshold == 0.5 and a.hist == (16, 0.25) and a.ply_max == 0.5 and not a.signed
    a = tool.parse_args([mesh, txt, "--threshold", "0.5", "--signed", "--ply", "o.ply", "--ply-max", "2"])
    assert a.signed and a.ply_max == 2.0 and a.hist is None
    for bad in ([mesh, txt], [mesh, txt, "--threshold", "-1"], [mesh, txt, "--threshold", "1", "--hist", "0,1"],
                [mesh, txt, "--threshold", "1", "--hist", "4"], [mesh, txt, "--threshold", "1", "--ply-max", "2"],
                [mesh, str(tmp_path / "missing.ply"), "--threshold", "1"], [mesh, txt, "--threshold", "0", "--ply", "o.ply"]):
        with pytest.raises(SystemExit):
            tool.parse_args(bad)


def test_header_and_documents_state_the_definition():
    text = open(os.path.join(ROOT, "include", "r3d.h")).read()
    for s in ("vc = d1*d4 - d3*d2", "LOWEST triangle index", "not an angle-weighted pseudonormal", "None of these kernels has been timed"):
        assert s in text, s
    assert "#define R3D_MESHDIST_SIGNED 1" in text and "#define R3D_VERSION 200" in text
    for doc in ("README.md", "DESIGN.md", "INTEGRATION.md"):
        assert "compare_clouds" in open(os.path.join(ROOT, doc)).read(), doc
    assert "4.5w Reconstruction evaluation" in open(os.path.join(ROOT, "DESIGN.md")).read()


def test_room_reconstruction_meets_the_median_bound_on_the_cpu():
    """The end-to-end bound of tests/test_gpu_compare.py, checked with the restatement alone: the marching-cubes mesh of the
    reference TSDF of tsdf_ref.room_scene() (0.2 m voxels) against the true room box -- the median accuracy distance is at most
    one voxel size."""
    import mesh_ref as MREF
    import tsdf_ref as REF
    s = REF.room_scene()
    xyz, _, tri = MREF.extract_mesh(REF.run(s)[0])
    v, box = room_box()
    dist = CR.mesh_distance(xyz, v, box)[0]
    med = float(np.median(dist))
    print("median accuracy distance %.4f m, max %.4f m, voxel %.2f m, %d vertices" % (med, dist.max(), s["vs"], len(xyz)))
    assert len(xyz) > 1000 and med <= s["vs"]
