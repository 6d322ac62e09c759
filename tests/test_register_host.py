"""CPU: global registration without a GPU -- argument validation of every entry of registration.py, and the properties of the
NumPy restatement (tests/register_ref.py) the GPU tests compare the kernels with."""
import importlib
import os
import re

import numpy as np
import pytest

import register_ref as REF
from helpers import PKG, ROOT


@pytest.fixture(scope="module")
def G():
    return importlib.import_module(PKG + ".registration")


def knn_lists(xyz, k):
    """Exact (d2, j) lists in the library's f32 expression, brute force: the host stand-in for r3d_nn_index_knn_self."""
    xyz = np.ascontiguousarray(xyz, np.float32)
    n = xyz.shape[0]
    d = [xyz[:, a][:, None] - xyz[:, a][None, :] for a in range(3)]
    d2 = (d[0].astype(np.float64) * d[0] + d[1].astype(np.float64) * d[1]).astype(np.float32)   # fmaf(dy,dy, dx*dx) has one rounding
    d2 = (d[2].astype(np.float64) * d[2] + d2.astype(np.float64)).astype(np.float32)
    d2[np.arange(n), np.arange(n)] = np.inf
    d2[~np.isfinite(d2)] = np.inf
    order = np.lexsort((np.broadcast_to(np.arange(n), (n, n)), d2), axis=1)[:, :k]
    dd = np.take_along_axis(d2, order, axis=1)
    idx = np.where(np.isfinite(dd), order, 0xffffffff).astype(np.uint32)
    if idx.shape[1] < k:
        idx = np.concatenate([idx, np.full((n, k - idx.shape[1]), 0xffffffff, np.uint32)], axis=1)
        dd = np.concatenate([dd, np.full((n, k - dd.shape[1]), np.inf, np.float32)], axis=1)
    return idx, dd.astype(np.float32)


def test_header_constants_are_the_restatements():
    text = open(os.path.join(ROOT, "include", "r3d.h")).read()
    for name, want in (("COS", REF.THETA_COS), ("SIN", REF.THETA_SIN)):
        body = re.search(r"#define R3D_FPFH_THETA_%s \\\n\s*\{([^}]*)\}" % name, text).group(1)
        got = np.array([float(v.strip().rstrip("f")) for v in body.split(",")], dtype=np.float32)
        assert np.array_equal(got, want)
    m = np.arange(1, 11)
    beta = -np.pi + 2 * np.pi * m / 11
    assert np.array_equal(REF.THETA_COS, np.cos(beta).astype(np.float32))
    assert np.array_equal(REF.THETA_SIN, np.sin(beta).astype(np.float32))
    assert "#define R3D_FPFH_DIM 33" in text and "#define R3D_REGISTER_RESULT_DOUBLES 32" in text


def test_theta_sectors_agree_with_arctan2():
    rng = np.random.default_rng(0)
    ang = rng.uniform(-np.pi, np.pi, 100_000)
    r = rng.uniform(0.1, 2.0, ang.size)
    x, y = (r * np.cos(ang)).astype(np.float32), (r * np.sin(ang)).astype(np.float32)
    th = np.arctan2(y.astype(np.float64), x.astype(np.float64))
    pos = (th + np.pi) / (2 * np.pi) * 11
    near = np.abs(pos - np.round(pos)) * (2 * np.pi / 11) <= 1e-6
    want = np.clip(np.floor(pos).astype(np.int64), 0, 10)
    got = REF.theta_bin(x, y)
    assert near.sum() < 20 and np.array_equal(got[~near], want[~near])
    assert got.min() == 0 and got.max() == 10
    # the axes: +x is bin 5, +y bin 8, -x (from above) bin 10, -y bin 2
    assert REF.theta_bin(np.float32([1, 0, -1, 0]), np.float32([0, 1, 0, -1])).tolist() == [5, 8, 10, 2]


def test_value_bins():
    f = np.float32([-1.0, -0.82, -0.8181, 0.0, 0.9999, 1.0, 1.5, -2.0])
    assert REF.bin11(f).tolist() == [0, 0, 1, 5, 10, 10, 10, 0]


def test_fpfh_rows_sum_to_200_per_sub_histogram():
    xyz, nrm = REF.cube(600, 1), REF.unit_normals(600, 2)
    nrm[::17] = 0
    idx, d2 = knn_lists(xyz, 8)
    f, s, c = REF.fpfh(xyz, nrm, idx, d2)
    assert s.dtype == np.uint8 and s.max() <= 8
    assert np.array_equal(s.reshape(-1, 3, 11).sum(axis=2), np.repeat(c[:, None], 3, axis=1))
    assert (c[::17] == 0).all() and (c > 0).sum() > 500
    sums = f.reshape(-1, 3, 11).sum(axis=2, dtype=np.float64)
    own = (c > 0)
    mem = REF.members(idx, d2, None)
    fed = (mem & (c[np.where(mem, idx, 0)] > 0) & (d2 > 0)).any(axis=1)
    assert np.abs(sums[own & fed] - 200.0).max() <= 200 * 40 * 2.0 ** -24        # ~40 f32 roundings per sum
    assert np.abs(sums[own & ~fed] - 100.0).max(initial=0) <= 100 * 20 * 2.0 ** -24
    assert np.abs(sums[~own & fed] - 100.0).max(initial=0) <= 100 * 40 * 2.0 ** -24
    # a radius cuts the lists
    f2, s2, c2 = REF.fpfh(xyz, nrm, idx, d2, radius=0.08)
    assert (c2 <= c).all() and (c2 < c).any()


def test_pose_from_three_exact_correspondences():
    rng = np.random.default_rng(3)
    for trial in range(20):
        T = REF.rigid(rng.uniform(90, 180), rng.normal(size=3), rng.uniform(-5, 5, 3))
        p = rng.uniform(-2, 2, (3, 3))
        q = p @ T[:3, :3].T + T[:3, 3]
        R, t, ok = REF.pose_from_pairs(p, q, 1e-9)
        assert ok and np.abs(R - T[:3, :3]).max() <= 1e-12 and np.abs(t - T[:3, 3]).max() <= 1e-12
    # collinear, repeated and stretched triples are no hypothesis
    line = np.outer([0.0, 1.0, 2.0], [1.0, 2.0, -1.0])
    assert not REF.pose_from_pairs(line, line, 0.1)[2]
    assert not REF.pose_from_pairs(p[[0, 0, 1]], q[[0, 0, 1]], 0.1)[2]
    assert not REF.pose_from_pairs(p, q * 1.5, 0.01)[2]
    assert REF.pose_from_pairs(p, q + rng.normal(size=(3, 3)) * 1e-3, 0.01)[2]


def test_sampler_agrees_with_the_library(G):
    S = importlib.import_module(PKG + ".segmentation")
    for seed in (0, 1, 2 ** 64 - 1):
        for h in (0, 1, 65535):
            for n in (3, 1000, 2 ** 32 - 1):
                assert REF.rows_of(seed, h, n) == S.ransac_rows(seed, h, n)


def test_device_order_sum_is_a_sum():
    rng = np.random.default_rng(5)
    for m in (1, 255, 257, 1000, 300_000):
        v, mask = rng.normal(size=m), rng.random(m) < 0.6
        got = REF.device_sum([[v], [v, v]], mask)
        assert abs(got[0] - v[mask].sum()) <= 1e-9 and abs(got[1] - 2 * v[mask].sum()) <= 2e-9


def test_ransac_restatement_recovers_a_known_motion():
    src, tgt, corr, T = REF.correspondences("outliers", 400, 1)
    r = REF.ransac(src, tgt, corr, 0.01, 512, 0)
    assert r.c_best >= 100 and np.abs(r.T - T).max() <= 1e-5 and r.n_inliers >= r.c_best and not r.degenerate
    assert r.mask.sum() == r.n_inliers and r.rms < 0.01
    src, tgt, corr, T = REF.correspondences("collinear", 50, 1)
    r = REF.ransac(src, tgt, corr, 0.01, 64, 0)
    assert r.n_valid == 0 and r.c_best == 0 and np.isnan(r.T).all() and not r.mask.any()


def test_matching_restatement_ties_and_nan():
    rng = np.random.default_rng(7)
    fb = rng.random((50, 33)).astype(np.float32)
    fb[20] = fb[10]
    fa = fb[[10, 3, 49]].copy()
    fa[1, 5] = np.nan
    corr, idx, dist = REF.match(fa, fb, mutual=False)
    assert idx.tolist() == [10, 0xffffffff, 49] and dist[0] == 0 and np.isinf(dist[1])
    assert corr.tolist() == [[0, 10], [2, 49]]
    corr, _, _ = REF.match(fa, fb, mutual=True)
    assert corr.tolist() == [[0, 10], [2, 49]]


def test_argument_validation(G):
    xyz, nrm = REF.cube(10, 0), REF.unit_normals(10, 0)
    f = np.zeros((10, 33), np.float32)
    corr = np.stack([np.arange(5), np.arange(5)], axis=1)
    bad_calls = [
        lambda: G.compute_fpfh(np.zeros((4, 2)), nrm),
        lambda: G.compute_fpfh(xyz, nrm[:5]),
        lambda: G.compute_fpfh(xyz, nrm, k=2),
        lambda: G.compute_fpfh(xyz, nrm, k=33),
        lambda: G.compute_fpfh(xyz, nrm, k=True),
        lambda: G.compute_fpfh(xyz, nrm, radius=0.0),
        lambda: G.compute_fpfh(xyz, nrm, radius=float("nan")),
        lambda: G.compute_fpfh_device(None, 2, 0, 0),
        lambda: G.compute_fpfh_device(None, 8, 0, 0, radius=-1.0),
        lambda: G.match_features(f[:, :32], f),
        lambda: G.match_features(f, np.zeros((0, 33), np.float32)),
        lambda: G.match_features(f, f, mutual=1),
        lambda: G.match_features_device(None, 0, 1, 0, 1, 0, mutual=True),
        lambda: G.registration_ransac(xyz, xyz, corr[:2], 0.1),
        lambda: G.registration_ransac(xyz, xyz, corr.astype(np.float32), 0.1),
        lambda: G.registration_ransac(xyz, xyz, corr - 1, 0.1),
        lambda: G.registration_ransac(xyz, xyz, corr, 0.0),
        lambda: G.registration_ransac(xyz, xyz, corr, float("inf")),
        lambda: G.registration_ransac(xyz, xyz, corr, 0.1, num_hypotheses=0),
        lambda: G.registration_ransac(xyz, xyz, corr, 0.1, num_hypotheses=65537),
        lambda: G.registration_ransac(xyz, xyz, corr, 0.1, seed=-1),
        lambda: G.registration_ransac(xyz, xyz, corr, 0.1, seed=2 ** 64),
        lambda: G.registration_ransac(np.zeros((0, 3), np.float32), xyz, corr, 0.1),
        lambda: G.registration_ransac_device(None, 0, 10, 0, 10, 0, 2, 0.1, 16, 0, 0),
        lambda: G.register_global(xyz, xyz, 0.0),
        lambda: G.register_global(xyz, xyz, -1.0),
        lambda: G.register_global(xyz[:, :2], xyz, 0.1),
        lambda: G.register_global(xyz, xyz, 0.1, k=2),
        lambda: G.register_global(xyz, xyz, 0.1, feature_radius=0),
        lambda: G.register_global(xyz, xyz, 0.1, num_hypotheses=0),
        lambda: G.register_global(xyz, xyz, 0.1, rounds=0),
        lambda: G.register_global(xyz, xyz, 0.1, seed=-1),
        lambda: G.register_global(xyz, xyz, 0.1, mutual="yes"),
        lambda: G.register_global(xyz, xyz, 0.1, refine=1),
    ]
    for i, call in enumerate(bad_calls):
        with pytest.raises(ValueError):
            call()
            pytest.fail("call %d raised nothing" % i)


def test_c_entries_reject_bad_arguments_without_a_gpu():
    L = importlib.import_module(PKG + "._lib")
    lib = L.load()
    assert lib.r3d_fpfh_knn(None, 8, 0.0, None, None, None, None) == L.ERR_INVALID
    assert lib.r3d_feature_match(None, None, 1, None, 1, 0, None, None, None, None) == L.ERR_INVALID
    assert lib.r3d_register_ransac(None, None, 3, None, 3, None, 3, 0.1, 8, 0, None, None, None) == L.ERR_INVALID
