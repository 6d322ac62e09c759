"""CPU: the k-NN / outlier reference (tests/outliers_ref.py), the command line other_tools/remove_outliers.py and the argument
checks of the new entry points (r3d_nn_index_knn_self, r3d_outlier_statistical, r3d_outlier_radius, r3d_select_rows) --
none of which needs a device."""
import ctypes as C
import importlib
import os
import subprocess
import sys

import numpy as np
import pytest

import outliers_ref as REF
from helpers import PKG, ROOT

TOOL = os.path.join(ROOT, PKG, "other_tools", "remove_outliers.py")


@pytest.mark.parametrize("seed,n,k", [(0, 600, 1), (1, 900, 9), (2, 700, 32)])
def test_brute_force_and_tree_oracles_agree(seed, n, k):
    rng = np.random.default_rng(seed)
    xyz = rng.random((n, 3)).astype(np.float32)
    xyz[:40] = xyz[40]                                              # 41 identical rows
    xyz[50:60] = np.round(xyz[50:60] * 4) / 4                       # a few lattice points: exact ties
    xyz[70] = np.nan
    xyz[71, 1] = np.inf
    a, b = REF.knn_brute(xyz, k), REF.knn_tree(xyz, k)
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
    assert (a[0][70] == REF.NO_ROW).all() and (a[0][71] == REF.NO_ROW).all()
    assert not np.isin(a[0], [70, 71]).any()
    assert np.array_equal(REF.ror_counts(xyz, 0.05), _brute_counts(xyz, 0.05))


def _brute_counts(xyz, radius):
    from oracle.icp_ref import pair_d2
    d = pair_d2(xyz, xyz)
    np.fill_diagonal(d, np.inf)
    return (d <= REF.r2_of(radius)).sum(axis=1)


def test_single_scored_point_has_zero_sigma():
    xyz = np.array([[0, 0, 0], [1, 0, 0], [np.nan, 0, 0]], np.float32)
    m, keep, (V, mu, sigma, T) = REF.sor(xyz, 1, 2.0)
    assert V == 2 and sigma == 0.0 and keep[:2].all() and not keep[2]   # both points see each other at distance 1
    m, keep, (V, mu, sigma, T) = REF.sor(xyz[[0, 2]], 1, 2.0)
    assert V == 0 and not keep.any()
    xyz = np.array([[0, 0, 0], [1, 0, 0], [3, 0, 0]], np.float32)
    m, keep, (V, mu, sigma, T) = REF.sor(xyz, 2, 1.0)
    assert V == 3 and m.tolist() == [2.0, 1.5, 2.5]


def test_lattice_keeps_every_point():
    g = np.stack(np.meshgrid(*[np.arange(6)] * 3, indexing="ij"), -1).reshape(-1, 3).astype(np.float32) * np.float32(0.5)
    m, keep, (V, mu, sigma, T) = REF.sor(g, 6, 1.0)
    assert V == g.shape[0]
    # interior points see six neighbours at 0.5, corner points fewer: sigma > 0, but every interior point is kept
    inner = ((g > 0) & (g < 2.5)).all(axis=1)
    assert keep[inner].all() and (m[inner] == 0.5).all()
    c, keep = REF.ror(g, 6, 0.5)                                  # pairs at exactly r2 = 0.25 count
    assert (c[inner] == 6).all() and keep[inner].all() and not keep[~inner].all()


def test_r2_rounds_once_to_float32():
    r = 0.1
    assert REF.r2_of(r) == np.float32(0.1 * 0.1) and REF.r2_of(r) != np.float32(np.float32(r) * np.float32(r))
    xyz = np.array([[0, 0, 0], [0.1, 0, 0]], np.float32)
    from oracle.icp_ref import pair_d2
    d = pair_d2(xyz[:1], xyz[1:])[0, 0]
    assert REF.ror_counts(xyz, r).tolist() == [int(d <= REF.r2_of(r))] * 2


def test_unscored_points():
    xyz = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0], [np.inf, 0, 0]], np.float32)
    m, keep, (V, mu, sigma, T) = REF.sor(xyz, 3, 2.0)
    assert V == 0 and np.isinf(m).all() and not keep.any()        # three candidates need four finite points
    idx, d2 = REF.knn(xyz, 3)
    assert (idx[:3, 2] == REF.NO_ROW).all() and np.isinf(d2[:3, 2]).all() and (idx[3] == REF.NO_ROW).all()


def run_tool(*args):
    return subprocess.run([sys.executable, TOOL] + list(args), capture_output=True, text=True, timeout=120)


def test_tool_help():
    r = run_tool("--help")
    assert r.returncode == 0 and "--statistical" in r.stdout and "--radius" in r.stdout and "--binary" in r.stdout


@pytest.mark.parametrize("args,message", [
    ([], "the following arguments are required"),
    (["in.ply", "out.ply"], "one of the arguments --statistical --radius is required"),
    (["in.ply", "out.ply", "--statistical", "20", "2", "--radius", "4", "0.1"], "not allowed with argument"),
    (["in.ply", "out.ply", "--statistical", "0", "2"], "K must be in [1, 32]"),
    (["in.ply", "out.ply", "--statistical", "33", "2"], "K must be in [1, 32]"),
    (["in.ply", "out.ply", "--statistical", "2.5", "2"], "K must be an integer"),
    (["in.ply", "out.ply", "--statistical", "20", "0"], "RATIO must be finite and positive"),
    (["in.ply", "out.ply", "--statistical", "20", "nan"], "RATIO must be finite and positive"),
    (["in.ply", "out.ply", "--radius", "0", "0.1"], "N must be >= 1"),
    (["in.ply", "out.ply", "--radius", "4", "-1"], "R must be finite and positive"),
    (["in.ply", "out.ply", "--radius", "4", "inf"], "R must be finite and positive"),
    (["in.ply", "out.ply", "--radius", "4", "abc"], "R must be a number"),
    (["in.ply", "out.ply", "--radius", "4"], "expected 2 arguments"),
    (["missing.ply", "out.ply", "--radius", "4", "0.1"], "does not exist"),
])
def test_tool_argument_errors(tmp_path, args, message):
    cwd = os.getcwd()
    os.chdir(tmp_path)
    try:
        (tmp_path / "in.ply").write_text("ply\nformat ascii 1.0\nelement vertex 0\nend_header\n")
        r = run_tool(*args)
    finally:
        os.chdir(cwd)
    assert r.returncode == 2
    assert message in r.stderr
    assert not (tmp_path / "out.ply").exists()


def test_entry_points_reject_bad_arguments_without_gpu():
    L = importlib.import_module(PKG + "._lib")
    lib = L.load()
    n = C.c_int64(-7)
    stats = (C.c_double * 4)(-1, -1, -1, -1)
    assert lib.r3d_nn_index_knn_self(None, 8, None, None) == L.ERR_INVALID
    assert "NULL" in L.last_error()
    assert lib.r3d_outlier_statistical(None, 20, 2.0, None, None, stats, C.byref(n)) == L.ERR_INVALID
    assert lib.r3d_outlier_radius(None, 0.1, 4, None, None, C.byref(n)) == L.ERR_INVALID
    assert lib.r3d_select_rows(None, None, 0, None, None, None, C.byref(n)) == L.ERR_INVALID
    assert lib.r3d_nn_index_knn_stats(None, C.byref(n)) == L.ERR_INVALID
    assert n.value == -7 and list(stats) == [-1, -1, -1, -1]


def test_python_wrappers_check_arguments_first():
    O = importlib.import_module(PKG + ".outliers")
    xyz = np.zeros((4, 3), np.float32)
    for k in (0, 33, 2.5, True, "8"):
        with pytest.raises(ValueError):
            O.knn(xyz, k)
        with pytest.raises(ValueError):
            O.remove_statistical_outlier(xyz, k)
    for ratio in (0.0, -1.0, float("nan"), float("inf"), "x"):
        with pytest.raises(ValueError):
            O.remove_statistical_outlier(xyz, 4, ratio)
    for pts, r in ((0, 0.1), (-1, 0.1), (1.5, 0.1), (4, 0.0), (4, -0.1), (4, float("inf")), (4, float("nan"))):
        with pytest.raises(ValueError):
            O.remove_radius_outlier(xyz, pts, r)
    with pytest.raises(ValueError):
        O.knn(np.zeros((4, 2), np.float32), 4)
    R = importlib.import_module(PKG)
    assert R.remove_statistical_outlier is O.remove_statistical_outlier and R.remove_radius_outlier is O.remove_radius_outlier
    assert R.knn is O.knn
