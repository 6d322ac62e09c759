"""GPU: exact k nearest neighbours of an index's own points and the outlier filters built on them (r3d_nn_index_knn_self,
r3d_outlier_statistical, r3d_outlier_radius, r3d_select_rows; outliers.py; other_tools/remove_outliers.py) against the
reference of tests/outliers_ref.py: lists, scores, masks and counts bit for bit, mu / sigma / T within 1e-12 relative."""
import ctypes as C
import importlib
import os
import subprocess
import sys

import numpy as np
import pytest

import outliers_ref as REF
from helpers import PKG, ROOT, r3d as _r3d
from test_gpu_bounds import Guarded

pytestmark = pytest.mark.gpu

KS = [1, 5, 8, 9, 20, 32]


@pytest.fixture(scope="module")
def R():
    return _r3d()


@pytest.fixture(scope="module")
def O(R):
    return importlib.import_module(PKG + ".outliers")


@pytest.fixture(scope="module")
def L(R):
    return importlib.import_module(PKG + "._lib")


@pytest.fixture(scope="module")
def ctx(R):
    c = R.Context(0)
    yield c
    c.close()


def _cube(n, seed):
    return np.random.default_rng(seed).random((n, 3)).astype(np.float32)


def _lattice(m, spacing=1.0):
    g = np.stack(np.meshgrid(*[np.arange(m)] * 3, indexing="ij"), -1).reshape(-1, 3)
    return (g.astype(np.float32) * np.float32(spacing))


def _room(R, n, seed=0):
    syn = importlib.import_module(PKG + ".synthetic")
    depth, q, t, K = syn.room_views(6, 120, 160, seed=seed)
    xyz = R.fuse_frames(depth, q, t, intrinsics=K)
    xyz = xyz[np.isfinite(xyz).all(axis=1)]
    return xyz[np.random.default_rng(seed).choice(xyz.shape[0], n, replace=False)]


def _hot(copies, background, seed):
    rng = np.random.default_rng(seed)
    xyz = np.concatenate([np.tile(np.float32([[0.25, 0.5, 0.75]]), (copies, 1)), rng.random((background, 3)).astype(np.float32)])
    return xyz[rng.permutation(xyz.shape[0])]


def _clouds(R):
    rng = np.random.default_rng(11)
    bad = _cube(3000, 12)
    bad[rng.choice(3000, 60, replace=False), rng.integers(0, 3, 60)] = np.nan
    bad[rng.choice(3000, 30, replace=False), rng.integers(0, 3, 30)] = np.inf
    bad[5, 0] = -np.inf
    return {"cube20k": _cube(20_000, 1), "room50k": _room(R, 50_000), "lattice": _lattice(14, 0.5),
            "nonfinite": bad, "offset1e4": _cube(8000, 3) + np.float32(1e4),
            "dups10k": _hot(10_000, 3000, 4)}


@pytest.fixture(scope="module")
def clouds(R):
    c = _clouds(R)
    return {name: (xyz, REF.knn(xyz, 32)) for name, xyz in c.items()}


class Index:
    """A device copy of the cloud and its NNIndex."""

    def __init__(self, R, ctx, xyz):
        icp = importlib.import_module(PKG + ".icp")
        self.ctx, self.n = ctx, xyz.shape[0]
        self.d_xyz = ctx.alloc(max(xyz.nbytes, 16)).upload(np.ascontiguousarray(xyz, np.float32))
        self.ix = icp.NNIndex(ctx, self.d_xyz.ptr, self.n)

    def close(self):
        self.ix.close()
        self.d_xyz.free()


def device_knn(R, ctx, xyz, k):
    ix = Index(R, ctx, xyz)
    n = xyz.shape[0]
    try:
        d_idx, d_d2 = ctx.alloc(n * k * 4), ctx.alloc(n * k * 4)
        ix.ix.knn_self(k, d_idx.ptr, d_d2.ptr)
        idx, d2 = d_idx.download(np.uint32, n * k).reshape(n, k), d_d2.download(np.float32, n * k).reshape(n, k)
        d_idx.free()
        d_d2.free()
        return idx, d2
    finally:
        ix.close()


def assert_lists(got, want, k):
    gi, gd = got
    wi, wd = want[0][:, :k], want[1][:, :k]
    bad = np.flatnonzero((gi != wi).any(axis=1) | (gd.view(np.uint32) != wd.view(np.uint32)).any(axis=1))
    assert bad.size == 0, "%d rows differ, first %d: got %s %s want %s %s" % (bad.size, bad[0], gi[bad[0]], gd[bad[0]],
                                                                               wi[bad[0]], wd[bad[0]])


@pytest.mark.parametrize("k", KS)
@pytest.mark.parametrize("n", [1, 2, "k", "k+1", 1023, 1024, 1025, 4097])
def test_knn_lists_small_clouds(R, ctx, k, n):
    n = {"k": k, "k+1": k + 1}.get(n, n)
    xyz = _cube(n, 100 + n)
    assert_lists(device_knn(R, ctx, xyz, k), REF.knn_brute(xyz, k), k)


@pytest.mark.parametrize("name", ["cube20k", "room50k", "lattice", "nonfinite", "offset1e4", "dups10k"])
def test_knn_lists_clouds(R, ctx, clouds, name):
    xyz, want = clouds[name]
    for k in KS:
        assert_lists(device_knn(R, ctx, xyz, k), want, k)


def check_sor(O, xyz, k, ratio, want_lists=None):
    got = O.remove_statistical_outlier(xyz, k, ratio)
    m, keep, (V, mu, sigma, T) = REF.sor(xyz, k, ratio, want_lists)
    assert np.array_equal(got.score.view(np.uint64), m.view(np.uint64)), np.flatnonzero(got.score != m)[:5]
    assert got.stats.V == V
    for a, b in ((got.stats.mu, mu), (got.stats.sigma, sigma), (got.stats.T, T)):
        assert abs(a - b) <= 1e-12 * max(abs(b), 1e-300), (a, b)
    mask = got.score <= got.stats.T
    assert np.array_equal(got.rows, np.flatnonzero(mask)) and np.array_equal(mask, keep)
    assert np.array_equal(got.xyz.view(np.uint32), xyz[mask].view(np.uint32))
    return got, keep


@pytest.mark.parametrize("name", ["cube20k", "room50k", "nonfinite", "offset1e4", "dups10k"])
@pytest.mark.parametrize("k,ratio", [(1, 1.0), (9, 2.0), (20, 2.0), (32, 0.5)])
def test_sor_matches_oracle(O, clouds, name, k, ratio):
    xyz, lists = clouds[name]
    check_sor(O, xyz, k, ratio, (lists[0][:, :k], lists[1][:, :k]))


def test_sor_lattice_keeps_every_point(O):
    xyz = _lattice(12, 0.25) + np.float32(0.125)
    got, _ = check_sor(O, xyz, 6, 0.1)
    inner = ((xyz > 0.2) & (xyz < 2.8)).all(axis=1)              # six neighbours at 0.25: the lowest score, all kept
    assert np.isin(np.flatnonzero(inner), got.rows).all()
    xyz = _lattice(10, 1.0)
    got = O.remove_statistical_outlier(xyz, 1, 1.0)                  # every point: one neighbour at exactly 1
    assert got.stats.sigma == 0.0 and got.rows.size == xyz.shape[0]


def test_sor_room_with_injected_outliers(R, O):
    surf = _room(R, 40_000, seed=2)
    rng = np.random.default_rng(2)
    lo, hi = surf.min(axis=0), surf.max(axis=0)
    noise = (lo + rng.random((400, 3)) * (hi - lo)).astype(np.float32)
    xyz = np.concatenate([surf, noise])
    perm = rng.permutation(xyz.shape[0])
    xyz, is_noise = xyz[perm], perm >= surf.shape[0]
    got, keep = check_sor(O, xyz, 20, 2.0)
    removed = ~np.isin(np.arange(xyz.shape[0]), got.rows)
    assert removed[is_noise].mean() == (~keep)[is_noise].mean() and removed[~is_noise].mean() == (~keep)[~is_noise].mean()
    assert removed[is_noise].mean() > removed[~is_noise].mean()
    # a row-shuffled cloud: the shuffled scores and mask, bit for bit; two runs: the same bits
    p = rng.permutation(xyz.shape[0])
    again = O.remove_statistical_outlier(xyz[p], 20, 2.0)
    assert np.array_equal(again.score.view(np.uint64), got.score[p].view(np.uint64))
    assert np.array_equal(np.sort(p[again.rows]), got.rows)
    twice = O.remove_statistical_outlier(xyz, 20, 2.0)
    assert np.array_equal(twice.score.view(np.uint64), got.score.view(np.uint64)) and twice.stats == got.stats


_COUNTS = {}


def check_ror(O, xyz, min_points, radius):
    got = O.remove_radius_outlier(xyz, min_points, radius)
    key = (xyz.tobytes(), radius)
    if key not in _COUNTS:
        _COUNTS[key] = REF.ror_counts(xyz, radius)
    c = np.minimum(_COUNTS[key], min_points)
    keep = _COUNTS[key] >= min_points
    assert np.array_equal(got.count.astype(np.int64), c)
    assert np.array_equal(got.rows, np.flatnonzero(keep))
    assert np.array_equal(got.xyz.view(np.uint32), xyz[keep].view(np.uint32))
    return got


@pytest.mark.parametrize("name,radius", [("cube20k", 0.03), ("room50k", 0.05), ("nonfinite", 0.08), ("offset1e4", 0.05),
                                         ("dups10k", 0.05)])
@pytest.mark.parametrize("min_points", [1, 5, "more than n"])
def test_ror_matches_oracle(O, clouds, name, radius, min_points):
    xyz = clouds[name][0]
    check_ror(O, xyz, xyz.shape[0] + 1 if min_points == "more than n" else min_points, radius)


def test_ror_lattice_counts_pairs_at_exactly_r2(O):
    xyz = _lattice(12, 0.5)
    got = check_ror(O, xyz, 6, 0.5)
    inner = ((xyz > 0) & (xyz < 5.5)).all(axis=1)
    assert (got.count[inner] == 6).all()


def test_hot_cluster_sor_and_ror(O):
    """100k copies of one point + 20k background: the strict cull keeps this linear."""
    xyz = _hot(100_000, 20_000, 7)
    check_sor(O, xyz, 20, 2.0)
    check_ror(O, xyz, 16, 0.05)
    check_ror(O, xyz, 3, 0.01)


@pytest.mark.parametrize("n", [1, 4095, 4096, 4097, 3 * 4096 + 17])
@pytest.mark.parametrize("kind", ["all", "none", "random"])
def test_select_rows(R, O, ctx, n, kind):
    xyz = _cube(n, n)
    keep = {"all": np.ones(n, np.uint8), "none": np.zeros(n, np.uint8),
            "random": (np.random.default_rng(n).random(n) < 0.3).astype(np.uint8) * np.uint8(7)}[kind]
    d_xyz, d_keep = ctx.alloc(n * 12).upload(xyz), ctx.alloc(n).upload(keep)
    d_out, d_rows = ctx.alloc(n * 12), ctx.alloc(n * 4)
    m = O.select_rows_device(ctx, d_xyz.ptr, n, d_keep.ptr, d_out.ptr, d_rows.ptr)
    want = np.flatnonzero(keep)
    assert m == want.size
    if m:
        assert np.array_equal(d_rows.download(np.uint32, m), want)
        assert np.array_equal(d_out.download(np.float32, 3 * m).reshape(-1, 3), xyz[want])
    for b in (d_xyz, d_keep, d_out, d_rows):
        b.free()


OFF = {1: 3, 4: 4, 8: 8}        # naturally aligned, not 16-byte aligned


def test_outputs_stay_inside_their_buffers(R, O, L, ctx):
    xyz = _cube(3 * 1024 + 17, 21)
    xyz[7] = np.nan
    n, k = xyz.shape[0], 9
    ix = Index(R, ctx, xyz)
    try:
        want_lists = REF.knn_brute(xyz, k)
        gi, gd = Guarded(ctx, n * k * 4, OFF[4], seed=1), Guarded(ctx, n * k * 4, OFF[4], seed=2)
        ix.ix.knn_self(k, gi.ptr, gd.ptr)
        assert_lists((gi.read(np.uint32, (n, k)), gd.read(np.float32, (n, k))), want_lists, k)
        m, keep, stats = REF.sor(xyz, k, 1.5, want_lists)
        gk, gs = Guarded(ctx, n, OFF[1], seed=3), Guarded(ctx, n * 8, OFF[8], seed=4)
        kept, st = O.statistical_outlier_device(ix.ix, k, 1.5, gk.ptr, gs.ptr)
        assert kept == keep.sum() and np.array_equal(gk.read(np.uint8).astype(bool), keep)
        assert np.array_equal(gs.read(np.float64).view(np.uint64), m.view(np.uint64))
        c, rkeep = REF.ror(xyz, 4, 0.1)
        gk2, gc = Guarded(ctx, n, OFF[1], seed=5), Guarded(ctx, n * 4, OFF[4], seed=6)
        assert O.radius_outlier_device(ix.ix, 4, 0.1, gk2.ptr, gc.ptr) == rkeep.sum()
        assert np.array_equal(gk2.read(np.uint8).astype(bool), rkeep) and np.array_equal(gc.read(np.uint32), c)
        mk = int(keep.sum())
        gx, gr = Guarded(ctx, mk * 12, OFF[4], seed=7), Guarded(ctx, mk * 4, OFF[4], seed=8)
        assert O.select_rows_device(ctx, ix.d_xyz.ptr, n, gk.ptr, gx.ptr, gr.ptr) == mk
        assert np.array_equal(gr.read(np.uint32), np.flatnonzero(keep))
        assert np.array_equal(gx.read(np.float32, (-1, 3)), xyz[keep])
        # invalid calls write nothing
        lib = ctx.lib
        h = C.c_int64(-5)
        gi2, gk3, gs3 = Guarded(ctx, n * k * 4, OFF[4], seed=9), Guarded(ctx, n, OFF[1], seed=10), Guarded(ctx, n * 8, OFF[8], seed=11)
        for bad_k in (0, 33):
            assert lib.r3d_nn_index_knn_self(ix.ix.handle, bad_k, gi2.ptr, None) == L.ERR_INVALID
            assert lib.r3d_outlier_statistical(ix.ix.handle, bad_k, 2.0, gk3.ptr, gs3.ptr, None, C.byref(h)) == L.ERR_INVALID
        for bad_ratio in (0.0, -1.0, float("nan"), float("inf")):
            assert lib.r3d_outlier_statistical(ix.ix.handle, 8, bad_ratio, gk3.ptr, gs3.ptr, None, C.byref(h)) == L.ERR_INVALID
        for r, mp in ((0.0, 4), (-0.1, 4), (float("inf"), 4), (float("nan"), 4), (0.1, 0), (0.1, -3)):
            assert lib.r3d_outlier_radius(ix.ix.handle, r, mp, gk3.ptr, None, C.byref(h)) == L.ERR_INVALID
        assert lib.r3d_outlier_statistical(ix.ix.handle, 8, 2.0, gk3.ptr, C.c_void_p(gk3.ptr - 4), None, C.byref(h)) == L.ERR_INVALID
        assert lib.r3d_select_rows(ctx.handle, ix.d_xyz.ptr, n, gk.ptr, C.c_void_p(ix.d_xyz.ptr + 12), None, C.byref(h)) == L.ERR_INVALID
        assert h.value == -5
        for g in (gi2, gk3, gs3):
            g.unchanged()
        assert ix.ix.knn_pairs() > 0
        for g in (gi, gd, gk, gs, gk2, gc, gx, gr, gi2, gk3, gs3):
            g.free()
    finally:
        ix.close()


def test_python_api_and_cli_on_a_ply(R, O, tmp_path):
    xyz = _room(R, 30_000, seed=9)
    xyz = np.concatenate([xyz, (xyz.min(0) + np.random.default_rng(9).random((300, 3)) * np.ptp(xyz, 0)).astype(np.float32)])
    src = str(tmp_path / "in.ply")
    R.cloud_io.write_ply_binary(src, xyz)
    xyz = R.cloud_io.read_ply(src).astype(np.float32)
    tool = os.path.join(ROOT, PKG, "other_tools", "remove_outliers.py")
    cases = [(["--statistical", "20", "2.0"], REF.sor(xyz, 20, 2.0)[1]), (["--radius", "16", "0.05"], REF.ror(xyz, 16, 0.05)[1])]
    for args, mask in cases:
        api = (O.remove_statistical_outlier(xyz, 20, 2.0) if args[0] == "--statistical" else O.remove_radius_outlier(xyz, 16, 0.05))
        assert np.array_equal(api.rows, np.flatnonzero(mask)) and np.array_equal(api.xyz, xyz[mask])
        for binary in ([], ["--binary"]):
            out = str(tmp_path / ("out%s.ply" % len(binary)))
            r = subprocess.run([sys.executable, tool, src, out] + args + binary, capture_output=True, text=True, timeout=300)
            assert r.returncode == 0, r.stderr[-2000:]
            n, kept = xyz.shape[0], int(mask.sum())
            assert "%d -> %d (%d removed)" % (n, kept, n - kept) in r.stdout
            back = R.cloud_io.read_ply(out)
            assert back.shape == (kept, 3)
            if binary:
                assert np.array_equal(back.astype(np.float32), xyz[mask])
