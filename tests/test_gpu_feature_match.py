"""GPU: nearest feature rows and the mutual filter (r3d_feature_match; registration.py) against the NumPy restatement of
include/r3d.h in tests/register_ref.py: idx and dist bit for bit, the correspondence list exactly."""
import ctypes as C
import importlib

import numpy as np
import pytest

import register_ref as REF
from helpers import PKG, r3d as _r3d
from test_gpu_bounds import Guarded

pytestmark = pytest.mark.gpu

NA, NB = [1, 63, 64, 65, 1000], [1, 255, 257, 5000]


@pytest.fixture(scope="module")
def R():
    return _r3d()


@pytest.fixture(scope="module")
def G(R):
    return importlib.import_module(PKG + ".registration")


@pytest.fixture(scope="module")
def L(R):
    return importlib.import_module(PKG + "._lib")


@pytest.fixture(scope="module")
def ctx(R):
    c = R.Context(0)
    yield c
    c.close()


def features(kind, na, nb, seed):
    rng = np.random.default_rng([seed, na, nb])
    fa, fb = (rng.random((na, 33)) * 100).astype(np.float32), (rng.random((nb, 33)) * 100).astype(np.float32)
    if kind == "ties":                 # duplicated target rows, and sources that ARE target rows: distance 0 twice
        fb[nb // 2:] = fb[:nb - nb // 2]
        fa[::2] = fb[rng.integers(0, nb, fa[::2].shape[0])]
    if kind == "nan":
        fa[::7, 3] = np.nan
        fb[::5, 32] = np.nan
        fb[1::11, 0] = np.inf
    if kind == "all_nan":
        fb[:, 16] = np.nan
    return fa, fb


def device_run(G, ctx, fa, fb, mutual, want_corr=True):
    na, nb = fa.shape[0], fb.shape[0]
    ga, gb = Guarded(ctx, fa.nbytes, 4, data=fa, seed=1), Guarded(ctx, fb.nbytes, 4, data=fb, seed=2)
    gi, gd = Guarded(ctx, na * 4, 4, seed=3), Guarded(ctx, na * 4, 4, seed=4)
    gc = Guarded(ctx, na * 8, 4, seed=5) if want_corr else None
    try:
        m = G.match_features_device(ctx, ga.ptr, na, gb.ptr, nb, gi.ptr, gd.ptr, gc.ptr if gc else None, mutual)
        idx, dist = gi.read(np.uint32), gd.read(np.float32)
        corr = gc.read(np.uint32, (na, 2))[:m] if gc else None
        ga.unchanged()
        gb.unchanged()
        return idx, dist, corr
    finally:
        for g in (ga, gb, gi, gd, gc):
            if g is not None:
                g.free()


_WANT = {}


def reference(key, fa, fb):
    if key not in _WANT:
        _WANT[key] = (REF.nearest_rows(fa, fb), REF.nearest_rows(fb, fa))
    return _WANT[key]


@pytest.mark.parametrize("kind", ["random", "ties", "nan", "all_nan"])
@pytest.mark.parametrize("nb", NB)
@pytest.mark.parametrize("na", NA)
def test_nearest_rows_and_mutual_list(G, ctx, na, nb, kind):
    fa, fb = features(kind, na, nb, 0)
    (wi, wd), (wbi, _) = reference((kind, na, nb), fa, fb)
    for mutual in (False, True):
        idx, dist, corr = device_run(G, ctx, fa, fb, mutual)
        assert np.array_equal(idx, wi), np.flatnonzero(idx != wi)[:5]
        assert np.array_equal(dist.view(np.uint32), wd.view(np.uint32)), np.flatnonzero(dist != wd)[:5]
        keep = wi != REF.NONE
        if mutual:
            keep &= wbi[np.where(keep, wi, 0).astype(np.int64)] == np.arange(na, dtype=np.uint32)
        rows = np.flatnonzero(keep).astype(np.uint32)
        assert np.array_equal(corr, np.stack([rows, wi[rows]], axis=1).reshape(-1, 2))
    if kind == "all_nan":
        assert (wi == REF.NONE).all() and np.isinf(wd).all() and corr.shape[0] == 0
    if kind == "ties" and nb > 1:
        assert (wd[::2] == 0).all()
        for j in np.unique(wi[::2]):                                            # the lowest of the equal rows
            assert np.flatnonzero((fb == fb[j]).all(axis=1))[0] == j


def test_two_rows_per_lane_and_many_chunks(G, ctx):
    """131 073 source rows take the two-rows-per-lane kernel with one row in its last block; 300 target rows: three tiles."""
    fa, fb = features("random", 2 * 256 * 256 + 1, 300, 3)
    fa[5] = fb[299]
    wi, wd = REF.nearest_rows(fa, fb)
    idx, dist, _ = device_run(G, ctx, fa, fb, False, want_corr=False)
    assert np.array_equal(idx, wi) and np.array_equal(dist.view(np.uint32), wd.view(np.uint32)) and idx[5] == 299


def _check_with_list(G, ctx, fa, fb, mutuals):
    (wi, wd), (wbi, _) = REF.nearest_rows(fa, fb), REF.nearest_rows(fb, fa)
    na = fa.shape[0]
    kept = {}
    for mutual in mutuals:
        idx, dist, corr = device_run(G, ctx, fa, fb, mutual)
        assert np.array_equal(idx, wi), np.flatnonzero(idx != wi)[:5]
        assert np.array_equal(dist.view(np.uint32), wd.view(np.uint32)), np.flatnonzero(dist != wd)[:5]
        keep = wi != REF.NONE
        if mutual:
            keep &= wbi[np.where(keep, wi, 0).astype(np.int64)] == np.arange(na, dtype=np.uint32)
        rows = np.flatnonzero(keep).astype(np.uint32)
        assert np.array_equal(corr, np.stack([rows, wi[rows]], axis=1).reshape(-1, 2))
        want, _, _ = REF.match(fa, fb, mutual=mutual)
        assert np.array_equal(corr, want)
        kept[mutual] = keep
    return kept


def test_compaction_above_65536_rows(G, ctx):
    """66 306 source rows: 260 workgroups of keep counts, more than the 256 threads of the scan's one workgroup (above 256 x 256
    rows).  Every 5th target row is NaN (nobody's neighbour); source rows are copies of
    target rows or NaN in runs that straddle wave (64) and workgroup (256) boundaries, and whole workgroups keep nothing."""
    na, nb = 65537 + 256 * 3 + 1, 300
    fa, fb = features("random", na, nb, 11)
    fb[::5, 32] = np.nan
    good = np.flatnonzero(np.isfinite(fb).all(axis=1))
    rng = np.random.default_rng(12)
    fa[:] = fb[good[rng.integers(0, good.size, na)]] + (rng.random((na, 33)) * 1e-3).astype(np.float32)
    for lo, hi in ((40, 90), (200, 300), (256 * 7, 256 * 9), (256 * 100 - 3, 256 * 100 + 70), (65536 - 130, 65536 + 130),
                   (256 * 258, 256 * 259), (na - 5, na - 1)):
        fa[lo:hi, 7] = np.nan                                         # dropped in both directions: no neighbour at all
    kept = _check_with_list(G, ctx, fa, fb, (False, True))
    assert not kept[False][256 * 7:256 * 9].any() and kept[False][256 * 9] and kept[False][65536 + 130] and kept[False][na - 1]
    per_block = np.add.reduceat(kept[True].astype(np.int64), np.arange(0, na, 256))
    assert (per_block == 0).any() and per_block.max() >= 1 and 0 < kept[True].sum() <= nb


SCAN_SEGMENT = 1024 * 256   # rows of `a` behind one segment of the shared tile scan: 1024 counters, one per workgroup of 256 rows


@pytest.mark.parametrize("na", [SCAN_SEGMENT - 1, SCAN_SEGMENT, SCAN_SEGMENT + 1, 2 * SCAN_SEGMENT + 257])
def test_keep_counts_across_the_scan_segments(G, ctx, na):
    """The keep counts go through the library's tile scan (r3d_compact_dev.h), which walks a row of counters in segments of 1024:
    source rows up to, at and past one segment, and two segments plus a workgroup and a row.  nb = 8.  A seeded 30 % of the source
    rows are all NaN (holes in every workgroup), one workgroup is all NaN and one is clean.  The expected list is not searched
    for again: it is the rule of include/r3d.h applied in NumPy to the d_idx_out the call wrote and, for mutual, to the rows of
    a plain b -> a call.  A mutual list holds at most nb = 8 rows, so only the plain list can fill a workgroup."""
    nb = 8
    rng = np.random.default_rng([21, na])
    fa, fb = (rng.random((na, 33)) * 100).astype(np.float32), (rng.random((nb, 33)) * 100).astype(np.float32)
    fa[rng.random(na) < 0.3] = np.nan
    fa[256 * 5:256 * 6] = np.nan
    fa[256 * 6:256 * 7] = (rng.random((256, 33)) * 100).astype(np.float32)
    fa[256 * 6 + 9] = fb[3]                                              # one pair that is mutual whatever the rest does
    idx_ba, _, _ = device_run(G, ctx, fb, fa, False, want_corr=False)
    for mutual in (False, True):
        idx, _, corr = device_run(G, ctx, fa, fb, mutual)
        keep = idx != REF.NONE
        if mutual:
            keep &= idx_ba[np.where(keep, idx, 0).astype(np.int64)] == np.arange(na, dtype=np.uint32)
        per_block = np.add.reduceat(keep.astype(np.int64), np.arange(0, na, 256))
        assert 0 < keep.sum() < na and (per_block == 0).any()
        assert mutual or (per_block == 256).any()
        rows = np.flatnonzero(keep).astype(np.uint32)
        assert corr.shape[0] == rows.size                                # h_m_out
        assert np.array_equal(corr, np.stack([rows, idx[rows]], axis=1).reshape(-1, 2))


def test_reverse_search_through_the_two_rows_per_lane_kernel(G, ctx):
    """300 source rows against 131 073 target rows, mutual: the b -> a search has 131 073 query rows"""
    fa, fb = features("random", 300, 2 * 256 * 256 + 1, 13)
    fb[::5, 32] = np.nan
    fb[131072] = fa[17]
    kept = _check_with_list(G, ctx, fa, fb, (True,))
    assert kept[True][17]


def test_host_entry_and_repeatability(G, ctx):
    fa, fb = features("ties", 700, 900, 5)
    a, b = G.match_features(fa, fb, mutual=True, ctx=ctx), G.match_features(fa, fb, mutual=True, ctx=ctx)
    want, wi, wd = REF.match(fa, fb, mutual=True)
    assert np.array_equal(a.corr, want) and np.array_equal(a.corr, b.corr) and np.array_equal(a.idx, wi)
    assert np.array_equal(a.dist.view(np.uint32), wd.view(np.uint32))
    every = G.match_features(fa, fb, mutual=False, ctx=ctx)
    assert every.corr.shape[0] == 700 and np.array_equal(every.corr[:, 1], wi)


def test_invalid_calls_write_nothing(L, ctx):
    fa, fb = features("random", 100, 120, 9)
    ga, gb = Guarded(ctx, fa.nbytes, 4, data=fa, seed=1), Guarded(ctx, fb.nbytes, 4, data=fb, seed=2)
    gi, gd, gc = Guarded(ctx, 400, 4, seed=3), Guarded(ctx, 400, 4, seed=4), Guarded(ctx, 800, 4, seed=5)
    m = C.c_int64(-5)
    lib = ctx.lib

    def call(c=ctx.handle, a=ga.ptr, na=100, b=gb.ptr, nb=120, mutual=1, i=gi.ptr, d=gd.ptr, corr=gc.ptr, m_=C.byref(m)):
        return lib.r3d_feature_match(c, a, na, b, nb, mutual, i, d, corr, m_)

    for kw in [dict(c=None), dict(a=None), dict(b=None), dict(i=None), dict(na=0), dict(nb=0), dict(na=-1), dict(nb=2 ** 32), dict(mutual=2),
               dict(mutual=-1), dict(corr=None), dict(m_=None), dict(corr=None, m_=None), dict(i=ga.ptr + 4), dict(d=gb.ptr), dict(d=gi.ptr),
               dict(corr=gd.ptr), dict(corr=ga.ptr + 8)]:
        assert call(**kw) == L.ERR_INVALID, kw
        for g in (ga, gb, gi, gd, gc):
            g.unchanged()
        assert m.value == -5
    assert call() == 0, L.last_error()
    assert 0 < m.value <= 100
    assert call(mutual=0, corr=None, m_=None) == 0, L.last_error()
    for g in (ga, gb, gi, gd, gc):
        g.free()
