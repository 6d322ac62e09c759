"""CPU: the references of tests/icp_parts_ref.py against independent NumPy / math.fsum, the properties its value sets are
named for, and the argument checks of the ICP driver's small entry points (none of which needs a device)."""
import ctypes as C
import importlib
import math

import numpy as np
import pytest

import icp_parts_ref as REF
from helpers import PKG


# ---- the references ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,n_classes", [(1, 1), (255, 3), (2049, 24), (20011, 32)])
def test_class_quantiles_against_sorted_indexing(n, n_classes):
    for kind in sorted(REF.VALUE_SETS):
        v, cls = REF.class_case(n, n_classes, kind, 1)
        for q in (0.0, 0.3, 0.5, 0.8, 1.0):
            vals, counts = REF.class_quantiles(v, cls, n_classes, q)
            for c in range(n_classes):
                mine = np.sort([x for x, k in zip(v.tolist(), cls.tolist()) if k == c and math.isfinite(x)])
                assert counts[c] == len(mine)
                if len(mine) == 0:
                    assert vals[c] == np.inf
                else:
                    assert vals[c] == np.float32(mine[int(math.floor(q * (len(mine) - 1)))])


def test_class_case_populations_are_uneven():
    v, cls = REF.class_case(20011, 24, "random_bits", 0)
    _, counts = REF.class_quantiles(v, cls, 24, 0.5)
    pop = np.bincount(cls, minlength=256)
    assert pop[1] == 1 and not pop[4:24:3].any()                         # a class of one; empty classes between full ones
    assert pop[24:].sum() > 1000 and pop[255] > 100                      # bytes that name no class
    assert pop[23] > 0 and counts[23] == 0                               # a populated class without a finite value
    assert pop[0] > 1 and np.unique(v[cls == 0]).size == 1               # a class of one repeated value
    assert counts.max() > 20 * max(1, counts[counts > 1].min())


def test_block_classes():
    assert REF.block_classes(7, 3).tolist() == [0, 0, 0, 1, 1, 1, 2]
    vals, counts = REF.class_quantiles([5, 1, np.nan, 3, -np.inf, np.inf, 2], REF.block_classes(7, 3), 2, 1.0)
    assert vals.tolist() == [5.0, 3.0] and counts.tolist() == [2, 1]     # block 2 is no class of a 2-class call


@pytest.mark.parametrize("n_classes,per_class", [(1, 1), (2, 7), (10, 257), (32, 5000)])
def test_trimmed_means_against_fsum(n_classes, per_class):
    for shift in range(len(REF.BLOCK_KINDS)):
        v, kinds = REF.trimmed_case(n_classes, per_class, shift)
        for keep in (0.0, 0.5, 0.8, 1.0):
            means, scales = REF.trimmed_means(v, n_classes, per_class, keep)
            for c in range(n_classes):
                f = sorted(x for x in v[c * per_class:(c + 1) * per_class].tolist() if math.isfinite(x))
                if not f:
                    assert kinds[c] == "no_finite" and means[c] == np.inf and scales[c] == 0
                    continue
                g = f[int(math.floor(keep * (len(f) - 1)))]
                kept = [x for x in f if x <= g]
                want = math.fsum(kept) / len(kept)
                assert abs(means[c] - want) <= 1e-13 * (math.fsum(map(abs, kept)) / len(kept)), (kinds[c], keep)
                assert abs(scales[c] - math.fsum(map(abs, kept)) / len(kept)) <= 1e-13 * scales[c]


def test_trimmed_mean_compares_arithmetically():
    # the statistic of rank 1 is a zero; both zeros and the negative value pass it, whatever the zero's sign
    for zeros in ((-0.0, 0.0), (0.0, -0.0)):
        v = np.array([-4.0, zeros[0], zeros[1], 8.0], np.float32)
        means, _ = REF.trimmed_means(v, 1, 4, 0.5)
        assert means[0] == -4.0 / 3
    means, _ = REF.trimmed_means(np.array([1, 1, 1, 0.5, 2, 1], np.float32), 1, 6, 0.5)     # ties with the statistic all count
    assert means[0] == 4.5 / 5
    v, kinds = REF.trimmed_case(10, 256, 0)
    b = v[kinds.index("zeros") * 256:][:256]
    assert np.signbit(b[b == 0]).any() and not np.signbit(b[b == 0]).all()
    b = v[kinds.index("ties") * 256:][:256]
    assert (b == REF.PR.quantile_lower(b, 0.5)[0]).sum() > 100


def test_value_sets_isolate_what_they_are_named_for():
    rng = np.random.default_rng(3)
    bits = {k: f(4096, rng).view(np.uint32) for k, f in REF.VALUE_SETS.items()}
    assert np.unique(bits["low_byte"] >> 8).size == 1 and np.unique(bits["low_byte"] & 0xff).size == 256
    assert np.unique(bits["top_byte"] & 0xffffff).size == 1 and np.unique(bits["top_byte"] >> 24).size == 256
    assert np.isfinite(bits["top_byte"].view(np.float32)).all()
    s = bits["straddle_zero"].view(np.float32)
    assert (s < 0).sum() > 1000 and (s > 0).sum() > 1000 and np.intersect1d(s[s > 0], -s[s < 0]).size > 30
    z = bits["zeros_subnormals"].view(np.float32)
    assert {0x00000000, 0x80000000, 0x00000001, 0x807fffff} <= set(bits["zeros_subnormals"].tolist()) and np.abs(z).max() < 1.2e-38
    w = (bits["wall"] >> 8).reshape(-1, 64)
    assert (w == w[:, :1]).all() and np.unique(w[:, 0]).size > 32
    r = bits["random_bits"].view(np.float32)
    assert np.isnan(r).any() and 0 < (~np.isfinite(r)).sum() < 64
    m = REF.mixed_values(20011, 0)
    assert np.isnan(m).any() and np.isposinf(m).any() and np.isneginf(m).any() and np.isfinite(m).mean() > 0.9


def test_row_mover_references():
    xyz = np.arange(12, dtype=np.float32).reshape(4, 3)
    got = REF.gather_rows(xyz, np.array([3, 0, 4, 5, 0xffffffff, 3], np.uint32))
    assert np.array_equal(got[[0, 1, 5]], xyz[[3, 0, 3]]) and np.isnan(got[2:5]).all()
    assert np.isnan(REF.gather_rows(np.zeros((0, 3), np.float32), np.array([0, 1], np.uint32))).all()
    assert np.array_equal(REF.gather_rows_strided(xyz, 1, 2, 2), xyz[[1, 3]])
    perm = np.array([2, 0, 3, 1], np.uint32)
    inv = REF.permutation_invert(perm, np.full(4, 77, np.uint32))
    assert inv[perm].tolist() == [0, 1, 2, 3]
    inv = REF.permutation_invert(np.array([2, 9, 0xffffffff, 1], np.uint32), np.array([70, 71, 72, 73], np.uint32))
    assert inv.tolist() == [70, 3, 0, 73]                                # skipped entries; unnamed slots keep their contents
    assert REF.remap(np.array([0, 2, 3, 0xffffffff], np.uint32), np.array([10, 11, 12], np.uint32)).tolist() == \
        [10, 12, REF.NO_ROW, REF.NO_ROW]
    assert (REF.remap(np.array([0, 1], np.uint32), np.zeros(0, np.uint32)) == REF.NO_ROW).all()
    rows = np.array([[0, 0, 0], [-0.0, 0, -0.0], [0, 0, 1e-45], [0, np.nan, 0], [1, 2, 3]], np.float32)
    out = REF.zero_rows_to_nan(rows)
    assert np.isnan(out[:2]).all() and np.array_equal(out[2:].view(np.uint32), rows[2:].view(np.uint32))
    assert rows[2, 2] != 0                                               # the smallest subnormal is not a zero


def test_apply_many_reference():
    p = np.random.default_rng(0).normal(size=(5, 3))
    Ts = REF.transforms(10, 0)
    got = REF.apply_many(p, Ts)
    assert got.shape == (10, 5, 3)
    for k in range(10):
        want = np.stack([Ts[k, :3, :3] @ x + Ts[k, :3, 3] for x in p])
        np.testing.assert_allclose(got[k], want, rtol=1e-13, atol=1e-9)
    assert np.array_equal(Ts[3], np.eye(4)) and abs(Ts[2, :3, 3]).min() >= 1e6
    sv = np.linalg.svd(Ts[1, :3, :3])[1]
    assert sv.max() - sv.min() > 1                                       # not a similarity
    assert REF.apply_many(p, np.zeros((0, 4, 4))).shape == (0, 5, 3)


# ---- the entry points, without a device --------------------------------------------------------------------------------
def test_new_symbol_resolves():
    L = importlib.import_module(PKG + "._lib")
    lib = L.load()
    assert "r3d_select_quantile_classes_f32" in L.SIGNATURES
    fn = lib.r3d_select_quantile_classes_f32
    assert fn.restype is C.c_int and len(fn.argtypes) == 9


def test_entry_points_reject_a_null_context():
    L = importlib.import_module(PKG + "._lib")
    lib = L.load()
    vals, counts = (C.c_float * 32)(*[-7.0] * 32), (C.c_int64 * 32)(*[-7] * 32)
    means = (C.c_double * 32)(*[-7.0] * 32)
    T = np.eye(4)
    calls = [
        lambda: lib.r3d_select_quantile_classes_f32(None, None, None, 24, 10, 0, 0.5, vals, counts),
        lambda: lib.r3d_select_quantile_f32(None, None, 0, 0.5, vals, counts),
        lambda: lib.r3d_select_quantile_f32_dev(None, None, 0, 0.5, None),
        lambda: lib.r3d_trimmed_means_f32(None, None, 4, 8, 0.5, means),
        lambda: lib.r3d_apply_T_many(None, None, L.F32, 0, T.ctypes.data, 1, None, L.F32),
        lambda: lib.r3d_apply_T_dev(None, None, L.F32, 0, T.ctypes.data, None, L.F32),
        lambda: lib.r3d_apply_T_dev(None, None, L.F32, 0, None, None, L.F32),
        lambda: lib.r3d_gather_rows(None, None, 0, None, 0, None),
        lambda: lib.r3d_gather_rows_strided(None, None, 0, 0, 1, 0, None),
        lambda: lib.r3d_permutation_invert(None, None, 0, None),
        lambda: lib.r3d_remap_u32(None, None, 0, None, 0),
        lambda: lib.r3d_cloud_zero_rows_to_nan(None, None, 0),
    ]
    for k, call in enumerate(calls):
        assert call() == L.ERR_INVALID, k
        assert "NULL" in L.last_error(), (k, L.last_error())
    assert list(vals) == [-7.0] * 32 and list(counts) == [-7] * 32 and list(means) == [-7.0] * 32
