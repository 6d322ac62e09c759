"""GPU: the small entry points the ICP driver is built from (include/r3d_internal_api.h), each called directly with the plain
NumPy reference of tests/icp_parts_ref.py beside it -- the whole-estimator tests only see them through a converged pose, which
a robust estimator reaches with a slightly wrong helper too.

  * per-class selection (select_count / select_pick_all of csrc/r3d_plane.hip) through the test hook
    r3d_select_quantile_classes_f32: both class modes, class counts up to the limit of 32, uneven populations, value sets that
    isolate each 8-bit digit of the order key; the workspace's "histogram is zero" record across changing class counts;
  * r3d_select_quantile_f32_dev, r3d_trimmed_means_f32 (class_sum_below_kernel);
  * r3d_apply_T_many (apply_many_kernel and the loop over apply_common), r3d_apply_T_dev;
  * r3d_gather_rows, r3d_gather_rows_strided, r3d_permutation_invert, r3d_remap_u32, r3d_cloud_zero_rows_to_nan.

Every device buffer is a `Guarded` of tests/test_gpu_bounds.py: 1 MiB bands on both sides that must come back intact, payloads
at offsets that are not 16-byte aligned."""
import ctypes as C
import importlib

import numpy as np
import pytest

import icp_parts_ref as REF
from helpers import PKG, r3d as _r3d
from oracle import fusion_ref as O
from oracle import plane_ref as PR
from test_gpu_bounds import G, Guarded, guard  # noqa: F401  (guard is a fixture)
from test_gpu_fusion import check

pytestmark = pytest.mark.gpu

QS = (0.0, 0.3, 0.5, 0.8, 1.0)
CLASS_COUNTS = [1, 3, 4, 5, 24, 31, 32]
SIZES = [1, 255, REF.PASS_SPAN - 1, REF.PASS_SPAN + 1, 20011]
DTYPE_PAIRS = [(np.float32, np.float32), (np.float64, np.float64), (np.float32, np.float64), (np.float64, np.float32)]
ROW_SIZES = [1, 255, 256, 257, 3 * 256 + 17]
OFFSETS = (0, 4, 12)


@pytest.fixture(scope="module")
def R():
    return _r3d()


@pytest.fixture(scope="module")
def L(R):
    return importlib.import_module(PKG + "._lib")


@pytest.fixture(scope="module")
def ctx(R):
    c = R.Context(0)
    yield c
    c.close()


def code(L, dt):
    return L.F32 if dt == np.float32 else L.F64


def xyz_off(dt):
    return 4 if dt == np.float32 else 8


def payload(g):
    """What a Guarded's payload held when it was uploaded."""
    return g.pattern[G + g.off:G + g.off + g.nbytes].copy()


# ---- per-class selection -----------------------------------------------------------------------------------------------
def select_classes(ctx, L, d_values, d_class, n_classes, per_class, n, q):
    vals, counts = np.full(REF.MAX_CLASSES + 1, -7, np.float32), np.full(REF.MAX_CLASSES + 1, -7, np.int64)
    L.check(ctx.lib.r3d_select_quantile_classes_f32(ctx.handle, d_values, d_class, n_classes, per_class, n, q, vals.ctypes.data,
                                                    counts.ctypes.data))
    assert (vals[n_classes:] == -7).all() and (counts[n_classes:] == -7).all()       # n_classes results, not one more
    return vals[:n_classes].copy(), counts[:n_classes].copy()


def assert_selection(got, want, what):
    np.testing.assert_array_equal(got[1], want[1], err_msg="finite counts, %s" % (what,))
    assert REF.same_selection(got[0], want[0]), (what, got[0], want[0])


@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("n_classes", CLASS_COUNTS)
def test_selection_by_class_byte(ctx, L, guard, n_classes, n):
    """A class byte per element (as the 24 direction classes of the point-to-plane sums): bytes >= n_classes and 255 take part in
    no class; empty classes between full ones, a class of one element, a class of NaN / +-inf only, a class of one repeated
    value.  Selected value bitwise (a zero of either sign), finite count exact."""
    for kind in sorted(REF.VALUE_SETS):
        v, cls = REF.class_case(n, n_classes, kind, 0)
        dv, dc = guard(v.nbytes, 4, v), guard(cls.nbytes, 3, cls, seed=1)
        for q in QS:
            got = select_classes(ctx, L, dv.ptr, dc.ptr, n_classes, 0, n, q)
            assert_selection(got, REF.class_quantiles(v, cls, n_classes, q), (kind, q))
        dv.unchanged()
        dc.unchanged()


@pytest.mark.parametrize("per_class", [1, 63, 64, 65, 1000])
@pytest.mark.parametrize("n_classes", CLASS_COUNTS)
def test_selection_by_contiguous_block(ctx, L, guard, n_classes, per_class):
    """Class = i / per_class (r3d_trimmed_means_f32's mode) for every total size: the last block is cut short, blocks from
    n_classes on belong to no class, classes the cloud does not reach are empty."""
    for n in SIZES:
        v = REF.mixed_values(n, per_class)
        if n >= 3 * per_class:
            v[per_class:2 * per_class] = np.nan                          # an empty class between full ones
            v[2 * per_class:3 * per_class] = np.float32(0.75)            # a class of one repeated value
        cls = REF.block_classes(n, per_class)
        dv = guard(v.nbytes, 4, v)
        for q in QS:
            got = select_classes(ctx, L, dv.ptr, None, n_classes, per_class, n, q)
            assert_selection(got, REF.class_quantiles(v, cls, n_classes, q), (n, q))
        dv.unchanged()


def test_selection_hook_checks_its_arguments(ctx, L, guard):
    v = guard(64, 4, np.arange(16, dtype=np.float32))
    c = guard(16, 1, np.zeros(16, np.uint8))
    vals, counts = np.full(33, -7, np.float32), np.full(33, -7, np.int64)

    def call(d_v, d_c, n_classes, per_class, n, q, hv=vals.ctypes.data, hc=counts.ctypes.data):
        return ctx.lib.r3d_select_quantile_classes_f32(ctx.handle, d_v, d_c, n_classes, per_class, n, q, hv, hc)
    for args in ((v.ptr, c.ptr, 0, 0, 16, 0.5), (v.ptr, c.ptr, 33, 0, 16, 0.5), (v.ptr, None, 4, 0, 16, 0.5), (v.ptr, None, 4, -1, 16, 0.5),
                 (v.ptr, c.ptr, 4, 4, 16, 0.5), (v.ptr, c.ptr, 4, 0, -1, 0.5), (v.ptr, c.ptr, 4, 0, 1 << 31, 0.5), (None, c.ptr, 4, 0, 16, 0.5),
                 (v.ptr, c.ptr, 4, 0, 16, -0.1), (v.ptr, c.ptr, 4, 0, 16, 1.5), (v.ptr, c.ptr, 4, 0, 16, float("nan"))):
        assert call(*args) == L.ERR_INVALID, args
    assert call(v.ptr, c.ptr, 4, 0, 16, 0.5, None) == L.ERR_INVALID and call(v.ptr, c.ptr, 4, 0, 16, 0.5, vals.ctypes.data, None) == L.ERR_INVALID
    assert (vals == -7).all() and (counts == -7).all()
    got = select_classes(ctx, L, None, None, 3, 5, 0, 0.5)               # nothing to rank: +inf and 0 for every class
    assert np.isposinf(got[0]).all() and not got[1].any()
    v.unchanged()
    c.unchanged()


# ---- the workspace record across class counts ----------------------------------------------------------------------------
def quantile_host(ctx, L, d_values, n, q):
    v, m = C.c_float(-7), C.c_int64(-7)
    L.check(ctx.lib.r3d_select_quantile_f32(ctx.handle, d_values, n, q, C.byref(v), C.byref(m)))
    return np.float32(v.value), m.value


def trimmed(ctx, L, d_values, n_classes, per_class, keep):
    out = np.full(REF.MAX_CLASSES + 1, -7.0)
    L.check(ctx.lib.r3d_trimmed_means_f32(ctx.handle, d_values, n_classes, per_class, keep, out.ctypes.data))
    assert (out[n_classes:] == -7).all()
    return out[:n_classes].copy()


def assert_trimmed(got, v, n_classes, per_class, keep, what=""):
    """|got - want| <= 1e-12 mean|kept values|: at most 5000 fp64 addends per block in another order than the reference's
    (5000 x 2^-53 = 5.6e-13 of the mean magnitude); +inf exactly for a block without finite values."""
    want, scale = REF.trimmed_means(v, n_classes, per_class, keep)
    dead = np.isinf(want)
    np.testing.assert_array_equal(np.isposinf(got), dead, err_msg=str(what))
    err = np.abs(got[~dead] - want[~dead])
    assert (err <= 1e-12 * scale[~dead]).all(), (what, keep, err, scale[~dead])


def test_selection_sequences_on_one_ctx(R, L):
    """24 -> 1 -> 32 -> 5 -> 24 -> 24 classes on one fresh context, twice with the entry points swapped (the hook in both class
    modes, r3d_trimmed_means_f32, r3d_select_quantile_f32 and its _dev form): every layout puts state words, picks or partial
    sums where another one keeps the histogram it presumes to be zero.  Every result against the reference, the second and
    third 24-class result bitwise the first.  On the fresh context the 32-class call is also the first to outgrow
    kWsSelect; afterwards an untrimmed 29-sums call over 65536 pairs (one partial row per workgroup: ~59 KB against the 32-class
    layout's 34 KB) and the largest n_classes x per_class so far make it grow again, and both rounds must repeat bit for bit."""
    c = R.Context(0)
    bufs = []

    def dev(a, off):
        bufs.append(Guarded(c, a.nbytes, off, a, seed=len(bufs)))
        return bufs[-1]
    try:
        vA, clsA = REF.class_case(20011, 24, "wall", 5)
        vB = REF.mixed_values(3000, 1)
        vC, _ = REF.trimmed_case(32, 100, 0)
        v5 = REF.mixed_values(5 * 65, 2)
        vT, _ = REF.trimmed_case(24, 257, 1)
        dA, dclsA, dB, dC, d5, dT = dev(vA, 4), dev(clsA, 1), dev(vB, 4), dev(vC, 12), dev(v5, 4), dev(vT, 4)
        out8 = Guarded(c, 8, 4, seed=99)
        bufs.append(out8)

        def hook24():
            got = select_classes(c, L, dA.ptr, dclsA.ptr, 24, 0, vA.size, 0.5)
            assert_selection(got, REF.class_quantiles(vA, clsA, 24, 0.5), "hook24")
            return got[0].tobytes() + got[1].tobytes()

        def q1():
            got = quantile_host(c, L, dB.ptr, vB.size, 0.3)
            want = PR.quantile_lower(vB, 0.3)
            assert got[1] == want[1] and REF.same_selection([got[0]], [want[0]])
            return np.float32(got[0]).tobytes()

        def q1_dev():
            L.check(c.lib.r3d_select_quantile_f32_dev(c.handle, dB.ptr, vB.size, 0.3, out8.ptr))
            raw = out8.bytes()
            want = PR.quantile_lower(vB, 0.3)
            assert raw[4:].view(np.uint32)[0] == want[1] and REF.same_selection(raw[:4].view(np.float32), [want[0]])
            return raw.tobytes()

        def tm(d, v, n_classes, per_class, keep):
            got = trimmed(c, L, d.ptr, n_classes, per_class, keep)
            assert_trimmed(got, v, n_classes, per_class, keep, ("sequence", n_classes))
            return got.tobytes()

        def hook_blocks(d, v, n_classes, per_class, q):
            got = select_classes(c, L, d.ptr, None, n_classes, per_class, v.size, q)
            assert_selection(got, REF.class_quantiles(v, REF.block_classes(v.size, per_class), n_classes, q), ("blocks", n_classes))
            return got[0].tobytes() + got[1].tobytes()

        tm24 = lambda: tm(dT, vT, 24, 257, 0.5)                          # noqa: E731
        rounds = [[hook24, q1, lambda: tm(dC, vC, 32, 100, 0.8), lambda: hook_blocks(d5, v5, 5, 65, 0.5), hook24, hook24],
                  [tm24, q1_dev, lambda: hook_blocks(dC, vC, 32, 100, 0.8), lambda: tm(d5, v5, 5, 65, 0.5), tm24, tm24]]

        def run():
            res = [[step() for step in steps] for steps in rounds]
            for r in res:
                assert r[4] == r[0] and r[5] == r[0]
            return res
        first = run()
        # kWsSelect grows: the untrimmed 29 sums keep one fp64 row per workgroup behind the 1-class head ...
        n_src = 65536
        src, idx = c.alloc(n_src * 12), c.alloc(n_src * 4)
        one, sums = c.alloc(64), c.alloc(29 * 8)
        L.check(c.lib.r3d_memset(c.handle, src.ptr, 0, n_src * 12))
        L.check(c.lib.r3d_memset(c.handle, idx.ptr, 0xff, n_src * 4))    # every match out of range: no pair is admissible
        L.check(c.lib.r3d_memset(c.handle, one.ptr, 0, 64))
        L.check(c.lib.r3d_icp_plane_accumulate(c.handle, src.ptr, n_src, one.ptr, one.ptr, 1, idx.ptr, None, -1.0, 0.0, 1.0, sums.ptr))
        assert not sums.download(np.float64, 29).any()
        for b in (src, idx, one, sums):
            b.free()
        # ... and a larger n_classes x per_class than any call before
        vBig, _ = REF.trimmed_case(32, 5000, 2)
        dBig = dev(vBig, 4)
        assert_trimmed(trimmed(c, L, dBig.ptr, 32, 5000, 0.5), vBig, 32, 5000, 0.5, "big")
        assert run() == first
        for b in bufs:
            if b is not out8:
                b.unchanged()
    finally:
        for b in bufs:
            b.free()
        c.close()


@pytest.mark.parametrize("n", [0, 1, 1000])
def test_select_quantile_dev_leaves_the_host_call_s_eight_bytes(ctx, L, guard, n):
    v = REF.mixed_values(n, 7)
    dv = guard(v.nbytes, 4, v)
    for q in QS:
        out = guard(8, 4, seed=int(q * 10))
        L.check(ctx.lib.r3d_select_quantile_f32_dev(ctx.handle, dv.ptr if n else None, n, q, out.ptr))
        raw = out.bytes()
        val, cnt = quantile_host(ctx, L, dv.ptr if n else None, n, q)
        assert raw[:4].view(np.uint32)[0] == np.float32(val).view(np.uint32) and raw[4:].view(np.uint32)[0] == cnt
        want = PR.quantile_lower(v, q)
        assert cnt == want[1] and REF.same_selection([val], [want[0]])
    dv.unchanged()


# ---- r3d_trimmed_means_f32 -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("per_class", [1, 7, 255, 256, 257, 5000])
@pytest.mark.parametrize("n_classes", [1, 2, 10, 32])
def test_trimmed_means(ctx, L, guard, n_classes, per_class):
    """One 256-thread workgroup per block: blocks shorter than, equal to and one longer than the workgroup.  Squared-distance
    like and mixed-sign blocks, blocks without a finite value (+inf), a statistic that ties with most of its block (all of them
    count), -0.0 and +0.0 around the statistic (the comparison is arithmetic)."""
    kinds_seen = set()
    for shift in (range(len(REF.BLOCK_KINDS)) if n_classes < len(REF.BLOCK_KINDS) else (0,)):
        v, kinds = REF.trimmed_case(n_classes, per_class, shift)
        kinds_seen |= set(kinds)
        dv = guard(v.nbytes, 4, v, seed=shift)
        for keep in (0.0, 0.5, 0.8, 1.0):
            assert_trimmed(trimmed(ctx, L, dv.ptr, n_classes, per_class, keep), v, n_classes, per_class, keep, kinds)
        dv.unchanged()
    assert kinds_seen == set(REF.BLOCK_KINDS)


def test_trimmed_means_argument_errors(ctx, L, guard):
    v = guard(33 * 4 * 4, 4, np.ones(33 * 4, np.float32))
    out = np.full(34, -7.0)
    for n_classes, per_class, keep in ((0, 4, 0.5), (33, 4, 0.5), (-1, 4, 0.5), (4, 0, 0.5), (4, -3, 0.5), (4, 4, -0.01), (4, 4, 1.01),
                                       (4, 4, float("nan"))):
        assert ctx.lib.r3d_trimmed_means_f32(ctx.handle, v.ptr, n_classes, per_class, keep, out.ctypes.data) == L.ERR_INVALID
    assert ctx.lib.r3d_trimmed_means_f32(ctx.handle, None, 4, 4, 0.5, out.ctypes.data) == L.ERR_INVALID
    assert ctx.lib.r3d_trimmed_means_f32(ctx.handle, v.ptr, 4, 4, 0.5, None) == L.ERR_INVALID
    assert (out == -7).all()
    v.unchanged()


# ---- r3d_apply_T_many / r3d_apply_T_dev -----------------------------------------------------------------------------------
def apply_many(ctx, L, d_in, idt, n, Ts, d_out, odt):
    Ts = np.ascontiguousarray(Ts, np.float64)
    return ctx.lib.r3d_apply_T_many(ctx.handle, d_in, code(L, idt), n, Ts.ctypes.data, len(Ts), d_out, code(L, odt))


def apply_one(ctx, L, d_in, idt, n, T, d_out, odt):
    T = np.ascontiguousarray(T, np.float64)
    return ctx.lib.r3d_apply_T(ctx.handle, d_in, code(L, idt), n, T.ctypes.data, d_out, code(L, odt))


@pytest.mark.parametrize("k", [1, 2, 10])
@pytest.mark.parametrize("n", [1, 255, 256, 257, 1025])
@pytest.mark.parametrize("idt,odt", DTYPE_PAIRS)
def test_apply_many_blocks_are_single_applies(ctx, L, guard, idt, odt, n, k):
    """Block k bitwise what r3d_apply_T writes for Ts[k] (f32 -> f32: the 2-D grid kernel against the tiled one, the same
    out_row arithmetic; the other dtype pairs: the loop over blocks), and within the apply tolerance of the oracle.  Among the
    transforms: an anisotropic scale with shear, a translation of 1e6."""
    rng = np.random.default_rng([n, k, np.dtype(idt).itemsize, np.dtype(odt).itemsize])
    p = (rng.normal(size=(n, 3)) * 50).astype(idt)
    Ts = REF.transforms(k, n)
    want = REF.apply_many(p, Ts)
    osz = np.dtype(odt).itemsize
    src = guard(p.nbytes, xyz_off(idt), p)
    out = guard(k * n * 3 * osz, 12 if odt == np.float32 else 8, seed=1)
    L.check(apply_many(ctx, L, src.ptr, idt, n, Ts, out.ptr, odt))
    got = out.read(odt, (k, n, 3))
    single = guard(n * 3 * osz, xyz_off(odt), seed=2)
    for j in range(k):
        L.check(apply_one(ctx, L, src.ptr, idt, n, Ts[j], single.ptr, odt))
        np.testing.assert_array_equal(got[j].view(np.uint8), single.read(odt, (n, 3)).view(np.uint8), err_msg="block %d" % j)
        check(got[j], want[j], odt)
    src.unchanged()


def test_apply_many_at_the_grid_limit(ctx, L, guard):
    """65535 transforms: the last count the 2-D grid takes (gridDim.y); 65536: the first that goes block by block.  Two points
    each, f32 -> f32; every block against the oracle, the two paths bitwise against each other, sampled blocks bitwise against
    r3d_apply_T."""
    n, kmax = 2, 65536
    rng = np.random.default_rng(65535)
    p = (rng.normal(size=(n, 3)) * 50).astype(np.float32)
    Ts = np.tile(np.eye(4), (kmax, 1, 1))
    Ts[:, :3, :] = rng.normal(size=(kmax, 3, 4))
    want = REF.apply_many(p, Ts)
    src = guard(p.nbytes, 4, p)
    got = {}
    for k in (kmax - 1, kmax):
        out = guard(k * n * 12, 12, seed=k)
        L.check(apply_many(ctx, L, src.ptr, np.float32, n, Ts[:k], out.ptr, np.float32))
        got[k] = out.read(np.float32, (k, n, 3))
        check(got[k].reshape(-1, 3), want[:k].reshape(-1, 3), np.float32)
    np.testing.assert_array_equal(got[kmax - 1].view(np.uint32), got[kmax][:kmax - 1].view(np.uint32))
    single = guard(n * 12, 4, seed=2)
    for j in (0, 1, 255, 256, 32768, kmax - 2, kmax - 1):
        L.check(apply_one(ctx, L, src.ptr, np.float32, n, Ts[j], single.ptr, np.float32))
        np.testing.assert_array_equal(got[kmax][j].view(np.uint32), single.read(np.float32, (n, 3)).view(np.uint32))
    src.unchanged()


@pytest.mark.parametrize("idt,odt", DTYPE_PAIRS)
def test_apply_many_no_ops(ctx, L, guard, idt, odt):
    p = np.ones((5, 3), idt)
    src, out = guard(p.nbytes, xyz_off(idt), p), guard(256, xyz_off(odt), seed=1)
    L.check(apply_many(ctx, L, src.ptr, idt, 5, np.zeros((0, 4, 4)), out.ptr, odt))
    L.check(ctx.lib.r3d_apply_T_many(ctx.handle, src.ptr, code(L, idt), 5, None, 0, out.ptr, code(L, odt)))
    L.check(apply_many(ctx, L, src.ptr, idt, 0, REF.transforms(3, 0), out.ptr, odt))
    out.unchanged()
    src.unchanged()


@pytest.mark.parametrize("n,k", [(1, 3), (257, 3), (1, 65536)])
@pytest.mark.parametrize("idt,odt", DTYPE_PAIRS)
def test_apply_many_refuses_an_output_that_overlaps_its_input(ctx, L, guard, idt, odt, n, k):
    """The k n rows of output must not contain the input cloud at ANY offset -- not only at offset 0: the copies would overwrite
    the cloud while other workgroups (or later blocks) still read it.  R3D_ERR_INVALID, nothing written, in every dtype pair and
    on both sides of the 65535-transform switch.  Ranges that merely touch are served."""
    rng = np.random.default_rng([n, k])
    p = (rng.normal(size=(n, 3)) * 50).astype(idt)
    Ts = REF.transforms(3, 1) if k == 3 else np.tile(np.eye(4), (k, 1, 1))
    ib, block = p.nbytes, n * 3 * np.dtype(odt).itemsize
    ob = k * block
    room = guard(ib + ob + ib + 64, 8, seed=5)
    lead = (ib + 15) // 8 * 8
    out = room.ptr + lead                                                # the output; inputs are tried around and inside it
    before = room.bytes()
    inside = [block, 12, 3 * np.dtype(idt).itemsize, ob - 4, 4 - ib]     # block 1; 12 bytes in; one point in; across either end
    for s in inside:
        if not -ib < s < ob:
            continue
        assert apply_many(ctx, L, out + s, idt, n, Ts, out, odt) == L.ERR_INVALID, s
        assert "overlap" in L.last_error()
    assert apply_many(ctx, L, out, idt, n, Ts, out, odt) == L.ERR_INVALID
    np.testing.assert_array_equal(room.bytes(), before)
    if k == 3:                                                           # the input right in front of / right behind the output
        for s in (-ib, ob):
            if (out + s) % np.dtype(idt).itemsize:                       # f64 rows behind 36 n bytes of f32 output: not a legal pointer
                continue
            L.check(ctx.lib.r3d_memcpy_h2d(ctx.handle, out + s, p.ctypes.data, ib))
            L.check(apply_many(ctx, L, out + s, idt, n, Ts, out, odt))
            raw = room.bytes()
            got = raw[lead:lead + ob].view(odt).reshape(k, n, 3)
            for j in range(k):
                check(got[j], O.apply_T(p, Ts[j]), odt)
            np.testing.assert_array_equal(raw[lead + s:lead + s + ib], p.reshape(-1).view(np.uint8))


@pytest.mark.parametrize("n", [1, 1023, 1025])
@pytest.mark.parametrize("idt,odt", DTYPE_PAIRS)
def test_apply_T_dev_is_apply_T_with_the_matrix_in_hbm(ctx, L, guard, idt, odt, n):
    rng = np.random.default_rng([n, 3, np.dtype(idt).itemsize, np.dtype(odt).itemsize])
    p = (rng.normal(size=(n, 3)) * 50).astype(idt)
    osz = np.dtype(odt).itemsize
    src = guard(p.nbytes, xyz_off(idt), p)
    for T in REF.transforms(3, n):
        d_T = guard(128, 8, T, seed=4)
        a, b = guard(n * 3 * osz, xyz_off(odt), seed=1), guard(n * 3 * osz, 12 if odt == np.float32 else 8, seed=2)
        L.check(apply_one(ctx, L, src.ptr, idt, n, T, a.ptr, odt))
        L.check(ctx.lib.r3d_apply_T_dev(ctx.handle, src.ptr, code(L, idt), n, d_T.ptr, b.ptr, code(L, odt)))
        ref = a.read(odt, (n, 3))
        np.testing.assert_array_equal(b.read(odt, (n, 3)).view(np.uint8), ref.view(np.uint8))
        check(ref, O.apply_T(p, T), odt)
        d_T.unchanged()
    src.unchanged()


# ---- row movers ------------------------------------------------------------------------------------------------------------
def assert_rows(got, want):
    """NaN rows where the reference has them (all three components), every other row bit for bit."""
    nan = np.isnan(want).all(axis=1)
    assert np.isnan(got[nan]).all()
    np.testing.assert_array_equal(got[~nan].view(np.uint32), want[~nan].view(np.uint32))


@pytest.mark.parametrize("n_out", ROW_SIZES)
def test_gather_rows(ctx, L, guard, n_out):
    rng = np.random.default_rng(n_out)
    cases = {}
    n_pts = 300
    rows = rng.integers(0, n_pts, n_out).astype(np.uint32)
    cases["permutation"] = (n_out, rng.permutation(n_out).astype(np.uint32))
    cases["repeats"] = (n_pts, rows)
    oob = rows.copy()
    oob[rng.integers(0, n_out, max(1, n_out // 5))] = rng.choice(np.array([n_pts, n_pts + 1, 0xffffffff], np.uint32), max(1, n_out // 5))
    oob[-1], oob[0] = n_pts, 0xffffffff
    cases["out_of_range"] = (n_pts, oob)
    cases["empty_cloud"] = (0, np.concatenate([rows[:n_out // 2], oob[n_out // 2:]]))
    for name, (n_points, idx) in cases.items():
        xyz = rng.normal(size=(n_points, 3)).astype(np.float32)
        want = REF.gather_rows(xyz, idx)
        assert name not in ("out_of_range", "empty_cloud") or np.isnan(want).any()
        src, d_idx = guard(xyz.nbytes, 4, xyz), guard(idx.nbytes, 4, idx, seed=1)
        for off in OFFSETS:
            out = guard(n_out * 12, off, seed=2)
            L.check(ctx.lib.r3d_gather_rows(ctx.handle, src.ptr, n_points, d_idx.ptr, n_out, out.ptr))
            assert_rows(out.read(np.float32, (n_out, 3)), want)
        src.unchanged()
        d_idx.unchanged()


@pytest.mark.parametrize("n_out", ROW_SIZES)
def test_gather_rows_strided(ctx, L, guard, n_out):
    rng = np.random.default_rng(n_out + 1000)
    picks = [(0, 1, n_out), (1, 2, n_out), (5, 7, n_out), (n_out - 1, 1, 1)]
    for first, step, m in picks:
        n_points = first + (m - 1) * step + 1                            # the selection's last row is the cloud's last row
        xyz = rng.normal(size=(n_points, 3)).astype(np.float32)
        want = REF.gather_rows_strided(xyz, first, step, m)
        src = guard(xyz.nbytes, 12, xyz)
        for off in OFFSETS:
            out = guard(m * 12, off, seed=2)
            L.check(ctx.lib.r3d_gather_rows_strided(ctx.handle, src.ptr, n_points, first, step, m, out.ptr))
            np.testing.assert_array_equal(out.read(np.float32, (m, 3)).view(np.uint32), want.view(np.uint32))
        out = guard(m * 12, 4, seed=3)
        for bad in ((n_points - 1, first, step, m), (n_points, first + 1, step, m), (n_points, first, step + 1, m + 1),
                    (n_points, first, 0, m), (n_points, -1, step, m), (n_points, first, -step, m), (n_points, first, step, -1)):
            assert ctx.lib.r3d_gather_rows_strided(ctx.handle, src.ptr, bad[0], bad[1], bad[2], bad[3], out.ptr) == L.ERR_INVALID, bad
        out.unchanged()
        src.unchanged()


@pytest.mark.parametrize("n", ROW_SIZES)
def test_permutation_invert(ctx, L, guard, n):
    rng = np.random.default_rng(n + 2000)
    perm = rng.permutation(n).astype(np.uint32)
    holes = perm.copy()
    holes[rng.integers(0, n, max(1, n // 7))] = rng.choice(np.array([n, n + 1, 0xffffffff], np.uint32), max(1, n // 7))
    holes[0] = n
    for p in (perm, holes):
        d_perm = guard(p.nbytes, 4, p)
        for off in OFFSETS:
            out = guard(n * 4, off, seed=off)
            previous = payload(out).view(np.uint32)
            L.check(ctx.lib.r3d_permutation_invert(ctx.handle, d_perm.ptr, n, out.ptr))
            got = out.read(np.uint32)
            np.testing.assert_array_equal(got, REF.permutation_invert(p, previous))     # skipped entries: the slot keeps the pattern
            if p is perm:
                np.testing.assert_array_equal(got[p], np.arange(n, dtype=np.uint32))
        assert ctx.lib.r3d_permutation_invert(ctx.handle, d_perm.ptr, n, d_perm.ptr) == L.ERR_INVALID
        d_perm.unchanged()


@pytest.mark.parametrize("n", ROW_SIZES)
def test_remap_u32_in_place(ctx, L, guard, n):
    rng = np.random.default_rng(n + 3000)
    for n_table in (0, 1, 300):
        table = rng.integers(0, 1 << 32, n_table, dtype=np.uint64).astype(np.uint32)
        vals = rng.integers(0, max(n_table, 1), n).astype(np.uint32)
        vals[rng.integers(0, n, max(1, n // 5))] = rng.choice(np.array([n_table, n_table + 1, 0xffffffff], np.uint32), max(1, n // 5))
        vals[0], vals[-1] = n_table, 0xffffffff if n > 1 else n_table
        want = REF.remap(vals, table)
        assert n_table or (want == REF.NO_ROW).all()
        d_table = guard(table.nbytes, 4, table, seed=1)
        for off in OFFSETS:
            d_vals = guard(vals.nbytes, off, vals, seed=2)
            L.check(ctx.lib.r3d_remap_u32(ctx.handle, d_vals.ptr, n, d_table.ptr, n_table))
            np.testing.assert_array_equal(d_vals.read(np.uint32), want)
        d_table.unchanged()


@pytest.mark.parametrize("n", [1, 256, 257])
def test_zero_rows_to_nan(ctx, L, guard, n):
    """(0,0,0) and (-0,0,-0) become NaN rows; (0,0,1e-45), (0,NaN,0) and ordinary points keep their bits."""
    rng = np.random.default_rng(n)
    special = np.array([[0, 0, 0], [-0.0, 0, -0.0], [0, 0, 1e-45], [0, np.nan, 0], [0, -0.0, 0], [1e-45, 0, 0], [0, np.inf, 0]], np.float32)
    for start in range(len(special) if n == 1 else 1):
        xyz = rng.normal(size=(n, 3)).astype(np.float32)
        k = np.arange(start, n + start, 3 if n > 1 else 1)
        xyz[k - start] = special[(k // 3 if n > 1 else k) % len(special)]
        want = REF.zero_rows_to_nan(xyz)
        for off in OFFSETS:
            buf = guard(xyz.nbytes, off, xyz, seed=off)
            L.check(ctx.lib.r3d_cloud_zero_rows_to_nan(ctx.handle, buf.ptr, n))
            got = buf.read(np.float32, (n, 3))
            became = np.isnan(want).all(axis=1) & ~np.isnan(xyz).all(axis=1)
            assert np.isnan(got[became]).all() and (n == 1 or became.sum() >= 2 * (n // 21))
            np.testing.assert_array_equal(got[~became].view(np.uint32), xyz[~became].view(np.uint32))
