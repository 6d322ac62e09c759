"""GPU: the three device primitives under the map-side features, each against the plain references of tests/sort_ref.py and
bit for bit -- there is no tolerance in this file:

  * the LSD radix sort (csrc/r3d_sort.hip) through r3d_sort_u64 and, for the bit range the NN index uses, r3d_sort_u64_bits:
    STABILITY (keys whose compared bits agree keep their input order; every key here carries its input position or random
    bits outside the compared span, so any other order among equal keys changes the words), the span's rounding to whole
    digits, pass counts 1..8 (copy-back and in-place parities), digit distributions that load one bin, one wave or one wave
    round, sorted input;
  * the tile-counter scan (digit_scan_kernel) across its 1024-counter segments, with 256 rows (sort) and with one (selection);
  * the order-preserving row selection (r3d_select_rows) at the same sizes, outputs inside guarded allocations.

The workspace kWsCounts is shared by all of them and only ever grows: the stale-workspace tests run a small job behind a large one
on ONE context, so the small job's padding counters hold the large job's numbers.

tests/test_sort_host.py checks, without a device, that every input used here has the property it is named for.
"""
import importlib

import numpy as np
import pytest

import sort_ref as REF
from helpers import PKG, r3d as _r3d
from oracle import octomap_ref as OM
from test_gpu_bounds import Guarded

pytestmark = pytest.mark.gpu

U = np.uint64
TILE = REF.TILE


@pytest.fixture(scope="module")
def R():
    return _r3d()


@pytest.fixture(scope="module")
def L(R):
    return importlib.import_module(PKG + "._lib")


@pytest.fixture(scope="module")
def O(R):
    return importlib.import_module(PKG + ".outliers")


@pytest.fixture(scope="module")
def ctx(R):
    c = R.Context(0)
    yield c
    c.close()


def same(got, want, what=""):
    """bit-for-bit equality with a message that says what kind of difference it is"""
    assert got.shape == want.shape, (what, got.shape, want.shape)
    if np.array_equal(got, want):
        return
    bad = np.flatnonzero(got != want)
    perm = np.array_equal(np.sort(got, axis=None), np.sort(want, axis=None))
    i = int(bad[0])
    raise AssertionError("%s: %d of %d elements differ, first at %d (got %#x, want %#x); %s"
                         % (what, bad.size, got.size, i, int(got.reshape(-1)[i]), int(want.reshape(-1)[i]),
                            "the same words in another order" if perm else "NOT a permutation of the input: words lost or made up"))


def device_sort(ctx, L, keys, first_bit, end_bit, entry="bits"):
    """keys sorted on the device; buffers up to a few tiles sit between guard bands"""
    n = keys.shape[0]
    call = (lambda p: ctx.lib.r3d_sort_u64(ctx.handle, p, n, end_bit)) if entry == "public" else \
           (lambda p: ctx.lib.r3d_sort_u64_bits(ctx.handle, p, n, first_bit, end_bit))
    if 0 < n <= 8 * TILE:
        g = Guarded(ctx, n * 8, 8, keys, seed=n)
        try:
            L.check(call(g.ptr))
            return g.read(np.uint64)
        finally:
            g.free()
    buf = ctx.alloc(max(n * 8, 16))
    try:
        if n:
            buf.upload(keys)
        L.check(call(buf.ptr))
        return buf.download(np.uint64, n)
    finally:
        buf.free()


def check_sort(ctx, L, keys, first_bit, end_bit, entry="bits", what=""):
    got = device_sort(ctx, L, keys, first_bit, end_bit, entry)
    same(got, REF.stable_sort_by_bits(keys, first_bit, end_bit), "%s bits [%d, %d) n=%d" % (what, first_bit, end_bit, keys.shape[0]))
    return got


# ---- stability through the public entry -----------------------------------------------------------------------------------
# (key_bits = 8 sorts exactly 8 bits, which hold at most 256 values: 257 runs with the wider spans only)
PUBLIC_CASES = [(kb, d) for kb in (8, 16, 20, 40) for d in (2, 3, 256, 257) if d <= 1 << REF.span(0, kb)[2]]


@pytest.mark.parametrize("n", [7 * 4096 + 1, 1_500_000])
@pytest.mark.parametrize("key_bits,distinct", PUBLIC_CASES)
def test_public_entry_is_stable(ctx, L, key_bits, distinct, n):
    """few distinct key values, so every tile holds long runs of equal keys; the input position sits above the rounded span"""
    keys = REF.few_values(n, 11, key_bits, distinct)
    check_sort(ctx, L, keys, 0, key_bits, "public", "%d values" % distinct)


def test_public_cases_cover_the_issue():
    assert len(PUBLIC_CASES) == 15 and (8, 257) not in PUBLIC_CASES


# ---- the bit range ---------------------------------------------------------------------------------------------------------
#             first_bit, end_bit -> passes
RANGE_CASES = [(0, 8), (0, 3), (0, 16), (0, 24), (0, 40), (0, 48), (0, 56), (0, 64), (0, 61),
               (8, 16), (8, 24), (8, 30), (8, 48), (8, 56), (8, 64),
               (17, 25), (17, 30), (17, 41), (17, 57), (17, 64),
               (21, 29), (21, 37), (21, 45), (21, 61), (21, 64),
               (40, 48), (40, 50), (40, 64)]


def test_range_cases_cover_the_issue():
    passes = {f: {REF.span(f, e)[1] for ff, e in RANGE_CASES if ff == f} for f in (0, 8, 17, 21, 40)}
    assert passes[0] == {1, 2, 3, 5, 6, 7, 8} and passes[8] == {1, 2, 3, 5, 6, 7}
    assert passes[17] == passes[21] == {1, 2, 3, 5, 6} and passes[40] == {1, 2, 3}      # (what fits below bit 64)


@pytest.mark.parametrize("n", [4097, 5 * 4096 + 3, 7 * 4096 + 1])
@pytest.mark.parametrize("first_bit,end_bit", RANGE_CASES)
def test_bit_range_junk_below(ctx, L, first_bit, end_bit, n):
    """random bits below first_bit (and above the span): among equal digits they must come out in input order"""
    check_sort(ctx, L, REF.range_keys(n, 5, first_bit, end_bit, "junk"), first_bit, end_bit, what="junk")


@pytest.mark.parametrize("first_bit,end_bit", [(0, 8), (8, 30), (17, 57), (21, 64), (40, 50)])
def test_bit_range_junk_below_large(ctx, L, first_bit, end_bit):
    check_sort(ctx, L, REF.range_keys(1_500_000, 6, first_bit, end_bit, "junk"), first_bit, end_bit, what="junk")


@pytest.mark.parametrize("first_bit,end_bit", [c for c in RANGE_CASES if c[0] > 0])
def test_bit_range_rows_below(ctx, L, first_bit, end_bit):
    """the NN index's layout: an ascending row number below first_bit.  The passes over it are skipped, and the result is
    still what a full sort of the words gives."""
    for n in sorted({min(n, 1 << first_bit) for n in (200, 4097, 7 * 4096 + 1, 131072, 1_500_000)}):
        keys = REF.range_keys(n, 7, first_bit, end_bit, "rows")
        got = check_sort(ctx, L, keys, first_bit, end_bit, what="rows")
        same(got, np.sort(keys), "rows, against a full sort, n=%d" % n)


@pytest.mark.parametrize("first_bit,end_bit", [(8, 8), (16, 8), (64, 64), (40, 17), (-1, 16), (-8, 64)])
def test_bit_range_falls_back_to_zero(ctx, L, first_bit, end_bit):
    """first_bit >= end_bit (or negative) counts as 0: the same words as a sort of [0, end_bit)"""
    assert REF.span(first_bit, end_bit)[0] == 0
    for n in (4097, 7 * 4096 + 1):
        keys = REF.range_keys(n, 8, first_bit, end_bit, "junk")
        got = check_sort(ctx, L, keys, first_bit, end_bit, what="fallback")
        same(got, REF.stable_sort_by_bits(keys, 0, end_bit), "fallback against first_bit = 0")


def test_bit_range_tiny(ctx, L, R):
    assert ctx.lib.r3d_sort_u64_bits(ctx.handle, None, 0, 8, 24) == 0
    assert ctx.lib.r3d_sort_u64_bits(ctx.handle, None, 2, 8, 24) == L.ERR_INVALID
    assert ctx.lib.r3d_sort_u64_bits(ctx.handle, None, -1, 8, 24) == L.ERR_INVALID
    for end in (0, 65):
        assert ctx.lib.r3d_sort_u64_bits(ctx.handle, None, 0, 0, end) == L.ERR_INVALID
    one = np.array([0xfedcba9876543210], U)
    for first, end in ((0, 64), (8, 24), (40, 48)):
        same(device_sort(ctx, L, one, first, end), one, "one key")
        same(device_sort(ctx, L, one[:0], first, end), one[:0], "no key")
    two = np.array([0x2_00_ff, 0x1_00_ff], U)
    same(device_sort(ctx, L, two, 0, 16), two, "two equal fields stay")
    same(device_sort(ctx, L, two, 8, 24), two[::-1], "two keys by their upper field")


# ---- digit distributions ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", REF.DISTRIBUTION_SIZES)
@pytest.mark.parametrize("name", sorted(REF.GENERATORS))
def test_distributions(ctx, L, name, n):
    """digit 0 carries the named property in input order; one pass (copy-back), two passes (in place, the second pass sees
    digit 1 in digit-0 order), and at the sizes below a million also the second digit alone and three passes"""
    keys = REF.GENERATORS[name](n, 21)
    check_sort(ctx, L, keys, 0, 8, what=name)
    check_sort(ctx, L, keys, 0, 16, what=name)
    check_sort(ctx, L, keys, 0, 16, "public", what=name)
    if n < 1_000_000:
        check_sort(ctx, L, keys, 8, 16, what=name)
        check_sort(ctx, L, keys, 0, 24, what=name)                  # third digit: the low byte of the position, ascending mod 256


@pytest.mark.parametrize("tiles", list(range(1, 10)))
def test_small_grids(ctx, L, tiles):
    """grids of fewer than 8 workgroups and just above: the workgroup -> tile map of the scatter"""
    for n in (tiles * TILE, tiles * TILE - 1):
        for name in ("uniform", "hot"):
            gen = REF.gen_uniform if name == "uniform" else REF.gen_hot
            check_sort(ctx, L, gen(n, 22), 0, 16, what=name)


# ---- sizes around the scan's segments ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["uniform", "hot"])
@pytest.mark.parametrize("delta", [-1, 0, 1])
@pytest.mark.parametrize("tiles", REF.SEGMENT_TILES)
def test_sort_across_scan_segments(ctx, L, tiles, delta, kind):
    n = tiles * TILE + delta
    keys = (REF.gen_uniform if kind == "uniform" else REF.gen_hot)(n, 23)
    check_sort(ctx, L, keys, 0, 16, what=kind)


# ---- row selection ---------------------------------------------------------------------------------------------------------
class Cloud:
    """one cloud of arbitrary float bit patterns on the device at a time (uploading 200 MB per mask would be most of the time)"""

    def __init__(self, ctx):
        self.ctx, self.n, self.xyz, self.d_xyz = ctx, None, None, None

    def get(self, n):
        if n != self.n:
            self.free()
            words = np.random.default_rng([31, n]).integers(0, 1 << 32, (n, 3), dtype=np.uint32)
            self.n, self.xyz = n, words.view(np.float32)
            self.d_xyz = self.ctx.alloc(n * 12).upload(self.xyz)
        return self.xyz, self.d_xyz

    def free(self):
        if self.d_xyz is not None:
            self.d_xyz.free()
        self.n = self.xyz = self.d_xyz = None


@pytest.fixture(scope="module")
def cloud(ctx):
    c = Cloud(ctx)
    yield c
    c.free()


def check_select(ctx, O, xyz, d_xyz, keep, what=""):
    """outputs sized for the kept rows only, between guard bands, at offsets that are not 16-byte aligned"""
    n = keep.shape[0]
    want_rows, want_xyz = REF.select_rows(xyz, keep)
    m = want_rows.size
    d_keep = ctx.alloc(n).upload(keep)
    gx, gr = Guarded(ctx, m * 12, 4, seed=41), Guarded(ctx, m * 4, 4, seed=42)
    try:
        got_m = O.select_rows_device(ctx, d_xyz.ptr, n, d_keep.ptr, gx.ptr, gr.ptr)
        rows, out = gr.read(np.uint32), gx.read(np.uint32, (m, 3))            # (asserts the bands)
        assert got_m == m, (what, n, got_m, m)
        same(rows, want_rows, "%s: rows of n=%d" % (what, n))
        same(out, want_xyz.view(np.uint32), "%s: xyz bits of n=%d" % (what, n))
        return rows, out
    finally:
        for b in (d_keep, gx, gr):
            b.free()


SELECT_CASES = [(t * TILE, m) for t in REF.SEGMENT_TILES for m in sorted(REF.MASKS)] + \
               [(t * TILE + d, "random30") for t in REF.SEGMENT_TILES for d in (-1, 1)]
SELECT_CASES.sort(key=lambda c: (c[0] + TILE // 2) // TILE)            # one upload of the cloud per tile count, nearly


@pytest.mark.parametrize("n,mask", SELECT_CASES)
def test_select_rows_across_scan_segments(ctx, O, cloud, n, mask):
    xyz, d_xyz = cloud.get(n)
    check_select(ctx, O, xyz, d_xyz, REF.MASKS[mask](n, 24), mask)


@pytest.mark.parametrize("n", [1, 4095, 4096, 4097, 3 * 4096 + 17])
@pytest.mark.parametrize("mask", sorted(REF.MASKS))
def test_select_rows_small(ctx, O, cloud, n, mask):
    xyz, d_xyz = cloud.get(n)
    check_select(ctx, O, xyz, d_xyz, REF.MASKS[mask](n, 25), mask)


# ---- a small job behind a large one on the same context --------------------------------------------------------------------
@pytest.mark.parametrize("first", ["sort", "voxel insert"])
def test_stale_workspace(R, L, O, first):
    """Counters beyond the last workgroup are padding and count as zero whatever they hold.  Here they hold the numbers of
    the job before: every step runs on one fresh context whose scratch only ever grew."""
    c = R.Context(0)
    cl = Cloud(c)
    try:
        if first == "sort":
            check_sort(c, L, REF.gen_hot(REF.SEGMENT_TILES[-1] * TILE, 51), 0, 16, what="large sort first")
        else:
            V = importlib.import_module(PKG + ".voxelmap")
            pts = (np.random.default_rng(52).normal(size=(3_000_000, 3)) * 8).astype(np.float32)
            codes, st = V.voxelize(pts, 0.1, c)
            want, dropped = OM.occupied_set(pts)
            assert st["voxels"] == len(want) > 1_000_000 and st["ignored_points"] == dropped
            same(codes, want, "voxel codes")
        check_sort(c, L, REF.gen_uniform(5 * TILE - 9, 53), 0, 16, what="5 tiles behind it")
        check_sort(c, L, REF.gen_hot(5 * TILE - 9, 53), 0, 8, what="5 tiles behind it, one pass")
        n = 3 * TILE + 17
        xyz, d_xyz = cl.get(n)
        for mask in ("random30", "all", "last_row"):
            check_select(c, O, xyz, d_xyz, REF.MASKS[mask](n, 54), mask + " on 4 tiles behind it")
        n = 1023 * TILE
        xyz, d_xyz = cl.get(n)
        check_select(c, O, xyz, d_xyz, REF.MASKS["random30"](n, 55), "1023 tiles")
        two = np.array([(7 << 16) | 0x0102, (3 << 16) | 0x0101], U)
        same(device_sort(c, L, two, 0, 16), two[::-1], "two keys")
        same(device_sort(c, L, two, 8, 16), two, "two keys, equal upper digit")
        check_sort(c, L, REF.gen_values_17(TILE + 1, 56), 0, 16, what="2 tiles at the end")
    finally:
        cl.free()
        c.close()


# ---- two runs, same bits -----------------------------------------------------------------------------------------------------
def test_two_runs_same_bits(ctx, L, O, cloud):
    keys = REF.gen_hot(2049 * TILE + 1, 61)
    a = check_sort(ctx, L, keys, 0, 16, what="first run")
    b = device_sort(ctx, L, keys, 0, 16)
    same(b, a, "second run of the same sort")
    n = 2049 * TILE + 1
    xyz, d_xyz = cloud.get(n)
    keep = REF.MASKS["flag_bytes"](n, 62)
    r1, x1 = check_select(ctx, O, xyz, d_xyz, keep, "first run")
    r2, x2 = check_select(ctx, O, xyz, d_xyz, keep, "second run")
    same(r2, r1, "rows of the second run")
    same(x2, x1, "xyz of the second run")
