"""CPU: the sort / selection references of tests/sort_ref.py on inputs small enough to check by eye, and every key generator
and keep mask against the property it is named for, in numbers -- so that a later edit cannot quietly turn an adversarial
input of tests/test_gpu_sort.py into a uniform one.  The argument checks of r3d_sort_u64_bits need no device either."""
import importlib

import numpy as np
import pytest

import sort_ref as REF
from helpers import PKG

U = np.uint64
SIZES = REF.DISTRIBUTION_SIZES


# ---- the reference itself -------------------------------------------------------------------------------------------------
def test_equal_keys_keep_their_input_order():
    #                 field 2 | payload 0 ... : sorted by bits [0, 8) only
    keys = np.array([0x0002, 0x0101, 0x0202, 0x0301, 0x0402, 0x0500, 0x0601], U)
    got = REF.stable_sort_by_bits(keys, 0, 8)
    assert got.tolist() == [0x0500, 0x0101, 0x0301, 0x0601, 0x0002, 0x0202, 0x0402]
    # a plain sort of the words orders the payloads too: here it agrees because they ascend, and must not when they descend
    rev = keys[::-1].copy()
    got = REF.stable_sort_by_bits(rev, 0, 8)
    assert got.tolist() == [0x0500, 0x0601, 0x0301, 0x0101, 0x0402, 0x0202, 0x0002]
    assert got.tolist() != np.sort(rev).tolist()


def test_bits_below_first_bit_are_not_compared():
    keys = np.array([0x1_07, 0x0_09, 0x1_01, 0x0_03], U)
    assert REF.stable_sort_by_bits(keys, 4, 12).tolist() == [0x0_09, 0x0_03, 0x1_07, 0x1_01]
    assert REF.stable_sort_by_bits(keys, 0, 12).tolist() == [0x0_03, 0x0_09, 0x1_01, 0x1_07]


@pytest.mark.parametrize("first,end,want", [
    (0, 1, (0, 1, 8)), (0, 8, (0, 1, 8)), (0, 9, (0, 2, 16)), (0, 20, (0, 3, 24)), (0, 40, (0, 5, 40)), (0, 64, (0, 8, 64)),
    (0, 61, (0, 8, 64)), (17, 30, (17, 2, 33)), (21, 64, (21, 6, 64)), (40, 64, (40, 3, 64)), (40, 41, (40, 1, 48)),
    (8, 8, (0, 1, 8)), (16, 8, (0, 1, 8)), (-1, 16, (0, 2, 16)), (64, 64, (0, 8, 64)),
])
def test_span_rounds_up_to_whole_digits(first, end, want):
    assert REF.span(first, end) == want


def test_rounded_span_is_compared_and_nothing_above_it():
    # key_bits = 4 sorts the whole low byte: bit 7 decides, bit 8 does not
    keys = np.array([0x080, 0x17f, 0x001, 0x100], U)
    assert REF.stable_sort_by_bits(keys, 0, 4).tolist() == [0x100, 0x001, 0x17f, 0x080]
    # first_bit = 60: one digit of four real bits, the rest reads as zero
    keys = np.array([0xf << 60 | 5, 0x1 << 60 | 9, 0xf << 60 | 1, 0x1 << 60 | 2], U)
    assert REF.stable_sort_by_bits(keys, 60, 64).tolist() == [0x1 << 60 | 9, 0x1 << 60 | 2, 0xf << 60 | 5, 0xf << 60 | 1]
    assert REF.sort_field(keys, 60, 64).dtype == np.uint8 and REF.sort_field(keys, 0, 64).dtype == np.uint64
    assert REF.sort_field(keys, 8, 40).dtype == np.uint32 and REF.sort_field(keys, 0, 33).dtype == np.uint64


def test_select_rows_reference():
    xyz = np.arange(18, dtype=np.float32).reshape(6, 3)
    rows, out = REF.select_rows(xyz, np.array([0, 1, 0, 255, 2, 0], np.uint8))
    assert rows.dtype == np.uint32 and rows.tolist() == [1, 3, 4]
    assert np.array_equal(out, xyz[[1, 3, 4]])
    rows, out = REF.select_rows(xyz, np.zeros(6, np.uint8))
    assert rows.size == 0 and out.shape == (0, 3)


# ---- what every generator promises ----------------------------------------------------------------------------------------
def tile_wave_counts(d, full_only=True):
    """[tiles][wave][bin] counts of an array of digits, full tiles only"""
    t = d.shape[0] // REF.TILE
    q = d[:t * REF.TILE].reshape(t * REF.WAVES, REF.TILE // REF.WAVES).astype(np.int64)
    flat = (np.arange(t * REF.WAVES)[:, None] * 256 + q).reshape(-1)
    return np.bincount(flat, minlength=t * REF.WAVES * 256).reshape(t, REF.WAVES, 256)


def rounds_of_one_digit(d):
    """number of aligned wave rounds (64 consecutive elements) whose digits are all the same"""
    r = d[:d.shape[0] // REF.ROUND * REF.ROUND].reshape(-1, REF.ROUND)
    return int((r == r[:, :1]).all(axis=1).sum())


@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("name", sorted(REF.GENERATORS))
def test_generator_layout(name, n):
    """every generator: n keys, the position above bit 16, the same keys for the same (n, seed) and others for another seed;
    at least two distinct payloads for some equal 16-bit key (here: for the most frequent one)"""
    keys = REF.GENERATORS[name](n, 3)
    assert keys.dtype == np.uint64 and keys.shape == (n,)
    assert np.array_equal(REF.payload(keys), np.arange(n, dtype=np.uint64))
    assert np.array_equal(keys, REF.GENERATORS[name](n, 3))
    if name not in ("sorted", "reverse_sorted"):
        assert not np.array_equal(keys, REF.GENERATORS[name](n, 4))
    low = (keys & U(0xffff)).astype(np.int64)
    if name not in ("sorted", "reverse_sorted") or n > 65536:       # (a ramp over 16 bits repeats a value only beyond 65536 keys)
        assert np.bincount(low).max() >= 2                          # payloads are distinct, so these are two payloads of one key
    d0 = REF.digits(keys, 0).astype(np.int64)
    assert np.bincount(d0).max() >= 16                              # ... and long runs per first-pass bin
    # the stable order differs from SOME unstable order: reversing the ties changes the words
    by0 = REF.stable_sort_by_bits(keys, 0, 8)
    assert not np.array_equal(by0, REF.stable_sort_by_bits(keys[::-1], 0, 8))


@pytest.mark.parametrize("n", SIZES)
def test_all_equal(n):
    keys = REF.gen_all_equal(n, 1)
    assert np.unique(keys & U(0xffff)).size == 1
    d0 = REF.digits(keys)
    assert rounds_of_one_digit(d0) == n // 64
    if n >= REF.TILE:
        assert (tile_wave_counts(d0).sum(axis=1).max(axis=1) == REF.TILE).all()      # one bin holds every whole tile


@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("period", [1, 64, 1024, 4096])
def test_alternating(n, period):
    keys = REF.GENERATORS["alternating_%d" % period](n, 1)
    d0, d1 = REF.digits(keys, 0), REF.digits(keys, 1)
    if n <= period:                                                                  # (one run: the case is "all equal" at this size)
        assert np.unique(d0).size == 1
        return
    a, b = d0[0], d0[period]
    assert a != b and np.unique(d0).size == 2
    i = np.arange(n)
    assert np.array_equal(d0, np.where((i // period) % 2 == 0, a, b))
    assert np.unique(d1).size == (2 if n > 2 * period else 1)
    if period == 1:
        assert rounds_of_one_digit(d0) == 0
        c = tile_wave_counts(d0)
        assert (c[:, :, a] == 512).all() and (c[:, :, b] == 512).all()
    if period == 64:
        assert rounds_of_one_digit(d0) == n // 64                                    # every wave round shares one digit
        assert (tile_wave_counts(d0)[:, :, a] == 512).all()
    if period == 1024:
        c = tile_wave_counts(d0)                                                     # a bin is one wave's alone ...
        assert (c[:, 0::2, a] == 1024).all() and (c[:, 1::2, a] == 0).all() and (c[:, 1::2, b] == 1024).all()
    if period == 4096 and n >= REF.TILE:
        c = tile_wave_counts(d0).sum(axis=1)                                         # ... or holds the whole tile
        assert (c.max(axis=1) == REF.TILE).all() and (c[0::2, a] == REF.TILE).all()
        if n >= 2 * REF.TILE:
            assert (c[1::2, b] == REF.TILE).all()


@pytest.mark.parametrize("n", SIZES)
def test_sorted_and_reverse_sorted(n):
    up, down = REF.gen_sorted(n, 1) & U(0xffff), REF.gen_reverse_sorted(n, 1) & U(0xffff)
    du, dd = np.diff(up.astype(np.int64)), np.diff(down.astype(np.int64))
    assert (du >= 0).all() and (du > 0).any() and (dd <= 0).all() and (dd < 0).any()
    assert up[0] == 0 and up[-1] == 65535 and down[0] == 65535 and down[-1] == 0
    assert np.unique(up).size == min(n, 65536)
    assert np.array_equal(REF.stable_sort_by_bits(REF.gen_sorted(n, 1), 0, 16), REF.gen_sorted(n, 1))
    # reverse sorted input: the stable result is NOT the reversed array once a value repeats (n > 65536)
    rs = REF.gen_reverse_sorted(n, 1)
    assert np.array_equal(REF.stable_sort_by_bits(rs, 0, 16), rs[::-1]) == (n <= 65536)


@pytest.mark.parametrize("n", SIZES)
def test_constant_digit(n):
    k0, k1 = REF.gen_constant_digit0(n, 1), REF.gen_constant_digit1(n, 1)
    assert np.unique(REF.digits(k0, 0)).size == 1 and np.unique(REF.digits(k0, 1)).size == 256
    assert np.unique(REF.digits(k1, 1)).size == 1 and np.unique(REF.digits(k1, 0)).size == 256


@pytest.mark.parametrize("n", SIZES)
def test_quarter_bins(n):
    keys = REF.gen_quarter_bins(n, 1)
    d0 = REF.digits(keys)
    c = tile_wave_counts(d0)                                                         # [tile][wave][bin]
    assert c.shape[0] == n // REF.TILE
    hot = int(d0[0])                                                                 # tile 0, wave 0 is all-hot
    for t in range(min(c.shape[0], 9)):
        assert c[t, t % 4, hot] == 1024 and c[t, :, hot].sum() == 1024              # one wave's quarter, one bin
    assert ((c > 0).sum(axis=1) <= 1).all()                                          # every bin: empty in >= 3 waves of 4
    if c.shape[0]:
        assert ((c.sum(axis=1) > 0).sum(axis=1) >= 150).all()                        # and the other quarters spread widely
    assert rounds_of_one_digit(d0) >= 16 * (n // REF.TILE)


@pytest.mark.parametrize("n", SIZES)
def test_hot(n):
    keys = REF.gen_hot(n, 1)
    low = (keys & U(0xffff)).astype(np.int64)
    counts = np.bincount(low, minlength=65536)
    share = counts.max() / n
    assert 0.88 <= share <= 0.93, share
    assert np.count_nonzero(counts) >= min(n // 20, 20000)                           # the background is spread out
    c = tile_wave_counts(REF.digits(keys)).sum(axis=1)
    if c.shape[0]:
        assert (c.max(axis=1) >= 0.85 * REF.TILE).all()                              # every tile: one bin takes most of it
    if n >= 1_000_000:
        assert rounds_of_one_digit(REF.digits(keys)) >= 1                            # 0.9^64 per round: ~28 expected


@pytest.mark.parametrize("n", SIZES)
def test_values_17(n):
    keys = REF.gen_values_17(n, 1)
    low = keys & U(0xffff)
    vals, counts = np.unique(low, return_counts=True)
    assert vals.size == 17 and np.unique(REF.digits(keys)).size == 17
    assert counts.min() >= n // 17 // 2                                              # each value: many payloads


def test_uniform():
    keys = REF.gen_uniform(1 << 20, 1)
    c = np.bincount((keys & U(0xffff)).astype(np.int64), minlength=65536)
    assert c.min() >= 1 and c.max() <= 48                                            # mean 16


@pytest.mark.parametrize("key_bits,distinct", [(8, 2), (8, 3), (8, 256), (16, 257), (20, 2), (20, 257), (40, 3), (40, 256)])
def test_few_values(key_bits, distinct):
    n = 7 * 4096 + 1
    keys = REF.few_values(n, 0, key_bits, distinct)
    _, _, top = REF.span(0, key_bits)
    field = keys & U((1 << top) - 1)
    assert np.unique(field).size == distinct
    assert np.array_equal(keys >> U(top), np.arange(n, dtype=np.uint64))
    if key_bits % 8 and distinct >= 256:
        assert (field >> U(key_bits)).any()                                          # the rounding is visible in the keys
    got = REF.stable_sort_by_bits(keys, 0, key_bits)
    gf, gp = (got & U((1 << top) - 1)).astype(np.int64), (got >> U(top)).astype(np.int64)
    assert (np.diff(gf) >= 0).all() and (np.diff(gp)[np.diff(gf) == 0] > 0).all()      # by field, then by input position
    assert np.array_equal(np.sort(gp), np.arange(n))


@pytest.mark.parametrize("first,end", [(0, 64), (8, 30), (17, 57), (21, 64), (40, 50), (16, 8)])
def test_range_keys(first, end):
    f, passes, top = REF.span(first, end)
    n = min(7 * 4096 + 1, 1 << f) if f else 7 * 4096 + 1
    junk = REF.range_keys(n, 0, first, end, "junk")
    field = REF.sort_field(junk, first, end)
    assert np.unique(field).size <= 2 ** passes and np.unique(field).size >= min(2 ** passes, 64) // 2
    if f:
        below = junk & U((1 << f) - 1)
        assert np.unique(below).size > min(n, 1 << f) // 4                           # junk, not a counter
        assert (np.diff(below.astype(np.int64)) < 0).any()
        # so a full sort of the words is NOT the stable order
        assert not np.array_equal(REF.stable_sort_by_bits(junk, first, end), np.sort(junk))
        rows = REF.range_keys(n, 0, first, end, "rows")
        assert np.array_equal(rows & U((1 << f) - 1), np.arange(n, dtype=np.uint64))
        assert top == 64 or not (rows >> U(top)).any()
        assert np.array_equal(REF.stable_sort_by_bits(rows, first, end), np.sort(rows))
    if top < 64:
        assert np.unique(junk >> U(top)).size > min(n, 1 << (64 - top)) // 2


@pytest.mark.parametrize("name", sorted(REF.MASKS))
def test_masks(name):
    n = 5 * 4096 + 9
    k = REF.MASKS[name](n, 2)
    assert k.dtype == np.uint8 and k.shape == (n,)
    kept = np.flatnonzero(k)
    want = {"all": n, "none": 0, "last_row": 1, "first_row": 1, "runs4096": 3 * 4096}.get(name)
    if want is not None:
        assert kept.size == want
    else:
        assert 0.28 * n < kept.size < 0.32 * n
    if name == "last_row":
        assert kept[0] == n - 1
    if name == "first_row":
        assert kept[0] == 0
    if name == "runs4096":
        assert k[:4096].all() and not k[4096:8192].any() and k[8192:12288].all()
    if name == "flag_bytes":
        assert k[kept].min() >= 2 and np.unique(k[kept]).size >= 200 and (k[kept] >= 0x80).any()
    else:
        assert k.max() <= 1


def test_segment_sizes_cross_the_scan_segments():
    """1024 tile counters = one segment of the scan; the sizes sit on both sides of one, two and four segments, with tile
    counts that are and are not multiples of 8 (the XCD map) and of the row stride's rounding"""
    t = REF.SEGMENT_TILES
    assert [(-(-x // REF.SEGMENT)) for x in t] == [1, 1, 2, 3, 5]
    assert [x % 8 for x in t] == [7, 0, 1, 1, 3]
    assert max(t) * REF.TILE + 1 < 17_000_000


def test_bits_entry_rejects_bad_arguments_without_gpu():
    L = importlib.import_module(PKG + "._lib")
    lib = L.load()
    assert lib.r3d_sort_u64_bits(None, None, 0, 0, 8) == L.ERR_INVALID
    assert "NULL" in L.last_error() or "ctx" in L.last_error()
