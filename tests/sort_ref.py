"""Plain NumPy references for the sort and selection primitives (csrc/r3d_sort.hip, select_*_kernel of csrc/r3d_knn.hip) and
the adversarial inputs their GPU tests run on.

The references restate what the headers promise and nothing of how the kernels work:
  * stable_sort_by_bits: r3d_radix_sort_u64 orders 64-bit keys by their bits [first_bit, end_bit), the span rounded up to
    whole 8-bit digits counted from first_bit (bits beyond 63 read as zero), and keys that agree on those bits keep their
    input order (r3d_sort.hip, header comment of r3d_radix_sort_u64);
  * select_rows: the rows with a nonzero flag, in input order (include/r3d.h, r3d_select_rows).

Every generator takes (n, seed) and returns n uint64 keys laid out as
    bits 0..7   digit 0 -- carries the property the generator is named for IN INPUT ORDER (a radix pass sees it as it is)
    bits 8..15  digit 1 -- the same family with other parameters (the second pass sees it in digit-0 order)
    bits 16..   the input position: no two keys are the same word, so the order among equal digits is visible.
tests/test_sort_host.py asserts each property in numbers; tests/test_gpu_sort.py sorts the same keys on the device.
"""
import numpy as np

TILE = 4096        # keys per workgroup (r3d_sort_dev.h kTile)
WAVES = 4          # waves per workgroup; wave w ranks elements [1024 w, 1024 (w + 1)) of its tile
ROUND = 64         # one wave round: 64 consecutive elements
SEGMENT = 1024     # tile counters per segment of the scan's walk over a row
PAYLOAD_SHIFT = 16
U = np.uint64


def span(first_bit, end_bit):
    """(first_bit as used, passes, top): the sort looks at bits [first, top), top = min(64, first + 8 passes)."""
    if first_bit < 0 or first_bit >= end_bit:
        first_bit = 0
    passes = (end_bit - first_bit + 7) // 8
    return first_bit, passes, min(64, first_bit + 8 * passes)


def sort_field(keys, first_bit, end_bit):
    """The bits the sort compares, as the smallest unsigned type that holds them."""
    first, _, top = span(first_bit, end_bit)
    width = top - first
    field = np.asarray(keys, np.uint64) >> U(first)
    if width < 64:
        field = field & U((1 << width) - 1)
    for t, w in ((np.uint8, 8), (np.uint16, 16), (np.uint32, 32)):
        if width <= w:
            return field.astype(t)
    return field


def stable_sort_by_bits(keys, first_bit, end_bit):
    keys = np.asarray(keys, np.uint64)
    return keys[np.argsort(sort_field(keys, first_bit, end_bit), kind="stable")]


def select_rows(xyz, keep):
    """(rows uint32 [m], xyz [m,3]) of the rows whose flag byte is not zero, in input order."""
    rows = np.flatnonzero(np.asarray(keep) != 0)
    return rows.astype(np.uint32), np.asarray(xyz)[rows]


# ---- key generators -------------------------------------------------------------------------------------------------------
def compose(d0, d1):
    """digit 0 | digit 1 << 8 | input position << 16"""
    n = d0.shape[0]
    return d0.astype(np.uint64) | (d1.astype(np.uint64) << U(8)) | (np.arange(n, dtype=np.uint64) << U(PAYLOAD_SHIFT))


def digits(keys, which=0):
    return ((np.asarray(keys, np.uint64) >> U(8 * which)) & U(0xff)).astype(np.uint8)


def payload(keys):
    return np.asarray(keys, np.uint64) >> U(PAYLOAD_SHIFT)


def gen_uniform(n, seed):
    rng = np.random.default_rng([seed, n, 0])
    return compose(rng.integers(0, 256, n, dtype=np.uint8), rng.integers(0, 256, n, dtype=np.uint8))


def gen_all_equal(n, seed):
    rng = np.random.default_rng([seed, n, 1])
    a, b = rng.integers(0, 256, 2)
    return compose(np.full(n, a, np.uint8), np.full(n, b, np.uint8))


def _alternating(n, seed, period):
    rng = np.random.default_rng([seed, n, 2, period])
    a, b = rng.choice(256, 2, replace=False)
    i = np.arange(n)
    d0 = np.where((i // period) % 2 == 0, a, b).astype(np.uint8)
    d1 = np.where((i // (2 * period)) % 2 == 0, b, a).astype(np.uint8)          # changes half as often
    return compose(d0, d1)


def gen_alternating_1(n, seed):
    return _alternating(n, seed, 1)


def gen_alternating_64(n, seed):
    return _alternating(n, seed, 64)


def gen_alternating_1024(n, seed):
    return _alternating(n, seed, 1024)


def gen_alternating_4096(n, seed):
    return _alternating(n, seed, 4096)


def _ramp16(n):
    """n values ascending over the whole 16-bit range (every value occurs once n >= 65536)."""
    if n <= 1:
        return np.zeros(n, np.uint64)
    return (np.arange(n, dtype=np.uint64) * U(65535)) // U(n - 1)


def gen_sorted(n, seed):
    v = _ramp16(n)
    return compose(v & U(0xff), v >> U(8))


def gen_reverse_sorted(n, seed):
    v = U(65535) - _ramp16(n)
    return compose(v & U(0xff), v >> U(8))


def gen_constant_digit0(n, seed):
    """digit 0 is one value for every key, digit 1 is random"""
    rng = np.random.default_rng([seed, n, 3])
    return compose(np.full(n, rng.integers(0, 256), np.uint8), rng.integers(0, 256, n, dtype=np.uint8))


def gen_constant_digit1(n, seed):
    """digit 0 is random, digit 1 is one value for every key"""
    rng = np.random.default_rng([seed, n, 4])
    return compose(rng.integers(0, 256, n, dtype=np.uint8), np.full(n, rng.integers(0, 256), np.uint8))


def gen_quarter_bins(n, seed):
    """In tile t the quarter of wave t % 4 holds one digit value H throughout; every other wave w draws from the values
    d != H with d % 4 == w.  Bin H of a tile is filled by one wave alone (1024 keys), and every other bin is empty in three
    waves of four."""
    rng = np.random.default_rng([seed, n, 5])
    hot = int(rng.integers(0, 256))
    i = np.arange(n)
    wave, tile = (i % TILE) // (TILE // WAVES), i // TILE
    pool = [np.array([d for d in range(256) if d % 4 == w and d != hot], np.uint8) for w in range(WAVES)]
    pick = rng.integers(0, 63, n)
    d0 = np.empty(n, np.uint8)
    for w in range(WAVES):
        m = wave == w
        d0[m] = pool[w][pick[m]]
    d0[wave == tile % WAVES] = hot
    d1 = ((tile * 7 + wave) % 256).astype(np.uint8)                              # long runs, other boundaries
    return compose(d0, d1)


def gen_hot(n, seed):
    """one 16-bit value takes 90 % of the keys, the rest is uniform"""
    rng = np.random.default_rng([seed, n, 6])
    v = rng.integers(0, 65536, n, dtype=np.uint16)
    v[rng.random(n, dtype=np.float32) < 0.9] = rng.integers(0, 65536)
    v = v.astype(np.uint64)
    return compose(v & U(0xff), v >> U(8))


def gen_values_17(n, seed):
    """keys drawn from 17 16-bit values (17 distinct low digits)"""
    rng = np.random.default_rng([seed, n, 7])
    lo = rng.choice(256, 17, replace=False).astype(np.uint64)
    vals = lo | (rng.integers(0, 256, 17).astype(np.uint64) << U(8))
    v = vals[rng.integers(0, 17, n)]
    return compose(v & U(0xff), v >> U(8))


GENERATORS = {
    "all_equal": gen_all_equal,
    "alternating_1": gen_alternating_1,
    "alternating_64": gen_alternating_64,
    "alternating_1024": gen_alternating_1024,
    "alternating_4096": gen_alternating_4096,
    "sorted": gen_sorted,
    "reverse_sorted": gen_reverse_sorted,
    "constant_digit0": gen_constant_digit0,
    "constant_digit1": gen_constant_digit1,
    "quarter_bins": gen_quarter_bins,
    "hot": gen_hot,
    "values_17": gen_values_17,
}

DISTRIBUTION_SIZES = [4095, 4096, 4097, 7 * 4096 + 1, 1_500_000]
SEGMENT_TILES = [1023, 1024, 1025, 2049, 4 * 1024 + 3]


def few_values(n, seed, key_bits, distinct):
    """Keys for the public entry: `distinct` values spread over the whole rounded span of key_bits (bits above key_bits
    inside the last digit included), the input position above the span."""
    _, _, top = span(0, key_bits)
    rng = np.random.default_rng([seed, n, key_bits, distinct])
    assert distinct <= 1 << top
    vals = set()
    while len(vals) < distinct:
        vals.update(int(v) for v in rng.integers(0, 1 << top, distinct - len(vals), dtype=np.uint64))
    vals = np.array(sorted(vals), np.uint64)
    rng.shuffle(vals)
    return vals[rng.integers(0, distinct, n)] | (np.arange(n, dtype=np.uint64) << U(top))


def range_keys(n, seed, first_bit, end_bit, low):
    """Keys for the bit range: every digit of the span takes one of two values (long runs of equal sort fields).
    low = "rows": the bits below first_bit hold the row number (needs n <= 2^first_bit), the bits above the span are zero --
                  the NN index's layout; a stable sort of the span then equals a full sort of the words.
    low = "junk": the bits below first_bit and above the span are random."""
    first, passes, top = span(first_bit, end_bit)
    rng = np.random.default_rng([seed, n, first_bit + 64, end_bit, int(low == "rows")])    # (first_bit may be negative)
    field = np.zeros(n, np.uint64)
    for p in range(passes):
        two = rng.choice(256, 2, replace=False).astype(np.uint64)
        field |= two[rng.integers(0, 2, n)] << U(8 * p)
    if top - first < 64:
        field &= U((1 << (top - first)) - 1)
    keys = field << U(first)
    below = U((1 << first) - 1)
    if low == "rows":
        assert n <= 1 << first
        return keys | np.arange(n, dtype=np.uint64)
    junk = rng.integers(0, 1 << 63, n, dtype=np.uint64) * U(2) + rng.integers(0, 2, n, dtype=np.uint64)
    above = U(0) if top == 64 else ~U((1 << top) - 1)
    return keys | (junk & (below | above))


# ---- keep masks -----------------------------------------------------------------------------------------------------------
def mask_all(n, seed):
    return np.ones(n, np.uint8)


def mask_none(n, seed):
    return np.zeros(n, np.uint8)


def mask_last(n, seed):
    k = np.zeros(n, np.uint8)
    k[n - 1] = 1
    return k


def mask_first(n, seed):
    k = np.zeros(n, np.uint8)
    k[0] = 1
    return k


def mask_random30(n, seed):
    return (np.random.default_rng([seed, n, 8]).random(n) < 0.3).astype(np.uint8)


def mask_runs4096(n, seed):
    return ((np.arange(n) // TILE) % 2 == 0).astype(np.uint8)


def mask_flag_bytes(n, seed):
    """30 % kept, the flag of a kept row any byte but 0 and 1 (0x80, 0xff, 2, ... )"""
    rng = np.random.default_rng([seed, n, 9])
    return np.where(rng.random(n) < 0.3, rng.integers(2, 256, n), 0).astype(np.uint8)


MASKS = {
    "all": mask_all,
    "none": mask_none,
    "last_row": mask_last,
    "first_row": mask_first,
    "random30": mask_random30,
    "runs4096": mask_runs4096,
    "flag_bytes": mask_flag_bytes,
}
