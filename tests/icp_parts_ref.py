"""Plain NumPy references for the small entry points the ICP driver (icp.py) is built from, and the inputs their GPU tests
run on: per-class selection, trimmed means, the row movers and the batched transform (include/r3d_internal_api.h).

The references restate what the header promises and nothing of how the kernels work; arithmetic is fp64.  Nothing here
imports the package under test.
  * class_quantiles: per class the finite float32 values sorted ascending, the element of rank floor(q (m - 1))
    (oracle/plane_ref.quantile_lower, the rule of r3d_select_quantile_f32); (+inf, 0) for a class without finite values;
  * trimmed_means: per block the fp64 mean of the finite values that are arithmetically <= the block's statistic;
  * gather_rows / gather_rows_strided / permutation_invert / remap / zero_rows_to_nan: the row movers;
  * apply_many: block k = oracle/fusion_ref.apply_T(p, Ts[k]).
tests/test_icp_parts_host.py checks the references against independent NumPy; tests/test_gpu_icp_parts.py runs the device.
"""
import numpy as np

from oracle import fusion_ref as O
from oracle import plane_ref as PR

NO_ROW = 0xffffffff
MAX_CLASSES = 32       # r3d_plane.hip kMaxBuckets
PASS_SPAN = 256 * 8    # elements per workgroup that size the selection's grid (select_enqueue)
U32 = np.uint32


# ---- selection ---------------------------------------------------------------------------------------------------------
def block_classes(n, per_class):
    """Class of element i in contiguous-block mode: i // per_class (a block number >= n_classes takes part in no class)."""
    return np.arange(n, dtype=np.int64) // int(per_class)


def class_quantiles(values, classes, n_classes, q):
    """(values float32[n_classes], counts int64[n_classes]): per class c the "lower" q order statistic of the finite values
    whose class is c.  `classes` holds one integer per element; numbers >= n_classes belong to no class."""
    v = np.asarray(values, dtype=np.float32).reshape(-1)
    cls = np.asarray(classes).reshape(-1).astype(np.int64)
    assert v.shape == cls.shape
    vals, counts = np.empty(n_classes, np.float32), np.zeros(n_classes, np.int64)
    for c in range(n_classes):
        vals[c], counts[c] = PR.quantile_lower(v[cls == c], q)
    return vals, counts


def same_selection(got, want):
    """Bitwise equal float32 arrays, except that a zero may come back with either sign (+0.0 and -0.0 tie in a sort)."""
    got, want = np.asarray(got, np.float32), np.asarray(want, np.float32)
    return bool(np.all((got.view(U32) == want.view(U32)) | ((got == 0) & (want == 0))))


def trimmed_means(values, n_classes, per_class, keep):
    """(means float64[n_classes], scales float64[n_classes]): block c = values[c per_class : (c + 1) per_class]; its mean over the
    finite values that compare <= the block's `keep` order statistic (arithmetic comparison: ties with the statistic all
    count, +0.0 passes a -0.0 statistic), +inf for a block without finite values.  scales[c] = mean |kept value|, the unit
    the summation error of the block is measured in (0 for a block without finite values)."""
    v = np.asarray(values, dtype=np.float32).reshape(n_classes, per_class)
    means, scales = np.full(n_classes, np.inf), np.zeros(n_classes)
    for c in range(n_classes):
        g, m = PR.quantile_lower(v[c], keep)
        if m == 0:
            continue
        f = v[c][np.isfinite(v[c])]
        kept = f[f <= g].astype(np.float64)
        means[c], scales[c] = kept.sum() / kept.size, np.abs(kept).sum() / kept.size
    return means, scales


# ---- row movers --------------------------------------------------------------------------------------------------------
def gather_rows(xyz, rows):
    """out[j] = xyz[rows[j]], a NaN row where rows[j] >= the number of rows."""
    xyz = np.asarray(xyz, np.float32).reshape(-1, 3)
    rows = np.asarray(rows).astype(np.int64)
    out = np.full((rows.size, 3), np.nan, np.float32)
    ok = rows < xyz.shape[0]
    out[ok] = xyz[rows[ok]]
    return out


def gather_rows_strided(xyz, first, step, n_out):
    xyz = np.asarray(xyz, np.float32).reshape(-1, 3)
    return xyz[first + step * np.arange(n_out, dtype=np.int64)].copy()


def permutation_invert(perm, previous):
    """inv[perm[j]] = j over `previous` (what the output held before): an entry >= n is skipped, a slot that no entry names keeps
    its previous contents.  Entries < n must be distinct (two writers of one slot would race on the device)."""
    perm = np.asarray(perm).astype(np.int64)
    inv = np.asarray(previous, np.uint32).copy()
    assert inv.size == perm.size
    ok = perm < perm.size
    assert np.unique(perm[ok]).size == ok.sum()
    inv[perm[ok]] = np.flatnonzero(ok).astype(np.uint32)
    return inv


def remap(values, table):
    """table[values[k]], 0xffffffff where values[k] is outside the table."""
    values, table = np.asarray(values).astype(np.int64), np.asarray(table, np.uint32)
    out = np.full(values.size, NO_ROW, np.uint32)
    ok = values < table.size
    out[ok] = table[values[ok]]
    return out


def zero_rows_to_nan(xyz):
    """Rows whose three coordinates all compare equal to 0 (so -0.0 counts) become NaN rows; every other row keeps its bits."""
    out = np.asarray(xyz, np.float32).reshape(-1, 3).copy()
    out[(out == 0).all(axis=1)] = np.nan
    return out


def apply_many(p, Ts):
    """[k][n][3] fp64: block k is the cloud moved by the k-th row-major 4x4."""
    Ts = np.asarray(Ts, np.float64).reshape(-1, 4, 4)
    return np.stack([O.apply_T(p, T) for T in Ts]) if len(Ts) else np.zeros((0, len(p), 3))


# ---- inputs ------------------------------------------------------------------------------------------------------------
# Value sets for a selection that walks the order key of a float32 one 8-bit digit at a time, top digit first: each isolates
# one digit, the sign flip of the key, or the counting path taken when a wave's 64 lanes want the same counter.
def _bits(u):
    return np.asarray(u, np.uint32).view(np.float32)


def values_low_byte(n, rng):
    """One exponent and mantissa, only the lowest byte differs: the first three passes see a single bin."""
    return _bits(U32(0x3fc01200) | rng.integers(0, 256, n, dtype=np.uint32))


def values_top_byte(n, rng):
    """Only the top byte differs (sign and seven exponent bits; bit 23 is clear, so every pattern is finite)."""
    return _bits((rng.integers(0, 256, n, dtype=np.uint32) << U32(24)) | U32(0x00345678))


def values_straddle_zero(n, rng):
    """Small magnitudes of both signs, many of them repeated with the sign flipped."""
    m = (rng.integers(1, 40, n) * 0.125).astype(np.float32)
    return np.where(rng.random(n) < 0.5, -m, m).astype(np.float32)


def values_zeros_subnormals(n, rng):
    pool = np.array([0x00000000, 0x80000000, 0x00000001, 0x80000001, 0x007fffff, 0x807fffff, 0x00000100, 0x80010000, 0x00800000,
                     0x80800000], np.uint32)
    return _bits(pool[rng.integers(0, pool.size, n)])


def values_wall(n, rng):
    """Runs of 64 consecutive values that share their three leading bytes, as the residuals of one wall do."""
    runs = -(-n // 64)
    lead = (rng.integers(0x3a0000, 0x3f0000, runs, dtype=np.uint32) << U32(8))
    return _bits(np.repeat(lead, 64)[:n] | rng.integers(0, 256, n, dtype=np.uint32))


def values_random_bits(n, rng):
    """Every bit pattern, NaN and infinities included as they come (1 in 256)."""
    return _bits(rng.integers(0, 1 << 32, n, dtype=np.uint64).astype(np.uint32))


VALUE_SETS = {"low_byte": values_low_byte, "top_byte": values_top_byte, "straddle_zero": values_straddle_zero,
              "zeros_subnormals": values_zeros_subnormals, "wall": values_wall, "random_bits": values_random_bits}
NONFINITE = np.array([np.nan, np.inf, -np.inf], np.float32)


def class_case(n, n_classes, kind, seed):
    """(values float32[n], class bytes uint8[n]) with deliberately uneven populations: every third class stays empty between
    full ones (one of them receives a single element), about one element in ten carries a byte >= n_classes (255 among them)
    and takes part in no class, the last populated class holds NaN / +-inf only and class 0 one repeated value."""
    rng = np.random.default_rng([n, n_classes, seed])
    v = VALUE_SETS[kind](n, rng).copy()
    full = [c for c in range(n_classes) if c % 3 != 1] or [0]
    weights = rng.random(len(full)) ** 3 + 0.01
    cls = np.asarray(full)[rng.choice(len(full), size=n, p=weights / weights.sum())].astype(np.uint8)
    if n_classes < 256:
        out = rng.random(n) < 0.1
        cls[out] = rng.choice(np.r_[np.arange(n_classes, min(n_classes + 3, 256)), 255], size=int(out.sum()))
    if n_classes >= 2 and n >= 8:
        cls[rng.integers(0, n)] = 1                                      # a class of one element
    if len(full) >= 3:
        dead = cls == full[-1]
        v[dead] = NONFINITE[rng.integers(0, 3, int(dead.sum()))]
    if len(full) >= 2:
        v[cls == 0] = np.float32(-2.5)
    return v, cls


def mixed_values(n, seed):
    """All the value sets one after another in stretches of 97 elements, with NaN / +-inf sprinkled in."""
    rng = np.random.default_rng([n, seed])
    kinds = sorted(VALUE_SETS)
    v = np.empty(n, np.float32)
    for k, lo in enumerate(range(0, n, 97)):
        hi = min(n, lo + 97)
        v[lo:hi] = VALUE_SETS[kinds[k % len(kinds)]](hi - lo, rng)
    bad = rng.random(n) < 0.03
    v[bad] = NONFINITE[rng.integers(0, 3, int(bad.sum()))]
    return v


BLOCK_KINDS = ("d2", "ties", "no_finite", "zeros", "mixed_sign", "one_finite")


def trimmed_block(per_class, kind, rng):
    """One block of r3d_trimmed_means_f32 input."""
    n = per_class
    if kind == "d2":                                                     # squared distances: non-negative, a long tail, some misses
        v = (rng.random(n) ** 2 * 10.0 ** rng.uniform(-4, 1, n)).astype(np.float32)
        v[rng.random(n) < 0.05] = np.inf
    elif kind == "ties":                                                 # the statistic is a value that many elements share
        v = rng.random(n).astype(np.float32) * 2
        v[rng.random(n) < 0.6] = np.float32(1.0)
    elif kind == "no_finite":
        v = NONFINITE[rng.integers(0, 3, n)]
    elif kind == "zeros":                                                # -0.0 and +0.0 in the middle of the order
        v = rng.normal(size=n).astype(np.float32)
        z = rng.random(n) < 0.5
        v[z] = np.where(rng.random(int(z.sum())) < 0.5, np.float32(-0.0), np.float32(0.0))
    elif kind == "mixed_sign":
        v = (rng.normal(size=n) * 10.0 ** rng.uniform(-3, 3, n)).astype(np.float32)
        v[rng.random(n) < 0.05] = np.nan
    else:
        v = np.full(n, np.nan, np.float32)
        v[rng.integers(0, n)] = np.float32(-7.25)
    return np.asarray(v, np.float32)


def trimmed_case(n_classes, per_class, shift, seed=0):
    """n_classes blocks, block c of kind BLOCK_KINDS[(c + shift) % 6]."""
    rng = np.random.default_rng([n_classes, per_class, shift, seed])
    kinds = [BLOCK_KINDS[(c + shift) % len(BLOCK_KINDS)] for c in range(n_classes)]
    return np.concatenate([trimmed_block(per_class, k, rng) for k in kinds]), kinds


def transforms(k, seed):
    """k row-major 4x4: a similarity each, then (from the second on) one anisotropic scale with shear, one with a translation of
    1e6, one identity -- what a multi-start never sends and a general 4x4 entry point still has to take."""
    rng = np.random.default_rng([k, seed])
    Ts = np.tile(np.eye(4), (k, 1, 1))
    for j in range(k):
        q, _ = np.linalg.qr(rng.normal(size=(3, 3)))
        Ts[j, :3, :3] = rng.uniform(0.5, 2.0) * q
        Ts[j, :3, 3] = rng.normal(size=3) * 5
    if k >= 2:
        Ts[1, :3, :3] = np.diag([0.25, 3.0, -1.5]) + np.triu(rng.normal(size=(3, 3)) * 0.1, 1)
    if k >= 3:
        Ts[2, :3, 3] = (1e6, -2e6, 3.5e6)
    if k >= 4:
        Ts[3] = np.eye(4)
    return Ts
