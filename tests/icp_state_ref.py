"""Plain restatement of what every estimation loop shares (csrc/r3d_sums_dev.h): the device-resident ICP state and its update,
and the fp64 sums as EXACT integers.  NumPy, Python integers and fractions only; the library is not imported.

The state (include/r3d.h, R3D_ICP_STATE_DOUBLES = 512 doubles):
  [0..15] T_total, [16..31] the last step, [32] steps solved, [33] status (sticky), [34] rms of the last step, [35] its weight,
  [36..47] reserved (zero after a reset, never written), [48 + k] rms of step k for k < 464.

The sums.  With coordinates that are integers of magnitude <= 512 and normals +-e_x, +-e_y, +-e_z every product a pair adds is
an integer, and every partial sum of them stays below 2^53: fp64 then adds them without rounding in ANY order and under any
choice of fused multiply-add, so the device's reduction tree has exactly one right answer, bit for bit, and a row left out or
taken twice anywhere in it changes that answer.  exact_sums18 / exact_sums29 work in int64 (the inputs bound every term below
2^21 and the sums below 2^41, far from 2^63); `headroom` asserts the 2^53 bound for the sum of the terms' MAGNITUDES, which
bounds every partial sum of every order.  tests/test_icp_state_host.py checks the int64 builders against loops over Python
integers and against the fp64 oracles."""
from fractions import Fraction

import numpy as np

STATE_DOUBLES = 512
T_TOTAL, T_STEP, ITERS, STATUS, RMS, PAIRS, HISTORY = 0, 16, 32, 33, 34, 35, 48
HISTORY_SLOTS = STATE_DOUBLES - HISTORY          # 464
U = 2.0 ** -53
IDENTITY = np.eye(4).reshape(16)
NO_ROW = 0xffffffff


# ---- the state ---------------------------------------------------------------------------------------------------------------
def reset():
    st = np.zeros(STATE_DOUBLES)
    st[T_TOTAL:T_TOTAL + 16] = IDENTITY
    st[T_STEP:T_STEP + 16] = IDENTITY
    return st


def matmul4(A, B):
    """A . B of two row-major 4x4 (16 doubles each), every entry summed over m = 0..3 in ascending order from 0.0, each product
    rounded (no fused multiply-add)"""
    out = np.zeros(16)
    for r in range(4):
        for c in range(4):
            v = 0.0
            for m in range(4):
                v += float(A[4 * r + m]) * float(B[4 * m + c])
            out[4 * r + c] = v
    return out


def advance(state, T, rms, bad, weight):
    """icp_state_advance: the state after one more step (a new array)."""
    st = np.array(state, dtype=np.float64)
    T = np.asarray(T, dtype=np.float64).reshape(16)
    st[T_TOTAL:T_TOTAL + 16] = matmul4(T, state[T_TOTAL:T_TOTAL + 16])
    st[T_STEP:T_STEP + 16] = T
    it = int(state[ITERS])
    if HISTORY + it < STATE_DOUBLES:
        st[HISTORY + it] = rms
    st[ITERS] = float(it + 1)
    if bad:
        st[STATUS] = 1.0
    st[RMS] = rms
    st[PAIRS] = weight
    return st


def product_exact(T, tot):
    """T . tot in fractions: (16 exact entries, 16 magnitudes sum_m |T[r][m]| |tot[m][c]|)"""
    Tf, Sf = [Fraction(float(v)) for v in T], [Fraction(float(v)) for v in tot]
    val, mag = [], []
    for r in range(4):
        for c in range(4):
            val.append(sum(Tf[4 * r + m] * Sf[4 * m + c] for m in range(4)))
            mag.append(sum(abs(Tf[4 * r + m] * Sf[4 * m + c]) for m in range(4)))
    return val, mag


def _integral(a):
    return all(float(v) == int(v) and abs(v) < 2 ** 20 for v in a)


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).reshape(-1).view(np.uint64)


def check_product(got, T, tot, what=""):
    """got = T . tot as the device may have formed it: every entry within 4 u sum_m |T[r][m]| |tot[m][c]| of the exact product
    (four additions starting from 0.0, each product either rounded or fused into its addition.  Not fused: the four product
    roundings together are at most u times that magnitude, and the first addition, to 0.0, is exact, so three additions round,
    each by at most u times a partial sum no larger than the magnitude.  Fused: four roundings of such partial sums.  Either
    way 4 u times the magnitude, to first order in u).  Where nothing can round -- T is the
    identity, or both matrices hold small integers -- the bits must be the exact product's."""
    T, tot, got = [np.asarray(a, dtype=np.float64).reshape(16) for a in (T, tot, got)]
    assert np.isfinite(T).all() and np.isfinite(tot).all(), (what, "non-finite factor")
    val, mag = product_exact(T, tot)
    exact = np.array_equal(bits(T), bits(IDENTITY)) or (_integral(T) and _integral(tot))
    for k in range(16):
        if exact:
            assert bits(got[k:k + 1])[0] == bits(np.array([float(val[k])]))[0], (what, "T_total entry %d: %r, exactly %r" % (k, got[k], float(val[k])))
        else:
            assert np.isfinite(got[k]), (what, "T_total entry %d is %r" % (k, got[k]))
            err = abs(Fraction(float(got[k])) - val[k])
            assert err <= 4 * Fraction(U) * mag[k], (what, "T_total entry %d: %r is %.3g from T_step . T_total, bound %.3g"
                                                     % (k, got[k], float(err), float(4 * Fraction(U) * mag[k])))


def check_advance(prev, got, T, rms, bad, weight, t_tol=0.0, rms_tol=0.0, what=""):
    """THE comparator of the state tests: `got` (512 doubles read back) is `prev` advanced by the step (T, rms, bad, weight).
      * [16..31] equals T within t_tol per entry (0: bit for bit; a degenerate step is the identity bit for bit whatever t_tol);
      * [34] equals rms within rms_tol (0: bit for bit); [35] equals weight bit for bit;
      * [0..15] is the step AS STORED times prev's T_total, by check_product;
      * all other cells equal advance(prev, the stored step, the stored rms, bad, weight) bit for bit: the count, the sticky
        status, the history slot (the stored rms's bits, in the slot the old count names, only while it is below 512), the
        reserved cells and the untouched rest of the history."""
    prev, got = np.asarray(prev, dtype=np.float64), np.asarray(got, dtype=np.float64)
    assert prev.shape == (STATE_DOUBLES,) and got.shape == (STATE_DOUBLES,)
    T = np.asarray(T, dtype=np.float64).reshape(16)
    step = got[T_STEP:T_STEP + 16]
    if bad or t_tol == 0.0:
        assert np.array_equal(bits(step), bits(IDENTITY if bad else T)), (what, "T_step", step, T)
    else:
        assert np.isfinite(step).all() and np.abs(step - T).max() <= t_tol, (what, "T_step differs by %.3g" % np.abs(step - T).max())
    if not (np.isfinite(rms) and np.isfinite(got[RMS])):               # sums of the caller's with a NaN / inf among them
        assert (np.isnan(rms) and np.isnan(got[RMS])) or got[RMS] == rms, (what, "rms", got[RMS], rms)
    elif rms_tol == 0.0:
        assert bits(got[RMS:RMS + 1])[0] == bits(np.array([rms]))[0], (what, "rms", got[RMS], rms)
    else:
        assert abs(got[RMS] - rms) <= rms_tol, (what, "rms %r, want %r within %.3g" % (got[RMS], rms, rms_tol))
    check_product(got[T_TOTAL:T_TOTAL + 16], step, prev[T_TOTAL:T_TOTAL + 16], what)
    want = advance(prev, step, got[RMS], bad, weight)
    want[T_TOTAL:T_TOTAL + 16] = got[T_TOTAL:T_TOTAL + 16]
    diff = np.flatnonzero(bits(got) != bits(want))
    assert diff.size == 0, (what, "state cells %s: got %s, want %s" % (diff[:8].tolist(), got[diff[:8]].tolist(), want[diff[:8]].tolist()))


def rms_tolerance(s):
    """How far the device's rms of 18 sums may lie from the host's: both evaluate e = s16 + s17 - 2 (s7 + s11 + s15) and
    sqrt(e / n) in fp64, the device free to fuse the multiply into the subtraction.  Each sees e within 4 u (|s16| + |s17| +
    2 (|s7| + |s11| + |s15|)) of the exact value; the quotient and the root add a relative 3 u."""
    s = np.asarray(s, dtype=np.float64)
    if not (np.isfinite(s).all() and s[0] > 0):
        return 0.0
    mag = abs(s[16]) + abs(s[17]) + 2 * (abs(s[7]) + abs(s[11]) + abs(s[15]))
    e = max(s[16] + s[17] - 2.0 * (s[7] + s[11] + s[15]), 0.0)
    rms = np.sqrt(e / s[0])
    de = 8 * U * mag
    return float(np.sqrt((e + de) / s[0]) - rms + 6 * U * rms)


# ---- exact sums --------------------------------------------------------------------------------------------------------------
def headroom(terms_abs_sum, what=""):
    """every partial sum of every summation order is bounded by the sum of the magnitudes: below 2^53 it is exact in fp64"""
    assert int(terms_abs_sum) < 2 ** 53, (what, int(terms_abs_sum))


def _finite_rows(a):
    return np.isfinite(a).all(axis=1)


def _ints(a, ok):
    """int64 copy of the rows `ok` of an integer-valued f32 array (other rows 0)"""
    a = np.asarray(a, dtype=np.float32)
    out = np.zeros(a.shape, dtype=np.int64)
    v = a[ok].astype(np.float64)
    assert np.array_equal(v, np.rint(v)) and (np.abs(v) <= 4096).all(), "the exact sums take integer-valued coordinates"
    out[ok] = v.astype(np.int64)
    return out


def _pairing(n, idx, n_tgt):
    if idx is None:
        j = np.arange(n, dtype=np.int64)
    else:
        j = np.asarray(idx, dtype=np.uint32).astype(np.int64)
    inside = j < n_tgt
    return np.where(inside, j, 0), inside


def _gate(ok, d2, max_d2):
    if max_d2 >= 0:
        with np.errstate(invalid="ignore"):
            ok = ok & (np.asarray(d2, dtype=np.float32) <= np.float32(max_d2))
    return ok


def exact_sums18(p, q, idx, d2=None, max_d2=-1.0, n_tgt=None):
    """The 18 sums of r3d_icp_sums.h over the pairs (p[k], q[idx[k]]) (idx None: q[k]) as Python integers:
    n, sum p (3), sum q (3), sum p_a q_b (9, a major), sum |p|^2, sum |q|^2.  A pair takes part when idx[k] < n_tgt, d2[k] <=
    max_d2 (fp32 comparison; only when max_d2 >= 0) and all six coordinates are finite."""
    p, q = np.asarray(p, dtype=np.float32).reshape(-1, 3), np.asarray(q, dtype=np.float32).reshape(-1, 3)
    n_tgt = q.shape[0] if n_tgt is None else int(n_tgt)
    j, ok = _pairing(p.shape[0], idx, n_tgt)
    ok = _gate(ok, d2, max_d2)
    qj = q[j]
    ok = ok & _finite_rows(p) & _finite_rows(qj)
    P, Q = _ints(p, ok)[ok], _ints(qj, ok)[ok]
    out = [int(ok.sum())] + [int(P[:, a].sum()) for a in range(3)] + [int(Q[:, a].sum()) for a in range(3)]
    out += [int((P[:, a] * Q[:, b]).sum()) for a in range(3) for b in range(3)]
    out += [int((P * P).sum()), int((Q * Q).sum())]
    headroom(max(int((np.abs(P)[:, :, None] * np.abs(Q)[:, None, :]).sum(axis=0).max(initial=0)), out[16], out[17], out[0]), "18 sums")
    return out


def axis_class(n_int):
    """direction class of an axis-aligned normal +-e_a (include/r3d_internal_api.h): 8 a + 4 [negative]"""
    a = np.abs(n_int).argmax(axis=1)
    return 8 * a + 4 * (n_int[np.arange(len(a)), a] < 0)


def exact_sums29(p, q, nrm, idx, d2=None, max_d2=-1.0, n_tgt=None, trim_q=0.0):
    """The 29 sums of r3d_plane_sums.h over the admissible pairs (p[k], q[idx[k]], nrm[idx[k]]) as Python integers:
    pairs, sum r^2, sum J r (6), upper triangle of sum J J^T (21, row-major), r = n . (p - q), J = [p x n ; n].
    Admissible (include/r3d_internal_api.h): idx[k] < n_tgt, the normal is not zero, p, q and the normal are finite, d2[k] <=
    max_d2 when max_d2 >= 0.  0 < trim_q < 1 (gate_scale 1): of the admissible pairs of one direction class only those whose r^2
    is <= the class's order statistic of rank floor(trim_q (m - 1)) among its m values.  Normals must be +-e_a.
    Returns (sums, mask of the pairs that took part)."""
    p, q, nrm = [np.asarray(a, dtype=np.float32).reshape(-1, 3) for a in (p, q, nrm)]
    n_tgt = q.shape[0] if n_tgt is None else int(n_tgt)
    j, ok = _pairing(p.shape[0], idx, n_tgt)
    ok = _gate(ok, d2, max_d2)
    qj, nj = q[j], nrm[j]
    ok = ok & _finite_rows(p) & _finite_rows(qj) & _finite_rows(nj)
    ok = ok & (np.nan_to_num(nj) != 0).any(axis=1)
    P, Q, N = _ints(p, ok), _ints(qj, ok), _ints(nj, ok)
    assert (np.abs(N[ok]).sum(axis=1) == 1).all(), "axis-aligned unit normals"
    r = (N * (P - Q)).sum(axis=1)
    if 0.0 < trim_q < 1.0:
        r2 = r * r
        assert (r2[ok] < 2 ** 24).all()                               # (float)(r r) is that integer
        cls = axis_class(N)
        keep = np.zeros_like(ok)
        tq = float(np.float32(trim_q))
        for c in np.unique(cls[ok]):
            m = ok & (cls == c)
            v = np.sort(r2[m])
            keep |= m & (r2 <= v[int(np.floor(tq * (v.size - 1)))])
        ok = keep
    P, N, r = P[ok], N[ok], r[ok]
    J = np.concatenate([np.cross(P, N), N], axis=1) if len(P) else np.zeros((0, 6), dtype=np.int64)
    out = [int(ok.sum()), int((r * r).sum())] + [int((J[:, a] * r).sum()) for a in range(6)]
    out += [int((J[:, a] * J[:, b]).sum()) for a in range(6) for b in range(a, 6)]
    aJ, ar = np.abs(J), np.abs(r)
    headroom(max([out[0], out[1]] + [int((aJ[:, a] * ar).sum()) for a in range(6)] + [int((aJ[:, a] * aJ[:, a]).sum()) for a in range(6)]),
             "29 sums")                                               # |J_a J_b| <= (J_a^2 + J_b^2) / 2: the diagonal bounds the rest
    return out, ok


def as_f64(ints):
    """the integers as the doubles they are (each below 2^53: exact)"""
    for v in ints:
        assert abs(v) < 2 ** 53
    return np.array([float(v) for v in ints], dtype=np.float64)


def check_sums(got, want_ints, what=""):
    """THE comparator of the exact-sums tests: every sum bit for bit the integer (so +0.0 for an empty sum, never -0.0)"""
    want = as_f64(want_ints)
    got = np.asarray(got, dtype=np.float64)
    assert got.shape == want.shape, (what, got.shape)
    diff = np.flatnonzero(bits(got) != bits(want))
    assert diff.size == 0, (what, "sums %s: got %s, exactly %s" % (diff.tolist(), got[diff].tolist(), want[diff].tolist()))


# ---- integer cases -----------------------------------------------------------------------------------------------------------
AXES = np.array([[1, 0, 0], [-1, 0, 0], [0, 1, 0], [0, -1, 0], [0, 0, 1], [0, 0, -1]], dtype=np.float32)


def int_cloud(n, seed, lim=512):
    """n rows of integer coordinates in [-lim, lim], none of them -0.0"""
    rng = np.random.default_rng([seed, n])
    return rng.integers(-lim, lim + 1, size=(n, 3)).astype(np.float32) + np.float32(0.0)


def axis_normals(n, seed, zero_share=0.05):
    """n axis-aligned unit normals over all six directions, a share of them the zero vector ("no plane here")"""
    rng = np.random.default_rng([seed, n, 7])
    nrm = AXES[rng.integers(0, 6, size=n)] + np.float32(0.0)
    nrm[rng.random(n) < zero_share] = 0.0
    return nrm


def sprinkle_bad_rows(idx, n_tgt, seed):
    """some entries == n_tgt, n_tgt + 1 and 0xffffffff: a caller's index array is data"""
    rng = np.random.default_rng([seed, len(idx), 11])
    idx = np.array(idx, dtype=np.uint32)
    for k, v in enumerate((n_tgt, n_tgt + 1, NO_ROW)):
        idx[rng.random(len(idx)) < 0.02] = v
        idx[(k * 97) % len(idx)] = v                                   # at least one of each, also in a cloud of a few rows
    return idx


def sprinkle_nonfinite(a, seed):
    """rows with a NaN, a +inf or a -inf coordinate (and one row holding +inf and -inf together)"""
    rng = np.random.default_rng([seed, len(a), 13])
    a = np.array(a, dtype=np.float32)
    for k, v in enumerate((np.nan, np.inf, -np.inf)):
        rows = np.flatnonzero(rng.random(len(a)) < 0.01)
        a[rows, rng.integers(0, 3, size=len(rows))] = v
        a[(k * 89 + 3) % len(a), k] = v
    if len(a) > 300:
        a[300, 0], a[300, 1] = np.inf, -np.inf
    return a


def good_sums18(seed, lim=8, n=60):
    """18 sums of a well-posed fit: an integer cloud, turned by a quarter about an axis, shifted, with integer noise"""
    rng = np.random.default_rng([seed, 17])
    p = rng.integers(-lim, lim + 1, size=(n, 3))
    R = [np.array([[0, -1, 0], [1, 0, 0], [0, 0, 1]]), np.array([[1, 0, 0], [0, 0, -1], [0, 1, 0]]), np.eye(3, dtype=np.int64)][seed % 3]
    q = p @ R.T + rng.integers(-3, 4, size=3) + rng.integers(-1, 2, size=(n, 3))
    return as_f64(exact_sums18(p.astype(np.float32), q.astype(np.float32), None))
