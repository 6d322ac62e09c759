"""CPU: tests/icp_state_ref.py against independent arithmetic, the host solvers on degenerate and non-finite sums, and the
mutation checks of the two comparators the GPU tests (tests/test_gpu_icp_state.py) rely on: a comparator that a wrong state
machine or a short reduction could pass would pin nothing."""
import ctypes as C
import importlib
from fractions import Fraction

import numpy as np
import pytest

import icp_state_ref as SR
import icp_parts_ref as REF
import track_ref as TR
from helpers import PKG
from oracle import icp_ref as OI
from oracle import plane_ref as PR


def _lib():
    return importlib.import_module(PKG + "._lib")


def host_umeyama(sums, with_scale):
    """(T [16], rms, bad) of r3d_umeyama_from_sums: the host build of the code the device solve runs"""
    L = _lib()
    s, T, rms = np.ascontiguousarray(sums, dtype=np.float64), np.full(16, 7.0), C.c_double(-7.0)
    rc = L.load().r3d_umeyama_from_sums(s.ctypes.data, int(with_scale), T.ctypes.data, C.byref(rms))
    assert rc in (L.OK, L.ERR_INVALID)
    return T, rms.value, int(rc != L.OK)


def host_plane_step(sums):
    L = _lib()
    s, T, rms = np.ascontiguousarray(sums, dtype=np.float64), np.full(16, 7.0), C.c_double(-7.0)
    rc = L.load().r3d_plane_step_from_sums(s.ctypes.data, T.ctypes.data, C.byref(rms))
    assert rc in (L.OK, L.ERR_INVALID)
    return T, rms.value, int(rc != L.OK)


def random_step(rng, scale=True):
    """a similarity [sR t; 0 1] as 16 doubles"""
    q, _ = np.linalg.qr(rng.normal(size=(3, 3)))
    T = np.eye(4)
    T[:3, :3] = q * (rng.uniform(0.5, 2.0) if scale else 1.0)
    T[:3, 3] = rng.normal(size=3) * 3
    return T.reshape(16)


# ---- advance -----------------------------------------------------------------------------------------------------------------
def matmul4_fused(A, B):
    """the other contraction: every product fused into its addition (one rounding per step), in exact arithmetic"""
    out = np.zeros(16)
    for r in range(4):
        for c in range(4):
            v = 0.0
            for m in range(4):
                v = float(Fraction(v) + Fraction(float(A[4 * r + m])) * Fraction(float(B[4 * m + c])))
            out[4 * r + c] = v
    return out


def test_advance_against_fractions_on_random_sequences():
    """60 random similarity steps: T_total stays within the per-entry bound of the exact product of the stored step and the
    previous total under BOTH contractions, and equals the exact product of all steps to 60 x that; every other cell as stated."""
    rng = np.random.default_rng(5)
    st = SR.reset()
    exact = [Fraction(int(v)) for v in SR.IDENTITY]
    for k in range(60):
        T, rms, bad = random_step(rng), float(rng.random()), int(k % 7 == 3)
        if bad:
            T = SR.IDENTITY.copy()
        new = SR.advance(st, T, rms, bad, 100.0 + k)
        SR.check_advance(st, new, T, rms, bad, 100.0 + k, what=k)
        fused = new.copy()
        fused[:16] = matmul4_fused(T, st[:16])
        SR.check_advance(st, fused, T, rms, bad, 100.0 + k, what=("fused", k))
        exact = [sum(Fraction(float(T[4 * r + m])) * exact[4 * m + c] for m in range(4)) for r in range(4) for c in range(4)]
        st = new
    assert st[SR.ITERS] == 60 and st[SR.STATUS] == 1.0 and not st[36:48].any() and not st[48 + 60:].any()
    err = max(abs(Fraction(float(st[k])) - exact[k]) for k in range(16))
    assert float(err) <= 60 * 4 * SR.U * float(max(abs(v) for v in exact)) * 16


def test_advance_scripted_sequence():
    """integer steps (exact products: bits), a degenerate step in the middle, the history's last slot and the steps after it"""
    A = np.array([0, -1, 0, 2, 1, 0, 0, -3, 0, 0, 1, 5, 0, 0, 0, 1], dtype=np.float64)       # quarter turn about z, shift
    B = np.array([1, 0, 0, 1, 0, 0, -1, 0, 0, 1, 0, 4, 0, 0, 0, 1], dtype=np.float64)        # quarter turn about x, shift
    st = SR.reset()
    assert SR.bits(st).tolist() == SR.bits(np.concatenate([np.eye(4).reshape(16), np.eye(4).reshape(16), np.zeros(480)])).tolist()
    s1 = SR.advance(st, A, 0.5, 0, 10.0)
    s2 = SR.advance(s1, B, 0.25, 0, 11.0)
    assert np.array_equal(s2[:16].reshape(4, 4), B.reshape(4, 4) @ A.reshape(4, 4))           # step . T_total, not T_total . step
    assert not np.array_equal(B.reshape(4, 4) @ A.reshape(4, 4), A.reshape(4, 4) @ B.reshape(4, 4))
    s3 = SR.advance(s2, SR.IDENTITY, 0.0, 1, 0.0)
    assert SR.bits(s3[:16]).tolist() == SR.bits(s2[:16]).tolist() and s3[33] == 1.0 and s3[32] == 3.0 and s3[50] == 0.0 and s3[34] == 0.0
    s4 = SR.advance(s3, A, 0.125, 0, 12.0)
    assert s4[33] == 1.0 and np.array_equal(s4[:16].reshape(4, 4), A.reshape(4, 4) @ B.reshape(4, 4) @ A.reshape(4, 4))
    assert s4[48:52].tolist() == [0.5, 0.25, 0.0, 0.125] and s4[32] == 4.0 and s4[34] == 0.125 and s4[35] == 12.0
    for prev, new, step in ((st, s1, (A, 0.5, 0, 10.0)), (s1, s2, (B, 0.25, 0, 11.0)), (s2, s3, (SR.IDENTITY, 0.0, 1, 0.0)), (s3, s4, (A, 0.125, 0, 12.0))):
        SR.check_advance(prev, new, *step)
    st = s4
    for k in range(4, 470):
        new = SR.advance(st, SR.IDENTITY, float(k), 0, 1.0)
        SR.check_advance(st, new, SR.IDENTITY, float(k), 0, 1.0)
        st = new
    assert st[32] == 470.0 and st[511] == 463.0 and st[34] == 469.0 and not st[36:48].any()


# ---- the integer sums against other arithmetic ---------------------------------------------------------------------------------
def slow_sums18(p, q, idx, d2, max_d2, n_tgt):
    """the same rules, one pair at a time, in Python integers"""
    out = [0] * 18
    for k in range(len(p)):
        j = k if idx is None else int(idx[k])
        if j >= n_tgt or (max_d2 >= 0 and not np.float32(d2[k]) <= np.float32(max_d2)):
            continue
        if not (np.isfinite(p[k]).all() and np.isfinite(q[j]).all()):
            continue
        P, Q = [int(v) for v in p[k]], [int(v) for v in q[j]]
        out[0] += 1
        for a in range(3):
            out[1 + a] += P[a]
            out[4 + a] += Q[a]
            for b in range(3):
                out[7 + 3 * a + b] += P[a] * Q[b]
            out[16] += P[a] * P[a]
            out[17] += Q[a] * Q[a]
    return out


def slow_sums29(p, q, nrm, idx, n_tgt):
    out = [0] * 29
    for k in range(len(p)):
        j = int(idx[k])
        if j >= n_tgt or not nrm[j].any() or not (np.isfinite(p[k]).all() and np.isfinite(q[j]).all() and np.isfinite(nrm[j]).all()):
            continue
        P, Q, N = [int(v) for v in p[k]], [int(v) for v in q[j]], [int(v) for v in nrm[j]]
        r = sum(N[a] * (P[a] - Q[a]) for a in range(3))
        J = [P[1] * N[2] - P[2] * N[1], P[2] * N[0] - P[0] * N[2], P[0] * N[1] - P[1] * N[0]] + N
        out[0] += 1
        out[1] += r * r
        m = 8
        for a in range(6):
            out[2 + a] += J[a] * r
            for b in range(a, 6):
                out[m] += J[a] * J[b]
                m += 1
    return out


@pytest.mark.parametrize("n", [1, 257, 1500])
def test_exact_sums18_against_python_integers_and_the_oracle(n):
    m = n + 40
    p, q = SR.sprinkle_nonfinite(SR.int_cloud(n, 1), 1), SR.sprinkle_nonfinite(SR.int_cloud(m, 2), 2)
    rng = np.random.default_rng(n)
    idx = SR.sprinkle_bad_rows(rng.integers(0, m, size=n), m, 3)
    d2 = rng.integers(0, 9, size=n).astype(np.float32)
    for use_idx, max_d2 in ((idx, -1.0), (idx, 4.0), (None, -1.0)):
        got = SR.exact_sums18(p, q, use_idx, d2, max_d2, m)
        assert got == slow_sums18(p, q, use_idx, d2, max_d2, m)
        # the oracle's plain fp64 sums of the same integers are exact too (it has no rule for rows >= n_tgt: those are cut here)
        rows = np.arange(n) if use_idx is None else np.flatnonzero(use_idx < m)
        j = rows if use_idx is None else use_idx[rows]
        want = OI.pair_sums(p[rows], q, j, d2[rows], max_d2)
        SR.check_sums(want, got, (n, max_d2))
    if n > 1:
        assert got[0] < n                                            # the non-finite rows were left out


@pytest.mark.parametrize("n", [1, 300, 2000])
def test_exact_sums29_against_python_integers_and_the_oracle(n):
    m = n + 25
    p, q, nrm = SR.sprinkle_nonfinite(SR.int_cloud(n, 4), 4), SR.int_cloud(m, 5), SR.axis_normals(m, 6)
    rng = np.random.default_rng(n)
    idx = SR.sprinkle_bad_rows(rng.integers(0, m, size=n), m, 7)
    got, kept = SR.exact_sums29(p, q, nrm, idx, n_tgt=m)
    assert got == slow_sums29(p, q, nrm, idx, m) and got[0] == kept.sum()
    SR.check_sums(PR.plane_sums(p, q, nrm, idx), got, n)
    # trimmed: small residuals so that ranks tie, against the oracle's selection and the parts reference's order statistic
    q2 = q.copy()
    inside = idx < m
    q2[idx[inside]] = np.nan_to_num(p[inside], nan=0.0, posinf=0.0, neginf=0.0) + rng.integers(-6, 7, size=(int(inside.sum()), 3)).astype(np.float32)
    got, kept = SR.exact_sums29(p, q2, nrm, idx, n_tgt=m, trim_q=0.5)
    SR.check_sums(PR.plane_sums(p, q2, nrm, idx, trim_q=0.5, gate_scale=1.0), got, ("trimmed", n))
    r2, cls = PR.plane_residuals(p, q2, nrm, idx)
    gates, counts = REF.class_quantiles(r2, cls, 24, 0.5)
    want_kept = np.array([cls[k] != 255 and r2[k] <= gates[cls[k]] for k in range(n)])
    assert np.array_equal(kept, want_kept) and counts.sum() >= got[0]
    if n >= 300:
        assert 0 < got[0] < counts.sum()


def test_exact_sums29_against_the_tracking_reference():
    """an integer raster through tests/track_ref.py's association: fx = fy = 1, cx = cy = 0, identity poses and points (u, v, 1)
    project onto their own pixel; the model holds integer points and axis normals.  Its plain fp64 sums are the integers."""
    h, w = 9, 13
    u, v = np.meshgrid(np.arange(w), np.arange(h))
    sv = np.stack([u, v, np.ones_like(u)], axis=-1).astype(np.float32)
    rng = np.random.default_rng(9)
    mv = sv + rng.integers(-2, 3, size=sv.shape).astype(np.float32)
    mn = SR.axis_normals(h * w, 8).reshape(h, w, 3)
    sv[2, 3, 0] = np.nan
    ident = np.concatenate([np.eye(3).reshape(9), np.zeros(3)])
    ref = TR.associate(sv, None, mv, mn, ident, np.eye(4), (1.0, 1.0, 0.0, 0.0), 3.0, -1.0)
    assert (ref.match >= 0).sum() > 0.5 * h * w
    idx = np.where(ref.match >= 0, ref.match, SR.NO_ROW).astype(np.uint32)
    got, kept = SR.exact_sums29(sv.reshape(-1, 3), mv.reshape(-1, 3), mn.reshape(-1, 3), idx)
    assert np.array_equal(kept, ref.match >= 0)
    SR.check_sums(ref.sums, got)


# ---- the host solvers on degenerate and non-finite sums ----------------------------------------------------------------------------
def degenerate_sums18():
    """all zeros; two pairs; five identical points (no spread, pairs = 5)"""
    two = SR.as_f64(SR.exact_sums18(np.array([[1, 2, 3], [4, 0, -2]], np.float32), np.array([[2, 2, 3], [4, 1, -2]], np.float32), None))
    same = SR.as_f64(SR.exact_sums18(np.tile(np.array([[3, -2, 5]], np.float32), (5, 1)), SR.int_cloud(5, 3, 8), None))
    return [("zeros", np.zeros(18)), ("two pairs", two), ("no spread", same)]


def test_host_umeyama_on_degenerate_sums():
    for name, s in degenerate_sums18():
        for ws in (0, 1):
            T, rms, bad = host_umeyama(s, ws)
            assert bad == 1 and np.array_equal(SR.bits(T), SR.bits(SR.IDENTITY)), (name, ws, T)
            assert np.isfinite(rms) and rms >= 0.0
        if name == "zeros":
            assert rms == 0.0
    T, rms, bad = host_umeyama(SR.good_sums18(0), 1)
    assert bad == 0 and np.isfinite(T).all() and rms > 0


def single_plane_sums29(n=400):
    """many pairs, one plane: three freedoms open"""
    p, q = SR.int_cloud(n, 21, 30), SR.int_cloud(n, 22, 30)
    nrm = np.tile(SR.AXES[4:5], (n, 1))
    return SR.as_f64(SR.exact_sums29(p, q, nrm, np.arange(n, dtype=np.uint32))[0])


def good_sums29(n=400):
    p = SR.int_cloud(n, 23, 30)
    q = p + np.random.default_rng(24).integers(-1, 2, size=p.shape).astype(np.float32)
    return SR.as_f64(SR.exact_sums29(p, q, SR.axis_normals(n, 25, 0.0), np.arange(n, dtype=np.uint32))[0])


def test_host_plane_step_on_degenerate_sums():
    few = good_sums29().copy()
    few[0] = 5.0
    for name, s in (("zeros", np.zeros(29)), ("five pairs", few), ("one plane", single_plane_sums29())):
        T, rms, bad = host_plane_step(s)
        assert bad == 1 and np.array_equal(SR.bits(T), SR.bits(SR.IDENTITY)), (name, T)
        assert np.isfinite(rms)
    assert single_plane_sums29()[0] == 400
    T, rms, bad = host_plane_step(good_sums29())
    assert bad == 0 and np.isfinite(T).all()


def assert_skipped_or_finite(T, bad, what):
    """the header's rule for an undefined fit: it is skipped (identity, flagged) -- or the step is a finite one"""
    if bad:
        assert np.array_equal(SR.bits(T), SR.bits(SR.IDENTITY)), (what, T)
    assert np.isfinite(T).all(), (what, "flagged" if bad else "accepted", T)


NONFINITE = (np.nan, np.inf, -np.inf)


@pytest.mark.parametrize("with_scale", [0, 1])
def test_host_umeyama_never_returns_a_non_finite_step(with_scale):
    for slot in range(18):
        for v in NONFINITE:
            s = SR.good_sums18(1)
            s[slot] = v
            T, _rms, bad = host_umeyama(s, with_scale)
            assert_skipped_or_finite(T, bad, (with_scale, slot, v))


def test_host_plane_step_never_returns_a_non_finite_step():
    for slot in range(29):
        for v in NONFINITE + (1e308, -1e308, 1e200):
            s = good_sums29()
            s[slot] = v
            T, _rms, bad = host_plane_step(s)
            assert_skipped_or_finite(T, bad, (slot, v))


# ---- mutations: the comparators must tell ------------------------------------------------------------------------------------------
def mutant_right_product(state, T, rms, bad, weight):
    st = SR.advance(state, T, rms, bad, weight)
    st[:16] = SR.matmul4(state[:16], T)
    return st


def mutant_clears_status(state, T, rms, bad, weight):
    st = SR.advance(state, T, rms, bad, weight)
    st[SR.STATUS] = 1.0 if bad else 0.0
    return st


def mutant_history_one_late(state, T, rms, bad, weight):
    st = SR.advance(state, T, rms, bad, weight)
    it = int(state[SR.ITERS])
    if SR.HISTORY + it < SR.STATE_DOUBLES:
        st[SR.HISTORY + it] = state[SR.HISTORY + it]
    if SR.HISTORY + it + 1 < SR.STATE_DOUBLES:
        st[SR.HISTORY + it + 1] = rms
    return st


def mutant_stops_counting(state, T, rms, bad, weight):
    st = SR.advance(state, T, rms, bad, weight)
    if int(state[SR.ITERS]) >= SR.HISTORY_SLOTS:
        st[SR.ITERS] = state[SR.ITERS]
    return st


def script(n_steps):
    """good, good, degenerate, good, then distinct rms values: what the GPU test drives"""
    rng = np.random.default_rng(3)
    steps = []
    for k in range(n_steps):
        bad = int(k == 2)
        steps.append((SR.IDENTITY.copy() if bad or k >= 4 else random_step(rng), 0.5 + k / 1024.0, bad, 60.0 - bad * 58))
    return steps


def run_against(device_advance, steps):
    """Plays `steps` on a simulated device and checks every transition as the GPU test does; returns the first step that the
    comparator rejects (None: all passed)."""
    st = SR.reset()
    for k, (T, rms, bad, w) in enumerate(steps):
        new = device_advance(st, T, rms, bad, w)
        try:
            SR.check_advance(st, new, T, rms, bad, w)
        except AssertionError:
            return k
        st = new
    return None


def test_comparator_accepts_the_reference_and_rejects_each_mutant():
    steps = script(470)
    assert run_against(SR.advance, steps) is None
    assert run_against(mutant_right_product, steps) == 1             # the second good step: products differ from there on
    assert run_against(mutant_clears_status, steps) == 3             # the good step after the degenerate one
    assert run_against(mutant_history_one_late, steps) == 0
    assert run_against(mutant_stops_counting, steps) == 464


def test_sums_comparator_rejects_a_builder_that_drops_row_256():
    """257 rows: row 256 is the one pair of the second workgroup, the one row of a second fold trip"""
    for n in (257, 600):
        p, q = SR.int_cloud(n, 31), SR.int_cloud(n, 32)
        nrm = SR.axis_normals(n, 33, 0.0)
        idx = np.arange(n, dtype=np.uint32)
        keep = np.arange(n) != 256
        full18, short18 = SR.exact_sums18(p, q, idx), SR.exact_sums18(p[keep], q, idx[keep])
        SR.check_sums(SR.as_f64(full18), full18)
        with pytest.raises(AssertionError):
            SR.check_sums(SR.as_f64(short18), full18)
        full29, short29 = SR.exact_sums29(p, q, nrm, idx)[0], SR.exact_sums29(p[keep], q, nrm, idx[keep])[0]
        SR.check_sums(SR.as_f64(full29), full29)
        with pytest.raises(AssertionError):
            SR.check_sums(SR.as_f64(short29), full29)
    with pytest.raises(AssertionError):
        SR.check_sums(-np.zeros(18), [0] * 18)                       # -0.0 is not the empty sum
