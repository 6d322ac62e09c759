"""GPU: what every estimation loop shares (csrc/r3d_sums_dev.h) at its edges, against tests/icp_state_ref.py.

Exact sums.  Integer coordinates of magnitude <= 512 and axis-aligned normals make every one of the 18 / 29 sums an integer
below 2^53: whatever the order of the reduction and whatever the compiler fuses, the device has one right answer, bit for bit,
and a row dropped or taken twice by block_reduce_store, fold_rows or a grid-stride loop changes it.  The row counts come from
the device's compute-unit count C: r3d_icp_accumulate_dev leaves min(ceil(n / 256), 4 C) partial rows, r3d_nn_index_query_sums
ceil(n / (256 S)), r3d_icp_plane_accumulate min(ceil(n / 256), C), r3d_track_accumulate ceil(H W / 1024).

The state machine, driven with sums of the test's choosing through r3d_icp_solve_dev and through each loop with scenes that make
a step degenerate: all 512 doubles, in a buffer with guard bands, against icp_state_ref.check_advance after every call."""
import importlib

import numpy as np
import pytest

import icp_state_ref as SR
import sums_bits_cases as SC
import track_ref as TR
from helpers import PKG, r3d as _r3d
from oracle import fusion_ref as O
from oracle import icp_ref as OI
from oracle import plane_ref as PR
from test_gpu_bounds import Guarded, guard  # noqa: F401  (guard is a fixture)
from test_gpu_track import assert_sums
from test_icp_state_host import NONFINITE, assert_skipped_or_finite, degenerate_sums18, host_umeyama

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def R():
    return _r3d()


@pytest.fixture(scope="module")
def L(R):
    return importlib.import_module(PKG + "._lib")


@pytest.fixture(scope="module")
def icp(R):
    return importlib.import_module(PKG + ".icp")


@pytest.fixture(scope="module")
def ctx(R):
    c = R.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def CU():
    return SC.compute_units()


def u32(a):
    return np.ascontiguousarray(a, dtype=np.uint32)


# ---- 3a: exact sums at the row-count edges ---------------------------------------------------------------------------------------
ACC_SIZES = {"1": lambda c: 1, "255": lambda c: 255, "256": lambda c: 256, "257": lambda c: 257, "65536": lambda c: 65536,
             "65537": lambda c: 65537, "cap": lambda c: 256 * 4 * c, "cap+1": lambda c: 256 * 4 * c + 1,
             "3cap+77": lambda c: 3 * 256 * 4 * c + 77}


@pytest.mark.parametrize("size", list(ACC_SIZES))
def test_accumulate_dev_sums_are_the_integers(ctx, L, guard, CU, size):
    """r3d_icp_accumulate_dev: one partial row, exactly 256, 257 (thread 0 of the finish folds a second row), the block cap 4 C
    and one pair more (the first workgroup's grid-stride loop makes a second trip for one pair), three trips and a ragged end.
    A permutation, an index array with rows at and past n_tgt and 0xffffffff, no index array (row k with row k, and the moments
    form d_tgt == d_src), a gate that some d2 meet exactly and some miss by one, rows with NaN / +inf / -inf in p and in q."""
    n = ACC_SIZES[size](CU)
    m = n + 5
    rng = np.random.default_rng(n)
    p, q = SR.int_cloud(n, 1), SR.int_cloud(m, 2)
    perm = u32(rng.permutation(m)[:n])
    wild = SR.sprinkle_bad_rows(perm, m, 3)
    d2 = rng.integers(0, 9, size=n).astype(np.float32)
    assert n < 9 or ((d2 == 4).any() and (d2 == 5).any())
    pn, qn = SR.sprinkle_nonfinite(p, 4), SR.sprinkle_nonfinite(q, 5)
    gp, gq, gperm, gwild, gd2 = guard(p.nbytes, 4, p), guard(q.nbytes, 8, q, seed=1), guard(n * 4, 4, perm, seed=2), guard(n * 4, 0, wild, seed=3), \
        guard(n * 4, 4, d2, seed=4)
    gpn, gqn = guard(p.nbytes, 0, pn, seed=5), guard(q.nbytes, 4, qn, seed=6)
    out = guard(18 * 8, 8, seed=7)

    def run(d_p, d_q, n_tgt, d_idx, d_d2, max_d2):
        L.check(ctx.lib.r3d_icp_accumulate_dev(ctx.handle, d_p.ptr, n, d_q.ptr, n_tgt, d_idx.ptr if d_idx else None,
                                               d_d2.ptr if d_d2 else None, max_d2, 0.0, out.ptr))
        return out.read(np.float64)
    SR.check_sums(run(gp, gq, m, gperm, None, -1.0), SR.exact_sums18(p, q, perm), "permutation")
    SR.check_sums(run(gp, gq, m, gwild, None, -1.0), SR.exact_sums18(p, q, wild), "rows past the target")
    SR.check_sums(run(gp, gq, m, None, None, -1.0), SR.exact_sums18(p, q, None), "no index array")
    mom = SR.exact_sums18(p, p, None)
    assert mom[16] == mom[17] == mom[7] + mom[11] + mom[15]
    SR.check_sums(run(gp, gp, n, None, None, -1.0), mom, "moments")
    SR.check_sums(run(gp, gq, m, gwild, gd2, 4.0), SR.exact_sums18(p, q, wild, d2, 4.0), "gated")
    want = SR.exact_sums18(pn, qn, wild)
    assert want[0] < n or n == 1
    SR.check_sums(run(gpn, gqn, m, gwild, None, -1.0), want, "non-finite rows")
    for g in (gp, gq, gperm, gwild, gd2, gpn, gqn):
        g.unchanged()


QUERY_SIZES = {"1": lambda s: 1, "256S-1": lambda s: 256 * s - 1, "256S": lambda s: 256 * s, "256S+1": lambda s: 256 * s + 1,
               "256x256S": lambda s: 256 * 256 * s, "256x256S+1": lambda s: 256 * 256 * s + 1}


@pytest.mark.parametrize("size", list(QUERY_SIZES))
@pytest.mark.parametrize("S", [1, 2, 4])
def test_query_sums_are_the_integers(ctx, L, icp, guard, S, size):
    """r3d_nn_index_query_sums, S sources per lane: ceil(n / (256 S)) partial rows, never capped -- 256 and 257 rows at the two
    largest sizes.  Target: the 16^3 lattice of even integers; sources: lattice points moved by -1 / 0 / +1 per axis, so every
    d2 is 0, 1, 2 or 3.  Expected: the integers over the idx and d2 THE SAME CALL returned (checked to be a point at that squared
    distance; which of several equally near ones is pinned in test_gpu_icp.py).  Unsorted sources, sources in the index's order,
    the same query again (bounded by the matches it finds in place) and the wave-local warm kernel (256 sources per row)."""
    n = QUERY_SIZES[size](S)
    g = np.arange(16, dtype=np.float32) * 2
    tgt = np.stack(np.meshgrid(g, g, g, indexing="ij"), axis=-1).reshape(-1, 3).copy()
    rng = np.random.default_rng([n, S])
    src = tgt[rng.integers(0, 4096, size=n)] + rng.integers(-1, 2, size=(n, 3)).astype(np.float32) + np.float32(0.0)
    gt = guard(tgt.nbytes, 0, tgt)
    gs = guard(src.nbytes, 0, src, seed=1)
    gi, gd, out = guard(n * 4, 4, seed=2), guard(n * 4, 8, seed=3), guard(18 * 8, 8, seed=4)
    index = icp.NNIndex(ctx, gt.ptr, 4096)
    ctx.set_tuning("nn_variant", S)
    try:
        def run(presorted, max_d2, cloud):
            L.check(ctx.lib.r3d_nn_index_query_sums(index.handle, gs.ptr, n, gi.ptr, gd.ptr, presorted, max_d2, 0.0, out.ptr))
            got, idx, d2 = out.read(np.float64), gi.read(np.uint32), gd.read(np.float32)
            assert (idx < 4096).all()
            diff = cloud.astype(np.int64) - tgt[idx].astype(np.int64)
            assert np.array_equal((diff * diff).sum(axis=1), d2.astype(np.int64)) and (d2 <= 3).all()
            want = SR.exact_sums18(cloud, tgt, idx, d2, max_d2)
            assert want[0] == (n if max_d2 < 0 else int((d2 <= max_d2).sum()))
            SR.check_sums(got, want, (presorted, max_d2))
            return d2
        d2 = run(0, -1.0, src)
        assert n < 64 or ((d2 == 1).any() and (d2 == 2).any())          # the gate below is met exactly and missed by one
        run(0, 1.0, src)
        index.sort_cloud(gs.ptr, n)
        ordered = gs.read(np.float32, (-1, 3))
        assert np.array_equal(np.sort(ordered.view("f4,f4,f4").ravel()), np.sort(src.view("f4,f4,f4").ravel()))
        run(1, -1.0, ordered)
        run(1, 1.0, ordered)                                            # warm: bounded by the matches already in gi
        ctx.set_tuning("nn_warm", 3)
        run(1, -1.0, ordered)                                           # the wave-local kernel
        run(1, 1.0, ordered)
    finally:
        ctx.set_tuning("nn_warm", 0)
        ctx.set_tuning("nn_variant", 0)
        index.close()
    gt.unchanged()


PLANE_SIZES = {"1": lambda c: 1, "255": lambda c: 255, "256": lambda c: 256, "257": lambda c: 257, "256C": lambda c: 256 * c,
               "256C+1": lambda c: 256 * c + 1, "5x256C+3": lambda c: 5 * 256 * c + 3}


@pytest.mark.parametrize("size", list(PLANE_SIZES))
def test_plane_accumulate_sums_are_the_integers(ctx, L, guard, CU, size):
    """r3d_icp_plane_accumulate, untrimmed and rank-trimmed (trim_q 0.5, gate_scale 1): min(ceil(n / 256), C) partial rows --
    one, two (the second holding one pair), C, and C with a second and a sixth grid-stride trip.  Normals over all six axis
    directions and some zero vectors, rows at and past n_tgt, source rows with NaN / +-inf.  The trimmed gates are worked out
    in integers per direction class by the rank rule of include/r3d_internal_api.h (every (float)(r r) is an integer < 2^24).
    The finish folds at most C rows here: on a device of 256 compute units or fewer fold_rows' second trip cannot be reached
    through this entry (r3d_track_accumulate and the 18-sum entries reach it)."""
    n = PLANE_SIZES[size](CU)
    m = n + 9
    rng = np.random.default_rng(n + 1)
    p, q, nrm = SR.sprinkle_nonfinite(SR.int_cloud(n, 11), 12), SR.int_cloud(m, 13), SR.axis_normals(m, 14)
    idx = SR.sprinkle_bad_rows(rng.integers(0, m, size=n), m, 15)
    d2 = rng.integers(0, 9, size=n).astype(np.float32)
    gp, gq, gn, gi, gd = guard(p.nbytes, 4, p), guard(q.nbytes, 0, q, seed=1), guard(q.nbytes, 8, nrm, seed=2), guard(n * 4, 4, idx, seed=3), \
        guard(n * 4, 0, d2, seed=4)
    out = guard(29 * 8, 8, seed=5)

    def run(d_d2, max_d2, trim_q):
        L.check(ctx.lib.r3d_icp_plane_accumulate(ctx.handle, gp.ptr, n, gq.ptr, gn.ptr, m, gi.ptr, d_d2.ptr if d_d2 else None, max_d2,
                                                 trim_q, 1.0, out.ptr))
        return out.read(np.float64)
    want, kept = SR.exact_sums29(p, q, nrm, idx, n_tgt=m)
    if n >= 255:
        assert 0.5 * n < want[0] < n and len(set(SR.axis_class(nrm[idx[kept]].astype(np.int64)).tolist())) == 6
    SR.check_sums(run(None, -1.0, 0.0), want, "untrimmed")
    SR.check_sums(run(gd, 4.0, 0.0), SR.exact_sums29(p, q, nrm, idx, d2, 4.0, m)[0], "gated")
    trimmed, kept_t = SR.exact_sums29(p, q, nrm, idx, n_tgt=m, trim_q=0.5)
    if n >= 255:
        assert 0.4 * want[0] < trimmed[0] < 0.7 * want[0]
    SR.check_sums(run(None, -1.0, 0.5), trimmed, "trimmed")
    for g in (gp, gq, gn, gi, gd):
        g.unchanged()


@pytest.mark.parametrize("h,w", [(1, 1), (32, 32), (512, 512), (512, 513), (513, 513)])
def test_track_accumulate_counts_its_matches_exactly(ctx, L, h, w):
    """r3d_track_accumulate: ceil(H W / 1024) partial rows -- 1, 1, 256, 257 and 258, the last two with a second fold trip.
    sums[0] is the number of matched pixels, exactly; the other 28 sums against the reference's plain fp64 sums under the rule
    of test_gpu_track.py (the projection decides the pairs, so this is no integer case)."""
    case = TR.analytic_case(h, w, 2.0, 1.0, (0.03, 0.02, -0.04))
    S = TR.inverse_pose(case["model_row"])
    ref = TR.associate(case["src_vertex"], None, case["model_vertex"], case["model_normal"], case["model_row"], S, case["K"], 0.5, -1.0)
    assert TR.rounding_margin(ref.upv) >= 1e-9
    n = h * w
    bufs = [Guarded(ctx, n * 12, off, case[k], seed=s) for s, (k, off) in enumerate([("src_vertex", 0), ("model_vertex", 8), ("model_normal", 4)])]
    g_match = Guarded(ctx, n * 4, 4, seed=9)
    try:
        cam = ctx.camera(h, w, *case["K"])
        sums, pose, S = np.zeros(29), np.ascontiguousarray(case["model_row"]), np.ascontiguousarray(S)
        L.check(ctx.lib.r3d_track_accumulate(ctx.handle, cam.handle, bufs[0].ptr, None, bufs[1].ptr, bufs[2].ptr, pose.ctypes.data,
                                             S.ctypes.data, 0.5, -1.0, sums.ctypes.data, g_match.ptr, None))
        match = g_match.read(np.int32)
        assert sums[0] == float((match >= 0).sum()) and np.array_equal(match, ref.match)
        assert n < 1024 or sums[0] >= 0.4 * n
        assert_sums(sums, ref.sums)
        for b in bufs:
            b.unchanged()
    finally:
        for b in bufs + [g_match]:
            b.free()


def test_continued_loops_count_their_pairs_exactly(ctx, L, icp, R):
    """A loop called again on the same state takes the warm query and, in the plane and tracking loops, the finish that writes
    no sums (sums_out == NULL).  65537 sources (257 rows, one pair in the last): [35] is the exact number of admissible pairs
    after every call -- the sources within the gate of the d2 the call left behind, the matches whose target has a normal."""
    src, tgt, _, _ = OI.synthetic_pair(n_tgt=65537, n_src=65537, s=1.0, angle_deg=0.3, t_norm=0.02, noise=0.005, seed=5)
    dev = icp.IcpDevice(src, tgt, ctx, True)
    try:
        dev.state_reset()
        dev.iterate(2, with_scale=False)                                # (two steps: the d2 left behind are the converged ones)
        st = dev.d_state.download(np.float64, 512)
        assert st[35] == 65537.0 and st[33] == 0.0
        gate = float(np.float32(np.sort(dev.d_d2.download(np.float32, dev.n))[dev.n // 2]))
        for k, iters in enumerate((1, 1, 2)):
            dev.iterate(iters, with_scale=False, max_d2=gate)
            st = dev.d_state.download(np.float64, 512)
            d2 = dev.d_d2.download(np.float32, dev.n)
            assert st[35] == float((d2 <= np.float32(gate)).sum()) and 0 < st[35] < 65537, (k, st[35])
            assert st[32] == 2 + sum((1, 1, 2)[:k + 1]) and st[33] == 0.0
    finally:
        dev.free()
    # point-to-plane: an organised 260 x 256 target, the first 65537 rows of the other view as the source
    syn = importlib.import_module(PKG + ".synthetic")
    h, w = 260, 256
    v = syn.two_views(h, w, yaw_deg=15.0, baseline=(0.35, 0.05, -0.2), depth_noise=0.002, seed=1)
    pa, pb = O.unproject(v["depth_a"], *v["K"]).astype(np.float32), O.unproject(v["depth_b"], *v["K"]).astype(np.float32)
    dev = icp.PlaneIcpDevice(pb[:65537], pa, (h, w), ctx=ctx, init=v["T_ab"])
    try:
        nrm = dev.normals()
        has = (nrm != 0).any(axis=1)
        assert 0.5 < has.mean() < 1.0
        dev.state_reset()
        for k, iters in enumerate((1, 1, 2)):
            dev.iterate(iters, 0.0, 1.0, -1.0)
            st = dev.d_state.download(np.float64, 512)
            idx = dev.d_idx.download(np.uint32, dev.n)
            assert st[35] == float(has[idx].sum()) and st[33] == 0.0, (k, st[35], has[idx].sum())
    finally:
        dev.free()
    # tracking: the pairs of the LAST pass are those of the reference association at the pose the state held before it
    tracking = importlib.import_module(PKG + ".tracking")
    case = TR.analytic_case(48, 64, 2.0, 1.0, (0.03, 0.02, -0.04))
    S = TR.inverse_pose(case["model_row"])
    dev = tracking.TrackDevice(case["src_vertex"], case["model_vertex"], case["model_normal"], case["model_row"], S, case["K"], ctx=ctx)
    try:
        T_before = np.eye(4)
        for k in range(3):
            dev.iterate(1, 0.5)
            st = dev.d_state.download(np.float64, 512)
            ref = TR.associate(case["src_vertex"], None, case["model_vertex"], case["model_normal"], case["model_row"], S, case["K"], 0.5,
                               -1.0, T_before)
            assert TR.rounding_margin(ref.upv) >= 1e-9
            assert st[35] == float((ref.match >= 0).sum()) and st[32] == k + 1
            T_before = st[:16].reshape(4, 4).copy()
    finally:
        dev.free()


# ---- 3b: the state machine, driven directly -----------------------------------------------------------------------------------------
T_TOL = 1e-12      # the project's bound for its solver against the oracle on inputs of this size (tests/test_icp_host.py)


class Driver:
    """r3d_icp_solve_dev on a state between guard bands; every call is checked in full against the reference's advance fed with
    the host solver's step for the same sums."""

    def __init__(self, ctx, L, guard):
        self.ctx, self.L = ctx, L
        self.state = guard(512 * 8, 8, seed=21)
        self.sums = guard(18 * 8, 8, seed=22)
        self.reset()

    def reset(self):
        self.L.check(self.ctx.lib.r3d_icp_state_reset(self.ctx.handle, self.state.ptr))
        self.prev = self.state.read(np.float64)

    def solve(self, s, with_scale, what=""):
        s = np.ascontiguousarray(s, dtype=np.float64)
        self.L.check(self.ctx.lib.r3d_memcpy_h2d(self.ctx.handle, self.sums.ptr, s.ctypes.data, s.nbytes))
        self.L.check(self.ctx.lib.r3d_icp_solve_dev(self.ctx.handle, self.sums.ptr, with_scale, self.state.ptr))
        got = self.state.read(np.float64)                               # (asserts the bands)
        T, rms, bad = host_umeyama(s, with_scale)
        SR.check_advance(self.prev, got, T, rms, bad, s[0], t_tol=T_TOL, rms_tol=SR.rms_tolerance(s), what=what)
        assert self.sums.read(np.float64).tobytes() == s.tobytes()
        prev, self.prev = self.prev, got
        return prev, got, bad


def test_reset_state_is_the_reference_s(ctx, L, guard):
    d = Driver(ctx, L, guard)
    assert d.prev.tobytes() == SR.reset().tobytes()


@pytest.mark.parametrize("with_scale", [0, 1])
def test_degenerate_step_in_the_middle(ctx, L, guard, with_scale):
    """good, good, degenerate, good -- for all zeros, two pairs and five identical points: the degenerate call leaves the
    identity step and T_total's bits, sets the status for good, counts, and records its rms like any other; the next good step
    composes onto the kept total as step . T_total (the two good steps before it do not commute)."""
    for name, bad_sums in degenerate_sums18():
        d = Driver(ctx, L, guard)
        for k in range(2):
            _, got, bad = d.solve(SR.good_sums18(k), with_scale, (name, k))
            assert not bad and got[33] == 0.0
        two = got
        before, got, bad = d.solve(bad_sums, with_scale, (name, "degenerate"))
        assert bad and got[:16].tobytes() == before[:16].tobytes() and got[16:32].tobytes() == SR.IDENTITY.tobytes()
        assert got[33] == 1.0 and got[32] == 3.0 and got[35] == bad_sums[0] and got[50] == got[34]
        if name == "no spread":
            assert got[34] > 0.0
        before, got, bad = d.solve(SR.good_sums18(2 if name != "zeros" else 1), with_scale, (name, "after"))
        assert not bad and got[33] == 1.0 and got[32] == 4.0 and got[:16].tobytes() != before[:16].tobytes()
        assert two[:16].tobytes() == before[:16].tobytes()
        assert np.abs(SR.matmul4(before[:16], got[16:32]) - got[:16]).max() > 1e-3    # T_total . step, the wrong order, is not it


def test_history_stops_at_slot_511_and_the_counter_goes_on(ctx, L, icp, guard):
    """470 calls with distinct rms values, then a reset: the first 464 in [48..511] bit for bit, [32] = 470, [34] the last,
    [36..47] still +0.0, the bands intact; IcpDevice.state() reports 464 history entries; the reset state is reset()'s bytes."""
    d = Driver(ctx, L, guard)
    base = SR.good_sums18(0)
    rms = []
    for k in range(470):
        s = base.copy()
        s[17] += 4.0 * k                                                # sum |q|^2: moves the rms, not the fit
        _, got, bad = d.solve(s, 1, k)
        rms.append(got[34])
    assert len(set(rms)) == 470 and got[32] == 470.0 and got[33] == 0.0
    assert got[48:512].tobytes() == np.array(rms[:464]).tobytes() and got[34] == rms[-1]
    assert got[36:48].tobytes() == np.zeros(12).tobytes()
    dev = icp.IcpDevice(np.zeros((3, 3), np.float32), np.zeros((3, 3), np.float32), ctx, False)
    try:
        dev.d_state.upload(got)
        st = dev.state()
        assert st["iterations"] == 470 and len(st["rms_history"]) == 464 and st["rms_history"] == rms[:464]
    finally:
        dev.free()
    d.reset()
    assert d.prev.tobytes() == SR.reset().tobytes()


@pytest.mark.parametrize("with_scale", [0, 1])
def test_non_finite_sums_never_reach_the_total(ctx, L, guard, with_scale):
    """A NaN, +inf or -inf in each of the 18 slots in turn, the rest from a good fit: the fit is skipped (identity step, status
    1) or the step is a finite one; T_total is finite after every call and after a good step on top."""
    d = Driver(ctx, L, guard)
    d.solve(SR.good_sums18(0), with_scale)
    skipped = 0
    for slot in range(18):
        for v in NONFINITE:
            s = SR.good_sums18(1)
            s[slot] = v
            _, got, bad = d.solve(s, with_scale, (slot, v))
            assert_skipped_or_finite(got[16:32], bad, (slot, v))
            assert np.isfinite(got[:16]).all(), (slot, v)
            skipped += bad
    assert skipped >= 12 and got[33] == 1.0                             # n and sum p in any of the three: no fit at all
    _, got, bad = d.solve(SR.good_sums18(2), with_scale)
    assert not bad and np.isfinite(got[:32]).all()


def test_device_solve_against_the_oracle(ctx, L, guard):
    """The 120 trials of test_icp_host.py's comparison with the oracle's numpy SVD, solved on the device from a reset state."""
    d = Driver(ctx, L, guard)
    rng = np.random.default_rng(0)
    worst = 0.0
    for trial in range(120):
        p = rng.normal(size=(40, 3)) * rng.uniform(0.1, 10)
        if trial % 5 == 0:
            p[:, 2] = 0.3
        _s, _t, T, _ = OI.synthetic_pair(n_tgt=8, n_src=4, seed=trial, s=rng.uniform(0.3, 3), angle_deg=rng.uniform(0, 179))
        q = p @ T[:3, :3].T + T[:3, 3] + rng.normal(size=p.shape) * 1e-3
        sums = OI.pair_sums(p.astype(np.float32), q.astype(np.float32), np.arange(40))
        for ws in (True, False):
            d.reset()
            _, got, bad = d.solve(sums, int(ws), trial)
            assert not bad
            worst = max(worst, np.abs(got[16:32].reshape(4, 4) - OI.umeyama_from_sums(sums, ws)).max())
    print("device solve against the oracle, worst |dT| over 240 fits: %.3g" % worst)
    assert worst < 1e-12, worst


# ---- 3c: degenerate steps inside each loop ----------------------------------------------------------------------------------------
def full_state(buf):
    return buf.download(np.float64, 512)


def assert_identity_state(st, iterations, what=""):
    assert st[33] == 1.0 and st[32] == float(iterations), (what, st[32:36])
    assert st[:16].tobytes() == SR.IDENTITY.tobytes() and st[16:32].tobytes() == SR.IDENTITY.tobytes(), what
    assert st[36:48].tobytes() == np.zeros(12).tobytes() and not st[48 + iterations:].any(), what


@pytest.mark.parametrize("culled", [False, True])
@pytest.mark.parametrize("source", ["far away", "one point 300 times"])
def test_similarity_loop_skips_and_then_goes_on(ctx, icp, culled, source):
    """r3d_icp_iterate, brute force and indexed.  A source 100 units from the target under a gate of 1 (no pair at all), or 300
    copies of one point (300 pairs, no spread): three iterations leave the status, three counted steps, identity matrices bit
    for bit and the cloud byte for byte.  Three ungated iterations on the same state then compose onto it like a host-stepped
    loop's, the status still 1.  (No coordinate is -0.0, so the identity move keeps every bit.)"""
    rng = np.random.default_rng(7)
    tgt = (rng.random((2000, 3)) * 4).astype(np.float32)
    if source == "far away":
        good = OI.apply_T32(tgt[rng.permutation(2000)[:1500]], OI.synthetic_pair(n_tgt=8, n_src=4, s=1.0, angle_deg=1.0, t_norm=0.05, seed=2)[2])
        src, max_d2, pairs = good + np.float32(100.0), 1.0, 0.0
    else:
        good = None
        src, max_d2, pairs = np.tile(np.array([[1.5, 2.25, 0.75]], np.float32), (300, 1)), -1.0, 300.0
    dev = icp.IcpDevice(src, tgt, ctx, culled)
    try:
        dev.state_reset()
        dev.sort_source()
        start = dev.d_src.download(np.uint8, dev.n * 12)
        dev.iterate(3, with_scale=False, max_d2=max_d2)
        st = full_state(dev.d_state)
        assert_identity_state(st, 3, source)
        assert st[35] == pairs and st[34] == st[50]
        assert dev.d_src.download(np.uint8, dev.n * 12).tobytes() == start.tobytes()
        if good is None:
            return
        # the same state, the cloud brought within reach: three good steps against a host-stepped loop over the same cloud
        dev.move_source(np.array([[1, 0, 0, -100.0], [0, 1, 0, -100.0], [0, 0, 1, -100.0], [0, 0, 0, 1]]))
        moved = dev.source()
        dev.iterate(3, with_scale=False)
        st = full_state(dev.d_state)
        b = icp.IcpDevice(moved, tgt, ctx, culled)
        T_total = np.eye(4)
        for _ in range(3):
            b.nn()
            T = icp.umeyama_from_sums(b.sums(), with_scale=False)
            b.move_source(T)
            T_total = T @ T_total
        b.free()
        assert st[33] == 1.0 and st[32] == 6.0 and st[35] == 1500.0
        np.testing.assert_allclose(st[:16].reshape(4, 4), T_total, rtol=0, atol=1e-9)
        assert np.abs(T_total - np.eye(4)).max() > 1e-3
    finally:
        dev.free()


@pytest.mark.parametrize("keep_original", [False, True])
def test_plane_loop_on_one_wall_then_on_a_scene(ctx, L, icp, keep_original):
    """r3d_icp_iterate_plane with and without d_src_orig: a camera facing one wall square on (many pairs, three freedoms open)
    leaves status 1, more than 6 pairs, identity matrices bit for bit and the cloud byte for byte.  The state is then copied to
    a device object holding a two-view scene: its good steps compose onto the kept state, and the status stays."""
    syn = importlib.import_module(PKG + ".synthetic")
    h, w = 60, 80
    z, _q, _t, K = syn.room_view(h, w, 0.0, (0.0, 0.0, 0.0), fx=2.0 * w)
    p = O.unproject(z.astype(np.float32), *K).astype(np.float32) + np.float32(0.0)
    dev = icp.PlaneIcpDevice(p, p, (h, w), ctx=ctx)
    try:
        dev.state_reset()
        start = dev.d_src.download(np.uint8, dev.n * 12)
        L.check(ctx.lib.r3d_icp_iterate_plane(ctx.handle, dev.index.handle, dev.d_src0.ptr if keep_original else None, dev.d_src.ptr, dev.n,
                                              dev.d_nrm.ptr, dev.d_idx.ptr, dev.d_d2.ptr, 3, 0.5, 20.0, -1.0, dev.d_state.ptr))
        st = full_state(dev.d_state)
        assert_identity_state(st, 3)
        assert st[35] > 6 and st[35] > 0.3 * dev.n
        assert dev.d_src.download(np.uint8, dev.n * 12).tobytes() == start.tobytes()
    finally:
        dev.free()
    h, w = 72, 96
    v = syn.two_views(h, w, yaw_deg=15.0, baseline=(0.35, 0.05, -0.2), depth_noise=0.002, seed=1)
    pa, pb = O.unproject(v["depth_a"], *v["K"]).astype(np.float32), O.unproject(v["depth_b"], *v["K"]).astype(np.float32)
    from test_gpu_plane_icp import rough
    T0 = rough(v["T_ab"])
    keep = np.any(pb != 0, axis=1)
    _T_ref, hist = PR.icp_point_to_plane(pb[keep], pa, PR.organized_normals(pa, h, w, 0.05), T0=T0, max_iter=3, trim_q=0.5, gate_scale=20.0, tol=0.0)
    dev = icp.PlaneIcpDevice(pb[keep], pa, (h, w), ctx=ctx, init=T0)
    try:
        dev.state_reset()
        dev.d_state.upload(st)
        prev = st
        for k in range(3):
            L.check(ctx.lib.r3d_icp_iterate_plane(ctx.handle, dev.index.handle, None, dev.d_src.ptr, dev.n, dev.d_nrm.ptr, dev.d_idx.ptr,
                                                  dev.d_d2.ptr, 1, 0.5, 20.0, -1.0, dev.d_state.ptr))
            got = full_state(dev.d_state)
            # the stored step and rms are the device's own; everything else must follow from them and the state before
            SR.check_advance(prev, got, got[16:32], got[34], 0, got[35], what=k)
            assert abs(got[34] - hist[k]) <= 1e-6 * hist[0] and got[35] > 1000
            prev = got
        assert prev[33] == 1.0 and prev[32] == 6.0 and np.abs(prev[:16] - SR.IDENTITY).max() > 1e-3
    finally:
        dev.free()


def test_tracking_loop_on_a_single_plane(ctx):
    """r3d_track_iterate: a model that is one plane facing the camera, as tests/test_track_host.py has it on the CPU."""
    from test_track_host import IDENT_ROW, plane_maps
    tracking = importlib.import_module(PKG + ".tracking")
    h, w = 24, 32
    K = (0.8 * w, 0.8 * w, (w - 1) / 2.0, (h - 1) / 2.0)
    mv, mn = plane_maps(h, w, K, 2.0)
    sv, _ = plane_maps(h, w, K, 2.05)
    guess = IDENT_ROW.copy()
    guess[9:] = (0.01, -0.02, 0.0)
    S = TR.inverse_pose(guess)
    ref = TR.associate(sv, None, mv, mn, guess, S, K, 0.5, -1.0)
    dev = tracking.TrackDevice(sv, mv, mn, guess, S, K, ctx=ctx)
    try:
        dev.iterate(4, 0.5)
        st = full_state(dev.d_state)
        assert_identity_state(st, 4)
        assert st[35] == float((ref.match >= 0).sum()) and st[35] > 0.5 * h * w
        assert dev.pose().tobytes() == TR.pose_from(np.eye(4), S).tobytes()
    finally:
        dev.free()


def test_tsdf_track_on_a_wall_gives_the_guess_back(ctx, R):
    """r3d_tsdf_track on the wall volume of test_gpu_tsdf.py: pairs, a singular system, the guess bit for bit, status 1."""
    import tsdf_ref
    s = tsdf_ref.wall_scene(False)
    V = R.TSDFVolume(s["origin"], s["vs"], s["dims"], s["tr"], ctx=ctx)
    try:
        buf = ctx.alloc(s["depths"].nbytes).upload(s["depths"])
        V.integrate_device(ctx.camera(24, 32, *s["K"]), buf.ptr, s["depths"].dtype, 1, s["poses"], s["scale"])
        ctx.sync()
        buf.free()
        guess = np.array(s["poses"][0], dtype=np.float64).reshape(12) + 0.0
        guess[9] = 0.01
        row, info = V.track(s["depths"][0], guess, intrinsics=s["K"], n_iters=4)
        assert info["status"] == 1 and info["pairs"] > 6 and info["iterations"] == 4
        assert row.tobytes() == guess.tobytes()
    finally:
        V.close()
