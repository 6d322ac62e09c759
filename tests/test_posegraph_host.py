"""CPU: the host half of multiway registration -- r3d_information_from_sums and r3d_posegraph_optimize (csrc/r3d_posegraph.cpp,
posegraph.PoseGraph) against the NumPy restatement in tests/posegraph_ref.py, against closed-form answers and on every argument
error.  No GPU is touched."""
import importlib
import math

import numpy as np
import pytest

import posegraph_ref as REF
from helpers import PKG

L = importlib.import_module(PKG + "._lib")
PG = importlib.import_module(PKG + ".posegraph")
INF = float("inf")


def lib_optimize(poses, nodes, Ts, infos, unc, dist, pref=1.0, thr=0.25, max_iters=100):
    """(rc, poses, weights, report) of r3d_posegraph_optimize on copies of the inputs"""
    poses = np.ascontiguousarray(poses, np.float64).copy()
    m = len(nodes)
    nodes = np.ascontiguousarray(nodes, np.int32).reshape(m, 2)
    Ts, infos = np.ascontiguousarray(Ts, np.float64).reshape(m, 16), np.ascontiguousarray(infos, np.float64).reshape(m, 36)
    unc = np.ascontiguousarray(unc, np.uint8).reshape(m)
    w, rep = np.full(max(m, 1), -3.0), np.full(8, -3.0)
    rc = L.load().r3d_posegraph_optimize(poses.shape[0], poses.ctypes.data, m, nodes.ctypes.data, Ts.ctypes.data, infos.ctypes.data,
                                         unc.ctypes.data, dist, pref, thr, max_iters, w.ctypes.data, rep.ctypes.data)
    return rc, poses, w[:m], rep


def relative(truth, s, t):
    """the exact T of an edge (s, t): p_t = T p_s"""
    return REF.inverse(truth[t]) @ truth[s]


def perturbed(rng, truth, angle, shift):
    out = truth.copy()
    for i in range(1, len(truth)):
        out[i] = REF.random_pose(rng, angle, shift) @ truth[i]
    return out


def worst(poses, truth):
    d = [REF.pose_distance(a, b) for a, b in zip(poses, truth)]
    return max(a for a, _ in d), max(b for _, b in d)


# ---- 1. information matrix ------------------------------------------------------------------------------------------------------

def test_information_from_sums():
    rng = np.random.default_rng(0)
    q = rng.normal(size=(40, 3)) * 3.0 + (1.0, -2.0, 0.5)
    d2 = rng.uniform(0.0, 0.01, 40)
    hand = np.array([7.0, 1.5, -2.25, 3.0, 10.0, 0.5, -0.75, 20.0, 1.25, 30.0, 0.28])
    made = np.concatenate([[40.0], q.sum(0), [(q[:, a] * q[:, b]).sum() for a, b in ((0, 0), (0, 1), (0, 2), (1, 1), (1, 2), (2, 2))],
                           [d2.sum()]])
    for s, n_src in ((hand, 9), (made, 50), (made, 40)):
        info, fit, rmse = PG.information_from_sums(s, n_src)
        want, wfit, wrmse = REF.information_from_sums(s, n_src)
        assert np.array_equal(info, want) and fit == wfit and rmse == wrmse
        assert np.array_equal(info, info.T) and info[5, 5] == s[0]
    # ... and the sums do make sum G^T G
    direct = REF.information_direct(q)
    assert np.abs(PG.information_from_sums(made, 40)[0] - direct).max() <= 1e-12 * np.abs(direct).max()
    info, fit, rmse = PG.information_from_sums(np.zeros(11), 25)
    assert not info.any() and fit == 0.0 and rmse == 0.0
    assert PG.information_from_sums(np.zeros(11), 0)[1:] == (0.0, 0.0)
    assert PG.information_from_sums(hand, 0)[1] == 0.0
    lib = L.load()
    out = np.zeros(36)
    assert lib.r3d_information_from_sums(None, 1, out.ctypes.data, None, None) == L.ERR_INVALID
    assert lib.r3d_information_from_sums(hand.ctypes.data, 1, None, None, None) == L.ERR_INVALID
    assert lib.r3d_information_from_sums(hand.ctypes.data, -1, out.ctypes.data, None, None) == L.ERR_INVALID
    assert lib.r3d_information_from_sums(hand.ctypes.data, 9, out.ctypes.data, None, None) == 0        # fitness / rmse are optional
    with pytest.raises(ValueError):
        PG.information_from_sums(np.zeros(10), 1)


def test_restatement_jacobian_against_differences():
    """the restatement's analytic derivative of an edge residual, which the library's solver is compared with"""
    rng = np.random.default_rng(1)
    for _ in range(5):
        Xs, Xt, T = (REF.random_pose(rng, 1.0, 2.0) for _ in range(3))
        _, J = REF.edge_residual(Xs, Xt, T, jacobian=True)
        h = 1e-6
        for k in range(6):
            d = np.zeros(6)
            d[k] = h
            col_s = (REF.edge_residual(REF.se3_exp(d) @ Xs, Xt, T) - REF.edge_residual(REF.se3_exp(-d) @ Xs, Xt, T)) / (2 * h)
            col_t = (REF.edge_residual(Xs, REF.se3_exp(d) @ Xt, T) - REF.edge_residual(Xs, REF.se3_exp(-d) @ Xt, T)) / (2 * h)
            assert np.abs(col_s - J[:, k]).max() <= 1e-7 and np.abs(col_t + J[:, k]).max() <= 1e-7


# ---- 2. consistent graph --------------------------------------------------------------------------------------------------------

def test_consistent_graph_is_recovered():
    rng = np.random.default_rng(2)
    truth = np.stack([REF.random_pose(rng, 1.0, 2.0) for _ in range(8)])
    nodes = [((i + 1) % 8, i) for i in range(8)] + [(2, 6), (5, 1), (7, 3), (0, 4)]
    Ts = [relative(truth, s, t) for s, t in nodes]
    infos, unc = [np.eye(6)] * len(nodes), [0] * len(nodes)
    start = perturbed(rng, truth, 0.2, 0.2)
    rc, poses, w, rep = lib_optimize(start, nodes, Ts, infos, unc, 0.05)
    assert rc == 0, L.last_error()
    ang, dist = worst(poses, truth)
    print("consistent graph: %d iterations, cost %.3e -> %.3e, worst %.2e rad %.2e m" % (rep[2], rep[0], rep[1], ang, dist))
    assert ang <= 1e-6 and dist <= 1e-6
    assert np.array_equal(poses[0].view(np.uint64), start[0].view(np.uint64))
    assert np.array_equal(poses[:, 3], np.tile([0.0, 0.0, 0.0, 1.0], (8, 1)))
    assert np.array_equal(w, np.ones(len(nodes))) and rep[3] == 0 and rep[4] == 0 and not rep[5:].any() and rep[1] <= rep[0]
    want, _, wrep = REF.posegraph_optimize(start, nodes, Ts, infos, unc, 0.05)
    assert np.abs(poses - want).max() <= 1e-9
    assert abs(rep[0] - wrep["initial_cost"]) <= 1e-12 * wrep["initial_cost"]
    # the class gives the same bits
    g = PG.PoseGraph(start)
    for (s, t), T in zip(nodes, Ts):
        g.add_edge(s, t, T, np.eye(6))
    report = g.optimize(0.05)
    assert np.array_equal(g.poses.view(np.uint64), poses.view(np.uint64)) and report["iterations"] == int(rep[2])
    assert np.array_equal(g.edge_weights, w) and not g.pruned.any() and not report["max_iters_reached"]


# ---- 3. analytic spread ---------------------------------------------------------------------------------------------------------

def test_loop_error_is_spread_evenly():
    N, delta = 9, 0.5
    step = REF.pose(np.zeros(3), (1.0, 0.0, 0.0))
    start = np.stack([REF.pose(np.zeros(3), (float(k), 0.0, 0.0)) for k in range(N + 1)])
    nodes = [(k + 1, k) for k in range(N)] + [(N, 0)]
    Ts = [step] * N + [REF.pose(np.zeros(3), (N - delta, 0.0, 0.0))]
    rc, poses, w, rep = lib_optimize(start, nodes, Ts, [np.eye(6)] * (N + 1), [0] * (N + 1), 0.05, pref=INF)
    assert rc == 0, L.last_error()
    for k in range(N + 1):
        want = REF.pose(np.zeros(3), (k * (1.0 - delta / (N + 1)), 0.0, 0.0))
        assert np.abs(poses[k] - want).max() <= 1e-9, (k, poses[k])
    # every edge carries delta / (N + 1): the cost is (N + 1) (delta / (N + 1))^2
    assert abs(rep[1] - delta ** 2 / (N + 1)) <= 1e-12 and abs(rep[0] - delta ** 2) <= 1e-12


# ---- 4. false loop closures -----------------------------------------------------------------------------------------------------

def false_loop_graph():
    rng = np.random.default_rng(4)
    truth = np.stack([REF.random_pose(rng, 1.0, 2.0) for _ in range(10)])
    ring = [((i + 1) % 10, i) for i in range(10)]
    right, wrong = [(3, 0), (7, 2), (9, 5)], [(6, 1), (8, 4)]
    nodes = ring + right + wrong
    Ts = [relative(truth, s, t) for s, t in nodes]
    quarter = REF.pose((0.0, math.pi / 2, 0.0), (3.0, 0.0, 0.0))          # wrong by 90 degrees and 3 m
    for e in (13, 14):
        Ts[e] = quarter @ Ts[e]
    infos = [1000.0 * np.eye(6)] * len(nodes)
    unc = [0] * 10 + [1] * 5
    start = perturbed(rng, truth, 0.05, 0.05)
    return truth, nodes, Ts, infos, unc, start


def check_false_loops(poses, w, report_pruned, truth):
    ang, dist = worst(poses, truth)
    assert ang <= 1e-6 and dist <= 1e-6, (ang, dist)
    assert report_pruned == 2 and np.array_equal(w[13:], [0.0, 0.0]) and (w[10:13] > 0.99).all() and np.array_equal(w[:10], np.ones(10))


def test_false_loop_closures_are_pruned():
    truth, nodes, Ts, infos, unc, start = false_loop_graph()
    chi2 = [REF.edge_residual(truth[s], truth[t], T) @ infos[0] @ REF.edge_residual(truth[s], truth[t], T)
            for (s, t), T in zip(nodes[13:], Ts[13:])]
    assert min(chi2) > 8000                                              # against mu = 1 x 0.05^2 x 1000 = 2.5
    # the restatement alone meets the bounds ...
    want, ww, wrep = REF.posegraph_optimize(start, nodes, Ts, infos, unc, 0.05)
    check_false_loops(want, ww, wrep["pruned"], truth)
    # ... and so does the library
    rc, poses, w, rep = lib_optimize(start, nodes, Ts, infos, unc, 0.05)
    assert rc == 0, L.last_error()
    print("false loops: %d iterations, cost %.3e -> %.3e, weights %s" % (rep[2], rep[0], rep[1], w[10:]))
    check_false_loops(poses, w, int(rep[3]), truth)
    assert np.abs(poses - want).max() <= 1e-9 and rep[4] == 0
    g = PG.PoseGraph(start)
    for (s, t), T, lam, u in zip(nodes, Ts, infos, unc):
        g.add_edge(s, t, T, lam, bool(u))
    report = g.optimize(0.05)
    assert report["pruned"] == 2 and g.pruned.tolist() == [False] * 13 + [True] * 2
    assert np.array_equal(g.poses.view(np.uint64), poses.view(np.uint64))
    # without the robust weights the wrong chords drag the graph away
    rc, dragged, w_inf, rep_inf = lib_optimize(start, nodes, Ts, infos, unc, 0.05, pref=INF)
    assert rc == 0 and np.array_equal(w_inf, np.ones(15)) and rep_inf[3] == 0
    assert worst(dragged, truth)[1] > 0.1
    want_inf, _, _ = REF.posegraph_optimize(start, nodes, Ts, infos, unc, 0.05, preference_loop_closure=INF)
    assert worst(want_inf, truth)[1] > 0.1


# ---- 5. argument errors ---------------------------------------------------------------------------------------------------------

def small_graph():
    truth = np.stack([REF.pose((0.0, 0.1 * k, 0.0), (float(k), 0.0, 0.0)) for k in range(4)])
    nodes = [(1, 0), (2, 1), (3, 2), (3, 0)]
    return truth, nodes, [relative(truth, s, t) for s, t in nodes], [np.eye(6) * 5.0 for _ in nodes], [0, 0, 0, 1]


def _set(a, index, value):
    a = np.array(a, np.float64)
    a[index] = value
    return a


def bad_inputs():
    """name -> (poses, nodes, Ts, infos, unc) with one thing wrong"""
    poses, nodes, Ts, infos, unc = small_graph()
    asym = _set(infos[1], (0, 1), 1e-6)
    out = {
        "node out of range": (poses, [(1, 0), (2, 1), (4, 2), (3, 0)], Ts, infos, unc),
        "negative node": (poses, [(1, 0), (2, 1), (3, -1), (3, 0)], Ts, infos, unc),
        "s == t": (poses, [(1, 0), (2, 2), (3, 2), (3, 0)], Ts, infos, unc),
        "NaN in a pose": (_set(poses, (2, 0, 3), np.nan), nodes, Ts, infos, unc),
        "inf in a T": (poses, nodes, [Ts[0], _set(Ts[1], (1, 3), np.inf)] + Ts[2:], infos, unc),
        "NaN in an information matrix": (poses, nodes, Ts, [_set(infos[0], (2, 2), np.nan)] + infos[1:], unc),
        "asymmetric information matrix": (poses, nodes, Ts, [infos[0], asym] + infos[2:], unc),
        "negative diagonal": (poses, nodes, Ts, infos[:3] + [_set(infos[3], (4, 4), -1.0)], unc),
        "bottom row of a pose": (_set(poses, (1, 3, 3), 2.0), nodes, Ts, infos, unc),
        "bottom row of node 0": (_set(poses, (0, 3, 0), 1e-3), nodes, Ts, infos, unc),
        "bottom row of a T": (poses, nodes, Ts[:2] + [_set(Ts[2], (3, 1), 0.5)] + Ts[3:], infos, unc),
        "unconnected node": (poses, [(1, 0), (2, 1), (2, 0), (1, 2)], Ts, infos, unc),
    }
    return out


@pytest.mark.parametrize("name", sorted(bad_inputs()))
def test_invalid_graphs_are_refused(name):
    poses, nodes, Ts, infos, unc = bad_inputs()[name]
    rc, after, w, rep = lib_optimize(poses, nodes, Ts, infos, unc, 0.05)
    assert rc == L.ERR_INVALID and L.last_error()
    assert np.array_equal(after.view(np.uint64), np.ascontiguousarray(poses, np.float64).view(np.uint64))
    assert (w == -3.0).all() and (rep == -3.0).all()
    with pytest.raises(ValueError):
        g = PG.PoseGraph(poses)
        for (s, t), T, lam, u in zip(nodes, Ts, infos, unc):
            g.add_edge(s, t, T, lam, bool(u))
        g.optimize(0.05)


def test_invalid_scalars_and_sizes():
    poses, nodes, Ts, infos, unc = small_graph()
    for kw in (dict(dist=0.0), dict(dist=-1.0), dict(dist=np.nan), dict(dist=INF), dict(pref=0.0), dict(pref=-1.0), dict(pref=np.nan),
               dict(thr=np.nan), dict(thr=INF), dict(max_iters=-1)):
        args = dict(dist=0.05)
        args.update(kw)
        rc, after, w, rep = lib_optimize(poses, nodes, Ts, infos, unc, **args)
        assert rc == L.ERR_INVALID, kw
        assert np.array_equal(after.view(np.uint64), poses.view(np.uint64)) and (rep == -3.0).all()
        g = PG.PoseGraph(poses)
        for (s, t), T, lam, u in zip(nodes, Ts, infos, unc):
            g.add_edge(s, t, T, lam, bool(u))
        with pytest.raises(ValueError):
            g.optimize(args["dist"], **{k: v for k, v in (("preference_loop_closure", args.get("pref")), ("prune_threshold", args.get("thr")),
                                                          ("max_iters", args.get("max_iters"))) if v is not None})
    # 513 nodes are refused, 0 too; NULL arrays
    many = np.tile(np.eye(4), (513, 1, 1))
    chain = [(k + 1, k) for k in range(512)]
    rc, after, _, _ = lib_optimize(many, chain, [np.eye(4)] * 512, [np.eye(6)] * 512, [0] * 512, 0.05)
    assert rc == L.ERR_INVALID and np.array_equal(after, many)
    with pytest.raises(ValueError):
        PG.PoseGraph(many)
    with pytest.raises(ValueError):
        PG.PoseGraph(np.zeros((0, 4, 4)))
    lib = L.load()
    p = poses.copy()
    n32, t64, i64, u8 = np.array(nodes, np.int32), np.array(Ts), np.array(infos), np.array(unc, np.uint8)
    assert lib.r3d_posegraph_optimize(0, p.ctypes.data, 0, None, None, None, None, 0.05, 1.0, 0.25, 10, None, None) == L.ERR_INVALID
    assert lib.r3d_posegraph_optimize(4, None, 4, n32.ctypes.data, t64.ctypes.data, i64.ctypes.data, u8.ctypes.data, 0.05, 1.0, 0.25, 10,
                                      None, None) == L.ERR_INVALID
    for drop in range(4):
        arrays = [n32.ctypes.data, t64.ctypes.data, i64.ctypes.data, u8.ctypes.data]
        arrays[drop] = None
        assert lib.r3d_posegraph_optimize(4, p.ctypes.data, 4, *arrays, 0.05, 1.0, 0.25, 10, None, None) == L.ERR_INVALID
    assert lib.r3d_posegraph_optimize(4, p.ctypes.data, -1, *arrays[:3], u8.ctypes.data, 0.05, 1.0, 0.25, 10, None, None) == L.ERR_INVALID
    assert np.array_equal(p, poses)
    # weights and report are optional; one node alone is a graph; max_iters = 0 evaluates only
    assert lib.r3d_posegraph_optimize(4, p.ctypes.data, 4, n32.ctypes.data, t64.ctypes.data, i64.ctypes.data, u8.ctypes.data, 0.05, 1.0,
                                      0.25, 10, None, None) == 0
    one = np.eye(4)[None].copy()
    assert lib.r3d_posegraph_optimize(1, one.ctypes.data, 0, None, None, None, None, 0.05, 1.0, 0.25, 10, None, None) == 0
    start = perturbed(np.random.default_rng(5), poses, 0.1, 0.1)
    rc, after, w, rep = lib_optimize(start, nodes, Ts, infos, unc, 0.05, pref=INF, max_iters=0)
    assert rc == 0 and np.array_equal(after, start) and rep[2] == 0 and rep[4] == 1 and rep[0] == rep[1] > 0


def test_posegraph_class_checks_its_edges():
    poses, nodes, Ts, infos, unc = small_graph()
    g = PG.PoseGraph(poses)
    for bad in (dict(s=4), dict(s=-1), dict(t=1.0), dict(s=True), dict(t=1), dict(T=np.eye(3)), dict(info=np.eye(5)), dict(uncertain=1)):
        args = dict(s=1, t=0, T=Ts[0], info=infos[0], uncertain=False)
        args.update(bad)
        with pytest.raises(ValueError):
            g.add_edge(**args)
    assert g.edges == []
    with pytest.raises(ValueError):
        g.optimize(0.05)                      # nodes 1..3 hang on nothing
    with pytest.raises(ValueError):
        PG.PoseGraph(np.eye(4))


# ---- 6. a loop closure pulls a drifting chain back --------------------------------------------------------------------------------

def test_loop_closure_pulls_a_drifting_chain_back():
    """Ten nodes on a circle of radius 3 m.  Every odometry edge is off by up to 0.01 rad and 0.02 m, so the chained poses
    drift; one exact uncertain edge joins the last node to the first again.  All L = 1000 I.  Linearised, that edge is one
    measurement of the closure in parallel with a chain of N = 9 equally weighted ones: least squares leaves 1 / (N + 1) = 0.1 of
    the last node's drift.  The bound is 0.2, a factor of two for the terms the linearisation drops and for the lever between
    rotation and translation, which the count of edges ignores.  The loop edge must keep its weight: its chi2 at the start is
    far below what pruning needs."""
    rng = np.random.default_rng(6)
    N = 9
    truth = np.stack([REF.pose((0.0, 2 * math.pi * k / (N + 1), 0.0), (3 * math.cos(2 * math.pi * k / (N + 1)), 0.0,
                                                                     3 * math.sin(2 * math.pi * k / (N + 1)))) for k in range(N + 1)])
    nodes = [(k + 1, k) for k in range(N)] + [(N, 0)]
    Ts = [relative(truth, k + 1, k) @ REF.random_pose(rng, 0.01, 0.02) for k in range(N)] + [relative(truth, N, 0)]
    chain = truth.copy()
    for k in range(N):
        chain[k + 1] = chain[k] @ Ts[k]
    infos, unc = [1000.0 * np.eye(6)] * (N + 1), [0] * N + [1]
    drift = REF.pose_distance(chain[N], truth[N])
    # mu = 1 x 0.5^2 x 1000 = 250 against a chi2 of the loop edge of 1000 |xi|^2 with |xi| a few hundredths
    rc, poses, w, rep = lib_optimize(chain, nodes, Ts, infos, unc, 0.5)
    assert rc == 0, L.last_error()
    left = REF.pose_distance(poses[N], truth[N])
    print("drifting chain: last node %.4f rad %.4f m off, with the loop %.4f rad %.4f m; worst node %.4f m -> %.4f m; loop weight %.4f"
          % (drift + left + (worst(chain, truth)[1], worst(poses, truth)[1], w[N])))
    assert drift[1] > 0.02 and rep[3] == 0 and w[N] > 0.9
    assert left[0] <= 0.2 * drift[0] and left[1] <= 0.2 * drift[1]
    assert worst(poses, truth)[1] < worst(chain, truth)[1]
    want, _, _ = REF.posegraph_optimize(chain, nodes, Ts, infos, unc, 0.5)
    assert np.abs(poses - want).max() <= 1e-9


# ---- 7. the solver under the host sanitizers ---------------------------------------------------------------------------------------

def test_solver_is_clean_under_host_sanitizers(tmp_path):
    """tests/c/posegraph_host_check.cpp + csrc/r3d_posegraph.cpp as one stand-alone program, host code built with
    AddressSanitizer and UndefinedBehaviorSanitizer: it must end with its own OK and without a sanitizer report."""
    import os
    import subprocess
    from helpers import ROOT
    csrc = os.path.join(ROOT, PKG, "csrc")
    exe = str(tmp_path / "posegraph_host_check")
    build = subprocess.run(["/opt/rocm/bin/hipcc", "-O1", "-g", "-std=c++17", "--offload-arch=gfx950", "-ffp-contract=off",
                            "-I" + os.path.join(ROOT, "include"), "-I" + csrc, "-Xarch_host", "-fsanitize=address,undefined",
                            "-Xarch_host", "-fno-sanitize-recover=undefined", "-x", "hip", os.path.join(csrc, "r3d_posegraph.cpp"),
                            os.path.join(ROOT, "tests", "c", "posegraph_host_check.cpp"), "-fsanitize=address,undefined", "-o", exe],
                           capture_output=True, text=True)
    assert build.returncode == 0, build.stderr[-2000:]
    run = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert run.returncode == 0 and "host check OK" in run.stdout, run.stdout[-1000:] + run.stderr[-2000:]
    assert "Sanitizer" not in run.stderr and "runtime error" not in run.stderr, run.stderr[-2000:]
