"""GPU: the pair sums of a registration (r3d_registration_sums) against the fp64 restatement in tests/posegraph_ref.py, the
information matrix and quality built on them (posegraph.registration_information / evaluate_registration) and multiway
registration end to end (posegraph.register_multiway, other_tools/multiway_registration.py)."""
import ctypes as C
import importlib
import os
import subprocess
import sys

import numpy as np
import pytest

import posegraph_ref as REF
from helpers import PKG, ROOT, r3d as _r3d
from test_gpu_bounds import Guarded

pytestmark = pytest.mark.gpu

N_TGT = 5000
U = 2.0 ** -53


@pytest.fixture(scope="module")
def R():
    return _r3d()


@pytest.fixture(scope="module")
def PG(R):
    return importlib.import_module(PKG + ".posegraph")


@pytest.fixture(scope="module")
def L(R):
    return importlib.import_module(PKG + "._lib")


@pytest.fixture(scope="module")
def ctx(R):
    c = R.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def target():
    rng = np.random.default_rng(0)
    tgt = (rng.uniform(-2.0, 2.0, (N_TGT, 3)) + (0.5, -1.0, 3.0)).astype(np.float32)
    tgt[7], tgt[4001] = np.nan, np.inf                                # rows no query can return: pairs with them are planted
    return tgt


def sums_call(ctx, gs, n_src, gt, n_tgt, gi, gd, max_d2, fill=-3.0):
    out = (C.c_double * 11)(*([fill] * 11))
    rc = ctx.lib.r3d_registration_sums(ctx.handle, gs, n_src, gt, n_tgt, gi, gd, max_d2, out)
    return rc, np.array(out[:])


def check(got, src, tgt, idx, d2, gate):
    want, mag = REF.registration_sums(src, tgt, idx, d2, gate)
    assert got[0] == want[0]
    assert (np.abs(got - want) <= max(want[0], 1.0) * U * mag).all(), (got - want, want[0] * U * mag)
    return want


@pytest.mark.parametrize("n_src", [1, 63, 64, 65, 255, 256, 257, 1000, 70001])
def test_sums_against_the_restatement(R, L, ctx, target, n_src):
    icp = importlib.import_module(PKG + ".icp")
    rng = np.random.default_rng(n_src)
    tgt = target
    rows = rng.integers(8, 4000, n_src)
    src = (tgt[rows].astype(np.float64) + rng.normal(size=(n_src, 3)) * 0.02).astype(np.float32)
    gs, gt = Guarded(ctx, src.nbytes, 4, data=src, seed=1), Guarded(ctx, tgt.nbytes, 4, data=tgt, seed=2)
    gi, gd = Guarded(ctx, n_src * 4, 4, seed=3), Guarded(ctx, n_src * 4, 4, seed=4)
    made = [gs, gt, gi, gd]
    index = icp.NNIndex(ctx, gt.ptr, N_TGT)
    try:
        index.query(gs.ptr, n_src, gi.ptr, gd.ptr)
        idx, d2 = gi.read(np.uint32), gd.read(np.float32)
        assert (idx < N_TGT).all() and np.isfinite(d2).all() and (d2 > 0).all()
        gi_in, gd_in = Guarded(ctx, idx.nbytes, 4, data=idx, seed=13), Guarded(ctx, d2.nbytes, 4, data=d2, seed=14)   # now inputs
        made += [gi_in, gd_in]

        def run(gate, p_src=gs, p_idx=gi_in, p_d2=gd_in):
            rc, got = sums_call(ctx, p_src.ptr, n_src, gt.ptr, N_TGT, p_idx.ptr, p_d2.ptr, gate)
            assert rc == 0, L.last_error()
            for g in (p_src, gt, p_idx, p_d2):
                g.unchanged()
            return got

        # a gate that passes everything, twice: the same bits
        everything = run(np.inf)
        want = check(everything, src, tgt, idx, d2, np.inf)
        assert want[0] == n_src
        assert np.array_equal(everything.view(np.uint64), run(np.inf).view(np.uint64))
        assert np.array_equal(everything.view(np.uint64), run(float(d2.max())).view(np.uint64))
        # one that passes nothing
        assert np.array_equal(run(float(np.nextafter(d2.min(), np.float32(0)))), np.zeros(11))
        assert np.array_equal(run(0.0), np.zeros(11))
        # one set exactly to a pair's d2: that pair is in; the next float below drops it
        edge = np.sort(d2)[n_src // 2]
        at, below = run(float(edge)), run(float(np.nextafter(edge, np.float32(0))))
        check(at, src, tgt, idx, d2, edge)
        check(below, src, tgt, idx, d2, np.nextafter(edge, np.float32(0)))
        assert at[0] == (d2 <= edge).sum() and below[0] == (d2 < edge).sum() and at[0] > below[0]
        # rows that are no points, on either side, and indices past the cloud: left out, nothing read behind the target
        src2, idx2, d22 = src.copy(), idx.copy(), d2.copy()
        picks = rng.permutation(n_src)
        for k, (row, what) in zip(picks, [("src", np.nan), ("src", np.inf), ("idx", 7), ("idx", 4001), ("idx", N_TGT), ("idx", N_TGT + 5),
                                          ("idx", 2 ** 32 - 1), ("d2", np.nan), ("src", -np.inf)]):
            if row == "src":
                src2[k, rng.integers(3)] = what
            elif row == "idx":
                idx2[k] = what
            else:
                d22[k] = what
        gs2, gi2, gd2 = (Guarded(ctx, a.nbytes, 4, data=a, seed=5 + j) for j, a in enumerate((src2, idx2, d22)))
        made += [gs2, gi2, gd2]
        planted = run(np.inf, gs2, gi2, gd2)
        want = check(planted, src2, tgt, idx2, d22, np.inf)
        assert want[0] == n_src - min(n_src, 9) and np.isfinite(planted).all()
    finally:
        index.close()
        for g in made:
            g.free()


def test_sums_empty_source_and_argument_errors(R, L, ctx, target):
    icp = importlib.import_module(PKG + ".icp")
    n_src = 300
    src = target[100:100 + n_src] + np.float32(0.01)
    gs, gt = Guarded(ctx, src.nbytes, 4, data=src, seed=1), Guarded(ctx, target.nbytes, 4, data=target, seed=2)
    gi, gd = Guarded(ctx, n_src * 4, 4, seed=3), Guarded(ctx, n_src * 4, 4, seed=4)
    index = icp.NNIndex(ctx, gt.ptr, N_TGT)
    try:
        index.query(gs.ptr, n_src, gi.ptr, gd.ptr)
        idx, d2 = gi.read(np.uint32), gd.read(np.float32)
        gi.free(), gd.free()
        gi, gd = Guarded(ctx, idx.nbytes, 4, data=idx, seed=13), Guarded(ctx, d2.nbytes, 4, data=d2, seed=14)   # now inputs
        rc, got = sums_call(ctx, gs.ptr, 0, gt.ptr, N_TGT, gi.ptr, gd.ptr, 1.0)
        assert rc == 0 and np.array_equal(got, np.zeros(11))
        rc, got = sums_call(ctx, None, 0, None, 0, None, None, 1.0)
        assert rc == 0 and np.array_equal(got, np.zeros(11))

        def call(c=ctx.handle, s=gs.ptr, ns=n_src, t=gt.ptr, nt=N_TGT, i=gi.ptr, d=gd.ptr, gate=1.0, out=True):
            res = (C.c_double * 11)(*([-3.0] * 11))
            rc = ctx.lib.r3d_registration_sums(c, s, ns, t, nt, i, d, gate, res if out else None)
            return rc, np.array(res[:])

        for kw in [dict(c=None), dict(s=None), dict(t=None), dict(i=None), dict(d=None), dict(out=False), dict(ns=-1), dict(nt=-1),
                   dict(nt=2 ** 32), dict(gate=-1.0), dict(gate=-1e-30), dict(gate=float("nan")), dict(gate=float("-inf"))]:
            rc, res = call(**kw)
            assert rc == L.ERR_INVALID and L.last_error(), kw
            assert (res == -3.0).all(), kw
        rc, res = call()
        assert rc == 0 and res[0] == n_src
        PG = importlib.import_module(PKG + ".posegraph")
        again = PG.registration_sums_device(ctx, gs.ptr, n_src, gt.ptr, N_TGT, gi.ptr, gd.ptr, 1.0)
        assert np.array_equal(again.view(np.uint64), res.view(np.uint64))
        with pytest.raises(ValueError):
            PG.registration_sums_device(ctx, gs.ptr, n_src, gt.ptr, N_TGT, gi.ptr, gd.ptr, -1.0)
        for g in (gs, gt, gi, gd):
            g.unchanged()
    finally:
        index.close()
        for g in (gs, gt, gi, gd):
            g.free()


# ---- information matrix and quality -------------------------------------------------------------------------------------------

def test_information_and_quality_of_an_exact_copy(R, PG, ctx):
    icp = importlib.import_module(PKG + ".icp")
    rng = np.random.default_rng(3)
    n, max_dist = 3000, 0.01
    tgt = rng.uniform(-2.0, 2.0, (n, 3)).astype(np.float32)
    T = REF.random_pose(rng, 1.0, 2.0)
    Ti = REF.inverse(T)
    src = (tgt.astype(np.float64) @ Ti[:3, :3].T + Ti[:3, 3]).astype(np.float32)
    extent = float(np.linalg.norm(tgt.max(0) - tgt.min(0)))
    info, fitness, rmse = PG.registration_information(src, tgt, T, max_dist, ctx=ctx)
    fit2, rmse2, pairs = PG.evaluate_registration(src, tgt, T, max_dist, ctx=ctx)
    print("exact copy: fitness %r, rmse %.3e (extent %.2f)" % (fitness, rmse, extent))
    assert fitness == 1.0 and rmse < 1e-5 * extent and (fit2, rmse2, pairs) == (fitness, rmse, n)
    # every target point is some pair's q exactly once.  Each sum is off by at most n u sum|terms| (as is the restatement's), and
    # sum|terms| of no entry exceeds the largest entry of the matrix
    direct = REF.information_direct(tgt)
    assert np.abs(info - direct).max() <= 4 * n * U * np.abs(direct).max()
    assert np.array_equal(info, info.T) and info[5, 5] == n
    # a ready index in place of the target
    d_tgt = ctx.alloc(tgt.nbytes).upload(tgt)
    index = icp.NNIndex(ctx, d_tgt.ptr, n)
    try:
        info3, fit3, rmse3 = PG.registration_information(src, index, T, max_dist)
        assert np.array_equal(info3, info) and (fit3, rmse3) == (fitness, rmse)
        # half the source moved away by 10 x max_dist
        half = src.copy()
        half[: n // 2] += (T[:3, :3].T @ np.array([10 * max_dist, 0.0, 0.0])).astype(np.float32)
        fit4, rmse4, pairs4 = PG.evaluate_registration(half, index, T, max_dist)
        assert fit4 == 0.5 and pairs4 == n // 2 and rmse4 < 1e-5 * extent
    finally:
        index.close()
        d_tgt.free()
    assert PG.evaluate_registration(np.zeros((0, 3), np.float32), tgt, T, max_dist, ctx=ctx) == (0.0, 0.0, 0)
    for bad in (dict(T=np.eye(3)), dict(max_dist=0.0), dict(max_dist=float("nan")), dict(src=np.zeros((4, 2))),
                dict(tgt=np.zeros((0, 3), np.float32))):
        args = dict(src=src, tgt=tgt, T=T, max_dist=max_dist)
        args.update(bad)
        with pytest.raises(ValueError):
            PG.registration_information(ctx=ctx, **args)


# ---- end to end ---------------------------------------------------------------------------------------------------------------------

VOXEL = 0.1
LOOPS = [(4, 0), (3, 0), (4, 1)]


@pytest.fixture(scope="module")
def views(R, ctx):
    """five views turning once about the room, each as a cloud in its camera frame, and the true pose of every cloud in the
    frame of cloud 0"""
    S = importlib.import_module(PKG + ".synthetic")
    depth, quats, ts, K = S.room_views(5, 60, 80)
    clouds = [R.unproject(d, K, ctx=ctx) for d in depth]
    w2c = [S.pose_matrix(q, t) for q, t in zip(quats, ts)]
    truth = np.stack([w2c[0] @ np.linalg.inv(X) for X in w2c])
    return clouds, truth


def worst_error(clouds, poses, truth):
    worst = 0.0
    for p, X, Xt in zip(clouds, poses, truth):
        p = p.astype(np.float64)
        worst = max(worst, float(np.linalg.norm((p @ X[:3, :3].T + X[:3, 3]) - (p @ Xt[:3, :3].T + Xt[:3, 3]), axis=1).max()))
    return worst


@pytest.fixture(scope="module")
def parts():
    """The cluttered room of tests/register_ref.py cut into four sectors of 210 degrees about the vertical axis, 90 degrees
    apart: neighbours share 120 degrees (0.51 to 0.61 of the source within 0.15 m at the true pose), and so do the last and the
    first.  Part k is given in its own frame: the true pose X_k (part k -> frame of part 0) chains small motions (4 degrees,
    0.1 m per step), which ICP from the identity can follow.  (With sectors of 150 degrees -- 0.37 to 0.51 -- the recipe's coarse
    stage, whose gate of 15 voxels is 1.5 m here, walks one pair into the room's 120-degree look-alike: DESIGN 4.5s.)"""
    import register_ref as RR
    rng = np.random.default_rng(8)
    P = RR.cluttered_room(0)
    az = np.degrees(np.arctan2(P[:, 2], P[:, 0]))
    truth, clouds, centre = [np.eye(4)], [], np.array([0.0, 0.3, 0.0])
    for k in range(1, 4):
        w = rng.normal(size=3)
        truth.append(truth[-1] @ REF.pose(w / np.linalg.norm(w) * np.radians(4.0), rng.uniform(-1.0, 1.0, 3) * 0.1 / np.sqrt(3.0)))
    views_ = []
    for k, X in enumerate(truth):
        inside = np.abs((az - 90.0 * k + 180.0) % 360.0 - 180.0) <= 105.0
        Xi = REF.inverse(X)
        clouds.append((P[inside] @ Xi[:3, :3].T + Xi[:3, 3]).astype(np.float32))
        views_.append(Xi[:3, :3] @ centre + Xi[:3, 3])
    return clouds, np.stack(truth), np.stack(views_)


def test_register_multiway_on_overlapping_parts(R, PG, ctx, parts):
    """Neighbours overlap and the last part sees the first again.  Two bounds on the worst point of any cloud: the recipe's own
    correspondence distance, 1.5 x voxel_size (a pose that leaves a point farther from its true place could not have been
    accepted by the pairs that made it), and, with the loop, 1.25 x the error of the chain alone (the loop edge's own
    registration noise may cost that much; it must not cost more).  A chain without loops has nothing to optimise and is left
    as it is.  The loop candidate must come through (fitness >= min_fitness) and keep its weight.
    Measured: 0.0010 m with and without the loop, loop fitness 0.624, weight 0.999999."""
    clouds, truth, origin = parts
    bound = 1.5 * VOXEL
    chain, g0, info0 = PG.register_multiway(clouds, VOXEL, loop_pairs=None, viewpoints=origin, ctx=ctx)
    assert np.abs(chain - info0["odometry"]).max() <= 1e-9 and len(g0.edges) == 3 and not info0["rejected"]
    err_chain = worst_error(clouds, chain, truth)
    poses, g, info = PG.register_multiway(clouds, VOXEL, loop_pairs=[(3, 0)], viewpoints=origin, ctx=ctx)
    err = worst_error(clouds, poses, truth)
    print("parts: odometry alone worst point %.4f m, with the loop (3, 0) %.4f m (bound %.3f); edges %s; rejected %s; report %s; weights %s"
          % (err_chain, err, bound, [(s, t, u, round(f, 3), round(r, 4)) for s, t, u, f, r in info["edges"]], info["rejected"],
             info["report"], g.edge_weights))
    assert err_chain <= bound and err <= bound
    assert err <= 1.25 * err_chain
    assert np.array_equal(poses[0], np.eye(4)) and poses.shape == (4, 4, 4)
    assert np.abs(info["odometry"] - info0["odometry"]).max() <= 1e-9
    assert not info["rejected"] and len(g.edges) == 4 and g.edges[3][:2] == (3, 0) and g.edges[3][4]
    assert not g.pruned.any() and g.edge_weights[3] > 0.25 and np.array_equal(g.edge_weights[:3], np.ones(3))
    assert all(f >= 0.3 for _, _, _, f, _ in info["edges"])


def test_register_multiway_raises_where_neighbours_share_nothing(PG, ctx, views):
    """synthetic.room_views(5, 60, 80) turns by 72 degrees per view with a horizontal field of view of 63 degrees.  Share of
    cloud s within 0.15 m of cloud t AT THE TRUE POSES (brute force on the host): (1, 0) 0.255, (2, 1) 0.000, (3, 2) 0.175,
    (4, 3) 0.000; view 0 is one wall and slivers of floor and ceiling (4093 + 709 of 4800 points), so nothing holds a slide along
    that wall.  No method registers this sequence, and register_multiway says so: the point-to-plane step of a consecutive pair
    is undefined and the call raises, naming the pair and the stage, with or without loop candidates."""
    clouds, _ = views
    origin = np.zeros((5, 3))
    for loops in (None, LOOPS):
        with pytest.raises(ValueError, match=r"clouds \d and \d cannot be registered \((coarse|fine) stage"):
            PG.register_multiway(clouds, VOXEL, loop_pairs=loops, viewpoints=origin, ctx=ctx)


def test_command_line_tool(R, tmp_path, parts, views):
    clouds, truth, _ = parts
    tool = os.path.join(ROOT, PKG, "other_tools", "multiway_registration.py")

    def run(cloud_list, name, *more):
        paths = []
        for k, c in enumerate(cloud_list):
            paths.append(str(tmp_path / ("%s_%d.ply" % (name, k))))
            R.cloud_io.write_ply_binary(paths[-1], c)
        return subprocess.run([sys.executable, tool] + paths + list(more), capture_output=True, text=True, timeout=300)

    out = tmp_path / "out"
    r = run(clouds, "part", "--voxel-size", str(VOXEL), "--out-dir", str(out))
    assert r.returncode == 0, r.stderr[-2000:]
    print(r.stdout.strip())
    got = np.stack([R.get_T(str(out / ("T_%d.txt" % k))) for k in range(4)])
    assert np.array_equal(got[0], np.eye(4)) and np.array_equal(got[:, 3], np.tile([0.0, 0.0, 0.0, 1.0], (4, 1)))
    err = worst_error(clouds, got, truth)
    print("command line, every pair two or more apart a loop candidate: worst point %.4f m" % err)
    assert err <= 1.5 * VOXEL
    assert R.cloud_io.read_ply(str(out / "merged.ply")).shape == (sum(c.shape[0] for c in clouds), 3)
    # a chain that does not hold: a message, exit status 1, nothing written
    none = tmp_path / "none"
    r = run(views[0], "view", "--voxel-size", str(VOXEL), "--out-dir", str(none))
    assert r.returncode == 1 and "cannot be registered" in r.stderr and not none.exists()
    assert run(clouds, "part", "--voxel-size", "0").returncode == 2
