"""GPU: RANSAC over correspondences (r3d_register_ransac; registration.py) against the NumPy restatement of include/r3d.h in
tests/register_ref.py, and the whole recipe (registration.register_global, other_tools/global_registration.py) end to end.

  1. the H counts, the best hypothesis, its count and pairs, the valid count, the final mask and its count: bit for bit;
  2. T against the restatement's T: |dT| <= 1e-9 entrywise (the restatement adds the refit's sums in the device's order; what is
     left is the SVD -- numpy.linalg.svd there, one-sided Jacobi here);
  3. end to end: a cluttered room seen in two overlapping parts, one part moved by 130 degrees and 6 m."""
import ctypes as C
import importlib
import os
import subprocess
import sys

import numpy as np
import pytest

import register_ref as REF
from helpers import PKG, ROOT, r3d as _r3d
from test_gpu_bounds import Guarded

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def R():
    return _r3d()


@pytest.fixture(scope="module")
def G(R):
    return importlib.import_module(PKG + ".registration")


@pytest.fixture(scope="module")
def L(R):
    return importlib.import_module(PKG + "._lib")


@pytest.fixture(scope="module")
def ctx(R):
    c = R.Context(0)
    yield c
    c.close()


def device_run(G, ctx, src, tgt, corr, thr, H, seed, want_counts=True):
    """(result block, mask bool [m], counts or None) through Guarded buffers."""
    m = corr.shape[0]
    gs = Guarded(ctx, src.nbytes, 4, data=src, seed=1)
    gt = Guarded(ctx, tgt.nbytes, 4, data=tgt, seed=2)
    gk = Guarded(ctx, corr.nbytes, 4, data=corr, seed=3)
    gm = Guarded(ctx, m, 3, seed=4)
    gc = Guarded(ctx, H * 4, 4, seed=5) if want_counts else None
    try:
        r = G.registration_ransac_device(ctx, gs.ptr, src.shape[0], gt.ptr, tgt.shape[0], gk.ptr, m, thr, H, seed, gm.ptr,
                                         gc.ptr if gc else None)
        mask = gm.read(np.uint8)
        assert set(np.unique(mask)) <= {0, 1}
        for g in (gs, gt, gk):
            g.unchanged()
        return r, mask.astype(bool), gc.read(np.uint32) if gc else None
    finally:
        for g in (gs, gt, gk, gm, gc):
            if g is not None:
                g.free()


def check_all(G, ctx, src, tgt, corr, thr, H, seed):
    want = REF.ransac(src, tgt, corr, thr, H, seed)
    r, mask, counts = device_run(G, ctx, src, tgt, corr, thr, H, seed)
    bad = np.flatnonzero(counts != want.counts)
    assert bad.size == 0, "%d of %d counts differ, first h = %d: got %d want %d" % (bad.size, H, bad[0], counts[bad[0]], want.counts[bad[0]])
    assert (int(r[16]), int(r[17]), int(r[21])) == (want.best_h, want.c_best, want.n_valid)
    assert r[18:21].astype(np.int64).tolist() == list(want.rows)
    assert not r[25:].any()
    T = r[:16].reshape(4, 4)
    if want.c_best < 3:
        assert np.isnan(T).all() and not mask.any() and r[22] == 0 and np.isnan(r[23])
        return r, mask, want
    assert T[3].tolist() == [0.0, 0.0, 0.0, 1.0]
    err = np.abs(T - want.T).max()
    print("m=%d H=%d seed=%d: c_best %d, |dT| %.3e" % (corr.shape[0], H, seed, want.c_best, err))
    assert err <= 1e-9
    assert bool(r[24]) == want.degenerate
    # the mask follows from the RETURNED pose exactly; equal to the restatement's whenever the two poses round to the same f32
    p, q = REF.gather_pairs(src, tgt, corr)
    again, n_in, rms = REF.final_mask(p, q, T, thr)
    assert np.array_equal(mask, again) and int(r[22]) == n_in
    assert abs(r[23] - rms) <= 1e-12 * max(rms, 1.0)
    if np.array_equal(T[:3].astype(np.float32), want.T[:3].astype(np.float32)):
        assert np.array_equal(mask, want.mask)
    return r, mask, want


@pytest.mark.parametrize("seed", [0, 7, 2 ** 64 - 1])
@pytest.mark.parametrize("H", [1, 1024, 65536])
@pytest.mark.parametrize("m", [3, 4, 1000])
@pytest.mark.parametrize("kind", ["clean", "outliers", "collinear", "repeated"])
def test_against_the_restatement(G, ctx, kind, m, H, seed):
    src, tgt, corr, T_true = REF.correspondences(kind, m, 11)
    r, mask, want = check_all(G, ctx, src, tgt, corr, 0.01, H, seed)
    if kind == "collinear":
        assert want.n_valid == 0 and want.c_best == 0
    if kind == "clean" and H >= 1024:
        assert want.c_best == m and mask.all() and np.abs(r[:16].reshape(4, 4) - T_true).max() <= 1e-5
    if kind == "outliers" and m == 1000 and H >= 1024:
        assert want.c_best >= 250 and np.abs(r[:16].reshape(4, 4) - T_true).max() <= 1e-5


@pytest.mark.parametrize("H", [255, 256, 257, 511, 512, 513, 1023, 1025])
def test_hypothesis_kernel_thresholds(G, ctx, H):
    """1025 pairs: five tiles, the last with one pair; H crosses the thresholds between one, two and four hypotheses per lane."""
    src, tgt, corr, _ = REF.correspondences("outliers", 1025, 3)
    check_all(G, ctx, src, tgt, corr, 0.02, H, 1)


def test_many_chunks_rows_out_of_range_and_nan_points(G, ctx):
    src, tgt, corr, _ = REF.correspondences("outliers", 20_001, 5)
    corr[::1000, 0] = 2 ** 32 - 1
    corr[1::1000, 1] = 20_001
    src[17] = np.nan
    tgt[23, 1] = np.inf
    r, mask, want = check_all(G, ctx, src, tgt, corr, 0.02, 4096, 2)
    assert want.c_best > 5000 and not mask[::1000].any() and not mask[1::1000].any() and not mask[17] and not mask[23]


def test_repeatable_and_invalid_calls(G, L, ctx):
    src, tgt, corr, _ = REF.correspondences("outliers", 3000, 9)
    a, b = device_run(G, ctx, src, tgt, corr, 0.01, 700, 4), device_run(G, ctx, src, tgt, corr, 0.01, 700, 4, want_counts=False)
    assert np.array_equal(a[0].view(np.uint64), b[0].view(np.uint64)) and np.array_equal(a[1], b[1]) and b[2] is None
    host = G.registration_ransac(src, tgt, corr, 0.01, 700, 4, want_counts=True, ctx=ctx)
    assert np.array_equal(host.T.view(np.uint64).reshape(-1), a[0][:16].view(np.uint64)) and np.array_equal(host.inliers, a[1])
    assert np.array_equal(host.counts, a[2]) and host.n_inliers == int(a[1].sum())
    m, H = 3000, 700
    gs, gt = Guarded(ctx, src.nbytes, 4, data=src, seed=1), Guarded(ctx, tgt.nbytes, 4, data=tgt, seed=2)
    gk, gm, gc = Guarded(ctx, corr.nbytes, 4, data=corr, seed=3), Guarded(ctx, m, 3, seed=4), Guarded(ctx, H * 4, 4, seed=5)
    res = (C.c_double * 32)(*([-3.0] * 32))
    lib = ctx.lib

    def call(c=ctx.handle, s=gs.ptr, ns=3000, t=gt.ptr, nt=3000, k=gk.ptr, m_=m, thr=0.01, H_=H, mask=gm.ptr, cnt=gc.ptr, res_=res):
        return lib.r3d_register_ransac(c, s, ns, t, nt, k, m_, thr, H_, 4, mask, cnt, res_)

    for kw in [dict(c=None), dict(s=None), dict(t=None), dict(k=None), dict(mask=None), dict(res_=None), dict(ns=0), dict(nt=0),
               dict(ns=2 ** 32), dict(m_=2), dict(m_=0), dict(m_=-1), dict(m_=2 ** 32), dict(H_=0), dict(H_=65537), dict(thr=0.0),
               dict(thr=-1.0), dict(thr=float("nan")), dict(thr=float("inf")), dict(mask=gs.ptr + 12), dict(mask=gk.ptr), dict(cnt=gt.ptr),
               dict(cnt=gm.ptr)]:
        assert call(**kw) == L.ERR_INVALID, kw
        for g in (gs, gt, gk, gm, gc):
            g.unchanged()
        assert all(v == -3.0 for v in res), kw
    assert call() == 0, L.last_error()
    assert np.array_equal(np.array(res[:]).view(np.uint64), a[0].view(np.uint64))
    for g in (gs, gt, gk, gm, gc):
        g.free()


# ---- end to end -------------------------------------------------------------------------------------------------------------------

VOXEL = 0.1
BOUND = 1.5 * VOXEL          # the recipe's distance_threshold


@pytest.fixture(scope="module")
def pair():
    """The scene and the condition on it: the restatement on its own (4096 hypotheses, seed 0) maps every source point to
    within the distance threshold of its true position."""
    s = REF.room_pair(0)
    T, down, corr, r = REF.recipe(s["src"], s["tgt"], VOXEL, s["src_view"], s["tgt_view"], 4096, 0)
    assert 8000 <= down.shape[0] <= 16000
    err = worst_error(s, T)
    print("restatement: %d correspondences, %d inliers, worst point %.4f of %.4f" % (corr.shape[0], r.n_inliers, err, BOUND))
    assert err <= BOUND
    return s


def worst_error(s, T):
    p = s["src"].astype(np.float64)
    return float(np.linalg.norm((p @ T[:3, :3].T + T[:3, 3]) - (p @ s["T"][:3, :3].T + s["T"][:3, 3]), axis=1).max())


def test_register_global_recovers_what_identity_icp_does_not(R, G, ctx, pair):
    s = pair
    angle = np.degrees(np.arccos((np.trace(s["T"][:3, :3]) - 1) / 2))
    assert angle >= 90 and np.linalg.norm(s["T"][:3, 3]) >= 3
    T, info = G.register_global(s["src"], s["tgt"], VOXEL, src_viewpoint=s["src_view"], tgt_viewpoint=s["tgt_view"], ctx=ctx)
    err = worst_error(s, T)
    print("register_global: %d correspondences, %d inliers, worst point %.4f of %.4f"
          % (info["correspondences"].shape[0], info["ransac"].n_inliers, err, BOUND))
    assert err <= BOUND
    T2, info2 = G.register_global(s["src"], s["tgt"], VOXEL, src_viewpoint=s["src_view"], tgt_viewpoint=s["tgt_view"], refine=True, ctx=ctx)
    err2 = worst_error(s, T2)
    print("with refine: worst point %.4f" % err2)
    assert err2 <= BOUND and "icp" in info2
    # the capability is new: point-to-plane ICP from the identity does not get there
    icp = importlib.import_module(PKG + ".icp")
    try:
        Ti, _ = icp.icp_point_to_plane(info["source_down"], info["target_down"],
                                       tgt_normals=importlib.import_module(PKG + ".normals").estimate_normals(
                                           info["target_down"], 32, viewpoint=s["tgt_view"], ctx=ctx).normals, ctx=ctx)
        err_icp = worst_error(s, Ti)
    except ValueError:
        err_icp = float("inf")
    print("identity-initialised ICP: worst point %.4f" % err_icp)
    assert err_icp > BOUND


def test_command_line_tool(R, tmp_path, pair):
    s = pair
    rng = np.random.default_rng(1)
    src, tgt = s["src"][rng.random(s["src"].shape[0]) < 0.5], s["tgt"][rng.random(s["tgt"].shape[0]) < 0.5]
    a, b, out_T, out_ply = (str(tmp_path / n) for n in ("src.ply", "tgt.ply", "T_data.txt", "moved.ply"))
    R.cloud_io.write_ply_binary(a, src)
    R.cloud_io.write_ply_binary(b, tgt)
    tool = os.path.join(ROOT, PKG, "other_tools", "global_registration.py")
    view = lambda v: ["%r" % float(c) for c in v]
    r = subprocess.run([sys.executable, tool, a, b, "--voxel", "0.1", "--out-T", out_T, "--out-ply", out_ply, "--rounds", "2",
                        "--source-viewpoint"] + view(s["src_view"]) + ["--target-viewpoint"] + view(s["tgt_view"]),
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    T = R.get_T(out_T)
    assert worst_error(s, T) <= BOUND
    moved = R.cloud_io.read_ply(out_ply)
    want = src.astype(np.float64) @ T[:3, :3].T + T[:3, 3]
    assert moved.shape == src.shape and np.abs(moved - want).max() <= 1e-4
    bad = subprocess.run([sys.executable, tool, a, b, "--voxel", "0"], capture_output=True, text=True, timeout=300)
    assert bad.returncode == 2
