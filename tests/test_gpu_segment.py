"""GPU: RANSAC plane segmentation (r3d_segment_plane; segmentation.py; other_tools/segment_planes.py) against the NumPy
restatement of include/r3d.h in tests/segment_ref.py.

  1. the H counts, the best hypothesis, its count and rows and the valid count: bit for bit;
  2. the final mask and its count: bit for bit against |t| <= thr recomputed from the RETURNED plane and centroid;
  3. the refined plane against a refit of the same inliers in np.longdouble + eigh: sin(angle) <= m 2^-50 (tr C + |c - a|^2) /
     (l1 - l0) (the fp64 summation bound, m 2^-53 per sum, x 8 for the anchor-centred sums and the centring, through Davis-Kahan)
     and the centroid within m 2^-50 (|c - a| + sqrt(tr C)); cases with l1 - l0 < 1e-6 l2 are left out of 3, and none of the six
     clouds may be such a case.  The bound has no term for the rounding of the returned centroid itself (half an ulp of |c|), so
     the cloud offset by 1e4 is sized for m 2^-50 (...) to exceed ulp(1e4).
Every check prints the fraction of its bound it used (run with -s)."""
import ctypes as C
import importlib
import os
import subprocess
import sys

import numpy as np
import pytest

import segment_ref as REF
from helpers import PKG, ROOT, r3d as _r3d
from test_gpu_bounds import Guarded
from test_segment_host import check_room

pytestmark = pytest.mark.gpu

SEEDS = [0, 2**64 - 1]


@pytest.fixture(scope="module")
def R():
    return _r3d()


@pytest.fixture(scope="module")
def S(R):
    return importlib.import_module(PKG + ".segmentation")


@pytest.fixture(scope="module")
def L(R):
    return importlib.import_module(PKG + "._lib")


@pytest.fixture(scope="module")
def ctx(R):
    c = R.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def room(R):
    syn = importlib.import_module(PKG + ".synthetic")
    depth, q, t, K = syn.room_views(6, 120, 160, seed=0)
    xyz = R.fuse_frames(depth, q, t, intrinsics=K)
    xyz = xyz[np.isfinite(xyz).all(axis=1)]
    assert xyz.shape == (115200, 3)
    return xyz


# name -> (cloud, thr, H); H n <= 5e7
def _clouds(room):
    return {"cube5k": (REF.cube(5000, 1), 0.02, 1000),
            "room": (room, 0.01, 256),
            "lattice": (REF.lattice_plane(), 0.01, 64),
            "nonfinite": (REF.nonfinite(), 0.01, 512),
            "offset1e4": (REF.cube(20_000, 3) + np.float32(1e4), 0.1, 256),
            "hot": (REF.hot(), 0.01, 257)}


CLOUDS = ["cube5k", "room", "lattice", "nonfinite", "offset1e4", "hot"]
_REF = {}


def reference(key, xyz, thr, H, seed):
    if key not in _REF:
        _REF[key] = REF.segment_plane(xyz, thr, H, seed)
    return _REF[key]


def device_run(S, ctx, xyz, thr, H, seed, want_counts=True):
    """(DevicePlane, mask bool [n], counts uint32 [H] or None) through Guarded output buffers."""
    n = xyz.shape[0]
    d_xyz = ctx.alloc(max(xyz.nbytes, 16)).upload(np.ascontiguousarray(xyz, np.float32))
    gm = Guarded(ctx, n, 3, seed=21)
    gc = Guarded(ctx, H * 4, 4, seed=22) if want_counts else None
    try:
        p = S.segment_plane_device(ctx, d_xyz.ptr, n, thr, H, seed, gm.ptr, gc.ptr if gc else None)
        mask = gm.read(np.uint8)
        assert set(np.unique(mask)) <= {0, 1}
        return p, mask.astype(bool), gc.read(np.uint32) if gc else None
    finally:
        d_xyz.free()
        gm.free()
        if gc:
            gc.free()


WORST = {"sin": 0.0, "centroid": 0.0}


def check_all(S, ctx, xyz, thr, H, seed, key=None, need_gap=False):
    want = reference(key or (xyz.tobytes(), thr, H, seed), xyz, thr, H, seed)
    p, mask, counts = device_run(S, ctx, xyz, thr, H, seed)
    # 1: bit for bit
    bad = np.flatnonzero(counts != want.counts)
    assert bad.size == 0, "%d of %d counts differ, first h = %d: got %d want %d" % (bad.size, H, bad[0], counts[bad[0]],
                                                                                 want.counts[bad[0]])
    assert (p.best_hypothesis, p.best_count, p.n_valid) == (want.best_h, want.c_best, want.n_valid)
    assert p.best_rows.tolist() == list(want.rows)
    if want.c_best < 3:
        assert p.n_inliers == 0 and not mask.any() and np.isnan(p.plane).all() and np.isnan(p.centroid).all()
        return p, mask, want
    # 2: the mask from the returned plane and centroid
    again = REF.final_mask(xyz, p.plane[:3], p.centroid, thr)
    assert np.array_equal(mask, again), np.flatnonzero(mask != again)[:5]
    assert p.n_inliers == int(again.sum())
    nrm = p.plane[:3]
    assert abs(np.linalg.norm(nrm) - 1.0) <= 1e-15
    k = int(np.argmax(np.abs(nrm)))
    assert nrm[k] > 0
    assert p.plane[3] == -((nrm[0] * p.centroid[0] + nrm[1] * p.centroid[1]) + nrm[2] * p.centroid[2])
    # 3: the refit
    c_ref, n_ref, sin_bound, c_bound, gap_ok = REF.refit_bounds(xyz, want.I0, want.anchor)
    assert gap_ok or not need_gap, "l1 - l0 < 1e-6 l2 on a cloud that must not be such a case"
    if gap_ok:
        sin_angle = float(np.linalg.norm(np.cross(nrm, n_ref)))
        c_err = float(np.sqrt(((p.centroid.astype(np.longdouble) - c_ref) ** 2).sum()))
        fs, fc = sin_angle / sin_bound, (c_err / c_bound if c_bound > 0 else 0.0 if c_err == 0 else np.inf)
        print("refit m=%d sin %.3e of bound %.3e (%.4f); centroid %.3e of bound %.3e (%.4f)"
              % (want.c_best, sin_angle, sin_bound, fs, c_err, c_bound, fc))
        WORST["sin"], WORST["centroid"] = max(WORST["sin"], fs), max(WORST["centroid"], fc)
        print("worst so far: sin %.4f centroid %.4f of the bound" % (WORST["sin"], WORST["centroid"]))
        assert sin_angle <= sin_bound and c_err <= c_bound
        lam = np.sort(p.eigenvalues)
        assert np.array_equal(lam, p.eigenvalues)
    return p, mask, want


@pytest.mark.parametrize("seed", SEEDS)
@pytest.mark.parametrize("name", CLOUDS)
def test_clouds_counts_mask_and_refit(S, ctx, room, name, seed):
    xyz, thr, H = _clouds(room)[name]
    p, mask, want = check_all(S, ctx, xyz, thr, H, seed, key=(name, seed), need_gap=True)
    assert want.c_best >= 3
    if name == "lattice":                                   # the exact plane comes back exactly
        assert p.plane.tolist() == [0.0, 0.0, 1.0, -0.5] and p.centroid[2] == 0.5 and p.eigenvalues[0] == 0.0
        assert np.array_equal(mask, xyz[:, 2] == np.float32(0.5))
    if name == "nonfinite":
        assert not mask[~np.isfinite(xyz).all(axis=1)].any()
    if name == "hot":
        assert want.n_valid < H // 2


@pytest.mark.parametrize("n", [3, 4, 63, 64, 65, 255, 256, 257, 1023, 1025, 4097])
def test_cloud_sizes(S, ctx, n):
    xyz = REF.cube(n, 100 + n)
    xyz[:, 2] *= np.float32(0.1)
    for seed in SEEDS:
        check_all(S, ctx, xyz, 0.02, 64, seed)


@pytest.mark.parametrize("H", [1, 2, 63, 64, 65, 255, 256, 257, 511, 512, 513, 1000, 1023, 1024, 1025, 4096])
def test_hypothesis_counts(S, ctx, H):
    """1025 points: three tiles, the last with one point; H crosses the thresholds between the kernels with one, two and four
    hypotheses per lane (512, 1024)."""
    xyz = REF.cube(1025, 7)
    xyz[:, 1] *= np.float32(0.1)
    for seed in SEEDS:
        check_all(S, ctx, xyz, 0.02, H, seed)


def test_many_chunks_and_hypothesis_blocks(S, ctx):
    """12 001 points under 4096 hypotheses: four hypothesis blocks, six chunks of four tiles, a 225-point tail tile."""
    xyz = REF.cube(12_001, 9)
    xyz[:, 0] *= np.float32(0.05)
    check_all(S, ctx, xyz, 0.01, 4096, 5)


def test_room_scene(S, room):
    syn = importlib.import_module(PKG + ".synthetic")
    for seed in range(5):
        planes, labels, counts = S.segment_planes(room, 0.01, 256, max_planes=6, seed=seed)
        check_room(planes, labels, counts, syn.ROOM_LO, syn.ROOM_HI)
        faces = REF.room_faces(planes, syn.ROOM_LO, syn.ROOM_HI)
        print("seed %d: worst 1 - |n_axis| %.2e, worst offset %.2e, unlabelled %d"
              % (seed, max(f[2] for f in faces), max(f[3] for f in faces), int((labels < 0).sum())))


def test_noisy_scene(S, ctx):
    xyz, normal = REF.noisy_plane()
    p, mask, want = check_all(S, ctx, xyz, 0.01, 512, 0, need_gap=True)
    sin_angle = np.linalg.norm(np.cross(p.plane[:3], normal))
    assert sin_angle <= np.sin(np.radians(0.5))


def test_no_plane_and_three_points(S, ctx):
    line = np.outer(np.arange(50, dtype=np.float32), np.float32([1, 2, -1]))
    p, mask, want = check_all(S, ctx, line, 0.01, 128, 0)
    assert p.n_inliers == 0 and p.n_valid == 0 and p.best_count == 0 and p.best_hypothesis == 0
    assert np.isnan(p.plane).all() and np.isnan(p.eigenvalues).all() and not mask.any()
    seg = S.segment_plane(line, 0.01, 128, 0, ctx=ctx)
    assert seg.rows.size == 0 and np.isnan(seg.plane).all()
    tri = np.float32([[0, 0, 0], [1, 0, 0], [0, 1, 0]])
    p, mask, want = check_all(S, ctx, tri, 0.01, 64, 0)
    assert p.n_inliers == 3 and mask.all() and p.best_count == 3 and p.plane.tolist() == [0.0, 0.0, 1.0, 0.0]
    seg = S.segment_plane(tri, 0.01, 64, 0, ctx=ctx)
    assert seg.rows.tolist() == [0, 1, 2] and seg.best_count == 3


def test_invariance_guards_and_invalid_calls(S, L, ctx):
    xyz, thr, H, seed = REF.cube(3 * 1024 + 17, 21), 0.02, 300, 3
    xyz[7] = np.nan
    n = xyz.shape[0]
    first = device_run(S, ctx, xyz, thr, H, seed)
    second = device_run(S, ctx, xyz, thr, H, seed)
    for a, b in zip(first[0], second[0]):
        assert np.array_equal(np.asarray(a, np.float64).view(np.uint64), np.asarray(b, np.float64).view(np.uint64))
    assert np.array_equal(first[1], second[1]) and np.array_equal(first[2], second[2])
    # no counts wanted: the same plane and mask
    third = device_run(S, ctx, xyz, thr, H, seed, want_counts=False)
    assert third[2] is None and np.array_equal(third[1], first[1])
    assert np.array_equal(third[0].plane.view(np.uint64), first[0].plane.view(np.uint64)) and third[0].n_inliers == first[0].n_inliers
    # invalid calls write nothing
    lib = ctx.lib
    d_xyz = ctx.alloc(n * 12).upload(xyz)
    gm, gc = Guarded(ctx, n, 3, seed=31), Guarded(ctx, H * 4, 4, seed=32)
    res, m = (C.c_double * 16)(*([-3.0] * 16)), C.c_int64(-5)

    def call(ctx_h=ctx.handle, xyz_p=d_xyz.ptr, n_=n, thr_=thr, H_=H, mask_p=gm.ptr, counts_p=gc.ptr, res_=res, m_=C.byref(m)):
        return lib.r3d_segment_plane(ctx_h, xyz_p, n_, thr_, H_, seed, mask_p, counts_p, res_, m_)

    bad_calls = [dict(ctx_h=None), dict(xyz_p=None), dict(mask_p=None), dict(res_=None), dict(m_=None), dict(n_=2), dict(n_=0),
                 dict(n_=-1), dict(n_=2**32), dict(H_=0), dict(H_=-1), dict(H_=65537), dict(thr_=0.0), dict(thr_=-0.01),
                 dict(thr_=float("nan")), dict(thr_=float("inf")), dict(mask_p=d_xyz.ptr + 12), dict(counts_p=gm.ptr)]
    for kw in bad_calls:
        assert call(**kw) == L.ERR_INVALID, kw
        gm.unchanged()
        gc.unchanged()
        assert m.value == -5 and all(v == -3.0 for v in res), kw
    assert call() == 0, L.last_error()
    assert m.value == first[0].n_inliers and np.array_equal(gm.read(np.uint8).astype(bool), first[1])
    assert np.array_equal(gc.read(np.uint32), first[2])
    for b in (d_xyz, gm, gc):
        b.free()


def test_segment_planes_labels_partition_the_rows(S, ctx):
    rng = np.random.default_rng(5)
    floor = np.concatenate([rng.random((3000, 2)) * 2, rng.normal(0, 0.001, (3000, 1))], axis=1)
    wall = np.concatenate([rng.normal(0, 0.001, (1500, 1)), rng.random((1500, 2)) * 2], axis=1)
    clutter = rng.random((400, 3)) * 2
    xyz = np.concatenate([floor, wall, clutter]).astype(np.float32)
    xyz = xyz[rng.permutation(xyz.shape[0])]
    planes, labels, counts = S.segment_planes(xyz, 0.01, 256, max_planes=4, min_inliers=500, seed=1, ctx=ctx)
    want = REF.segment_planes(xyz, 0.01, 256, 4, 500, 1)
    assert planes.shape == (2, 4) == want[0].shape and np.array_equal(labels, want[1]) and np.array_equal(counts, want[2])
    assert np.abs(planes - want[0]).max() <= 1e-9
    assert labels.min() == -1 and labels.max() == 1
    for k in range(2):
        assert (labels == k).sum() == counts[k]
        rows = np.flatnonzero(labels == k)
        a, b, c, d = planes[k]
        assert np.abs(xyz[rows].astype(np.float64) @ [a, b, c] + d).max() <= 0.01 + 1e-12
    assert (labels < 0).sum() == xyz.shape[0] - counts.sum()
    assert abs(planes[0][2]) > 0.999 and abs(planes[1][0]) > 0.999
    one = S.segment_plane(xyz, 0.01, 256, 1, ctx=ctx)
    assert np.array_equal(one.rows, np.flatnonzero(labels == 0)) and np.array_equal(one.plane, planes[0])
    none = S.segment_planes(xyz, 0.01, 256, max_planes=4, min_inliers=10_000, seed=1, ctx=ctx)
    assert none[0].shape == (0, 4) and (none[1] == -1).all() and none[2].size == 0


def test_command_line_tool(R, tmp_path):
    rng = np.random.default_rng(8)
    floor = np.concatenate([rng.random((2000, 2)) * 2 + 0.5, np.zeros((2000, 1))], axis=1)      # no point of one plane is on the other
    wall = np.concatenate([np.zeros((1000, 1)), rng.random((1000, 2)) * 2 + 0.5], axis=1)
    xyz = np.concatenate([floor, wall, rng.random((50, 3)) * 2 + 0.5]).astype(np.float32)
    src, out = str(tmp_path / "in.ply"), str(tmp_path / "out.ply")
    R.cloud_io.write_ply_binary(src, xyz)
    tool = os.path.join(ROOT, PKG, "other_tools", "segment_planes.py")
    r = subprocess.run([sys.executable, tool, src, out, "--threshold", "0.01", "--hypotheses", "128", "--max-planes", "3", "--min-inliers",
                        "500", "--seed", "2"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [ln.split() for ln in r.stdout.strip().splitlines()]
    assert len(lines) == 2 and all(len(ln) == 5 for ln in lines), r.stdout
    assert sorted(int(ln[4]) for ln in lines) == [1000, 2000]
    assert R.cloud_io.read_ply(out).shape == (xyz.shape[0], 3)
    bad = subprocess.run([sys.executable, tool, src, out, "--threshold", "0"], capture_output=True, text=True, timeout=300)
    assert bad.returncode == 2
