"""CPU: the host side of the depth consistency filter (include/r3d.h "Depth consistency"; consistency.py) -- the source window, the
fp64 relative pose of the restatement against a plain 4x4 product, every argument error the C calls raise without a device, and a
semantic check of the rule itself on the restatement (tests/consistency_ref.py): it drops injected floaters and keeps clean pixels.
No compute entry point runs here."""
import ctypes as C
import importlib

import numpy as np
import pytest

import consistency_ref as CR
from helpers import PKG, r3d as _r3d


@pytest.fixture(scope="module")
def R():
    return _r3d()


@pytest.fixture(scope="module")
def L():
    return importlib.import_module(PKG + "._lib")


def test_window_sources(R):
    assert R.window_sources(5, 2).tolist() == [[1, 2, -1, -1], [0, 2, 3, -1], [0, 1, 3, 4], [1, 2, 4, -1], [2, 3, -1, -1]]
    assert R.window_sources(4, 1).tolist() == [[1, -1], [0, 2], [1, 3], [2, -1]]
    t = R.window_sources(3, 8)                                   # radius >= F: everybody else, then padding
    assert t.shape == (3, 16) and t.dtype == np.int32
    assert t[:, :2].tolist() == [[1, 2], [0, 2], [0, 1]] and (t[:, 2:] == -1).all()
    one = R.window_sources(1, 3)                                 # F = 1: an all-empty table
    assert one.shape == (1, 6) and (one == -1).all()
    assert R.window_sources(0, 2).shape == (0, 4)
    for bad in (0, 9, -1):
        with pytest.raises(ValueError):
            R.window_sources(4, bad)
    with pytest.raises(ValueError):
        R.window_sources(-1, 2)


def test_python_argument_errors(R):
    d = np.ones((3, 4, 5), np.float32)
    q, t = np.tile([0.0, 0.0, 0.0, 1.0], (3, 1)), np.zeros((3, 3))
    for kw in ({"rel_tol": 0.0}, {"rel_tol": float("nan")}, {"rel_tol": 1e-60}, {"min_consistent": -1}, {"max_violations": 256},
               {"min_consistent": 1.5}, {"radius": 0}, {"radius": 9}, {"sources": [[1], [2]]}, {"sources": [[1], [2], [3]]},
               {"sources": [[1], [1], [0]]}, {"sources": [[1.0], [2.0], [0.0]]}, {"sources": np.zeros((3, 17), np.int32) - 1}):
        with pytest.raises(ValueError):
            R.depth_consistency(d, q, t, **kw)
        with pytest.raises(ValueError):
            R.fuse_frames_consistent(d, q, t, **kw)
    with pytest.raises(ValueError):
        R.depth_consistency(d, q[:2], t[:2])


def test_relative_pose_is_the_4x4_product(R):
    S = importlib.import_module(PKG + ".synthetic")
    rng = np.random.default_rng(5)
    q = rng.normal(size=(6, 4))
    t = rng.normal(size=(6, 3)) * 5
    poses = R.poses_w2c(q, t)
    for r in range(6):
        for s in range(6):
            Tr, Ts = S.pose_matrix(q[r], t[r]), S.pose_matrix(q[s], t[s])
            want = Ts @ np.linalg.inv(Tr)                          # camera r -> world -> camera s
            Rsr, tsr = CR.relative_pose64(poses, r, s)
            assert np.abs(Rsr - want[:3, :3]).max() <= 1e-12 and np.abs(tsr - want[:3, 3]).max() <= 1e-12, (r, s)
            R32, t32 = CR.relative_row(poses, r, s)
            assert R32.dtype == np.float32 and np.array_equal(R32, Rsr.reshape(9).astype(np.float32)) and np.array_equal(t32, tsr.astype(np.float32))
    Rsr, tsr = CR.relative_pose64(poses, 2, 2)
    assert np.abs(Rsr - np.eye(3)).max() <= 1e-12 and np.abs(tsr).max() <= 1e-12


def test_argument_errors_without_gpu(L):
    """Everything r3d_depth_consistency, _host and r3d_compact_rows_by_mask refuse before they need a context, in the header's order."""
    lib = L.load()
    pose = np.tile(np.r_[np.eye(3).reshape(9), np.zeros(3)], (3, 1))
    src = np.array([[1, 2], [0, 2], [0, 1]], np.int32)

    def call(fn, dtype=L.DEPTH_F32, n_frames=3, scale=1.0, h_pose=pose, h_src=src, n_sources=2, rel_tol=0.01, min_c=2, max_v=0):
        rc = fn(None, None, None, dtype, n_frames, scale, None if h_pose is None else h_pose.ctypes.data,
                None if h_src is None else h_src.ctypes.data, n_sources, rel_tol, min_c, max_v, None, None, None)
        return rc, L.last_error()

    for fn in (lib.r3d_depth_consistency, lib.r3d_depth_consistency_host):
        cases = [({"dtype": 3}, "unknown depth dtype 3"), ({"dtype": -1}, "unknown depth dtype"), ({"n_frames": -1}, "n_frames must be >= 0"),
                 ({"n_sources": 0}, "n_sources must be in [1, 16], got 0"), ({"n_sources": 17}, "n_sources must be in [1, 16], got 17"),
                 ({"rel_tol": 0.0}, "rel_tol"), ({"rel_tol": -0.01}, "rel_tol"), ({"rel_tol": float("nan")}, "rel_tol"),
                 ({"rel_tol": float("inf")}, "rel_tol"), ({"rel_tol": 1e39}, "rel_tol"), ({"rel_tol": 1e-60}, "rel_tol"),
                 ({"min_c": -1}, "min_consistent"), ({"min_c": 256}, "min_consistent"), ({"max_v": -1}, "max_violations"),
                 ({"max_v": 256}, "max_violations"), ({"scale": float("nan")}, "depth_scale"), ({"scale": 1e39}, "depth_scale"),
                 ({"h_pose": None}, "NULL pose or source table"), ({"h_src": None}, "NULL pose or source table"),
                 ({"h_src": np.array([[1, 3], [0, 2], [0, 1]], np.int32)}, "source 1 of frame 0 is 3"),
                 ({"h_src": np.array([[1, 2], [0, -2], [0, 1]], np.int32)}, "source 1 of frame 1 is -2"),
                 ({"h_src": np.array([[1, 2], [0, 2], [2, 1]], np.int32)}, "frame 2 lists itself as source 0"),
                 ({}, "ctx is NULL"), ({"n_frames": 0}, "ctx is NULL"),
                 ({"h_src": np.array([[1, -1], [-1, -1], [0, 0]], np.int32)}, "ctx is NULL")]      # a valid table: holes and repeats
        for kw, text in cases:
            rc, msg = call(fn, **kw)
            assert rc == L.ERR_INVALID and text in msg, (kw, rc, msg)
        # the order: the earlier check speaks
        assert "dtype" in call(fn, dtype=7, n_sources=0, rel_tol=0.0)[1]
        assert "n_sources" in call(fn, n_sources=0, rel_tol=0.0, h_src=None)[1]
        assert "rel_tol" in call(fn, rel_tol=0.0, min_c=-1)[1]
        assert "is 3" in call(fn, h_src=np.array([[0, 3], [0, 2], [0, 1]], np.int32))[1]      # range before "lists itself"
    n = C.c_int64(-7)
    for args, text in (((None, None, None, 0, None, None, None, 0, None), "n_out is NULL"),
                       ((None, None, None, -1, None, None, None, 0, C.byref(n)), "bad cloud size"),
                       ((None, None, None, 1 << 32, None, None, None, 0, C.byref(n)), "bad cloud size"),
                       ((None, None, None, 4, None, None, None, -1, C.byref(n)), "cap must be >= 0"),
                       ((None, None, None, 4, None, None, None, 0, C.byref(n)), "ctx is NULL")):
        assert lib.r3d_compact_rows_by_mask(*args) == L.ERR_INVALID and text in L.last_error(), (args, L.last_error())
    assert n.value == -7


# ---- the rule itself: does it do what it is for? ---------------------------------------------------------------------------------
FRAMES, SHAPE, REL_TOL, SHARE = 24, (72, 96), 0.03, 0.01


def test_rule_drops_floaters_and_keeps_clean_pixels(R):
    """24 views turning once inside the box room (15 degrees apart, radius 2: four sources each), 72 x 96.  1 % of the pixels have
    their depth halved (floaters in front of the walls), another 1 % are pushed out by 30 % (points behind the walls).  Measured on
    the restatement with rel_tol 0.03, min_consistent 2, max_violations 0:
        injected floaters that project inside >= 1 source and are dropped      1.0000 of 1489       asserted >= 0.98
        pushed-out pixels that project inside >= 1 source and are dropped      1.0000               asserted >= 0.98
        untouched pixels with >= 2 sources in view that are kept               0.9640 of 138777     asserted >= 0.93
        the same share with no pixel corrupted                                 1.0000               asserted >= 0.99
    What the untouched pixels lose is the price of max_violations = 0: a pushed-out pixel of a SOURCE reads as "sees past the point",
    and four sources with 1 % of such pixels each veto about 4 % of the clean pixels.  The margins sit below the measured values
    by that much and no more, so a rule that no longer rejects floaters, or rejects the scene, fails."""
    S = importlib.import_module(PKG + ".synthetic")
    clean, q, t, K = S.room_views(FRAMES, *SHAPE, seed=3)
    pick = np.random.default_rng(11).random(clean.shape)
    floater, pushed = pick < SHARE, (pick >= SHARE) & (pick < 2 * SHARE)
    depths = clean.copy()
    depths[floater] *= np.float32(0.5)
    depths[pushed] *= np.float32(1.3)
    poses, src = R.poses_w2c(q, t), R.window_sources(FRAMES, 2)
    votes, keep, filtered, seen = CR.depth_consistency(depths, poses, src, K, REL_TOL, 2, 0, with_in_view=True)
    a, b, c = floater & (seen >= 1), pushed & (seen >= 1), ~floater & ~pushed & (seen >= 2)
    dropped_floaters, dropped_pushed, kept_clean = 1.0 - keep[a].mean(), 1.0 - keep[b].mean(), keep[c].mean()
    print("floaters dropped %.4f of %d; pushed-out dropped %.4f of %d; untouched kept %.4f of %d"
          % (dropped_floaters, a.sum(), dropped_pushed, b.sum(), kept_clean, c.sum()))
    assert a.sum() >= 1000 and c.sum() >= 100000
    assert dropped_floaters >= 0.98 and dropped_pushed >= 0.98 and kept_clean >= 0.93
    assert np.array_equal(filtered, np.where(keep.astype(bool), depths, np.float32(0)))
    votes0, keep0, _, seen0 = CR.depth_consistency(clean, poses, src, K, REL_TOL, 2, 0, with_in_view=True)
    print("uncorrupted: kept %.4f of the pixels with >= 2 sources in view, %d violations" % (keep0[seen0 >= 2].mean(), votes0[..., 1].sum()))
    assert keep0[seen0 >= 2].mean() >= 0.99
