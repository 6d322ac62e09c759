"""CPU: the RANSAC plane segmentation's sampler (r3d_ransac_rows, no GPU needed) against its known answers and the NumPy
reference of tests/segment_ref.py; the Python layer's argument checks; and the reference itself on closed forms and on the two
scenes whose conditions tests/test_gpu_segment.py asserts of the device -- asserted here first, so the GPU test never asks of the
library what the specification alone cannot meet."""
import ctypes as C
import importlib

import numpy as np
import pytest

import segment_ref as REF
from helpers import PKG

KATS = [(0, 0, 115200, (101757, 49712, 3045)),
        (0, 1, 115200, (111845, 12251, 37707)),
        (1234, 1023, 3, (1, 0, 0)),
        (2**64 - 1, 65535, 4294967295, (1849050423, 1676756274, 503342300))]


@pytest.fixture(scope="module")
def L():
    return importlib.import_module(PKG + "._lib")


@pytest.fixture(scope="module")
def S():
    return importlib.import_module(PKG + ".segmentation")


def fused_room(seed=0):
    """synthetic.room_views(6, 120, 160) fused by the fp64 oracle and rounded to f32: the GPU test's 115 200-point room."""
    from oracle import fusion_ref
    syn = importlib.import_module(PKG + ".synthetic")
    depth, q, t, K = syn.room_views(6, 120, 160, seed=seed)
    xyz = fusion_ref.fuse_frames(depth, q, t, *K).astype(np.float32)
    return xyz[np.isfinite(xyz).all(axis=1)]


def test_sampler_known_answers(L, S):
    assert REF.splitmix64(REF.GOLDEN) == 0xe220a8397b1dcdaf          # the first hash of seed 0
    lib = L.load()
    rows = (C.c_uint32 * 3)()
    for seed, h, n, want in KATS:
        assert REF.rows_of(seed, h, n) == want
        assert lib.r3d_ransac_rows(seed, h, n, rows) == 0, L.last_error()
        assert tuple(rows) == want
        assert S.ransac_rows(seed, h, n) == want
    rng = np.random.default_rng(0)
    for _ in range(300):
        seed, h, n = int(rng.integers(0, 2**64, dtype=np.uint64)), int(rng.integers(0, 65536)), int(rng.integers(1, 2**32))
        assert S.ransac_rows(seed, h, n) == REF.rows_of(seed, h, n)
        assert max(REF.rows_of(seed, h, n)) < n
    assert lib.r3d_ransac_rows(0, 0, 0, rows) == L.ERR_INVALID and lib.r3d_ransac_rows(0, 0, 2**32, rows) == L.ERR_INVALID
    assert lib.r3d_ransac_rows(0, 0, 5, None) == L.ERR_INVALID


def test_symbols_are_exported_and_bound(L):
    lib = L.load()
    for name in ("r3d_segment_plane", "r3d_ransac_rows"):
        assert hasattr(lib, name) and name in L.SIGNATURES
    r3d = importlib.import_module(PKG)
    assert callable(r3d.segment_plane) and callable(r3d.segment_planes)
    res, m = (C.c_double * 16)(), C.c_int64(-7)
    assert lib.r3d_segment_plane(None, None, 10, 0.01, 16, 0, None, None, res, C.byref(m)) == L.ERR_INVALID
    assert m.value == -7 and all(v == 0.0 for v in res)


def test_python_layer_rejects_bad_arguments_before_the_gpu(S):
    xyz = REF.cube(50, 0)
    for bad in (0.0, -1.0, float("nan"), float("inf"), "x", None):
        with pytest.raises(ValueError):
            S.segment_plane(xyz, bad)
        with pytest.raises(ValueError):
            S.segment_planes(xyz, bad)
    for bad in (0, -1, 65537, 2.5, True, None):
        with pytest.raises(ValueError):
            S.segment_plane(xyz, 0.01, bad)
        with pytest.raises(ValueError):
            S.segment_planes(xyz, 0.01, bad)
    for bad in (-1, 2**64, 1.5, None):
        with pytest.raises(ValueError):
            S.segment_plane(xyz, 0.01, 16, bad)
    with pytest.raises(ValueError):
        S.segment_plane(xyz[:2], 0.01, 16)
    with pytest.raises(ValueError):
        S.segment_plane(np.zeros((5, 2), np.float32))
    with pytest.raises(ValueError):
        S.segment_planes(xyz, 0.01, 16, max_planes=-1)
    with pytest.raises(ValueError):
        S.segment_planes(xyz, 0.01, 16, min_inliers=0)
    with pytest.raises(ValueError):
        S.segment_plane_device(None, 0, 2, 0.01, 16, 0, 0)
    # nothing to segment: no GPU is touched
    planes, labels, counts = S.segment_planes(xyz[:2], 0.01, 16)
    assert planes.shape == (0, 4) and labels.tolist() == [-1, -1] and counts.size == 0


def test_reference_exact_lattice_plane():
    xyz = REF.lattice_plane()
    for seed in (0, 2**64 - 1):
        r = REF.segment_plane(xyz, 0.01, 64, seed)
        on = xyz[:, 2] == np.float32(0.5)
        assert r.c_best == on.sum() == 1600 and np.array_equal(r.mask, on) and np.array_equal(r.I0, on)
        assert r.plane.tolist() == [0.0, 0.0, 1.0, -0.5]
        assert r.centroid[2] == 0.5 and r.eigenvalues[0] == 0.0


def test_reference_closed_forms_and_edges():
    # three points: one hypothesis can only be valid when it draws all three rows
    tri = np.float32([[0, 0, 0], [1, 0, 0], [0, 1, 0]])
    r = REF.segment_plane(tri, 0.01, 64, 0)
    assert r.n_valid > 0 and r.c_best == 3 and r.mask.sum() == 3 and r.plane.tolist() == [0.0, 0.0, 1.0, -0.0]
    # collinear points: every triple is invalid
    line = np.outer(np.arange(50, dtype=np.float32), np.float32([1, 2, -1]))
    r = REF.segment_plane(line, 0.01, 128, 0)
    assert r.n_valid == 0 and r.c_best == 0 and not r.mask.any() and np.isnan(r.plane).all() and not r.counts.any()
    # non-finite rows are nobody's inliers and make their hypotheses invalid
    bad = REF.nonfinite()
    hyp = REF.hypotheses(bad, 512, 1)
    finite = np.isfinite(bad).all(axis=1)
    assert not hyp.valid[~finite[hyp.rows].all(axis=1)].any() and hyp.valid.any() and not hyp.valid.all()
    r = REF.segment_plane(bad, 0.01, 512, 1)
    assert not r.mask[~finite].any() and not r.I0[~finite].any() and r.c_best > 100
    # mostly duplicate triples
    hyp = REF.hypotheses(REF.hot(), 256, 0)
    assert 0 < hyp.valid.sum() < 128
    # sign rule: the lowest axis wins ties
    assert REF.orient(np.array([-0.5, 0.5, 0.1])).tolist() == [0.5, -0.5, -0.1]
    assert REF.orient(np.array([0.1, -0.7, 0.7])).tolist() == [-0.1, 0.7, -0.7]


def check_room(planes, labels, counts, lo, hi):
    """The room conditions of the issue: six planes, one per face, 1 - |n_axis| <= 1e-6, offsets within 1e-3, <= 0.1 % unlabelled."""
    assert planes.shape == (6, 4) and counts.shape == (6,)
    faces = REF.room_faces(planes, lo, hi)
    assert sorted((a, s) for a, s, _, _ in faces) == [(a, s) for a in range(3) for s in range(2)], faces
    for _, _, tilt, off in faces:
        assert tilt <= 1e-6 and off <= 1e-3, faces
    assert (labels < 0).mean() <= 1e-3
    for k in range(6):
        assert (labels == k).sum() == counts[k]


@pytest.fixture(scope="module")
def room():
    return fused_room()


@pytest.mark.parametrize("seed", range(5))
def test_reference_room_scene(room, seed):
    syn = importlib.import_module(PKG + ".synthetic")
    assert room.shape == (115200, 3)
    planes, labels, counts = REF.segment_planes(room, 0.01, 256, 6, 100, seed)
    check_room(planes, labels, counts, syn.ROOM_LO, syn.ROOM_HI)


def test_reference_noisy_scene():
    xyz, normal = REF.noisy_plane()
    r = REF.segment_plane(xyz, 0.01, 512, 0)
    got = r.plane[:3]
    sin_angle = np.linalg.norm(np.cross(got, normal))
    assert sin_angle <= np.sin(np.radians(0.5)), np.degrees(np.arcsin(sin_angle))
    assert 0.6 * xyz.shape[0] <= r.mask.sum() <= 0.8 * xyz.shape[0]
    c, n_ref, sin_bound, c_bound, gap_ok = REF.refit_bounds(xyz, r.I0, r.anchor)
    assert gap_ok and sin_bound < 1e-6 and c_bound < 1e-9       # the GPU test's bounds are meaningful on this scene
