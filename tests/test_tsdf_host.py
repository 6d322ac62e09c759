"""CPU: the TSDF volume's NumPy reference (tests/tsdf_ref.py) on closed forms -- the conditions tests/test_gpu_tsdf.py asserts of
the device are asserted of the specification here first -- plus the library's argument errors and the Python layer's checks, none
of which needs a GPU."""
import ctypes as C
import importlib

import numpy as np
import pytest

import tsdf_ref as REF
from helpers import PKG


@pytest.fixture(scope="module")
def L():
    return importlib.import_module(PKG + "._lib")


@pytest.fixture(scope="module")
def T():
    return importlib.import_module(PKG + ".tsdf")


@pytest.mark.parametrize("wide", [False, True])
@pytest.mark.parametrize("dtype", [np.float32, np.uint8, np.uint16])
def test_reference_fronto_parallel_wall(wide, dtype):
    s = REF.wall_scene(wide, dtype)
    vol, passed, xyz, nrm = REF.run(s)
    REF.check_wall(s, xyz, nrm)
    nx, ny, _ = s["dims"]
    assert (len(xyz) == nx * ny) == (not wide)            # the narrow volume is inside the frustum, the wide one is not
    # linear interpolation is exact up to its roundings: x and y are untouched voxel centres
    gx, gy, _ = vol.centres()
    assert np.isin(xyz[:, 0], gx).all() and np.isin(xyz[:, 1], gy).all()


def test_reference_room():
    s = REF.room_scene()
    vol, passed, xyz, nrm = REF.run(s)
    REF.check_room(s, xyz)
    lens = np.linalg.norm(nrm.astype(np.float64), axis=1)
    assert (np.abs(lens[lens > 0] - 1.0) <= 1e-6).all() and (lens > 0).mean() > 0.99
    # the gradient points towards the cameras, which are inside the room: away from the nearest face
    mid = (np.asarray(s["lo"]) + np.asarray(s["hi"])) / 2
    towards = ((mid - xyz) * nrm).sum(axis=1)
    assert (towards > 0).mean() > 0.97
    # what the GPU file relies on: the eight views overlap pairwise, never fourfold along a crossing
    assert 0 < len(REF.extract(vol, 2)[0]) < len(xyz) and len(REF.extract(vol, 4)[0]) == 0


def test_reference_boundary_pixels_fall_on_the_stated_side():
    s = REF.boundary_scene()
    vol, passed, _, _ = REF.run(s)
    gx, gy, gz = vol.centres()
    assert gz[0] == 1.0 and -0.5 in gx and 3.5 in gx and -0.375 in gy and 2.625 in gy
    x0, x1 = int(np.nonzero(gx == -0.5)[0][0]), int(np.nonzero(gx == 3.5)[0][0])
    y0, y1 = int(np.nonzero(gy == -0.375)[0][0]), int(np.nonzero(gy == 2.625)[0][0])
    F = np.float32
    assert F(8) * (gx[x0] / gz[0]) + F(3.5) + F(0.5) == 0 and F(8) * (gx[x1] / gz[0]) + F(3.5) + F(0.5) == 32
    assert F(8) * (gy[y0] / gz[0]) + F(2.5) + F(0.5) == 0 and F(8) * (gy[y1] / gz[0]) + F(2.5) + F(0.5) == 24
    w = vol.w[0]
    assert w[y0, x0] == 1 and w[y0, x0 - 1] == 0 and w[y0 - 1, x0] == 0           # u + 0.5 = 0 is inside, one voxel less is not
    assert w[y0, x1] == 0 and w[y0, x1 - 1] == 1 and w[y1, x0] == 0 and w[y1 - 1, x0] == 1   # = W, = H are outside
    assert vol.tsdf[0, y0, x0] == 0.5


@pytest.mark.parametrize("dtype", [np.uint8, np.uint16, np.float32])
def test_reference_weights_count_the_frames_that_pass(dtype):
    s = REF.random_scene((33, 9, 5), 6, dtype, (24, 32), seed=1)
    vol, passed, _, _ = REF.run(s)
    per_frame = np.zeros_like(vol.w)
    for f in range(6):
        one = REF.Volume(s["origin"], s["vs"], s["dims"], s["tr"])
        n = REF.integrate(one, s["depths"][f:f + 1], s["poses"][f:f + 1], s["K"], s["scale"])
        assert set(np.unique(one.w)) <= {0.0, 1.0} and one.w.sum() == n
        per_frame += one.w
    assert np.array_equal(vol.w, per_frame) and vol.w.sum() == passed
    assert 0 < passed < 6 * vol.w.size                      # some pairs pass, some are rejected
    assert (vol.tsdf[vol.w == 0] == 0).all() and np.abs(vol.tsdf).max() <= 1.0 and vol.tsdf.min() < 0 < vol.tsdf.max()


def test_reference_batch_equals_frame_by_frame():
    s = REF.random_scene((65, 3, 2), 9, np.float32, (24, 32), seed=2)
    whole, _, xyz, nrm = REF.run(s)
    step = REF.Volume(s["origin"], s["vs"], s["dims"], s["tr"])
    for f in range(9):
        REF.integrate(step, s["depths"][f:f + 1], s["poses"][f:f + 1], s["K"], s["scale"])
    assert np.array_equal(whole.tsdf.view(np.uint32), step.tsdf.view(np.uint32)) and np.array_equal(whole.w, step.w)
    xyz2, nrm2 = REF.extract(step)
    assert len(xyz) > 0 and np.array_equal(xyz.view(np.uint32), xyz2.view(np.uint32)) and np.array_equal(nrm.view(np.uint32), nrm2.view(np.uint32))


def test_reference_unseen_volume_stays_empty():
    s = REF.random_scene((17, 4, 3), 5, np.uint16, (24, 32), seed=3, unseen=True)
    vol, passed, xyz, nrm = REF.run(s)
    assert passed == 0 and not vol.tsdf.any() and not vol.w.any() and xyz.shape == (0, 3) and nrm.shape == (0, 3)


def test_poses_w2c_is_the_inverse_of_the_fusion_table(T):
    r3d = importlib.import_module(PKG)
    rng = np.random.default_rng(0)
    q, t = rng.normal(size=(5, 4)), rng.normal(size=(5, 3))
    w2c, c2w = T.poses_w2c(q, t), r3d.pose_table(q, t)
    assert w2c.shape == (5, 12) and np.array_equal(w2c[:, 9:], t) and np.array_equal(c2w[:, 9:], t)
    for k in range(5):
        assert np.abs(w2c[k, :9].reshape(3, 3) @ c2w[k, :9].reshape(3, 3) - np.eye(3)).max() <= 1e-12
    with pytest.raises(ValueError):
        T.poses_w2c(q, t[:4])


def test_symbols_are_exported_and_bound(L, T):
    lib = L.load()
    names = ("r3d_tsdf_create", "r3d_tsdf_destroy", "r3d_tsdf_reset", "r3d_tsdf_integrate", "r3d_tsdf_integrate_host", "r3d_tsdf_volume",
             "r3d_tsdf_extract_points")
    for name in names:
        assert hasattr(lib, name) and name in L.SIGNATURES
    r3d = importlib.import_module(PKG)
    assert r3d.TSDFVolume is T.TSDFVolume and r3d.poses_w2c is T.poses_w2c
    header = open(importlib.import_module("helpers").ROOT + "/include/r3d.h").read()
    assert "#define R3D_TSDF_CHUNK %d " % T.CHUNK in header


def test_argument_errors_without_gpu(L):
    lib = L.load()
    assert lib.r3d_tsdf_destroy(None) == 0
    origin = (C.c_double * 3)(0.0, 0.0, 0.0)
    h = C.c_void_p(7)
    assert lib.r3d_tsdf_create(None, origin, 0.1, 4, 4, 4, 0.3, C.byref(h)) == L.ERR_INVALID and h.value is None
    assert lib.r3d_tsdf_create(None, origin, 0.1, 4, 4, 4, 0.3, None) == L.ERR_INVALID
    assert lib.r3d_tsdf_reset(None) == L.ERR_INVALID
    pose = (C.c_double * 12)()
    for n_frames, dtype in ((1, L.DEPTH_U8), (-1, L.DEPTH_U8), (1, 7), (0, L.DEPTH_F32)):
        assert lib.r3d_tsdf_integrate(None, None, None, dtype, n_frames, 1.0, pose) == L.ERR_INVALID
        assert lib.r3d_tsdf_integrate_host(None, None, None, dtype, n_frames, 1.0, pose) == L.ERR_INVALID
    n, p = C.c_int64(-7), C.c_void_p(5)
    assert lib.r3d_tsdf_volume(None, C.byref(p), C.byref(n)) == L.ERR_INVALID and n.value == -7 and p.value == 5
    assert lib.r3d_tsdf_extract_points(None, 1.0, None, None, 0, C.byref(n)) == L.ERR_INVALID and n.value == -7
    assert "NULL" in L.last_error()


def test_python_layer_rejects_bad_arguments_before_the_gpu(T):
    good = dict(origin=(0, 0, 0), voxel_size=0.1, dims=(4, 4, 4), sdf_trunc=0.3)
    for key, bads in (("origin", [(0, 0), (0, 0, float("nan")), (0, 0, float("inf")), "x"]),
                      ("voxel_size", [0.0, -1.0, float("nan"), float("inf"), 1e-60, None, True]),
                      ("sdf_trunc", [0.0, -0.5, float("nan"), 1e60, None]),
                      ("dims", [(4, 4), (0, 4, 4), (4, -1, 4), (2048, 2048, 512), (1.5, 2, 2), None])):
        for bad in bads:
            with pytest.raises((ValueError, TypeError)):
                T.TSDFVolume(**dict(good, **{key: bad}))
