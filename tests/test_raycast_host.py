"""CPU: the conditions tests/test_gpu_raycast.py relies on, asserted of the NumPy reference (tests/raycast_ref.py) itself -- the
wall, the sphere, the room's round trip and the structural cases -- so that the inputs are fair before a card sees them; and the
Python layer's argument checks, which need no GPU."""
import importlib

import numpy as np
import pytest

import mesh_ref as MREF
import raycast_ref as RC
import tsdf_ref as REF
from helpers import PKG

F = np.float32


def test_wall():
    """Every pixel whose ray meets the wall inside the box of voxel centres (float64, 1e-3 clear of the faces) is a hit; its
    depth is within raycast_ref.wall_depth_bound of d -- derived there from f32 rounding: 64 * 2^-24 * (|o_z| + nz vs + tr) =
    9.0e-6 for this scene; the reference's measured worst error is 2.4e-7 (one ulp of d) -- and its normal within 2^-20 of
    (0, 0, -1) (measured: exact)."""
    s = REF.wall_scene()
    vol = REF.run(s)[0]
    depth, vertex, normal, hit = RC.cast_view(vol, s["poses"][0], s["K"], (24, 32), step=RC.WALL_STEP)
    assert RC.WALL_STEP + s["vs"] <= s["tr"]                  # both bracketing samples lie in the untruncated band
    err, nerr = RC.check_wall(s, depth, vertex, normal)
    print("wall: hits %d, worst |depth - d| %.3g (bound %.3g), worst normal error %.3g" % (hit.sum(), err, RC.wall_depth_bound(s), nerr))
    assert np.array_equal(hit, RC.hits(vertex)) and np.array_equal(hit, depth > 0)
    assert (~hit).any()                                       # the volume is narrower than the image


def test_sphere():
    vol = MREF.sphere_volume()
    depth, vertex, normal = RC.raycast(vol, RC.sphere_poses(), RC.SPHERE_K, (24, 32), step=0.5)
    worst_r, worst_cos = RC.check_sphere(vertex, normal)
    print("sphere: worst | |vertex - centre| - r | %.3g voxel, worst cosine %.5f" % (worst_r, worst_cos))
    assert np.array_equal(depth > 0, RC.hits(vertex))


def test_round_trip_of_the_room():
    s = REF.room_scene()
    vol = REF.run(s)[0]
    poses = REF.poses_w2c(s["quats"], s["ts"])
    depth, vertex, normal = RC.raycast(vol, poses, s["K"], (96, 128))
    share, err = RC.check_round_trip(s, depth, vertex)
    print("room: %.3f of the pixels hit, worst |depth - input| %.3g (voxel diagonal %.3g)" % (share, err, np.sqrt(3.0) * s["vs"]))


def test_a_volume_without_cells_gives_all_misses():
    for dims in ((1, 5, 5), (7, 6, 1), (4, 1, 4)):
        vol = MREF.random_volume(dims, 3)
        centre = np.array(dims) / 2.0
        pose = RC.look_at(centre - np.array([0.3, 0.2, 9.0]), centre)
        depth, vertex, normal, hit = RC.cast_view(vol, pose, RC.SPHERE_K, (5, 7), step=0.25)
        assert not hit.any() and not depth.any()
        assert (vertex.view(np.uint32) == RC.NONE).all() and (normal.view(np.uint32) == RC.NONE).all()


def test_a_camera_looking_away_gives_all_misses():
    vol = MREF.sphere_volume()
    pose = RC.look_at((10.0, 10.0, -12.0), (10.0, 10.0, -40.0))
    depth, vertex, normal, hit = RC.cast_view(vol, pose, RC.SPHERE_K, (24, 32), step=0.5)
    assert not hit.any() and not depth.any() and (vertex.view(np.uint32) == RC.NONE).all()


ZERO_K = (40.0, 40.0, 16.0, 12.0)            # integer principal point: pixel (12, 16) looks along the optical axis


def test_rays_with_a_zero_direction_component():
    """identity pose, ui = cx: dw_x is exactly zero down that column (and dw_y along the row vi = cy).  With the camera between
    the x slabs the column hits; with the camera outside them the column misses while its neighbours may still enter the box."""
    s = REF.wall_scene()
    vol = REF.run(s)[0]
    R, C = RC.prepare_pose(s["poses"][0])
    assert float((F(16.0) - F(ZERO_K[2])) / F(ZERO_K[0])) == 0.0
    depth, vertex, normal, hit = RC.cast_view(vol, s["poses"][0], ZERO_K, (24, 32), step=RC.WALL_STEP)
    assert hit[12, 16] and hit[:, 16].sum() > 3 and hit[12, :].sum() > 3
    assert vertex[12, 16, 0] == 0.0 and vertex[12, 16, 1] == 0.0
    assert abs(float(depth[12, 16]) - s["d"]) <= RC.wall_depth_bound(s)
    shifted = s["poses"][0].copy()
    shifted[9] = -0.6                                          # t = -R C: the camera centre at x = +0.6, outside [-0.375, 0.375]
    depth, vertex, normal, hit = RC.cast_view(vol, shifted, ZERO_K, (24, 32), step=RC.WALL_STEP)
    assert not hit[:, 16].any() and hit.any()


def test_camera_centre_inside_the_volume():
    vol = MREF.sphere_volume()
    pose = RC.look_at((1.5, 2.0, 1.5), (10.0, 10.0, 10.0))
    depth, vertex, normal, hit = RC.cast_view(vol, pose, RC.SPHERE_K, (24, 32), step=0.5)
    assert hit.sum() >= 100 and (~hit).sum() >= 100
    RC.check_sphere(vertex[None], normal[None])


def test_t_far_truncates_and_t_near_beyond_the_surface_misses():
    vol = MREF.sphere_volume()
    pose = RC.sphere_poses()[0]                                # 22 voxels in front of the sphere's centre
    C = np.array([10.0, 10.0, -12.0])
    full = RC.cast_view(vol, pose, RC.SPHERE_K, (24, 32), step=0.5)
    cut = RC.cast_view(vol, pose, RC.SPHERE_K, (24, 32), step=0.5, t_far=17.0)
    assert 0 < cut[3].sum() < full[3].sum() and not (cut[3] & ~full[3]).any()
    assert np.array_equal(cut[1][cut[3]].view(np.uint32), full[1][cut[3]].view(np.uint32))    # the same march where it ends in time
    assert np.linalg.norm(cut[1][cut[3]].astype(np.float64) - C, axis=1).max() <= 17.0
    assert np.linalg.norm(full[1][full[3] & ~cut[3]].astype(np.float64) - C, axis=1).min() > 17.0 - 0.5
    beyond = RC.cast_view(vol, pose, RC.SPHERE_K, (24, 32), step=0.5, t_near=24.0)            # starts inside the sphere
    assert not beyond[3].any() and not beyond[0].any()


def test_invalid_voxels_make_holes_and_min_weight_counts():
    ref = MREF.random_volume((16, 16, 17), 5, invalid=0.1)
    centre = np.array([8.0, 8.0, 8.5])
    pose = RC.look_at(centre + np.array([3.0, -2.0, -20.0]), centre)
    full = RC.cast_view(MREF.random_volume((16, 16, 17), 5), pose, RC.SPHERE_K, (24, 32), step=0.25)
    holes = RC.cast_view(ref, pose, RC.SPHERE_K, (24, 32), step=0.25)
    assert full[3].sum() > 100 and holes[3].sum() > 100 and not np.array_equal(full[1].view(np.uint32), holes[1].view(np.uint32))
    none = RC.cast_view(ref, pose, RC.SPHERE_K, (24, 32), step=0.25, min_weight=2.0)
    assert not none[3].any()


def test_product_does_not_import_the_reference():
    import os
    from helpers import ROOT
    for base, _, files in os.walk(os.path.join(ROOT, PKG)):
        for name in files:
            if name.endswith(".py"):
                with open(os.path.join(base, name)) as fh:
                    assert "raycast_ref" not in fh.read(), name


def test_python_layer_rejects_bad_arguments_without_a_gpu():
    T = importlib.import_module(PKG + ".tsdf")
    assert T._ray_range(None, 0.0, float("inf"), 0.05) == (0.05, 0.0, float("inf"))
    assert T._ray_range(0.1, 1, 2, 0.05) == (0.1, 1.0, 2.0)
    for step, tn, tf in ((0.0, 0.0, 1.0), (-1.0, 0.0, 1.0), (float("nan"), 0.0, 1.0), (float("inf"), 0.0, 1.0), (1e-60, 0.0, 1.0),
                         (0.1, -0.5, 1.0), (0.1, float("nan"), 1.0), (0.1, float("inf"), float("inf")), (0.1, 1.0, 1.0),
                         (0.1, 2.0, 1.0), (0.1, 0.0, float("nan")), (0.1, "a", 1.0), (0.1, True, 2.0), ("x", 0.0, 1.0)):
        with pytest.raises(ValueError):
            T._ray_range(step, tn, tf, 0.05)
