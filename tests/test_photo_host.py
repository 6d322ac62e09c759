"""CPU: the colour-tracking reference (tests/photo_ref.py, a NumPy restatement of include/r3d.h "TSDF colour tracking") on images
whose gradients are known, its Jacobian against finite differences of its own residual, the textured corridor where depth alone
cannot see along the axis, the statistics of the GPU test's inputs, and the argument checks that need no device."""
import ctypes as C
import importlib
import os
import re

import numpy as np
import pytest

import photo_ref as PR
import raycast_color_ref as RCC
import track_ref as TR
import tsdf_color_ref as TC
from helpers import PKG, ROOT

F = np.float32
NEW_SYMBOLS = ["r3d_intensity_map", "r3d_track_accumulate_rgb", "r3d_track_iterate_rgb", "r3d_tsdf_track_rgb"]


def test_ramp_image_gives_the_gradient_inside_and_nan_at_edges():
    h, w = 6, 9
    v, u = np.meshgrid(np.arange(h), np.arange(w), indexing="ij")
    grey = (10 + 4 * u + 6 * v).astype(np.uint8)
    rgb = np.stack([grey] * 3, axis=-1)
    depth = np.ones((h, w), F)
    I, packed = PR.intensity_map(rgb, depth, 0.05)
    assert I.dtype == F and packed.dtype == F and packed.shape == (h, w, 4)
    # the luma of a grey pixel is the grey value to f32 rounding; the gradient is the ramp's slope
    assert np.abs(I - grey).max() <= 255 * 2.0 ** -22
    assert np.array_equal(packed[..., 0].view(np.uint32), I.view(np.uint32)) and np.all(packed[..., 3] == 0)
    gx, gy = packed[..., 1], packed[..., 2]
    assert np.isnan(gx[:, [0, -1]]).all() and np.isnan(gy[[0, -1], :]).all()
    assert np.abs(gx[:, 1:-1] - 4).max() <= 255 * 2.0 ** -22 and np.abs(gy[1:-1, :] - 6).max() <= 255 * 2.0 ** -22
    # ... and bit for bit the written formula of the map's own intensities
    assert np.array_equal(gx[:, 1:-1].view(np.uint32), (F(0.5) * (I[:, 2:] - I[:, :-2])).view(np.uint32))
    assert np.array_equal(gy[1:-1, :].view(np.uint32), (F(0.5) * (I[2:, :] - I[:-2, :])).view(np.uint32))
    # an invalid pixel: no intensity there, no gradient there or next to it along the axis of the difference
    for bad in (0.0, -1.0, np.nan, np.inf):
        d = depth.copy()
        d[2, 4] = bad
        I2, p2 = PR.intensity_map(rgb, d, 0.05)
        assert np.isnan(I2[2, 4]) and np.isnan(p2[2, 4, 1:3]).all()
        assert np.isnan(p2[2, [3, 5], 1]).all() and np.isnan(p2[[1, 3], 4, 2]).all()
        assert np.isfinite(p2[2, [3, 5], 2]).all() and np.isfinite(p2[[1, 3], 4, 1]).all()
        assert np.isfinite(I2).sum() == h * w - 1
    # a depth jump: none across it, on either side; max_jump = inf takes every valid neighbour
    d = depth.copy()
    d[:, 5:] = 1.2
    _, p3 = PR.intensity_map(rgb, d, 0.05)
    assert np.isnan(p3[:, 4:6, 1]).all() and np.isfinite(p3[:, [3, 6], 1]).all() and np.isfinite(p3[1:-1, :, 2]).all()
    _, p4 = PR.intensity_map(rgb, d, np.inf)
    assert np.isfinite(p4[:, 1:-1, 1]).all()
    _, p5 = PR.intensity_map(rgb, d, 0.0)      # 0: only equal depths
    assert np.isfinite(p5[:, [1, 2, 3, 6, 7], 1]).all() and np.isnan(p5[:, 4:6, 1]).all()
    # rasters too small for a difference
    for shape in [(1, 1), (2, 2), (1, 5)]:
        _, p = PR.intensity_map(np.zeros(shape + (3,), np.uint8), np.ones(shape, F), 1.0)
        assert np.isnan(p[..., 2]).all() and (np.isnan(p[..., 1]).all() or shape[1] >= 3)


def test_jacobian_against_finite_differences_of_the_residual():
    """A model intensity that is linear in (u, v) has the bilinear interpolant and the central differences of the same plane, so
    rI under a small twist xi of T_total changes by J . xi up to second order.  eps = 1e-6: the second-order term is ~1e-12 of
    the first's scale, the fp64 rounding of rI (~255 x 2^-52) over 2 eps is ~3e-8."""
    h, w = 24, 32
    case = TR.analytic_case(h, w, 1.0, 0.5, (0.02, 0.01, -0.02))
    v, u = np.meshgrid(np.arange(h), np.arange(w), indexing="ij")
    packed = np.stack([20 + 3.0 * u + 2.0 * v, np.full((h, w), 3.0), np.full((h, w), 2.0), np.zeros((h, w))], axis=-1).astype(F)
    Is = np.full((h, w), 100.0, F)
    S = TR.inverse_pose(case["model_row"])
    args = (case["src_vertex"], None, case["model_vertex"], case["model_normal"], case["model_row"], S, case["K"], 0.5, -1.0, Is, packed,
            1.0, 1e9)
    base = PR.associate(*args)
    assert len(base.pixels) >= 0.5 * h * w
    eps = 1e-6
    for k in range(6):
        xi = np.zeros(6)
        xi[k] = eps
        rI = []
        for sign in (1.0, -1.0):
            wv, t = sign * xi[:3], sign * xi[3:]
            T = np.eye(4)
            T[:3, :3] += np.array([[0, -wv[2], wv[1]], [wv[2], 0, -wv[0]], [-wv[1], wv[0], 0]])
            T[:3, 3] = t
            a = PR.associate(*args, T_total=T)
            full = np.full(h * w, np.nan)
            full[a.pixels] = a.rI
            rI.append(full[base.pixels])
        fd = (rI[0] - rI[1]) / (2 * eps)
        keep = np.isfinite(fd)
        assert keep.sum() >= 0.9 * len(base.pixels)
        scale = np.abs(base.J[keep]).max()
        assert np.abs(fd[keep] - base.J[keep, k]).max() <= 1e-5 * scale, (k, np.abs(fd[keep] - base.J[keep, k]).max(), scale)


def test_symbols_in_header_and_signatures():
    L = importlib.import_module(PKG + "._lib")
    header = open(os.path.join(ROOT, "include", "r3d.h")).read()
    for name in NEW_SYMBOLS:
        assert re.search(r"^int %s\(" % name, header, re.M), name
        assert name in L.SIGNATURES
        n_args = len(re.search(r"^int %s\((.*?)\);" % name, header, re.M | re.S).group(1).split(","))
        assert len(L.SIGNATURES[name][1]) == n_args, name
    assert "TSDF colour tracking" in header and "Not done here: photometric" not in header
    assert "r3d_tsdf_track_pyramid" in header.split("TSDF colour tracking")[-1]     # the limitation is stated


def test_library_argument_errors_without_device():
    """NULL handles are refused before any device is touched, and nothing is written to the host outputs"""
    L = importlib.import_module(PKG + "._lib")
    lib = L.load()
    s = np.full(32, 7.0)
    p = s.ctypes.data
    assert lib.r3d_intensity_map(None, p, p, 1, 2, 2, 0.05, None, None) == L.ERR_INVALID and "NULL" in L.last_error()
    assert lib.r3d_track_accumulate_rgb(None, None, p, None, p, p, p, p, 0.5, -1.0, p, p, 1.0, 1.0, p, None, None, None) == L.ERR_INVALID
    assert "NULL" in L.last_error()
    assert lib.r3d_track_iterate_rgb(None, None, p, None, p, p, p, p, 0.5, -1.0, p, p, 1.0, 1.0, 1, p) == L.ERR_INVALID
    assert lib.r3d_tsdf_track_rgb(None, None, p, L.DEPTH_F32, 1.0, p, p, 1.0, 0.05, 0.0, float("inf"), 0.05, 0.5, -1.0, 1.0, 1.0, 1, p,
                                  p) == L.ERR_INVALID
    assert np.all(s == 7.0)


def test_python_layer_argument_checks():
    tracking = importlib.import_module(PKG + ".tracking")
    assert tracking.photo_args(None, None) == (tracking.PHOTO_WEIGHT, tracking.I_MAX)
    for bad in [(-1.0, 1.0), (float("nan"), 1.0), (float("inf"), 1.0), (1.0, 0.0), (1.0, float("inf")), ("x", 1.0)]:
        with pytest.raises(ValueError):
            tracking.photo_args(*bad)
    rgb, d = np.zeros((4, 5, 3), np.uint8), np.ones((4, 5), F)
    for args in [(rgb.astype(np.float32), d, 0.05), (rgb, d.astype(np.float64), 0.05), (rgb, d[:3], 0.05), (rgb, d, -1.0),
                 (rgb, d, float("nan")), (rgb[..., :2], d, 0.05)]:
        with pytest.raises(ValueError):
            tracking.intensity_map(*args)
    tool = importlib.import_module(PKG + ".other_tools.integrate_tsdf")
    base = ["--voxel-size", "1", "--trunc", "3"]
    ok = tool.parse_args(base + ["--track", "--color-dir", "c", "--track-color"])
    assert ok.track and ok.track_color
    for bad in (["--track-color"], ["--track", "--track-color"], ["--color-dir", "c", "--track-color"],
                ["--track", "--color-dir", "c", "--track-color", "--track-pyramid", "4,2"], ["--track", "--color-dir", "c"]):
        with pytest.raises(SystemExit):
            tool.parse_args(base + bad)


@pytest.fixture(scope="module")
def corridor():
    """four frames 0.1 m apart along the axis integrated with their colours; a fifth frame 0.1 m further on, guessed at the
    fourth's pose; the model's maps ray-cast at that guess and both intensity maps (all by the NumPy references)"""
    tracking = importlib.import_module(PKG + ".tracking")
    depths, rgbs, rows, K = PR.corridor_frames([0.0, 0.1, 0.2, 0.3])
    vol = TC.ColorVolume(PR.CORRIDOR_ORIGIN, PR.CORRIDOR_VS, PR.CORRIDOR_DIMS, PR.CORRIDOR_TR)
    TC.integrate(vol, depths, rgbs, rows, K)
    d_new, rgb_new, true_row, _ = PR.corridor_view(0.4)
    guess = rows[-1]
    depth, vertex, normal, rgb = RCC.raycast(vol, guess[None], K, PR.CORRIDOR_SHAPE)
    sv = TR.camera_points(d_new.astype(np.float64), K).astype(F)
    sv[d_new <= 0] = 0.0
    Is, _ = PR.intensity_map(rgb_new, sv[..., 2], 0.3)
    _, packed = PR.intensity_map(rgb[0], depth[0], 0.3)
    return dict(sv=sv, vertex=vertex[0], normal=normal[0], guess=guess, true_row=true_row, K=K, Is=Is, packed=packed,
                w=tracking.PHOTO_WEIGHT, i_max=tracking.I_MAX)


def test_corridor_depth_alone_is_blind_along_the_axis_and_colour_is_not(corridor):
    c = corridor
    before = PR.along_axis_error(c["guess"], c["true_row"])
    assert abs(before + 0.1) < 1e-9
    row_d, info_d = PR.track(c["sv"], None, c["vertex"], c["normal"], c["guess"], c["K"], 2 * PR.CORRIDOR_TR, -1.0, 10)
    after_d = PR.along_axis_error(row_d, c["true_row"])
    # depth only: the step is reported singular, or (the ray-cast planes are not exact planes) it is solved and goes nowhere
    assert info_d["status"] == 1 or abs(after_d) >= 0.9 * abs(before), (info_d, after_d)
    row_c, info_c = PR.track(c["sv"], None, c["vertex"], c["normal"], c["guess"], c["K"], 2 * PR.CORRIDOR_TR, -1.0, 10, c["Is"], c["packed"],
                             c["w"], c["i_max"])
    after_c = PR.along_axis_error(row_c, c["true_row"])
    print("corridor: along-axis error %.5f -> depth only %.5f, with colour %.5f (%d photometric pairs, rms %.2f)"
          % (before, after_d, after_c, info_c["photo_pairs"], info_c["photo_rms"]))
    assert info_c["status"] == 0 and info_c["photo_pairs"] >= 0.2 * c["Is"].size
    assert abs(after_c) <= 0.2 * abs(before)
    e = TR.pose_error(row_c, c["true_row"])
    assert e[1] <= 0.02 and e[0] <= 0.5


@pytest.mark.parametrize("h,w", [(31, 33), (32, 32), (25, 41), (48, 64)])
def test_dirty_inputs_leave_the_reference_enough_to_check(h, w):
    case = PR.dirty_case(h, w, 1)
    n = h * w
    reasons = {k: 0 for k in PR.REASONS}
    for which in ("truth", "offset", "behind", "shifted"):
        a = PR.associate(case["src_vertex"], None, case["model_vertex"], case["model_normal"], case["model_row"], case["S"][which],
                         case["K"], 0.5, -1.0, case["src_intensity"], case["model_packed"], 1e-4, PR.DIRTY_I_MAX)
        for k in reasons:
            reasons[k] += a.reasons[k]
        if which == "truth":
            assert a.sums[29] >= 0.25 * n, (a.sums[29], n)
            assert np.isfinite(a.photo).sum() == a.sums[29]
    assert all(v > 0 for v in reasons.values()), reasons
