"""CPU: the tracking reference (tests/track_ref.py, a NumPy restatement of include/r3d.h "TSDF tracking") against hand-made and
analytic cases, and the argument checks of the Python layer and of the library that need no device."""
import ctypes as C
import importlib

import numpy as np
import pytest

import track_ref as TR
from helpers import PKG

K57 = (5.0, 5.0, 3.0, 2.0)     # a 5 x 7 raster: fx, fy, cx, cy
IDENT_ROW = np.concatenate([np.eye(3).reshape(9), np.zeros(3)])


def plane_maps(h, w, K, z=2.0):
    """a wall z = const seen by a camera at the origin: camera-frame = world vertex map, normal (0, 0, -1)"""
    v = TR.camera_points(np.full((h, w), z), K).astype(np.float32)
    n = np.zeros((h, w, 3), np.float32)
    n[..., 2] = -1.0
    return v, n


def test_every_reject_code():
    h, w = 5, 7
    mv, mn = plane_maps(h, w, K57)
    sv = mv.copy()
    sn = mn.copy()                                 # source normals = model normals
    want = np.arange(h * w, dtype=np.int32)
    sv[0, 0] = (np.nan, 0, 1)
    want[0] = -1
    sv[0, 1] = (0, 0, 0)                            # Z = 0: no measurement
    want[1] = -1
    sv[0, 2] = (0.1, 0.1, -2.0)
    want[2] = -1
    sv[0, 3] = (np.inf, 0, 1)
    want[3] = -1
    sv[1, 0] = (-9.0, 0.0, 2.0)                     # projects left of the image
    want[7] = -2
    sv[1, 1] = (0.0, 9.0, 2.0)                      # below it
    want[8] = -2
    mv[2, 2] = np.nan                               # a miss of the ray caster
    mn[2, 2] = np.nan
    want[2 * w + 2] = -3
    mn[2, 3] = 0.0                                  # a surface without a normal
    want[2 * w + 3] = -3
    sv[3, 3] *= np.float32(1.5)                     # same pixel, 1 m behind the wall
    want[3 * w + 3] = -4
    sn[4, 4] = (0.0, 0.0, 1.0)                      # faces the other way
    want[4 * w + 4] = -5
    sn[4, 5] = 0.0                                  # no source normal
    want[4 * w + 5] = -5
    sn[4, 6] = (np.nan, 0, 0)
    want[4 * w + 6] = -5
    a = TR.associate(sv, sn, mv, mn, IDENT_ROW, np.eye(4), K57, 0.5, 0.5)
    assert a.match.tolist() == want.tolist()
    assert set(a.match[a.match < 0].tolist()) == {-1, -2, -3, -4, -5}
    assert a.sums[0] == (want >= 0).sum() and np.all(a.residual == 0)
    # without source normals code -5 cannot occur and those pixels match
    b = TR.associate(sv, None, mv, mn, IDENT_ROW, np.eye(4), K57, 0.5, 0.5)
    want2 = want.copy()
    want2[[4 * w + 4, 4 * w + 5, 4 * w + 6]] = [4 * w + 4, 4 * w + 5, 4 * w + 6]
    assert b.match.tolist() == want2.tolist()
    # behind the model camera: -2 everywhere a source point exists
    S = np.eye(4)
    S[2, 3] = -10.0
    c = TR.associate(sv, None, mv, mn, IDENT_ROW, S, K57, 0.5, -1.0)
    assert set(c.match.tolist()) == {-1, -2}


def test_identical_frame_gives_identity():
    case = TR.analytic_case(24, 32, 0.0, 0.0, (0.0, 0.0, 0.0))
    S = TR.inverse_pose(case["model_row"])
    a = TR.associate(case["src_vertex"], None, case["model_vertex"], case["model_normal"], case["model_row"], S, case["K"], 0.5, -1.0)
    assert np.array_equal(a.match, np.arange(24 * 32, dtype=np.int32))
    assert np.abs(a.residual).max() <= 1e-6        # the two maps are f32 roundings of the same points
    icp = importlib.import_module(PKG + ".icp")
    T, rms = icp.plane_step_from_sums(a.sums)
    assert np.abs(T - np.eye(4)).max() <= 1e-6 and rms <= 1e-6
    row, info = TR.track(case["src_vertex"], None, case["model_vertex"], case["model_normal"], case["model_row"], case["K"], 0.5, -1.0, 3)
    assert info["status"] == 0
    ang, dist = TR.pose_error(row, case["model_row"])
    assert ang <= 1e-4 and dist <= 1e-5


# (h, w, yaw step in degrees, pitch step, centre step, rotation bound in degrees, centre bound in metres)
CONVERGENCE = [(48, 64, 2.0, 1.0, (0.03, 0.02, -0.04), 0.05, 0.002),
               (96, 128, 5.0, 2.5, (0.08, 0.05, -0.11), 0.01, 0.001)]


@pytest.mark.parametrize("h,w,dyaw,dpitch,dc,rot_max,centre_max", CONVERGENCE)
def test_convergence_on_analytic_maps(h, w, dyaw, dpitch, dc, rot_max, centre_max):
    """Guess = the model pose, dist_max 0.5, no normal gate, 10 iterations.  At 48 x 64 (start 2.236 degrees / 0.0539 m) a
    float64 evaluation of the specification stands at 0.0125 degrees / 3.6e-4 m from the fourth iteration on, 2885 of 3072
    pixels matched; the floor is nearest-pixel pairs across room edges.  The bounds 0.05 degrees / 0.002 m are 4-5 x that, so
    that a restatement which orders its arithmetic differently still passes.  At 96 x 128 (yaw + 5, pitch + 2.5 degrees, centre
    + (0.08, 0.05, -0.11): start 5.59 degrees / 0.145 m) it ends at 0.0045 degrees / 2.0e-4 m; bounds 0.01 degrees / 0.001 m."""
    case = TR.analytic_case(h, w, dyaw, dpitch, dc)
    before = TR.pose_error(case["model_row"], case["true_row"])
    row, info = TR.track(case["src_vertex"], None, case["model_vertex"], case["model_normal"], case["model_row"], case["K"], 0.5, -1.0, 10)
    after = TR.pose_error(row, case["true_row"])
    print("analytic %dx%d: %.4f deg / %.4f m -> %.5f deg / %.6f m, %d of %d matched" %
          (h, w, before[0], before[1], after[0], after[1], info["matched"], h * w))
    if (h, w) == (48, 64):
        assert abs(before[0] - 2.236) < 1e-3 and abs(before[1] - 0.0539) < 1e-4
    else:
        assert abs(before[0] - 5.59) < 1e-2 and abs(before[1] - 0.145) < 1e-3
    assert info["status"] == 0
    assert after[0] < rot_max and after[1] < centre_max, after
    assert info["matched"] >= 0.8 * h * w


def test_single_wall_is_degenerate():
    h, w = 24, 32
    K = (0.8 * w, 0.8 * w, (w - 1) / 2.0, (h - 1) / 2.0)
    mv, mn = plane_maps(h, w, K, 2.0)
    sv, _ = plane_maps(h, w, K, 2.05)
    guess = IDENT_ROW.copy()
    guess[9:] = (0.01, -0.02, 0.0)
    row, info = TR.track(sv, None, mv, mn, guess, K, 0.5, -1.0, 4)
    assert info["status"] == 1 and info["pairs"] > 0.5 * h * w
    assert row.tobytes() == guess.tobytes()


def test_pose_composition_inverts():
    rng = np.random.default_rng(3)
    syn = importlib.import_module(PKG + ".synthetic")
    row = TR.pose_row(rng.normal(size=4), rng.normal(size=3))
    S = TR.inverse_pose(row)
    assert np.abs(S @ TR.pose_matrix(row) - np.eye(4)).max() < 1e-14
    assert np.abs(TR.pose_from(np.eye(4), S) - row).max() < 1e-14
    tracking = importlib.import_module(PKG + ".tracking")
    assert tracking.inverse_pose(row).tobytes() == S.tobytes()
    T = syn.pose_matrix(rng.normal(size=4), rng.normal(size=3) * 0.1)
    assert tracking.pose_from_state(T, S).tobytes() == TR.pose_from(T, S).tobytes()
    # M = T . S maps the source camera to the world: the pose found is its inverse
    assert np.abs(TR.pose_matrix(TR.pose_from(T, S)) @ (T @ S) - np.eye(4)).max() < 1e-13


# ---- validation without a device -------------------------------------------------------------------------------------------------
class _NoDevice:
    """stands where a context would: any use of it is a failure of "ValueError before anything is allocated" """

    def __getattr__(self, name):
        raise AssertionError("the context was used (%s) before the arguments were checked" % name)


def test_python_layer_validation():
    tracking = importlib.import_module(PKG + ".tracking")
    tsdf = importlib.import_module(PKG + ".tsdf")
    ok = np.zeros((5, 7, 3), np.float32)
    ctx = _NoDevice()
    bad_calls = [
        dict(src_vertex=ok.astype(np.float64)), dict(src_vertex=ok[0]), dict(src_vertex=np.zeros((5, 7, 2), np.float32)),
        dict(model_vertex=np.zeros((5, 8, 3), np.float32)), dict(model_normal=ok.astype(np.float64)),
        dict(src_normal=np.zeros((4, 7, 3), np.float32)), dict(model_pose_w2c=np.zeros(11)), dict(S=np.eye(3)),
        dict(intrinsics=(1.0, 1.0, 0.0)), dict(dist_max=0.0), dict(dist_max=np.inf), dict(dist_max=np.nan), dict(cos_min=1.5),
        dict(cos_min=np.nan), dict(dist_max="far"),
    ]
    base = dict(src_vertex=ok, model_vertex=ok, model_normal=ok, model_pose_w2c=IDENT_ROW, S=np.eye(4), intrinsics=K57, dist_max=0.5,
                cos_min=-1.0, src_normal=None, ctx=ctx)
    for bad in bad_calls:
        with pytest.raises(ValueError):
            tracking.track_sums(**{**base, **bad})
    # TSDFVolume.track / track_and_integrate: a volume object without a device behind it
    V = tsdf.TSDFVolume.__new__(tsdf.TSDFVolume)
    V.ctx, V.handle, V.color, V.voxel_size, V.sdf_trunc = ctx, None, False, 0.05, 0.2
    depth = np.ones((5, 7), np.float32)
    for kwargs in [dict(depth=depth[0]), dict(depth=depth.astype(np.float64)), dict(pose_guess_w2c=np.zeros(11)),
                   dict(pose_guess_w2c=np.full(12, np.nan)), dict(n_iters=-1), dict(n_iters=465), dict(n_iters=2.5), dict(dist_max=0.0),
                   dict(dist_max=np.inf), dict(max_angle_deg=180.0), dict(max_angle_deg=-1.0), dict(max_jump=-0.1), dict(min_weight=0.0),
                   dict(step=0.0), dict(t_near=-1.0), dict(t_near=2.0, t_far=1.0)]:
        with pytest.raises(ValueError):
            V.track(**{**dict(depth=depth, pose_guess_w2c=IDENT_ROW, intrinsics=K57), **kwargs})
    for kwargs in [dict(depths=np.ones((2, 5, 7), np.float64)), dict(first_pose_w2c=np.zeros(13)), dict(n_iters=-3), dict(dist_max=-1.0)]:
        with pytest.raises(ValueError):
            V.track_and_integrate(**{**dict(depths=np.ones((2, 5, 7), np.float32), first_pose_w2c=IDENT_ROW, intrinsics=K57), **kwargs})
    V.color = True
    with pytest.raises(ValueError):
        V.track_and_integrate(np.ones((2, 5, 7), np.float32), IDENT_ROW, intrinsics=K57)
    V.handle = None   # (nothing to destroy)


def test_library_argument_errors_without_device():
    """NULL handles are refused before any device is touched, and nothing is written to the host outputs"""
    L = importlib.import_module(PKG + "._lib")
    lib = L.load()
    sums = np.full(29, 7.0)
    pose, S = IDENT_ROW.copy(), np.eye(4)
    assert lib.r3d_track_accumulate(None, None, None, None, None, None, pose.ctypes.data, S.ctypes.data, 0.5, -1.0, sums.ctypes.data,
                                    None, None) == L.ERR_INVALID
    assert np.all(sums == 7.0)
    assert lib.r3d_track_iterate(None, None, None, None, None, None, pose.ctypes.data, S.ctypes.data, 0.5, -1.0, 1, None) == L.ERR_INVALID
    out, info = np.full(12, 7.0), np.full(4, 7.0)
    assert lib.r3d_tsdf_track(None, None, None, L.DEPTH_F32, 1.0, pose.ctypes.data, 1.0, 0.05, 0.0, C.c_double(float("inf")), 0.05, 0.5,
                              -1.0, 1, out.ctypes.data, info.ctypes.data) == L.ERR_INVALID
    assert np.all(out == 7.0) and np.all(info == 7.0)
    assert "NULL" in L.last_error()
