"""CPU: the depth-pyramid reference (tests/pyramid_ref.py, a NumPy restatement of include/r3d.h "Depth pyramid") on hand-written
blocks, the level camera rule, and the argument checks of the Python layer and of the library that need no device."""
import ctypes as C
import importlib

import numpy as np
import pytest

import pyramid_ref as PR
import track_ref as TR
from helpers import PKG

F = np.float32
INF, NAN = F(np.inf), F(np.nan)
IDENT_ROW = np.concatenate([np.eye(3).reshape(9), np.zeros(3)])
K57 = (5.0, 5.0, 3.0, 2.0)


def half1(block, max_jump):
    """the one output of one 2 x 2 block"""
    out = PR.depth_half(np.array(block, dtype=F).reshape(2, 2), max_jump)
    assert out.shape == (1, 1) and out.dtype == F
    return out[0, 0]


def test_half_sampler_on_hand_written_blocks():
    # all valid: the sum runs in block order from 0.0f and is divided by the count
    assert half1([1, 2, 3, 4], INF) == F(2.5)
    assert half1([4, 3, 2, 1], 3.0) == F(2.5)
    want = (((F(0.0) + F(0.1)) + F(0.2)) + F(0.3)) / F(3.0)
    assert half1([0.1, 0.2, 0.3, 7.0], 0.5).tobytes() == want.tobytes()
    # one valid; none valid gives 0 ("no measurement")
    assert half1([0, NAN, 2.5, -1], 0.05) == F(2.5)
    assert half1([0, NAN, INF, -1], INF) == F(0.0) and half1([0, 0, 0, 0], 0.0) == F(0.0)
    assert half1([-INF, -0.0, NAN, INF], 1.0) == F(0.0)
    # a NaN, +inf, 0 or negative entry takes no part, wherever it stands
    for bad in (NAN, INF, F(0.0), F(-2.0), -INF):
        for at in range(4):
            block = [2.0, 2.0, 2.0, 2.0]
            block[at] = bad
            assert half1(block, INF) == F(2.0), (bad, at)
            block = [1.0, 2.0, 4.0, 8.0]
            keep = [v for k, v in enumerate(block) if k != at]
            block[at] = bad
            assert half1(block, INF) == ((F(keep[0]) + F(keep[1])) + F(keep[2])) / F(3.0), (bad, at)
    # foreground wins: a block across a depth edge is the near side only, wherever the near pixels stand
    assert half1([1.0, 3.0, 1.02, 3.0], 0.05) == (F(1.0) + F(1.02)) / F(2.0)
    assert half1([3.0, 3.0, 3.0, 1.0], 0.05) == F(1.0)
    # a jump exactly equal to max_jump is included, one ulp over is excluded
    assert F(1.25) - F(1.0) == F(0.25)
    assert half1([1.0, 1.25, 0, 0], 0.25) == F(1.125)
    over = np.nextafter(F(1.25), INF)
    assert over - F(1.0) > F(0.25) and half1([1.0, over, 0, 0], 0.25) == F(1.0)
    assert half1([1.0, 1.25, 0, 0], np.nextafter(F(0.25), F(0.0))) == F(1.0)
    # max_jump 0: the minimum and its exact copies; +inf: every valid depth
    assert half1([2.0, 1.5, 1.5, 9.0], 0.0) == F(1.5)
    assert half1([2.0, 1.5, 1.5, 9.0], INF) == F(3.5)
    assert half1([3e38, 3e38, 0, 0], INF) == INF      # the f32 sum overflows as the specification's does


def test_half_sampler_shapes_and_block_layout():
    d = np.arange(1, 5 * 7 + 1, dtype=F).reshape(5, 7)
    out = PR.depth_half(d, INF)
    assert out.shape == (2, 3)                        # the odd last row and column are dropped
    for v in range(2):
        for u in range(3):
            b = [d[2 * v, 2 * u], d[2 * v, 2 * u + 1], d[2 * v + 1, 2 * u], d[2 * v + 1, 2 * u + 1]]
            assert out[v, u] == (((F(0.0) + b[0]) + b[1]) + b[2] + b[3]) / F(4.0)
    levels = PR.depth_levels(np.ones((17, 65), F), 4, 0.05)
    assert [a.shape for a in levels] == [(17, 65), (8, 32), (4, 16), (2, 8)]


def test_level_camera_rule():
    tracking = importlib.import_module(PKG + ".tracking")
    K = (102.4, 99.7, 63.5, 47.25)
    assert tracking.pyramid_intrinsics(K, 0) == K
    K1 = tracking.pyramid_intrinsics(K, 1)
    assert K1 == (0.5 * K[0], 0.5 * K[1], 0.5 * (K[2] - 0.5), 0.5 * (K[3] - 0.5)) == PR.pyramid_intrinsics(K, 1)
    # the ray of a coarse pixel goes through the centre of its 2 x 2 fine block
    for u in range(0, 64, 7):
        assert abs((u - K1[2]) / K1[0] - ((2 * u + 0.5) - K[2]) / K[0]) <= 1e-15
        assert abs((u - K1[3]) / K1[1] - ((2 * u + 0.5) - K[3]) / K[1]) <= 1e-15
    K3 = tracking.pyramid_intrinsics(K, 3)
    assert K3 == PR.pyramid_intrinsics(K, 3) == tracking.pyramid_intrinsics(tracking.pyramid_intrinsics(K1, 1), 1)
    for u in range(8):                               # three halvings: pixel u covers fine pixels 8u .. 8u + 7, centre 8u + 3.5
        assert abs((u - K3[2]) / K3[0] - ((8 * u + 3.5) - K[2]) / K[0]) <= 1e-15
    for bad in (-1, 1.5, True):
        with pytest.raises(ValueError):
            tracking.pyramid_intrinsics(K, bad)
    with pytest.raises(ValueError):
        tracking.pyramid_intrinsics((1.0, 2.0, 3.0), 1)


def test_pyramid_shape_on_odd_sizes():
    tracking = importlib.import_module(PKG + ".tracking")
    assert tracking.pyramid_shape(480, 640, 0) == (480, 640)
    assert tracking.pyramid_shape(480, 640, 2) == (120, 160)
    assert tracking.pyramid_shape(5, 7, 1) == (2, 3) == PR.pyramid_shape(5, 7, 1)
    assert tracking.pyramid_shape(17, 65, 1) == (8, 32)
    assert tracking.pyramid_shape(17, 65, 3) == (2, 8)
    assert tracking.pyramid_shape(17, 65, 5) == (0, 2)
    assert tracking.pyramid_shape(3, 3, 1) == (1, 1)
    with pytest.raises(ValueError):
        tracking.pyramid_shape(4, 4, -1)


def test_reference_loop_with_one_level_is_the_one_level_loop():
    case = TR.analytic_case(24, 32, 2.0, 1.0, (0.03, 0.02, -0.04))
    level = {"src_vertex": case["src_vertex"], "src_normal": None, "model_vertex": case["model_vertex"],
             "model_normal": case["model_normal"], "K": case["K"]}
    row, info = PR.track([level], [5], case["model_row"], 0.5, -1.0)
    want, winfo = TR.track(case["src_vertex"], None, case["model_vertex"], case["model_normal"], case["model_row"], case["K"], 0.5, -1.0, 5)
    assert row.tobytes() == want.tobytes() and info["status"] == winfo["status"] == 0
    assert info["iterations"] == 5 and len(info["rms_history"]) == 5 and info["rms"] == winfo["rms"] == info["rms_history"][-1]
    # a level with 0 iterations is skipped; its maps are never read
    row2, info2 = PR.track([level, None], [5, 0], case["model_row"], 0.5, -1.0)
    assert row2.tobytes() == want.tobytes() and info2["iterations"] == 5


# ---- validation without a device -------------------------------------------------------------------------------------------------
class _NoDevice:
    """stands where a context would: any use of it is a failure of "ValueError before any device use" """

    def __getattr__(self, name):
        raise AssertionError("the context was used (%s) before the arguments were checked" % name)


class _Cam:
    height, width, fx, fy, cx, cy, handle = 5, 7, 5.0, 5.0, 3.0, 2.0, None


BAD_PYRAMIDS = [(), [], (1,) * 9, (-1,), (3, -2), (2.5,), (3, "4"), (True, 2), (400, 65), 7, (None,),
                (1, 1, 1, 1)]                           # a 5 x 7 raster halves twice: 2 x 3, 1 x 1, then nothing is left


def test_python_layer_validation():
    tracking = importlib.import_module(PKG + ".tracking")
    tsdf = importlib.import_module(PKG + ".tsdf")
    assert tracking.MAX_LEVELS == 8 and tracking.MAX_ITERS == 464
    assert tracking.pyramid_levels((10, 5, 4), 96, 128) == [10, 5, 4]
    assert tracking.pyramid_levels(np.array([3, 0, 2]), 5, 7) == [3, 0, 2]
    assert tracking.pyramid_levels((400, 64), 5, 7) == [400, 64]
    assert tracking.pyramid_levels((1,) * 8, 128, 128) == [1] * 8
    with pytest.raises(ValueError):
        tracking.pyramid_levels((1,) * 8, 127, 128)
    ctx = _NoDevice()
    V = tsdf.TSDFVolume.__new__(tsdf.TSDFVolume)
    V.ctx, V.handle, V.color, V.voxel_size, V.sdf_trunc = ctx, None, False, 0.05, 0.2
    depth = np.ones((5, 7), F)
    for bad in BAD_PYRAMIDS:
        with pytest.raises(ValueError):
            V.track(depth, IDENT_ROW, intrinsics=K57, pyramid_iters=bad)
        with pytest.raises(ValueError):
            V.track_device(_Cam(), 0, np.float32, IDENT_ROW, pyramid_iters=bad)
        with pytest.raises(ValueError):
            V.track_and_integrate(np.ones((2, 5, 7), F), IDENT_ROW, intrinsics=K57, pyramid_iters=bad)
    # the other arguments are still checked on the pyramid path, and n_iters is not used there
    for kwargs in [dict(dist_max=0.0), dict(max_angle_deg=180.0), dict(max_jump=-0.1), dict(step=0.0), dict(pose_guess_w2c=np.zeros(11))]:
        with pytest.raises(ValueError):
            V.track(**{**dict(depth=depth, pose_guess_w2c=IDENT_ROW, intrinsics=K57, pyramid_iters=(2, 1)), **kwargs})
    with pytest.raises(AssertionError, match="the context was used"):      # valid: the first thing it does is use the device
        V.track(depth, IDENT_ROW, intrinsics=K57, pyramid_iters=(2, 1), n_iters=-5)
    # depth_half
    for bad in [dict(depth=depth.astype(np.float64)), dict(depth=depth[0]), dict(depth=np.ones((1, 7), F)), dict(depth=np.ones((5, 1), F)),
                dict(max_jump=-1.0), dict(max_jump=np.nan), dict(max_jump="far")]:
        with pytest.raises(ValueError):
            tracking.depth_half(**{**dict(depth=depth, max_jump=0.05, ctx=ctx), **bad})
    V.handle = None   # (nothing to destroy)


def test_command_line_arguments():
    tool = importlib.import_module(PKG + ".other_tools.integrate_tsdf")
    base = ["--voxel-size", "4", "--trunc", "12"]
    assert tool.parse_args(base + ["--track"]).track_pyramid is None
    assert tool.parse_args(base + ["--track", "--track-pyramid", "10,5,4"]).track_pyramid == [10, 5, 4]
    for bad in (["--track-pyramid", "10,5,4"], ["--track", "--track-pyramid", "10,x"], ["--track", "--track-pyramid", "3,-1"],
                ["--track", "--track-pyramid", "1,1,1,1,1,1,1,1,1"], ["--track", "--track-pyramid", ""]):
        with pytest.raises(SystemExit):
            tool.parse_args(base + bad)


def test_library_argument_errors_without_device():
    """NULL handles are refused before any device is touched, and nothing is written to the host outputs"""
    L = importlib.import_module(PKG + "._lib")
    lib = L.load()
    out = C.c_void_p(0x1234)
    assert lib.r3d_camera_half(None, C.byref(out)) == L.ERR_INVALID
    assert out.value == 0x1234 and "NULL" in L.last_error()
    sentinel = np.full(4, 7.0, F)
    assert lib.r3d_depth_half(None, sentinel.ctypes.data, 1, 2, 2, 0.05, sentinel.ctypes.data) == L.ERR_INVALID
    assert np.all(sentinel == 7.0) and "NULL" in L.last_error()
    pose = IDENT_ROW.copy()
    got, info, rms = np.full(12, 7.0), np.full(4, 7.0), np.full(19, 7.0)
    cams = (C.c_void_p * 3)(None, None, None)
    iters = (C.c_int * 3)(10, 5, 4)
    inf = C.c_double(float("inf"))

    def call(vol=None, cams=cams, n_levels=3, iters=iters):
        return lib.r3d_tsdf_track_pyramid(vol, cams, n_levels, iters, None, L.DEPTH_F32, 1.0, pose.ctypes.data, 1.0, 0.05, 0.0, inf, 0.05, 0.5,
                                          -1.0, got.ctypes.data, info.ctypes.data, rms.ctypes.data)
    assert call() == L.ERR_INVALID and "NULL" in L.last_error()
    assert call(cams=None) == L.ERR_INVALID and "NULL" in L.last_error()
    assert call(iters=None) == L.ERR_INVALID and "NULL" in L.last_error()
    for n in (0, -1, 9):
        assert call(n_levels=n) == L.ERR_INVALID and "n_levels" in L.last_error()
    assert np.all(got == 7.0) and np.all(info == 7.0) and np.all(rms == 7.0)
