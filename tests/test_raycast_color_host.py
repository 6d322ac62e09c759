"""CPU: the ray-cast colour rule (include/r3d.h, "TSDF ray-cast colour") in its NumPy restatement (tests/raycast_color_ref.py)
against values worked out by hand on a one-cell volume -- what tests/test_gpu_raycast_color.py asserts of the device is asserted
of the specification here first -- plus the Python layer's checks, the library's NULL-argument errors and the command line's
usage error, none of which needs a GPU.  (The library's error for a volume without the colour plane needs a volume handle, hence
a device: tests/test_gpu_raycast_color.py has it.)"""
import ctypes as C
import importlib
import os
import subprocess
import sys

import numpy as np
import pytest

import raycast_color_ref as RCC
import raycast_ref as RC
import tsdf_color_ref as CREF
from helpers import PKG, ROOT

F = np.float32


def one_cell(means_z0, means_z1, n=2):
    """a 2 x 2 x 2 volume of unit voxels at the origin: tsdf +0.5 on the plane z = 0 and -0.5 on z = 1 (the surface lies half way),
    weight n, and the colour sums n * means_z0 / n * means_z1 on the two planes"""
    vol = CREF.ColorVolume((0.0, 0.0, 0.0), 1.0, (2, 2, 2), 1.0)
    vol.tsdf[0], vol.tsdf[1] = F(0.5), F(-0.5)
    vol.w[:] = F(n)
    vol.n[:] = n
    vol.sums[0], vol.sums[1] = np.array(means_z0, np.uint32) * n, np.array(means_z1, np.uint32) * n
    return vol


def cell0(f):
    """cell (0, 0, 0) at the fractions f, as hit_cell returns them for one point"""
    return [np.zeros(1, np.int64)] * 3, [np.array([v], F) for v in f]


def test_means_interpolate_x_then_y_then_z():
    vol = one_cell((0, 0, 0), (0, 0, 0), n=1)
    # channel 0: the corner number k = jx + 2 jy + 4 jz times 8; channel 1: 100 at corner 1 only; channel 2: 255 everywhere
    for k in range(8):
        vol.sums[k >> 2, (k >> 1) & 1, k & 1] = (8 * k, 100 if k == 1 else 0, 255)
    got = RCC.cell_colors(vol.sums, vol.n, *cell0((0.25, 0.5, 0.75)))
    # channel 0 is linear in the corner index: 8 (fx + 2 fy + 4 fz) = 8 (0.25 + 1 + 3) = 34, every step exact in f32
    # channel 1: c[0][0] = 0 + 0.25 * 100 = 25; b[0] = 25 + 0.5 * (0 - 25) = 12.5; m = 12.5 + 0.75 * (0 - 12.5) = 3.125 -> 3
    assert got.tolist() == [[34, 3, 255]] and got.dtype == np.uint8
    assert RCC.cell_colors(vol.sums, vol.n, *cell0((0.0, 0.0, 0.0))).tolist() == [[0, 0, 255]]
    assert RCC.cell_colors(vol.sums, vol.n, *cell0((0.5, 0.0, 0.0))).tolist() == [[4, 50, 255]]
    assert RCC.cell_colors(vol.sums, vol.n, *cell0((0.0, 0.5, 0.0))).tolist() == [[8, 0, 255]]      # y: corners 0 and 2
    assert RCC.cell_colors(vol.sums, vol.n, *cell0((0.0, 0.0, 0.5))).tolist() == [[16, 0, 255]]     # z: corners 0 and 4


def test_half_rounds_up_empty_corner_counts_as_zero_and_both_clamps():
    vol = one_cell((0, 0, 0), (0, 0, 0), n=2)
    vol.sums[0, 0, 0], vol.sums[0, 0, 1] = (20, 20, 2000), (26, 99, 2000)     # corners 0 and 1: means (10, 10, 1000), (13, 49.5, 1000)
    half = cell0((0.5, 0.0, 0.0))
    # 10 + 0.5 * 3 = 11.5 -> 12 (half up); 10 + 0.5 * 39.5 = 29.75 -> 30; 1000 -> clamped to 255
    assert RCC.cell_colors(vol.sums, vol.n, *half).tolist() == [[12, 30, 255]]
    vol.n[0, 0, 1] = 0                                                         # corner 1 was never touched: its mean is 0, not 26 / 0
    # 10 + 0.5 * (0 - 10) = 5; the same; 1000 + 0.5 * (0 - 1000) = 500 -> 255
    assert RCC.cell_colors(vol.sums, vol.n, *half).tolist() == [[5, 5, 255]]
    vol.n[0, 0, 1] = 3                                                         # 26 / 3 rounds in f32: the quotient is one rounding
    m = F(10) + F(0.5) * (F(26) / F(3) - F(10))
    assert RCC.cell_colors(vol.sums, vol.n, *half)[0, 0] == int(np.floor(m + F(0.5))) == 9
    # the lower clamp: no fraction in [0, 1) reaches it from sums >= 0; the rule clamps all the same.  10 - 0.5 * 3 = 8.5 -> 9,
    # 10 - 2 * 39.5 = -69 -> 0
    vol.n[0, 0, 1] = 2
    assert RCC.cell_colors(vol.sums, vol.n, *cell0((-0.5, 0.0, 0.0)))[0, 0] == 9
    assert RCC.cell_colors(vol.sums, vol.n, *cell0((-2.0, 0.0, 0.0))).tolist() == [[4, 0, 255]]


ONE_CELL_K = (8.0, 8.0, 2.0, 2.0)                   # a 5 x 5 raster whose pixel (2, 2) looks straight down +z
ONE_CELL_POSE = np.concatenate([np.eye(3).reshape(9), [-1.0, -1.0, 2.0]])     # the camera at (1, 1, -2)


def test_reference_on_one_cell_by_hand():
    """The central ray: C = (1, 1, -2), dw = (0, 0, 1) exactly.  The z slab is [0.5, 1.5], so tmin = 2.5; with step 0.5 sample 0
    sits on the plane z = 0 (S = 0.5) and sample 1 half way (S = 0): r = 1, t* = 3, and the hit-point sample has f = (0.5, 0.5,
    0.5) in cell (0, 0, 0).  Every interpolation is then a midpoint: m = (mean_z0 + mean_z1) / 2."""
    vol = one_cell((10, 20, 31), (20, 41, 32))
    depth, vertex, normal, rgb, hit = RCC.cast_view(vol, ONE_CELL_POSE, ONE_CELL_K, (5, 5), step=0.5)
    assert hit[2, 2] and depth[2, 2] == F(3.0) and vertex[2, 2].tolist() == [1.0, 1.0, 1.0] and normal[2, 2].tolist() == [0.0, 0.0, -1.0]
    assert rgb.dtype == np.uint8 and rgb[2, 2].tolist() == [15, 31, 32]           # 15, 30.5 -> 31, 31.5 -> 32
    assert hit.any() and (~hit).any()
    assert not rgb[~hit].any() and not depth[~hit].any()                          # a miss: 0, 0, 0 with depth 0
    # the geometry is raycast_ref's, bit for bit, and the stacked form agrees with the single view
    d2, v2, n2, h2 = RC.cast_view(vol, ONE_CELL_POSE, ONE_CELL_K, (5, 5), step=0.5)
    assert np.array_equal(h2, hit)
    for a, b in ((depth, d2), (vertex, v2), (normal, n2)):
        assert np.array_equal(a.view(np.uint32), b.view(np.uint32))
    both = RCC.raycast(vol, np.stack([ONE_CELL_POSE, ONE_CELL_POSE]), ONE_CELL_K, (5, 5), step=0.5)
    assert both[3].shape == (2, 5, 5, 3) and np.array_equal(both[3][0], rgb) and np.array_equal(both[3][1], rgb)
    assert [a.shape for a in RCC.raycast(vol, np.zeros((0, 12)), ONE_CELL_K, (5, 5))] == [(0, 5, 5), (0, 5, 5, 3), (0, 5, 5, 3), (0, 5, 5, 3)]
    # a plane of one colour returns it on every hit, whatever the fractions
    flat = one_cell((200, 30, 90), (200, 30, 90), n=7)
    rgb = RCC.cast_view(flat, ONE_CELL_POSE, ONE_CELL_K, (5, 5), step=0.5)[3]
    assert (rgb[hit] == np.array((200, 30, 90), np.uint8)).all() and hit.sum() > 1


# ---- the Python layer, the library and the command line without a device ------------------------------------------------------------
class _NoDevice:
    """stands where a context would: any use of it is a failure of "ValueError before any device use" """

    def __getattr__(self, name):
        raise AssertionError("the context was used (%s) before the arguments were checked" % name)


def _unbound_volume(color):
    tsdf = importlib.import_module(PKG + ".tsdf")
    V = tsdf.TSDFVolume.__new__(tsdf.TSDFVolume)
    V.ctx, V.handle, V.color, V.voxel_size, V.sdf_trunc, V.dims = _NoDevice(), None, color, 0.05, 0.2, (4, 4, 4)
    return V


def test_python_layer_refuses_colour_from_a_plain_volume_before_any_device_use():
    plain = _unbound_volume(False)
    q, t = [[0.0, 0.0, 0.0, 1.0]], [[0.0, 0.0, 0.0]]
    with pytest.raises(ValueError, match="without colour"):
        plain.raycast(q, t, (5, 7), with_colors=True)
    with pytest.raises(ValueError, match="without colour"):
        plain.raycast_device(None, 1, np.zeros((1, 12)), None, None, None, d_rgb=1 << 20)
    # a volume with colour checks the other arguments as before, still without a device
    coloured = _unbound_volume(True)
    for kw in (dict(step=0.0), dict(t_near=-1.0), dict(min_weight=0.0)):
        with pytest.raises(ValueError):
            coloured.raycast(q, t, (5, 7), with_colors=True, **kw)
    with pytest.raises(ValueError):
        coloured.raycast(q, t, (0, 7), with_colors=True)
    with pytest.raises(ValueError):
        coloured.raycast_device(None, 2, np.zeros((1, 12)), None, None, None, d_rgb=1 << 20)
    for V in (plain, coloured):
        V.handle = None   # (nothing to destroy)
    import inspect
    tsdf = importlib.import_module(PKG + ".tsdf")
    assert list(inspect.signature(tsdf.TSDFVolume.raycast_device).parameters)[-1] == "d_rgb"      # the new keywords come last
    assert list(inspect.signature(tsdf.TSDFVolume.raycast).parameters)[-1] == "with_colors"
    assert inspect.signature(tsdf.TSDFVolume.raycast).parameters["with_colors"].default is False


def test_library_argument_errors_without_device():
    """NULL handles are refused before any device is touched, and nothing is written"""
    L = importlib.import_module(PKG + "._lib")
    lib = L.load()
    assert "r3d_tsdf_raycast_rgb" in L.SIGNATURES and "int r3d_tsdf_raycast_rgb(" in open(os.path.join(ROOT, "include", "r3d.h")).read()
    pose = np.concatenate([np.eye(3).reshape(9), np.zeros(3)])
    out = np.full(64, 7, np.uint8)
    inf = C.c_double(float("inf"))
    assert lib.r3d_tsdf_raycast_rgb(None, None, 1, pose.ctypes.data, 1.0, 0.05, 0.0, inf, None, None, None, out.ctypes.data) == L.ERR_INVALID
    assert "NULL" in L.last_error()
    assert lib.r3d_tsdf_raycast_rgb(None, None, 0, None, 1.0, 0.05, 0.0, inf, None, None, None, None) == L.ERR_INVALID
    assert np.all(out == 7)
    assert lib.r3d_version() == 200


def test_command_line_wants_the_colour_directory():
    tool = os.path.join(ROOT, PKG, "other_tools", "integrate_tsdf.py")
    env = dict(os.environ, PYTHONPATH=ROOT)
    r = subprocess.run([sys.executable, tool, "--voxel-size", "8", "--trunc", "24", "--raycast-color"], env=env, capture_output=True,
                       text=True, timeout=120)
    assert r.returncode == 2 and "usage:" in r.stderr and "--color-dir" in r.stderr and "Traceback" not in r.stderr, r.stderr[-500:]
    r = subprocess.run([sys.executable, tool, "--help"], env=env, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "--raycast-color" in r.stdout
