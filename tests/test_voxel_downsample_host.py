"""CPU: the voxel-grid downsampling wrappers (voxelmap.VoxelGrid / voxel_down_sample, r3d_voxelgrid_* and the
other_tools/voxel_down_sample.py command line) -- loud without a device, argument errors caught before any device work."""
import ctypes as C
import importlib
import os
import subprocess
import sys

import numpy as np
import pytest

from helpers import PKG, ROOT

TOOL = os.path.join(ROOT, PKG, "other_tools", "voxel_down_sample.py")


@pytest.fixture(scope="module")
def R():
    return importlib.import_module(PKG)


@pytest.fixture(scope="module")
def V(R):
    return importlib.import_module(PKG + ".voxelmap")


def gpu_visible(R):
    lib = R.load_library()
    n = C.c_int(0)
    return lib.r3d_device_count(C.byref(n)) == 0 and n.value > 0


def test_without_a_device_the_wrappers_raise(R, V):
    """No CPU fallback: without an MI355X both entry points raise R3DError.  (Where a GPU is visible the same calls must
    simply work: one voxel, the mean of its two points.)"""
    xyz = np.array([[0.01, 0.02, 0.03], [0.03, 0.04, 0.05]], np.float32)
    if gpu_visible(R):
        got = V.voxel_down_sample(xyz, 0.1)
        assert got.counts.tolist() == [2] and np.allclose(got.xyz, [[0.02, 0.03, 0.04]], atol=1e-7)
        return
    with pytest.raises(R.R3DError):
        V.voxel_down_sample(xyz, 0.1)
    with pytest.raises(R.R3DError):
        V.VoxelGrid(0.1)
    assert R.VoxelGrid is V.VoxelGrid and R.voxel_down_sample is V.voxel_down_sample


@pytest.mark.parametrize("xyz,size,rgba", [
    (np.zeros((4, 2), np.float32), 0.1, None),                           # not [N,3]
    (np.zeros(12, np.float32), 0.1, None),
    (np.zeros((4, 3), np.float32), 0.0, None),                           # voxel size
    (np.zeros((4, 3), np.float32), -0.5, None),
    (np.zeros((4, 3), np.float32), float("nan"), None),
    (np.zeros((4, 3), np.float32), 0.1, np.zeros(3, np.uint32)),         # one colour word per point
    (np.zeros((4, 3), np.float32), 0.1, np.zeros((4, 3), np.uint8)),     # words, not [N,3] bytes
    (np.zeros((4, 3), np.float32), 0.1, np.zeros(4, np.float32)),
])
def test_argument_errors_before_device_work(V, xyz, size, rgba):
    with pytest.raises(ValueError):
        V.voxel_down_sample(xyz, size, rgba)


def test_grid_argument_errors(R, V):
    with pytest.raises(ValueError):
        V.VoxelGrid(0.0)
    with pytest.raises(ValueError):
        V.VoxelGrid(0.1, capacity=-1)
    L = importlib.import_module(PKG + "._lib")
    lib = L.load()
    h, n = C.c_void_p(), C.c_int64()
    assert lib.r3d_voxelgrid_create(None, 0.1, 1024, 0, C.byref(h)) == L.ERR_INVALID
    assert lib.r3d_voxelgrid_destroy(None) == 0
    assert lib.r3d_voxelgrid_clear(None) == L.ERR_INVALID
    assert lib.r3d_voxelgrid_insert(None, None, None, 0) == L.ERR_INVALID
    assert lib.r3d_voxelgrid_insert_host(None, None, None, 0) == L.ERR_INVALID
    assert lib.r3d_voxelgrid_stats(None, None, None, None) == L.ERR_INVALID
    assert lib.r3d_voxelgrid_extract(None, None, None, None, None, 0, C.byref(n)) == L.ERR_INVALID
    assert "NULL" in L.last_error()


def run_tool(*args):
    return subprocess.run([sys.executable, TOOL] + list(args), capture_output=True, text=True, timeout=120)


def test_tool_help():
    r = run_tool("--help")
    assert r.returncode == 0
    assert "usage:" in r.stdout and "--voxel-size" in r.stdout and "--binary" in r.stdout


@pytest.mark.parametrize("args,message", [
    ([], "the following arguments are required"),
    (["only_one.ply"], "the following arguments are required"),
    (["in.ply", "out.ply", "--voxel-size", "0"], "--voxel-size must be positive"),
    (["in.ply", "out.ply", "--voxel-size", "abc"], "invalid float value"),
    (["does_not_exist.ply", "out.ply"], "does not exist"),
])
def test_tool_argument_errors(tmp_path, args, message):
    cwd = os.getcwd()
    os.chdir(tmp_path)
    try:
        if args and args[0] == "in.ply":
            (tmp_path / "in.ply").write_text("ply\nformat ascii 1.0\nelement vertex 0\nend_header\n")
        r = run_tool(*args)
    finally:
        os.chdir(cwd)
    assert r.returncode == 2
    assert message in r.stderr
    assert not (tmp_path / "out.ply").exists()
