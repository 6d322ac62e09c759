"""GPU: the command-line tools of the depth consistency filter on the golden working directory scene3 --
other_tools/fuse_consistent.py writes the PLY of fuse_frames_consistent's cloud and prints its counts, and
other_tools/integrate_tsdf.py --consistency integrates the filtered rasters instead of the raw ones."""
import os
import shutil
import subprocess
import sys

import numpy as np
import pytest

from helpers import PKG, ROOT, r3d as _r3d

pytestmark = pytest.mark.gpu

K = (20.0, 20.0, 15.5, 11.5)
ENV = dict(R3D_FX="20", R3D_FY="20", R3D_CX="15.5", R3D_CY="11.5")
RULE = dict(radius=2, rel_tol=0.1, min_consistent=1, max_violations=3)


@pytest.fixture(scope="module")
def R():
    return _r3d()


@pytest.fixture
def work(golden_dir, tmp_path):
    w = tmp_path / "work"
    shutil.copytree(os.path.join(golden_dir, "scene3", "depth"), w / "depth")
    shutil.copytree(os.path.join(golden_dir, "scene3", "camera_pose"), w / "camera_pose")
    return w


def inputs(R, work):
    names, quats, ts = R.read_pose_file(str(work / "camera_pose" / "image_colmap_simi_2.txt"))
    return R.cloud_io.read_depth_batch([str(work / "depth" / n) for n in names]), quats, ts


def run(tool, args, work):
    r = subprocess.run([sys.executable, os.path.join(ROOT, PKG, "other_tools", tool)] + args, cwd=str(work),
                       env=dict(os.environ, PYTHONPATH=ROOT, **ENV), capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-1000:] + r.stderr[-2000:]
    return r.stdout.split("\n")


def test_fuse_consistent_tool(R, work):
    depths, quats, ts = inputs(R, work)
    xyz, keep = R.fuse_frames_consistent(depths, quats, ts, K, **RULE)
    assert 0 < len(xyz) < keep.size
    lines = run("fuse_consistent.py", ["--radius", "2", "--rel-tol", "0.1", "--min-consistent", "1", "--max-violations", "3"], work)
    assert "frames 3 pixels %d kept %d dropped %d -> ./ply/fused_consistent.ply" % (keep.size, len(xyz), keep.size - len(xyz)) in lines
    assert open(str(work / "ply" / "fused_consistent.ply"), "rb").read() == R.cloud_io.format_ply(xyz)
    bad = subprocess.run([sys.executable, os.path.join(ROOT, PKG, "other_tools", "fuse_consistent.py"), "--radius", "9"], cwd=str(work),
                         env=dict(os.environ, PYTHONPATH=ROOT), capture_output=True, text=True, timeout=300)
    assert bad.returncode == 2 and "radius" in bad.stderr


def test_integrate_tsdf_consistency_flag(R, work):
    depths, quats, ts = inputs(R, work)
    keep, filtered = R.depth_consistency(depths, quats, ts, K, **RULE)[2:]
    V = R.TSDFVolume((-300.0, -300.0, -300.0), 8.0, (75, 75, 75), 24.0)
    try:
        V.integrate(filtered, quats, ts, intrinsics=K)
        want_xyz, want_nrm = V.extract_point_cloud(1.0)
        V.reset()
        V.integrate(depths, quats, ts, intrinsics=K)
        raw_xyz = V.extract_point_cloud(1.0)[0]
    finally:
        V.close()
    assert 0 < len(want_xyz) < len(raw_xyz)                      # the filter changes what is integrated
    args = ["--voxel-size", "8", "--trunc", "24", "--origin", "-300", "-300", "-300", "--dims", "75", "75", "75", "--consistency", "2,0.1,1,3"]
    lines = run("integrate_tsdf.py", args, work)
    assert "consistency kept %d of %d pixels" % (int(keep.sum()), keep.size) in lines
    xyz, nrm = R.cloud_io.read_ply_normals(str(work / "ply" / "tsdf_surface.ply"))
    assert np.array_equal(xyz.view(np.uint32), want_xyz.view(np.uint32)) and np.array_equal(nrm.view(np.uint32), want_nrm.view(np.uint32))
