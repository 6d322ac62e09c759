"""CPU: the parts of normal estimation that need no GPU -- argument errors raised before any GPU work, the C entry point's own
argument checks, tests/normals_ref.py against closed-form cases, the PLY layout with normals, the command line's --help and
argument errors."""
import ctypes as C
import importlib
import os
import subprocess
import sys

import numpy as np
import pytest

import normals_ref as REF
from helpers import PKG, ROOT, r3d as _r3d

TOOL = os.path.join(ROOT, PKG, "other_tools", "estimate_normals.py")


@pytest.fixture(scope="module")
def R():
    return _r3d()


@pytest.fixture(scope="module")
def NM(R):
    return importlib.import_module(PKG + ".normals")


def brute_lists(xyz, k):
    x = xyz.astype(np.float64)
    d = ((x[:, None, :] - x[None, :, :]) ** 2).sum(-1)
    np.fill_diagonal(d, np.inf)
    o = np.argsort(d, axis=1, kind="stable")[:, :k]
    return o.astype(np.uint32), np.take_along_axis(d, o, axis=1).astype(np.float32)


def test_exported_names(R, NM):
    for name in ("Normals", "estimate_normals", "estimate_normals_device", "estimate_covariances", "fused_viewpoints"):
        assert getattr(R, name) is getattr(NM, name)
    assert NM.Normals._fields == ("normals", "curvature", "count")
    assert hasattr(R.cloud_io, "write_ply_normals") and hasattr(R.cloud_io, "read_ply_normals")


@pytest.mark.parametrize("kwargs", [
    dict(k=2), dict(k=33), dict(k=8.0), dict(k=True), dict(k="8"), dict(radius=0.0), dict(radius=-1.0), dict(radius=float("nan")),
    dict(radius=float("inf")), dict(radius="near"), dict(viewpoint=(0, 0)), dict(viewpoint=(0, 0, float("nan"))),
    dict(viewpoint=(0, 0, 0), viewpoints=np.zeros((2, 3)), points_per_view=4), dict(viewpoints=np.zeros((2, 3))),
    dict(viewpoints=np.zeros((2, 3)), points_per_view=0), dict(viewpoints=np.zeros((2, 2)), points_per_view=4),
    dict(viewpoints=np.zeros((0, 3)), points_per_view=4), dict(viewpoints=np.full((2, 3), np.inf), points_per_view=4),
    dict(points_per_view=4), dict(viewpoint=(0, 0, 0), points_per_view=4), dict(viewpoints=np.zeros((2, 3)), points_per_view=2.5)])
def test_argument_errors_before_any_gpu_work(NM, kwargs):
    xyz = np.zeros((10, 3), np.float32)
    with pytest.raises(ValueError):
        NM.estimate_normals(xyz, **kwargs)
    if set(kwargs) <= {"k", "radius"}:
        with pytest.raises(ValueError):
            NM.estimate_covariances(xyz, kwargs.get("k", 8), kwargs.get("radius"))


def test_cloud_shape_errors(NM):
    for bad in (np.zeros((10, 2)), np.zeros(9), np.zeros((2, 3, 3))):
        with pytest.raises(ValueError):
            NM.estimate_normals(bad)
        with pytest.raises(ValueError):
            NM.estimate_covariances(bad, 8)


def test_c_entry_point_rejects_a_null_index(R):
    L = importlib.import_module(PKG + "._lib")
    lib = R.load_library()
    assert "r3d_normals_knn" in L.SIGNATURES
    assert lib.r3d_normals_knn(None, 8, 0.0, None, 0, 1, None, None, None, None) == L.ERR_INVALID
    assert "index" in L.last_error()


def test_fused_viewpoints_are_the_camera_centres(R, NM):
    syn = importlib.import_module(PKG + ".synthetic")
    _, q, t, _ = syn.room_views(5, 8, 8, seed=1)
    got = NM.fused_viewpoints(q, t)
    assert got.shape == (5, 3) and got.dtype == np.float64
    for f in range(5):
        T = syn.pose_matrix(q[f], t[f])                                            # world -> camera
        assert np.abs(T[:3, :3] @ got[f] + T[:3, 3]).max() <= 1e-12                # the centre maps to the camera origin
        assert np.abs(got[f] - R.pose_to_T(R.pose_table(q[f:f + 1], t[f:f + 1])[0, :9].reshape(3, 3), t[f])[:3, 3]).max() <= 1e-15


def test_reference_on_a_plane_and_a_line():
    g = np.stack(np.meshgrid(np.arange(12), np.arange(12), indexing="ij"), -1).reshape(-1, 2) / 16.0
    xyz = np.concatenate([g, 0.25 * g[:, :1] + 0.5 * g[:, 1:]], axis=1).astype(np.float32)
    idx, d2 = brute_lists(xyz, 8)
    r = REF.normals(xyz, idx, d2)
    n0 = np.array([0.25, 0.5, -1.0]) / np.linalg.norm([0.25, 0.5, -1.0])
    assert r.plane.all() and (r.count == 8).all()
    assert np.linalg.norm(np.cross(r.n, n0), axis=1).max() <= 1e-12 and np.abs(r.curvature).max() <= 1e-12
    up = REF.orient(r.n, xyz)
    assert (up[:, 2] > 0).all()                                                     # the largest component, z, made positive
    seen = REF.orient(r.n, xyz, viewpoints=[[0.3, 0.3, -5.0]])
    assert (seen[:, 2] < 0).all() and np.array_equal(seen, -up)
    per = REF.orient(r.n, xyz, viewpoints=[[0.3, 0.3, 5.0], [0.3, 0.3, -5.0]], points_per_view=100)
    assert (per[:100, 2] > 0).all() and (per[100:, 2] < 0).all()
    # points on one line: no plane, zero rows
    line = np.stack([np.arange(20) / 8.0] * 3, axis=1).astype(np.float32) * np.float32([1, 2, 4])
    idx, d2 = brute_lists(line, 4)
    r = REF.normals(line, idx, d2)
    assert (r.line | ~r.plane).all()


def test_reference_covariance_by_hand_radius_and_tails():
    xyz = np.float32([[0, 0, 0], [1, 0, 0], [0, 2, 0], [0, 0, 4], [np.nan, 0, 0]])
    idx = np.uint32([[1, 2, 3], [0, 2, 3], [0, 1, 3], [0, 1, 2], [0xffffffff] * 3])
    d2 = np.float32([[1, 4, 16], [1, 5, 17], [4, 5, 20], [16, 17, 20], [np.inf] * 3])
    count, Cv = REF.raw_covariance(xyz, idx, d2)
    assert count.tolist() == [3, 3, 3, 3, 0]
    # point 0: e = (1,0,0), (0,2,0), (0,0,4); m = 4: C_xx = (1 - 1/4)/4, C_xy = (0 - 1*2/4)/4, ...
    assert np.array_equal(Cv[0], [(1 - 0.25) / 4, (0 - 0.5) / 4, (0 - 1.0) / 4, (4 - 1.0) / 4, (0 - 2.0) / 4, (16 - 4.0) / 4])
    count, Cv = REF.raw_covariance(xyz, idx, d2, radius=2.0)                        # d2 <= 4 stays
    assert count.tolist() == [2, 1, 1, 0, 0]
    assert np.array_equal(Cv[0], [(1 - 1 / 3) / 3, (0 - 2 / 3) / 3, 0, (4 - 4 / 3) / 3, 0, 0])
    r = REF.normals(xyz, idx, d2, radius=2.0)
    assert r.plane.tolist() == [True, False, False, False, False] and (r.cov[1:] == 0).all() and (r.n[1:] == 0).all()
    assert abs(abs(r.n[0, 2]) - 1.0) <= 1e-15                                        # three points in z = 0


def test_ply_with_normals_round_trip_and_layout(R, tmp_path):
    rng = np.random.default_rng(3)
    xyz, nrm = rng.normal(size=(37, 3)).astype(np.float32), rng.normal(size=(37, 3)).astype(np.float32)
    nrm[5] = 0
    xyz[6, 1] = np.nan
    rgb = rng.integers(0, 256, (37, 3), dtype=np.uint8)
    p = str(tmp_path / "a.ply")
    R.cloud_io.write_ply_normals(p, xyz, nrm)
    raw = open(p, "rb").read()
    head = (b"ply\nformat binary_little_endian 1.0\nelement vertex 37\nproperty float x\nproperty float y\nproperty float z\n"
            b"property float nx\nproperty float ny\nproperty float nz\nend_header\n")
    assert raw.startswith(head) and len(raw) == len(head) + 37 * 24
    assert raw[len(head):] == np.concatenate([xyz, nrm], axis=1).astype("<f4").tobytes()
    a, b = R.cloud_io.read_ply_normals(p)
    assert np.array_equal(a.view(np.uint32), xyz.view(np.uint32)) and np.array_equal(b.view(np.uint32), nrm.view(np.uint32))
    R.cloud_io.write_ply_normals(p, xyz, nrm, rgb=rgb)
    raw = open(p, "rb").read()
    assert b"property uchar red\nproperty uchar green\nproperty uchar blue\nend_header\n" in raw
    body = raw[raw.index(b"end_header\n") + 11:]
    assert len(body) == 37 * 27 and body[24:27] == rgb[0].tobytes()
    a, b = R.cloud_io.read_ply_normals(p)
    assert np.array_equal(a.view(np.uint32), xyz.view(np.uint32)) and np.array_equal(b.view(np.uint32), nrm.view(np.uint32))
    R.cloud_io.write_ply_normals(p, np.zeros((0, 3)), np.zeros((0, 3)))
    a, b = R.cloud_io.read_ply_normals(p)
    assert a.shape == (0, 3) and b.shape == (0, 3)
    for bad in (dict(xyz=xyz, normals=nrm[:5]), dict(xyz=xyz[:, :2], normals=nrm), dict(xyz=xyz, normals=nrm, rgb=rgb[:4])):
        with pytest.raises(ValueError):
            R.cloud_io.write_ply_normals(p, **bad)
    # the existing binary layout has no normals: the new reader says so, the old reader is unchanged
    R.cloud_io.write_ply_binary(p, xyz)
    with pytest.raises(ValueError):
        R.cloud_io.read_ply_normals(p)
    assert R.cloud_io.read_ply(p).shape == (37, 3)
    R.cloud_io.write_ply(p, xyz[:5])
    with pytest.raises(ValueError):
        R.cloud_io.read_ply_normals(p)


def run_tool(*args):
    return subprocess.run([sys.executable, TOOL] + list(args), capture_output=True, text=True, timeout=120)


def test_command_line_help_and_argument_errors(R, tmp_path):
    r = run_tool("--help")
    assert r.returncode == 0 and "--k" in r.stdout and "--radius" in r.stdout and "--viewpoint" in r.stdout
    src = str(tmp_path / "in.ply")
    R.cloud_io.write_ply_binary(src, np.zeros((4, 3), np.float32))
    out = str(tmp_path / "out.ply")
    for args, text in (([src, out], "--k"), ([src, out, "--k", "2"], "K must be in [3, 32]"), ([src, out, "--k", "33"], "K must be in"),
                       ([src, out, "--k", "x"], "K must be an integer"), ([src, out, "--k", "8", "--radius", "0"], "R must be finite and positive"),
                       ([src, out, "--k", "8", "--radius", "nan"], "R must be"), ([src, out, "--k", "8", "--radius", "r"], "R must be a number"),
                       ([src, out, "--k", "8", "--viewpoint", "0", "0"], "--viewpoint"),
                       ([src, out, "--k", "8", "--viewpoint", "0", "0", "inf"], "X Y Z must be finite"),
                       ([str(tmp_path / "missing.ply"), out, "--k", "8"], "does not exist")):
        r = run_tool(*args)
        assert r.returncode == 2 and text in r.stderr, (args, r.stderr[-300:])
        assert not os.path.exists(out)
