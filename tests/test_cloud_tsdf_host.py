"""CPU: the cloud -> TSDF restatement (tests/cloud_tsdf_ref.py) -- whether the nearest-tangent-plane rule is good enough to mesh from,
measured on the Fibonacci sphere --, the geometry of surface.volume_for_cloud, and what the library, the header and the tool say
without a GPU."""
import ctypes as C
import importlib
import os
import re

import numpy as np
import pytest

import cloud_tsdf_ref as CT
from helpers import PKG, ROOT

# RMS radial error of the zero crossings of the sphere case (N = 1000, R = 1, true normals, 24^3, vs = 0.1): the restatement gives
# 8.3604e-4 with a truncation of 4 voxels and of 3 alike (the crossings lie within one voxel of the surface, inside either band);
# the bound is 1.5 x that: it is there to catch a broken rule, not rounding.
RMS_RESTATEMENT = 8.3604e-4
RMS_BOUND = 1.5 * RMS_RESTATEMENT
_SPHERE = {}


def sphere_volume(trunc_voxels):
    """(vol [n,2], touched, case) of the sphere case through the restatement, computed once per session"""
    if trunc_voxels not in _SPHERE:
        case = CT.sphere_case(trunc_voxels=trunc_voxels)
        origin, vs, dims, tr, xyz, normals = case
        vol, touched = CT.integrate_cloud(np.zeros((dims[0] * dims[1] * dims[2], 2), np.float32), origin, vs, dims, tr, xyz, normals)
        _SPHERE[trunc_voxels] = (vol, touched, case)
    return _SPHERE[trunc_voxels]


def radial_rms(points, radius=1.0):
    e = np.linalg.norm(np.asarray(points, np.float64), axis=1) - radius
    return float(np.sqrt(np.mean(e * e))), float(np.abs(e).max())


@pytest.mark.parametrize("trunc_voxels", [4, 3])
def test_rule_reconstructs_the_sphere(trunc_voxels):
    vol, touched, (origin, vs, dims, tr, xyz, normals) = sphere_volume(trunc_voxels)
    pts = CT.zero_crossings(vol, origin, vs, dims)
    rms, worst = radial_rms(pts)
    cells = CT.cells_crossing_sphere(origin, vs, dims)
    open_cells = CT.cells_with_invalid_corner(vol, dims, cells)
    print("trunc %d voxels: %d voxels touched, %d crossings, rms %.4e max %.4e (bound %.4e); %d cells cross the sphere, %d lack a corner"
          % (trunc_voxels, touched, len(pts), rms, worst, RMS_BOUND, len(cells), open_cells))
    assert len(pts) > 1000 and rms <= RMS_BOUND
    assert len(cells) == 1898 and open_cells == 0          # marching cubes closes the surface
    w = vol[:, 1]
    assert set(np.unique(w)) == {0.0, 1.0} and touched == int(w.sum()) and (np.abs(vol[:, 0]) <= 1).all()
    assert (vol[w == 0] == 0).all()                        # a skipped voxel keeps every bit


def test_restatement_properties():
    """the rule's edges on the restatement itself: what the GPU tests then demand bit for bit"""
    o, vs, dims, tr = (0.0, 0.0, 0.0), 0.125, (8, 1, 1), 0.5
    cx = CT.centres(o, vs, dims)[0]
    zero = np.zeros((8, 2), np.float32)
    up = np.array([[1.0, 0.0, 0.0]], np.float32)

    def run(p, n=up, vol=zero):
        return CT.integrate_cloud(vol, o, vs, dims, tr, np.asarray(p, np.float32).reshape(-1, 3), np.asarray(n, np.float32).reshape(-1, 3))

    # a point exactly tr from the centre of voxel 0, along x: inside; the next representable distance: outside
    y = z = np.float32(0.0625)
    at = np.float32(cx[0] + np.float32(0.5))
    vol, touched = run([[at, y, z]])
    assert vol[0, 1] == 1 and vol[0, 0] == -1 and touched == int(vol[:, 1].sum())
    vol, _ = run([[np.nextafter(at, np.float32(2)), y, z]])
    assert vol[0, 1] == 0
    # ties: the lowest index wins, so swapping two equidistant points with different normals changes the sign
    a, b = [cx[3] - np.float32(0.25), y, z], [cx[3] + np.float32(0.25), y, z]
    va, _ = run([a, b], [[1, 0, 0], [-1, 0, 0]])
    vb, _ = run([b, a], [[-1, 0, 0], [1, 0, 0]])
    assert va[3, 0] == np.float32(0.5) and vb[3, 0] == np.float32(0.5)      # a at s = +0.25, b (normal -x) at s = +0.25 as well
    va, _ = run([a, b], [[1, 0, 0], [1, 0, 0]])
    vb, _ = run([b, a], [[1, 0, 0], [1, 0, 0]])
    assert va[3, 0] == np.float32(0.5) and vb[3, 0] == np.float32(-0.5)
    # the winner's normal decides: zero or NaN -> skipped, not handed to the runner-up; non-finite rows never win
    v0, _ = run([[cx[3], y, z], [cx[3] + np.float32(0.01), y, z]], [[0, 0, 0], [1, 0, 0]])
    assert v0[3, 1] == 0 and v0[4, 1] == 1
    v0, _ = run([[cx[3], y, z], [cx[3] + np.float32(0.01), y, z]], [[np.nan, 0, 1], [1, 0, 0]])
    assert v0[3, 1] == 0
    v0, _ = run([[np.nan, y, z], [np.inf, y, z], [cx[3], y, z]], [[1, 0, 0]] * 3)
    assert v0[3, 1] == 1 and v0[3, 0] == 0
    # non-unit normals clamp at +-1; composition is the running average
    v0, _ = run([[cx[3], y, z]], [[100, 0, 0]])
    assert v0[4, 0] == 1 and v0[2, 0] == -1 and v0[3, 0] == 0
    v1, _ = run([[cx[3], y, z]])
    v2, _ = run([[cx[3], y, z]], vol=v1)
    assert np.array_equal(v2[:, 0], v1[:, 0]) and np.array_equal(v2[:, 1], 2 * v1[:, 1])
    assert np.array_equal(zero, np.zeros((8, 2), np.float32))                # the inputs are not modified


def test_volume_for_cloud_geometry():
    S = importlib.import_module(PKG + ".surface")
    xyz, _ = CT.fibonacci_sphere(1000)
    origin, dims, trunc = S.cloud_volume_geometry(xyz, 0.1, 4, margin_voxels=2)
    assert dims == (24, 24, 24) and np.allclose(origin, -1.2) and trunc == pytest.approx(0.4)
    origin, dims, trunc = S.cloud_volume_geometry(xyz, 0.1)                  # the default margin is the truncation
    assert dims == (28, 28, 28) and np.allclose(origin, -1.4)
    pts = np.array([[0.05, 1.0, -0.31], [0.26, 1.0, -0.3], [np.nan, 5, 5], [np.inf, 0, 0]], np.float32)
    origin, dims, trunc = S.cloud_volume_geometry(pts, 0.1, 3, margin_voxels=0)
    assert dims == (3, 1, 1) and np.allclose(origin, [0.0, 1.0, -0.4]) and trunc == pytest.approx(0.3)
    lo, hi = origin, origin + np.array(dims) * 0.1
    finite = pts[:2].astype(np.float64)
    assert (finite >= lo - 1e-6).all() and (finite < hi + 1e-6).all()        # every finite point is inside
    origin, dims, _ = S.cloud_volume_geometry(pts, 0.1, 3)
    assert dims == (9, 7, 7) and np.allclose(origin, [-0.3, 0.7, -0.7])
    for bad in (lambda: S.cloud_volume_geometry(np.full((2, 3), np.nan), 0.1), lambda: S.cloud_volume_geometry(np.zeros((0, 3)), 0.1),
                lambda: S.cloud_volume_geometry(pts, 0.0), lambda: S.cloud_volume_geometry(pts, 0.1, 0),
                lambda: S.cloud_volume_geometry(pts, 0.1, 2.5), lambda: S.cloud_volume_geometry(pts, 0.1, 4, -1),
                lambda: S.cloud_volume_geometry(pts[:, :2], 0.1), lambda: S.cloud_volume_geometry(pts, float("nan"))):
        with pytest.raises(ValueError):
            bad()
    far = np.array([[0, 0, 0], [1000, 1000, 1000]], np.float32)
    with pytest.raises(ValueError, match="more than mesh extraction takes"):
        S.cloud_volume_geometry(far, 1.0)                                    # 1009^3 > 2^32 / 5
    assert S.cloud_volume_geometry(far, 1.1)[1] == (918, 918, 918) and 918 ** 3 <= S.MAX_MESH_VOXELS < 951 ** 3
    assert 5 * S.MAX_MESH_VOXELS < 1 << 32 <= 5 * (S.MAX_MESH_VOXELS + 1)
    R = importlib.import_module(PKG)
    assert R.volume_for_cloud is S.volume_for_cloud and R.reconstruct_surface is S.reconstruct_surface


def test_header_exports_and_bindings():
    text = open(os.path.join(ROOT, "include", "r3d.h")).read()
    assert "/* ---- TSDF from an oriented cloud (csrc/r3d_tsdf_cloud.hip" in text
    flat = re.sub(r"\s+", " ", text)
    assert ("int r3d_tsdf_integrate_cloud(r3d_tsdf* vol, r3d_nn_index* index, const float* d_normals, const uint32_t* d_rgba, "
            "int64_t* n_touched_out);") in flat
    assert ("int r3d_tsdf_integrate_cloud_host(r3d_tsdf* vol, const float* h_xyz, const float* h_normals, const uint32_t* h_rgba, "
            "int64_t n, int64_t* n_touched_out);") in flat
    section = text[text.index("/* ---- TSDF from an oriented cloud"):text.index("int r3d_tsdf_integrate_cloud(")]
    section = re.sub(r"\s+", " ", re.sub(r"\n \*", " ", section))          # the comment's line breaks and their stars
    for phrase in ("fmaf(dz,dz, fmaf(dy,dy, dx*dx))", "lowest index wins", "d2 <= tr * tr", "fmaxf(-1.0f, fminf(1.0f, s / tr))",
                   "w1 = w + 1.0f", "ONE frame", "not handed to the runner-up", "keeps every bit", "brute force", "tsdf_cloud_chunk",
                   "running averages", "n_touched_out != NULL", "R3D_ERR_INVALID"):
        assert phrase in section, phrase
    L = importlib.import_module(PKG + "._lib")
    lib = L.load()
    for name in ("r3d_tsdf_integrate_cloud", "r3d_tsdf_integrate_cloud_host"):
        assert name in L.SIGNATURES and hasattr(lib, name)
    V = importlib.import_module(PKG + ".tsdf").TSDFVolume
    assert callable(V.integrate_cloud) and callable(V.integrate_cloud_device)
    csrc = os.path.join(ROOT, PKG, "csrc")
    assert "r3d_tsdf_cloud.hip" in open(os.path.join(csrc, "Makefile")).read()
    assert "kScratchSlots = 15" in open(os.path.join(csrc, "r3d_internal.h")).read()
    makefile = open(os.path.join(csrc, "Makefile")).read()
    assert "r3d_tsdf_cloud_host.cpp" in makefile
    kernels, host = open(os.path.join(csrc, "r3d_tsdf_cloud.hip")).read(), open(os.path.join(csrc, "r3d_tsdf_cloud_host.cpp")).read()
    assert "r3d_scratch(" not in kernels and "__global__" not in host              # kernels in one file, workspaces in the other
    assert set(re.findall(r"r3d_scratch\(\s*ctx,\s*(\w+)", host)) == {"kWsSpare", "kWsCounts"} and "r3d_nn_index_query(" in host
    assert "cloud_buf" in open(os.path.join(csrc, "r3d_tsdf.hip")).read()           # the volume's buffers go with r3d_tsdf_destroy


def test_argument_errors_without_gpu():
    L = importlib.import_module(PKG + "._lib")
    lib = L.load()
    fake = C.create_string_buffer(1024)                       # stands in for an object the checks must refuse before they use it
    p = C.addressof(fake)
    n = C.c_int64(-7)
    for args in ((None, p, p, None, C.byref(n)), (p, None, p, None, C.byref(n)), (p, p, None, None, C.byref(n))):
        assert lib.r3d_tsdf_integrate_cloud(*args) == L.ERR_INVALID, args
        assert L.last_error()
    for args in ((None, p, p, None, 3, C.byref(n)), (p, p, p, None, -1, C.byref(n)), (p, None, p, None, 3, C.byref(n)),
                 (p, p, None, None, 3, C.byref(n)), (p, p, p, None, 1 << 32, C.byref(n)),
                 (p, p, p, p, 3, C.byref(n))):              # colours for a volume without the plane (all zero bytes: no plane)
        assert lib.r3d_tsdf_integrate_cloud_host(*args) == L.ERR_INVALID, args
        assert L.last_error()
    assert n.value == -7 and not fake.raw.strip(b"\0")
    assert lib.r3d_tsdf_integrate_cloud_host(p, None, None, None, 0, C.byref(n)) == L.OK and n.value == 0    # an empty cloud
    assert not fake.raw.strip(b"\0")


def test_tool_arguments():
    tool = importlib.import_module(PKG + ".other_tools.reconstruct_surface")
    base = ["in.ply", "out.ply", "--voxel-size", "0.1"]
    args = tool.parse_args(base)
    assert (args.trunc_voxels, args.knn, args.viewpoint, args.mesh_smooth, args.mesh_largest) == (4, None, None, None, False)
    args = tool.parse_args(base + ["--trunc-voxels", "3", "--knn", "12", "--viewpoint", "0,1.5,-2", "--mesh-largest", "--mesh-smooth", "taubin,5"])
    assert (args.trunc_voxels, args.knn, args.viewpoint, args.mesh_largest) == (3, 12, [0.0, 1.5, -2.0], True)
    assert args.mesh_smooth["method"] == "taubin" and args.mesh_smooth["iterations"] == 5
    for extra in (["--knn", "12"], ["--knn", "2", "--viewpoint", "0,0,0"], ["--viewpoint", "0,0"], ["--viewpoint", "0,0,nan"],
                  ["--trunc-voxels", "0"], ["--voxel-size", "-1"], ["--mesh-smooth", "median,5"], ["--mesh-min-component", "0"]):
        with pytest.raises(SystemExit):
            tool.parse_args(base + extra)
    with pytest.raises(SystemExit):
        tool.parse_args(["in.ply", "out.ply"])


def test_tool_refuses_to_guess_an_orientation(tmp_path):
    """a PLY without normals and no --viewpoint: the tool stops before it touches a device"""
    R = importlib.import_module(PKG)
    tool = importlib.import_module(PKG + ".other_tools.reconstruct_surface")
    xyz, normals = CT.fibonacci_sphere(50)
    plain, oriented = str(tmp_path / "plain.ply"), str(tmp_path / "oriented.ply")
    R.cloud_io.write_ply_binary(plain, xyz)
    with pytest.raises(SystemExit, match="cannot be guessed"):
        tool.main([plain, str(tmp_path / "out.ply"), "--voxel-size", "0.1"])
    colors = CT.sphere_colors(normals)
    R.cloud_io.write_ply_normals(oriented, xyz, normals, rgb=colors)
    got = tool.read_cloud(R, tool.parse_args([oriented, "out.ply", "--voxel-size", "0.1"]))
    assert np.array_equal(got[0], xyz) and np.array_equal(got[1], normals) and np.array_equal(got[2], colors)
    R.cloud_io.write_ply_normals(oriented, xyz, normals)
    assert tool.read_cloud(R, tool.parse_args([oriented, "out.ply", "--voxel-size", "0.1"]))[2] is None
    assert len(R.cloud_io.read_ply_normals(oriented)) == 2
    # normals that the file has stand, whatever --viewpoint says; a broken file with normals is reported, not read as a plain cloud
    got = tool.read_cloud(R, tool.parse_args([oriented, "out.ply", "--voxel-size", "0.1", "--knn", "5", "--viewpoint", "0,0,0"]))
    assert np.array_equal(got[1], normals)
    short = str(tmp_path / "short.ply")
    with open(oriented, "rb") as f, open(short, "wb") as g:
        g.write(f.read()[:-100])
    with pytest.raises(SystemExit, match="too short"):
        tool.read_cloud(R, tool.parse_args([short, "out.ply", "--voxel-size", "0.1", "--viewpoint", "0,0,0"]))
