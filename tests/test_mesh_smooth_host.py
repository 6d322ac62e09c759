"""CPU: the mesh smoothing restatement (tests/mesh_smooth_ref.py) on the meshes the GPU tests use -- their conditions are asserted
here first --, its properties, whether the filters do what they are for, and what the library and the header say without a GPU."""
import ctypes as C
import importlib
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import mesh_ref as MREF
import mesh_smooth_ref as MS
from helpers import PKG, ROOT
from test_mesh_cc_host import volume_mesh

# mesh -> (vertices, triangles, E, smallest degree or None, largest degree, boundary vertices, isolated vertices)
MESHES = {"sphere": (720, 1436, 4308, 4, 9, 0, 0),
          ((9, 8, 7), 5, 0.0): (653, 1042, 3416, None, 14, 290, 0),
          ((16, 16, 16), 85, 0.3): (2847, 723, 3240, None, 10, 1051, 1786)}
CENTRE = np.array([10.0, 10.0, 10.0])
_ADJ = {}


def adjacency_of(key):
    """mesh_smooth_ref.adjacency of a named mesh, computed once per session"""
    if key not in _ADJ:
        xyz, _, tri = volume_mesh(key)
        _ADJ[key] = MS.adjacency(tri, len(xyz))
    return _ADJ[key]


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


@pytest.mark.parametrize("key", list(MESHES), ids=str)
def test_conditions_of_the_reference_meshes(key):
    xyz, _, tri = volume_mesh(key)
    nv, nt, e, dmin, dmax, n_boundary, n_isolated = MESHES[key]
    assert (len(xyz), len(tri)) == (nv, nt)
    rs, nb, bd = adjacency_of(key)
    deg = np.diff(rs.astype(np.int64))
    assert (int(rs[-1]), len(nb), int(deg.max()), int(bd.sum()), int((deg == 0).sum())) == (e, e, dmax, n_boundary, n_isolated)
    if dmin is not None:
        assert deg.min() == dmin
    for a, b in zip((rs, nb, bd), MS.adjacency_loops(tri, nv)):
        assert a.dtype == b.dtype and np.array_equal(a, b)


@pytest.mark.parametrize("key", list(MESHES), ids=str)
def test_adjacency_properties(key):
    xyz, _, tri = volume_mesh(key)
    nv = len(xyz)
    rs, nb, bd = adjacency_of(key)
    assert rs[0] == 0 and (np.diff(rs.astype(np.int64)) >= 0).all() and rs[-1] % 2 == 0
    owner = np.repeat(np.arange(nv), np.diff(rs.astype(np.int64)))
    assert (nb != owner).all() and (nb < nv).all()                                  # no self-entries
    same_row = owner[1:] == owner[:-1]
    assert (nb[1:][same_row] > nb[:-1][same_row]).all()                             # ascending and distinct in every row
    pairs = set(zip(owner.tolist(), nb.tolist()))
    assert all((v, u) in pairs for u, v in pairs)                                   # symmetric
    assert not bd[np.diff(rs.astype(np.int64)) == 0].any()
    rng = np.random.default_rng(5)
    shuffled = tri[rng.permutation(len(tri))]
    rotated = np.stack([np.roll(t, k) for t, k in zip(shuffled, rng.integers(0, 3, len(shuffled)))]) if len(tri) else shuffled
    for other in (shuffled, rotated):
        for a, b in zip((rs, nb, bd), MS.adjacency(other, nv)):
            assert np.array_equal(a, b)
    rs2, nb2, bd2 = MS.adjacency(np.concatenate([tri, tri]), nv)                    # every edge has two sides or more now
    assert np.array_equal(rs2, rs) and np.array_equal(nb2, nb) and not bd2.any()


def test_adjacency_by_hand():
    rs, nb, bd = MS.adjacency(np.array([[0, 1, 2]], np.int32), 3)
    assert rs.tolist() == [0, 2, 4, 6] and nb.tolist() == [1, 2, 0, 2, 0, 1] and bd.tolist() == [1, 1, 1]
    # an invalid triangle gives nothing; (2, 2, 3) has one side twice, (2, 3) and (3, 2): the edge {2, 3} is not boundary
    tri = np.array([[0, 1, 2], [2, 2, 3], [4, 4, 4], [-1, 0, 1], [0, 1, 6], [5, 4, -2 ** 31]], np.int32)
    rs, nb, bd = MS.adjacency(tri, 6)
    assert rs.tolist() == [0, 2, 4, 7, 8, 8, 8] and nb.tolist() == [1, 2, 0, 2, 0, 1, 3, 2] and bd.tolist() == [1, 1, 1, 0, 0, 0]
    for a, b in zip((rs, nb, bd), MS.adjacency_loops(tri, 6)):
        assert np.array_equal(a, b)
    assert [a.tolist() for a in MS.adjacency(np.zeros((0, 3), np.int32), 5)] == [[0] * 6, [], [0] * 5]
    assert [a.tolist() for a in MS.adjacency(np.array([[0, 1, 2]], np.int32), 0)] == [[0], [], []]
    hub = MS.adjacency(MS.fan(5000), 5002)
    assert hub[0][1] == 5001 and hub[1][:5001].tolist() == list(range(1, 5002)) and hub[2].all()


def test_fixed_points_of_the_steps():
    xyz, tri = MS.grid(9, 7)
    rs, nb, bd = MS.adjacency(tri, len(xyz))
    assert bd.sum() == 2 * (9 + 7) - 4
    out = MS.smooth(xyz, rs, nb, bd, MS.smooth_factors("taubin", 5))
    assert np.array_equal(bits(out[:, 2]), bits(xyz[:, 2]))                         # the plane's normal direction: no motion at all
    assert np.array_equal(bits(out[bd == 1]), bits(xyz[bd == 1])) and (bits(out[bd == 0])[:, :2] != bits(xyz[bd == 0])[:, :2]).any()
    assert np.array_equal(bits(MS.smooth(xyz, rs, nb, None, [])), bits(xyz))        # no step: the input's bits
    assert np.array_equal(bits(MS.smooth(xyz, rs, nb, np.ones(len(xyz), np.uint8), [0.5, 1.0, 2.5])), bits(xyz))
    assert np.array_equal(bits(MS.smooth(xyz, rs, nb, None, [0.0, 0.0])), bits(xyz))
    key = ((16, 16, 16), 85, 0.3)
    p, _, _ = volume_mesh(key)
    rs, nb, bd = adjacency_of(key)
    alone = np.diff(rs.astype(np.int64)) == 0
    out = MS.smooth(p, rs, nb, None, [0.5, -0.53, 1.0])
    assert alone.sum() == 1786 and np.array_equal(bits(out[alone]), bits(p[alone])) and (bits(out[~alone]) != bits(p[~alone])).any()
    small = p[:60]                                                                 # the loops agree with the rounds
    rs, nb, bd = MS.adjacency(MS.fan(58), 60)
    assert np.array_equal(bits(MS.step(small, rs, nb, None, 0.7)), bits(MS.step_loops(small, rs, nb, None, 0.7)))


def noisy_sphere():
    """(clean xyz, triangles, noisy xyz, the vertices' mean radius): isotropic Gaussian noise of 0.1 mean edge, seed 3"""
    xyz, _, tri = volume_mesh("sphere")
    e = MREF.directed_edges(tri)
    mean_edge = np.linalg.norm(xyz[e[:, 0]].astype(np.float64) - xyz[e[:, 1]], axis=1).mean()
    radius = np.linalg.norm(xyz.astype(np.float64) - CENTRE, axis=1).mean()
    assert abs(radius - 6.29) < 0.01 and abs(mean_edge - 0.97) < 0.01
    noisy = (xyz.astype(np.float64) + np.random.default_rng(3).normal(0.0, 0.1 * mean_edge, xyz.shape)).astype(np.float32)
    return xyz, tri, noisy, radius


def radial_rms(p, radius):
    return float(np.sqrt(((np.linalg.norm(p.astype(np.float64) - CENTRE, axis=1) - radius) ** 2).mean()))


def test_taubin_smooths_without_shrinking_and_laplacian_shrinks():
    """Measured with this restatement (seed 3, sigma 0.1 mean edge, 10 iterations; DESIGN.md 4.5j''): radial RMS about the clean
    radius 0.0955 -> 0.0381 for Taubin (ratio 0.399) and -> 0.341 for Laplacian; enclosed volume 1031.8 clean, 1038.6 after Taubin
    (+0.66 %), 873.2 after Laplacian (0.846 of the clean one)."""
    xyz, tri, noisy, radius = noisy_sphere()
    rs, nb, _ = adjacency_of("sphere")
    clean_volume = MS.enclosed_volume(xyz, tri, CENTRE)
    taubin = MS.smooth(noisy, rs, nb, None, MS.smooth_factors("taubin", 10))
    laplace = MS.smooth(noisy, rs, nb, None, MS.smooth_factors("laplacian", 10))
    before, after = radial_rms(noisy, radius), radial_rms(taubin, radius)
    v_taubin, v_laplace = MS.enclosed_volume(taubin, tri, CENTRE), MS.enclosed_volume(laplace, tri, CENTRE)
    print("radial rms %.4f -> taubin %.4f (ratio %.3f), laplacian %.4f; volume clean %.1f taubin %.1f laplacian %.1f (%.3f)"
          % (before, after, after / before, radial_rms(laplace, radius), clean_volume, v_taubin, v_laplace, v_laplace / clean_volume))
    assert after <= 0.55 * before
    assert abs(v_taubin - clean_volume) <= 0.02 * clean_volume
    assert v_laplace < 0.90 * clean_volume


def test_vertex_normals():
    xyz, nrm, tri = volume_mesh("sphere")
    n = MS.vertex_normals(xyz, tri)
    assert np.array_equal(bits(n), bits(MS.vertex_normals_loops(xyz, tri)))
    assert np.abs(np.linalg.norm(n.astype(np.float64), axis=1) - 1.0).max() < 1e-6
    radial = xyz.astype(np.float64) - CENTRE
    radial /= np.linalg.norm(radial, axis=1)[:, None]
    worst = np.degrees(np.arccos((n * radial).sum(axis=1).min()))
    print("worst angle between a vertex normal and the radius: %.2f degrees" % worst)   # measured 6.55
    assert worst < 10.0                                                              # (a face normal is held to 10 by check_sphere)
    assert ((n * nrm).sum(axis=1) > 0).all()                                         # the sign of the TSDF normals they replace
    key = ((16, 16, 16), 85, 0.3)
    p, fb, t = volume_mesh(key)
    alone = np.diff(adjacency_of(key)[0].astype(np.int64)) == 0
    with_fb, without = MS.vertex_normals(p, t, fb), MS.vertex_normals(p, t)
    assert np.array_equal(bits(with_fb[alone]), bits(fb[alone])) and not without[alone].any()
    assert np.array_equal(bits(with_fb[~alone]), bits(without[~alone])) and (np.abs(without[~alone]).sum(axis=1) > 0).all()
    assert np.array_equal(bits(with_fb), bits(MS.vertex_normals_loops(p, t, fb)))
    flat = MS.vertex_normals(p[:5], np.array([[0, 0, 1], [2, 2, 2], [3, 4, 3]], np.int32), fb[:5])   # all degenerate: exact zeros
    assert np.array_equal(bits(flat), bits(fb[:5]))
    moved, normals = MS.smooth_mesh(p, t, "laplacian", 2, normals=fb)
    assert np.array_equal(bits(normals), bits(MS.vertex_normals(moved, t, fb))) and np.array_equal(bits(moved[alone]), bits(p[alone]))


# ---- the library without a device ----------------------------------------------------------------------------------------------
def test_argument_errors_without_gpu():
    L = importlib.import_module(PKG + "._lib")
    lib = L.load()
    e = C.c_int64(-7)
    pe = C.byref(e)
    fake = C.create_string_buffer(4096)                          # stands in for a context: every check below fails before it is read
    ctx = C.addressof(fake)
    buf = np.zeros(256, np.uint32)
    p = buf.ctypes.data
    adjacency_calls = [(None, p, 1, 3, p + 64, None, 0, None, pe),
                       (ctx, p, 1, 3, p + 64, None, 0, None, None),
                       (ctx, p, -1, 3, p + 64, None, 0, None, pe),
                       (ctx, p, 1, -3, p + 64, None, 0, None, pe),
                       (ctx, p, 1, 3, p + 64, None, -1, None, pe),
                       (ctx, None, 1, 3, p + 64, None, 0, None, pe),
                       (ctx, p, 1, 3, None, None, 0, None, pe),
                       (ctx, p, 1, 3, p + 64, None, 1, None, pe),
                       (ctx, p, 1, 3, p + 8, None, 0, None, pe),                    # row_start overlaps the triangles
                       (ctx, p, 1, 3, p + 64, p + 8, 6, None, pe),                  # the neighbours overlap the triangles
                       (ctx, p, 1, 3, p + 64, None, 0, p + 11, pe),                 # the boundary flags overlap the triangles
                       (ctx, p, 1, 3, p + 64, p + 76, 6, None, pe),                 # the neighbours overlap row_start
                       (ctx, p, 1, 3, p + 64, p + 128, 6, p + 130, pe)]             # the boundary flags overlap the neighbours
    for args in adjacency_calls:
        assert lib.r3d_mesh_adjacency(*args) == L.ERR_INVALID, args
        assert L.last_error()
    f = (C.c_double * 3)(0.5, -0.53, 0.5)
    nan, inf = (C.c_double * 2)(0.5, float("nan")), (C.c_double * 1)(float("inf"))
    smooth_calls = [(None, p, p + 64, 3, p + 128, p + 192, None, f, 3),
                    (ctx, p, p + 64, -1, p + 128, p + 192, None, f, 3),
                    (ctx, p, p + 64, 3, p + 128, p + 192, None, f, -1),
                    (ctx, p, p + 64, 3, p + 128, p + 192, None, f, 4097),
                    (ctx, p, p + 64, 3, p + 128, p + 192, None, None, 1),
                    (ctx, p, p + 64, 3, p + 128, p + 192, None, nan, 2),
                    (ctx, p, p + 64, 3, p + 128, p + 192, None, inf, 1),
                    (ctx, None, p + 64, 3, p + 128, p + 192, None, f, 3),
                    (ctx, p, None, 3, p + 128, p + 192, None, f, 3),
                    (ctx, p, p + 64, 3, None, p + 192, None, f, 3),
                    (ctx, p, p, 3, p + 128, p + 192, None, f, 3),                   # in place
                    (ctx, p, p + 32, 3, p + 128, p + 192, None, f, 0),              # a partial overlap, even without a step
                    (ctx, p, p + 120, 3, p + 128, p + 192, None, f, 3),             # out overlaps row_start
                    (ctx, p, p + 64, 3, p + 128, p + 96, None, f, 3),               # out overlaps the neighbours
                    (ctx, p, p + 64, 3, p + 128, p + 192, p + 98, f, 3)]            # out overlaps the locked flags
    for args in smooth_calls:
        assert lib.r3d_mesh_smooth(*args) == L.ERR_INVALID, args
        assert L.last_error()
    normal_calls = [(None, p, 3, p + 64, 1, None, p + 128),
                    (ctx, p, -3, p + 64, 1, None, p + 128),
                    (ctx, p, 3, p + 64, -1, None, p + 128),
                    (ctx, p, 3, None, 1, None, p + 128),
                    (ctx, None, 3, p + 64, 1, None, p + 128),
                    (ctx, p, 3, p + 64, 1, None, None),
                    (ctx, p, 3, p + 64, 1, None, p + 32),                           # the normals overlap the positions
                    (ctx, p, 3, p + 64, 1, None, p + 72),                           # ... the triangles
                    (ctx, p, 3, p + 64, 1, p + 160, p + 128)]                       # ... the fallback rows
    for args in normal_calls:
        assert lib.r3d_mesh_vertex_normals(*args) == L.ERR_INVALID, args
        assert L.last_error()
    assert e.value == -7 and not buf.any() and not fake.raw.strip(b"\0")
    limit = (2 ** 32 + 5) // 6                                   # the first triangle count with 6 M >= 2^32
    assert lib.r3d_mesh_adjacency(ctx, p, limit, 3, p + 64, None, 0, None, pe) == L.ERR_UNSUPPORTED
    assert lib.r3d_mesh_adjacency(ctx, p, 0, 2 ** 31, p + 64, None, 0, None, pe) == L.ERR_UNSUPPORTED
    assert lib.r3d_mesh_vertex_normals(ctx, p, 3, p + 64, limit, None, p + 128) == L.ERR_UNSUPPORTED
    assert lib.r3d_mesh_smooth(ctx, p, p + 64, 2 ** 31, p + 128, p + 192, None, f, 3) == L.ERR_UNSUPPORTED
    assert e.value == -7 and not buf.any()


def test_python_argument_errors_and_factors_without_gpu():
    M = importlib.import_module(PKG + ".mesh")
    assert M.smooth_factors() == [0.5, -0.53] * 10 and M.smooth_factors("laplacian", 3, 0.25, mu=None) == [0.25] * 3
    assert M.smooth_factors("taubin", 0) == [] and M.smooth_factors("taubin", 2, 0.4, -0.5) == [0.4, -0.5, 0.4, -0.5]
    assert M.smooth_factors("taubin", 2048) == MS.smooth_factors("taubin", 2048) and len(M.smooth_factors("laplacian", 4096)) == 4096
    for bad in (("median", 1), ("taubin", -1), ("taubin", 1.5), ("taubin", True), ("taubin", 2049), ("laplacian", 4097),
                ("taubin", 1, 0.0), ("taubin", 1, -0.5), ("taubin", 1, float("nan")), ("taubin", 1, "0.5"), ("taubin", 1, 0.5, 0.53),
                ("taubin", 1, 0.5, -0.5), ("taubin", 1, 0.5, -0.4), ("taubin", 1, 0.5, float("-inf")), ("taubin", 1, 0.5, None)):
        with pytest.raises(ValueError):
            M.smooth_factors(*bad)
    assert M.smooth_params(("laplacian", 3)) == {"method": "laplacian", "iterations": 3, "lam": 0.5, "mu": -0.53, "lock_boundary": True}
    assert M.smooth_params({"iterations": 2, "lock_boundary": 0})["lock_boundary"] is False
    for bad in ("taubin", 5, {"iteration": 2}, ("taubin", 1, 0.5, -0.53, True, 1), {"method": "x"}):
        with pytest.raises(ValueError):
            M.smooth_params(bad)
    xyz, tri = np.zeros((3, 3), np.float32), [[0, 1, 2]]
    for call in (lambda: M.smooth_mesh(xyz.astype(np.float64), tri), lambda: M.smooth_mesh(np.zeros((3, 2), np.float32), tri),
                 lambda: M.smooth_mesh(xyz, np.zeros((1, 2), np.int32)), lambda: M.smooth_mesh(xyz, tri, method="x"),
                 lambda: M.smooth_mesh(xyz, tri, normals=np.zeros((2, 3), np.float32)), lambda: M.smooth_mesh(xyz, tri, iterations=-1),
                 lambda: M.compute_vertex_normals(xyz, tri, fallback=np.zeros((3, 3), np.float64)),
                 lambda: M.compute_vertex_normals(xyz[:, :2], tri), lambda: M.mesh_adjacency(tri, -1),
                 lambda: M.mesh_adjacency(np.zeros((2, 3), np.float32), 3)):
        with pytest.raises(ValueError):
            call()
    with pytest.raises(ValueError):
        M.smooth_mesh_device(None, 0, 0, 3, 0, 0, None, [0.5, float("nan")])
    with pytest.raises(ValueError):
        M.smooth_mesh_device(None, 0, 0, 3, 0, 0, None, [0.5] * 4097)
    tool = importlib.import_module(PKG + ".other_tools.integrate_tsdf")
    base = ["--voxel-size", "1", "--trunc", "3"]
    for extra in (["--mesh-smooth", "taubin,5"], ["--mesh", "--mesh-smooth-free-boundary"], ["--mesh", "--mesh-smooth", "taubin"],
                  ["--mesh", "--mesh-smooth", "median,5"], ["--mesh", "--mesh-smooth", "taubin,x"], ["--mesh", "--mesh-smooth", "taubin,5,0.5,0.6"],
                  ["--mesh", "--mesh-smooth", "taubin,5,0.5,-0.53,1"], ["--mesh", "--mesh-smooth", "taubin,-1"]):
        with pytest.raises(SystemExit):
            tool.parse_args(base + extra)
    args = tool.parse_args(base + ["--mesh", "--mesh-smooth", "laplacian,4,0.25", "--mesh-smooth-free-boundary"])
    assert args.mesh_smooth == {"method": "laplacian", "iterations": 4, "lam": 0.25, "mu": -0.53, "lock_boundary": False}
    assert tool.parse_args(base + ["--mesh"]).mesh_smooth is None


def test_header_signatures_and_layout():
    text = open(os.path.join(ROOT, "include", "r3d.h")).read()
    assert "/* ---- Mesh smoothing (csrc/r3d_mesh_smooth.hip" in text
    flat = re.sub(r"\s+", " ", text)
    assert ("int r3d_mesh_adjacency(r3d_ctx* ctx, const int32_t* d_tri, int64_t n_triangles, int64_t n_vertices, "
            "uint32_t* d_row_start_out, uint32_t* d_neighbours_out, int64_t cap_neighbours, uint8_t* d_boundary_out, "
            "int64_t* n_neighbours_out);") in flat
    assert ("int r3d_mesh_smooth(r3d_ctx* ctx, const float* d_xyz_in, float* d_xyz_out, int64_t n_vertices, const uint32_t* d_row_start, "
            "const uint32_t* d_neighbours, const uint8_t* d_locked, const double* factors, int n_factors);") in flat
    assert ("int r3d_mesh_vertex_normals(r3d_ctx* ctx, const float* d_xyz, int64_t n_vertices, const int32_t* d_tri, "
            "int64_t n_triangles, const float* d_fallback, float* d_normals_out);") in flat
    section = text[text.index("/* ---- Mesh smoothing"):text.index("int r3d_mesh_adjacency(")]
    for phrase in ("ASCENDING INDEX", "exactly one", "counted with multiplicity", "true E", "R3D_ERR_UNSUPPORTED", "Jacobi", "[0, 4096]",
                   "keeps its bits", "ASCENDING t", "(+0, +0, +0)", "0 < len < inf", "ASYNCHRONOUS", "synchronises", "ping-pong"):
        assert phrase in section, phrase
    L = importlib.import_module(PKG + "._lib")
    lib = L.load()
    for name in ("r3d_mesh_adjacency", "r3d_mesh_smooth", "r3d_mesh_vertex_normals"):
        assert name in L.SIGNATURES and hasattr(lib, name)
    csrc = os.path.join(ROOT, PKG, "csrc")
    kernels, host = open(os.path.join(csrc, "r3d_mesh_smooth.hip")).read(), open(os.path.join(csrc, "r3d_mesh_smooth_host.cpp")).read()
    assert "r3d_scratch(" not in kernels and "__global__" not in host              # kernels in one file, workspaces in the other
    assert set(re.findall(r"r3d_scratch\(\s*ctx,\s*(\w+)", host)) == {"kWsMeshSmooth"}
    assert "atomic" not in kernels.split("#include", 1)[1] and "tri_valid" in kernels and "bool tri_valid" not in kernels
    internal = open(os.path.join(csrc, "r3d_internal.h")).read()
    assert "kWsMeshSmooth" in internal and "kScratchSlots = 15" in internal


HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")


@pytest.mark.skipif(shutil.which(HIPCC) is None and not os.path.exists(HIPCC), reason="hipcc not available")
def test_no_mesh_smooth_kernel_uses_scratch(tmp_path):
    """tools/isa_stats.py on the gfx950 listing of csrc/r3d_mesh_smooth.hip: seven kernels, no private segment, no spills; the step
    kernel gathers a neighbour's row with one 12-byte load and stores its own with one 12-byte store."""
    src, out = os.path.join(ROOT, PKG, "csrc", "r3d_mesh_smooth.hip"), str(tmp_path / "mesh_smooth.s")
    subprocess.run([HIPCC, "-O3", "-std=c++17", "--offload-arch=gfx950", "-ffp-contract=off", "-fPIC", "-I" + os.path.join(ROOT, "include"),
                    "--cuda-device-only", "-S", src, "-o", out], check=True, capture_output=True)
    r = subprocess.run(["python3", os.path.join(ROOT, "tools", "isa_stats.py"), out, "ms_"], check=True, capture_output=True, text=True)
    kernels = re.findall(r"^\S*?ms_(\w+?)_kernel\S* instrs", r.stdout, re.M)
    assert sorted(kernels) == ["corner_keys", "heads_count", "heads_write", "normals", "rows", "side_keys", "step"], r.stdout
    assert "scratch_" not in r.stdout and "buffer_" not in r.stdout
    text = open(out).read()
    assert len(re.findall(r"\.amdhsa_private_segment_fixed_size 0\n", text)) == 7 == text.count(".amdhsa_private_segment_fixed_size")
    assert set(re.findall(r"\.vgpr_spill_count:\s+(\d+)", text)) == {"0"}
    step = r.stdout[r.stdout.index("ms_step_kernel"):].split("\n")[1]
    assert "'global_load_dwordx3': 3" in step and "'global_store_dwordx3': 1" in step and "atomic" not in step, step
