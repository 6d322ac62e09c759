"""CPU: the TSDF mesh's specification.  The generated case table (csrc/r3d_mc_table.h, tools/make_mc_table.py) against
tests/mesh_ref.py's own tracing, the reference mesh on closed forms -- the conditions tests/test_gpu_mesh.py asserts of the device
are asserted of the specification here first -- the PLY mesh files, and the argument errors that need no GPU."""
import ctypes as C
import importlib
import importlib.util
import os
import re

import numpy as np
import pytest

import mesh_ref as MREF
import tsdf_ref as REF
from helpers import PKG, ROOT

HEADER = os.path.join(ROOT, PKG, "csrc", "r3d_mc_table.h")


@pytest.fixture(scope="module")
def L():
    return importlib.import_module(PKG + "._lib")


@pytest.fixture(scope="module")
def T():
    return importlib.import_module(PKG + ".tsdf")


@pytest.fixture(scope="module")
def IO():
    return importlib.import_module(PKG + ".cloud_io")


@pytest.fixture(scope="module")
def table():
    """the committed header's 256 case words -> per case the list of triangles (edge id triples)"""
    text = open(HEADER).read()
    body = text[text.index("kMcCase[256]"):]
    words = [int(w, 16) for w in re.findall(r"0x([0-9a-f]{16})ull", body[:body.index("};")])]
    assert len(words) == 256
    out = []
    for w in words:
        n, ids = w & 7, [(w >> (3 + 4 * i)) & 15 for i in range(15)]
        assert all(e == 0 for e in ids[3 * n:]) and w >> 63 == 0
        out.append([tuple(ids[3 * t:3 * t + 3]) for t in range(n)])
    return out


def test_generated_header_is_a_fresh_generator_run():
    spec = importlib.util.spec_from_file_location("make_mc_table", os.path.join(ROOT, "tools", "make_mc_table.py"))
    gen = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(gen)
    assert gen.render().encode() == open(HEADER, "rb").read()


def test_table_equals_the_reference_tracing(table):
    for m in range(256):
        assert tuple(table[m]) == MREF.case_triangles(m), m
    text = open(HEADER).read()
    corners = [int(v) for v in re.search(r"kMcEdgeCorner\[12\] = \{([^}]*)\}", text).group(1).split(",")]
    axes = [int(v) for v in re.search(r"kMcEdgeAxis\[12\] = \{([^}]*)\}", text).group(1).split(",")]
    assert [(corners[e], axes[e]) for e in range(12)] == [(MREF.edge_corners(e)[0], MREF.edge_corners(e)[2]) for e in range(12)]


def test_table_histogram_and_edge_use(table):
    counts = [len(t) for t in table]
    assert sum(counts) == 820 and max(counts) == 5
    assert [counts.count(c) for c in range(6)] == [2, 16, 50, 80, 76, 32]
    for m in range(256):
        used = sorted({e for t in table[m] for e in t})
        assert used == MREF.crossing_edges(m), m             # each of its crossing edges, and only those
        for t in table[m]:
            assert len(set(t)) == 3


def test_consecutive_loop_edges_share_a_cell_face():
    def faces_of(e):
        lo, hi, _ = MREF.edge_corners(e)
        return {(b, MREF.CORNERS[lo][b]) for b in range(3) if MREF.CORNERS[lo][b] == MREF.CORNERS[hi][b]}
    for m in range(256):
        loops = MREF.case_loops(m)
        assert sorted(e for l in loops for e in l) == MREF.crossing_edges(m)
        assert [l[0] for l in loops] == sorted(l[0] for l in loops) and all(l[0] == min(l) for l in loops)
        for l in loops:
            assert len(l) >= 3
            for a, b in zip(l, l[1:] + l[:1]):
                assert faces_of(a) & faces_of(b), (m, l)


def test_single_negative_corner_winds_away_from_it(table):
    def point(e):
        lo, hi, _ = MREF.edge_corners(e)
        return (MREF.CORNERS[lo] + MREF.CORNERS[hi]) / 2.0
    for k in range(8):
        (t,) = table[1 << k]
        a, b, c = [point(e) for e in t]
        assert np.cross(b - a, c - a) @ (np.full(3, 0.5) - MREF.CORNERS[k]) > 0


@pytest.fixture(scope="module")
def sphere():
    return MREF.extract_mesh(MREF.sphere_volume())


def test_reference_sphere_is_closed_and_outward(sphere):
    xyz, nrm, tri = sphere
    volume, cosine = MREF.check_sphere(xyz, tri)             # closed, V - E + F = 2, every vertex used, volume within 3 %, normals within 10 degrees
    assert tri.dtype == np.int32 and len(xyz) == len(REF.extract(MREF.sphere_volume())[0])
    # the vertex normals (the volume's gradient) point outward like the triangles
    assert ((xyz.astype(np.float64) - 10.0) * nrm).sum(axis=1).min() > 0


def outer_planes(vol, voxel, axis):
    """the outer faces (axis b, side) of the volume in which the volume edge (voxel, axis) lies"""
    c = (voxel % vol.nx, voxel // vol.nx % vol.ny, voxel // (vol.nx * vol.ny))
    dims = (vol.nx, vol.ny, vol.nz)
    return {(b, c[b]) for b in range(3) if b != axis and c[b] in (0, dims[b] - 1)}


@pytest.mark.parametrize("seed", [0, 1, 2])
def test_reference_random_volumes_agree_across_shared_faces(seed):
    vol = MREF.random_volume((9, 8, 7), seed)
    xyz, nrm, tri = MREF.extract_mesh(vol)
    assert len(tri) > 500
    assert (tri[:, 0] != tri[:, 1]).all() and (tri[:, 1] != tri[:, 2]).all() and (tri[:, 2] != tri[:, 0]).all()
    assert np.array_equal(np.unique(tri), np.arange(len(xyz)))                # every vertex is used
    ids = MREF.vertex_ids(vol)
    where = np.nonzero(ids >= 0)[0]                                             # vertex id -> 3 * voxel + axis
    planes = [outer_planes(vol, int(q) // 3, int(q) % 3) for q in where]
    n = len(xyz)
    e = MREF.directed_edges(tri)
    fwd = dict(zip(*np.unique(e[:, 0] * n + e[:, 1], return_counts=True)))
    inner = 0
    for key, count in fwd.items():
        u, v = divmod(int(key), n)
        if planes[u] & planes[v]:
            continue                                         # both volume edges in one outer face: the mesh's border may pass here
        inner += 1
        assert fwd.get(v * n + u, 0) == count, (u, v)            # (counts above 1 occur: two fans with a diagonal in one face)
    assert inner > 1000


def test_reference_with_invalid_voxels():
    vol = MREF.random_volume((9, 8, 7), 5, invalid=0.1)
    assert 0.03 < (vol.w == 0).mean() < 0.2
    xyz, nrm, tri, cells = MREF.extract_mesh(vol, with_cells=True)
    assert len(tri) > 50 and tri.min() >= 0 and tri.max() < len(xyz)
    full = MREF.extract_mesh(MREF.random_volume((9, 8, 7), 5))[2]
    assert len(tri) < len(full)
    # every triangle lies in its cell, and that cell has eight valid corners
    z, rem = np.divmod(cells, vol.ny * vol.nx)
    y, x = np.divmod(rem, vol.nx)
    lo = np.stack([x, y, z], axis=1) + 0.5                   # the cell's corner 0 (voxel size 1, origin 0)
    p = xyz[tri].astype(np.float64)                          # [M, 3 vertices, 3]
    assert (p >= lo[:, None, :]).all() and (p <= lo[:, None, :] + 1.0).all()
    for k in range(8):
        dx, dy, dz = MREF.CORNERS[k]
        assert (vol.w[z + dz, y + dy, x + dx] >= 1).all()


@pytest.mark.parametrize("dims", [(1, 6, 5), (7, 1, 5), (7, 6, 1)])
def test_reference_flat_volumes_have_no_triangles(dims):
    vol = MREF.random_volume(dims, 7)
    xyz, nrm, tri = MREF.extract_mesh(vol)
    assert tri.shape == (0, 3) and len(xyz) == len(REF.extract(vol)[0]) > 0


@pytest.mark.parametrize("wide", [False, True])
def test_reference_wall(wide):
    s = REF.wall_scene(wide)
    vol = REF.run(s)[0]
    xyz, nrm, tri = MREF.extract_mesh(vol)
    REF.check_wall(s, xyz, nrm)
    m = MREF.check_wall_mesh(s, xyz, tri)
    if not wide:
        nx, ny, _ = s["dims"]
        assert m == 2 * (nx - 1) * (ny - 1)


def test_reference_room():
    s = REF.room_scene()
    vol = REF.run(s)[0]
    xyz, nrm, tri = MREF.extract_mesh(vol)
    assert len(tri) > 1000 and tri.min() >= 0 and tri.max() < len(xyz)
    REF.check_room(s, xyz[tri.reshape(-1)])                  # every triangle has all its vertices within the bound
    fewer = MREF.extract_mesh(vol, 2)[2]
    assert 0 < len(fewer) < len(tri)


def test_ply_mesh_round_trip(IO, sphere, tmp_path):
    xyz, nrm, tri = sphere
    a, b = str(tmp_path / "a.ply"), str(tmp_path / "b.ply")
    IO.write_ply_mesh(a, xyz, nrm, tri)
    x2, n2, t2 = IO.read_ply_mesh(a)
    assert t2.dtype == np.int32 and np.array_equal(t2, tri)
    assert np.array_equal(x2.view(np.uint32), xyz.view(np.uint32)) and np.array_equal(n2.view(np.uint32), nrm.view(np.uint32))
    IO.write_ply_mesh(b, x2, n2, t2.astype(np.int64))
    data = open(a, "rb").read()
    assert data == open(b, "rb").read()
    head = data[:data.index(b"end_header\n")].decode().rstrip("\n").split("\n")
    assert head[:3] == ["ply", "format binary_little_endian 1.0", "element vertex %d" % len(xyz)]
    assert head[-2:] == ["element face %d" % len(tri), "property list uchar int vertex_indices"]
    assert len(data) == data.index(b"end_header\n") + 11 + 24 * len(xyz) + 13 * len(tri)
    # its vertex rows are what read_ply_normals reads
    x3, n3 = IO.read_ply_normals(a)
    assert np.array_equal(x3, xyz) and np.array_equal(n3, nrm)
    # the empty mesh
    IO.write_ply_mesh(b, np.zeros((0, 3), np.float32), np.zeros((0, 3), np.float32), np.zeros((0, 3), np.int32))
    assert [v.shape for v in IO.read_ply_mesh(b)] == [(0, 3)] * 3


def test_ply_mesh_rejects_bad_triangles(IO, sphere, tmp_path):
    xyz, nrm, tri = sphere
    path = str(tmp_path / "bad.ply")
    bads = [tri.astype(np.float32), tri.reshape(-1), tri[:, :2], np.zeros((2, 4), np.int32), tri + len(xyz), -tri - 1]
    hi = tri.copy()
    hi[-1, 2] = len(xyz)
    lo = tri.copy()
    lo[0, 0] = -1
    for bad in bads + [hi, lo]:
        with pytest.raises(ValueError):
            IO.write_ply_mesh(path, xyz, nrm, bad)
    with pytest.raises(ValueError):
        IO.write_ply_mesh(path, xyz, nrm[:-1], tri)
    assert not os.path.exists(path)
    # a file whose face names a vertex that is not there
    IO.write_ply_mesh(path, xyz, nrm, tri)
    data = bytearray(open(path, "rb").read())
    data[-4:] = np.array([len(xyz)], "<i4").tobytes()
    open(path, "wb").write(bytes(data))
    with pytest.raises(ValueError):
        IO.read_ply_mesh(path)
    open(path, "wb").write(bytes(data[:-5]))
    with pytest.raises(ValueError):
        IO.read_ply_mesh(path)
    IO.write_ply_normals(path, xyz, nrm)
    with pytest.raises(ValueError):
        IO.read_ply_mesh(path)


def test_symbol_is_exported_and_bound(L, T):
    lib = L.load()
    assert hasattr(lib, "r3d_tsdf_extract_mesh") and "r3d_tsdf_extract_mesh" in L.SIGNATURES
    assert callable(T.TSDFVolume.extract_mesh_device) and callable(T.TSDFVolume.extract_triangle_mesh)
    header = open(os.path.join(ROOT, "include", "r3d.h")).read()
    assert "820 triangles" in header and "int r3d_tsdf_extract_mesh(" in header


def test_argument_errors_without_gpu(L, T):
    lib = L.load()
    nv, nt = C.c_int64(-7), C.c_int64(-9)
    assert lib.r3d_tsdf_extract_mesh(None, 1.0, None, None, 0, None, 0, C.byref(nv), C.byref(nt)) == L.ERR_INVALID
    assert (nv.value, nt.value) == (-7, -9) and "NULL" in L.last_error()
    assert lib.r3d_tsdf_extract_mesh(None, 1.0, None, None, 0, None, 0, None, None) == L.ERR_INVALID
    for bad in (0, -1.0, float("nan"), float("inf"), 1e-60, None, True, "x"):
        with pytest.raises((ValueError, TypeError)):
            T.TSDFVolume.extract_triangle_mesh(object(), bad)     # rejected before the volume is looked at
        with pytest.raises((ValueError, TypeError)):
            T.TSDFVolume.extract_mesh_device(object(), bad, None, None, 0, None, 0)
