"""CPU: the mesh component restatement (tests/mesh_cc_ref.py) on the meshes the GPU tests use -- their conditions are asserted
here first --, its properties, and what the library and the header say without a GPU."""
import ctypes as C
import importlib
import os
import re

import numpy as np
import pytest

import mesh_cc_ref as CC
import mesh_ref as MREF
from helpers import PKG, ROOT

# random_volume arguments -> (vertices, triangles, components, largest component's triangles, vertices no triangle names)
VOLUMES = {((9, 8, 7), 5, 0.0): (653, 1042, 11, 955, 0),
           ((16, 16, 17), 86, 0.0): (6179, 11589, 73, 10916, 0),
           ((16, 16, 16), 85, 0.3): (2847, 723, 168, None, 1786),
           ((40, 9, 5), 3, 0.2): (1517, 671, 85, None, 717)}
_MESHES = {}


def volume_mesh(key):
    """(xyz, normals, triangles) of mesh_ref.random_volume(*key), computed once per session"""
    if key not in _MESHES:
        _MESHES[key] = MREF.extract_mesh(MREF.sphere_volume() if key == "sphere" else MREF.random_volume(*key))
    return _MESHES[key]


@pytest.mark.parametrize("key", list(VOLUMES))
def test_conditions_of_the_reference_meshes(key):
    xyz, _, tri = volume_mesh(key)
    nv, nt, ncomp, largest, unnamed = VOLUMES[key]
    assert (len(xyz), len(tri)) == (nv, nt)
    labels, tri_labels, rows, bad = CC.components(tri, nv)
    assert bad == 0 and len(rows) == ncomp
    assert nv - len(np.unique(tri)) == unnamed
    assert rows[:, 2].sum() == nt and rows[:, 1].sum() == nv - unnamed
    if largest is not None:
        assert rows[:, 2].max() == largest
    if key == ((16, 16, 17), 86, 0.0):
        assert np.sort(rows[:, 2])[-2] <= 98
    assert len(rows) > 1 and rows[:, 2].min() < 5                # floaters: the thresholds of the filter tests separate something


def test_sphere_is_one_component():
    xyz, _, tri = volume_mesh("sphere")
    labels, tri_labels, rows, bad = CC.components(tri, len(xyz))
    assert rows.tolist() == [[0, len(xyz), 1436]] and bad == 0 and (labels == 0).all() and (tri_labels == 0).all()


@pytest.mark.parametrize("key", list(VOLUMES))
def test_labels_are_minima_and_do_not_depend_on_triangle_order(key):
    xyz, _, tri = volume_mesh(key)
    nv = len(xyz)
    labels, tri_labels, rows, _ = CC.components(tri, nv)
    assert (labels <= np.arange(nv)).all() and (labels[labels] == labels).all()
    for lab in np.unique(labels):
        assert np.flatnonzero(labels == lab)[0] == lab           # the label is the smallest vertex that carries it
    assert (labels[tri] == labels[tri[:, :1]]).all()             # a triangle's vertices share one label
    # vertices of different triangles share a label only through a chain: brute force over the components' vertex sets
    sets = {}
    for a, b, c in tri.tolist():
        group = set((a, b, c))
        for k in [k for k, s in sets.items() if s & group]:
            group |= sets.pop(k)
        sets[min(group)] = group
    assert sorted(sets) == rows[:, 0].tolist()
    for k, s in sets.items():
        assert (labels[sorted(s)] == k).all() and len(s) == rows[rows[:, 0] == k][0, 1]
    perm = np.random.default_rng(7).permutation(len(tri))
    again = CC.components(tri[perm], nv)
    assert np.array_equal(again[0], labels) and np.array_equal(again[1], tri_labels[perm]) and np.array_equal(again[2], rows)


@pytest.mark.parametrize("key", list(VOLUMES))
def test_filter_is_idempotent_and_names_every_kept_vertex(key):
    xyz, nrm, tri = volume_mesh(key)
    for mt, largest in ((1, False), (2, False), (5, False), (99, False), (1, True), (5, True)):
        x, n, t = CC.remove_small(xyz, nrm, tri, mt, largest)
        assert np.array_equal(np.unique(t), np.arange(len(x)))   # every kept vertex is named, nothing else is
        rows = CC.components(t, len(x))[2]
        assert (rows[:, 2] >= mt).all() and (not largest or len(rows) <= 1)
        x2, n2, t2 = CC.remove_small(x, n, t, mt, largest)
        assert np.array_equal(x2, x) and np.array_equal(n2, n) and np.array_equal(t2, t)
        if mt == 1 and not largest:                              # only the vertices without a triangle go
            assert len(t) == len(tri) and len(x) == len(np.unique(tri))
    full = CC.components(tri, len(xyz))[2]
    big = int(full[:, 2].max())
    assert len(CC.remove_small(xyz, nrm, tri, big, False)[2]) >= big
    assert [len(a) for a in CC.remove_small(xyz, nrm, tri, big + 1, False)] == [0, 0, 0]
    assert [len(a) for a in CC.remove_small(xyz, nrm, tri, big + 1, True)] == [0, 0, 0]


def test_small_cases_by_hand():
    tri = np.array([[4, 5, 6], [0, 1, 2], [2, 2, 3], [9, 9, 9], [-1, 0, 1], [0, 1, 10], [7, 8, 2**31 - 1], [6, 5, 4]], np.int32)
    labels, tl, rows, bad = CC.components(tri, 10)
    assert labels.tolist() == [0, 0, 0, 0, 4, 4, 4, 7, 8, 9]
    assert tl.tolist() == [4, 0, 0, 9, CC.NO_LABEL, CC.NO_LABEL, CC.NO_LABEL, 4] and bad == 3
    assert rows.tolist() == [[0, 4, 2], [4, 3, 2], [9, 1, 1]]
    kept, out = CC.filter_components(tri, 10, labels, 2, False)
    assert kept.tolist() == [0, 1, 2, 3, 4, 5, 6] and out.tolist() == [[4, 5, 6], [0, 1, 2], [2, 2, 3], [6, 5, 4]]
    kept, out = CC.filter_components(tri, 10, labels, 1, True)   # a tie of 2 and 2: the smaller label wins
    assert kept.tolist() == [0, 1, 2, 3] and out.tolist() == [[0, 1, 2], [2, 2, 3]]
    assert [len(a) for a in CC.filter_components(tri, 10, labels, 3, True)] == [0, 0]
    assert [a.shape for a in CC.components(np.zeros((0, 3), np.int32), 0)[:3]] == [(0,), (0,), (0, 3)]
    assert CC.components(np.zeros((0, 3), np.int32), 3)[0].tolist() == [0, 1, 2]


def test_shapes_of_the_synthetic_meshes():
    rng = np.random.default_rng(11)
    for ids in (None, np.arange(5002)[::-1], rng.permutation(5002)):
        t = CC.strip(5000, ids)
        labels, _, rows, _ = CC.components(t[rng.permutation(5000)], 5002)
        assert (labels == 0).all() and rows.tolist() == [[0, 5002, 5000]]
    assert CC.components(CC.disjoint(4096), 3 * 4096)[2][:, 0].tolist() == list(range(0, 3 * 4096, 3))
    t, nv = CC.fans(64, 5)
    assert CC.components(t, nv)[2].tolist() == [[0, nv, 320]]
    assert len(CC.components(t[t[:, 0] != 0], nv)[2]) == 0       # (only the hub joins the fans: every triangle names it)


def test_argument_errors_without_gpu():
    L = importlib.import_module(PKG + "._lib")
    lib = L.load()
    a, b = C.c_int64(-7), C.c_int64(-9)
    pa, pb = C.byref(a), C.byref(b)
    fake = C.create_string_buffer(4096)                          # stands in for a context: every check below fails before it is read
    ctx = C.addressof(fake)
    buf = np.zeros(64, np.uint32)
    p = buf.ctypes.data
    comp_calls = [(None, p, 1, 3, p + 64, None, None, 0, pa, pb),
                  (ctx, p, 1, 3, p + 64, None, None, 0, None, pb),
                  (ctx, p, 1, 3, p + 64, None, None, 0, pa, None),
                  (ctx, p, -1, 3, p + 64, None, None, 0, pa, pb),
                  (ctx, p, 1, -3, p + 64, None, None, 0, pa, pb),
                  (ctx, p, 1, 3, p + 64, None, None, -1, pa, pb),
                  (ctx, None, 1, 3, p + 64, None, None, 0, pa, pb),
                  (ctx, p, 1, 3, None, None, None, 0, pa, pb),
                  (ctx, p, 1, 3, p + 64, None, None, 1, pa, pb),
                  (ctx, p, 1, 3, p + 8, None, None, 0, pa, pb),              # the labels overlap the triangles
                  (ctx, p, 1, 3, p + 64, p + 8, None, 0, pa, pb),            # the triangle labels overlap the triangles
                  (ctx, p, 1, 3, p + 64, p + 72, None, 0, pa, pb),           # the two label arrays overlap
                  (ctx, p, 1, 3, p + 64, None, p + 68, 1, pa, pb)]           # the rows overlap the labels
    for args in comp_calls:
        assert lib.r3d_mesh_components(*args) == L.ERR_INVALID, args
        assert L.last_error()
    filt_calls = [(None, p, 1, 3, p + 64, 1, 0, None, 0, None, 0, pa, pb),
                  (ctx, p, 1, 3, p + 64, 1, 0, None, 0, None, 0, None, pb),
                  (ctx, p, 1, 3, p + 64, 1, 0, None, 0, None, 0, pa, None),
                  (ctx, p, 1, 3, p + 64, 0, 0, None, 0, None, 0, pa, pb),    # min_triangles = 0
                  (ctx, p, 1, 3, p + 64, -5, 1, None, 0, None, 0, pa, pb),
                  (ctx, p, -1, 3, p + 64, 1, 0, None, 0, None, 0, pa, pb),
                  (ctx, p, 1, -1, p + 64, 1, 0, None, 0, None, 0, pa, pb),
                  (ctx, p, 1, 3, p + 64, 1, 0, None, -1, None, 0, pa, pb),
                  (ctx, p, 1, 3, p + 64, 1, 0, None, 0, None, -1, pa, pb),
                  (ctx, None, 1, 3, p + 64, 1, 0, None, 0, None, 0, pa, pb),
                  (ctx, p, 1, 3, None, 1, 0, None, 0, None, 0, pa, pb),
                  (ctx, p, 1, 3, p + 64, 1, 0, None, 1, None, 0, pa, pb),
                  (ctx, p, 1, 3, p + 64, 1, 0, None, 0, None, 1, pa, pb),
                  (ctx, p, 1, 3, p + 64, 1, 0, p + 8, 3, None, 0, pa, pb),   # kept vertices overlap the triangles
                  (ctx, p, 1, 3, p + 64, 1, 0, None, 0, p + 68, 1, pa, pb),  # triangles out overlap the labels
                  (ctx, p, 1, 3, p + 64, 1, 0, p + 128, 3, p + 132, 1, pa, pb)]   # the two outputs overlap
    for args in filt_calls:
        assert lib.r3d_mesh_filter_components(*args) == L.ERR_INVALID, args
        assert L.last_error()
    assert (a.value, b.value) == (-7, -9) and not buf.any() and not fake.raw.strip(b"\0")
    big = 2 ** 31
    assert lib.r3d_mesh_components(ctx, p, 0, big, p + 64, None, None, 0, pa, pb) == L.ERR_UNSUPPORTED
    assert lib.r3d_mesh_filter_components(ctx, p, big, 3, p + 64, 1, 0, None, 0, None, 0, pa, pb) == L.ERR_UNSUPPORTED
    assert (a.value, b.value) == (-7, -9)


def test_python_argument_errors_without_gpu():
    M = importlib.import_module(PKG + ".mesh")
    for bad in (0, -1, 1.5, True, None):
        with pytest.raises(ValueError):
            M._min_triangles(bad)
    for bad in (np.zeros((2, 2), np.int32), np.zeros((2, 3), np.float32), np.array([[0, 1, 2**40]])):
        with pytest.raises(ValueError):
            M._triangles(bad)
    assert M._triangles([]).shape == (0, 3) and M._triangles(np.array([[0, 1, 2]], np.int64)).dtype == np.int32
    with pytest.raises(ValueError):
        M.mesh_components(np.zeros((1, 3), np.int32), -1)
    with pytest.raises(ValueError):
        M.remove_small_components(np.zeros((3, 3), np.float64), np.zeros((3, 3), np.float32), [[0, 1, 2]])
    tool = importlib.import_module(PKG + ".other_tools.integrate_tsdf")
    base = ["--voxel-size", "1", "--trunc", "3"]
    for extra in (["--mesh-largest"], ["--mesh-min-component", "5"], ["--mesh", "--mesh-min-component", "0"]):
        with pytest.raises(SystemExit):
            tool.parse_args(base + extra)
    args = tool.parse_args(base + ["--mesh", "--mesh-min-component", "5", "--mesh-largest"])
    assert args.mesh_min_component == 5 and args.mesh_largest


def test_header_has_the_section_and_the_signatures():
    text = open(os.path.join(ROOT, "include", "r3d.h")).read()
    assert "/* ---- Mesh components (csrc/r3d_mesh_cc.hip" in text
    flat = re.sub(r"\s+", " ", text)
    assert ("int r3d_mesh_components(r3d_ctx* ctx, const int32_t* d_tri, int64_t n_triangles, int64_t n_vertices, "
            "uint32_t* d_vertex_label_out, uint32_t* d_tri_label_out, uint32_t* d_comp_out, int64_t cap_components, "
            "int64_t* n_components_out, int64_t* n_invalid_out);") in flat
    assert ("int r3d_mesh_filter_components(r3d_ctx* ctx, const int32_t* d_tri, int64_t n_triangles, int64_t n_vertices, "
            "const uint32_t* d_vertex_label, int64_t min_triangles, int keep_largest, uint32_t* d_kept_vertices_out, "
            "int64_t cap_vertices, int32_t* d_tri_out, int64_t cap_triangles, int64_t* n_vertices_out, "
            "int64_t* n_triangles_out);") in flat
    section = text[text.index("/* ---- Mesh components"):text.index("int r3d_mesh_components(")]
    for phrase in ("SHARED VERTEX", "0xFFFFFFFF", "smallest vertex index", "ascending label", "strictly decreasing", "atomicMin",
                   "ties going to the smallest label", "r3d_gather_rows", "R3D_ERR_UNSUPPORTED", "synchronises once"):
        assert phrase in section, phrase
    src = open(os.path.join(ROOT, PKG, "csrc", "r3d_mesh_cc.hip")).read()
    claims = re.findall(r"r3d_scratch\(\s*ctx,\s*(\w+)", src)                      # its own workspace, none of the shared ones
    assert claims and set(claims) == {"kWsMeshCc"} and src.count("r3d_scratch(") == len(claims)
    assert '#include "r3d_unionfind_dev.h"' in src
    L = importlib.import_module(PKG + "._lib")
    assert "r3d_mesh_components" in L.SIGNATURES and "r3d_mesh_filter_components" in L.SIGNATURES
