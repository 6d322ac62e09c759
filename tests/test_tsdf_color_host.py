"""CPU: the colour rules of the TSDF volume (include/r3d.h, "TSDF colour") in their NumPy restatement (tests/tsdf_color_ref.py) on
closed forms -- what tests/test_gpu_tsdf_color.py asserts of the device is asserted of the specification here first -- plus the
coloured mesh PLY, the library's argument errors and the Python layer's checks, none of which needs a GPU."""
import ctypes as C
import importlib

import numpy as np
import pytest

import tsdf_color_ref as CREF
import tsdf_ref as REF
from helpers import PKG


@pytest.fixture(scope="module")
def L():
    return importlib.import_module(PKG + "._lib")


@pytest.fixture(scope="module")
def T():
    return importlib.import_module(PKG + ".tsdf")


@pytest.fixture(scope="module")
def IO():
    return importlib.import_module(PKG + ".cloud_io")


@pytest.mark.parametrize("n_frames", [1, 3, 7])
@pytest.mark.parametrize("c", [(200, 17, 255), (0, 0, 0), (1, 128, 254)])
def test_reference_wall_of_one_colour(c, n_frames):
    s = CREF.repeated(REF.wall_scene(), n_frames)
    vol, passed, colors = CREF.run(s, CREF.uniform_colors(s, [c] * n_frames))
    assert len(colors) == REF.wall_expected_columns(s) > 0
    assert (colors == np.array(c, np.uint8)).all()            # F c / F = c and c + r * 0 = c, exactly
    assert np.array_equal(vol.n, vol.w.astype(np.uint32)) and np.array_equal(vol.n.astype(np.float32), vol.w)
    assert vol.n.max() == n_frames and passed == int(vol.n.sum())
    assert np.array_equal(vol.sums, vol.n[..., None] * np.array(c, np.uint32))


def test_reference_sums_are_the_accepted_frames_colours():
    s = REF.random_scene((33, 9, 5), 6, np.uint16, (24, 32), seed=1)
    cs = np.array([(255, 0, 10), (3, 250, 77), (90, 91, 92), (0, 0, 0), (255, 255, 255), (17, 200, 31)], np.uint8)
    vol, passed, _ = CREF.run(s, CREF.uniform_colors(s, cs))
    want = np.zeros_like(vol.sums)
    for f in range(6):
        one = REF.Volume(s["origin"], s["vs"], s["dims"], s["tr"])
        REF.integrate(one, s["depths"][f:f + 1], s["poses"][f:f + 1], s["K"], s["scale"])
        assert set(np.unique(one.w)) <= {0.0, 1.0}
        want += one.w.astype(np.uint32)[..., None] * cs[f].astype(np.uint32)
    assert np.array_equal(vol.sums, want) and 0 < passed < 6 * vol.n.size
    assert np.array_equal(vol.n.astype(np.float32), vol.w)


def test_reference_sums_ignore_frame_order_and_splits():
    s = REF.random_scene((65, 3, 2), 9, np.float32, (24, 32), seed=2)
    rgb = CREF.random_colors(s)
    whole, _, colors = CREF.run(s, rgb)
    assert whole.n.max() > 1 and len(colors) > 0
    perm = np.random.default_rng(0).permutation(9)
    assert not np.array_equal(perm, np.arange(9))
    p = dict(s, depths=s["depths"][perm], poses=s["poses"][perm])
    shuffled, _, _ = CREF.run(p, rgb[perm])
    assert np.array_equal(shuffled.sums, whole.sums) and np.array_equal(shuffled.n, whole.n)
    step = CREF.ColorVolume(s["origin"], s["vs"], s["dims"], s["tr"])
    for f in range(9):
        CREF.integrate(step, s["depths"][f:f + 1], rgb[f:f + 1], s["poses"][f:f + 1], s["K"], s["scale"])
    assert np.array_equal(step.sums, whole.sums) and np.array_equal(step.n, whole.n)
    assert np.array_equal(step.tsdf.view(np.uint32), whole.tsdf.view(np.uint32))
    assert np.array_equal(CREF.extract_colors(step), colors)
    for cut in (1, 4, 8):
        two = CREF.ColorVolume(s["origin"], s["vs"], s["dims"], s["tr"])
        CREF.integrate(two, s["depths"][:cut], rgb[:cut], s["poses"][:cut], s["K"], s["scale"])
        CREF.integrate(two, s["depths"][cut:], rgb[cut:], s["poses"][cut:], s["K"], s["scale"])
        assert np.array_equal(two.sums, whole.sums) and np.array_equal(two.n, whole.n)


def test_reference_two_coloured_wall_blends_between_the_colours():
    s = CREF.repeated(REF.wall_scene(), 2)
    left, right = np.array((250, 10, 40), np.uint8), np.array((20, 200, 40), np.uint8)
    rgb = np.empty(s["depths"].shape + (3,), np.uint8)
    rgb[:, :, :16], rgb[:, :, 16:] = left, right
    vol, _, colors = CREF.run(s, rgb)
    lo, hi = np.minimum(left, right), np.maximum(left, right)
    assert len(colors) > 0 and (colors >= lo).all() and (colors <= hi).all()
    assert (colors == left).all(axis=1).any() and (colors == right).all(axis=1).any()


def test_reference_colour_words_and_rounding():
    assert CREF.pack(np.array([[1, 2, 3], [255, 0, 128]], np.uint8)).tolist() == [0x030201, 0x8000ff]
    # two voxels along x with means 10 and 11 and tsdf -1 / +3: r = 0.25, m = 10.25 -> 10; tsdf -1 / +1: m = 10.5 -> 11
    for B, want in ((3.0, 10), (1.0, 11)):
        vol = CREF.ColorVolume((0, 0, 0), 1.0, (2, 1, 1), 1.0)
        vol.tsdf[0, 0] = (-1.0, B)
        vol.w[:] = 2
        vol.n[:] = 2
        vol.sums[0, 0, 0], vol.sums[0, 0, 1] = 20, 22
        assert CREF.extract_colors(vol).tolist() == [[want] * 3]


def test_reference_unseen_volume_has_no_colour():
    s = REF.random_scene((17, 4, 3), 5, np.uint16, (24, 32), seed=3, unseen=True)
    vol, passed, colors = CREF.run(s, CREF.random_colors(s))
    assert passed == 0 and not vol.sums.any() and not vol.n.any() and colors.shape == (0, 3)


# ---- the coloured mesh PLY ----------------------------------------------------------------------------------------------------------
def _tetrahedron():
    xyz = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0], [0, 0, 1.5]], np.float32)
    nrm = np.array([[-1, -1, -1], [1, 0, 0], [0, 1, 0], [0, 0, 1]], np.float32)
    tri = np.array([[0, 2, 1], [0, 1, 3], [0, 3, 2], [1, 2, 3]], np.int32)
    rgb = np.array([[255, 0, 1], [2, 254, 3], [4, 5, 253], [128, 127, 126]], np.uint8)
    return xyz, nrm, tri, rgb


def test_ply_mesh_with_colours_round_trips(IO, tmp_path):
    xyz, nrm, tri, rgb = _tetrahedron()
    a, b, c = [str(tmp_path / n) for n in ("a.ply", "b.ply", "c.ply")]
    IO.write_ply_mesh(a, xyz, nrm, tri, rgb=rgb)
    x2, n2, t2, c2 = IO.read_ply_mesh(a, with_colors=True)
    assert c2.dtype == np.uint8 and np.array_equal(c2, rgb) and np.array_equal(t2, tri) and t2.dtype == np.int32
    assert np.array_equal(x2.view(np.uint32), xyz.view(np.uint32)) and np.array_equal(n2.view(np.uint32), nrm.view(np.uint32))
    x3, n3, t3 = IO.read_ply_mesh(a)                         # the default return is the three arrays, whatever the file holds
    assert np.array_equal(x3, xyz) and np.array_equal(n3, nrm) and np.array_equal(t3, tri)
    data = open(a, "rb").read()
    head = data[:data.index(b"end_header\n")].decode().split("\n")
    assert head[9:12] == ["property uchar red", "property uchar green", "property uchar blue"]
    assert len(data) == data.index(b"end_header\n") + 11 + 27 * 4 + 13 * 4
    xn, nn = IO.read_ply_normals(a)                          # the vertex rows are write_ply_normals(rgb=...)'s
    assert np.array_equal(xn, xyz) and np.array_equal(nn, nrm)
    # without rgb: the bytes of the unchanged call path (four positional arguments), and no colours come back
    IO.write_ply_mesh(b, xyz, nrm, tri)
    IO.write_ply_mesh(c, xyz, nrm, tri, rgb=None)
    plain = open(b, "rb").read()
    assert plain == open(c, "rb").read() and b"red" not in plain
    assert len(plain) == plain.index(b"end_header\n") + 11 + 24 * 4 + 13 * 4
    assert plain[plain.index(b"end_header\n") + 11:][:96] == np.concatenate([xyz, nrm], axis=1).astype("<f4").tobytes()
    assert IO.read_ply_mesh(b, with_colors=True)[3] is None
    # the empty coloured mesh
    IO.write_ply_mesh(c, np.zeros((0, 3), np.float32), np.zeros((0, 3), np.float32), np.zeros((0, 3), np.int32), rgb=np.zeros((0, 3), np.uint8))
    assert [v.shape for v in IO.read_ply_mesh(c, with_colors=True)] == [(0, 3)] * 4


def test_ply_mesh_rejects_a_wrong_rgb(IO, tmp_path):
    import os
    xyz, nrm, tri, rgb = _tetrahedron()
    path = str(tmp_path / "bad.ply")
    for bad in (rgb[:3], rgb[:, :2], rgb.reshape(-1), rgb.astype(np.float32), rgb.astype(np.int32), CREF.pack(rgb)):
        with pytest.raises(ValueError):
            IO.write_ply_mesh(path, xyz, nrm, tri, rgb=bad)
    assert not os.path.exists(path)
    IO.write_ply_mesh(path, xyz, nrm, tri, rgb=rgb)
    data = open(path, "rb").read()
    open(path, "wb").write(data[:-1])                        # too short for its announced rows
    with pytest.raises(ValueError):
        IO.read_ply_mesh(path, with_colors=True)


# ---- the library and the Python layer without a GPU ---------------------------------------------------------------------------------
NAMES = ("r3d_tsdf_create_rgb", "r3d_tsdf_integrate_rgb", "r3d_tsdf_integrate_rgb_host", "r3d_tsdf_colors", "r3d_tsdf_extract_colors")


def test_symbols_are_exported_and_bound(L, T):
    lib = L.load()
    for name in NAMES:
        assert hasattr(lib, name) and name in L.SIGNATURES
    header = open(importlib.import_module("helpers").ROOT + "/include/r3d.h").read()
    for name in NAMES:
        assert "int %s(" % name in header
    for method in ("colors", "colors_device_view", "extract_colors_device"):
        assert callable(getattr(T.TSDFVolume, method))


def test_argument_errors_without_gpu(L):
    lib = L.load()
    origin = (C.c_double * 3)(0.0, 0.0, 0.0)
    h = C.c_void_p(7)
    assert lib.r3d_tsdf_create_rgb(None, origin, 0.1, 4, 4, 4, 0.3, C.byref(h)) == L.ERR_INVALID and h.value is None
    assert lib.r3d_tsdf_create_rgb(None, origin, 0.1, 4, 4, 4, 0.3, None) == L.ERR_INVALID
    pose = (C.c_double * 12)()
    px = (C.c_uint8 * 3)()
    for n_frames, dtype in ((1, L.DEPTH_U8), (-1, L.DEPTH_U8), (1, 7), (0, L.DEPTH_F32)):
        assert lib.r3d_tsdf_integrate_rgb(None, None, None, dtype, n_frames, 1.0, pose, px) == L.ERR_INVALID
        assert lib.r3d_tsdf_integrate_rgb_host(None, None, None, dtype, n_frames, 1.0, pose, px) == L.ERR_INVALID
    n, p = C.c_int64(-7), C.c_void_p(5)
    assert lib.r3d_tsdf_colors(None, C.byref(p), C.byref(n)) == L.ERR_INVALID and n.value == -7 and p.value == 5
    assert lib.r3d_tsdf_colors(None, None, None) == L.ERR_INVALID
    word = C.c_uint32(0xabcdef)
    for mw, cap, out in ((1.0, 0, C.byref(n)), (1.0, 1, C.byref(n)), (1.0, -1, C.byref(n)), (0.0, 1, C.byref(n)), (-1.0, 1, C.byref(n)),
                         (float("nan"), 1, C.byref(n)), (1.0, 1, None)):
        assert lib.r3d_tsdf_extract_colors(None, mw, C.byref(word), cap, out) == L.ERR_INVALID
    assert n.value == -7 and word.value == 0xabcdef
    assert "NULL" in L.last_error()


def _unbound_volume(T, color):
    """a TSDFVolume that never met a device: what the argument checks see before anything is allocated"""
    v = object.__new__(T.TSDFVolume)
    v.handle, v.ctx, v.color, v.dims, v.n_voxels, v.voxel_size = None, None, color, (4, 4, 4), 64, 0.1
    return v


def test_python_layer_rejects_bad_colour_arguments_before_the_gpu(T):
    depth = np.ones((2, 5, 7), np.float32)
    q, t = [[0, 0, 0, 1]] * 2, [[0, 0, 0]] * 2
    rgb = np.zeros((2, 5, 7, 3), np.uint8)
    plain, coloured = _unbound_volume(T, False), _unbound_volume(T, True)
    with pytest.raises(ValueError, match="without colour"):
        plain.integrate(depth, q, t, rgb=rgb)
    with pytest.raises(ValueError, match="missing"):
        coloured.integrate(depth, q, t)
    for bad in (rgb[:1], rgb[:, :4], rgb[..., :2], rgb.astype(np.float32), rgb.astype(np.uint16), rgb.reshape(2, 5, 21), rgb[0],
                np.zeros((2, 7, 5, 3), np.uint8)):
        with pytest.raises(ValueError, match="rgb must be"):
            coloured.integrate(depth, q, t, rgb=bad)
    with pytest.raises(ValueError, match="rgb must be"):
        coloured.integrate(depth[0], q[:1], t[:1], rgb=rgb)             # one raster, two images
    with pytest.raises(ValueError, match="without colour"):
        plain.integrate_device(None, 1, np.uint8, 1, np.zeros((1, 12)), d_rgb=2)
    with pytest.raises(ValueError, match="missing"):
        coloured.integrate_device(None, 1, np.uint8, 1, np.zeros((1, 12)))
    with pytest.raises(ValueError):
        plain.colors()
    for call in (plain.extract_point_cloud, plain.extract_triangle_mesh):
        with pytest.raises(ValueError, match="color=True"):
            call(1.0, with_colors=True)
    with pytest.raises(ValueError):
        coloured.extract_colors_device(0.0, None, 0)
    assert T._unpack_rgba(np.array([0x030201, 0xff8000ff], np.uint32)).tolist() == [[1, 2, 3], [255, 0, 128]]
