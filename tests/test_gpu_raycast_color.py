"""GPU: r3d_tsdf_raycast_rgb against tests/raycast_color_ref.py, BYTE FOR BYTE on the colour image and BIT FOR BIT on the three
geometry maps, which must also be the bits r3d_tsdf_raycast writes for the same arguments.  tests/test_raycast_color_host.py
asserts the reference against hand-worked values first.  Volumes: one cell, 3 x 2 x 2, 9 x 7 x 5 (reference arrays uploaded into
both planes, some valid voxels with n == 0) and a tsdf_ref.random_scene integrated on the device with noise colours; rasters 1 x 1,
5 x 7 and 17 x 33 (partial 8 x 8 and 16 x 16 tiles on both edges); 1 view and one more than the pose ring's chunk.  Every cast
writes into test_gpu_bounds.Guarded buffers, the colour image at byte offsets 0 to 3."""
import ctypes as C
import functools
import importlib
import os
import shutil
import subprocess
import sys

import numpy as np
import pytest

import mesh_ref as MREF
import raycast_color_ref as RCC
import raycast_ref as RC
import tsdf_color_ref as CREF
import tsdf_ref as REF
from helpers import PKG, ROOT, r3d as _r3d
from test_gpu_bounds import Guarded
from test_gpu_raycast import bits, poses_around, raster_K

pytestmark = pytest.mark.gpu

INF = float("inf")
CHUNK = 32                               # R3D_TSDF_CHUNK (asserted against the package below)


@pytest.fixture(scope="module")
def R():
    return _r3d()


@pytest.fixture(scope="module")
def L(R):
    return importlib.import_module(PKG + "._lib")


@pytest.fixture(scope="module")
def T(R):
    return importlib.import_module(PKG + ".tsdf")


@pytest.fixture(scope="module")
def ctx(R):
    c = R.Context(0)
    yield c
    c.close()


def random_color_volume(dims, seed, invalid):
    """mesh_ref.random_volume's tsdf and weights (0 or 1) in a ColorVolume whose counts are 1 to 4 on the valid voxels -- except for
    one in eight of them, which keeps n == 0 next to sums that are not zero (its mean is 0 by the rule) -- and sums up to 255 n"""
    src = MREF.random_volume(dims, seed, invalid=invalid)
    vol = CREF.ColorVolume(src.o.astype(np.float64), float(src.vs), dims, float(src.tr))
    vol.tsdf, vol.w = src.tsdf, src.w
    rng = np.random.default_rng([seed, 31] + list(dims))
    n = rng.integers(1, 5, vol.n.shape).astype(np.uint32)
    vol.sums = rng.integers(0, 255 * n[..., None] + 1, vol.sums.shape).astype(np.uint32)
    vol.n = np.where((vol.w > 0) & (rng.random(vol.n.shape) >= 0.125), n, 0).astype(np.uint32)
    return vol


# (kind, dims, seed, raster, n_views): "dense" / "holes" = random_color_volume(invalid = 0.0 / 0.1) uploaded, "scene" =
# tsdf_ref.random_scene with tsdf_color_ref.random_colors integrated on the device.  The reference of every case has hits and misses
# (asserted: the seeds are ones for which it does); a 1 x 1 raster has one pixel a view, so it comes with CHUNK + 1 views.
CASES = [
    ("dense", (2, 2, 2), 57, (5, 7), 1),
    ("dense", (2, 2, 2), 39, (1, 1), CHUNK + 1),
    ("holes", (3, 2, 2), 15, (17, 33), 1),
    ("holes", (3, 2, 2), 23, (5, 7), CHUNK + 1),
    ("dense", (9, 7, 5), 5, (17, 33), 1),
    ("holes", (9, 7, 5), 47, (1, 1), CHUNK + 1),
    ("scene", (16, 16, 17), 86, (17, 33), 1),
    ("scene", (16, 16, 17), 86, (5, 7), CHUNK + 1),
]


@functools.lru_cache(maxsize=None)
def case_reference(kind, dims, seed, shape, nv):
    """(reference volume, scene and its colour images or None, poses, K, step, the four reference maps): computed once, never modified"""
    if kind == "scene":
        s = REF.random_scene(dims, 9, np.float32, (24, 32), seed=seed)
        rgb = CREF.random_colors(s, seed)
        ref = CREF.run(s, rgb)[0]
    else:
        s, rgb, ref = None, None, random_color_volume(dims, seed, 0.1 if kind == "holes" else 0.0)
    K, poses, step = raster_K(shape), poses_around(ref, nv, seed), float(ref.vs) * 0.5
    return ref, s, rgb, poses, K, step, RCC.raycast(ref, poses, K, shape, step=step)


def upload(ctx, ptr, array):
    raw = np.ascontiguousarray(array)
    importlib.import_module(PKG + "._lib").check(ctx.lib.r3d_memcpy_h2d(ctx.handle, ptr, raw.ctypes.data, raw.nbytes))


def uploaded(T, ctx, ref):
    """a device volume with colour holding the reference volume's arrays in both planes"""
    V = T.TSDFVolume(ref.o.astype(np.float64), float(ref.vs), (ref.nx, ref.ny, ref.nz), float(ref.tr), ctx=ctx, color=True)
    p, n = V.device_view()
    upload(ctx, p, np.stack([ref.tsdf.reshape(-1), ref.w.reshape(-1)], axis=1).astype(np.float32))
    q, m = V.colors_device_view()
    assert m == n == ref.n.size
    upload(ctx, q, np.concatenate([ref.sums.reshape(-1, 3), ref.n.reshape(-1, 1)], axis=1).astype(np.uint32))
    ctx.sync()
    return V


def integrated(T, ctx, s, rgb):
    V = T.TSDFVolume(s["origin"], s["vs"], s["dims"], s["tr"], ctx=ctx, color=True)
    depths, images = s["depths"], np.ascontiguousarray(rgb)
    f, h, w = depths.shape
    cam = ctx.camera(h, w, *s["K"])
    d_depth, d_rgb = ctx.alloc(depths.nbytes).upload(depths), ctx.alloc(images.nbytes).upload(images)
    V.integrate_device(cam, d_depth.ptr, depths.dtype, f, s["poses"] if "poses" in s else REF.poses_w2c(s["quats"], s["ts"]), s["scale"],
                       d_rgb=d_rgb.ptr)
    ctx.sync()
    d_depth.free()
    d_rgb.free()
    return V


def raw_planes(ctx, V):
    ctx.sync()
    p, n = V.device_view()
    a = np.empty(n * 8, np.uint8)
    ctx.lib.r3d_download(ctx.handle, a.ctypes.data, p, a.nbytes)
    q, _ = V.colors_device_view()
    b = np.empty(n * 16, np.uint8)
    ctx.lib.r3d_download(ctx.handle, b.ctypes.data, q, b.nbytes)
    return a, b


def cast(L, ctx, V, poses, K, shape, want=(True, True, True, True), seed=0, rgb=True, **kw):
    """r3d_tsdf_raycast_rgb (rgb=False: r3d_tsdf_raycast, three outputs) into guarded buffers (asserting the guard bands): the float
    maps at offsets 0, 4, 8 rotated by the seed, the colour image at byte offset seed % 4.  The maps asked for, else None."""
    H, W = shape
    poses = np.ascontiguousarray(poses, dtype=np.float64).reshape(-1, 12)
    nv = len(poses)
    n = nv * H * W
    cam = ctx.camera(H, W, *K)
    offs = [(0, 4, 8)[(j + seed) % 3] for j in range(3)] + [seed % 4]
    sizes, tails, types = (4, 12, 12, 3), ((), (3,), (3,), (3,)), (np.float32,) * 3 + (np.uint8,)
    want = tuple(want) if rgb else tuple(want)[:3]
    g = [Guarded(ctx, n * size, off=off, seed=seed + off) if on else None for on, size, off in zip(want, sizes, offs)]
    args = (V.handle, cam.handle, nv, poses.ctypes.data, kw.get("min_weight", 1.0), kw.get("step", V.voxel_size), kw.get("t_near", 0.0),
            kw.get("t_far", INF)) + tuple(b.ptr if b else None for b in g)
    L.check((ctx.lib.r3d_tsdf_raycast_rgb if rgb else ctx.lib.r3d_tsdf_raycast)(*args))
    out = []
    for b, tail, dtype in zip(g, tails, types):
        out.append(b.bytes().view(dtype).reshape((nv, H, W) + tail) if b else None)
        if b:
            b.free()
    return out


def assert_same(got, want, what=""):
    """the three float maps bit for bit, and the colour image (where both have one) byte for byte"""
    for g, w, name in zip(got, want, ("depth", "vertex", "normal", "rgb")):
        assert g.shape == w.shape and g.dtype == w.dtype, (what, name, g.shape, w.shape, g.dtype, w.dtype)
        a, b = (g, w) if name == "rgb" else (bits(g), bits(w))
        bad = np.flatnonzero(a.reshape(-1) != b.reshape(-1))
        assert bad.size == 0, "%s %s: %d entries differ, first at %d: %r != %r" % (what, name, bad.size, bad[0], g.reshape(-1)[bad[0]], w.reshape(-1)[bad[0]])


def test_chunk_is_what_the_cases_assume(T):
    assert T.CHUNK == CHUNK


@pytest.mark.parametrize("case", CASES, ids=lambda c: "%s-%dx%dx%d-%dx%d-%d" % ((c[0],) + c[1] + c[3] + (c[4],)))
def test_matches_the_reference(T, L, ctx, case):
    kind, dims, seed, shape, nv = case
    ref, s, images, poses, K, step, want = case_reference(*case)
    h = RC.hits(want[1])
    assert h.any() and (~h).any(), (h.sum(), h.size)              # the reference has hits and misses
    assert want[3][h].any() and not want[3][~h].any() and np.array_equal(h, want[0] > 0)
    k = CASES.index(case)
    V = integrated(T, ctx, s, images) if s is not None else uploaded(T, ctx, ref)
    before = raw_planes(ctx, V)
    plain = cast(L, ctx, V, poses, K, shape, seed=k, rgb=False, step=step)        # r3d_tsdf_raycast on the colour volume
    got = cast(L, ctx, V, poses, K, shape, seed=k, step=step)
    again = cast(L, ctx, V, poses, K, shape, seed=k + 1, rgb=False, step=step)    # ... and after the colour call
    assert_same(got, want, "against the reference:")
    assert_same(got[:3], plain, "against r3d_tsdf_raycast:")      # the geometry is that call's, bit for bit
    assert_same(again, plain, "r3d_tsdf_raycast after the colour call:")
    after = raw_planes(ctx, V)
    assert np.array_equal(after[0], before[0]) and np.array_equal(after[1], before[1])      # both planes are only read
    V.close()


WALL_COLORS = ((200, 30, 90), (10, 220, 140))


def test_wall_of_two_colours_is_exact(T, L, ctx):
    """The fronto-parallel wall of tsdf_ref.wall_scene, seen three times with an image that is one colour on its left half (columns
    0 to 15) and another on its right.  A voxel reads pixel ui = floor(40 x / z + 16), so the voxels left of x = 0 (x index 0 to 7;
    no centre lies on x = 0) only ever add the left colour and the others the right one.  In a cell whose eight corners lie in one
    half every mean is (float) (n c) / (float) n = c exactly (n c = 3 * 255 at most, far below 2^24), interpolating equal values
    returns them (M0 + f * 0), and floorf(c + 0.5f) = c: the colour comes back exactly, no tolerance."""
    s = CREF.repeated(REF.wall_scene(), 3)
    left, right = [np.array(c, np.uint8) for c in WALL_COLORS]
    images = np.empty(s["depths"].shape + (3,), np.uint8)
    images[:, :, :16], images[:, :, 16:] = left, right
    ref = CREF.run(s, images)[0]
    gx = ref.centres()[0]
    assert (gx[:8] < 0).all() and (gx[8:] > 0).all() and int(ref.n.max()) == 3
    V = integrated(T, ctx, s, images)
    got = cast(L, ctx, V, s["poses"][:1], s["K"], (24, 32), step=RC.WALL_STEP)
    depth, vertex, _, rgb = [a[0] for a in got]
    h = RC.hits(vertex)
    RC.check_wall(REF.wall_scene(), depth, vertex, got[2][0])
    idx, _ = RCC.hit_cell(ref, [np.ascontiguousarray(vertex[..., a][h]) for a in range(3)])
    in_left, in_right = idx[0] + 1 <= 7, idx[0] >= 8             # the cell's x pair lies wholly in one half
    assert in_left.sum() > 20 and in_right.sum() > 20
    assert (rgb[h][in_left] == left).all() and (rgb[h][in_right] == right).all()
    assert (~h).any() and not rgb[~h].any() and not depth[~h].any()
    assert_same(got, RCC.raycast(ref, s["poses"][:1], s["K"], (24, 32), step=RC.WALL_STEP))
    # the scene's principal point keeps every ray out of the cells that straddle x = 0 (x index 7); half a pixel further, the
    # column ui = 16 runs through them: the halves stay exact, and the straddling cells are the reference's mixture
    K2 = (40.0, 40.0, 16.0, 11.5)
    got = cast(L, ctx, V, s["poses"][:1], K2, (24, 32), seed=2, step=RC.WALL_STEP)
    vertex, rgb = got[1][0], got[3][0]
    h = RC.hits(vertex)
    idx, _ = RCC.hit_cell(ref, [np.ascontiguousarray(vertex[..., a][h]) for a in range(3)])
    in_left, in_right = idx[0] + 1 <= 7, idx[0] >= 8
    assert in_left.sum() > 20 and in_right.sum() > 20 and (~(in_left | in_right)).sum() > 5
    assert (rgb[h][in_left] == left).all() and (rgb[h][in_right] == right).all()
    mixed = rgb[h][~(in_left | in_right)].astype(int)
    assert ((mixed >= np.minimum(left, right)) & (mixed <= np.maximum(left, right))).all()
    assert_same(got, RCC.raycast(ref, s["poses"][:1], K2, (24, 32), step=RC.WALL_STEP))
    V.close()
    # one colour everywhere: that colour on every hit, 0, 0, 0 with depth 0 on every miss
    uniform = CREF.uniform_colors(s, [WALL_COLORS[0]] * 3)
    V = integrated(T, ctx, s, uniform)
    depth, vertex, _, rgb = [a[0] for a in cast(L, ctx, V, s["poses"][:1], s["K"], (24, 32), seed=1, step=RC.WALL_STEP)]
    h = RC.hits(vertex)
    assert h.any() and (~h).any() and np.array_equal(h, depth > 0)
    assert (rgb[h] == left).all() and not rgb[~h].any()
    V.close()


def test_room_round_trip_through_the_python_api(R, ctx):
    """cast a coloured room, integrate the cast depth and colour image into a fresh volume, cast that from the same pose"""
    s = REF.room_scene()
    images = CREF.random_colors(s, 3)
    shape, v = (96, 128), slice(2, 3)
    ref = CREF.ColorVolume(s["origin"], s["vs"], s["dims"], s["tr"])
    poses = REF.poses_w2c(s["quats"], s["ts"])
    CREF.integrate(ref, s["depths"], images, poses, s["K"], s["scale"])
    want = RCC.raycast(ref, poses[v], s["K"], shape)
    ref2 = CREF.ColorVolume(s["origin"], s["vs"], s["dims"], s["tr"])
    CREF.integrate(ref2, want[0], want[3], poses[v], s["K"])
    want2 = RCC.raycast(ref2, poses[v], s["K"], shape)
    h2 = RC.hits(want2[1])
    assert h2.mean() >= 0.5 and len(np.unique(want2[3][h2], axis=0)) > 100
    V = R.TSDFVolume(s["origin"], s["vs"], s["dims"], s["tr"], ctx=ctx, color=True)
    V.integrate(s["depths"], s["quats"], s["ts"], intrinsics=s["K"], depth_scale=s["scale"], rgb=images)
    got = V.raycast(s["quats"][v], s["ts"][v], shape, intrinsics=s["K"], with_colors=True)
    assert len(got) == 4 and got[3].dtype == np.uint8
    assert_same(got, want, "first cast:")
    default = V.raycast(s["quats"][v], s["ts"][v], shape, intrinsics=s["K"])               # the default return is unchanged
    assert len(default) == 3
    assert_same(default, want[:3], "without the flag:")
    empty = V.raycast(s["quats"][:0], s["ts"][:0], (4, 5), with_colors=True)
    assert [a.shape for a in empty] == [(0, 4, 5), (0, 4, 5, 3), (0, 4, 5, 3), (0, 4, 5, 3)] and empty[3].dtype == np.uint8
    V.close()
    V2 = R.TSDFVolume(s["origin"], s["vs"], s["dims"], s["tr"], ctx=ctx, color=True)
    V2.integrate(got[0], s["quats"][v], s["ts"][v], intrinsics=s["K"], rgb=got[3])          # depth and image go back in as they came out
    got2 = V2.raycast(s["quats"][v], s["ts"][v], shape, intrinsics=s["K"], with_colors=True)
    assert_same(got2, want2, "second cast:")
    V2.close()
    P = R.TSDFVolume(s["origin"], s["vs"], s["dims"], s["tr"], ctx=ctx)
    with pytest.raises(ValueError):
        P.raycast(s["quats"][v], s["ts"][v], shape, intrinsics=s["K"], with_colors=True)
    with pytest.raises(ValueError):
        P.raycast_device(ctx.camera(4, 5, *s["K"]), 1, poses[v], None, None, None, d_rgb=1 << 20)
    P.close()


@pytest.fixture(scope="module")
def dense(T, ctx):
    """one uploaded volume shared by the tests that do not vary the shape: (V, ref, poses, K, shape, step, want)"""
    ref = random_color_volume((9, 7, 5), 5, 0.1)
    shape = (17, 33)
    K, poses = raster_K(shape), poses_around(ref, 5, 11)
    want = RCC.raycast(ref, poses, K, shape, step=0.5)
    h = RC.hits(want[1])
    assert h.any() and (~h).any()
    V = uploaded(T, ctx, ref)
    yield V, ref, poses, K, shape, 0.5, want
    V.close()


def test_any_subset_of_outputs_at_every_byte_offset(dense, L, ctx):
    V, ref, poses, K, shape, step, want = dense
    before = raw_planes(ctx, V)
    for mask in range(16):                                        # mask 0: all four NULL, a valid no-op
        on = tuple(bool(mask >> j & 1) for j in range(4))
        got = cast(L, ctx, V, poses, K, shape, want=on, seed=mask, step=step)     # the colour image at byte offset mask % 4
        for j in range(4):
            if on[j]:
                assert_same([got[j]], [want[j]], "mask %d, output %d:" % (mask, j))
            else:
                assert got[j] is None
    for off in range(4):                                          # the image alone and with all maps, at every offset
        assert np.array_equal(cast(L, ctx, V, poses, K, shape, want=(False, False, False, True), seed=off, step=step)[3], want[3])
        assert_same(cast(L, ctx, V, poses, K, shape, seed=4 + off, step=step), want, "offset %d:" % off)
    after = raw_planes(ctx, V)
    assert np.array_equal(after[0], before[0]) and np.array_equal(after[1], before[1])


def test_repeats_and_splits_give_the_same_bytes(dense, L, ctx):
    V, ref, poses, K, shape, step, want = dense
    assert_same(cast(L, ctx, V, poses, K, shape, step=step), want)
    assert_same(cast(L, ctx, V, poses, K, shape, seed=5, step=step), want, "a second run:")
    V.extract_point_cloud(with_colors=True)
    assert_same(cast(L, ctx, V, poses, K, shape, seed=6, step=step), want, "after an extraction:")
    for cut in (1, 3):                                            # the views in two calls
        two = [cast(L, ctx, V, poses[:cut], K, shape, seed=7, step=step), cast(L, ctx, V, poses[cut:], K, shape, seed=8, step=step)]
        assert_same([np.concatenate([t[j] for t in two]) for j in range(4)], want, "split at %d:" % cut)
    for kw in (dict(step=0.25), dict(step=1.0, t_near=3.0), dict(step=0.5, t_far=8.0), dict(step=0.5, min_weight=0.5)):
        assert_same(cast(L, ctx, V, poses, K, shape, **kw), RCC.raycast(ref, poses, K, shape, **kw), "%r:" % (kw,))


def test_invalid_calls_write_nothing(R, T, dense, L, ctx):
    V, ref, poses, K, shape, step, want = dense
    lib = ctx.lib
    H, W = shape
    nv = len(poses)
    n = nv * H * W
    cam = ctx.camera(H, W, *K)
    other = R.Context(0)
    foreign = other.camera(H, W, *K)
    plain = T.TSDFVolume(ref.o.astype(np.float64), float(ref.vs), (ref.nx, ref.ny, ref.nz), float(ref.tr), ctx=ctx)
    gd, gv, gn, gc = Guarded(ctx, n * 4, seed=1), Guarded(ctx, n * 12, off=4, seed=2), Guarded(ctx, n * 12, off=8, seed=3), Guarded(ctx, n * 3, off=1, seed=4)
    guards = (gd, gv, gn, gc)
    before = [g.bytes().copy() for g in guards]
    planes_before = raw_planes(ctx, V)
    p = np.ascontiguousarray(poses).ctypes.data
    vol_ptr, n_vox = V.device_view()
    col_ptr, _ = V.colors_device_view()
    nan = float("nan")
    good = (V.handle, cam.handle, nv, p, 1.0, step, 0.0, INF, gd.ptr, gv.ptr, gn.ptr, gc.ptr)
    names = ("vol", "cam", "n_views", "poses", "mw", "step", "t_near", "t_far", "depth", "vertex", "normal", "rgb")

    def call(**kw):
        args = list(good)
        for k, v in kw.items():
            args[names.index(k)] = v
        return lib.r3d_tsdf_raycast_rgb(*args)

    diag = float(np.sqrt(8.0 ** 2 + 6.0 ** 2 + 4.0 ** 2))
    bad = [dict(vol=None), dict(cam=None), dict(cam=foreign.handle), dict(n_views=-1), dict(poses=None),      # r3d_tsdf_raycast's own
           dict(mw=0.0), dict(mw=-1.0), dict(mw=nan), dict(mw=INF), dict(mw=1e-60),
           dict(step=0.0), dict(step=-0.5), dict(step=nan), dict(step=INF), dict(step=1e-60),
           dict(t_near=-0.1), dict(t_near=nan), dict(t_near=INF), dict(t_far=0.0), dict(t_near=2.0, t_far=2.0), dict(t_near=2.0, t_far=1.0),
           dict(t_far=nan),
           dict(vertex=gd.ptr), dict(normal=gv.ptr + 12), dict(depth=gv.ptr + 4 * 3), dict(depth=vol_ptr), dict(normal=vol_ptr + n_vox * 8 - 4),
           dict(step=diag / 65537.0),
           dict(rgb=gd.ptr), dict(rgb=gd.ptr + n * 4 - 1), dict(rgb=gv.ptr + 5), dict(rgb=gn.ptr + n * 12 - 1),   # the image on another output
           dict(depth=gc.ptr + 1), dict(vertex=gc.ptr + n * 3 - 1),
           dict(rgb=vol_ptr), dict(rgb=vol_ptr + n_vox * 8 - 1),                                                # on the tsdf plane
           dict(rgb=col_ptr), dict(rgb=col_ptr + n_vox * 16 - 1), dict(rgb=col_ptr - n * 3 + 1),                # on the colour plane
           dict(depth=col_ptr), dict(normal=col_ptr + n_vox * 16 - 4)]                                          # a map on the plane it reads
    for kw in bad:
        assert call(**kw) == L.ERR_INVALID, kw
    big = ctx.camera((1 << 24) + 1, 1, *K)
    assert call(cam=big.handle) == L.ERR_INVALID
    # a volume without the colour plane, whatever the pointers and the number of views
    for kw in (dict(), dict(rgb=None), dict(depth=None, vertex=None, normal=None, rgb=None), dict(n_views=0, poses=None)):
        assert call(vol=plain.handle, **kw) == L.ERR_INVALID, kw
        assert "colour" in L.last_error()
    assert call(n_views=0, poses=None) == L.OK
    assert call(depth=None, vertex=None, normal=None, rgb=None) == L.OK       # a valid no-op
    assert call(step=diag / 65000.0, depth=None, vertex=None, normal=None, rgb=None) == L.OK
    for g, b in zip(guards, before):
        assert np.array_equal(g.bytes(), b)
    planes = raw_planes(ctx, V)
    assert np.array_equal(planes[0], planes_before[0]) and np.array_equal(planes[1], planes_before[1])
    assert call() == L.OK                                         # and the good call is good
    got = [g.bytes().view(t).reshape((nv, H, W) + tail) for g, t, tail in zip(guards, (np.float32,) * 3 + (np.uint8,), ((), (3,), (3,), (3,)))]
    assert_same(got, want)
    assert call(rgb=None) == L.OK                                 # without the image: what r3d_tsdf_raycast does
    assert_same([g.bytes().view(np.float32).reshape((nv, H, W) + tail) for g, tail in zip(guards[:3], ((), (3,), (3,)))], want[:3])
    assert np.array_equal(gc.bytes().view(np.uint8).reshape(nv, H, W, 3), want[3])
    for g in guards:
        g.free()
    plain.close()
    other.close()


def test_command_line_with_raycast_color_flag(R, ctx, golden_dir, tmp_path):
    from PIL import Image
    rng = np.random.default_rng(5)
    tool = os.path.join(ROOT, PKG, "other_tools", "integrate_tsdf.py")
    args = ["--voxel-size", "8", "--trunc", "24", "--origin", "-300", "-300", "-300", "--dims", "75", "75", "75", "--min-weight", "1",
            "--color-dir", "rgb", "--mesh", "--raycast"]
    K = (20.0, 20.0, 15.5, 11.5)
    env = dict(os.environ, PYTHONPATH=ROOT, R3D_FX="20", R3D_FY="20", R3D_CX="15.5", R3D_CY="11.5")
    runs = {}
    for where, extra in (("work", ["--raycast-color"]), ("plain", [])):
        d = tmp_path / where
        shutil.copytree(os.path.join(golden_dir, "scene3", "depth"), d / "depth")
        shutil.copytree(os.path.join(golden_dir, "scene3", "camera_pose"), d / "camera_pose")
        if where == "work":
            names, quats, ts = R.read_pose_file(str(d / "camera_pose" / "image_colmap_simi_2.txt"))
            depths = R.cloud_io.read_depth_batch([str(d / "depth" / n) for n in names])
            images = rng.integers(0, 256, depths.shape + (3,), dtype=np.uint8)
        os.makedirs(d / "rgb")
        for name, image in zip(names, images):
            Image.fromarray(image).save(str(d / "rgb" / name))
        r = subprocess.run([sys.executable, tool] + args + extra, cwd=str(d), env=env, capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stdout[-1000:] + r.stderr[-2000:]
        runs[where] = r
    work, plain = tmp_path / "work", tmp_path / "plain"
    line = "raycast colour %d frames -> ./raycast_color/" % len(names)
    assert runs["work"].stdout.split("\n").count(line) == 1
    V = R.TSDFVolume((-300, -300, -300), 8, (75, 75, 75), 24, ctx=ctx, color=True)
    V.integrate(depths, quats, ts, intrinsics=K, rgb=images)
    want = V.raycast(quats, ts, depths.shape[1:], intrinsics=K, with_colors=True)
    V.close()
    assert (want[0] > 0).sum() > 100 and len(np.unique(want[3].reshape(-1, 3), axis=0)) > 100
    assert sorted(os.listdir(str(work / "raycast_color"))) == sorted(n + ".npy" for n in names)
    for k, name in enumerate(names):
        got = np.load(str(work / "raycast_color" / (name + ".npy")))
        assert got.dtype == np.uint8 and got.shape == depths.shape[1:] + (3,) and np.array_equal(got, want[3][k])
        assert np.array_equal(bits(np.load(str(work / "raycast" / (name + ".npy")))), bits(want[0][k]))   # --raycast: depth only, as before
    # without the flag: no directory, the other lines exactly, and every other file byte for byte
    assert not (plain / "raycast_color").exists() and "raycast colour" not in runs["plain"].stdout
    assert runs["plain"].stdout == runs["work"].stdout.replace(line + "\n", "")
    for sub in ("ply", "raycast"):
        assert sorted(os.listdir(str(work / sub))) == sorted(os.listdir(str(plain / sub)))
        for f in os.listdir(str(work / sub)):
            assert open(str(work / sub / f), "rb").read() == open(str(plain / sub / f), "rb").read(), (sub, f)
