"""GPU: voxel-grid downsampling (r3d_voxelgrid_*, voxelmap.VoxelGrid / voxel_down_sample, other_tools/voxel_down_sample.py)
against an fp64 / int64 oracle written here: OctoMap keys and Morton codes from oracle/octomap_ref, then np.unique and
np.add.reduceat.  Codes, counts and colour must be exact; centroids within ulp_f32(m) + res * 2^-28 of the exact mean m;
every output bit independent of runs, insert chunking and host / device insert."""
import ctypes as C
import importlib
import os
import subprocess
import sys

import numpy as np
import pytest

from helpers import PKG, ROOT, r3d as _r3d
from oracle import fusion_ref as O
from oracle import octomap_ref as OM
from test_gpu_bounds import G, Guarded

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def R():
    return _r3d()


@pytest.fixture(scope="module")
def V(R):
    return importlib.import_module(PKG + ".voxelmap")


@pytest.fixture(scope="module")
def L(R):
    return importlib.import_module(PKG + "._lib")


@pytest.fixture(scope="module")
def ctx(R):
    c = R.Context(0)
    yield c
    c.close()


def oracle(xyz, res, rgba=None):
    """(codes, counts, mean xyz fp64, rgba words or None, ignored) of the occupied voxels, ascending code."""
    xyz = np.asarray(xyz, dtype=np.float32)
    k, ok = OM.voxel_keys(xyz, res)
    codes = OM.morton(k[ok])
    order = np.argsort(codes, kind="stable")
    sc = codes[order]
    uniq, start, counts = np.unique(sc, return_index=True, return_counts=True)
    if uniq.size == 0:
        return uniq, counts.astype(np.int64), np.zeros((0, 3)), (None if rgba is None else np.zeros(0, np.uint32)), int((~ok).sum())
    mean = np.add.reduceat(xyz[ok][order].astype(np.float64), start, axis=0) / counts[:, None]
    words = None
    if rgba is not None:
        w = np.asarray(rgba, dtype=np.uint32)[ok][order].astype(np.int64)
        n = counts.astype(np.int64)
        words = np.zeros(uniq.size, np.uint32)
        for c in range(3):
            s = np.add.reduceat((w >> (8 * c)) & 0xff, start)
            words |= ((2 * s + n) // (2 * n)).astype(np.uint32) << np.uint32(8 * c)
    return uniq, counts.astype(np.int64), mean, words, int((~ok).sum())


def assert_matches(got, stats, xyz, res, rgba=None):
    codes, counts, mean, words, ignored = oracle(xyz, res, rgba)
    assert stats["ignored_points"] == ignored and stats["overflow"] == 0
    assert stats["voxels"] == codes.size == got.codes.size
    assert np.array_equal(got.codes, codes)
    assert np.array_equal(got.counts.astype(np.int64), counts)
    tol = np.spacing(np.abs(mean).astype(np.float32)).astype(np.float64) + res * 2.0 ** -28
    err = np.abs(got.xyz.astype(np.float64) - mean)
    assert (err <= tol).all(), "centroid off by %.3g (tol %.3g) at voxel %d" % (err.max(), tol.flat[np.argmax(err - tol)],
                                                                               np.argmax((err - tol).max(axis=1)))
    if rgba is None:
        assert got.rgba is None
    else:
        assert np.array_equal(got.rgba, words)


def run_grid(V, ctx, xyz, res, rgba=None, cap=None):
    vg = V.VoxelGrid(res, cap or max(1 << 10, 2 * len(xyz)), rgba is not None, ctx)
    try:
        vg.insert(xyz, rgba)
        return vg.extract(), vg.stats()
    finally:
        vg.close()


def with_junk(rng, xyz, res, frac=0.01):
    """NaN, inf and out-of-key-range points mixed into the cloud."""
    n = len(xyz)
    m = max(1, int(n * frac))
    idx = rng.choice(n, size=min(m, n), replace=False)
    bad = xyz.copy()
    junk = np.array([np.nan, np.inf, -np.inf, 40000 * res, -40000 * res, 1e30], dtype=np.float32)
    bad[idx, rng.integers(0, 3, size=idx.size)] = junk[rng.integers(0, junk.size, size=idx.size)]
    return bad


def colours(rng, n):
    return rng.integers(0, 1 << 32, size=n, dtype=np.uint64).astype(np.uint32)   # alpha byte set: it must be ignored


PARITY = [(0, 1.0, False, False), (1, 1.0, True, False), (7, 0.2, False, True), (1000, 1.0, True, True),
          (4097, 0.05, False, True), (300_000, 3.0, True, True), (300_000, 30.0, False, False), (1_000_000, 1.0, True, True)]


@pytest.mark.parametrize("n,spread,colour,junk", PARITY)
def test_parity_with_oracle_and_voxel_set(V, ctx, n, spread, colour, junk):
    rng = np.random.default_rng([n, int(spread * 100)])
    res = 0.1
    xyz = (rng.normal(size=(n, 3)) * spread + rng.normal(size=3) * 5).astype(np.float32)
    if junk and n:
        xyz = with_junk(rng, xyz, res)
    rgba = colours(rng, n) if colour else None
    got, st = run_grid(V, ctx, xyz, res, rgba)
    assert_matches(got, st, xyz, res, rgba)
    assert st["ignored_points"] == OM.occupied_set(xyz, res)[1]
    vs = V.VoxelSet(res, max(1 << 10, 2 * n), ctx)
    try:
        vs.insert(xyz)
        assert np.array_equal(vs.codes(), got.codes)
        assert vs.stats()["ignored_points"] == st["ignored_points"]
    finally:
        vs.close()


def test_faces_negatives_tiny_and_key_range_edges(V, ctx):
    rng = np.random.default_rng(11)
    res = 0.1
    pts = []
    k = np.arange(-60, 61)
    face = (k * np.float32(res)).astype(np.float32)                    # exactly on voxel faces, as f32
    for axis in range(3):
        p = rng.uniform(-3, 3, size=(face.size, 3)).astype(np.float32)
        p[:, axis] = face
        pts.append(p)
    neg = -rng.uniform(0, res, size=(500, 3)).astype(np.float32)        # the voxel [-res, 0) on every axis
    tiny = np.array([[0.0, -0.0, 1e-45], [-1e-45, 1e-38, -1e-38], [1e-30, -1e-30, 0.0], [-0.0, -0.0, -0.0]], np.float32)
    lim = np.float32(32768 * res)
    edges = np.array([np.nextafter(lim, np.float32(0)), lim, np.nextafter(lim, np.float32(np.inf)),
                      -lim, np.nextafter(-lim, np.float32(0)), np.nextafter(-lim, np.float32(-np.inf)),
                      np.float32(32767.5 * res), np.float32(-32767.5 * res)], np.float32)
    e = np.stack([edges, np.zeros_like(edges), np.zeros_like(edges)], axis=1)
    pts += [neg, tiny, e, e[:, [1, 0, 2]], e[:, [2, 1, 0]]]
    xyz = np.concatenate(pts).astype(np.float32)
    rgba = colours(rng, len(xyz))
    got, st = run_grid(V, ctx, xyz, res, rgba)
    assert_matches(got, st, xyz, res, rgba)
    assert st["ignored_points"] > 0          # the points beyond the key range
    assert np.array_equal(got.codes, OM.occupied_set(xyz, res)[0])


def test_hot_voxels_with_background(V, ctx):
    """~4 M points in 16 voxels plus a uniform background, shuffled: LDS aggregation and global contention."""
    rng = np.random.default_rng(5)
    res = 0.1
    centres = np.floor(rng.uniform(-20, 20, size=(16, 3)) / res) * res
    hot = centres[rng.integers(0, 16, size=4_000_000)] + rng.uniform(0.001, res - 0.001, size=(4_000_000, 3))
    bg = rng.uniform(-50, 50, size=(300_000, 3))
    xyz = np.concatenate([hot, bg]).astype(np.float32)
    xyz = xyz[rng.permutation(len(xyz))]
    rgba = colours(rng, len(xyz))
    got, st = run_grid(V, ctx, xyz, res, rgba)
    assert_matches(got, st, xyz, res, rgba)
    assert got.counts.max() > 200_000


def test_fused_surfaces_with_colour(R, V, ctx):
    """Frames of slanted planes through fuse_frames_rgb: 3-10 points per voxel, real fused rgba words."""
    F, H, W = 3, 120, 160
    j, i = np.mgrid[0:H, 0:W]
    depths = np.stack([(60 + (i * 0.4 + j * 0.3 + 10 * f)).clip(1, 255).astype(np.uint8) for f in range(F)])
    rng = np.random.default_rng(3)
    q, t = rng.normal(size=(F, 4)), rng.normal(size=(F, 3)) * 2
    rgb = rng.integers(0, 256, size=(F, H, W, 3), dtype=np.uint8)
    xyz, rgba = R.fuse_frames_rgb(depths, rgb, q, t, ctx=ctx)
    e_norm, _ = O.parity_errors(xyz, O.fuse_frames(depths, q, t))
    assert e_norm <= 1e-6
    res = 0.8
    got, st = run_grid(V, ctx, xyz, res, rgba)
    assert 3 <= len(xyz) / st["voxels"] <= 10
    assert_matches(got, st, xyz, res, rgba)
    one = V.voxel_down_sample(xyz, res, rgba, ctx=ctx)
    for a, b in zip(one, got):
        assert np.array_equal(a, b)


def _bits(d):
    return [np.ascontiguousarray(a).view(np.uint8).tobytes() for a in d]


def test_determinism_runs_chunks_and_device_insert(V, ctx):
    rng = np.random.default_rng(9)
    res = 0.05
    n = 400_000
    xyz = np.concatenate([rng.normal(size=(n // 2, 3)), rng.normal(size=(n // 2, 3)) * 0.05]).astype(np.float32)
    rgba = colours(rng, n)
    first, _ = run_grid(V, ctx, xyz, res, rgba)
    again, _ = run_grid(V, ctx, xyz, res, rgba)
    assert _bits(first) == _bits(again)
    cuts = [0, 1, 777, 90_001, 250_000, n]
    chunks = [(cuts[k], cuts[k + 1]) for k in range(5)]
    vg = V.VoxelGrid(res, 2 * n, True, ctx)
    try:
        for k in rng.permutation(5):
            lo, hi = chunks[k]
            vg.insert(xyz[lo:hi], rgba[lo:hi])
        chunked = vg.extract()
        vg.clear()
        d_xyz, d_rgba = ctx.alloc(n * 12).upload(xyz), ctx.alloc(n * 4).upload(rgba)
        vg.insert_device(d_xyz.ptr, n, d_rgba.ptr)
        dev = vg.extract()
        d_xyz.free()
        d_rgba.free()
    finally:
        vg.close()
    assert _bits(chunked) == _bits(first)
    assert _bits(dev) == _bits(first)
    assert_matches(first, {"voxels": first.codes.size, "ignored_points": 0, "overflow": 0}, xyz, res, rgba)


def test_overflow_reports_and_recovers(R, V, L, ctx):
    rng = np.random.default_rng(4)
    res = 0.1
    xyz = rng.uniform(-100, 100, size=(5000, 3)).astype(np.float32)   # ~5000 distinct voxels into 1024 slots
    vg = V.VoxelGrid(res, 1000, False, ctx)
    try:
        vg.insert(xyz)
        st = vg.stats()
        assert st["overflow"] > 0 and st["voxels"] == 1024
        with pytest.raises(R.R3DError) as e:
            vg.extract()
        assert e.value.code == L.ERR_NOMEM
        vg.clear()
        assert vg.stats() == {"voxels": 0, "ignored_points": 0, "overflow": 0}
        vg.insert(xyz[:300])
        got = vg.extract()
        assert_matches(got, vg.stats(), xyz[:300], res)
    finally:
        vg.close()
    got, st = run_grid(V, ctx, xyz, res, cap=1 << 14)
    assert_matches(got, st, xyz, res)


def test_argument_errors_and_guarded_outputs(R, V, L, ctx):
    lib = ctx.lib
    rng = np.random.default_rng(8)
    res = 0.1
    n = 5000
    xyz = (rng.normal(size=(n, 3)) * 2).astype(np.float32)
    rgba = colours(rng, n)
    h = C.c_void_p()
    assert lib.r3d_voxelgrid_create(ctx.handle, res, 1024, 0, None) == L.ERR_INVALID
    assert lib.r3d_voxelgrid_create(ctx.handle, -1.0, 1024, 0, C.byref(h)) == L.ERR_INVALID
    assert lib.r3d_voxelgrid_create(ctx.handle, res, -1, 0, C.byref(h)) == L.ERR_INVALID
    assert lib.r3d_voxelgrid_create(ctx.handle, res, 1024, 6, C.byref(h)) == L.ERR_INVALID
    assert lib.r3d_voxelgrid_insert(None, None, None, 1) == L.ERR_INVALID
    assert lib.r3d_voxelgrid_destroy(None) == 0
    n_out = C.c_int64(-7)
    assert lib.r3d_voxelgrid_extract(None, None, None, None, None, 0, C.byref(n_out)) == L.ERR_INVALID
    plain, colour = V.VoxelGrid(res, 1 << 14, False, ctx), V.VoxelGrid(res, 1 << 14, True, ctx)
    d_xyz, d_rgba = ctx.alloc(n * 12).upload(xyz), ctx.alloc(n * 4).upload(rgba)
    try:
        assert lib.r3d_voxelgrid_insert(plain.handle, d_xyz.ptr, None, -1) == L.ERR_INVALID
        assert lib.r3d_voxelgrid_insert(plain.handle, None, None, 5) == L.ERR_INVALID
        assert lib.r3d_voxelgrid_insert(plain.handle, d_xyz.ptr, d_rgba.ptr, n) == L.ERR_INVALID   # colour, grid without
        assert lib.r3d_voxelgrid_insert(colour.handle, d_xyz.ptr, None, n) == L.ERR_INVALID        # no colour, grid with
        assert lib.r3d_voxelgrid_insert_host(plain.handle, None, None, 5) == L.ERR_INVALID
        with pytest.raises(ValueError):
            plain.insert(xyz, rgba)
        with pytest.raises(ValueError):
            colour.insert(xyz)
        colour.insert_device(d_xyz.ptr, n, d_rgba.ptr)
        plain.insert_device(d_xyz.ptr, n)
        m = colour.extract_device()
        assert m == plain.extract_device() == oracle(xyz, res)[0].size
        want = colour.extract()
        # cap too small: nothing written, *n_out set
        g_small = Guarded(ctx, (m - 1) * 12, 4, seed=1)
        n_out.value = -7
        assert lib.r3d_voxelgrid_extract(colour.handle, g_small.ptr, None, None, None, m - 1, C.byref(n_out)) == L.ERR_INVALID
        assert n_out.value == m
        g_small.unchanged()
        g_small.free()
        # colour out of a grid without colour
        g = Guarded(ctx, m * 4, 4, seed=2)
        assert lib.r3d_voxelgrid_extract(plain.handle, None, g.ptr, None, None, m, C.byref(n_out)) == L.ERR_INVALID
        g.unchanged()
        # overlapping outputs: counts inside the xyz range
        gx = Guarded(ctx, m * 12, 4, seed=3)
        assert lib.r3d_voxelgrid_extract(colour.handle, gx.ptr, None, gx.ptr + 8, None, m, C.byref(n_out)) == L.ERR_INVALID
        gx.unchanged()
        g.free()
        gx.free()
        # every output at a legal, not 16-byte aligned offset inside guard bands
        for off_x, off_c, off_n, off_k in [(4, 4, 4, 8), (12, 8, 20, 24), (0, 0, 0, 0)]:
            gx, gc = Guarded(ctx, m * 12, off_x, seed=4), Guarded(ctx, m * 4, off_c, seed=5)
            gn, gk = Guarded(ctx, m * 4, off_n, seed=6), Guarded(ctx, m * 8, off_k, seed=7)
            assert lib.r3d_voxelgrid_extract(colour.handle, gx.ptr, gc.ptr, gn.ptr, gk.ptr, m + 3, C.byref(n_out)) == 0
            assert n_out.value == m
            assert np.array_equal(gx.read(np.float32, (-1, 3)).view(np.uint32), want.xyz.view(np.uint32))
            assert np.array_equal(gc.read(np.uint32), want.rgba)
            assert np.array_equal(gn.read(np.uint32), want.counts)
            assert np.array_equal(gk.read(np.uint64), want.codes)
            for b in (gx, gc, gn, gk):
                b.free()
        # any subset of the outputs
        gk = Guarded(ctx, m * 8, 8, seed=9)
        assert lib.r3d_voxelgrid_extract(plain.handle, None, None, None, gk.ptr, m, C.byref(n_out)) == 0
        assert np.array_equal(gk.read(np.uint64), want.codes)
        gk.free()
        # the input cloud is only read
        assert np.array_equal(d_xyz.download(np.float32, 3 * n).reshape(-1, 3), xyz)
    finally:
        d_xyz.free()
        d_rgba.free()
        plain.close()
        colour.close()
    assert G == 1 << 20


def test_command_line_tool(V, R, ctx, tmp_path):
    rng = np.random.default_rng(12)
    xyz = (rng.normal(size=(20000, 3)) * 3).astype(np.float32)
    src, dst, dst_bin = tmp_path / "in.ply", tmp_path / "out.ply", tmp_path / "out_bin.ply"
    R.cloud_io.write_ply(str(src), xyz)
    tool = os.path.join(ROOT, PKG, "other_tools", "voxel_down_sample.py")
    r = subprocess.run([sys.executable, tool, str(src), str(dst), "--voxel-size", "0.25"], capture_output=True, text=True,
                       timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    cloud = R.cloud_io.read_ply(str(src)).astype(np.float32)          # what the tool read: the %.4f text of xyz
    want = V.voxel_down_sample(cloud, 0.25, ctx=ctx)
    assert "%d points -> %d voxels (0 ignored)" % (len(cloud), len(want.xyz)) in r.stdout
    got = R.cloud_io.read_ply(str(dst))
    expect = np.array([[float("%.4f" % v) for v in row] for row in want.xyz.astype(np.float64)])
    assert got.shape == expect.shape and np.array_equal(got, expect)
    r = subprocess.run([sys.executable, tool, str(src), str(dst_bin), "--voxel-size", "0.25", "--binary"], capture_output=True,
                       text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert np.array_equal(R.cloud_io.read_ply(str(dst_bin)).astype(np.float32), want.xyz)
