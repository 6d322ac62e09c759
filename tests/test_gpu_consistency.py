"""GPU: the depth consistency filter (r3d_depth_consistency, r3d_depth_consistency_host, r3d_compact_rows_by_mask; consistency.py)
against the NumPy restatement tests/consistency_ref.py, bit for bit: votes, keep and filtered in every case, with every device
output inside a guarded allocation (test_gpu_bounds.Guarded) whose bands must stay untouched.  Shapes are the smallest at which the
kernel can go wrong: 37 x 53 is no multiple of the 32 x 8 workgroup tile or the 32 x 2 wave tile in either direction, 1 x 1 and
1 x 65 leave one row of a tile and cross one tile edge; 6 frames put more than one frame on blockIdx.y."""
import ctypes as C
import importlib

import numpy as np
import pytest

import consistency_ref as CR
from helpers import PKG, r3d as _r3d
from test_gpu_bounds import Guarded

pytestmark = pytest.mark.gpu

F, H, W = 6, 37, 53


@pytest.fixture(scope="module")
def R():
    return _r3d()


@pytest.fixture(scope="module")
def L():
    return importlib.import_module(PKG + "._lib")


@pytest.fixture(scope="module")
def ctx(R):
    c = R.Context(0)
    yield c
    c.close()


def scene(R, frames=F, h=H, w=W, seed=0, behind_last=False, level=False):
    """(depth f32 [frames,h,w] in metres, quats, ts, K): views of the box room a few degrees and decimetres apart, so neighbours
    overlap; 3 % of the pixels halved and 3 % pushed out by 30 %, so all three verdicts of a source occur.  behind_last: the last
    frame stands where frame 0 stands and looks the other way -- every point frame 0 sees has p.z < 0 in it.  level: all cameras
    at one height and without pitch, so the one row of a 1 x w raster maps onto the one row of its neighbours."""
    S = importlib.import_module(PKG + ".synthetic")
    rng = np.random.default_rng(seed)
    depths, quats, ts, K = [], [], [], None
    for f in range(frames):
        c = np.array([0.3, -0.1, 0.2]) + 0.15 * rng.uniform(-1, 1, 3)
        yaw = 0.4 + 0.07 * f
        if behind_last and f == frames - 1:
            c, yaw = centre0, 0.4 + np.pi
        if f == 0:
            centre0 = c
        if level:
            c[1] = -0.1
        z, q, t, K = S.room_view(h, w, yaw, c, pitch=0.0 if level else 0.05 * f)
        depths.append(z.astype(np.float32))
        quats.append(q)
        ts.append(t)
    d = np.stack(depths)
    pick = rng.random(d.shape)
    d[pick < 0.03] *= np.float32(0.5)
    d[(pick >= 0.03) & (pick < 0.06)] *= np.float32(1.3)
    return d, np.array(quats), np.array(ts), K


def quantised(d, dtype):
    """(raster of dtype, depth_scale): metres -> 1/32 m steps in a byte, millimetres in a u16 -- scales other than 1"""
    if dtype == np.uint8:
        return np.clip(np.rint(d * 32.0), 0, 255).astype(np.uint8), 1.0 / 32.0
    if dtype == np.uint16:
        return np.clip(np.rint(d * 1000.0), 0, 65535).astype(np.uint16), 0.001
    return (d * np.float32(4.0)).astype(np.float32), 0.25


def run_device(R, ctx, depths, poses, src, K, scale=1.0, rel_tol=0.03, min_c=2, max_v=0, outputs=("votes", "keep", "filtered"), in_off=0):
    """the device call with the rasters at in_off bytes into a guarded allocation and every requested output guarded too; returns
    {name: array}; the guards of all buffers are checked"""
    f, h, w = depths.shape
    n = f * h * w
    cam = ctx.camera(h, w, *K)
    bufs = {"in": Guarded(ctx, depths.nbytes, in_off, depths, seed=1)}
    sizes = {"votes": 2 * n, "keep": n, "filtered": 4 * n}
    for k, name in enumerate(outputs):
        bufs[name] = Guarded(ctx, sizes[name], 0, seed=2 + k)
    try:
        ptr = {name: bufs[name].ptr if name in bufs else None for name in sizes}
        R.depth_consistency_device(ctx, cam, bufs["in"].ptr, depths.dtype, f, poses, src, ptr["votes"], ptr["keep"], ptr["filtered"],
                                   rel_tol=rel_tol, min_consistent=min_c, max_violations=max_v, depth_scale=scale)
        bufs["in"].unchanged()
        got = {}
        if "votes" in bufs:
            got["votes"] = bufs["votes"].read(np.uint8, (f, h, w, 2))
        if "keep" in bufs:
            got["keep"] = bufs["keep"].read(np.uint8, (f, h, w))
        if "filtered" in bufs:
            got["filtered"] = bufs["filtered"].read(np.float32, (f, h, w))
        return got
    finally:
        for b in bufs.values():
            b.free()


def assert_bits(got, want):
    votes, keep, filtered = want
    if "votes" in got:
        bad = np.argwhere(got["votes"] != votes)
        assert bad.size == 0, "votes differ at %d places, first %s: got %s want %s" % (len(bad), bad[0], got["votes"][tuple(bad[0][:3])],
                                                                                       votes[tuple(bad[0][:3])])
    if "keep" in got:
        assert np.array_equal(got["keep"], keep), "keep differs at %d pixels" % (got["keep"] != keep).sum()
    if "filtered" in got:
        assert np.array_equal(got["filtered"].view(np.uint32), filtered.view(np.uint32)), "filtered differs"


@pytest.fixture(scope="module")
def base(R):
    d, q, t, K = scene(R)
    return d, q, t, K, R.poses_w2c(q, t)


@pytest.mark.parametrize("dtype", [np.uint8, np.uint16, np.float32])
def test_dtypes_with_a_scale(R, ctx, base, dtype):
    d, q, t, K, poses = base
    raster, scale = quantised(d, dtype)
    if dtype == np.float32:                                     # what a float raster may hold besides depths
        flat = raster.reshape(-1)
        flat[5::97] = np.nan
        flat[11::101] = np.inf
        flat[17::103] = -0.0
        flat[23::107] = -2.5
        flat[29::109] = 0.0
        flat[31::113] = -np.inf
    src = R.window_sources(F, 2)
    want = CR.depth_consistency(raster, poses, src, K, 0.03, 2, 0, scale)
    votes = want[0]
    occluded = CR.depth_consistency(raster, poses, src, K, 0.03, 2, 0, scale, with_in_view=True)[3].astype(int) - votes.sum(-1)
    assert votes[..., 0].sum() > 1000 and votes[..., 1].sum() > 100 and occluded.sum() > 100 and 0 < want[1].mean() < 1   # the case has teeth
    assert_bits(run_device(R, ctx, raster, poses, src, K, scale), want)
    if dtype == np.float32:
        assert (want[2].view(np.uint32)[~want[1].astype(bool)] == 0).all()        # +0.0f, never -0.0f or NaN


TABLES = {
    "S=1": lambda R: R.window_sources(F, 2)[:, 1:2],
    "S=16 repeated": lambda R: np.array([[(r + 1 + k % (F - 1)) % F for k in range(16)] for r in range(F)], np.int32),
    "hole in the middle": lambda R: np.array([[(r + 1) % F, -1, (r + 2) % F, -1, (r + F - 1) % F] for r in range(F)], np.int32),
    "a frame without sources": lambda R: np.where(np.arange(F)[:, None] == 2, -1, R.window_sources(F, 1)).astype(np.int32),
}


@pytest.mark.parametrize("name", sorted(TABLES))
def test_source_tables(R, ctx, base, name):
    d, q, t, K, poses = base
    src = TABLES[name](R)
    want = CR.depth_consistency(d, poses, src, K, 0.03, 2, 0)
    if name == "a frame without sources":
        assert not want[0][2].any() and not want[1][2].any() and want[1].any()
    if name == "S=16 repeated":
        assert want[0].max() > 4                                # repeated entries vote more than once
    assert_bits(run_device(R, ctx, d, poses, src, K), want)


def test_only_source_behind_the_frame(R, ctx):
    d, q, t, K = scene(R, behind_last=True)
    poses = R.poses_w2c(q, t)
    src = R.window_sources(F, 1)
    src[0] = [F - 1, -1]
    want = CR.depth_consistency(d, poses, src, K, 0.03, 1, 0, with_in_view=True)
    assert not want[3][0].any() and not want[0][0].any() and not want[1][0].any() and want[1][1:].any()   # p.z <= 0 everywhere
    assert_bits(run_device(R, ctx, d, poses, src, K, min_c=1), want[:3])


@pytest.mark.parametrize("min_c,max_v", [(0, 0), (2, 16), (0, 255), (255, 0)])
def test_thresholds(R, ctx, base, min_c, max_v):
    d, q, t, K, poses = base
    src = R.window_sources(F, 2)
    want = CR.depth_consistency(d, poses, src, K, 0.03, min_c, max_v)
    if (min_c, max_v) == (0, 255):
        assert want[1].all()                                   # every pixel of this scene has a depth
    if min_c == 255:
        assert not want[1].any()
    assert_bits(run_device(R, ctx, d, poses, src, K, min_c=min_c, max_v=max_v), want)


@pytest.mark.parametrize("h,w", [(1, 1), (1, 65)])
def test_thin_rasters(R, ctx, h, w):
    d, q, t, K = scene(R, 3, h, w, seed=4, level=True)
    poses, src = R.poses_w2c(q, t), R.window_sources(3, 1)
    want = CR.depth_consistency(d, poses, src, K, 0.05, 1, 0)
    if w == 65:
        assert want[0].any()
    assert_bits(run_device(R, ctx, d, poses, src, K, rel_tol=0.05, min_c=1), want)


@pytest.mark.parametrize("outputs", [("votes",), ("keep",), ("filtered",)])
def test_each_output_alone(R, ctx, base, outputs):
    d, q, t, K, poses = base
    src = R.window_sources(F, 2)
    want = CR.depth_consistency(d, poses, src, K, 0.03, 2, 0)
    assert_bits(run_device(R, ctx, d, poses, src, K, outputs=outputs), want)


@pytest.mark.parametrize("off", [1, 3])
def test_u8_at_an_odd_address(R, ctx, base, off):
    d, q, t, K, poses = base
    raster, scale = quantised(d, np.uint8)
    src = R.window_sources(F, 2)
    want = CR.depth_consistency(raster, poses, src, K, 0.03, 2, 0, scale)
    assert_bits(run_device(R, ctx, raster, poses, src, K, scale, in_off=off), want)


def test_host_call_is_the_device_call(R, ctx, base):
    d, q, t, K, poses = base
    for dtype in (np.uint16, np.float32):
        raster, scale = quantised(d, dtype)
        want = CR.depth_consistency(raster, poses, R.window_sources(F, 2), K, 0.02, 1, 1, scale)
        cons, viol, keep, filtered = R.depth_consistency(raster, q, t, K, radius=2, rel_tol=0.02, min_consistent=1, max_violations=1,
                                                         depth_scale=scale, ctx=ctx)
        assert keep.dtype == bool and cons.dtype == np.uint8
        assert_bits({"votes": np.stack([cons, viol], -1), "keep": keep.astype(np.uint8), "filtered": filtered}, want)
    cons, viol, keep, filtered = R.depth_consistency(d[0], q[:1], t[:1], K, ctx=ctx)           # one raster: no sources, nothing kept
    assert cons.shape == (1, H, W) and not keep.any() and not filtered.any()


def test_workspace_reuse_between_calls(R, ctx, base):
    """two table widths on one context, the wide one first, give what a fresh context gives for each"""
    d, q, t, K, poses = base
    tables = [TABLES["S=16 repeated"](R), TABLES["S=1"](R), R.window_sources(F, 2)]
    shared = [run_device(R, ctx, d, poses, src, K) for src in tables + tables[:1]]
    for src, got in zip(tables + tables[:1], shared):
        fresh = R.Context(0)
        try:
            want = run_device(R, fresh, d, poses, src, K)
        finally:
            fresh.close()
        for name in want:
            assert np.array_equal(got[name].view(np.uint8), want[name].view(np.uint8)), name
        assert_bits(got, CR.depth_consistency(d, poses, src, K, 0.03, 2, 0))


def test_device_argument_errors(R, L, ctx, base):
    d, q, t, K, poses = base
    cam = ctx.camera(H, W, *K)
    src = R.window_sources(F, 2)
    n = F * H * W
    buf = ctx.alloc(16 * n)
    other = R.Context(0)
    try:
        def call(d_depth, votes, keep, filtered, camera=cam):
            rc = ctx.lib.r3d_depth_consistency(ctx.handle, camera.handle, d_depth, L.DEPTH_F32, F, 1.0, poses.ctypes.data, src.ctypes.data,
                                               src.shape[1], 0.03, 2, 0, votes, keep, filtered)
            return rc, L.last_error()
        p = buf.ptr
        assert call(p, p + 4 * n, p + 6 * n, p + 8 * n)[0] == L.OK
        for args, text in (((None, p + 4 * n, None, None), "NULL depth pointer"), ((p, None, None, None), "no output given"),
                           ((p, p + 4 * n + 1, None, None), "2-byte aligned"),
                           ((p, p + 4 * n - 2, None, None), "overlaps"), ((p, None, p + 4 * n - 1, None), "overlaps"),
                           ((p, None, None, p + 4 * n - 4), "overlaps"), ((p + 8, None, None, p), "overlaps"),
                           ((p, p + 4 * n, p + 6 * n - 1, None), "overlaps"), ((p, None, p + 4 * n, p + 5 * n - 4), "overlaps")):
            rc, msg = call(*args)
            assert rc == L.ERR_INVALID and text in msg, (args, rc, msg)
        rc, msg = call(p, p + 4 * n, None, None, camera=other.camera(H, W, *K))
        assert rc == L.ERR_INVALID and "another context" in msg
        ctx.sync()
    finally:
        other.close()
        buf.free()


# ---- the filtered cloud -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rule", ["some", "all", "none"])
@pytest.mark.parametrize("with_rgb", [False, True])
def test_fuse_frames_consistent_is_a_subsequence(R, ctx, base, rule, with_rgb):
    d, q, t, K, poses = base
    kw = {"some": dict(min_consistent=2, max_violations=0), "all": dict(min_consistent=0, max_violations=255),
          "none": dict(min_consistent=255, max_violations=0)}[rule]
    rgb = np.random.default_rng(3).integers(0, 256, size=(F, H, W, 3), dtype=np.uint8)
    want_keep = CR.depth_consistency(d, poses, R.window_sources(F, 2), K, 0.03, kw["min_consistent"], kw["max_violations"])[1].astype(bool)
    m = int(want_keep.sum())
    assert {"some": 0 < m < d.size and m % 4096 != 0, "all": m == d.size and m % 4096 != 0, "none": m == 0}[rule]   # a partial last tile
    if with_rgb:
        xyz, rgba, keep = R.fuse_frames_consistent(d, q, t, K, radius=2, rel_tol=0.03, rgb=rgb, ctx=ctx, **kw)
        all_xyz, all_rgba = R.fuse_frames_rgb(d, rgb, q, t, K, ctx=ctx)
        assert rgba.dtype == np.uint32 and np.array_equal(rgba, all_rgba[keep.ravel()])
    else:
        xyz, keep = R.fuse_frames_consistent(d, q, t, K, radius=2, rel_tol=0.03, ctx=ctx, **kw)
        all_xyz = R.fuse_frames(d, q, t, K, ctx=ctx)
    assert keep.dtype == bool and np.array_equal(keep, want_keep)
    assert xyz.shape == (m, 3) and xyz.dtype == np.float32
    assert np.array_equal(xyz.view(np.uint32), all_xyz[keep.ravel()].view(np.uint32))


@pytest.mark.parametrize("n", [1, 4095, 4096, 4097, 3 * 4096 + 17])
def test_compact_rows_by_mask(R, L, ctx, n):
    """the call itself at the tile edges of the compaction (4096 rows), outputs guarded: all rows of the mask, a cap below the count
    (only cap rows written, the count still true), the count alone, and the overlap refusal"""
    rng = np.random.default_rng(n)
    xyz = rng.normal(size=(n, 3)).astype(np.float32)
    xyz[rng.random(n) < 0.01] = np.nan
    rgba = rng.integers(0, 1 << 32, size=n, dtype=np.uint32)
    mask = (rng.random(n) < 0.4).astype(np.uint8) * rng.integers(1, 256, size=n).astype(np.uint8)      # any non-zero byte keeps
    mask[-1] = 1
    rows = np.flatnonzero(mask)
    m = len(rows)
    d_xyz, d_rgba, d_mask = Guarded(ctx, xyz.nbytes, 0, xyz, 1), Guarded(ctx, rgba.nbytes, 0, rgba, 2), Guarded(ctx, n, 0, mask, 3)
    made = [d_xyz, d_rgba, d_mask]
    try:
        assert R.compact_rows_device(ctx, d_xyz.ptr, d_rgba.ptr, n, d_mask.ptr, None, None, 0) == m
        for cap, colour in ((m, True), (m, False), (max(m // 2, 1), True), (m + 5, True)):
            o_xyz, o_rgba = Guarded(ctx, cap * 12, 0, seed=4), Guarded(ctx, cap * 4, 0, seed=5)
            made += [o_xyz, o_rgba]
            got = R.compact_rows_device(ctx, d_xyz.ptr, d_rgba.ptr if colour else None, n, d_mask.ptr, o_xyz.ptr, o_rgba.ptr if colour else None, cap)
            assert got == m
            k = min(cap, m)
            out = o_xyz.read(np.uint32, (cap, 3))
            assert np.array_equal(out[:k], xyz[rows[:k]].view(np.uint32))
            assert np.array_equal(out[k:].view(np.uint8).ravel(), o_xyz.pattern[(1 << 20) + 12 * k:(1 << 20) + 12 * cap])   # rows past the count
            words = o_rgba.read(np.uint32)
            if colour:
                assert np.array_equal(words[:k], rgba[rows[:k]])
            else:
                o_rgba.unchanged()
        for g in (d_xyz, d_rgba, d_mask):
            g.unchanged()
        cnt = C.c_int64(-1)
        rc = ctx.lib.r3d_compact_rows_by_mask(ctx.handle, d_xyz.ptr, None, n, d_mask.ptr, d_xyz.ptr + 12 * (n - 1), None, m, C.byref(cnt))
        assert rc == L.ERR_INVALID and "overlaps" in L.last_error()
        rc = ctx.lib.r3d_compact_rows_by_mask(ctx.handle, d_xyz.ptr, None, n, d_mask.ptr, made[3].ptr, made[4].ptr, m, C.byref(cnt))
        assert rc == L.ERR_INVALID and "go together" in L.last_error()
        ctx.sync()
    finally:
        for g in made:
            g.free()


def test_filtered_rasters_integrate_as_they_stand(R, ctx, base):
    """filtered, in HBM, fed to integrate_device (float32, depth_scale 1) gives the volume that integrate() of the restatement's
    filtered rasters gives, bit for bit"""
    d, q, t, K, poses = base
    raster, scale = quantised(d, np.uint16)
    src = R.window_sources(F, 2)
    want = CR.depth_consistency(raster, poses, src, K, 0.03, 2, 0, scale)[2]
    n = F * H * W
    cam = ctx.camera(H, W, *K)
    d_in, d_filtered = ctx.alloc(raster.nbytes).upload(raster), ctx.alloc(4 * n)
    a = R.TSDFVolume((-4.0, -1.5, -3.0), 0.25, (32, 12, 24), 0.5, ctx=ctx)
    b = R.TSDFVolume((-4.0, -1.5, -3.0), 0.25, (32, 12, 24), 0.5, ctx=ctx)
    try:
        R.depth_consistency_device(ctx, cam, d_in.ptr, raster.dtype, F, poses, src, d_filtered=d_filtered.ptr, rel_tol=0.03, depth_scale=scale)
        a.integrate_device(cam, d_filtered.ptr, np.float32, F, poses)
        b.integrate(want, q, t, intrinsics=K)
        (ta, wa), (tb, wb) = a.volume(), b.volume()
        assert wb.max() >= 2 and 0 < (wb > 0).mean() < 1
        assert np.array_equal(ta.view(np.uint32), tb.view(np.uint32)) and np.array_equal(wa.view(np.uint32), wb.view(np.uint32))
    finally:
        a.close()
        b.close()
        d_in.free()
        d_filtered.free()
