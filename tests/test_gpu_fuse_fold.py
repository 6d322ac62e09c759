"""GPU: staging folded into the fused launch ("fuse_stage_fold") and the three-phase tile body of the f32 lane kernel.

Every combination of fuse_stage_fold 0/1 and fuse_prefetch 0/1/2 gives the cloud of the unstaged launch bit for bit -- u8, u16
and f32 depth, with and without pose, at C2's shape, below a tile's width, on ragged rows and over many staging chunks -- and
the staging counter "fuse_sweeps" counts the same staged chunks whether or not the staging is folded."""
import importlib

import numpy as np
import pytest

from helpers import r3d as _r3d
from oracle import fusion_ref as O

pytestmark = pytest.mark.gpu

DEPTHS = {np.uint8: 1.0, np.uint16: 1e-3, np.float32: 1.0}   # depth scale per raster type
DTYPE_IDS = {np.uint8: 0, np.uint16: 1, np.float32: 2}


@pytest.fixture(scope="module")
def R():
    return _r3d()


@pytest.fixture(scope="module")
def ctx(R):
    c = R.Context(0)
    yield c
    c.close()


@pytest.fixture(autouse=True)
def _defaults(ctx):
    yield
    for k, v in (("fuse_stage_fold", 1), ("fuse_prefetch", 0), ("fuse_chunk_mb", 0)):
        ctx.set_tuning(k, v)
    ctx.inputs_fresh()


def raster(rng, dt, F, H, W):
    if dt == np.float32:
        return (rng.random((F, H, W)) * 8).astype(np.float32)
    hi = 256 if dt == np.uint8 else 65536
    return rng.integers(0, hi, size=(F, H, W), dtype=dt)


def run_all(R, ctx, d, pose, chunk_mb=0):
    """{(fold, prefetch): (cloud as u32 bits, sweeps counted)} for one raster, pose table or None"""
    F, H, W = d.shape
    n = F * H * W
    cam = ctx.camera(H, W, *R.REF_INTRINSICS)
    L = importlib.import_module(R.__name__ + "._lib")
    d_depth, d_out = ctx.alloc(d.nbytes).upload(d), ctx.alloc(n * 12)
    d_pose = ctx.alloc(pose.nbytes).upload(pose) if pose is not None else None
    ctx.set_tuning("fuse_chunk_mb", chunk_mb)
    out = {}
    for fold in (0, 1):
        for pf in (0, 1, 2):
            ctx.set_tuning("fuse_stage_fold", fold)
            ctx.set_tuning("fuse_prefetch", pf)
            ctx.inputs_fresh()                      # auto stages only rasters it has not seen: make every launch "fresh"
            L.check(ctx.lib.r3d_memset(ctx.handle, d_out.ptr, 0xff, n * 12))
            s0 = ctx.get_tuning("fuse_sweeps")
            if d_pose is not None:
                R.fuse_frames_device(ctx, cam, d_depth.ptr, d.dtype, F, d_pose.ptr, d_out.ptr, np.float32, DEPTHS[d.dtype.type])
            else:
                R.unproject_device(ctx, cam, d_depth.ptr, d.dtype, F, d_out.ptr, np.float32, DEPTHS[d.dtype.type])
            out[(fold, pf)] = (d_out.download(np.uint32, n * 3), ctx.get_tuning("fuse_sweeps") - s0)
    return out


def check_all(d, out, staged_chunks):
    """every cloud equals the unstaged one; prefetch 2 stages every chunk, auto (0) a fresh raster above its 8 MB floor"""
    want = out[(0, 1)][0]
    auto = staged_chunks if d.nbytes > (8 << 20) else 0
    for key, (bits, sweeps) in out.items():
        assert np.array_equal(bits, want), key
        assert sweeps == {0: auto, 1: 0, 2: staged_chunks}[key[1]], (key, sweeps)
    return want


@pytest.mark.parametrize("dt", [np.uint8, np.uint16, np.float32], ids=["u8", "u16", "f32"])
@pytest.mark.parametrize("with_pose", [True, False], ids=["pose", "nopose"])
@pytest.mark.parametrize("shape", [(3, 13, 97), (5, 3, 1281), (4, 384, 1280)], ids=["97x13", "1281x3", "1280x384"])
def test_fold_and_prefetch_keep_the_bits(R, ctx, dt, with_pose, shape):
    rng = np.random.default_rng([DTYPE_IDS[dt], int(with_pose)] + list(shape))
    F, H, W = shape
    d = raster(rng, dt, F, H, W)
    pose = R.pose_table(rng.normal(size=(F, 4)), rng.normal(size=(F, 3)) * 10) if with_pose else None
    want = check_all(d, run_all(R, ctx, d, pose), 1)
    # ... and that cloud is the reference's
    e_norm, e_comp = O.parity_errors(want.view(np.float32).reshape(-1, 3), reference(R, d.astype(np.float64) * DEPTHS[dt], pose))
    assert e_norm <= 1e-6 and e_comp <= 1e-4, (e_norm, e_comp)


def reference(R, z, pose):
    """fp64 world points: X=(i-cx)/fx*Z, Y=(j-cy)/fy*Z, then Rinv (p - t) with the pose table's Rinv (row-major) and t"""
    F, H, W = z.shape
    fx, fy, cx, cy = R.REF_INTRINSICS
    u = (np.arange(W, dtype=np.float64) - cx) / fx
    v = (np.arange(H, dtype=np.float64) - cy) / fy
    X = u[None, None, :] * z
    Y = v[None, :, None] * z
    p = np.stack([X, Y, z], axis=-1).reshape(F, -1, 3)
    if pose is not None:
        Rinv = pose[:, :9].reshape(F, 3, 3)
        t = pose[:, 9:12]
        p = np.einsum("fij,fnj->fni", Rinv, p - t[:, None, :])
    return p.reshape(-1, 3)


@pytest.mark.parametrize("dt", [np.uint8, np.uint16], ids=["u8", "u16"])
def test_many_chunks_fold_counts_one_sweep_per_chunk(R, ctx, dt):
    """fuse_chunk_mb 1 over a 1280x384 batch: a chunk of 2 (u8) or 1 (u16) frames per launch, each staged chunk counted once"""
    rng = np.random.default_rng(5)
    F, H, W = 9, 384, 1280
    d = raster(rng, dt, F, H, W)
    pose = R.pose_table(rng.normal(size=(F, 4)), rng.normal(size=(F, 3)) * 10)
    frame_bytes = H * W * np.dtype(dt).itemsize
    per_chunk = max(1, (1 << 20) // frame_bytes)
    chunks = -(-F // per_chunk)
    assert chunks >= 5
    check_all(d, run_all(R, ctx, d, pose, chunk_mb=1), chunks)


def test_c2_fold_and_prefetch_keep_the_bits(R, ctx):
    """the headline shape: 100 x 1280x384 u8 frames with poses, 48,000 whole tiles, one staged chunk of 49 MB"""
    rng = np.random.default_rng(2)
    F, H, W = 100, 384, 1280
    d = raster(rng, np.uint8, F, H, W)
    pose = R.pose_table(rng.normal(size=(F, 4)), rng.normal(size=(F, 3)) * 10)
    want = check_all(d, run_all(R, ctx, d, pose), 1)
    fr = rng.choice(F, size=3, replace=False)                   # spot-check three frames against the reference
    got = want.view(np.float32).reshape(F, -1, 3)[fr]
    e_norm, e_comp = O.parity_errors(got, reference(R, d[fr].astype(np.float64), pose[fr]))
    assert e_norm <= 1e-6 and e_comp <= 1e-4, (e_norm, e_comp)
