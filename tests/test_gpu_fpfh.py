"""GPU: FPFH descriptors (r3d_fpfh_knn; registration.py) against the NumPy restatement of include/r3d.h in tests/register_ref.py.
The neighbour lists come from the device's own r3d_nn_index_knn_self and the normals are an input, so spfh, count and fpfh are
compared bit for bit."""
import importlib

import numpy as np
import pytest

import register_ref as REF
from helpers import PKG, r3d as _r3d
from test_gpu_bounds import Guarded

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def R():
    return _r3d()


@pytest.fixture(scope="module")
def G(R):
    return importlib.import_module(PKG + ".registration")


@pytest.fixture(scope="module")
def L(R):
    return importlib.import_module(PKG + "._lib")


@pytest.fixture(scope="module")
def ctx(R):
    c = R.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def room(R):
    syn = importlib.import_module(PKG + ".synthetic")
    depth, q, t, K = syn.room_views(2, 60, 80, seed=0)
    xyz = R.fuse_frames(depth, q, t, intrinsics=K)
    return np.ascontiguousarray(xyz[np.isfinite(xyz).all(axis=1)], np.float32)


def _clouds(room):
    """name -> (cloud, normals)"""
    out = {"cube": (REF.cube(2000, 1), REF.unit_normals(2000, 2)),
           "room": (room, REF.unit_normals(room.shape[0], 3)),
           "lattice": (REF.lattice(13), REF.axis_normals(13 ** 3, 4)),
           "offset1e4": (REF.cube(3000, 5) + np.float32(1e4), REF.unit_normals(3000, 6))}
    xyz, nrm = REF.cube(2500, 7), REF.unit_normals(2500, 8)
    xyz[::97] = np.nan
    xyz[5::101, 1] = np.inf
    out["nonfinite"] = (xyz, nrm)
    xyz = REF.cube(2000, 9)
    xyz[1000:] = xyz[:1000]                                   # every point twice: d2 = 0 heads every list
    out["duplicates"] = (xyz, REF.unit_normals(2000, 10))
    nrm = REF.unit_normals(2000, 12)
    nrm[::3] = 0
    nrm[1::50, 2] = np.nan
    out["zero_normals"] = (REF.cube(2000, 11), nrm)
    return out


CLOUDS = ["cube", "room", "lattice", "offset1e4", "nonfinite", "duplicates", "zero_normals"]


def device_run(R, G, ctx, xyz, nrm, k, radius, want_optional=True):
    """(fpfh, spfh, count, idx, d2) with the outputs in Guarded buffers."""
    icp = importlib.import_module(PKG + ".icp")
    n = xyz.shape[0]
    d_xyz = ctx.alloc(max(xyz.nbytes, 16)).upload(np.ascontiguousarray(xyz, np.float32))
    gn = Guarded(ctx, n * 12, 4, data=np.ascontiguousarray(nrm, np.float32), seed=1)
    index = icp.NNIndex(ctx, d_xyz.ptr, n)
    d_idx, d_d2 = ctx.alloc(n * k * 4), ctx.alloc(n * k * 4)
    gf = Guarded(ctx, n * 33 * 4, 4, seed=2)
    gs = Guarded(ctx, n * 33, 1, seed=3) if want_optional else None
    gc = Guarded(ctx, n * 4, 4, seed=4) if want_optional else None
    try:
        index.knn_self(k, d_idx.ptr, d_d2.ptr)
        idx, d2 = d_idx.download(np.uint32, n * k).reshape(n, k), d_d2.download(np.float32, n * k).reshape(n, k)
        G.compute_fpfh_device(index, k, gn.ptr, gf.ptr, gs.ptr if gs else None, gc.ptr if gc else None, radius=radius)
        f = gf.read(np.float32, (n, 33))
        gn.unchanged()
        return f, gs.read(np.uint8, (n, 33)) if gs else None, gc.read(np.uint32) if gc else None, idx, d2
    finally:
        index.close()
        for b in (d_xyz, gn, d_idx, d_d2, gf, gs, gc):
            if b is not None:
                b.free()


def check(R, G, ctx, xyz, nrm, k, radius):
    f, s, c, idx, d2 = device_run(R, G, ctx, xyz, nrm, k, radius)
    wf, ws, wc = REF.fpfh(xyz, nrm, idx, d2, radius)
    assert np.array_equal(c, wc), np.flatnonzero(c != wc)[:5]
    bad = np.flatnonzero((s != ws).any(axis=1))
    assert bad.size == 0, "spfh rows differ, first %d: got %s want %s" % (bad[0], s[bad[0]], ws[bad[0]])
    bad = np.flatnonzero((f.view(np.uint32) != wf.view(np.uint32)).any(axis=1))
    assert bad.size == 0, "%d fpfh rows differ, first %d: got %s want %s" % (bad.size, bad[0], f[bad[0]], wf[bad[0]])
    return f, s, c


@pytest.mark.parametrize("k", [3, 8, 32])
@pytest.mark.parametrize("name", CLOUDS)
def test_clouds_bit_for_bit(R, G, ctx, room, name, k):
    xyz, nrm = _clouds(room)[name]
    spacing = {"lattice": 1.5, "room": 0.25, "offset1e4": 0.12}.get(name, 0.1)
    for radius in (None, spacing):
        f, s, c = check(R, G, ctx, xyz, nrm, k, radius)
        assert c.max() <= k and (c > 0).any()
        if name == "nonfinite":
            assert not f[~np.isfinite(xyz).all(axis=1)].any()
        if name == "zero_normals":
            assert not s[::3].any() and (c[::3] == 0).all()


@pytest.mark.parametrize("n", [1, 2, 4, 255, 257])
def test_tiny_clouds(R, G, ctx, n):
    xyz, nrm = REF.cube(n, 20 + n), REF.unit_normals(n, 30 + n)
    f, s, c = check(R, G, ctx, xyz, nrm, 3, None)
    if n == 1:
        assert not f.any() and c[0] == 0


def test_repeatable_optional_outputs_and_host_entry(R, G, ctx):
    xyz, nrm = REF.cube(3001, 40), REF.unit_normals(3001, 41)
    a = device_run(R, G, ctx, xyz, nrm, 16, 0.1)
    b = device_run(R, G, ctx, xyz, nrm, 16, 0.1, want_optional=False)
    assert b[1] is None and b[2] is None and np.array_equal(a[0].view(np.uint32), b[0].view(np.uint32))
    host = G.compute_fpfh(xyz, nrm, k=16, radius=0.1, ctx=ctx)
    assert np.array_equal(host.fpfh.view(np.uint32), a[0].view(np.uint32)) and np.array_equal(host.spfh, a[1])
    assert np.array_equal(host.count, a[2])
    # normals estimated by the call itself: the same as handing them in
    nest = importlib.import_module(PKG + ".normals").estimate_normals(xyz, 16, radius=0.1, ctx=ctx).normals
    own = G.compute_fpfh(xyz, None, k=16, radius=0.1, ctx=ctx)
    assert np.array_equal(own.fpfh.view(np.uint32), G.compute_fpfh(xyz, nest, k=16, radius=0.1, ctx=ctx).fpfh.view(np.uint32))
    assert G.compute_fpfh(np.zeros((0, 3), np.float32), ctx=ctx).fpfh.shape == (0, 33)


def test_invalid_calls_write_nothing(R, L, ctx):
    icp = importlib.import_module(PKG + ".icp")
    n = 500
    xyz, nrm = REF.cube(n, 50), REF.unit_normals(n, 51)
    d_xyz = ctx.alloc(n * 12).upload(xyz)
    index = icp.NNIndex(ctx, d_xyz.ptr, n)
    gn = Guarded(ctx, n * 12, 4, data=nrm, seed=5)
    gf, gs, gc = Guarded(ctx, n * 132, 4, seed=6), Guarded(ctx, n * 33, 1, seed=7), Guarded(ctx, n * 4, 4, seed=8)
    lib = ctx.lib

    def call(ix=index.handle, k=8, radius=0.0, nrm_p=gn.ptr, f_p=gf.ptr, s_p=gs.ptr, c_p=gc.ptr):
        return lib.r3d_fpfh_knn(ix, k, radius, nrm_p, f_p, s_p, c_p)

    for kw in [dict(ix=None), dict(k=2), dict(k=33), dict(k=0), dict(radius=float("nan")), dict(nrm_p=None), dict(f_p=None),
               dict(f_p=gn.ptr), dict(s_p=gn.ptr + 12), dict(s_p=gf.ptr + 4), dict(c_p=gs.ptr), dict(c_p=gf.ptr + 128)]:
        assert call(**kw) == L.ERR_INVALID, kw
        for g in (gn, gf, gs, gc):
            g.unchanged()
    assert call() == 0, L.last_error()
    assert gf.read(np.float32).any()
    index.close()
    for b in (d_xyz, gn, gf, gs, gc):
        b.free()
