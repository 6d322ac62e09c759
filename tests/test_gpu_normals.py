"""GPU: normals of an unorganised cloud (r3d_normals_knn; normals.py; cloud_io.write_ply_normals; other_tools/estimate_normals.py)
against tests/normals_ref.py.  The neighbour lists come from the device's own r3d_nn_index_knn_self (pinned against
outliers_ref by test_gpu_outliers.py); counts and covariances are compared bit for bit, normals against numpy.linalg.eigh:

    unit length within 2^-22; direction sin(angle) <= 2^-22 + 1e-12 * l2 / (l1 - l0)

(rounding a unit fp64 vector to f32 turns it by at most sqrt(3) * 2^-25; an fp64 symmetric eigen-solver has backward error of
order 1e-14 |C| and Davis-Kahan gives sin <= 2 |E| / gap; 1e-12 leaves a factor of about 25).  Points with
(l1 - l0) / l2 < 1e-6 are left out of the direction check -- their normal is not determined by the data -- and must instead
satisfy |C n - l0 n| <= 1e-9 * l2 + sqrt(3) * 2^-25 * (l2 - l0).  The second term is the f32 rounding of the stored vector, the
same sqrt(3) * 2^-25 as above: a perturbation d of n changes C n - l0 n by (C - l0) d, up to (l2 - l0) |d|.  Without it the
check cannot be met by any f32 output: numpy.linalg.eigh's own eigenvector rounded to f32 leaves 2.7e-8 .. 4.5e-8 * l2 on the
cube, box-room and sphere clouds of this file (measured on the CPU with normals_ref).  The left-out points are capped at 2 % of
every cloud of continuous random coordinates at k >= 8."""
import ctypes as C
import importlib
import os
import subprocess
import sys

import numpy as np
import pytest

import normals_ref as REF
from helpers import PKG, ROOT, r3d as _r3d
from test_gpu_bounds import Guarded

pytestmark = pytest.mark.gpu

KS = [3, 8, 9, 20, 32]
EPS_LEN = 2.0 ** -22
EPS_F32_TURN = np.sqrt(3.0) * 2.0 ** -25
CONTINUOUS = ("cube20k", "room50k", "boxroom", "sphere")
RADIUS = {"cube20k": 0.046, "room50k": 0.15, "lattice": 0.5, "nonfinite": 0.08, "offset1e4": 0.06, "dups10k": 0.05,
          "boxroom": 0.07, "sphere": 0.04}


@pytest.fixture(scope="module")
def R():
    return _r3d()


@pytest.fixture(scope="module")
def NM(R):
    return importlib.import_module(PKG + ".normals")


@pytest.fixture(scope="module")
def L(R):
    return importlib.import_module(PKG + "._lib")


@pytest.fixture(scope="module")
def ctx(R):
    c = R.Context(0)
    yield c
    c.close()


def _cube(n, seed):
    return np.random.default_rng(seed).random((n, 3)).astype(np.float32)


def _lattice(m, spacing=1.0):
    g = np.stack(np.meshgrid(*[np.arange(m)] * 3, indexing="ij"), -1).reshape(-1, 3)
    return (g.astype(np.float32) * np.float32(spacing))


def _room(R, n, seed=0):
    syn = importlib.import_module(PKG + ".synthetic")
    depth, q, t, K = syn.room_views(6, 120, 160, seed=seed)
    xyz = R.fuse_frames(depth, q, t, intrinsics=K)
    xyz = xyz[np.isfinite(xyz).all(axis=1)]
    return xyz[np.random.default_rng(seed).choice(xyz.shape[0], n, replace=False)]


def _hot(copies, background, seed):
    rng = np.random.default_rng(seed)
    xyz = np.concatenate([np.tile(np.float32([[0.25, 0.5, 0.75]]), (copies, 1)), rng.random((background, 3)).astype(np.float32)])
    return xyz[rng.permutation(xyz.shape[0])]


def _boxroom(n, seed, sigma=0.005, spray=0.01):
    """Six planes of the box [0,4] x [0,3] x [0,2.5] with Gaussian noise sigma along the plane normal + a uniform spray."""
    rng = np.random.default_rng(seed)
    lo, hi = np.zeros(3), np.array([4.0, 3.0, 2.5])
    p = lo + rng.random((n, 3)) * (hi - lo)
    face = rng.integers(0, 6, n)
    ax = face // 2
    p[np.arange(n), ax] = np.where(face % 2 == 0, lo[ax], hi[ax]) + rng.normal(0, sigma, n)
    s = rng.random(n) < spray
    p[s] = lo + rng.random((int(s.sum()), 3)) * (hi - lo)
    return p.astype(np.float32)


def _sphere(n, seed):
    v = np.random.default_rng(seed).normal(size=(n, 3))
    return (v / np.linalg.norm(v, axis=1, keepdims=True)).astype(np.float32)


@pytest.fixture(scope="module")
def clouds(R):
    rng = np.random.default_rng(11)
    bad = _cube(3000, 12)
    bad[rng.choice(3000, 60, replace=False), rng.integers(0, 3, 60)] = np.nan
    bad[rng.choice(3000, 30, replace=False), rng.integers(0, 3, 30)] = np.inf
    bad[5, 0] = -np.inf
    return {"cube20k": _cube(20_000, 1), "room50k": _room(R, 50_000), "lattice": _lattice(14, 0.5), "nonfinite": bad,
            "offset1e4": _cube(8000, 3) + np.float32(1e4), "dups10k": _hot(10_000, 3000, 4), "boxroom": _boxroom(30_000, 5),
            "sphere": _sphere(20_000, 6)}


class Index:
    """A device copy of the cloud and its NNIndex."""

    def __init__(self, ctx, xyz):
        icp = importlib.import_module(PKG + ".icp")
        self.ctx, self.n = ctx, xyz.shape[0]
        self.d_xyz = ctx.alloc(max(xyz.nbytes, 16)).upload(np.ascontiguousarray(xyz, np.float32))
        self.ix = icp.NNIndex(ctx, self.d_xyz.ptr, self.n)

    def close(self):
        self.ix.close()
        self.d_xyz.free()


class Out:
    pass


def device_run(ctx, xyz, k, radius=None, views=None, ppv=1, lists=True):
    """knn_self's lists and r3d_normals_knn's four outputs for one cloud."""
    ix = Index(ctx, xyz)
    n = xyz.shape[0]
    bufs = []
    try:
        def alloc(nbytes):
            bufs.append(ctx.alloc(max(nbytes, 16)))
            return bufs[-1]
        o = Out()
        if lists:
            d_idx, d_d2 = alloc(n * k * 4), alloc(n * k * 4)
            ix.ix.knn_self(k, d_idx.ptr, d_d2.ptr)
            o.idx, o.d2 = d_idx.download(np.uint32, n * k).reshape(n, k), d_d2.download(np.float32, n * k).reshape(n, k)
        d_n, d_c, d_cov, d_m = alloc(n * 12), alloc(n * 4), alloc(n * 48), alloc(n * 4)
        v = None if views is None else np.ascontiguousarray(views, np.float64).reshape(-1, 3)
        ix.ix.normals_knn(k, 0.0 if radius is None else radius, v, ppv, d_n.ptr, d_c.ptr, d_cov.ptr, d_m.ptr)
        o.normals, o.curvature = d_n.download(np.float32, 3 * n).reshape(n, 3), d_c.download(np.float32, n)
        o.cov, o.count = d_cov.download(np.float64, 6 * n).reshape(n, 6), d_m.download(np.uint32, n)
        return o
    finally:
        for b in bufs:
            b.free()
        ix.close()


_RUNS = {}


def run(ctx, clouds, name, k, with_radius):
    key = (name, k, with_radius)
    if key not in _RUNS:
        radius = RADIUS[name] if with_radius else None
        got = device_run(ctx, clouds[name], k, radius)
        _RUNS[key] = (got, REF.normals(clouds[name], got.idx, got.d2, radius))
    return _RUNS[key]


def bits(a):
    return np.ascontiguousarray(a).view(np.uint64 if a.dtype == np.float64 else np.uint32)


def check_normals(got_normals, want, cap=None, label=""):
    """Test 2 of the module docstring for one run: got_normals [N,3] f32 against a normals_ref Result."""
    g = got_normals.astype(np.float64)
    zero = (got_normals == 0).all(axis=1)
    sure = want.plane & ~want.line                               # the plane decision is determined by the data
    assert not zero[sure].any(), "%s: %d points with a plane got a zero normal" % (label, int(zero[sure].sum()))
    assert zero[~want.plane & ~want.line].all(), "%s: a point without a plane got a normal" % label
    rows = np.flatnonzero(sure)
    length = np.linalg.norm(g[rows], axis=1)
    assert np.abs(length - 1.0).max(initial=0.0) <= EPS_LEN, (label, np.abs(length - 1.0).max())
    l = want.l[rows]
    ratio = (l[:, 1] - l[:, 0]) / l[:, 2]
    out = ratio < 1e-6
    print("%s: %d rows, %d left out of the direction check (%.4f %%), %d without a plane" %
          (label, rows.size, int(out.sum()), 100.0 * out.mean() if rows.size else 0.0, int((~want.plane).sum())))
    if cap is not None:
        assert out.sum() <= cap * got_normals.shape[0], "%s: %d of %d points left out" % (label, out.sum(), got_normals.shape[0])
    sin = np.linalg.norm(np.cross(g[rows], want.n[rows]), axis=1)
    bound = EPS_LEN + 1e-12 * l[:, 2] / np.where(out, 1.0, l[:, 1] - l[:, 0])
    worst = (sin / bound)[~out].max(initial=0.0)
    print("%s: worst sin / bound %.3f" % (label, worst))
    assert worst <= 1.0, (label, worst)
    M = REF.matrices(want.cov[rows][out])
    res = np.linalg.norm(np.einsum("nab,nb->na", M, g[rows][out]) - l[out, :1] * g[rows][out], axis=1)
    lim = 1e-9 * l[out, 2] + EPS_F32_TURN * (l[out, 2] - l[out, 0])
    assert (res <= lim).all(), (label, float((res / lim).max()))


# ---- 1. counts and covariance, bit for bit ----------------------------------------------------------------------------------
@pytest.mark.parametrize("with_radius", [False, True], ids=["knn", "hybrid"])
@pytest.mark.parametrize("k", KS)
@pytest.mark.parametrize("name", list(RADIUS))
def test_counts_and_covariance_bits(ctx, clouds, name, k, with_radius):
    got, want = run(ctx, clouds, name, k, with_radius)
    assert np.array_equal(got.count, want.count), np.flatnonzero(got.count != want.count)[:5]
    sure = ~want.line
    bad = np.flatnonzero((bits(got.cov) != bits(want.cov)).any(axis=1) & sure)
    assert bad.size == 0, "%d rows differ, first %d: got %s want %s" % (bad.size, bad[0], got.cov[bad[0]], want.cov[bad[0]])
    # a neighbourhood on one line to within rounding: either decision, but then exactly the zero row or exactly the covariance
    for i in np.flatnonzero(want.line):
        assert (got.cov[i] == 0).all() or np.array_equal(bits(got.cov[i]), bits(want.raw_cov[i]))
    if with_radius and k >= 8:
        assert (got.count < k).any(), "the radius cuts no list: the hybrid search is not exercised"


# ---- 2. normals and curvature against eigh; without viewpoints the largest component is positive ---------------------------
@pytest.mark.parametrize("with_radius", [False, True], ids=["knn", "hybrid"])
@pytest.mark.parametrize("k", KS)
@pytest.mark.parametrize("name", list(RADIUS))
def test_normals_against_eigh(ctx, clouds, name, k, with_radius):
    got, want = run(ctx, clouds, name, k, with_radius)
    cap = 0.02 if name in CONTINUOUS and k >= 8 else None
    check_normals(got.normals, want, cap, "%s k=%d %s" % (name, k, "hybrid" if with_radius else "knn"))
    sure = want.plane & ~want.line
    # curvature: l0 is known to about 1e-16 l2 absolutely, the quotient is rounded to f32 once
    err = np.abs(got.curvature.astype(np.float64) - want.curvature)[sure]
    assert (err <= 1e-12 + 2.0 ** -23 * want.curvature[sure]).all(), err.max()
    assert (got.curvature[(got.normals == 0).all(axis=1)] == 0).all()
    # sign: the component of largest magnitude is positive (a component within f32 rounding of the largest may stand in)
    g = got.normals[sure]
    top = np.abs(g).max(axis=1, keepdims=True)
    assert (np.where(np.abs(g) >= top - 2.0 ** -22, g, -1.0).max(axis=1) > 0).all()


# ---- 3. sign ------------------------------------------------------------------------------------------------------------------
def test_sign_one_viewpoint(ctx, clouds):
    for name, view in (("boxroom", (2.0, 1.5, 1.25)), ("sphere", (0.0, 0.0, 0.0)), ("cube20k", (3.0, -2.0, 0.5))):
        xyz = clouds[name]
        plain, _ = run(ctx, clouds, name, 20, False)
        got = device_run(ctx, xyz, 20, None, views=[view], lists=False)
        dot = (got.normals.astype(np.float64) * (np.float64(view) - xyz.astype(np.float64))).sum(axis=1)
        nz = (got.normals != 0).any(axis=1)
        assert (dot[nz] >= 0).all(), dot[nz].min()
        same = (bits(got.normals) == bits(plain.normals)).all(axis=1)
        neg = (bits(got.normals) == bits(-plain.normals)).all(axis=1)
        assert (same | neg).all() and np.array_equal(bits(got.cov), bits(plain.cov)) and np.array_equal(got.count, plain.count)
        assert np.array_equal(bits(got.curvature), bits(plain.curvature))
        if name == "sphere":                                     # seen from the centre every normal points inwards
            assert ((got.normals * xyz).sum(axis=1)[nz] < 0).all()


def test_sign_per_frame_viewpoints_on_a_fused_room(R, NM, ctx):
    syn = importlib.import_module(PKG + ".synthetic")
    F, H, W, k = 6, 120, 160, 20
    depth, q, t, K = syn.room_views(F, H, W, seed=3)
    xyz = R.fuse_frames(depth, q, t, intrinsics=K)
    views = NM.fused_viewpoints(q, t)
    centres = np.array([-np.linalg.inv(syn.pose_matrix(q[f], t[f])[:3, :3]) @ syn.pose_matrix(q[f], t[f])[:3, 3] for f in range(F)])
    assert np.abs(views - centres).max() <= 1e-12
    plain = device_run(ctx, xyz, k)
    got = device_run(ctx, xyz, k, views=views, ppv=H * W, lists=False)
    want = REF.normals(xyz, plain.idx, plain.d2)
    v = views[np.minimum(np.arange(xyz.shape[0]) // (H * W), F - 1)]
    dot = (got.normals.astype(np.float64) * (v - xyz.astype(np.float64))).sum(axis=1)
    nz = (got.normals != 0).any(axis=1)
    assert nz.mean() > 0.99 and (dot[nz] >= 0).all()
    assert ((bits(got.normals) == bits(plain.normals)).all(axis=1) | (bits(got.normals) == bits(-plain.normals)).all(axis=1)).all()
    # the wall a point lies on, from its coordinates; the inward direction of that wall
    lo, hi = syn.ROOM_LO, syn.ROOM_HI
    on = np.concatenate([np.abs(xyz - lo) < 1e-3, np.abs(xyz - hi) < 1e-3], axis=1)          # [N,6]: lo xyz, hi xyz
    one_wall = on.sum(axis=1) == 1
    wall = on.argmax(axis=1)
    nb_wall = np.take_along_axis(on[plain.idx.astype(np.int64) % xyz.shape[0]], wall[:, None, None], axis=2)[:, :, 0]
    ok = one_wall & nb_wall.all(axis=1) & (plain.idx != REF.NO_ROW).all(axis=1)
    with np.errstate(invalid="ignore", divide="ignore"):
        ok &= want.plane & ((want.l[:, 1] - want.l[:, 0]) / want.l[:, 2] > 1e-3)
    inward = np.where(wall < 3, 1.0, -1.0)
    comp = got.normals[np.arange(xyz.shape[0]), wall % 3] * inward
    assert ok.mean() > 0.5 and (comp[ok] > 0.99).all(), (ok.mean(), comp[ok].min())
    # the single-camera form: view 0 for every row, whatever points_per_view says
    one = device_run(ctx, xyz, k, views=views[:1], ppv=7, lists=False)
    d1 = (one.normals.astype(np.float64) * (views[0] - xyz.astype(np.float64))).sum(axis=1)
    assert (d1[(one.normals != 0).any(axis=1)] >= 0).all()


# ---- 4. rows without a plane --------------------------------------------------------------------------------------------------
def test_no_plane_rows(ctx, clouds):
    for name in ("nonfinite", "dups10k", "cube20k"):
        xyz = clouds[name]
        got, want = run(ctx, clouds, name, 9, True)
        dead = ~np.isfinite(xyz).all(axis=1) | (want.count < 2)
        if name == "dups10k":
            dead |= (xyz == np.float32([0.25, 0.5, 0.75])).all(axis=1)
            assert (want.count[(xyz == np.float32([0.25, 0.5, 0.75])).all(axis=1)] == 9).all()
        assert dead.any()
        for a in (got.normals, got.curvature, got.cov):
            assert (bits(a)[dead] == 0).all()
        assert (got.count[~np.isfinite(xyz).all(axis=1)] == 0).all()
    # appended non-finite rows and far, isolated points change nobody else's result
    xyz = clouds["cube20k"]
    extra = np.full((50, 3), np.nan, np.float32)
    extra[10:20, 1] = np.inf
    extra[20:25] = np.float32(1e3) * (1 + np.arange(5, dtype=np.float32))[:, None]
    extra[45:] = 0.5
    extra[45:, 2] = -np.inf
    base, _ = run(ctx, clouds, "cube20k", 9, True)
    more = device_run(ctx, np.concatenate([xyz, extra]), 9, RADIUS["cube20k"], lists=False)
    n = xyz.shape[0]
    for a, b in ((base.normals, more.normals), (base.curvature, more.curvature), (base.cov, more.cov), (base.count, more.count)):
        assert np.array_equal(bits(a) if a.dtype != np.uint32 else a, bits(b[:n]) if b.dtype != np.uint32 else b[:n])
        assert (bits(b[n:]) == 0).all() if b.dtype != np.uint32 else (b[n:] == 0).all()


# ---- 5. invariance ------------------------------------------------------------------------------------------------------------
def test_two_runs_and_shuffled_rows(ctx, clouds):
    k = 20
    for name in ("boxroom", "lattice"):
        xyz = clouds[name]
        a, want = run(ctx, clouds, name, k, False)
        b = device_run(ctx, xyz, k, lists=False)
        for f in ("normals", "curvature", "cov"):
            assert np.array_equal(bits(getattr(a, f)), bits(getattr(b, f)))
        assert np.array_equal(a.count, b.count)
        p = np.random.default_rng(5).permutation(xyz.shape[0])
        s = device_run(ctx, xyz[p], k)
        # rows whose k + 1 nearest distances are all different: the same members in the same order, hence the same bits
        wide = device_run(ctx, xyz, k + 1)
        tied = (wide.d2[:, 1:] == wide.d2[:, :-1]).any(axis=1)
        assert name == "lattice" or tied.mean() < 0.05
        free = ~tied[p]
        for f in ("normals", "curvature", "cov"):
            assert np.array_equal(bits(getattr(s, f))[free], bits(getattr(a, f)[p])[free]), f
        assert np.array_equal(s.count[free], a.count[p][free])
        check_normals(s.normals, REF.normals(xyz[p], s.idx, s.d2), None, name + " shuffled")


# ---- 6. guard bands, optional outputs, invalid calls --------------------------------------------------------------------------
def test_outputs_stay_inside_their_buffers(ctx, L):
    xyz = _cube(3 * 1024 + 17, 21)
    xyz[7] = np.nan
    n, k = xyz.shape[0], 9
    full = device_run(ctx, xyz, k, 0.08)
    ix = Index(ctx, xyz)
    lib = ctx.lib
    views = np.array([[0.5, 0.5, 5.0], [1.0, 2.0, 3.0]])
    try:
        made = []

        def guards(seed):
            g = [Guarded(ctx, n * 12, 4, seed=seed), Guarded(ctx, n * 4, 4, seed=seed + 1), Guarded(ctx, n * 48, 8, seed=seed + 2),
                 Guarded(ctx, n * 4, 4, seed=seed + 3)]
            made.extend(g)
            return g
        for mask in range(8):                                    # optional outputs NULL in every combination
            gn, gc, gv, gm = guards(10 * mask)
            ix.ix.normals_knn(k, 0.08, None, 1, gn.ptr, gc.ptr if mask & 1 else None, gv.ptr if mask & 2 else None,
                              gm.ptr if mask & 4 else None)
            assert np.array_equal(bits(gn.read(np.float32, (n, 3))), bits(full.normals))
            (assert_eq if mask & 1 else assert_untouched)(gc, np.float32, full.curvature)
            (assert_eq if mask & 2 else assert_untouched)(gv, np.float64, full.cov.reshape(-1))
            (assert_eq if mask & 4 else assert_untouched)(gm, np.uint32, full.count)
        gn, gc, gv, gm = guards(100)
        vp = views.ctypes.data
        bad = [dict(k=2), dict(k=33), dict(k=0), dict(radius=float("nan")), dict(n_views=-1), dict(n_views=2, table=None),
               dict(n_views=2, ppv=0), dict(n_views=1, ppv=-4), dict(normals=None),
               dict(curv=gn.ptr + 8), dict(cov=gn.ptr), dict(count=gc.ptr), dict(cov=gm.ptr - 8), dict(count=gn.ptr + 12 * n - 4), dict(curv=gv.ptr + 40)]
        for case in bad:
            a = dict(k=k, radius=0.08, table=vp, n_views=0, ppv=1, normals=gn.ptr, curv=gc.ptr, cov=gv.ptr, count=gm.ptr)
            a.update(case)
            rc = lib.r3d_normals_knn(ix.ix.handle, a["k"], a["radius"], a["table"], a["n_views"], a["ppv"], a["normals"], a["curv"],
                                     a["cov"], a["count"])
            assert rc == L.ERR_INVALID, case
        assert lib.r3d_normals_knn(None, k, 0.0, None, 0, 1, gn.ptr, None, None, None) == L.ERR_INVALID
        for g in (gn, gc, gv, gm):
            g.unchanged()
        # the index holds its own copy of the cloud (the caller cannot address it): the caller's buffer may even be an output
        ix.ix.normals_knn(k, 0.08, None, 1, ix.d_xyz.ptr)
        assert np.array_equal(bits(ix.d_xyz.download(np.float32, 3 * n).reshape(n, 3)), bits(full.normals))
        for g in made:
            g.free()
    finally:
        ix.close()


def assert_eq(g, dtype, want):
    assert np.array_equal(bits(g.read(dtype)), bits(np.ascontiguousarray(want)))


def assert_untouched(g, dtype, want):
    g.unchanged()


# ---- 7. closed forms ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", [8, 20, 32])
def test_points_on_a_plane(ctx, k):
    g = np.stack(np.meshgrid(np.arange(64), np.arange(64), indexing="ij"), -1).reshape(-1, 2) / 64.0     # dyadic: z is exact
    xyz = np.concatenate([g, (0.25 * g[:, :1] + 0.5 * g[:, 1:])], axis=1).astype(np.float32)
    got = device_run(ctx, xyz, k)
    n0 = np.array([0.25, 0.5, -1.0]) / np.linalg.norm([0.25, 0.5, -1.0])
    want = REF.normals(xyz, got.idx, got.d2)
    assert want.plane.all()
    l = want.l
    bound = EPS_LEN + 1e-12 * l[:, 2] / (l[:, 1] - l[:, 0])
    sin = np.linalg.norm(np.cross(got.normals.astype(np.float64), n0), axis=1)
    assert (sin <= bound).all(), (sin / bound).max()
    assert np.abs(got.curvature).max() <= 1e-12
    check_normals(got.normals, want, 0.0, "plane k=%d" % k)


@pytest.mark.parametrize("k", [8, 20])
def test_points_on_a_sphere(ctx, clouds, k):
    xyz = clouds["sphere"]
    got, _ = run(ctx, clouds, "sphere", k, False)
    h = float(np.sqrt(got.d2[:, k - 1].astype(np.float64).max()))   # the largest k-th neighbour distance found
    dot = np.abs((got.normals.astype(np.float64) * xyz.astype(np.float64)).sum(axis=1))
    print("sphere k=%d: h = %.4f, min |n . p| = %.6f, bound %.6f" % (k, h, dot.min(), 1 - h * h))
    assert (dot >= 1 - h * h).all(), (dot.min(), 1 - h * h)


# ---- 8. through the stack -----------------------------------------------------------------------------------------------------
def test_python_api_ply_and_cli(R, NM, ctx, clouds, tmp_path):
    xyz = clouds["boxroom"]
    dev, _ = run(ctx, clouds, "boxroom", 20, False)
    api = NM.estimate_normals(xyz, ctx=ctx)
    assert np.array_equal(bits(api.normals), bits(dev.normals)) and np.array_equal(bits(api.curvature), bits(dev.curvature))
    assert np.array_equal(api.count, dev.count)
    assert np.array_equal(bits(NM.estimate_covariances(xyz, 20, ctx=ctx)), bits(dev.cov))
    hy, _ = run(ctx, clouds, "boxroom", 9, True)
    api = NM.estimate_normals(xyz, 9, radius=RADIUS["boxroom"], ctx=ctx)
    assert np.array_equal(bits(api.normals), bits(hy.normals)) and np.array_equal(api.count, hy.count)
    assert np.array_equal(bits(NM.estimate_covariances(xyz, 9, RADIUS["boxroom"], ctx=ctx)), bits(hy.cov))
    empty = NM.estimate_normals(np.zeros((0, 3), np.float32), ctx=ctx)
    assert empty.normals.shape == (0, 3) and empty.count.shape == (0,)
    # PLY round trip, and the script on a plain binary PLY
    view = (2.0, 1.5, 1.25)
    api = NM.estimate_normals(xyz, 12, viewpoint=view, ctx=ctx)
    path = str(tmp_path / "n.ply")
    R.cloud_io.write_ply_normals(path, xyz, api.normals, rgb=np.full((xyz.shape[0], 3), 200, np.uint8))
    back_xyz, back_n = R.cloud_io.read_ply_normals(path)
    assert np.array_equal(bits(back_xyz), bits(xyz)) and np.array_equal(bits(back_n), bits(api.normals))
    src, out = str(tmp_path / "in.ply"), str(tmp_path / "out.ply")
    R.cloud_io.write_ply_binary(src, xyz)
    tool = os.path.join(ROOT, PKG, "other_tools", "estimate_normals.py")
    r = subprocess.run([sys.executable, tool, src, out, "--k", "12", "--viewpoint"] + [str(v) for v in view],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    assert "%d points, %d without a normal" % (xyz.shape[0], int((api.normals == 0).all(axis=1).sum())) in r.stdout
    back_xyz, back_n = R.cloud_io.read_ply_normals(out)
    assert np.array_equal(bits(back_xyz), bits(xyz)) and np.array_equal(bits(back_n), bits(api.normals))


def test_point_to_plane_icp_with_estimated_normals(R, NM, ctx):
    syn = importlib.import_module(PKG + ".synthetic")
    icp = importlib.import_module(PKG + ".icp")
    v = syn.two_views(120, 160, yaw_deg=15.0, baseline=(0.35, 0.05, -0.2))
    pa, pb = R.unproject(v["depth_a"], v["K"], ctx=ctx), R.unproject(v["depth_b"], v["K"], ctx=ctx)
    E = np.eye(4)
    E[:3, :3] = [[np.cos(0.08), 0, np.sin(0.08)], [0, 1, 0], [-np.sin(0.08), 0, np.cos(0.08)]]
    E[:3, 3] = (0.05, -0.04, 0.05)
    nrm = NM.estimate_normals(pa, viewpoint=(0, 0, 0), ctx=ctx).normals
    T, info = icp.icp_point_to_plane(pb, pa, tgt_shape=None, tgt_normals=nrm, init=E @ v["T_ab"], ctx=ctx)
    T0, _ = icp.icp_point_to_plane(pb, pa, tgt_shape=(120, 160), init=E @ v["T_ab"], ctx=ctx)
    print("point-to-plane against T_ab: estimated normals %.3e (%d iterations), organised normals %.3e" %
          (np.abs(T - v["T_ab"]).max(), info["iterations"], np.abs(T0 - v["T_ab"]).max()))
    assert np.isfinite(T).all() and np.array_equal(T[3], [0, 0, 0, 1])
    Rm = T[:3, :3]
    assert np.abs(Rm @ Rm.T - np.eye(3)).max() <= 1e-9 and abs(np.linalg.det(Rm) - 1.0) <= 1e-9
