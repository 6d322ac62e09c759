"""Seeded inputs at the edges of f32 -- subnormal, overflowing and signed-zero values -- for the kernels whose specification
(include/r3d.h) is a chain of IEEE f32 operations with "f32 denormals kept", and, per case, the facts that prove the case bites:
how many compared elements are subnormal or made from a subnormal operand, and that flush-to-zero arithmetic would give other
bits.  tests/test_f32_edges_host.py asserts those facts of the restatements alone; tests/test_gpu_f32_edges.py compares the device
with the same expectations bit for bit.  Test infrastructure only."""
import functools

import numpy as np

import bilateral_ref as BR
import mesh_ref as MREF
import project_ref as PR
import pyramid_ref as PYR
import raycast_ref as RC
import tsdf_ref as REF

F = np.float32
TINY = np.finfo(F).tiny                   # 2^-126
FLT_MAX = np.finfo(F).max
DENORM_MIN = F(2.0 ** -149)
NO_ROW = np.uint32(0xffffffff)


# ---- helpers ------------------------------------------------------------------------------------------------------------------
def bits(a):
    return np.ascontiguousarray(a, dtype=F).view(np.uint32)


def is_sub(a):
    """elementwise: a non-zero f32 below 2^-126 in magnitude"""
    a = np.asarray(a, dtype=F)
    return (a != 0) & (np.abs(a) < TINY)


def flush(a):
    """what a flush-to-zero unit makes of an f32 operand or result: subnormals become zeros of the same sign"""
    a = np.asarray(a, dtype=F)
    return np.where(is_sub(a), np.copysign(F(0.0), a), a).astype(F)


def same_bits(got, want):
    """equal uint32 words where `want` is not NaN and equal NaN masks (a NaN's sign and payload are the generating unit's: x86
    makes 0xffc00000 of inf - inf, the device 0x7fc00000; neither is part of the contract, as in project_ref.eq_bits)"""
    got, want = np.ascontiguousarray(got, dtype=F), np.ascontiguousarray(want, dtype=F)
    if got.shape != want.shape:
        return False
    nan = np.isnan(want)
    return bool(np.array_equal(np.isnan(got), nan) and np.array_equal(bits(got)[~nan], bits(want)[~nan]))


def first_mismatch(got, want):
    g, w = np.ascontiguousarray(got, dtype=F).reshape(-1), np.ascontiguousarray(want, dtype=F).reshape(-1)
    if g.shape != w.shape:
        return ("shape", g.shape, w.shape)
    bad = np.flatnonzero((np.isnan(g) != np.isnan(w)) | (~np.isnan(w) & (bits(g) != bits(w))))
    return (0,) if bad.size == 0 else (int(bad.size), int(bad[0]), float(g[bad[0]]), float(w[bad[0]]), hex(bits(g)[bad[0]]), hex(bits(w)[bad[0]]))


def random_subnormals(rng, size, signed=True):
    """uniformly drawn non-zero subnormals (1 .. 2^23 - 1 units of 2^-149)"""
    v = rng.integers(1, 1 << 23, size=size).astype(np.uint32).view(F)
    return np.where(rng.random(size) < 0.5, -v, v).astype(F) if signed else v


# ---- case 1: NN and exact k-NN on integer lattices times a power of two ------------------------------------------------------------
NN_SHAPE = (257, 1025)
NN_SCALES = {"tiny": -70, "huge": 64, "large": 60}
KNN_KS = (1, 8, 32)


def _d2_of(D, e):
    """the f32 d2 of the integer squared distance D at scale 2^e: D 2^(2e), exact where it is finite (D < 2^14 has at most 14
    bits), +inf from 2^128 on -- whatever the evaluation order, since every partial sum is such a number too"""
    with np.errstate(over="ignore"):
        return (D.astype(np.float64) * 2.0 ** (2 * e)).astype(F)


@functools.lru_cache(None)
def nn_lattice():
    """(src [257,3], tgt [1025,3]) int64 in [0, 64): a third of the sources sit on a target, targets repeat (ties across tiles)"""
    rng = np.random.default_rng(20240601)
    n, m = NN_SHAPE
    tgt = rng.integers(0, 64, (m, 3))
    tgt[900:] = tgt[:125]                                   # duplicates 900 rows apart: lowest row must win
    src = rng.integers(0, 64, (n, 3))
    src[::3] = tgt[rng.integers(0, m, len(src[::3]))]
    return src, tgt


def nn_case(name):
    """dict(src, tgt f32; idx u32 [n], d2 f32 [n]: the integer answer; facts)"""
    e = NN_SCALES[name]
    si, ti = nn_lattice()
    D = ((si[:, None, :] - ti[None, :, :]) ** 2).sum(-1)                    # int64, exact
    d2 = _d2_of(D, e)
    d2[~np.isfinite(d2)] = np.inf
    idx = np.argmin(d2, axis=1)                                             # first (lowest) index among equals
    best = d2[np.arange(len(idx)), idx]
    idx = np.where(np.isfinite(best), idx, 0).astype(np.uint32)             # no finite distance: (0, +inf)
    src, tgt = (si * 2.0 ** e).astype(F), (ti * 2.0 ** e).astype(F)
    assert np.array_equal(src.astype(np.float64), si * 2.0 ** e) and np.array_equal(tgt.astype(np.float64), ti * 2.0 ** e)
    ftz_idx = np.argmin(flush(d2), axis=1).astype(np.uint32)
    facts = dict(n=len(idx), subnormal=int(is_sub(best).sum()), zero=int((best == 0).sum()), inf=int(np.isinf(best).sum()),
                 ties=int(((d2 == best[:, None]).sum(1) > 1).sum()), ftz_differs=int(((ftz_idx != idx) | (bits(flush(best)) != bits(best))).sum()),
                 pairs_subnormal=int(is_sub(d2).sum()), pairs=int(d2.size))
    return dict(src=src, tgt=tgt, idx=idx, d2=best.astype(F), facts=facts)


def knn_case(name, k=32):
    """dict(xyz f32 [1025,3]; idx u32 [n,k], d2 f32 [n,k]: the integer answer, ascending (d2, row), (0xffffffff, +inf) tails)"""
    e = NN_SCALES[name]
    _, ti = nn_lattice()
    D = ((ti[:, None, :] - ti[None, :, :]) ** 2).sum(-1)
    d2 = _d2_of(D, e)
    d2[~np.isfinite(d2)] = np.inf
    np.fill_diagonal(d2, np.inf)
    order = np.argsort(d2, axis=1, kind="stable")[:, :k]
    dd = np.take_along_axis(d2, order, axis=1)
    idx = np.where(np.isfinite(dd), order, NO_ROW).astype(np.uint32)
    fo = np.argsort(flush(d2), axis=1, kind="stable")[:, :k]
    fd = flush(np.take_along_axis(d2, fo, axis=1))
    facts = dict(n=int(dd.size), subnormal=int(is_sub(dd).sum()), zero=int((dd == 0).sum()), inf=int(np.isinf(dd).sum()),
                 full_rows=int(np.isfinite(dd).all(1).sum()), ftz_differs=int(((fo != order) | (bits(fd) != bits(dd))).sum()))
    return dict(xyz=(ti * 2.0 ** e).astype(F), idx=idx, d2=dd.astype(F), facts=facts)


# ---- case 2: TSDF integration of a scene scaled by 2^-k ------------------------------------------------------------------------------
TSDF_K = 127                               # vs = 0.05 2^-127 and tr = 0.12 2^-127 are subnormal; pc.z ~ (0.3 .. 4) 2^-127 straddles 2^-126
TSDF_CASES = [((65, 3, 2), np.uint16), ((65, 3, 2), np.float32), ((130, 9, 5), np.uint16), ((130, 9, 5), np.float32)]
TSDF_FRAMES, TSDF_RASTER = 33, (24, 32)


def tsdf_scene(dims, dtype, k=TSDF_K):
    """tsdf_ref.random_scene with every length multiplied by 2^-k: origin, voxel size, truncation, pose translations, depth scale.
    The rotations, the intrinsics and the raster's numbers stay, so u, v and sdf / tr are those of the unscaled scene up to the
    roundings of the subnormal range."""
    s = REF.random_scene(dims, TSDF_FRAMES, dtype, TSDF_RASTER, seed=7 + dims[0])
    f = 2.0 ** -k
    s = dict(s)
    s["origin"] = tuple(np.asarray(s["origin"]) * f)
    s["vs"], s["tr"], s["scale"] = s["vs"] * f, s["tr"] * f, s["scale"] * f
    s["poses"] = s["poses"].copy()
    s["poses"][:, 9:] *= f
    return s


def _pcz(s):
    vol = REF.Volume(s["origin"], s["vs"], s["dims"], s["tr"])
    gx, gy, gz = vol.centres()
    X, Y, Z = gx[None, None, :], gy[None, :, None], gz[:, None, None]
    P = s["poses"].astype(F)
    return np.stack([((p[6] * X + p[7] * Y) + p[8] * Z) + p[11] for p in P])


@functools.lru_cache(None)
def tsdf_case(dims, dtype):
    """dict(scene, ref (Volume), passed, xyz, nrm, facts)"""
    s = tsdf_scene(dims, dtype)
    ref, passed, xyz, nrm = REF.run(s)
    z = _pcz(s)
    front = z[z > 0]
    flat = dict(s)                                                           # the inputs as a flushing unit sees them
    flat["origin"] = tuple(float(v) for v in flush(np.asarray(s["origin"], dtype=np.float64).astype(F)))
    flat["vs"], flat["tr"], flat["scale"] = float(flush(F(s["vs"]))), float(flush(F(s["tr"]))), float(flush(F(s["scale"])))
    flat["poses"] = s["poses"].copy()
    flat["poses"][:, 9:] = flush(s["poses"][:, 9:].astype(F))
    fref, fpassed, fxyz, _ = REF.run(flat)
    facts = dict(passed=passed, voxels=int(ref.w.size), seen=int((ref.w > 0).sum()), points=len(xyz),
                 vs_subnormal=bool(is_sub(ref.vs)), tr_subnormal=bool(is_sub(ref.tr)), scale_subnormal=bool(is_sub(F(s["scale"]))),
                 pcz_subnormal=int(is_sub(front).sum()), pcz_normal=int((front >= TINY).sum()),
                 xyz_subnormal=int(is_sub(xyz).sum()), xyz_n=int(xyz.size),
                 ftz_passed=fpassed, ftz_volume_differs=not np.array_equal(bits(fref.tsdf), bits(ref.tsdf)),
                 ftz_points_differ=not (fxyz.shape == xyz.shape and np.array_equal(bits(fxyz), bits(xyz))))
    return dict(scene=s, ref=ref, passed=passed, xyz=xyz, nrm=nrm, facts=facts)


# ---- case 3: volumes written straight into the arrays ---------------------------------------------------------------------------------
VOLUME_DIMS = [(9, 8, 7), (130, 9, 5)]
RAYCAST_SHAPE, RAYCAST_VIEWS = (17, 65), 3
SMALL = F(2.0 ** -64)                     # gradients of this size: m0 m0 + ... is about 2^-128, subnormal


def edge_volume(dims, seed=3):
    """Origin 0, voxel size 1, truncation 3, all weights 1.  Voxels with x below nx / 2 hold tiny values only -- random subnormals,
    +-2^-149, +-(2^-126 - 2^-149), +-0.0, +-2^-126, and values around +-2^-64 whose differences square into the subnormal range;
    the other half mixes ordinary values in (-1, 1) with the tiny ones, and a few neighbouring voxels there hold +-FLT_MAX / 2
    (A - B == FLT_MAX exactly) and +-0.75 FLT_MAX (A - B overflows)."""
    rng = np.random.default_rng([seed] + list(dims))
    nx, ny, nz = dims
    vol = REF.Volume((0.0, 0.0, 0.0), 1.0, dims, 3.0)
    shape = vol.tsdf.shape
    sub = random_subnormals(rng, shape)
    special = rng.choice(np.array([DENORM_MIN, -DENORM_MIN, TINY - DENORM_MIN, -(TINY - DENORM_MIN)], dtype=F), shape)
    zero = np.where(rng.random(shape) < 0.5, F(-0.0), F(0.0)).astype(F)
    tiny = np.where(rng.random(shape) < 0.5, -TINY, TINY).astype(F)
    small = (rng.uniform(-1, 1, shape) * float(SMALL)).astype(F)
    ordinary = rng.uniform(-1, 1, shape).astype(F)
    ordinary[ordinary == 0] = F(0.5)
    pick = rng.random(shape)
    left = np.select([pick < 0.35, pick < 0.45, pick < 0.60, pick < 0.70], [sub, special, zero, tiny], small)
    right = np.select([pick < 0.20, pick < 0.25, pick < 0.35, pick < 0.40], [sub, special, zero, tiny], ordinary)
    t = np.where(np.arange(nx)[None, None, :] < nx // 2, left, right).astype(F)
    x0 = nx - 3
    t[0, 0, x0], t[0, 0, x0 + 1] = FLT_MAX / 2, -FLT_MAX / 2
    t[nz - 1, ny - 1, x0], t[nz - 1, ny - 1, x0 + 1] = -0.75 * FLT_MAX, 0.75 * FLT_MAX
    t[nz - 1, 0, x0], t[nz - 2, 0, x0] = 0.75 * FLT_MAX, -0.75 * FLT_MAX
    vol.tsdf, vol.w = t, np.ones(shape, F)
    return vol


def flushed_volume(vol):
    out = vol.copy()
    out.tsdf = flush(vol.tsdf)
    return out


def _crossings(vol):
    """per axis: (A, B) of every crossing edge"""
    out = []
    for ax in (2, 1, 0):
        A = vol.tsdf
        B = REF._shift(A, ax, 1, A)
        has = REF._shift(np.ones(A.shape, bool), ax, 1, np.zeros(A.shape, bool))
        c = has & ((A < 0) != (B < 0))
        out.append((A[c], B[c]))
    return np.concatenate([a for a, _ in out]), np.concatenate([b for _, b in out])


# The hooks are module-level functions without state: tests/call_order_cases.py memoises tsdf_ref.extract by its pickled arguments
# when it shares a session with this file.
def _sq_ones(sq, total):
    """a squared length of 1: the normals that come back are the unnormalised gradients m themselves"""
    return np.ones_like(total)


def _sq_flush(sq, total):
    """the squared length as a flushing unit forms it: every product and both sums flushed"""
    q = [flush(v) for v in sq]
    return flush(flush(q[0] + q[1]) + q[2])


@functools.lru_cache(None)
def volume_case(dims):
    """dict(vol, xyz, nrm, tri, facts): tsdf_ref.extract / mesh_ref.extract_mesh of edge_volume(dims)"""
    vol = edge_volume(dims)
    xyz, nrm = REF.extract(vol, 1.0)
    _, m = REF.extract(vol, 1.0, squares=_sq_ones)
    with np.errstate(all="ignore"):
        total = (m[:, 0] * m[:, 0] + m[:, 1] * m[:, 1]) + m[:, 2] * m[:, 2]
    assert total.dtype == F
    _, _, tri = MREF.extract_mesh(vol)
    A, B = _crossings(vol)
    with np.errstate(over="ignore"):
        diff = A - B
    neg0 = lambda a: (a == 0) & np.signbit(a)
    fxyz, fnrm = REF.extract(flushed_volume(vol), 1.0, squares=_sq_flush)     # inputs and the squared length's terms flushed
    _, inrm = REF.extract(vol, 1.0, squares=_sq_flush)                        # the squared length's terms alone
    facts = dict(points=len(xyz), triangles=len(tri), crossings_both_subnormal=int((is_sub(A) & is_sub(B)).sum()),
                 crossings_negative_zero=int((neg0(A) | neg0(B)).sum()), crossings_with_subnormal=int((is_sub(A) | is_sub(B)).sum()),
                 difference_overflows=int(np.isinf(diff).sum()), difference_is_flt_max=int((np.abs(diff) == FLT_MAX).sum()),
                 sq_length_subnormal=int(is_sub(total).sum()), sq_length_zero=int((total == 0).sum()),
                 unit_normals_from_subnormal_length=int((is_sub(total) & (np.abs(nrm).sum(1) > 0)).sum()),
                 zero_normals=int((np.abs(nrm).sum(1) == 0).sum()), nan_normals=int(np.isnan(nrm).any(1).sum()),
                 ftz_count_differs=len(fxyz) != len(xyz),
                 ftz_normals_differ_by_squares_alone=int((~np.isnan(nrm) & (bits(inrm) != bits(nrm))).any(1).sum()))
    return dict(vol=vol, xyz=xyz, nrm=nrm, tri=tri, facts=facts)


def raycast_poses(vol, n=RAYCAST_VIEWS, seed=5):
    """look-at cameras outside the volume, one towards the tiny half, one towards the ordinary half, one at the centre"""
    dims = np.array([vol.nx, vol.ny, vol.nz], dtype=np.float64)
    c = dims / 2.0
    r = float(np.linalg.norm(dims)) / 2 + 2.0
    rng = np.random.default_rng([seed, n] + [int(d) for d in dims])
    rows = []
    for v in range(n):
        d = rng.normal(size=3)
        d[2] = -abs(d[2]) - 0.5
        d /= np.linalg.norm(d)
        target = c + np.array([(-0.25, 0.25, 0.0)[v % 3] * dims[0], 0.0, 0.0])
        rows.append(RC.look_at(target + d * r * 1.3, target))
    return np.stack(rows)


def raycast_K(shape=RAYCAST_SHAPE):
    H, W = shape
    f = 1.2 * max(H, W, 4)
    return (f, f, float(W // 2), float(H // 2))


@functools.lru_cache(None)
def raycast_case(dims):
    """dict(vol, poses, K, shape, step, want (depth, vertex, normal), facts)"""
    vol = edge_volume(dims)
    poses, K, step = raycast_poses(vol), raycast_K(), 0.5
    want = RC.raycast(vol, poses, K, RAYCAST_SHAPE, step=step)
    flat = RC.raycast(flushed_volume(vol), poses, K, RAYCAST_SHAPE, step=step)
    h, fh = RC.hits(want[1]), RC.hits(flat[1])
    both = h & fh
    # a hit whose cell holds a subnormal corner is computed from a subnormal operand: the vertex decides the cell
    g = [np.floor(want[1][..., a][h] - F(0.5)) for a in range(3)]
    ix = [np.clip(q.astype(np.int64), 0, n - 2) for q, n in zip(g, (vol.nx, vol.ny, vol.nz))]
    corner_sub = np.zeros(int(h.sum()), bool)
    for k in range(8):
        corner_sub |= is_sub(vol.tsdf[ix[2] + (k >> 2), ix[1] + ((k >> 1) & 1), ix[0] + (k & 1)])
    facts = dict(pixels=int(h.size), hits=int(h.sum()), misses=int((~h).sum()), hits_in_cells_with_subnormal=int(corner_sub.sum()),
                 ftz_hit_mask_differs=int((h != fh).sum()),
                 ftz_depth_differs=int((bits(want[0])[both] != bits(flat[0])[both]).sum()),
                 ftz_normal_differs=int((bits(want[2])[both] != bits(flat[2])[both]).any(-1).sum()))
    return dict(vol=vol, poses=poses, K=K, shape=RAYCAST_SHAPE, step=step, want=want, facts=facts)


# ---- case 4: depth pyramid and bilateral filter ---------------------------------------------------------------------------------------
RASTERS = [(33, 31), (17, 65)]
HALF_MAX_JUMP = float(FLT_MAX)            # every valid tap of a block enters the mean: sums of two huge depths overflow
# The range table is exp(-t^2 / 2), t < 3, whatever sigma_r is: no entry is below 0.011.  The SPATIAL table is the one that can
# underflow: with sigma_s = sqrt(1/2) its entries are exp(-(dx^2 + dy^2)), subnormal for 88 <= dx^2 + dy^2 <= 103 and zero beyond.
BILATERAL = (8, float(np.sqrt(0.5)), 2.0 ** 21)       # radius, sigma_s, sigma_r: cut = 3 2^21 keeps every finite pair below 2^22


def edge_depth(h, w, seed=1):
    """Left 60 % of the columns: subnormal positives and normals below 2^-120, with a few isolated depths of about 2^20 (their
    table weight times 2^20 is all that a far tap adds to a tiny sum).  The rest: ordinary depths 0.5 .. 4 next to subnormal ones,
    and the invalid kinds.  A 2 x 2 block of 0.9 FLT_MAX at an even position: its sum overflows."""
    rng = np.random.default_rng([seed, h, w])
    d = np.empty((h, w), F)
    sub = random_subnormals(rng, (h, w), signed=False)
    low = (rng.uniform(1, 2, (h, w)) * 2.0 ** rng.integers(-126, -119, (h, w))).astype(F)
    pick = rng.random((h, w))
    left = np.where(pick < 0.6, sub, low)
    left = np.where(pick > 0.994, (rng.uniform(1, 2, (h, w)) * 2.0 ** 20).astype(F), left)
    ordinary = rng.uniform(0.5, 4.0, (h, w)).astype(F)
    right = np.where(pick < 0.3, sub, ordinary)
    for k, bad in enumerate([0.0, -1.5, np.nan, np.inf, -np.inf, -float(DENORM_MIN)]):
        right = np.where((pick >= 0.9 + 0.015 * k) & (pick < 0.9 + 0.015 * (k + 1)), F(bad), right)
    split = (3 * w) // 5
    d[:, :split], d[:, split:] = left[:, :split], right[:, split:]
    d[h - 3, 2], d[2, 4] = DENORM_MIN, TINY - DENORM_MIN
    d[4:6, w - 4:w - 2] = F(0.9) * FLT_MAX
    return d.astype(F)


@functools.lru_cache(None)
def half_case(h, w):
    d = edge_depth(h, w)
    want = PYR.depth_half(d, HALF_MAX_JUMP)
    flat = PYR.depth_half(flush(d), HALF_MAX_JUMP)
    oh, ow = want.shape
    blocks = d[:2 * oh, :2 * ow].reshape(oh, 2, ow, 2)
    from_sub = (is_sub(blocks) & (blocks > 0)).any(axis=(1, 3))
    facts = dict(outputs=int(want.size), subnormal=int(is_sub(want).sum()), from_subnormal=int(from_sub.sum()), inf=int(np.isinf(want).sum()),
                 ftz_differs=int((bits(flush(flat)) != bits(want)).sum()))
    return dict(depth=d, max_jump=HALF_MAX_JUMP, want=want, facts=facts)


def bilateral_tables():
    """the restatement's tables (np.exp): the host test compares the library's with these entry by entry"""
    return BR.weights(*BILATERAL)


def bilateral_expect(d, tables, ftz=False):
    """bilateral_ref.depth_bilateral; ftz: on flushed depths with flushed tables (the weight products' subnormal operand) and a
    flushed result"""
    with np.errstate(over="ignore"):                                          # the block of 0.9 FLT_MAX: num overflows, by design
        if not ftz:
            return BR.depth_bilateral(d, BILATERAL[0], *tables)
        spatial, rng, cut, inv_step = tables
        return flush(BR.depth_bilateral(flush(d), BILATERAL[0], flush(spatial), flush(rng), cut, inv_step))


def bilateral_facts(d, tables):
    want = bilateral_expect(d, tables)
    spatial = np.asarray(tables[0], dtype=F)
    ok = BR.valid(d)
    with np.errstate(over="ignore"):
        tables_only = BR.depth_bilateral(d, BILATERAL[0], flush(spatial), *tables[1:])  # the subnormal weights alone flushed
    return dict(outputs=int(want.size), valid=int(ok.sum()), subnormal=int(is_sub(want).sum()), centre_subnormal=int((is_sub(d) & ok).sum()),
                inf=int(np.isinf(want).sum()), table_subnormal=int(is_sub(spatial).sum()), table_zero=int((spatial == 0).sum()),
                table_entries=int(spatial.size), ftz_differs=int((bits(bilateral_expect(d, tables, ftz=True)) != bits(want)).sum()),
                ftz_differs_by_table_alone=int((bits(tables_only) != bits(want)).sum()))


# ---- case 5: the torch-facing projection kernels -----------------------------------------------------------------------------------
PROJECT_SHAPE = (2, 2, 130)
PROJECT_EPS = F(0.0)                      # den = c2 + 0: a subnormal c2 stays the divisor (1e-7 would swallow it)


@functools.lru_cache(None)
def project_case():
    """project_ref.dense_inputs with, pixel by pixel in three interleaved classes: as it is; depth and upstream gradients scaled
    into the subnormal range and the point scaled by 2^-127 (all four coordinates: c_i and den subnormal, their quotient ordinary);
    depth a random subnormal, gradients about 2^-120 (products with rays and with 1 / den underflow)."""
    B, H, W = PROJECT_SHAPE
    hw = H * W
    inp = {k: v.copy() for k, v in PR.dense_inputs(B, H, W, seed=9).items()}
    rng = np.random.default_rng(99)
    cls = np.arange(hw) % 3
    a, b = cls == 1, cls == 2
    inp["depth"][:, a] = (inp["depth"][:, a].astype(np.float64) * 2.0 ** -130).astype(F)
    inp["depth"][:, b] = random_subnormals(rng, (B, int(b.sum())))
    inp["gcam"][:, :, a] = (inp["gcam"][:, :, a].astype(np.float64) * 2.0 ** -128).astype(F)
    inp["gcam"][:, :, b] = (inp["gcam"][:, :, b].astype(np.float64) * 2.0 ** -120).astype(F)
    inp["points"][:, :, a] = (inp["points"][:, :, a].astype(np.float64) * 2.0 ** -127).astype(F)
    g = inp["gpix"].reshape(B, hw, 2)
    g[:, a] = (g[:, a].astype(np.float64) * 2.0 ** -128).astype(F)
    g[:, b] = (g[:, b].astype(np.float64) * 2.0 ** -120).astype(F)
    inp["gpix"] = g.reshape(B, H, W, 2)
    want = project_expect(inp)
    flat = project_expect({k: flush(v) for k, v in inp.items()})
    c, den, inv, d = PR.chain_f32(inp["gpix"], inp["points"], inp["P"], H, W, PROJECT_EPS)
    facts = {"inputs_subnormal": {k: int(is_sub(v).sum()) for k, v in inp.items()}, "den_subnormal": int(is_sub(den).sum()),
             "d_subnormal": int(is_sub(d).sum())}
    for name in want:
        w = want[name] if name != "cam" else want[name][:, :3]
        f = flat[name] if name != "cam" else flat[name][:, :3]
        n = ~np.isnan(w)
        facts[name] = dict(n=int(w.size), subnormal=int(is_sub(w).sum()), nan=int((~n).sum()),
                           ftz_differs=int(((np.isnan(f) != ~n) | (n & (bits(flush(f)) != bits(w)))).sum()))
    # the pixels of classes a and b are made from subnormal operands throughout
    facts["from_subnormal_fraction"] = float((a | b).mean())
    return dict(inp=inp, want=want, facts=facts)


def project_expect(inp):
    B, H, W = PROJECT_SHAPE
    return dict(cam=PR.cam_points_f32(inp["depth"], inp["inv_K"], H, W), gdep=PR.grad_depth_f32(inp["gcam"], inp["inv_K"], H, W),
                pix=PR.pix_f32(inp["points"], inp["P"], H, W, PROJECT_EPS),
                gpts=PR.grad_points_f32(inp["gpix"], inp["points"], inp["P"], H, W, PROJECT_EPS))


# ---- case 6: f32 in, f32 out through the fp64 paths ----------------------------------------------------------------------------------
APPLY_N = 1025
APPLY_KS = (0, 1, 30, -1)                 # T = 2^-k P: pass-through, halving (ties), deep into the subnormal range, doubling (overflow)
PERM = (2, 0, 1)                          # out[a] = 2^-k in[PERM[a]]
UNPROJECT_SHAPE = (25, 41)                # 1025 pixels; fx = fy = 1, cx = cy = 0: X = u Z with integer u, exact in fp64


@functools.lru_cache(None)
def apply_points():
    """[1025, 3] f32, no zeros: a third subnormal, a third between 2^-126 and 2^-96, the rest ordinary or within a factor 2 of
    FLT_MAX; and rows of hand-made values: odd multiples of 2^-149 (halved: exact ties), 2^-125 - 2^-149 (halved: the tie that
    rounds up to 2^-126), the largest subnormal, 2^-126, 2^-149, FLT_MAX and the first value whose double overflows"""
    rng = np.random.default_rng(606)
    n = APPLY_N
    sub = random_subnormals(rng, (n, 3))
    low = (rng.uniform(1, 2, (n, 3)) * 2.0 ** rng.integers(-126, -96, (n, 3)) * rng.choice([-1, 1], (n, 3))).astype(F)
    ordinary = (rng.normal(size=(n, 3)) * 10).astype(F)
    ordinary[ordinary == 0] = F(1.0)
    top = (rng.uniform(0.5, 1.0, (n, 3)) * float(FLT_MAX) * rng.choice([-1, 1], (n, 3))).astype(F)
    pick = rng.random((n, 3))
    x = np.select([pick < 0.34, pick < 0.67, pick < 0.87], [sub, low, ordinary], top).astype(F)
    hand = np.array([3 * 2.0 ** -149, 5 * 2.0 ** -149, 2.0 ** -125 - 2.0 ** -149, 2.0 ** -126 - 2.0 ** -149, 2.0 ** -126, 2.0 ** -149,
                     float(FLT_MAX), 2.0 ** 127 * (1 + 2.0 ** -23), 7 * 2.0 ** -149], dtype=np.float64).astype(F)
    x[:3, :] = hand.reshape(3, 3)
    x[3:6, :] = -hand.reshape(3, 3)
    return x


def apply_T(k):
    T = np.zeros((4, 4))
    for a in range(3):
        T[a, PERM[a]] = 2.0 ** -k
    T[3, 3] = 1.0
    return T


def apply_pose(k):
    """r3d_se3_apply's 12 doubles: Rinv row-major, t"""
    return np.concatenate([apply_T(k)[:3, :3].reshape(9), np.zeros(3)])


def apply_expect(x, k):
    with np.errstate(over="ignore"):
        return (x[:, list(PERM)].astype(np.float64) * 2.0 ** -k).astype(F)


def apply_facts(x, k):
    want = apply_expect(x, k)
    exact = x[:, list(PERM)].astype(np.float64) * 2.0 ** -k
    units = exact / 2.0 ** -149
    tie = (np.abs(exact) < 2.0 ** -126) & (np.abs(units - np.floor(units) - 0.5) == 0)
    with np.errstate(over="ignore"):
        flat = flush((flush(x)[:, list(PERM)].astype(np.float64) * 2.0 ** -k).astype(F))
    return dict(n=int(want.size), in_subnormal=int(is_sub(x).sum()), out_subnormal=int(is_sub(want).sum()), ties=int(tie.sum()),
                rounds_up_to_tiny=int(((np.abs(want) == TINY) & (np.abs(exact) < 2.0 ** -126)).sum()),
                inf=int(np.isinf(want).sum()), inexact=int((want.astype(np.float64) != exact).sum()),
                ftz_differs=int((bits(flat) != bits(want)).sum()))


@functools.lru_cache(None)
def unproject_depth():
    """[25, 41] f32 drawn like apply_points (first column of it), signs kept: r3d_unproject masks nothing"""
    return np.ascontiguousarray(apply_points()[:, 0].reshape(UNPROJECT_SHAPE))


def unproject_expect(d, k):
    H, W = d.shape
    with np.errstate(over="ignore"):
        Z = d.astype(np.float64) * 2.0 ** -k
        X = np.arange(W, dtype=np.float64)[None, :] * Z
        Y = np.arange(H, dtype=np.float64)[:, None] * Z
        return np.stack([X, Y, Z], -1).reshape(-1, 3).astype(F)


def unproject_facts(d, k):
    want = unproject_expect(d, k)
    with np.errstate(over="ignore"):
        flat = flush(unproject_expect(flush(d), k))
    return dict(n=int(want.size), in_subnormal=int(is_sub(d).sum()), out_subnormal=int(is_sub(want).sum()), inf=int(np.isinf(want).sum()),
                from_subnormal=int(3 * is_sub(d).sum()), ftz_differs=int((bits(flat) != bits(want)).sum()))
