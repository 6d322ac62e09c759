"""NumPy restatement of the torch-facing projection kernels (f4: csrc/r3d_backproject.hip behind torch_ops.BackprojectDepth
and torch_ops.Project3D), after the evaluation order written in include/r3d.h.

Two families:

  *_f32   the header chains in np.float32, one operation per rounding, vectorised over pixels.  The library is built with
          -ffp-contract=off and f32 division is correctly rounded, so these are the BIT-LEVEL expectation of every per-pixel
          output (cam_points, grad_depth, pix, grad_points).
  *_f64   the same quantities, plus the twelve per-image sums grad_P, from the f32 inputs promoted to float64.  Nothing in
          between is rounded to f32 -- see chain_f64 for the one place where that is a decision.

grad_P_bound() is the derived per-entry bound of the twelve sums; dense_inputs() and shapes() are the input sets the CPU and
the GPU tests share, so that what the CPU tests prove about the inputs holds for exactly what the GPU tests run.
"""
import numpy as np

U = 2.0 ** -24                 # unit roundoff of f32 (round to nearest)
EPS = np.float32(1e-7)         # upstream Project3D's eps, as the f32 the C ABI receives
THREADS = 256                  # kThreads of r3d_backproject.hip
FWD_CAP_PER_CU = 16            # workgroups per CU at which the three forward-style launches cap their grid
GRAD_CAP_PER_CU = 4            # ... and project3d_grad_kernel
MI355X_CUS = 256               # what the CPU tests assume; the GPU tests read the device


# ---- launch geometry ---------------------------------------------------------------------------------------------------
def grid_width(hw, cus, per_cu=GRAD_CAP_PER_CU):
    """Workgroups along x as the launch computes them: min(ceil(hw / 256), per_cu * CUs)."""
    return min(-(-hw // THREADS), per_cu * cus)


def trips(hw, width):
    """Passes of the grid-stride loop the busiest lane makes."""
    return -(-hw // (width * THREADS))


def _xy(H, W, dtype):
    ys, xs = np.divmod(np.arange(H * W), W)
    return xs.astype(dtype), ys.astype(dtype)


# ---- f32 restatements: the bit-level expectation ---------------------------------------------------------------------------
def rays_f32(inv_K, H, W):
    """[B][3][hw]: (k_c0*x + k_c1*y) + k_c2."""
    k = np.asarray(inv_K, np.float32)
    fx, fy = _xy(H, W, np.float32)
    return np.stack([(k[:, c, 0:1] * fx + k[:, c, 1:2] * fy) + k[:, c, 2:3] for c in range(3)], 1)


def cam_points_f32(depth, inv_K, H, W):
    """[B][4][hw]: z * ray, and a plane of exact ones."""
    B = depth.shape[0]
    z = np.asarray(depth, np.float32).reshape(B, 1, H * W)
    with np.errstate(all="ignore"):
        cam = z * rays_f32(inv_K, H, W)
    return np.concatenate([cam, np.ones((B, 1, H * W), np.float32)], 1)


def grad_depth_f32(gcam, inv_K, H, W):
    """[B][hw]: (g0*r0 + g1*r1) + g2*r2 (the ones plane carries no gradient)."""
    g, r = np.asarray(gcam, np.float32), rays_f32(inv_K, H, W)
    with np.errstate(all="ignore"):
        return (g[:, 0] * r[:, 0] + g[:, 1] * r[:, 1]) + g[:, 2] * r[:, 2]


def _c(P, x):
    """c_i = ((P_i0*px + P_i1*py) + P_i2*pz) + P_i3*pw in the dtype of the arguments: [B][3][hw]."""
    return np.stack([((P[:, i, 0:1] * x[:, 0] + P[:, i, 1:2] * x[:, 1]) + P[:, i, 2:3] * x[:, 2]) + P[:, i, 3:4] * x[:, 3]
                     for i in range(3)], 1)


def pix_f32(points, P, H, W, eps=EPS):
    """[B][H][W][2]: ((c_i / den) / (W-1 or H-1) - 0.5) * 2 with den = c2 + eps."""
    x, m = np.asarray(points, np.float32), np.asarray(P, np.float32)
    with np.errstate(all="ignore"):
        c = _c(m, x)
        den = c[:, 2] + np.float32(eps)
        px = ((c[:, 0] / den) / np.float32(W - 1) - np.float32(0.5)) * np.float32(2)
        py = ((c[:, 1] / den) / np.float32(H - 1) - np.float32(0.5)) * np.float32(2)
    return np.stack([px, py], -1).reshape(x.shape[0], H, W, 2)


def chain_f32(gpix, points, P, H, W, eps=EPS):
    """The backward chain in f32: c [B][3][hw], den, inv and d [B][3][hw] (d loss / d c)."""
    x, m = np.asarray(points, np.float32), np.asarray(P, np.float32)
    g = np.asarray(gpix, np.float32).reshape(x.shape[0], H * W, 2)
    gw, gh = np.float32(2) / np.float32(W - 1), np.float32(2) / np.float32(H - 1)
    with np.errstate(all="ignore"):
        c = _c(m, x)
        den = c[:, 2] + np.float32(eps)
        inv = np.float32(1) / den
        d0 = (g[..., 0] * gw) * inv
        d1 = (g[..., 1] * gh) * inv
        d2 = (-(d0 * c[:, 0] + d1 * c[:, 1])) * inv
    return c, den, inv, np.stack([d0, d1, d2], 1)


def grad_points_f32(gpix, points, P, H, W, eps=EPS):
    """[B][4][hw]: (P_0k*d0 + P_1k*d1) + P_2k*d2."""
    m = np.asarray(P, np.float32)
    d = chain_f32(gpix, points, P, H, W, eps)[3]
    with np.errstate(all="ignore"):
        return np.stack([(m[:, 0, k:k + 1] * d[:, 0] + m[:, 1, k:k + 1] * d[:, 1]) + m[:, 2, k:k + 1] * d[:, 2]
                         for k in range(4)], 1)


# ---- f64 statements -----------------------------------------------------------------------------------------------------------
def rays_f64(inv_K, H, W):
    k = np.asarray(inv_K, np.float32).astype(np.float64)
    fx, fy = _xy(H, W, np.float64)
    return np.stack([k[:, c, 0:1] * fx + k[:, c, 1:2] * fy + k[:, c, 2:3] for c in range(3)], 1)


def cam_points_f64(depth, inv_K, H, W):
    B = depth.shape[0]
    z = np.asarray(depth, np.float32).astype(np.float64).reshape(B, 1, H * W)
    return np.concatenate([z * rays_f64(inv_K, H, W), np.ones((B, 1, H * W))], 1)


def grad_depth_f64(gcam, inv_K, H, W):
    g = np.asarray(gcam, np.float32).astype(np.float64)
    return (g[:, :3] * rays_f64(inv_K, H, W)).sum(1)


def chain_f64(gpix, points, P, H, W, eps=EPS, drop_d1c1=False):
    """c, den, d in float64 from the f32 inputs promoted to float64.

    Rounding: NOTHING here is rounded to f32.  The one step where that is a decision is den = c2 + eps.  The device forms c2
    in f32 and adds the f32 eps in f32, and include/r3d.h states exactly that chain for the DEVICE; it does not make the f32
    value of den part of the mathematical definition -- the layer's definition is c2 + eps.  So c2 is formed in f64, the
    f32 value of eps (the number the C ABI receives, promoted exactly) is added in f64, and den stays f64.  Rounding den to
    f32 here would import one of the device's roundings into the reference and hide an error in precisely that step.
    gw = 2/(W-1) and gh = 2/(H-1) are likewise the f64 quotients, not the f32 ones the host code passes.

    gpix may be None (forward only: d is None).  drop_d1c1 removes the second term of d2 -- a deliberate defect for the test
    that shows the reference can fail."""
    x = np.asarray(points, np.float32).astype(np.float64)
    m = np.asarray(P, np.float32).astype(np.float64)
    c = _c(m, x)
    den = c[:, 2] + float(np.float32(eps))
    if gpix is None:
        return c, den, None
    g = np.asarray(gpix, np.float32).astype(np.float64).reshape(x.shape[0], H * W, 2)
    d0 = g[..., 0] * (2.0 / (W - 1)) / den
    d1 = g[..., 1] * (2.0 / (H - 1)) / den
    d2 = -(d0 * c[:, 0] + (0.0 if drop_d1c1 else d1 * c[:, 1])) / den
    return c, den, np.stack([d0, d1, d2], 1)


def pix_f64(points, P, H, W, eps=EPS):
    c, den, _ = chain_f64(None, points, P, H, W, eps)
    out = np.stack([(c[:, 0] / den / (W - 1) - 0.5) * 2, (c[:, 1] / den / (H - 1) - 0.5) * 2], -1)
    return out.reshape(c.shape[0], H, W, 2)


def grad_points_f64(gpix, points, P, H, W, eps=EPS):
    d = chain_f64(gpix, points, P, H, W, eps)[2]
    return np.einsum("bik,bip->bkp", np.asarray(P, np.float32).astype(np.float64), d)


def grad_P_f64(gpix, points, P, H, W, eps=EPS, drop_d1c1=False):
    """(want [B][3][4], abs_sum [B][3][4]): the sums over pixels of d_i * x_k and of |d_i * x_k|."""
    d = chain_f64(gpix, points, P, H, W, eps, drop_d1c1)[2]
    x = np.asarray(points, np.float32).astype(np.float64)
    return np.einsum("bip,bkp->bik", d, x), np.einsum("bip,bkp->bik", np.abs(d), np.abs(x))


# Roundings inside one term d_i * x_k, counted from the header chain (every f32 operation on the way, not only the longest
# path through it):
#   inv   = 1 / (c2 + eps):  c2 is 4 products + 3 sums = 7, the eps add 1, the reciprocal 1                          =  9
#   d0,d1 = (g * (2/(W-1))) * inv:  the quotient 2/(W-1) 1, its product with g 1, inv 9, the product with inv 1      = 12
#   rows 0 and 1:  d_i * x_k = 12 + 1                                                                                 = 13
#   d2    = (-(d0*c0 + d1*c1)) * inv:  one branch d_i*c_i is 12 + 7 (c_i) + 1 = 20, the two branches meet in one sum 1,
#           the negation is exact, inv AGAIN 9 (it enters a second time), the product with it 1                      = 31
#   row 2:         d2 * x_k = 31 + 1                                                                                  = 32
K_ROUNDINGS = np.array([13, 13, 32], dtype=np.float64)
SHUFFLE_STEPS = 6              # offsets 32, 16, 8, 4, 2, 1 of the wave reduction
WAVE_ADDS = 3                  # four waves of a workgroup: 0 + r0 is exact, three real additions follow


def grad_P_bound(gpix, points, P, H, W, width, eps=EPS):
    """Per entry [B][3][4]:  (n + k) * u * sum_p |d_i(p) * x_k(p)|  +  |want| * u.

    n = trips(hw, width) + 6 + 3 is the longest chain of f32 additions a term passes through: one per pass of the
    grid-stride loop into the lane's accumulator, six shuffle steps, three additions across the waves.  The second stage adds
    the workgroup partials in f64 (exact to well below u here), and its cast to f32 is the `|want| * u`.
    k = K_ROUNDINGS[i] is counted above.  `width` is the launch's grid width (grid_width())."""
    want, abs_sum = grad_P_f64(gpix, points, P, H, W, eps)
    n = trips(H * W, width) + SHUFFLE_STEPS + WAVE_ADDS
    return (n + K_ROUNDINGS)[None, :, None] * U * abs_sum + np.abs(want) * U


# ---- comparison ---------------------------------------------------------------------------------------------------------------
def eq_bits(got, want):
    """f32 arrays: equal uint32 views where `want` is not NaN, equal NaN masks elsewhere (NaN sign and payload are not part
    of the contract)."""
    got, want = np.ascontiguousarray(got), np.ascontiguousarray(want)
    assert got.dtype == np.float32 and want.dtype == np.float32, (got.dtype, want.dtype)
    if got.shape != want.shape:
        return False
    nan = np.isnan(want)
    if not np.array_equal(np.isnan(got), nan):
        return False
    return bool(np.array_equal(got.view(np.uint32)[~nan], want.view(np.uint32)[~nan]))


def first_mismatch(got, want):
    """For an assertion message: (count, flat index, got, want) of the entries eq_bits() objects to."""
    g, w = np.ascontiguousarray(got).reshape(-1), np.ascontiguousarray(want).reshape(-1)
    bad = np.flatnonzero((np.isnan(g) != np.isnan(w)) | (~np.isnan(w) & (g.view(np.uint32) != w.view(np.uint32))))
    return (0,) if bad.size == 0 else (int(bad.size), int(bad[0]), float(g[bad[0]]), float(w[bad[0]]))


# ---- the shared input sets ----------------------------------------------------------------------------------------------------
DEN_MIN = np.float32(0.25)


def _signed(rng, lo, hi, size):
    """Random sign, magnitude log-uniform in [lo, hi]."""
    mag = np.exp(rng.uniform(np.log(lo), np.log(hi), size))
    return np.where(rng.random(size) < 0.5, -mag, mag)


def dense_inputs(B, H, W, seed=0):
    """The "dense" input set of a raster: every term of every chain is present and has to be right by sign.

      inv_K   a full 3 x 3 block, mixed sign, magnitudes log-uniform in [1e-3, 1] (row 3 and column 3 random too: unused)
      P       twelve random entries of mixed sign.  The diagonal is 0.5..1, the rest 0.02..0.2, so that each c_i has one
              leading term: a rounding count is a relative-error count only where sums do not cancel, and
              test_project_host.py checks, set by set, that the k of grad_P_bound covers the terms' own f32 error
      points  px, py, pz of mixed sign, magnitudes 0.5..2 (pz 0.5..4); pw in [0.5, 2]
      den     c2 + eps (f32) has both signs in every image with |den| >= 0.25: pz is rejection-sampled
      depth   normal(0, 20), so about half negative; +0.0, -0.0 and a negative value at the first three pixels when there are
              that many
      gcam    normal(0, 1)
      gpix    normal(0, 1) in magnitude.  The sign of g.x is that of px * den and the sign of g.y that of py * den (symmetric
              around zero, so still normal(0, 1) entry by entry), the latter times the sign of P_00 * P_11 of the image.  The
              sums grad_P[0][0] and grad_P[1][1] then do not cancel, and max|want| -- the yardstick of the old tolerance --
              stays of the order of sum|terms| at every raster size instead of shrinking like 1/sqrt(hw); and the leading
              parts of d0*c0 and d1*c1 agree in sign, so that d2 is not mostly the difference of two equal numbers (a
              four-pixel image whose d2 all but cancels has an f32 error no rounding count covers).  The minor terms of
              c_i still give both sign patterns within every image, and every other entry is a sum of mixed signs."""
    hw = H * W
    rng = np.random.default_rng([seed, B, H, W])
    inv_K = _signed(rng, 1e-3, 1.0, (B, 4, 4)).astype(np.float32)
    mag = rng.uniform(0.02, 0.2, (B, 3, 4))
    for i in range(3):
        mag[:, i, i] = rng.uniform(0.5, 1.0, B)
    P = np.where(rng.random((B, 3, 4)) < 0.5, -mag, mag).astype(np.float32)
    pts = np.empty((B, 4, hw), np.float32)
    pts[:, 0:2] = np.where(rng.random((B, 2, hw)) < 0.5, -1, 1) * rng.uniform(0.5, 2.0, (B, 2, hw))
    pts[:, 3] = rng.uniform(0.5, 2.0, (B, hw))
    todo = np.ones((B, hw), bool)
    sign = np.zeros((1, hw), np.float32)
    sign[0, :2] = (1, -1)[:hw]                     # both signs in every image, however small: the first two pixels are told theirs
    while todo.any():
        n = int(todo.sum())
        pts[:, 2][todo] = np.where(rng.random(n) < 0.5, -1, 1) * rng.uniform(0.5, 4.0, n)
        den = _c(P, pts)[:, 2] + EPS
        todo = (np.abs(den) < DEN_MIN) | (sign * den < 0)
    depth = (rng.normal(size=(B, hw)) * 20).astype(np.float32)
    if hw >= 2:
        depth[:, 0], depth[:, 1] = 0.0, -0.0
    if hw >= 3:
        depth[:, 2] = -np.abs(depth[:, 2])
    gcam = rng.normal(size=(B, 4, hw)).astype(np.float32)
    gpix = np.abs(rng.normal(size=(B, hw, 2))).astype(np.float32)
    gpix[..., 0] = np.copysign(gpix[..., 0], pts[:, 0] * den)
    gpix[..., 1] = np.copysign(gpix[..., 1], pts[:, 1] * den * (P[:, 0, 0] * P[:, 1, 1])[:, None])
    return dict(depth=depth, inv_K=inv_K, gcam=gcam, points=pts, P=P, gpix=gpix.reshape(B, H, W, 2))


def shapes(cus):
    """The rasters of the GPU tests for a device of `cus` compute units: (backproject only, both layers, forward stride
    cases, gradient stride cases)."""
    back_only = [(1, 1, 1), (1, 1, 300), (1, 300, 1)]
    both = [(1, 2, 2), (2, 16, 16), (3, 7, 37), (2, 5, 51)]
    fwd_stride = [(1, 16 * cus + 1, 257), (2, 32 * cus + 3, 257)]
    grad_stride = [(2, 4 * cus + 1, 257), (1, 12 * cus + 5, 257)]
    return back_only, both, fwd_stride, grad_stride


DENSE_CASE = (3, 7, 37)        # "the dense case" of the tests that need one: 259 pixels, one workgroup plus three lanes
BIG_BATCH = (65535, 2, 2)      # the grid.y limit
