"""Global registration on the MI355X: FPFH descriptors, feature matching and RANSAC over the correspondences -- the recipe users
of Open3D run in front of ICP when nobody has a rough pose (compute_fpfh_feature, registration_ransac_based_on_feature_matching;
no parity with Open3D or PCL is claimed).  Semantics: include/r3d.h (r3d_fpfh_knn, r3d_feature_match, r3d_register_ransac) and
DESIGN.md section 4.5r.

register_global is the whole recipe for two host clouds; the stages are compute_fpfh, match_features and registration_ransac.
compute_fpfh_device takes an NNIndex over a device cloud and device pointers.
"""
import collections
import ctypes as C

import numpy as np

from . import _lib as L
from ._args import colour_words, positive as _check_positive
from .device import default_context
from .normals import _check_k, _check_radius
from .outliers import Cloud, _cloud
from .segmentation import MAX_HYPOTHESES, _check_hypotheses, _check_seed

FPFH_DIM = 33
RESULT_DOUBLES = 32

Fpfh = collections.namedtuple("Fpfh", ["fpfh", "spfh", "count"])
Fpfh.__doc__ = ("FPFH rows [N,33] float32 (theta, alpha, phi; 11 bins each), the SPFH pair counts [N,33] uint8 and the number of "
                "pairs counted per point [N] uint32.")
Matches = collections.namedtuple("Matches", ["corr", "idx", "dist"])
Matches.__doc__ = ("corr [M,2] uint32 (row of a, row of b; a ascending), idx [Na] uint32 = the nearest row of b of every row of a "
                   "(0xffffffff: none), dist [Na] float32 = its squared feature distance.")
RansacResult = collections.namedtuple("RansacResult", ["T", "inliers", "best_hypothesis", "best_count", "best_pairs", "n_valid",
                                                       "n_inliers", "rms", "refit_degenerate", "counts"])
RansacResult.__doc__ = ("T [4,4] float64 (NaN when no hypothesis had 3 inliers), inliers [M] bool over the correspondences, the best "
                        "hypothesis, its count and its three correspondence rows, the number of valid hypotheses, the final inlier "
                        "count and rms, whether the refit was undefined, counts [H] uint32 or None.")


def _features(f, what):
    f = np.ascontiguousarray(f, dtype=np.float32)
    if f.ndim != 2 or f.shape[1] != FPFH_DIM:
        raise ValueError("%s must be [N,%d]" % (what, FPFH_DIM))
    if not 1 <= f.shape[0] < 1 << 32:
        raise ValueError("%s needs 1 <= N < 2^32 rows, got %d" % (what, f.shape[0]))
    return f


def _normals(normals, n):
    nrm = np.ascontiguousarray(normals, dtype=np.float32)
    if nrm.shape != (n, 3):
        raise ValueError("normals must be [%d,3], got %r" % (n, nrm.shape))
    return nrm


def _correspondences(corr):
    c = np.ascontiguousarray(corr)
    if c.ndim != 2 or c.shape[1] != 2 or c.dtype.kind not in "iu":
        raise ValueError("corr must be an integer [M,2] array")
    if c.shape[0] < 3 or c.shape[0] >= 1 << 32:
        raise ValueError("RANSAC needs 3 <= M < 2^32 correspondences, got %d" % c.shape[0])
    if c.size and (c.min() < 0 or c.max() >= 1 << 32):
        raise ValueError("corr holds row numbers outside [0, 2^32)")
    return np.ascontiguousarray(c, dtype=np.uint32)


def _check_bool(v, what):
    if not isinstance(v, (bool, np.bool_)):
        raise ValueError("%s must be True or False, got %r" % (what, v))
    return bool(v)


# ---- device pointers -----------------------------------------------------------------------------------------------------

def compute_fpfh_device(index, k, d_normals, d_fpfh, d_spfh=None, d_count=None, radius=None):
    """FPFH of the index's own cloud into d_fpfh [n][33] float32 from d_normals [n][3] float32; optional d_spfh [n][33] uint8
    and d_count [n] uint32.  Asynchronous on the index's context."""
    k, r = _check_k(k), _check_radius(radius)
    L.check(index.ctx.lib.r3d_fpfh_knn(index.handle, k, r, d_normals, d_fpfh, d_spfh, d_count))


def match_features_device(ctx, d_a, na, d_b, nb, d_idx, d_dist=None, d_corr=None, mutual=False):
    """Nearest row of b for every row of a into d_idx [na] uint32 (d_dist [na] float32 optional).  With d_corr ([na][2] uint32)
    the kept correspondences are compacted into it and their number is returned (synchronous); otherwise None (asynchronous)."""
    mutual = _check_bool(mutual, "mutual")
    if d_corr is None:
        if mutual:
            raise ValueError("mutual matching needs d_corr")
        L.check(ctx.lib.r3d_feature_match(ctx.handle, d_a, int(na), d_b, int(nb), 0, d_idx, d_dist, None, None))
        return None
    m = C.c_int64()
    L.check(ctx.lib.r3d_feature_match(ctx.handle, d_a, int(na), d_b, int(nb), 1 if mutual else 0, d_idx, d_dist, d_corr, C.byref(m)))
    return m.value


def registration_ransac_device(ctx, d_src, ns, d_tgt, nt, d_corr, m, distance_threshold, num_hypotheses, seed, d_inlier,
                               d_counts=None):
    """r3d_register_ransac on device pointers: d_inlier [m] uint8, d_counts [num_hypotheses] uint32 (optional); returns the
    32-double result block as an array.  Synchronous."""
    thr, hyp, seed = _check_positive(distance_threshold, "distance_threshold"), _check_hypotheses(num_hypotheses), _check_seed(seed)
    if int(m) < 3:
        raise ValueError("RANSAC needs at least 3 correspondences, got %d" % m)
    res = (C.c_double * RESULT_DOUBLES)()
    L.check(ctx.lib.r3d_register_ransac(ctx.handle, d_src, int(ns), d_tgt, int(nt), d_corr, int(m), thr, hyp, seed, d_inlier, d_counts,
                                        res))
    return np.array(res[:], np.float64)


# ---- host arrays ---------------------------------------------------------------------------------------------------------

def compute_fpfh(xyz, normals=None, k=32, radius=None, ctx=None):
    """Fpfh of every point of an [N,3] cloud from its k nearest neighbours (those within `radius` when given).  normals [N,3]:
    as normals.estimate_normals returns them (zero rows: no normal); None: estimated here with the same k and radius."""
    xyz, k, r = _cloud(xyz), _check_k(k), _check_radius(radius)
    n = xyz.shape[0]
    nrm = None if normals is None else _normals(normals, n)
    if n == 0:
        return Fpfh(np.zeros((0, FPFH_DIM), np.float32), np.zeros((0, FPFH_DIM), np.uint8), np.zeros(0, np.uint32))
    with Cloud(ctx or default_context(), xyz) as c:
        d_n = c.alloc(n * 12)
        if nrm is None:
            c.index.normals_knn(k, r, None, 1, d_n.ptr)
        else:
            d_n.upload(nrm)
        d_f, d_s, d_c = c.alloc(n * FPFH_DIM * 4), c.alloc(n * FPFH_DIM), c.alloc(n * 4)
        L.check(c.ctx.lib.r3d_fpfh_knn(c.index.handle, k, r, d_n.ptr, d_f.ptr, d_s.ptr, d_c.ptr))
        return Fpfh(d_f.download_array(np.float32, (n, FPFH_DIM)), d_s.download_array(np.uint8, (n, FPFH_DIM)), d_c.download(np.uint32, n))


def match_features(fa, fb, mutual=True, ctx=None):
    """Matches: every row of fa [Na,33] against its nearest row of fb [Nb,33] (squared L2, the lowest row of equal distances);
    mutual: only the pairs that are each other's nearest."""
    fa, fb, mutual = _features(fa, "fa"), _features(fb, "fb"), _check_bool(mutual, "mutual")
    ctx = ctx or default_context()
    na, nb = fa.shape[0], fb.shape[0]
    with ctx.buffers() as B:
        d_a, d_b = B.upload(fa), B.upload(fb)
        d_idx, d_dist, d_corr = B.alloc(na * 4), B.alloc(na * 4), B.alloc(na * 8)
        m = match_features_device(ctx, d_a.ptr, na, d_b.ptr, nb, d_idx.ptr, d_dist.ptr, d_corr.ptr, mutual)
        return Matches(d_corr.download_array(np.uint32, (m, 2)), d_idx.download(np.uint32, na), d_dist.download(np.float32, na))


def _result(r, inliers, counts):
    return RansacResult(r[:16].reshape(4, 4).copy(), inliers, int(r[16]), int(r[17]), r[18:21].astype(np.uint32), int(r[21]), int(r[22]),
                        float(r[23]), bool(r[24]), counts)


def registration_ransac(src, tgt, corr, distance_threshold, num_hypotheses=4096, seed=0, want_counts=False, ctx=None):
    """RansacResult: the rigid T (tgt ~ T src) that brings the most correspondences corr [M,2] (row of src, row of tgt) within
    distance_threshold among num_hypotheses three-pair samples, refitted to those pairs by least squares."""
    src, tgt, corr = _cloud(src), _cloud(tgt), _correspondences(corr)
    thr, hyp, seed = _check_positive(distance_threshold, "distance_threshold"), _check_hypotheses(num_hypotheses), _check_seed(seed)
    if src.shape[0] < 1 or tgt.shape[0] < 1:
        raise ValueError("both clouds need at least one point")
    ctx = ctx or default_context()
    m = corr.shape[0]
    with ctx.buffers() as B:
        d_src, d_tgt, d_corr, d_in = B.upload(src), B.upload(tgt), B.upload(corr), B.alloc(m)
        d_cnt = B.alloc(hyp * 4) if want_counts else None
        r = registration_ransac_device(ctx, d_src.ptr, src.shape[0], d_tgt.ptr, tgt.shape[0], d_corr.ptr, m, thr, hyp, seed, d_in.ptr,
                                       d_cnt.ptr if d_cnt else None)
        return _result(r, d_in.download(np.uint8, m) != 0, d_cnt.download(np.uint32, hyp) if d_cnt else None)


def _viewpoint(v, what):
    if v is None:
        return None
    v = np.asarray(v, dtype=np.float64)
    if v.shape != (3,) or not np.isfinite(v).all():
        raise ValueError("%s must be None or three finite numbers, got %r" % (what, v))
    return v


def register_global(src, tgt, voxel_size, k=32, feature_radius=5.0, num_hypotheses=MAX_HYPOTHESES, rounds=4, seed=0, mutual=True,
                    refine=False, src_viewpoint=None, tgt_viewpoint=None, ctx=None):
    """(T, info): the rigid T with tgt ~ T src, found without a starting pose.  Both clouds are voxel-downsampled to
    voxel_size; normals and FPFH come from the k nearest neighbours within feature_radius x voxel_size; the features are matched
    (mutual: both ways); RANSAC with distance_threshold = 1.5 x voxel_size runs `rounds` times with seeds seed, seed + 1, ...
    and the round with the most final inliers wins (the first of equals).  refine: T starts icp.icp_point_to_plane on the
    downsampled clouds (the target's normals are the ones estimated here; pairs farther apart than the RANSAC threshold stay out).  info: the downsampled clouds, the correspondences,
    the winning RansacResult and, with refine, ICP's info.  ValueError when fewer than 3 correspondences survive or no round
    finds a pose.
    src_viewpoint / tgt_viewpoint: where each cloud was seen from, in its own frame; the normals are turned towards it.  FPFH
    depends on the normals' signs, and the default sign rule (largest component positive) does not turn with the cloud: clouds
    that may be rotated by more than a few tens of degrees against each other need their viewpoints (a single-view scan in its
    camera frame: (0, 0, 0))."""
    src, tgt = _cloud(src), _cloud(tgt)
    vs, k = _check_positive(voxel_size, "voxel_size"), _check_k(k)
    fr = _check_positive(feature_radius, "feature_radius")
    hyp, seed = _check_hypotheses(num_hypotheses), _check_seed(seed)
    if isinstance(rounds, bool) or not isinstance(rounds, (int, np.integer)) or int(rounds) < 1:
        raise ValueError("rounds must be an integer >= 1, got %r" % (rounds,))
    mutual, refine = _check_bool(mutual, "mutual"), _check_bool(refine, "refine")
    views = (_viewpoint(src_viewpoint, "src_viewpoint"), _viewpoint(tgt_viewpoint, "tgt_viewpoint"))
    ctx = ctx or default_context()
    from . import voxelmap
    from .normals import estimate_normals
    radius, thr = fr * vs, 1.5 * vs
    down, nrm, feat = [], [], []
    for cloud, view in zip((src, tgt), views):
        d = np.ascontiguousarray(voxelmap.voxel_down_sample(cloud, vs, ctx=ctx).xyz, dtype=np.float32)
        if d.shape[0] < 3:
            raise ValueError("a cloud has fewer than 3 occupied voxels at voxel_size %g" % vs)
        n = estimate_normals(d, k, radius=radius, viewpoint=view, ctx=ctx).normals
        down.append(d)
        nrm.append(n)
        feat.append(compute_fpfh(d, n, k, radius, ctx=ctx).fpfh)
    matches = match_features(feat[0], feat[1], mutual, ctx=ctx)
    if matches.corr.shape[0] < 3:
        raise ValueError("only %d correspondences survive the matching; RANSAC needs 3" % matches.corr.shape[0])
    best = None
    for r in range(int(rounds)):
        res = registration_ransac(down[0], down[1], matches.corr, thr, hyp, (seed + r) % (1 << 64), ctx=ctx)
        if np.isfinite(res.T).all() and (best is None or res.n_inliers > best.n_inliers):
            best = res
    if best is None:
        raise ValueError("no hypothesis brought 3 correspondences within %g" % thr)
    T = best.T
    info = {"source_down": down[0], "target_down": down[1], "correspondences": matches.corr, "ransac": best,
            "distance_threshold": thr}
    if refine:
        from .icp import icp_point_to_plane
        # the clouds overlap in part only: pairs farther apart than RANSAC's threshold belong to the rest and stay out of ICP
        T, info["icp"] = icp_point_to_plane(down[0], down[1], tgt_normals=nrm[1], init=T, max_dist=thr, ctx=ctx)
    return T, info


def register_colored(src, src_rgba, tgt, tgt_rgba, voxel_sizes=(0.04, 0.02, 0.01), iters=(50, 30, 14), init=None, k=None, i_max=None,
                     lambda_geometric=None, max_dist_voxels=2.0, ctx=None):
    """(T, info): coloured ICP coarse to fine (colored_icp.icp_colored has the pairwise step; no parity with Open3D's
    colored_icp recipe is claimed).  Per scale s: both clouds are voxel-downsampled WITH colour to voxel_sizes[s], the target gets
    normals and colour gradients from its k nearest neighbours, and icp_colored runs iters[s] iterations from the previous scale's
    T with pairs farther apart than max_dist_voxels x voxel_sizes[s] left out.  voxel_sizes: coarse to fine, in the clouds' unit.
    info: one icp_colored info per scale under "scales", with the voxel size and the downsampled sizes.  ValueError when a scale's
    step is undefined (status 1) or a cloud has fewer than 6 occupied voxels."""
    from . import colored_icp as CI, voxelmap
    from .normals import estimate_normals
    src, tgt = _cloud(src), _cloud(tgt)
    src_w, tgt_w = colour_words(src_rgba, src.shape[0], "src_rgba"), colour_words(tgt_rgba, tgt.shape[0], "tgt_rgba")
    try:
        sizes, its = [float(v) for v in voxel_sizes], [int(v) for v in iters]
    except (TypeError, ValueError):
        raise ValueError("voxel_sizes must be numbers and iters integers")
    if not sizes or len(sizes) != len(its):
        raise ValueError("voxel_sizes and iters must have the same length >= 1, got %d and %d" % (len(sizes), len(its)))
    for v in sizes:
        _check_positive(v, "voxel size")
    if any(i < 1 for i in its):
        raise ValueError("every entry of iters must be >= 1, got %r" % (its,))
    k = CI.K if k is None else _check_k(k)
    i_max = CI.I_MAX if i_max is None else i_max
    lam = CI.LAMBDA_GEOMETRIC if lambda_geometric is None else lambda_geometric
    CI.photo_weight(lam)
    far = _check_positive(max_dist_voxels, "max_dist_voxels")
    T = np.eye(4)
    if init is not None:
        T = np.array(init, dtype=np.float64)
        if T.shape != (4, 4) or not np.isfinite(T).all():
            raise ValueError("init must be a finite 4x4 matrix")
    ctx = ctx or default_context()
    info = {"scales": []}
    for vs, it in zip(sizes, its):
        ds, dt = voxelmap.voxel_down_sample(src, vs, rgba=src_w, ctx=ctx), voxelmap.voxel_down_sample(tgt, vs, rgba=tgt_w, ctx=ctx)
        if ds.xyz.shape[0] < 6 or dt.xyz.shape[0] < 6:
            raise ValueError("a cloud has fewer than 6 occupied voxels at voxel size %g" % vs)
        nrm = estimate_normals(dt.xyz, k, ctx=ctx).normals
        T, one = CI.icp_colored(ds.xyz, ds.rgba, dt.xyz, dt.rgba, tgt_normals=nrm, init=T, max_iter=it, max_dist=far * vs,
                                lambda_geometric=lam, i_max=i_max, k=k, ctx=ctx)
        one.update({"voxel_size": vs, "source_points": int(ds.xyz.shape[0]), "target_points": int(dt.xyz.shape[0])})
        info["scales"].append(one)
        if one["status"]:
            raise ValueError("coloured ICP step undefined at voxel size %g: fewer than 6 pairs, or geometry and colour together "
                             "leave a freedom unconstrained" % vs)
    return T, info
