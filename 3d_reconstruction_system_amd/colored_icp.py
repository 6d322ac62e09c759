"""Coloured ICP on the MI355X: cloud-to-cloud registration whose pairs carry a photometric residual next to the point-to-plane
one (Park, Zhou and Koltun, ICCV 2017 -- what users of Open3D call registration_colored_icp; no parity with Open3D is claimed).
It registers where the geometry alone leaves a freedom open: one wall, a floor, parallel walls, a corridor.  Semantics:
include/r3d.h ("Coloured ICP") and DESIGN.md section 4.5t.

colour_gradients gives every point of a coloured cloud its intensity and the gradient of the intensity over its tangent plane;
icp_colored is the pairwise registration; registration.register_colored the coarse-to-fine recipe over voxel sizes.  Colours are
the [N] uint32 words r | g << 8 | b << 16 of fuse_frames_rgb, voxel_down_sample and TSDFVolume.extract_point_cloud.
"""
import collections
import math

import numpy as np

from . import _lib as L
from ._args import colour_words as _words, positive as _positive
from .device import default_context
from .icp import NNIndex, STATE_DOUBLES
from .normals import _check_k, _check_radius
from .outliers import Cloud, _cloud

_Cloud = Cloud            # the name this class had while it was private: callers written against it keep working

COLOR_SUMS = 31            # R3D_COLOR_ICP_SUMS: the 29 plane sums, the photometric pair count, the sum of rI^2
# defaults from the sweep of DESIGN.md section 4.5t (one scene: a starting point, not a law)
K = 8                      # neighbours behind a colour gradient
I_MAX = 40.0               # the largest |intensity difference| a pair may have (tracking.I_MAX)
LAMBDA_GEOMETRIC = 0.968   # Park et al.'s weight of the geometric term

ColourGradients = collections.namedtuple("ColourGradients", ["intensity", "gradient", "count"])
ColourGradients.__doc__ = ("Intensity [N] float32 in 0..255, its tangent-plane gradient [N,3] float32 per length unit (NaN rows: no "
                           "gradient), neighbours used [N] uint32.")


def _normals(normals, n):
    nrm = np.asarray(normals)
    if nrm.dtype.kind != "f" or nrm.shape != (n, 3):
        raise ValueError("normals must be a float [%d,3] array, got %s %r" % (n, nrm.dtype, nrm.shape))
    return np.ascontiguousarray(nrm, dtype=np.float32)


def photo_weight(lambda_geometric):
    """w_photo = ((1 - lambda) / lambda) / 255^2: Park et al.'s objective (1 - lambda) E_colour + lambda E_geometry divided by
    lambda, with intensities in 0..255 where theirs are in 0..1."""
    try:
        lam = float(lambda_geometric)
    except (TypeError, ValueError):
        raise ValueError("lambda_geometric must be in (0, 1], got %r" % (lambda_geometric,))
    if not (0.0 < lam <= 1.0):
        raise ValueError("lambda_geometric must be in (0, 1], got %r" % (lambda_geometric,))
    return ((1.0 - lam) / lam) / 255.0 ** 2


def intensity(rgba):
    """[N] float32: I = (0.299f R + 0.587f G) + 0.114f B of colour words, the library's rule evaluated in f32 as written (one
    multiply or add per rounding), so these are the bits r3d_color_gradient_knn writes."""
    w = np.asarray(rgba, dtype=np.uint32)
    f = np.float32
    r, g, b = (w & 255).astype(f), ((w >> 8) & 255).astype(f), ((w >> 16) & 255).astype(f)
    return (f(0.299) * r + f(0.587) * g) + f(0.114) * b


def colour_gradients_device(index, k, d_normals, d_rgba, d_intensity, d_grad, d_count=None, radius=None):
    """r3d_color_gradient_knn on an NNIndex over a device cloud and device pointers; asynchronous."""
    k, r = _check_k(k), _check_radius(radius)
    L.check(index.ctx.lib.r3d_color_gradient_knn(index.handle, k, r, d_normals, d_rgba, d_intensity, d_grad, d_count))


def colour_gradients(tgt, tgt_rgba, normals, k=K, radius=None, ctx=None):
    """ColourGradients of a coloured cloud with normals: per point the intensity of its colour and the gradient of the intensity
    over its tangent plane, fitted to its k nearest neighbours (those within `radius` when given)."""
    xyz, k, r = _cloud(tgt), _check_k(k), _check_radius(radius)
    n = xyz.shape[0]
    rgba, nrm = _words(tgt_rgba, n, "tgt_rgba"), _normals(normals, n)
    if n == 0:
        return ColourGradients(np.zeros(0, np.float32), np.zeros((0, 3), np.float32), np.zeros(0, np.uint32))
    with Cloud(ctx or default_context(), xyz) as c:
        d_n, d_w = c.upload(nrm), c.upload(rgba)
        d_i, d_g, d_c = c.alloc(n * 4), c.alloc(n * 12), c.alloc(n * 4)
        L.check(c.ctx.lib.r3d_color_gradient_knn(c.index.handle, k, r, d_n.ptr, d_w.ptr, d_i.ptr, d_g.ptr, d_c.ptr))
        return ColourGradients(d_i.download(np.float32, n), d_g.download_array(np.float32, (n, 3)), d_c.download(np.uint32, n))


def icp_colored(src, src_rgba, tgt, tgt_rgba, tgt_normals=None, init=None, max_iter=30, max_dist=None, lambda_geometric=LAMBDA_GEOMETRIC,
                i_max=I_MAX, k=K, w_photo=None, ctx=None):
    """(T, info): the rigid T (4x4) with tgt ~ T src from coloured clouds.  Every iteration, all on the GPU with no host round
    trip: exact nearest neighbours -> per pair the point-to-plane residual and, through the target's intensity gradient, a
    photometric one -> 31 sums -> 6x6 solve -> move.  tgt_normals=None: normals.estimate_normals(tgt, k).
    init: 4x4 rough pose; None = identity.  max_dist: pairs farther apart than this never take part.
    lambda_geometric in (0, 1]: Park et al.'s balance, turned into w_photo = ((1 - lambda) / lambda) / 255^2; w_photo= gives the
    weight of a photometric pair against a geometric pair's 1 directly.  i_max: the largest |intensity difference| a pair may have.
    info: pairs, rms (geometric, of the last step), photo_pairs, photo_rms, status (1: some step was undefined and skipped -- too
    few pairs, or geometry and colour together still leave a freedom open), iterations, rms_history."""
    src, tgt = _cloud(src), _cloud(tgt)
    n, m = src.shape[0], tgt.shape[0]
    if m < 1 or n < 6:
        raise ValueError("need a target cloud and at least 6 source points")
    src_w, tgt_w = _words(src_rgba, n, "src_rgba"), _words(tgt_rgba, m, "tgt_rgba")
    nrm = None if tgt_normals is None else _normals(tgt_normals, m)
    k = _check_k(k)
    w = photo_weight(lambda_geometric) if w_photo is None else float(w_photo)
    if not (math.isfinite(w) and w >= 0.0):
        raise ValueError("w_photo must be finite and >= 0, got %r" % (w_photo,))
    i_max = _positive(i_max, "i_max")
    max_d2 = -1.0 if max_dist is None else _positive(max_dist, "max_dist") ** 2
    if isinstance(max_iter, bool) or not isinstance(max_iter, (int, np.integer)) or int(max_iter) < 1:
        raise ValueError("max_iter must be an integer >= 1, got %r" % (max_iter,))
    T0 = np.eye(4)
    if init is not None:
        T0 = np.array(init, dtype=np.float64)
        if T0.shape != (4, 4) or not np.isfinite(T0).all():
            raise ValueError("init must be a finite 4x4 matrix")
    ctx = ctx or default_context()
    if nrm is None:
        from .normals import estimate_normals
        nrm = estimate_normals(tgt, k, ctx=ctx).normals
    with Cloud(ctx, tgt) as c:
        lib, h = ctx.lib, ctx.handle
        d_n, d_w = c.upload(nrm), c.upload(tgt_w)
        d_i, d_g = c.alloc(m * 4), c.alloc(m * 12)
        L.check(lib.r3d_color_gradient_knn(c.index.handle, k, 0.0, d_n.ptr, d_w.ptr, d_i.ptr, d_g.ptr, None))
        # the source: moved by init, put into the index's order where it lies then (rigid moves preserve the order), its
        # intensities permuted alongside
        d_src, d_src0, d_perm = c.upload(src), c.alloc(n * 12), c.alloc(n * 4)
        if init is not None:
            L.check(lib.r3d_apply_T(h, d_src.ptr, L.F32, n, np.ascontiguousarray(T0).ctypes.data, d_src.ptr, L.F32))
        c.index.sort_cloud(d_src.ptr, n, d_perm.ptr)
        perm = d_perm.download(np.uint32, n)
        d_si = c.upload(intensity(src_w)[perm])
        d_idx, d_d2 = c.alloc(n * 4), c.alloc(n * 4)
        d_state, d_sums = c.alloc(STATE_DOUBLES * 8), c.alloc(COLOR_SUMS * 8)
        L.check(lib.r3d_icp_state_reset(h, d_state.ptr))
        L.check(lib.r3d_memcpy_d2d(h, d_src0.ptr, d_src.ptr, n * 12))
        L.check(lib.r3d_icp_iterate_color(h, c.index.handle, d_src0.ptr, d_src.ptr, d_si.ptr, n, d_n.ptr, d_i.ptr, d_g.ptr, d_idx.ptr,
                                          d_d2.ptr, int(max_iter), max_d2, w, i_max, d_state.ptr, d_sums.ptr))
        st, s = d_state.download(np.float64, STATE_DOUBLES), d_sums.download(np.float64, COLOR_SUMS)
    it = int(st[32])
    info = {"pairs": float(st[35]), "rms": float(st[34]), "photo_pairs": float(s[29]),
            "photo_rms": float(np.sqrt(s[30] / s[29])) if s[29] > 0 else 0.0, "status": int(st[33]), "iterations": it,
            "rms_history": st[48:48 + min(it, STATE_DOUBLES - 48)].tolist(), "w_photo": w}
    return st[0:16].reshape(4, 4) @ T0, info
