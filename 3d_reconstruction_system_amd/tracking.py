"""Frame-to-model tracking on the MI355X: projective point-to-plane ICP of a new depth frame against the vertex and normal map a
TSDF volume predicts for a pose (TSDFVolume.raycast).  The model maps are organised rasters, so a source point's partner is one
projection and one gather away -- no nearest-neighbour index.  Semantics: include/r3d.h ("TSDF tracking"), DESIGN.md section 4.5m.

track_sums is one association pass from host arrays (the 29 sums of the point-to-plane step, the per-pixel match and residual);
TrackDevice keeps the maps and the ICP state in HBM and runs whole iterations without a host round trip.  The whole step for one
depth frame -- ray cast, unproject, normals, loop, pose -- is TSDFVolume.track; with pyramid_iters it runs coarse to fine over a
depth pyramid (depth_half, pyramid_intrinsics, pyramid_shape: include/r3d.h "Depth pyramid").

With a colour volume the loop can carry a photometric term next to the geometric one (include/r3d.h "TSDF colour tracking",
DESIGN.md section 4.5p): intensity_map makes the intensity and gradient maps both sides read, TrackDevice takes them as
src_intensity= / model_packed= and runs sums_rgb / iterate_rgb, and TSDFVolume.track(rgb=) is the whole step.

depth_bilateral smooths a depth raster without mixing surfaces, from the host-made weight tables bilateral_weights returns
(include/r3d.h "Depth bilateral filter"); TSDFVolume.track(bilateral=) tracks on the filtered frame.
"""
import numpy as np

from . import _lib as L
from .device import default_context
from .icp import PLANE_SUMS, STATE_DOUBLES, STATE_HISTORY

MAX_ITERS = STATE_DOUBLES - STATE_HISTORY   # what the state's history holds
MAX_LEVELS = 8                              # R3D_TRACK_MAX_LEVELS
RGB_SUMS = PLANE_SUMS + 2                   # [29] the photometric pair count, [30] the sum of rI^2
# the colour term's defaults, from the sweep of DESIGN.md section 4.5p: the weight of a photometric pair against a geometric
# pair's 1 (metres^2 per intensity^2, intensities in 0..255) and the largest |intensity difference| a pair may have
PHOTO_WEIGHT = 1e-5
I_MAX = 40.0


def pyramid_intrinsics(K, level):
    """(fx, fy, cx, cy) after `level` halvings of the raster (r3d_camera_half's arithmetic, in double): a coarse pixel u' stands
    for the fine pixels 2 u' and 2 u' + 1, whose centre is 2 u' + 0.5, so fx' = 0.5 fx and cx' = 0.5 (cx - 0.5)."""
    try:
        fx, fy, cx, cy = [float(v) for v in K]
    except (TypeError, ValueError):
        raise ValueError("intrinsics must be (fx, fy, cx, cy), got %r" % (K,))
    if isinstance(level, bool) or int(level) != level or level < 0:
        raise ValueError("level must be an integer >= 0, got %r" % (level,))
    for _ in range(int(level)):
        fx, fy, cx, cy = 0.5 * fx, 0.5 * fy, 0.5 * (cx - 0.5), 0.5 * (cy - 0.5)
    return fx, fy, cx, cy


def pyramid_shape(h, w, level):
    """(H, W) after `level` halvings: an odd last row or column is dropped each time."""
    if isinstance(level, bool) or int(level) != level or level < 0:
        raise ValueError("level must be an integer >= 0, got %r" % (level,))
    return int(h) >> int(level), int(w) >> int(level)


def pyramid_levels(pyramid_iters, h, w):
    """The iteration counts of a coarse-to-fine call as a list of ints, fine to coarse; ValueError for an empty sequence, more
    than MAX_LEVELS entries, a negative or non-integer entry, a sum over MAX_ITERS or an [h, w] raster too small to be halved
    len - 1 times."""
    try:
        entries = list(pyramid_iters)
    except TypeError:
        raise ValueError("pyramid_iters must be a sequence of iteration counts, fine to coarse, got %r" % (pyramid_iters,))
    if not 1 <= len(entries) <= MAX_LEVELS:
        raise ValueError("pyramid_iters must have 1 to %d entries, got %d" % (MAX_LEVELS, len(entries)))
    for v in entries:
        if isinstance(v, (bool, str, bytes)) or not isinstance(v, (int, float, np.integer, np.floating)) or int(v) != v or v < 0:
            raise ValueError("pyramid_iters must hold integers >= 0, got %r" % (v,))
    entries = [int(v) for v in entries]
    if sum(entries) > MAX_ITERS:
        raise ValueError("pyramid_iters must add up to at most %d, got %d" % (MAX_ITERS, sum(entries)))
    if min(pyramid_shape(h, w, len(entries) - 1)) < 1:
        raise ValueError("a %d x %d raster cannot be halved %d times" % (h, w, len(entries) - 1))
    return entries


def depth_half(depth, max_jump, ctx=None):
    """One pyramid level: the [H >> 1, W >> 1] float32 raster of a host [H,W] float32 depth raster.  Every output is the mean of
    the valid (finite, > 0) depths of its 2 x 2 block that lie within max_jump of the block's nearest one -- foreground wins, no
    depth is invented between two surfaces -- and 0 where the block has none.  max_jump >= 0, inf allowed."""
    d = np.asarray(depth)
    if d.dtype != np.float32 or d.ndim != 2 or d.shape[0] < 2 or d.shape[1] < 2:
        raise ValueError("depth must be a float32 [H,W] raster of at least 2 x 2, got %s of shape %s" % (d.dtype, list(d.shape)))
    try:
        mj = float(max_jump)
    except (TypeError, ValueError):
        raise ValueError("max_jump must be a number >= 0, got %r" % (max_jump,))
    if not mj >= 0.0:
        raise ValueError("max_jump must be >= 0, got %r" % (max_jump,))
    d = np.ascontiguousarray(d)
    c = ctx or default_context()
    h, w = d.shape
    oh, ow = pyramid_shape(h, w, 1)
    with c.buffers() as B:
        d_in, d_out = B.upload(d), B.alloc(oh * ow * 4)
        L.check(c.lib.r3d_depth_half(c.handle, d_in.ptr, 1, h, w, mj, d_out.ptr))
        return d_out.download_array(np.float32, (oh, ow))


MAX_BILATERAL_RADIUS = 8                    # R3D_BILATERAL_MAX_RADIUS
BILATERAL_RANGE_BINS = 256                  # R3D_BILATERAL_RANGE_BINS


def bilateral_args(bilateral):
    """(radius, sigma_s, sigma_r) of a `bilateral=` argument as the library takes them; ValueError otherwise"""
    try:
        radius, sigma_s, sigma_r = bilateral
        exact = not isinstance(radius, (bool, str, bytes)) and int(radius) == radius
        radius, sigma_s, sigma_r = int(radius), float(sigma_s), float(sigma_r)
    except (TypeError, ValueError, OverflowError):
        raise ValueError("bilateral must be (radius, sigma_s, sigma_r), got %r" % (bilateral,))
    if not exact or not 0 <= radius <= MAX_BILATERAL_RADIUS:
        raise ValueError("the bilateral radius must be an integer in [0, %d], got %r" % (MAX_BILATERAL_RADIUS, bilateral[0]))
    if not (np.isfinite(sigma_s) and sigma_s > 0.0 and np.isfinite(sigma_r) and sigma_r > 0.0):
        raise ValueError("sigma_s and sigma_r must be finite and > 0, got %r and %r" % (sigma_s, sigma_r))
    with np.errstate(over="ignore", under="ignore"):
        cut, inv_step = np.float32(3.0 * sigma_r), np.float32(BILATERAL_RANGE_BINS / (3.0 * sigma_r))
    if not (np.isfinite(cut) and cut > 0.0 and np.isfinite(inv_step) and inv_step > 0.0):
        raise ValueError("sigma_r = %r leaves the float32 range (cut %r, inv_step %r)" % (sigma_r, cut, inv_step))
    return radius, sigma_s, sigma_r


def bilateral_weights(radius, sigma_s, sigma_r):
    """The weight tables of the depth bilateral filter exactly as the device call uses them (include/r3d.h "Depth bilateral
    filter"): (spatial [2r+1, 2r+1] float32, range [256] float32, cut, inv_step).  spatial[dy + r, dx + r] =
    exp(-(dx^2 + dy^2) / (2 sigma_s^2)), sigma_s in pixels; range[k] = exp(-0.5 (3 k / 256)^2); cut = 3 sigma_r (metres) and
    inv_step = 256 / cut, as float32.  Host only: needs the library, not a GPU."""
    r, ss, sr = bilateral_args((radius, sigma_s, sigma_r))
    import ctypes as C
    spatial, rng = np.zeros((2 * r + 1, 2 * r + 1), dtype=np.float32), np.zeros(BILATERAL_RANGE_BINS, dtype=np.float32)
    cut, inv_step = C.c_float(0.0), C.c_float(0.0)
    L.check(L.load().r3d_bilateral_weights(r, ss, sr, spatial.ctypes.data, rng.ctypes.data, C.addressof(cut), C.addressof(inv_step)))
    return spatial, rng, float(cut.value), float(inv_step.value)


def depth_bilateral(depth, radius, sigma_s, sigma_r, ctx=None):
    """The bilateral-filtered [H,W] float32 raster of a host [H,W] float32 depth raster: every valid (finite, > 0) pixel becomes
    the weighted mean of the valid depths of its (2 radius + 1)^2 window that lie within 3 sigma_r (metres) of it, weighted by
    a Gaussian of sigma_s pixels in the image and of sigma_r in depth (bilateral_weights' tables); an invalid pixel becomes 0.
    Surfaces more than 3 sigma_r apart never mix; radius 0 returns the valid depths as they are."""
    d = np.asarray(depth)
    if d.dtype != np.float32 or d.ndim != 2 or d.shape[0] < 1 or d.shape[1] < 1:
        raise ValueError("depth must be a float32 [H,W] raster, got %s of shape %s" % (d.dtype, list(d.shape)))
    r, ss, sr = bilateral_args((radius, sigma_s, sigma_r))
    d = np.ascontiguousarray(d)
    c = ctx or default_context()
    h, w = d.shape
    with c.buffers() as B:
        d_in, d_out = B.upload(d), B.alloc(d.nbytes)
        L.check(c.lib.r3d_depth_bilateral(c.handle, d_in.ptr, 1, h, w, r, ss, sr, d_out.ptr))
        return d_out.download_array(np.float32, (h, w))


def photo_args(photo_weight, i_max):
    """(w_photo, i_max) as the library takes them (None: the defaults above); ValueError otherwise"""
    try:
        w = PHOTO_WEIGHT if photo_weight is None else float(photo_weight)
        im = I_MAX if i_max is None else float(i_max)
    except (TypeError, ValueError):
        raise ValueError("photo_weight and i_max must be numbers, got %r and %r" % (photo_weight, i_max))
    if not (np.isfinite(w) and w >= 0.0):
        raise ValueError("photo_weight must be finite and >= 0, got %r" % (photo_weight,))
    if not (np.isfinite(im) and im > 0.0):
        raise ValueError("i_max must be finite and > 0, got %r" % (i_max,))
    return w, im


def intensity_map(rgb, valid, max_jump, ctx=None):
    """(I [H,W] float32, packed [H,W,4] float32 {I, gx, gy, 0}) of a host colour image rgb [H,W,3] uint8 (R, G, B): the luma
    0.299 R + 0.587 G + 0.114 B in 0..255 and its central differences.  valid [H,W] float32 marks the pixels that count (finite
    and > 0: a depth raster); I is NaN elsewhere, and a gradient is NaN on the raster's border, next to an invalid pixel and
    across a depth jump of more than max_jump (>= 0, inf allowed)."""
    c_img, d = np.asarray(rgb), np.asarray(valid)
    if c_img.dtype != np.uint8 or c_img.ndim != 3 or c_img.shape[2] != 3 or c_img.shape[0] < 1 or c_img.shape[1] < 1:
        raise ValueError("rgb must be a uint8 [H,W,3] image, got %s of shape %s" % (c_img.dtype, list(c_img.shape)))
    if d.dtype != np.float32 or d.shape != c_img.shape[:2]:
        raise ValueError("valid must be a float32 raster of shape %s, got %s of shape %s" % (list(c_img.shape[:2]), d.dtype, list(d.shape)))
    try:
        mj = float(max_jump)
    except (TypeError, ValueError):
        raise ValueError("max_jump must be a number >= 0, got %r" % (max_jump,))
    if not mj >= 0.0:
        raise ValueError("max_jump must be >= 0, got %r" % (max_jump,))
    c_img, d = np.ascontiguousarray(c_img), np.ascontiguousarray(d)
    c = ctx or default_context()
    h, w = d.shape
    with c.buffers() as B:
        d_rgb, d_valid, d_i, d_packed = B.upload(c_img), B.upload(d), B.alloc(h * w * 4), B.alloc(h * w * 16)
        L.check(c.lib.r3d_intensity_map(c.handle, d_rgb.ptr, d_valid.ptr, 1, h, w, mj, d_i.ptr, d_packed.ptr))
        return d_i.download_array(np.float32, (h, w)), d_packed.download_array(np.float32, (h, w, 4))


def inverse_pose(pose_w2c):
    """4x4 camera -> world of a 12-double world -> camera row (R row-major, t), in the library's order:
    S[a][b] = R[b][a], S[a][3] = -((R[0][a] t0 + R[1][a] t1) + R[2][a] t2)."""
    g = _pose_row(pose_w2c, "pose_w2c")
    R, t = g[:9].reshape(3, 3), g[9:]
    S = np.zeros((4, 4), dtype=np.float64)
    for a in range(3):
        for b in range(3):
            S[a, b] = R[b, a]
        S[a, 3] = -((R[0, a] * t[0] + R[1, a] * t[1]) + R[2, a] * t[2])
    S[3, 3] = 1.0
    return S


def _matmul4(A, B):
    """A . B of two 4x4, every entry summed over m = 0..3 in ascending order from 0.0 (the device solve's loop)."""
    out = np.zeros((4, 4), dtype=np.float64)
    for r in range(4):
        for c in range(4):
            v = 0.0
            for m in range(4):
                v += A[r, m] * B[m, c]
            out[r, c] = v
    return out


def pose_from_state(T_total, S):
    """The world -> camera row (12 doubles) of M = T_total . S: R = M[:3,:3]^T, t = -R . M[:3,3]."""
    M = _matmul4(np.asarray(T_total, dtype=np.float64).reshape(4, 4), np.asarray(S, dtype=np.float64).reshape(4, 4))
    out = np.empty(12, dtype=np.float64)
    for a in range(3):
        for b in range(3):
            out[3 * a + b] = M[b, a]
        out[9 + a] = -((M[0, a] * M[0, 3] + M[1, a] * M[1, 3]) + M[2, a] * M[2, 3])
    return out


def _pose_row(p, what):
    g = np.ascontiguousarray(p, dtype=np.float64).reshape(-1)
    if g.shape != (12,):
        raise ValueError("%s must be 12 numbers (R row-major, t), got shape %s" % (what, np.shape(p)))
    return g


def _map(a, what, shape=None):
    m = np.asarray(a)
    if m.dtype != np.float32 or m.ndim != 3 or m.shape[2] != 3 or m.shape[0] < 1 or m.shape[1] < 1:
        raise ValueError("%s must be a float32 [H,W,3] map, got %s of shape %s" % (what, m.dtype, list(m.shape)))
    if shape is not None and m.shape != shape:
        raise ValueError("%s has shape %s, the source vertex map %s" % (what, list(m.shape), list(shape)))
    return np.ascontiguousarray(m)


def _gates(dist_max, cos_min):
    try:
        d, c = float(dist_max), float(cos_min)
    except (TypeError, ValueError):
        raise ValueError("dist_max and cos_min must be numbers, got %r and %r" % (dist_max, cos_min))
    if not (np.isfinite(d) and d > 0.0):
        raise ValueError("dist_max must be finite and > 0, got %r" % (dist_max,))
    if not (-1.0 <= c <= 1.0):
        raise ValueError("cos_min must be in [-1, 1], got %r" % (cos_min,))
    return d, c


def _check_inputs(src_vertex, src_normal, model_vertex, model_normal, model_pose_w2c, S, intrinsics):
    sv = _map(src_vertex, "src_vertex")
    sn = None if src_normal is None else _map(src_normal, "src_normal", sv.shape)
    mv, mn = _map(model_vertex, "model_vertex", sv.shape), _map(model_normal, "model_normal", sv.shape)
    pose = _pose_row(model_pose_w2c, "model_pose_w2c")
    S = np.ascontiguousarray(S, dtype=np.float64)
    if S.shape != (4, 4):
        raise ValueError("S must be a 4x4 (source camera -> world), got shape %s" % (S.shape,))
    try:
        K = tuple(float(v) for v in intrinsics)
    except (TypeError, ValueError):
        raise ValueError("intrinsics must be (fx, fy, cx, cy), got %r" % (intrinsics,))
    if len(K) != 4:
        raise ValueError("intrinsics must be (fx, fy, cx, cy), got %r" % (intrinsics,))
    return sv, sn, mv, mn, pose, S, K


class TrackDevice:
    """The new frame's maps (camera frame) and the model's maps (world) resident on one GPU, with the device-resident ICP state.
    src_vertex [H,W,3] float32 (fusion.unproject's rows), src_normal the same or None (no normal gate), model_vertex /
    model_normal [H,W,3] float32 as TSDFVolume.raycast returns them for the pose model_pose_w2c (12 doubles), S the 4x4 guess
    source camera -> world.  src_intensity [H,W] float32 and model_packed [H,W,4] float32 (intensity_map's two results, for the
    frame's image and for the model's) are the colour term's maps: sums_rgb and iterate_rgb need both."""

    def __init__(self, src_vertex, model_vertex, model_normal, model_pose_w2c, S, intrinsics, src_normal=None, ctx=None,
                 src_intensity=None, model_packed=None):
        sv, sn, mv, mn, self.model_pose, self.S, K = _check_inputs(src_vertex, src_normal, model_vertex, model_normal, model_pose_w2c, S,
                                                             intrinsics)
        if (src_intensity is None) != (model_packed is None):
            raise ValueError("src_intensity and model_packed go together: give both or neither")
        if src_intensity is not None:
            si, mp = np.asarray(src_intensity), np.asarray(model_packed)
            if si.dtype != np.float32 or si.shape != sv.shape[:2]:
                raise ValueError("src_intensity must be a float32 %s raster, got %s of shape %s" % (list(sv.shape[:2]), si.dtype, list(si.shape)))
            if mp.dtype != np.float32 or mp.shape != sv.shape[:2] + (4,):
                raise ValueError("model_packed must be a float32 %s map, got %s of shape %s" % (list(sv.shape[:2]) + [4], mp.dtype, list(mp.shape)))
            si, mp = np.ascontiguousarray(si), np.ascontiguousarray(mp)
        self.ctx = c = ctx or default_context()
        self.h, self.w = sv.shape[:2]
        self.n = self.h * self.w
        self.cam = c.camera(self.h, self.w, *K)
        self._buffers = B = c.buffers()   # everything below, until free()
        try:
            self.d_src_vertex, self.d_model_vertex, self.d_model_normal = B.upload(sv), B.upload(mv), B.upload(mn)
            self.d_src_normal = None if sn is None else B.upload(sn)
            self.d_src_intensity = self.d_model_packed = self.d_photo = None
            if src_intensity is not None:
                self.d_src_intensity, self.d_model_packed, self.d_photo = B.upload(si), B.upload(mp), B.alloc(self.n * 4)
            self.d_match, self.d_residual = B.alloc(self.n * 4), B.alloc(self.n * 4)
            self.d_state = B.alloc(STATE_DOUBLES * 8)
            self.state_reset()
        except BaseException:
            B.close()
            raise

    def _maps(self):
        return (self.d_src_vertex.ptr, None if self.d_src_normal is None else self.d_src_normal.ptr, self.d_model_vertex.ptr,
                self.d_model_normal.ptr, self.model_pose.ctypes.data, self.S.ctypes.data)

    def state_reset(self):
        L.check(self.ctx.lib.r3d_icp_state_reset(self.ctx.handle, self.d_state.ptr))

    def sums(self, dist_max, cos_min=-1.0):
        """One pass at the guess S itself (T_total = I): (sums [29], match [H,W] int32, residual [H,W] float32)."""
        d, cm = _gates(dist_max, cos_min)
        sums = np.zeros(PLANE_SUMS, dtype=np.float64)
        L.check(self.ctx.lib.r3d_track_accumulate(self.ctx.handle, self.cam.handle, *self._maps(), d, cm, sums.ctypes.data,
                                                  self.d_match.ptr, self.d_residual.ptr))
        return (sums, self.d_match.download(np.int32, self.n).reshape(self.h, self.w),
                self.d_residual.download(np.float32, self.n).reshape(self.h, self.w))

    def iterate(self, n_iters, dist_max, cos_min=-1.0):
        """n_iters whole iterations (associate at T_total . S, 29 sums, solve, T_total updated) with no host round trip."""
        d, cm = _gates(dist_max, cos_min)
        n_iters = int(n_iters)
        if not 0 <= n_iters <= MAX_ITERS:
            raise ValueError("n_iters must be in [0, %d], got %d" % (MAX_ITERS, n_iters))
        L.check(self.ctx.lib.r3d_track_iterate(self.ctx.handle, self.cam.handle, *self._maps(), d, cm, n_iters, self.d_state.ptr))

    def _photo(self, photo_weight, i_max):
        if self.d_src_intensity is None:
            raise ValueError("the colour term needs src_intensity= and model_packed= (tracking.intensity_map makes them)")
        return (self.d_src_intensity.ptr, self.d_model_packed.ptr) + photo_args(photo_weight, i_max)

    def sums_rgb(self, dist_max, cos_min=-1.0, photo_weight=None, i_max=None):
        """sums() with the colour term: (sums [31], match [H,W] int32, residual [H,W] float32, photo [H,W] float32).  The first
        29 sums hold both terms' normal equations ([0], [1]: the geometric pairs alone), [29] and [30] the photometric pair count
        and the sum of their squared intensity differences; photo is that difference per pixel, NaN where no pair entered."""
        d, cm = _gates(dist_max, cos_min)
        photo = self._photo(photo_weight, i_max)
        sums = np.zeros(RGB_SUMS, dtype=np.float64)
        L.check(self.ctx.lib.r3d_track_accumulate_rgb(self.ctx.handle, self.cam.handle, *self._maps(), d, cm, *photo, sums.ctypes.data,
                                                      self.d_match.ptr, self.d_residual.ptr, self.d_photo.ptr))
        return (sums, self.d_match.download(np.int32, self.n).reshape(self.h, self.w),
                self.d_residual.download(np.float32, self.n).reshape(self.h, self.w),
                self.d_photo.download(np.float32, self.n).reshape(self.h, self.w))

    def iterate_rgb(self, n_iters, dist_max, cos_min=-1.0, photo_weight=None, i_max=None):
        """iterate() with the colour term, on the same state."""
        d, cm = _gates(dist_max, cos_min)
        photo = self._photo(photo_weight, i_max)
        n_iters = int(n_iters)
        if not 0 <= n_iters <= MAX_ITERS:
            raise ValueError("n_iters must be in [0, %d], got %d" % (MAX_ITERS, n_iters))
        L.check(self.ctx.lib.r3d_track_iterate_rgb(self.ctx.handle, self.cam.handle, *self._maps(), d, cm, *photo, n_iters,
                                                   self.d_state.ptr))

    def state(self):
        st = self.d_state.download(np.float64, STATE_DOUBLES)
        it = int(st[32])
        return {"T_total": st[0:16].reshape(4, 4).copy(), "T_step": st[16:32].reshape(4, 4).copy(), "iterations": it,
                "degenerate": bool(st[33]), "rms": float(st[34]), "pairs": float(st[35]),
                "rms_history": st[STATE_HISTORY:STATE_HISTORY + min(it, MAX_ITERS)].tolist()}

    def pose(self):
        """The tracked world -> camera row (12 doubles) of the state as it stands."""
        return pose_from_state(self.state()["T_total"], self.S)

    def free(self):
        self.ctx.sync()
        self._buffers.close()


def track_sums(src_vertex, model_vertex, model_normal, model_pose_w2c, S, intrinsics, dist_max, cos_min=-1.0, src_normal=None,
               ctx=None):
    """One association pass from host arrays: (sums [29] float64, match [H,W] int32, residual [H,W] float32).  match holds the
    model pixel vj W + uj of every matched source pixel, else the reject code: -1 no source point, -2 projects outside the model
    image, -3 no model surface there, -4 farther than dist_max, -5 normals disagree (only with src_normal)."""
    _gates(dist_max, cos_min)
    dev = TrackDevice(src_vertex, model_vertex, model_normal, model_pose_w2c, S, intrinsics, src_normal=src_normal, ctx=ctx)
    try:
        return dev.sums(dist_max, cos_min)
    finally:
        dev.free()
