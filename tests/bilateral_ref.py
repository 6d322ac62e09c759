"""NumPy restatement of include/r3d.h "Depth bilateral filter", written from the header text.  The filter takes the weight tables as
arguments, so with the library's own tables (tracking.bilateral_weights) it reproduces the device output bit for bit; weights()
restates the tables themselves with np.exp.  Also here: the organised normals of a camera-frame vertex map (r3d_normals_organized's
rule, in double; used to measure what the filter does for the normals) and the seeded noisy room frame the tests share."""
import numpy as np

F = np.float32
BINS = 256
MAX_RADIUS = 8


def weights(radius, sigma_s, sigma_r):
    """(spatial [2r+1, 2r+1] f32, range [256] f32, cut f32, inv_step f32): host doubles rounded once to f32"""
    r = int(radius)
    dy, dx = np.meshgrid(np.arange(-r, r + 1), np.arange(-r, r + 1), indexing="ij")
    spatial = np.exp(-(dx * dx + dy * dy).astype(np.float64) / (2.0 * float(sigma_s) * float(sigma_s))).astype(F)
    t = 3.0 * np.arange(BINS, dtype=np.float64) / 256.0
    rng = np.exp(-0.5 * t * t).astype(F)
    return spatial, rng, F(3.0 * float(sigma_r)), F(256.0 / (3.0 * float(sigma_r)))


def valid(d):
    return np.isfinite(d) & (d > 0)


def depth_bilateral(depth, radius, spatial, rng, cut, inv_step):
    """[H,W] f32.  Every pixel's taps are visited dy outer, dx inner, one tap of all pixels at a time: each pixel's num and den
    grow in the header's order, every operation a separately rounded f32 one."""
    d = np.ascontiguousarray(depth, dtype=F)
    h, w = d.shape
    r = int(radius)
    spatial, rng = np.asarray(spatial, dtype=F).reshape(2 * r + 1, 2 * r + 1), np.asarray(rng, dtype=F).reshape(BINS)
    cut, inv_step = F(cut), F(inv_step)
    ok = valid(d)
    dc = np.where(ok, d, F(1.0))
    num, den = np.zeros((h, w), dtype=F), np.zeros((h, w), dtype=F)
    for dy in range(-r, r + 1):
        for dx in range(-r, r + 1):
            tap, tap_ok = np.zeros((h, w), dtype=F), np.zeros((h, w), dtype=bool)
            v0, v1, u0, u1 = max(0, -dy), min(h, h - dy), max(0, -dx), min(w, w - dx)
            if v0 >= v1 or u0 >= u1:
                continue                                               # every tap of this offset lies outside the raster
            src = d[v0 + dy:v1 + dy, u0 + dx:u1 + dx]
            tap_ok[v0:v1, u0:u1] = valid(src)
            tap[v0:v1, u0:u1] = np.where(valid(src), src, F(0.0))
            a = np.abs(tap - dc)
            take = ok & tap_ok & (a <= cut)
            k = np.minimum(BINS - 1, np.where(take, a * inv_step, F(0.0)).astype(np.int32))
            wgt = spatial[dy + r, dx + r] * rng[k]
            num = np.where(take, num + wgt * tap, num)
            den = np.where(take, den + wgt, den)
    assert num.dtype == F and den.dtype == F
    return np.where(ok, num / np.where(ok, den, F(1.0)), F(0.0)).astype(F)


def normals_organized(vertex, max_jump):
    """[H,W,3] float64 unit normals of a camera-frame vertex map, turned towards the origin; the zero vector on the border, where
    the centre or one of the four neighbours is non-finite or at the origin, across a range jump of more than max_jump x the
    centre's range, and where the cross product vanishes (include/r3d.h: r3d_normals_organized)."""
    p = np.asarray(vertex, dtype=np.float64)
    h, w, _ = p.shape
    n = np.zeros((h, w, 3))
    if h < 3 or w < 3:
        return n
    rng = np.sqrt((p * p).sum(-1))
    good = np.isfinite(p).all(-1) & (rng > 0)
    c = (slice(1, -1), slice(1, -1))
    nb = [(slice(1, -1), slice(2, None)), (slice(1, -1), slice(0, -2)), (slice(2, None), slice(1, -1)), (slice(0, -2), slice(1, -1))]
    keep = good[c].copy()
    with np.errstate(invalid="ignore"):
        for s in nb:
            keep &= good[s] & (np.abs(rng[s] - rng[c]) <= max_jump * rng[c])
        a, b = p[nb[0]] - p[nb[1]], p[nb[2]] - p[nb[3]]
        m = np.cross(a, b)
        length = np.sqrt((m * m).sum(-1))
        keep &= np.isfinite(length) & (length > 0)
        m = m / np.where(keep, length, 1.0)[..., None]
        m = np.where(((m * p[c]).sum(-1) > 0)[..., None], -m, m)
    n[c] = np.where(keep[..., None], m, 0.0)
    return n


def mean_normal_angle_deg(normal, normal_clean):
    """mean angle in degrees between two normal maps over the pixels where both have a normal; also that pixel count"""
    both = (np.abs(normal).sum(-1) > 0) & (np.abs(normal_clean).sum(-1) > 0)
    cosine = np.clip((normal[both] * normal_clean[both]).sum(-1), -1.0, 1.0)
    return float(np.degrees(np.arccos(cosine)).mean()), int(both.sum())


# The noisy frame of the tests and of DESIGN 4.5q: the scene of test_gpu_track.test_frame_to_model_on_a_real_volume (16 room_views
# of 96 x 128, pose 2 as the guess, the new frame 2 degrees of yaw and 0.05 m away), z noise of 0.5 % (15 mm at 3 m), filtered with
# a 7 x 7 window, sigma_s 2 pixels, sigma_r 0.05 m (cut 0.15 m).
NOISE_SIGMA, NOISE_SEED = 0.005, 7
FILTER = (3, 2.0, 0.05)
MAX_JUMP = 0.05


def room_frame():
    """dict: H, W, K, n_frames, i, depths / quats / ts (the views that fill the volume), guess (pose row i), clean and noisy
    (the new frame, f32), true_row"""
    import importlib

    import track_ref as TR
    from helpers import PKG
    syn = importlib.import_module(PKG + ".synthetic")
    H, W, n_frames, i = 96, 128, 16, 2
    depths, quats, ts, K = syn.room_views(n_frames, H, W, seed=0)
    guess = TR.pose_row(quats[i], ts[i])
    T_i = TR.pose_matrix(guess)
    c_i = -T_i[:3, :3].T @ T_i[:3, 3]
    yaw_i = 2 * np.pi * i / n_frames + 0.1
    z, q, t, _ = syn.room_view(H, W, yaw_i + np.radians(2.0), c_i + np.array([0.03, 0.0, 0.04]))
    return {"H": H, "W": W, "K": K, "n_frames": n_frames, "i": i, "depths": depths, "quats": quats, "ts": ts, "guess": guess,
            "yaw": yaw_i, "centre": c_i, "clean": z.astype(F), "noisy": noisy(z, NOISE_SIGMA, NOISE_SEED), "true_row": TR.pose_row(q, t)}


def noisy(z, sigma, seed):
    """z (1 + sigma N(0, 1)) as f32: multiplicative Gaussian noise on z, as synthetic.two_views makes it"""
    rng = np.random.default_rng(seed)
    return (np.asarray(z, dtype=np.float64) * (1.0 + rng.normal(size=np.shape(z)) * sigma)).astype(F)
