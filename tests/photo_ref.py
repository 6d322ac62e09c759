"""NumPy restatement of include/r3d.h, "TSDF colour tracking": the intensity and gradient maps in f32, steps 11..16 of the
association pass in fp64 on top of tests/track_ref.py (steps 1..10), the 31 sums as plain fp64 sums, and the loop on the state of
tests/icp_state_ref.py.  Written from the header text, not from the kernels.  Every elementwise expression keeps the header's order
of operations, so the maps and (float) rI are comparable bit for bit.  Also the textured corridor the tests track in."""
import importlib

import numpy as np

import icp_state_ref as SR
import track_ref as TR
from helpers import PKG

F = np.float32


# ---- r3d_intensity_map -------------------------------------------------------------------------------------------------------------
def luma(rgb):
    """I = (0.299f R + 0.587f G) + 0.114f B, f32"""
    c = np.asarray(rgb)
    assert c.dtype == np.uint8 and c.shape[-1] == 3
    r, g, b = [c[..., k].astype(F) for k in range(3)]
    out = (F(0.299) * r + F(0.587) * g) + F(0.114) * b
    assert out.dtype == F
    return out


def _central(I, d, ok, axis, max_jump):
    """0.5f (I(+1) - I(-1)) along axis; NaN on the border, where the pixel or a neighbour is invalid, or across a depth jump"""
    out = np.full(I.shape, np.nan, dtype=F)
    n = I.shape[axis]
    if n < 3:
        return out
    mid, lo, hi = [tuple(slice(None) if a != axis else s for a in range(2)) for s in (slice(1, n - 1), slice(0, n - 2), slice(2, n))]
    with np.errstate(all="ignore"):
        good = ok[mid] & ok[lo] & ok[hi] & ~(np.abs(d[lo] - d[mid]) > F(max_jump)) & ~(np.abs(d[hi] - d[mid]) > F(max_jump))
        g = F(0.5) * (I[hi] - I[lo])
    assert g.dtype == F
    out[mid] = np.where(good, g, F(np.nan))
    return out


def intensity_map(rgb, valid, max_jump):
    """(I [H,W] f32, packed [H,W,4] f32 {I, gx, gy, 0}); valid [H,W] f32: a pixel counts iff its value is finite and > 0"""
    d = np.asarray(valid, dtype=F)
    with np.errstate(all="ignore"):
        ok = np.isfinite(d) & (d > 0)
    raw = luma(rgb)
    I = np.where(ok, raw, F(np.nan)).astype(F)
    gx, gy = _central(raw, d, ok, 1, max_jump), _central(raw, d, ok, 0, max_jump)
    packed = np.stack([I, gx, gy, np.zeros_like(I)], axis=-1)
    return I, np.ascontiguousarray(packed)


# ---- the association pass with the colour term -------------------------------------------------------------------------------------
REASONS = ("border", "nan_tap", "grad", "i_max")


def associate(src_vertex, src_normal, model_vertex, model_normal, model_pose, S, K, dist_max, cos_min, src_intensity, model_packed,
              w_photo, i_max, T_total=None):
    """track_ref.associate's Pass with: sums [31]; photo [H*W] f32 ((float) rI, NaN where no photometric pair entered);
    reasons {name: pixels that had a geometric pair but no photometric one, by the first test that failed}; margins: the
    distances of u, v (step 11) to an integer and of |rI| to i_max over the pixels that reached those tests."""
    out = TR.associate(src_vertex, src_normal, model_vertex, model_normal, model_pose, S, K, dist_max, cos_min, T_total)
    sv = np.asarray(src_vertex, dtype=F)
    H, W = sv.shape[:2]
    n_px = H * W
    geo = np.flatnonzero(out.match >= 0)
    x, y, z = [sv.reshape(n_px, 3)[geo, a].astype(np.float64) for a in range(3)]
    pose = np.asarray(model_pose, dtype=np.float64).reshape(12)
    Rm, tm = pose[:9].reshape(3, 3), pose[9:]
    fx, fy, cx, cy = [float(v) for v in K]
    M = TR.matmul4(np.eye(4) if T_total is None else np.asarray(T_total, dtype=np.float64), np.asarray(S, dtype=np.float64))
    MP = np.asarray(model_packed, dtype=F).reshape(n_px, 4)
    Is = np.asarray(src_intensity, dtype=F).reshape(n_px)[geo].astype(np.float64)
    with np.errstate(all="ignore"):
        p = np.stack([((M[a, 0] * x + M[a, 1] * y) + M[a, 2] * z) + M[a, 3] for a in range(3)], axis=1)
        pm = np.stack([((Rm[a, 0] * p[:, 0] + Rm[a, 1] * p[:, 1]) + Rm[a, 2] * p[:, 2]) + tm[a] for a in range(3)], axis=1)
        u = fx * (pm[:, 0] / pm[:, 2]) + cx
        v = fy * (pm[:, 1] / pm[:, 2]) + cy
        u0, v0 = np.floor(u), np.floor(v)                                                                     # 11
        inside = (u0 >= 0) & (u0 + 1.0 <= W - 1.0) & (v0 >= 0) & (v0 + 1.0 <= H - 1.0)
        fu, fv = u - u0, v - v0
        j = np.where(inside, v0 * W + u0, 0).astype(np.int64)
        j = np.minimum(j, max(n_px - W - 2, 0))                                    # (only rows that are not `inside` are clamped)
        taps = [MP[np.minimum(j + o, n_px - 1)].astype(np.float64) for o in (0, 1, W, W + 1)]                   # 12
        val = []
        for c in range(3):
            t00, t01, t10, t11 = [t[:, c] for t in taps]
            top = t00 + fu * (t01 - t00)
            bot = t10 + fu * (t11 - t10)
            val.append(top + fv * (bot - top))
        rI = val[0] - Is                                                                                      # 13
        gfx, gfy = val[1] * fx, val[2] * fy                                                                   # 14
        b0, b1 = gfx / pm[:, 2], gfy / pm[:, 2]
        b2 = -(gfx * pm[:, 0] + gfy * pm[:, 1]) / (pm[:, 2] * pm[:, 2])
        a = np.stack([(Rm[0, c] * b0 + Rm[1, c] * b1) + Rm[2, c] * b2 for c in range(3)], axis=1)
        ok_r, ok_a = np.isfinite(rI), np.isfinite(a).all(axis=1)                                              # 15
        ok_i = np.abs(rI) <= i_max
    live = inside & ok_r & ok_a & ok_i
    out.reasons = {"border": int((~inside).sum()), "nan_tap": int((inside & ~ok_r).sum()), "grad": int((inside & ok_r & ~ok_a).sum()),
                   "i_max": int((inside & ok_r & ok_a & ~ok_i).sum())}
    uv = np.concatenate([u, v])
    out.floor_margin = float(np.abs(uv - np.round(uv)).min()) if uv.size else 1.0
    gate = np.abs(np.abs(rI[inside & ok_r & ok_a]) - i_max)
    out.i_max_margin = float(gate.min()) if gate.size else 1.0
    photo = np.full(n_px, np.nan, dtype=F)
    photo[geo[live]] = rI[live].astype(F)
    out.photo = photo
    pl, al, rl = p[live], a[live], rI[live]
    J = np.concatenate([np.cross(pl, al), al], axis=1) if len(pl) else np.zeros((0, 6))
    out.J, out.rI, out.pixels = J, rl, geo[live]
    sums = np.zeros(31)
    sums[:29] = out.sums
    wJ = w_photo * J
    sums[2:8] += (wJ * rl[:, None]).sum(axis=0)                                                               # 16
    k = 8
    for r in range(6):
        for c in range(r, 6):
            sums[k] += np.sum(wJ[:, r] * J[:, c])
            k += 1
    sums[29] = float(len(rl))
    sums[30] = np.sum(rl * rl)
    out.sums = sums
    return out


def loop(src_vertex, src_normal, model_vertex, model_normal, model_pose, S, K, dist_max, cos_min, n_iters, src_intensity=None,
         model_packed=None, w_photo=0.0, i_max=1.0):
    """(state [512], info): n_iters iterations of associate -> sums -> step on icp_state_ref's state.  Without the two intensity
    maps it is the depth-only loop (track_ref.associate)."""
    icp = importlib.import_module(PKG + ".icp")
    st = SR.reset()
    info = {"photo_pairs": 0.0, "photo_rms": 0.0}
    for _ in range(n_iters):
        T_total = st[SR.T_TOTAL:SR.T_TOTAL + 16].reshape(4, 4)
        if src_intensity is None:
            a = TR.associate(src_vertex, src_normal, model_vertex, model_normal, model_pose, S, K, dist_max, cos_min, T_total)
        else:
            a = associate(src_vertex, src_normal, model_vertex, model_normal, model_pose, S, K, dist_max, cos_min, src_intensity,
                          model_packed, w_photo, i_max, T_total)
            info["photo_pairs"] = float(a.sums[29])
            info["photo_rms"] = float(np.sqrt(a.sums[30] / a.sums[29])) if a.sums[29] > 0 else 0.0
        rms = float(np.sqrt(max(a.sums[1], 0.0) / a.sums[0])) if a.sums[0] > 0 else 0.0
        try:
            T, _ = icp.plane_step_from_sums(a.sums[:29])
            bad = 0
        except ValueError:
            T, bad = np.eye(4), 1
        st = SR.advance(st, T, rms, bad, a.sums[0])
    info.update(status=int(st[SR.STATUS]), pairs=float(st[SR.PAIRS]), rms=float(st[SR.RMS]), iterations=int(st[SR.ITERS]))
    return st, info


def track(src_vertex, src_normal, model_vertex, model_normal, guess_row, K, dist_max, cos_min, n_iters, src_intensity=None,
          model_packed=None, w_photo=0.0, i_max=1.0):
    """r3d_tsdf_track_rgb (r3d_tsdf_track without the intensity maps) from ready-made maps: (pose row, info)"""
    S = TR.inverse_pose(guess_row)
    st, info = loop(src_vertex, src_normal, model_vertex, model_normal, guess_row, S, K, dist_max, cos_min, n_iters, src_intensity,
                    model_packed, w_photo, i_max)
    if info["status"]:
        return np.asarray(guess_row, dtype=np.float64).reshape(12).copy(), info
    return TR.pose_from(st[SR.T_TOTAL:SR.T_TOTAL + 16].reshape(4, 4), S), info


# ---- the textured corridor ---------------------------------------------------------------------------------------------------------
# A box that is 2 m wide, with its floor 1 m below the cameras (y points down), and so long and so high that its ends and its
# ceiling lie far outside the volume: what the volume holds is a floor and two parallel walls.  Sliding along z changes no depth.
CORRIDOR_LO = np.array([-1.0, -40.0, -40.0])
CORRIDOR_HI = np.array([1.0, 1.0, 40.0])
CORRIDOR_VS, CORRIDOR_TR = 0.05, 0.15
CORRIDOR_ORIGIN = (-1.3, -0.9, 0.3)
CORRIDOR_DIMS = (52, 44, 84)            # x -1.3 .. 1.3, y -0.9 .. 1.3, z 0.3 .. 4.5
CORRIDOR_SHAPE = (48, 64)
CORRIDOR_PITCH = 0.25                   # looking slightly down: floor and both walls in sight
CORRIDOR_T_FAR = 4.0


def texture(world):
    """[...,3] uint8 colour of world points: per channel a sum of sinusoids along z (the corridor's axis) and across it, with
    wavelengths of 8 to 31 voxels"""
    w = np.asarray(world, dtype=np.float64)
    s = w[..., 0] + w[..., 1]                                   # across: runs up the walls and over the floor
    z = w[..., 2]
    ch = []
    for k, (lz, ls, ph) in enumerate([(0.9, 1.2, 0.3), (0.6, 0.8, 1.1), (0.4, 1.0, 2.0)]):
        val = 128.0 + 60.0 * np.sin(2 * np.pi * z / lz + ph) + 45.0 * np.sin(2 * np.pi * (z + 0.5 * s) / (1.7 * lz) + 2 * ph) \
            + 20.0 * np.sin(2 * np.pi * s / ls + k)
        ch.append(np.clip(np.round(val), 0, 255))
    return np.stack(ch, axis=-1).astype(np.uint8)


def corridor_view(z_centre, x_centre=0.0, yaw=0.0, shape=CORRIDOR_SHAPE):
    """(depth f32 [H,W] with 0 beyond CORRIDOR_T_FAR, rgb uint8 [H,W,3], pose row [12], K) of a camera in the corridor at
    (x_centre, 0, z_centre) looking along +z"""
    syn = importlib.import_module(PKG + ".synthetic")
    h, w = shape
    z, q, t, K = syn.room_view(h, w, yaw, np.array([x_centre, 0.0, z_centre]), pitch=CORRIDOR_PITCH, lo=CORRIDOR_LO, hi=CORRIDOR_HI)
    row = TR.pose_row(q, t)
    T = TR.pose_matrix(row)
    cam = TR.camera_points(z, K)
    world = (cam.reshape(-1, 3) - T[:3, 3]) @ T[:3, :3]
    rgb = texture(world).reshape(h, w, 3)
    depth = np.where(z <= CORRIDOR_T_FAR, z, 0.0).astype(F)
    return depth, rgb, row, K


def corridor_frames(zs):
    views = [corridor_view(zc) for zc in zs]
    return (np.stack([v[0] for v in views]), np.stack([v[1] for v in views]), np.stack([v[2] for v in views]), views[0][3])


def along_axis_error(row, true_row):
    """the difference of the camera centres along the corridor's axis (world z), signed"""
    Ta, Tb = TR.pose_matrix(row), TR.pose_matrix(true_row)
    ca, cb = -Ta[:3, :3].T @ Ta[:3, 3], -Tb[:3, :3].T @ Tb[:3, 3]
    return float(ca[2] - cb[2])


# ---- "dirty" inputs of the association tests ---------------------------------------------------------------------------------------
DIRTY_I_MAX = 20.0
DIRTY_MAX_JUMP = 0.25


def dirty_case(h, w, seed):
    """track_ref.analytic_case with what real maps carry, at rates that leave the colour term enough to work on: ~3 % missing
    model rows (NaN) and a few zero / infinite model normals; source rows with Z = 0, NaN, +-inf and negative z; random unit
    source normals near the model's, some zero; two colour images of the same smooth pattern, the frame's with noise so that
    some differences pass DIRTY_I_MAX, and the four maps r3d_intensity_map's restatement makes of them (the model's validity
    raster is its depth, 0 where a row is missing; the frame's the z column of its vertex map)."""
    rng = np.random.default_rng([seed, h, w, 5])
    case = TR.analytic_case(h, w, 2.0, 1.0, (0.03, 0.02, -0.04))
    n = h * w
    mv, mn, sv = [case[k].reshape(n, 3).copy() for k in ("model_vertex", "model_normal", "src_vertex")]
    Rm, tm = case["model_row"][:9].reshape(3, 3), case["model_row"][9:]
    model_depth = (mv.astype(np.float64) @ Rm[2] + tm[2]).astype(F)
    miss = rng.random(n) < 0.03
    mv[miss] = np.nan
    mn[miss] = np.nan
    model_depth[miss] = 0.0
    mn[rng.random(n) < 0.01] = 0.0
    mn[rng.random(n) < 0.005, 1] = np.inf
    kind = rng.random(n)
    sv[kind < 0.01] = 0.0
    sv[(kind >= 0.01) & (kind < 0.02), 0] = np.nan
    sv[(kind >= 0.02) & (kind < 0.03), 1] = np.inf
    sv[(kind >= 0.03) & (kind < 0.04), 2] = -np.inf
    sv[(kind >= 0.04) & (kind < 0.05), 2] *= -1.0
    base = np.nan_to_num(case["model_normal"].reshape(n, 3).astype(np.float64), nan=0.0, posinf=0.0) @ Rm.T
    sn = base + rng.normal(size=(n, 3)) * 0.25
    with np.errstate(invalid="ignore", divide="ignore"):
        sn = sn / np.linalg.norm(sn, axis=1, keepdims=True)
    sn = sn.astype(F)
    sn[rng.random(n) < 0.05] = 0.0
    sn[rng.random(n) < 0.02, 2] = np.nan
    v, u = np.meshgrid(np.arange(h), np.arange(w), indexing="ij")
    smooth = np.stack([128 + 70 * np.sin(0.12 * u + 0.07 * v + k) + 40 * np.cos(0.05 * u - 0.14 * v + 2 * k) for k in range(3)], axis=-1)
    model_rgb = np.clip(np.round(smooth), 0, 255).astype(np.uint8)
    src_rgb = np.clip(np.round(smooth + rng.normal(size=smooth.shape) * 12.0), 0, 255).astype(np.uint8)
    case.update(model_vertex=mv.reshape(h, w, 3), model_normal=mn.reshape(h, w, 3), src_vertex=sv.reshape(h, w, 3),
                src_normal=sn.reshape(h, w, 3), model_rgb=model_rgb, src_rgb=src_rgb, model_depth=model_depth.reshape(h, w))
    case["src_intensity"], _ = intensity_map(src_rgb, case["src_vertex"][..., 2], DIRTY_MAX_JUMP)
    _, case["model_packed"] = intensity_map(model_rgb, case["model_depth"], DIRTY_MAX_JUMP)
    c2w_model = TR.inverse_pose(case["model_row"])
    turn, shift, nudge = np.eye(4), np.eye(4), np.eye(4)
    turn[0, 0] = turn[2, 2] = -1.0          # half a turn about y
    shift[:3, 3] = (3.0, 0.0123, 0.0)
    nudge[:3, 3] = (0.0131, 0.0077, 0.0)    # the model's own pose would put every source point on a pixel centre: floor(u) undecided
    case["S"] = {"truth": TR.inverse_pose(case["true_row"]), "offset": c2w_model @ nudge, "behind": c2w_model @ turn,
                 "shifted": c2w_model @ shift}
    return case
