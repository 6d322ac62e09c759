"""NumPy restatement of the TSDF ray casting's specification (include/r3d.h, "TSDF ray casting"): every operation on np.float32
arrays in the written order, all pixels of a view at once, the march in a Python loop over k (only the pixels still marching
take part).  The pose preparation is float64 in the written order.  x86 f32 addition, multiplication, division, floor and sqrt are
IEEE and keep denormals, so this file defines every bit the device must produce.  Reads tsdf_ref.Volume.  Test infrastructure
only."""
import numpy as np

F = np.float32
MAX_K = 65536
NONE = np.uint32(0x7FC00000)            # the word of a missing vertex / normal component


def prepare_pose(row):
    """(R [3,3] f32, C [3] f32) of one world -> camera row (R row-major, t): C_k = -((R[0][k] t0 + R[1][k] t1) + R[2][k] t2) in
    float64, then one rounding to f32."""
    row = np.asarray(row, dtype=np.float64).reshape(12)
    R, t = row[:9].reshape(3, 3), row[9:]
    C = np.array([-((R[0, k] * t[0] + R[1, k] * t[1]) + R[2, k] * t[2]) for k in range(3)], dtype=np.float64)
    assert R.dtype == np.float64 and C.dtype == np.float64
    return R.astype(F), C.astype(F)


def _sample(vol, mw, p):
    """p: three f32 arrays.  (ok, T [8] arrays in corner order k = dx + 2 dy + 4 dz, f [3] arrays)"""
    dims = (vol.nx, vol.ny, vol.nz)
    ivs = F(1.0) / vol.vs
    g = [(p[a] - vol.o[a]) * ivs - F(0.5) for a in range(3)]
    i = [np.floor(q) for q in g]
    f = [g[a] - i[a] for a in range(3)]
    ok = np.ones(p[0].shape, bool)
    for a in range(3):
        ok &= (i[a] >= F(0.0)) & (i[a] <= F(dims[a] - 2))            # as floats: NaN fails
    idx = [np.where(ok, i[a], F(0.0)).astype(np.int64) for a in range(3)]
    for a in range(3):
        ok &= idx[a] <= dims[a] - 2                                   # (float)(n - 2) inexact: n > 2^24 + 2 only
        idx[a] = np.where(ok, idx[a], 0)
    T = []
    for k in range(8):
        dx, dy, dz = k & 1, (k >> 1) & 1, k >> 2
        x, y, z = idx[0] + dx, idx[1] + dy, idx[2] + dz
        if min(dims) < 2:                                             # no cell: nothing to read
            T.append(np.zeros(p[0].shape, F))
            ok &= False
            continue
        T.append(vol.tsdf[z, y, x])
        ok &= vol.w[z, y, x] >= mw
    assert all(q.dtype == F for q in g + i + f + T) and ivs.dtype == F
    return ok, T, f


def _trilinear(T, f):
    c00, c10 = T[0] + f[0] * (T[1] - T[0]), T[2] + f[0] * (T[3] - T[2])          # c[jy][jz]
    c01, c11 = T[4] + f[0] * (T[5] - T[4]), T[6] + f[0] * (T[7] - T[6])
    b0, b1 = c00 + f[1] * (c10 - c00), c01 + f[1] * (c11 - c01)
    S = b0 + f[2] * (b1 - b0)
    assert S.dtype == F
    return S


def _gradient(T, sa, sb, sc, fb, fc):
    d00, d10 = T[sa] - T[0], T[sa + sb] - T[sb]                                    # D[jb][jc]
    d01, d11 = T[sa + sc] - T[sc], T[sa + sb + sc] - T[sb + sc]
    e0, e1 = d00 + fb * (d10 - d00), d01 + fb * (d11 - d01)
    return e0 + fc * (e1 - e0)


def cast_view(vol, pose_row, intrinsics, shape, min_weight=1.0, step=None, t_near=0.0, t_far=np.inf):
    """One view: (depth [H,W] f32, vertex [H,W,3] f32, normal [H,W,3] f32, hit [H,W] bool)."""
    H, W = shape
    R, C = prepare_pose(pose_row)
    fx, fy, cx, cy = [F(v) for v in intrinsics]
    mw, s = F(min_weight), F(vol.vs if step is None else step)
    tn, tf = F(t_near), F(t_far)
    assert mw > 0 and s > 0 and np.isfinite(s) and np.isfinite(tn) and tn >= 0 and tf > tn
    dims = (vol.nx, vol.ny, vol.nz)
    diag = np.sqrt(float(sum((d - 1) ** 2 for d in dims)))
    assert float(vol.vs) * diag / float(s) < MAX_K
    with np.errstate(all="ignore"):
        ui = np.broadcast_to(np.arange(W).astype(F)[None, :], (H, W)).reshape(-1)
        vi = np.broadcast_to(np.arange(H).astype(F)[:, None], (H, W)).reshape(-1)
        x, y = (ui - cx) / fx, (vi - cy) / fy
        ln = np.sqrt((x * x + y * y) + F(1.0))
        n = [x / ln, y / ln, F(1.0) / ln]
        dw = [(R[0, k] * n[0] + R[1, k] * n[1]) + R[2, k] * n[2] for k in range(3)]
        assert all(q.dtype == F for q in n + dw)
        tmin, tmax = np.full(H * W, tn, F), np.full(H * W, tf, F)
        alive = np.full(H * W, min(dims) >= 2)
        for a in range(3):
            lo = vol.o[a] + F(0.5) * vol.vs
            hi = vol.o[a] + (F(dims[a] - 1) + F(0.5)) * vol.vs
            assert lo.dtype == F and hi.dtype == F
            zero = dw[a] == 0
            alive &= ~zero | ((lo <= C[a]) & (C[a] <= hi))
            q1, q2 = (lo - C[a]) / dw[a], (hi - C[a]) / dw[a]
            tmin = np.where(zero, tmin, np.fmax(tmin, np.fmin(q1, q2)))              # fmaxf / fminf: a NaN operand loses
            tmax = np.where(zero, tmax, np.fmin(tmax, np.fmax(q1, q2)))
        alive &= tmin <= tmax
        assert tmin.dtype == F and tmax.dtype == F

        act = np.flatnonzero(alive)
        prev_ok, A = np.zeros(len(act), bool), np.zeros(len(act), F)
        hit_px, hit_t = [], []
        for k in range(MAX_K + 1):
            t = tmin[act] + F(k) * s
            go = t <= tmax[act]
            act, prev_ok, A, t = act[go], prev_ok[go], A[go], t[go]
            if len(act) == 0:
                break
            ok, T, f = _sample(vol, mw, [C[a] + t * dw[a][act] for a in range(3)])
            B = np.where(ok, _trilinear(T, f), F(0.0))
            h = prev_ok & ok & (A > 0) & (B <= 0)                                   # (prev_ok: k >= 1)
            if h.any():
                r = A[h] / (A[h] - B[h])
                ts = (tmin[act[h]] + F(k - 1) * s) + r * s
                assert r.dtype == F and ts.dtype == F
                hit_px.append(act[h])
                hit_t.append(ts)
                act, ok, B = act[~h], ok[~h], B[~h]
            prev_ok, A = ok, B

        depth = np.zeros(H * W, F)
        vertex = np.full((H * W, 3), NONE, np.uint32).view(F)
        normal = np.full((H * W, 3), NONE, np.uint32).view(F)
        hit = np.zeros(H * W, bool)
        if hit_px:
            px, ts = np.concatenate(hit_px), np.concatenate(hit_t)
            ok, T, f = _sample(vol, mw, [C[a] + ts * dw[a][px] for a in range(3)])
            G = [_gradient(T, 1, 2, 4, f[1], f[2]), _gradient(T, 2, 1, 4, f[0], f[2]), _gradient(T, 4, 1, 2, f[0], f[1])]
            L = np.sqrt((G[0] * G[0] + G[1] * G[1]) + G[2] * G[2])
            assert L.dtype == F and all(q.dtype == F for q in G)
            ok &= L > 0
            px, ts, L = px[ok], ts[ok], L[ok]
            hit[px] = True
            depth[px] = ts * n[2][px]
            for a in range(3):
                vertex[px, a] = C[a] + ts * dw[a][px]
                normal[px, a] = G[a][ok] / L
    assert depth.dtype == F and vertex.dtype == F and normal.dtype == F
    return depth.reshape(H, W), vertex.reshape(H, W, 3), normal.reshape(H, W, 3), hit.reshape(H, W)


def raycast(vol, poses_w2c, intrinsics, shape, min_weight=1.0, step=None, t_near=0.0, t_far=np.inf):
    """(depth [V,H,W], vertex [V,H,W,3], normal [V,H,W,3]) f32 for poses_w2c [V,12] float64."""
    poses = np.asarray(poses_w2c, dtype=np.float64).reshape(-1, 12)
    H, W = shape
    out = [cast_view(vol, p, intrinsics, shape, min_weight, step, t_near, t_far)[:3] for p in poses]
    if not out:
        return np.zeros((0, H, W), F), np.zeros((0, H, W, 3), F), np.zeros((0, H, W, 3), F)
    return tuple(np.stack([o[j] for o in out]) for j in range(3))


def hits(depth_or_vertex):
    """the hit mask of a vertex map [..., 3] (rows that are not the missing-row NaN)"""
    return ~np.isnan(np.asarray(depth_or_vertex)[..., 0])


# ---- poses and checks shared by tests/test_raycast_host.py (asserted of this reference first) and tests/test_gpu_raycast.py -----
def look_at(centre, target, up=(0.0, 1.0, 0.0)):
    """a world -> camera row for a camera at `centre` whose +z axis points at `target` (x right, y down the image)"""
    c, tgt = np.asarray(centre, dtype=np.float64), np.asarray(target, dtype=np.float64)
    z = (tgt - c) / np.linalg.norm(tgt - c)
    x = np.cross(np.asarray(up, dtype=np.float64), z)
    x /= np.linalg.norm(x)
    y = np.cross(z, x)
    R = np.stack([x, y, z])                                   # rows: the camera axes in the world
    return np.concatenate([R.reshape(9), -R @ c])


SPHERE_K = (30.0, 30.0, 15.5, 11.5)                           # 24 x 32: a 56 x 44 degree view


def sphere_poses():
    """three cameras outside the 20^3 sphere volume (centre (10, 10, 10)), looking at the sphere from different sides"""
    return np.stack([look_at((10.0, 10.0, -12.0), (10.0, 10.0, 10.0)),
                     look_at((31.0, 16.0, 24.0), (10.0, 10.0, 10.0)),
                     look_at((-6.0, -9.0, 3.0), (10.5, 9.0, 10.0))])


def check_sphere(vertex, normal, radius=6.3):
    """per view >= 100 hits and >= 100 misses; hits within a quarter voxel of the sphere; normals within 10 degrees of radial"""
    worst_r = worst_cos = None
    for v in range(len(vertex)):
        h = hits(vertex[v])
        assert h.sum() >= 100 and (~h).sum() >= 100, (v, h.sum())
        assert np.array_equal(h, hits(normal[v]))
        p = vertex[v][h].astype(np.float64) - 10.0
        dist = np.linalg.norm(p, axis=1)
        assert np.abs(dist - radius).max() <= 0.25, np.abs(dist - radius).max()
        cosine = (normal[v][h].astype(np.float64) * p).sum(axis=1) / dist
        assert cosine.min() >= np.cos(np.radians(10.0)), cosine.min()
        worst_r = max(worst_r or 0.0, np.abs(dist - radius).max())
        worst_cos = min(worst_cos or 1.0, cosine.min())
    return worst_r, worst_cos


def wall_expected_hits(s, shape, margin=1e-3):
    """[H,W] bool, in float64: the pixels of the identity pose whose ray meets z = d strictly inside the box of voxel centres in
    x and y -- with the assertion that no ray meets it within `margin` of a face (so that f32 rounding cannot move one across)"""
    import tsdf_ref as REF
    vol = REF.Volume(s["origin"], s["vs"], s["dims"], s["tr"])
    gx, gy, gz = [c.astype(np.float64) for c in vol.centres()]
    assert gz[0] + margin < s["d"] < gz[-1] - margin
    fx, fy, cx, cy = s["K"]
    H, W = shape
    X = (np.arange(W)[None, :] - cx) / fx * s["d"] + 0 * np.arange(H)[:, None]
    Y = (np.arange(H)[:, None] - cy) / fy * s["d"] + 0 * np.arange(W)[None, :]
    for q, g in ((X, gx), (Y, gy)):
        assert (np.abs(q - g[0]) > margin).all() and (np.abs(q - g[-1]) > margin).all()
    return (X > gx[0]) & (X < gx[-1]) & (Y > gy[0]) & (Y < gy[-1])


WALL_STEP = 0.05


def wall_depth_bound(s):
    """|depth - d| of a wall hit, from f32 rounding alone; u = 2^-24, M = |o_z| + nz vs + tr bounds the z of everything touched.
    Under the identity pose C = 0 and dw = n exactly, and the stored tsdf depends on z alone bit for bit (pc.z is the voxel
    centre's z, the raster is constant), so the x and y interpolations return their operands and the tsdf is linear in z over the
    cells the bracketing samples touch (step + vs <= tr).  What remains, in metres:
      * a stored value: the centre (2 roundings <= 2 u M), sdf and the quotient (<= 2 u tr): e_T <= 4 u M;
      * where a sample is taken: p_z = t dw_z (u M) and g = (p - o) ivs - 0.5 (ivs, the difference, the product, the sum: <= 3 u
        of a grid coordinate <= nz, i.e. 3 u M): <= 4 u M; the z interpolation: 3 roundings of values <= 1: <= 3 u tr.
        So a sample is off by e_S <= 4 u M + 4 u M + 3 u tr <= 11 u M;
      * r = A / (A - B), where A - B = s n.z / tr: the error of r times the s n.z it is multiplied by is <= 3 e_S + 2 u s;
      * t* = t_(k-1) + r s and depth = t* n.z: 3 roundings of numbers <= t <= M / n.z, n.z >= 0.9 in this image.
    Sum: 33 u M + 2 u s + 3 u M / 0.9 < 40 u M.  The bound used is 64 u M."""
    oz, nz = abs(float(np.float32(s["origin"][2]))), s["dims"][2]
    return 64 * 2.0 ** -24 * (oz + nz * s["vs"] + s["tr"])


def check_wall(s, depth, vertex, normal):
    want = wall_expected_hits(s, depth.shape)
    h = hits(vertex)
    assert want.sum() > 0 and (h | ~want).all(), (want.sum(), (want & ~h).sum())      # every expected pixel is a hit
    err = np.abs(depth[want].astype(np.float64) - s["d"]).max()
    assert err <= wall_depth_bound(s), (err, wall_depth_bound(s))
    nerr = np.abs(normal[want].astype(np.float64) - np.array([0.0, 0.0, -1.0])).max()
    assert nerr <= 2.0 ** -20, nerr
    return err, nerr


def check_round_trip(s, depth, vertex):
    """on pixels that hit, |depth - input depth| <= one voxel diagonal; at least half of the pixels hit"""
    h = hits(vertex)
    assert h.mean() >= 0.5, h.mean()
    err = np.abs(depth[h].astype(np.float64) - s["depths"][h].astype(np.float64)).max()
    assert err <= np.sqrt(3.0) * s["vs"], err
    return float(h.mean()), err
