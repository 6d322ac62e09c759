"""NumPy restatement of the TSDF volume's specification (include/r3d.h, "TSDF volume"): every operation on np.float32 arrays in the
written order, frames applied in a Python loop, all voxels of the volume at once.  x86 f32 addition, multiplication, division,
floor and sqrt are IEEE, so this file defines every bit the device must produce.  Test infrastructure only."""
import numpy as np

F = np.float32


class Volume:
    def __init__(self, origin, voxel_size, dims, sdf_trunc):
        self.o = np.asarray(origin, dtype=np.float64).astype(F)
        self.vs, self.tr = F(voxel_size), F(sdf_trunc)
        self.nx, self.ny, self.nz = [int(d) for d in dims]
        self.tsdf = np.zeros((self.nz, self.ny, self.nx), F)
        self.w = np.zeros((self.nz, self.ny, self.nx), F)

    def centres(self):
        """(cx [nx], cy [ny], cz [nz]) f32: c = o + ((float) idx + 0.5f) * vs"""
        return tuple(self.o[a] + (np.arange(n).astype(F) + F(0.5)) * self.vs for a, n in enumerate((self.nx, self.ny, self.nz)))

    def copy(self):
        v = Volume(self.o, self.vs, (self.nx, self.ny, self.nz), self.tr)
        v.tsdf, v.w = self.tsdf.copy(), self.w.copy()
        return v


def integrate(vol, depths, poses_w2c, intrinsics, depth_scale=1.0):
    """depths [F,H,W] (u8 / u16 / f32), poses_w2c [F,12] float64 (R row-major, t), intrinsics (fx, fy, cx, cy).  Returns the
    number of (voxel, frame) pairs that passed every test."""
    depths = np.asarray(depths)
    n_frames, H, W = depths.shape
    poses = np.asarray(poses_w2c, dtype=np.float64).reshape(n_frames, 12).astype(F)
    fx, fy, cx, cy = [F(v) for v in intrinsics]
    scale = F(depth_scale)
    gx, gy, gz = vol.centres()
    X, Y, Z = gx[None, None, :], gy[None, :, None], gz[:, None, None]
    passed = 0
    with np.errstate(all="ignore"):
        for f in range(n_frames):
            R, t = poses[f, :9], poses[f, 9:]
            pc = [((R[3 * k] * X + R[3 * k + 1] * Y) + R[3 * k + 2] * Z) + t[k] for k in range(3)]
            ok = pc[2] > 0
            u = fx * (pc[0] / pc[2]) + cx
            v = fy * (pc[1] / pc[2]) + cy
            ui, vi = np.floor(u + F(0.5)), np.floor(v + F(0.5))
            ok &= (ui >= 0) & (ui < F(W)) & (vi >= 0) & (vi < F(H))
            col = np.where(ok, ui, 0).astype(np.int64)
            row = np.where(ok, vi, 0).astype(np.int64)
            d = depths[f][row, col].astype(F) * scale
            ok &= (d > 0) & np.isfinite(d)
            sdf = d - pc[2]
            ok &= ~(sdf < -vol.tr)
            tn = np.minimum(F(1.0), sdf / vol.tr)
            w1 = vol.w + F(1.0)
            new = (vol.tsdf * vol.w + tn) / w1
            assert new.dtype == F and w1.dtype == F and tn.dtype == F and d.dtype == F
            vol.tsdf = np.where(ok, new, vol.tsdf)
            vol.w = np.where(ok, w1, vol.w)
            passed += int(ok.sum())
    return passed


def _shift(a, axis, step, fill):
    """b[q] = a[q + step e_axis] where that voxel exists, else fill[q]"""
    out = fill.copy()
    src = [slice(None)] * 3
    dst = [slice(None)] * 3
    if step > 0:
        src[axis], dst[axis] = slice(step, None), slice(None, -step)
    else:
        src[axis], dst[axis] = slice(None, step), slice(-step, None)
    out[tuple(dst)] = a[tuple(src)]
    return out


def extract(vol, min_weight=1.0, squares=None):
    """(xyz [n,3], normals [n,3]) f32 in the specified order: linear voxel order, per voxel the axes x, y, z.  squares: an optional
    hook (terms [3], total) -> total on the normal's squared length, for tests that look at it or flush its subnormals."""
    mw = F(min_weight)
    assert mw > 0
    T, valid = vol.tsdf, vol.w >= mw
    false = np.zeros_like(valid)
    AX = (2, 1, 0)                          # array axis of the volume axes x, y, z
    cross, r_of, grad = [], [], []
    with np.errstate(all="ignore"):
        for a in range(3):
            B = _shift(T, AX[a], 1, T)
            nvalid = _shift(valid, AX[a], 1, false)          # outside the volume: no neighbour
            cross.append(valid & nvalid & ((T < 0) != (B < 0)))
            r_of.append(T / (T - B))
            hi = np.where(_shift(valid, AX[a], 1, false), _shift(T, AX[a], 1, T), T)
            lo = np.where(_shift(valid, AX[a], -1, false), _shift(T, AX[a], -1, T), T)
            grad.append(hi - lo)
        sel = np.stack(cross, axis=-1).reshape(-1, 3)        # [voxel][axis]
        vox, axis = np.nonzero(sel)                          # row-major: voxel-major, then axis
        gx, gy, gz = vol.centres()
        z, rem = np.divmod(vox, vol.ny * vol.nx)
        y, x = np.divmod(rem, vol.nx)
        pos = np.stack([gx[x], gy[y], gz[z]], axis=1).astype(F)
        r = np.stack(r_of, axis=-1).reshape(-1, 3)[vox, axis].astype(F)
        pos[np.arange(len(vox)), axis] = pos[np.arange(len(vox)), axis] + r * vol.vs
        step = np.array([1, vol.nx, vol.nx * vol.ny])[axis]
        G = np.stack([g.reshape(-1) for g in grad], axis=1)  # [voxel][b]
        gv, gn = G[vox], G[vox + step]
        m = gv + r[:, None] * (gn - gv)
        sq = [m[:, b] * m[:, b] for b in range(3)]
        total = (sq[0] + sq[1]) + sq[2]
        if squares is not None:                              # a test's view of (or hand on) the squared length and its terms
            total = squares(sq, total)
        ln = np.sqrt(total)
        assert m.dtype == F and ln.dtype == F and pos.dtype == F
        nrm = np.where((ln > 0)[:, None], m / ln[:, None], F(0.0)).astype(F)
    return pos, nrm


# ---- scenes shared by tests/test_tsdf_host.py (conditions asserted of this reference first) and tests/test_gpu_tsdf.py ----------
def identity_poses(n):
    p = np.zeros((n, 12))
    p[:, 0] = p[:, 4] = p[:, 8] = 1.0
    return p


WALL_K = (40.0, 40.0, 15.5, 11.5)      # 24 x 32 raster: at z = 2 the image spans |x| < 0.8, |y| < 0.6


def wall_scene(wide=False, dtype=np.float32):
    """A constant-depth raster seen through the identity pose and a volume straddling z = d.  wide: the volume sticks out of the
    frustum on both sides in x.  Returns dict(origin, vs, dims, tr, depths, poses, K, scale, d)."""
    if np.dtype(dtype) == np.float32:
        d, scale = 2.03, 1.0
        depths = np.full((1, 24, 32), d, np.float32)
        d = float(np.float32(d))
    else:
        d, scale = 2.0, 0.125
        depths = np.full((1, 24, 32), 16, dtype)
    origin = (-1.2, -0.3, 1.8) if wide else (-0.4, -0.3, 1.8)
    dims = (48, 12, 8) if wide else (16, 12, 8)
    return dict(origin=origin, vs=0.05, dims=dims, tr=0.15, depths=depths, poses=identity_poses(1), K=WALL_K, scale=scale, d=d)


def wall_expected_columns(s):
    """Columns (x, y) whose two voxels around z = d both project into the image -- in float64, with the assertion that no voxel of
    those layers is within 1e-3 pixel of the image border (so that f32 rounding cannot move one across)."""
    vol = Volume(s["origin"], s["vs"], s["dims"], s["tr"])
    gx, gy, gz = [c.astype(np.float64) for c in vol.centres()]
    k = int(np.searchsorted(gz, s["d"], side="right")) - 1
    assert 0 <= k < len(gz) - 1 and gz[k] <= s["d"] < gz[k + 1]
    fx, fy, cx, cy = s["K"]
    H, W = s["depths"].shape[1:]
    inside = np.ones((len(gy), len(gx)), bool)
    for z in (gz[k], gz[k + 1]):
        u = fx * gx[None, :] / z + cx + 0.5
        v = fy * gy[:, None] / z + cy + 0.5
        for q, n in ((u, W), (v, H)):
            assert (np.abs(q - 0) > 1e-3).all() and (np.abs(q - n) > 1e-3).all()
        inside &= (np.floor(u) >= 0) & (np.floor(u) < W) & (np.floor(v) >= 0) & (np.floor(v) < H)
    return int(inside.sum())


def check_wall(s, xyz, nrm):
    """The issue's conditions on the fronto-parallel wall."""
    oz, nz = abs(float(np.float32(s["origin"][2]))), s["dims"][2]
    bound = 16 * 2.0 ** -24 * (oz + nz * s["vs"] + s["tr"])
    assert len(xyz) == wall_expected_columns(s) and len(xyz) > 0
    assert np.abs(xyz[:, 2].astype(np.float64) - s["d"]).max() <= bound
    assert np.abs(nrm.astype(np.float64) - np.array([0.0, 0.0, -1.0])).max() <= 2.0 ** -22


def room_scene():
    """synthetic.room_views(8, 96, 128) and a 0.2 m grid around the room (0.3 m margin, truncation 0.6 m)."""
    import importlib
    from helpers import PKG
    syn = importlib.import_module(PKG + ".synthetic")
    depth, q, t, K = syn.room_views(8, 96, 128, seed=0)
    vs, margin = 0.2, 0.3
    lo, hi = syn.ROOM_LO - margin, syn.ROOM_HI + margin
    dims = tuple(int(np.ceil((hi[a] - lo[a]) / vs - 1e-9)) for a in range(3))
    return dict(origin=tuple(lo), vs=vs, dims=dims, tr=0.6, depths=depth, quats=q, ts=t, K=K, scale=1.0, lo=syn.ROOM_LO, hi=syn.ROOM_HI)


def check_room(s, xyz):
    """Every point within one voxel diagonal of the room's faces."""
    p = xyz.astype(np.float64)
    lo, hi = np.asarray(s["lo"]), np.asarray(s["hi"])
    outside = np.linalg.norm(np.maximum(np.maximum(lo - p, p - hi), 0.0), axis=1)
    inside = np.minimum(p - lo, hi - p).min(axis=1)
    dist = np.where(outside > 0, outside, inside)
    assert len(p) > 1000 and dist.max() <= np.sqrt(3.0) * s["vs"], (len(p), dist.max())


BOUNDARY_K = (8.0, 8.0, 3.5, 2.5)


def boundary_scene():
    """Voxel centres on the 1/8 lattice, z = 1 and 1.125, identity pose, fx = fy = 8: at z = 1 the voxel x = -0.5 projects to
    u + 0.5 = 0 exactly (inside) and x = 3.5 to u + 0.5 = 32 = W exactly (outside); likewise y = -0.375 and y = 2.625 for H = 24."""
    depths = np.full((1, 24, 32), 1.5, np.float32)
    return dict(origin=(-1.0625, -0.5625, 0.9375), vs=0.125, dims=(48, 30, 2), tr=1.0, depths=depths, poses=identity_poses(1),
                K=BOUNDARY_K, scale=1.0)


def rot_y(a):
    return np.array([[np.cos(a), 0, np.sin(a)], [0, 1, 0], [-np.sin(a), 0, np.cos(a)]])


def rot_x(a):
    return np.array([[1, 0, 0], [0, np.cos(a), -np.sin(a)], [0, np.sin(a), np.cos(a)]])


def random_scene(dims, n_frames, dtype, hw, seed, offset=0.0, unseen=False):
    """A volume of 0.05 m voxels around (offset, 0, 2) and n_frames cameras scattered around it: some see it whole, some see a
    part, some have part of it (or all of it: unseen) behind them.  Rasters: a coarse random pattern of depths around the camera-volume
    distances, so that the signs alternate and crossings abound; f32 rasters carry 0, NaN, +-inf and negative pixels, integer
    ones zeros.  No denormal arises: depths are 0 or >= 2^-10 in magnitude, sdf is a difference of such numbers and voxel
    coordinates of magnitude >= 2^-6 ulp-spaced, products and quotients stay far above 2^-126."""
    rng = np.random.default_rng([seed, n_frames, hw[0]] + list(dims))
    H, W = hw
    vs, tr = 0.05, 0.12
    ext = np.array(dims) * vs
    centre = np.array([offset, 0.0, 2.0])
    origin = centre - ext / 2
    K = (1.25 * W, 1.25 * W, (W - 1) / 2.0, (H - 1) / 2.0)
    poses = np.zeros((n_frames, 12))
    dist = np.zeros(n_frames)
    for f in range(n_frames):
        c = centre + rng.uniform(-1, 1, 3) * np.array([ext[0] / 2 + 0.5, 0.3, 0.2]) - np.array([0, 0, rng.uniform(0.0, 2.0)])
        aim = np.arctan2(centre[0] - c[0], centre[2] - c[2])            # towards the volume's centre, give or take
        yaw = aim + rng.uniform(-0.3, 0.3) + (np.pi if (unseen or f % 7 == 5) else 0.0)
        Rwc = rot_y(yaw) @ rot_x(rng.uniform(-0.2, 0.2))
        R = Rwc.T
        poses[f, :9], poses[f, 9:] = R.reshape(9), -R @ c
        dist[f] = max(0.3, centre[2] - c[2])
    coarse = rng.uniform(-0.3, 0.3, (n_frames, (H + 3) // 4, (W + 3) // 4))
    metric = dist[:, None, None] + np.repeat(np.repeat(coarse, 4, axis=1), 4, axis=2)[:, :H, :W]
    holes = rng.random((n_frames, H, W))
    if np.dtype(dtype) == np.float32:
        depths, scale = metric.astype(np.float32), 1.0
        for k, bad in enumerate((0.0, np.nan, np.inf, -np.inf, -1.5)):
            depths[(holes >= 0.02 * k) & (holes < 0.02 * (k + 1))] = bad
    elif np.dtype(dtype) == np.uint16:
        depths, scale = np.clip(np.round(metric * 1000), 1, 65535).astype(np.uint16), 0.001
        depths[holes < 0.05] = 0
    else:
        depths, scale = np.clip(np.round(metric * 32), 1, 255).astype(np.uint8), 1.0 / 32
        depths[holes < 0.05] = 0
    return dict(origin=tuple(origin), vs=vs, dims=tuple(dims), tr=tr, depths=depths, poses=poses, K=K, scale=scale)


def run(s, min_weight=1.0):
    """The reference on a scene dict: (Volume, passed, xyz, normals)."""
    vol = Volume(s["origin"], s["vs"], s["dims"], s["tr"])
    poses = s["poses"] if "poses" in s else poses_w2c(s["quats"], s["ts"])
    passed = integrate(vol, s["depths"], poses, s["K"], s["scale"])
    xyz, nrm = extract(vol, min_weight)
    return vol, passed, xyz, nrm


def poses_w2c(quats, ts):
    """The package's poses_w2c (the pose file's rotation and t as they stand)."""
    import importlib
    from helpers import PKG
    return importlib.import_module(PKG + ".tsdf").poses_w2c(quats, ts)
