"""NumPy restatement of the TSDF volume's colour rules (include/r3d.h, "TSDF colour") on top of tests/tsdf_ref.py: the colour plane
holds uint32 sums {sum_r, sum_g, sum_b, n} per voxel, a frame adds the bytes of the pixel the depth rule read, and a surface point
takes the two voxels' mean colours interpolated like its position -- f32 throughout, in the written order.  The acceptance mask
per frame is restated here (tsdf_ref.integrate does not return it); integrate() asserts that the tsdf / weight it produces on the
way are tsdf_ref's, bit for bit.  Test infrastructure only."""
import numpy as np

import tsdf_ref as REF

F = np.float32


class ColorVolume(REF.Volume):
    def __init__(self, origin, voxel_size, dims, sdf_trunc):
        super().__init__(origin, voxel_size, dims, sdf_trunc)
        self.sums = np.zeros((self.nz, self.ny, self.nx, 3), np.uint32)
        self.n = np.zeros((self.nz, self.ny, self.nx), np.uint32)


def integrate(vol, depths, rgb, poses_w2c, intrinsics, depth_scale=1.0):
    """depths [F,H,W], rgb [F,H,W,3] uint8, poses_w2c [F,12]: tsdf_ref.integrate plus the colour sums.  Returns the number of
    (voxel, frame) pairs that passed every test."""
    depths, rgb = np.asarray(depths), np.asarray(rgb)
    n_frames, H, W = depths.shape
    assert rgb.shape == (n_frames, H, W, 3) and rgb.dtype == np.uint8
    check = REF.Volume(vol.o, vol.vs, (vol.nx, vol.ny, vol.nz), vol.tr)
    check.tsdf, check.w = vol.tsdf.copy(), vol.w.copy()
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
            vol.tsdf = np.where(ok, new, vol.tsdf)
            vol.w = np.where(ok, w1, vol.w)
            vol.sums = vol.sums + np.where(ok[..., None], rgb[f][row, col].astype(np.uint32), np.uint32(0))   # uint32: wraps
            vol.n = vol.n + ok.astype(np.uint32)
            passed += int(ok.sum())
    assert vol.sums.dtype == np.uint32 and vol.n.dtype == np.uint32
    assert REF.integrate(check, depths, poses_w2c, intrinsics, depth_scale) == passed
    assert np.array_equal(vol.tsdf.view(np.uint32), check.tsdf.view(np.uint32)) and np.array_equal(vol.w, check.w)
    return passed


def _mean(s, n):
    """(float) sum / (float) n per channel, 0 where n == 0"""
    with np.errstate(all="ignore"):
        return np.where((n > 0)[:, None], s.astype(F) / n.astype(F)[:, None], F(0.0)).astype(F)


def extract_colors(vol, min_weight=1.0):
    """[n,3] uint8: the colour of every row of tsdf_ref.extract(vol, min_weight), in its order."""
    mw = F(min_weight)
    assert mw > 0
    T, valid = vol.tsdf, vol.w >= mw
    false = np.zeros_like(valid)
    AX = (2, 1, 0)
    cross, r_of = [], []
    with np.errstate(all="ignore"):
        for a in range(3):
            B = REF._shift(T, AX[a], 1, T)
            nvalid = REF._shift(valid, AX[a], 1, false)
            cross.append(valid & nvalid & ((T < 0) != (B < 0)))
            r_of.append(T / (T - B))
        vox, axis = np.nonzero(np.stack(cross, axis=-1).reshape(-1, 3))   # voxel-major, then axis: the points' order
        r = np.stack(r_of, axis=-1).reshape(-1, 3)[vox, axis].astype(F)
        # these are tsdf_ref's rows: same count, and the moved coordinate of every position is centre + r * vs
        xyz, _ = REF.extract(vol, min_weight)
        assert len(xyz) == len(vox)
        z, rem = np.divmod(vox, vol.ny * vol.nx)
        y, x = np.divmod(rem, vol.nx)
        c = np.stack([vol.centres()[0][x], vol.centres()[1][y], vol.centres()[2][z]], axis=1).astype(F)
        k = np.arange(len(vox))
        assert np.array_equal((c[k, axis] + r * vol.vs).view(np.uint32), np.ascontiguousarray(xyz[k, axis]).view(np.uint32))
        step = np.array([1, vol.nx, vol.nx * vol.ny])[axis]
        S, N = vol.sums.reshape(-1, 3), vol.n.reshape(-1)
        mv, mu = _mean(S[vox], N[vox]), _mean(S[vox + step], N[vox + step])
        m = mv + r[:, None] * (mu - mv)
        q = np.minimum(np.maximum(np.floor(m + F(0.5)), F(0.0)), F(255.0))
        assert m.dtype == F and q.dtype == F
    return q.astype(np.uint8).reshape(-1, 3)


def pack(rgb):
    """the words r | g << 8 | b << 16 of [n,3] uint8 rows"""
    c = np.asarray(rgb).astype(np.uint32).reshape(-1, 3)
    return c[:, 0] | c[:, 1] << np.uint32(8) | c[:, 2] << np.uint32(16)


def random_colors(s, seed=0):
    """[F,H,W,3] uint8 noise for the scene dict s (tsdf_ref's scenes stay as they are)"""
    rng = np.random.default_rng([seed, 77] + list(s["depths"].shape))
    return rng.integers(0, 256, s["depths"].shape + (3,), dtype=np.uint8)


def uniform_colors(s, colors):
    """frame f entirely of colors[f]"""
    c = np.asarray(colors, dtype=np.uint8).reshape(-1, 1, 1, 3)
    assert len(c) == s["depths"].shape[0]
    return np.ascontiguousarray(np.broadcast_to(c, s["depths"].shape + (3,)))


def repeated(s, n_frames):
    """the one-frame scene s seen n_frames times"""
    out = dict(s)
    out["depths"] = np.repeat(s["depths"], n_frames, axis=0)
    out["poses"] = np.repeat(np.asarray(s["poses"]), n_frames, axis=0)
    return out


def run(s, rgb, min_weight=1.0):
    """The reference on a scene dict and its colour images: (ColorVolume, passed, colours [n,3] uint8)."""
    vol = ColorVolume(s["origin"], s["vs"], s["dims"], s["tr"])
    passed = integrate(vol, s["depths"], rgb, s["poses"], s["K"], s["scale"])
    return vol, passed, extract_colors(vol, min_weight)
