"""NumPy restatement of the ray-cast colour rule (include/r3d.h, "TSDF ray-cast colour") on top of tests/raycast_ref.py and
tests/tsdf_color_ref.py: the geometry of a view is raycast_ref.cast_view's, and the colour of a hit is the trilinear value of
the hit cell's eight mean colours at the hit-point sample's fractions -- f32 throughout, in the written order.  cast_view does
not return that cell and those fractions, so they are recomputed here from the hit point as the header's "Sample at t" writes
them: the vertex row of a hit IS the point p(t*) the sample was taken at, bit for bit (the same expression C_a + t* dw_a), and
hit_cell asserts that raycast_ref's own sample of it is valid with the same fractions.  Reads tsdf_color_ref.ColorVolume.
Test infrastructure only."""
import numpy as np

import raycast_ref as RC

F = np.float32


def hit_cell(vol, p):
    """p: three f32 arrays, the hit points.  ((ix, iy, iz) int64 arrays, (fx, fy, fz) f32 arrays): the cell and the fractions"""
    ivs = F(1.0) / vol.vs
    g = [(p[a] - vol.o[a]) * ivs - F(0.5) for a in range(3)]
    i = [np.floor(q) for q in g]
    f = [g[a] - i[a] for a in range(3)]
    assert all(q.dtype == F for q in g + i + f) and ivs.dtype == F
    return [q.astype(np.int64) for q in i], f


def cell_colors(sums, n, idx, f):
    """sums [nz,ny,nx,3] uint32, n [nz,ny,nx] uint32; idx, f from hit_cell.  [P,3] uint8: per channel the eight corners' means
    M_k = (float) sum_k / (float) n_k (0 where n_k == 0), interpolated x first, then y, then z, rounded half up and clamped."""
    M = []
    with np.errstate(all="ignore"):
        for k in range(8):
            x, y, z = idx[0] + (k & 1), idx[1] + ((k >> 1) & 1), idx[2] + (k >> 2)
            s, c = sums[z, y, x], n[z, y, x]
            assert s.dtype == np.uint32 and c.dtype == np.uint32
            M.append(np.where((c > 0)[:, None], s.astype(F) / c.astype(F)[:, None], F(0.0)).astype(F))
    fx, fy, fz = [np.asarray(q, dtype=F)[:, None] for q in f]
    c00, c10 = M[0] + fx * (M[1] - M[0]), M[2] + fx * (M[3] - M[2])          # c[jy][jz]
    c01, c11 = M[4] + fx * (M[5] - M[4]), M[6] + fx * (M[7] - M[6])
    b0, b1 = c00 + fy * (c10 - c00), c01 + fy * (c11 - c01)
    m = b0 + fz * (b1 - b0)
    q = np.fmin(np.fmax(np.floor(m + F(0.5)), F(0.0)), F(255.0))             # fmaxf / fminf
    assert m.dtype == F and q.dtype == F
    return q.astype(np.uint8)


def cast_view(vol, pose_row, intrinsics, shape, min_weight=1.0, step=None, t_near=0.0, t_far=np.inf):
    """One view of a ColorVolume: raycast_ref.cast_view's (depth, vertex, normal) + rgb [H,W,3] uint8 + hit [H,W] bool."""
    depth, vertex, normal, hit = RC.cast_view(vol, pose_row, intrinsics, shape, min_weight, step, t_near, t_far)
    rgb = np.zeros(tuple(shape) + (3,), np.uint8)                            # a miss is 0, 0, 0
    if hit.any():
        p = [np.ascontiguousarray(vertex[..., a][hit]) for a in range(3)]
        idx, f = hit_cell(vol, p)
        ok, _, f_rc = RC._sample(vol, F(min_weight), p)                      # the sample the normal was computed from
        assert ok.all() and all(np.array_equal(f[a].view(np.uint32), f_rc[a].view(np.uint32)) for a in range(3))
        rgb[hit] = cell_colors(vol.sums, vol.n, idx, f)
    return depth, vertex, normal, rgb, hit


def raycast(vol, poses_w2c, intrinsics, shape, min_weight=1.0, step=None, t_near=0.0, t_far=np.inf):
    """(depth [V,H,W], vertex [V,H,W,3], normal [V,H,W,3]) f32 and rgb [V,H,W,3] uint8 for poses_w2c [V,12] float64."""
    poses = np.asarray(poses_w2c, dtype=np.float64).reshape(-1, 12)
    H, W = shape
    out = [cast_view(vol, p, intrinsics, shape, min_weight, step, t_near, t_far)[:4] for p in poses]
    if not out:
        return np.zeros((0, H, W), F), np.zeros((0, H, W, 3), F), np.zeros((0, H, W, 3), F), np.zeros((0, H, W, 3), np.uint8)
    return tuple(np.stack([o[j] for o in out]) for j in range(4))
