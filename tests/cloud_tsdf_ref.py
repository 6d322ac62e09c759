"""NumPy restatement of include/r3d.h "TSDF from an oriented cloud", written from the header text: brute force over all voxels and
all points, every operation on np.float32 in the written order (NumPy neither fuses a multiply with an add nor reorders), the two
fmaf of the distance as correctly rounded fused multiply-adds.  Also the geometry the tests measure the rule with: the Fibonacci
sphere and the zero crossings of a volume.  Test infrastructure: the product never imports it.
"""
import numpy as np

F32 = np.float32


def fma32(a, b, c):
    """fmaf(a, b, c) for float32 arrays, correctly rounded: the product of two f32 is exact in f64; the f64 sum is rounded TO ODD
    (its exact error comes from the two-sum), and an odd-rounded 53-bit value rounds to the 24-bit result of the exact sum."""
    p = a.astype(np.float64) * b.astype(np.float64)
    c = np.broadcast_to(c.astype(np.float64), p.shape)
    with np.errstate(all="ignore"):
        s = p + c
        bb = s - p
        err = (p - (s - bb)) + (c - bb)
        even = (s.view(np.int64) & 1) == 0
        fix = np.isfinite(s) & (err != 0) & even
        s = np.where(fix, np.nextafter(s, np.where(err > 0, np.inf, -np.inf)), s)
        return s.astype(F32)


def centres(origin, voxel_size, dims):
    """(cx [nx], cy [ny], cz [nz]) float32: c = o + ((float) idx + 0.5f) * vs"""
    o, vs = np.asarray(origin, np.float64).astype(F32), F32(voxel_size)
    return tuple(o[a] + (np.arange(dims[a]).astype(F32) + F32(0.5)) * vs for a in range(3))


def integrate_cloud(vol, origin, voxel_size, dims, sdf_trunc, xyz, normals, col=None, rgba=None, chunk=1024):
    """One cloud into vol [n_voxels,2] float32 {tsdf, weight} (linear index (z ny + y) nx + x) and, with rgba [N] uint32, into col
    [n_voxels,4] uint32 {sum_r, sum_g, sum_b, n}: new arrays and the number of voxels updated.  The inputs are not modified."""
    vol = np.array(vol, dtype=F32).reshape(-1, 2)
    col = None if col is None else np.array(col, dtype=np.uint32).reshape(-1, 4)
    p = np.ascontiguousarray(xyz, F32).reshape(-1, 3)
    nrm = np.ascontiguousarray(normals, F32).reshape(-1, 3)
    nx, ny, nz = dims
    assert vol.shape[0] == nx * ny * nz and nrm.shape == p.shape
    if p.shape[0] == 0:
        return (vol, 0) if col is None else (vol, col, 0)
    cx, cy, cz = centres(origin, voxel_size, dims)
    tr = F32(sdf_trunc)
    tr2 = tr * tr
    touched = 0
    lin = np.arange(nx * ny * nz)
    with np.errstate(all="ignore"):
        for lo in range(0, len(lin), chunk):
            i = lin[lo:lo + chunk]
            x, y, z = i % nx, (i // nx) % ny, i // (nx * ny)
            c = np.stack([cx[x], cy[y], cz[z]], axis=1)                                   # [V,3]
            dx, dy, dz = (c[:, None, a] - p[None, :, a] for a in range(3))                # [V,N]
            d2 = fma32(dz, dz, fma32(dy, dy, dx * dx))
            d2 = np.where(np.isfinite(d2), d2, F32(np.inf))                               # non-finite pairs never win
            j = np.argmin(d2, axis=1)                                                     # the lowest index among ties
            best = d2[np.arange(len(i)), j]
            n = nrm[j]
            ok = (best <= tr2) & np.isfinite(n).all(axis=1) & (n != 0).any(axis=1)
            q = p[j]
            s = ((c[:, 0] - q[:, 0]) * n[:, 0] + (c[:, 1] - q[:, 1]) * n[:, 1]) + (c[:, 2] - q[:, 2]) * n[:, 2]
            tn = np.fmax(F32(-1.0), np.fmin(F32(1.0), s / tr))                            # fminf / fmaxf: the other operand of a NaN
            t, w = vol[i, 0], vol[i, 1]
            w1 = w + F32(1.0)
            new_t = (t * w + tn) / w1
            assert new_t.dtype == F32 and tn.dtype == F32 and best.dtype == F32
            vol[i[ok], 0], vol[i[ok], 1] = new_t[ok], w1[ok]
            if col is not None:
                word = np.asarray(rgba, np.uint32)[j[ok]]
                col[i[ok], 0] += word & 0xff
                col[i[ok], 1] += (word >> 8) & 0xff
                col[i[ok], 2] += (word >> 16) & 0xff
                col[i[ok], 3] += 1
            touched += int(ok.sum())
    return (vol, touched) if col is None else (vol, col, touched)


def fibonacci_sphere(n, radius=1.0):
    """(xyz [n,3], normals [n,3]) float32: n points spread over the sphere of `radius` about 0 by the golden angle, and their true
    unit normals"""
    k = np.arange(n, dtype=np.float64) + 0.5
    z = 1.0 - 2.0 * k / n
    r = np.sqrt(1.0 - z * z)
    phi = k * (np.pi * (3.0 - np.sqrt(5.0)))
    u = np.stack([r * np.cos(phi), r * np.sin(phi), z], axis=1)
    return (u * radius).astype(F32), u.astype(F32)


def sphere_colors(normals):
    """[n,3] uint8: a colour that varies smoothly over the sphere"""
    return np.clip(np.floor((np.asarray(normals, np.float64) * 0.5 + 0.5) * 255.0 + 0.5), 0, 255).astype(np.uint8)


def zero_crossings(vol, origin, voxel_size, dims, min_weight=1.0):
    """[K,3] float64: the surface points of "TSDF volume" (one per volume edge whose two voxels are valid and differ in sign, at
    c + r vs along the edge with r = A / (A - B)), in float64 from the volume's float32 values"""
    nx, ny, nz = dims
    t = np.asarray(vol, F32).reshape(nz, ny, nx, 2)
    T, W = t[..., 0].astype(np.float64), t[..., 1]
    cx, cy, cz = (a.astype(np.float64) for a in centres(origin, voxel_size, dims))
    C = np.stack(np.broadcast_arrays(cx[None, None, :], cy[None, :, None], cz[:, None, None]), axis=-1)   # [nz,ny,nx,3]
    out = []
    for a, axis in enumerate((2, 1, 0)):                                                                  # x, y, z edges
        sl0 = [slice(None)] * 3
        sl1 = [slice(None)] * 3
        sl0[axis], sl1[axis] = slice(0, -1), slice(1, None)
        sl0, sl1 = tuple(sl0), tuple(sl1)
        A, B = T[sl0], T[sl1]
        m = (W[sl0] >= min_weight) & (W[sl1] >= min_weight) & ((A < 0) != (B < 0))
        pts = C[sl0][m].copy()
        pts[:, a] += (A[m] / (A[m] - B[m])) * float(F32(voxel_size))
        out.append(pts)
    return np.concatenate(out, axis=0)


def cells_crossing_sphere(origin, voxel_size, dims, radius=1.0):
    """[M,3] integer (x, y, z) of the cells (corner 0 = that voxel) whose eight corners are not all on one side of the sphere of
    `radius` about 0"""
    cx, cy, cz = (a.astype(np.float64) for a in centres(origin, voxel_size, dims))
    d = np.sqrt(cx[None, None, :] ** 2 + cy[None, :, None] ** 2 + cz[:, None, None] ** 2) - radius        # [nz,ny,nx]
    inside = d < 0
    corners = [inside[dz:dims[2] - 1 + dz, dy:dims[1] - 1 + dy, dx:dims[0] - 1 + dx] for dz in (0, 1) for dy in (0, 1) for dx in (0, 1)]
    n_in = np.sum(corners, axis=0)
    z, y, x = np.nonzero((n_in > 0) & (n_in < 8))
    return np.stack([x, y, z], axis=1)


def cells_with_invalid_corner(vol, dims, cells, min_weight=1.0):
    """how many of `cells` have a corner voxel with weight < min_weight"""
    nx, ny, nz = dims
    W = np.asarray(vol, F32).reshape(nz, ny, nx, 2)[..., 1]
    bad = np.zeros(len(cells), bool)
    for dz in (0, 1):
        for dy in (0, 1):
            for dx in (0, 1):
                bad |= W[cells[:, 2] + dz, cells[:, 1] + dy, cells[:, 0] + dx] < min_weight
    return int(bad.sum())


def sphere_case(n=1000, dim=24, voxel_size=0.1, trunc_voxels=4):
    """the quality case: (origin, voxel_size, dims, sdf_trunc, xyz, normals) of the Fibonacci sphere of radius 1 centred in a
    dim^3 volume"""
    xyz, normals = fibonacci_sphere(n)
    origin = np.full(3, -0.5 * dim * voxel_size)
    return origin, voxel_size, (dim, dim, dim), trunc_voxels * voxel_size, xyz, normals
