"""NumPy / Python restatement of the TSDF mesh's specification (include/r3d.h, "TSDF mesh"): marching cubes whose vertices are
tsdf_ref.extract's rows and whose triangles index them.  The loop tracing per case is written here from the specification's text,
geometrically (faces as point sets, their corner cycles ordered by the outward normal), and does NOT import the generated table
csrc/r3d_mc_table.h or its generator: tests/test_mesh_host.py compares the two.  Test infrastructure only."""
import functools
import itertools

import numpy as np

import tsdf_ref as REF

F = np.float32
CORNERS = [np.array([k & 1, (k >> 1) & 1, k >> 2]) for k in range(8)]        # corner k = dx + 2 dy + 4 dz


def edge_id(p, q):
    """the cell edge e = 4 a + u + 2 v between corner points p and q"""
    diff = np.nonzero(p != q)[0]
    assert len(diff) == 1
    a = int(diff[0])
    lo = np.minimum(p, q)
    u, v = [int(lo[b]) for b in range(3) if b != a]
    return 4 * a + u + 2 * v


def edge_corners(e):
    """(lower corner k, upper corner k, axis) of cell edge e"""
    a, j = divmod(e, 4)
    d = np.zeros(3, int)
    d[[b for b in range(3) if b != a]] = (j & 1, j >> 1)
    hi = d.copy()
    hi[a] = 1
    return int(d @ (1, 2, 4)), int(hi @ (1, 2, 4)), a


@functools.lru_cache(None)
def face_cycles():
    """The 6 faces' corners, counter-clockwise as seen from outside the cell: sorted by their angle around the outward normal."""
    out = []
    for axis, side in itertools.product(range(3), (0, 1)):
        normal = np.zeros(3)
        normal[axis] = 1.0 if side else -1.0
        ks = [k for k in range(8) if CORNERS[k][axis] == side]
        mid = np.mean([CORNERS[k] for k in ks], axis=0)
        # a right-handed frame (t1, t2, normal): counter-clockwise seen from where the normal points to is the order of atan2(t2, t1)
        t1 = np.zeros(3)
        t1[(axis + 1) % 3] = 1.0
        t2 = np.cross(normal, t1)
        ang = [np.arctan2((CORNERS[k] - mid) @ t2, (CORNERS[k] - mid) @ t1) for k in ks]
        out.append(tuple(k for _, k in sorted(zip(ang, ks))))
    return tuple(out)


def case_segments(m):
    """directed segments (from edge, to edge) of case m"""
    segs = []
    for cyc in face_cycles():
        neg = [bool((m >> k) & 1) for k in cyc]
        for s in range(4):
            if neg[s] and not neg[s - 1]:                    # a run of negative corners starts at position s
                stop = s
                while neg[(stop + 1) % 4]:
                    stop += 1
                enter = edge_id(CORNERS[cyc[s - 1]], CORNERS[cyc[s]])
                leave = edge_id(CORNERS[cyc[stop % 4]], CORNERS[cyc[(stop + 1) % 4]])
                segs.append((enter, leave))
    return segs


@functools.lru_cache(None)
def case_loops(m):
    nxt = dict(case_segments(m))
    assert len(nxt) == len(case_segments(m)) and sorted(nxt) == sorted(nxt.values())
    loops, todo = [], sorted(nxt)
    while todo:
        start = todo[0]
        loop = [start]
        while nxt[loop[-1]] != start:
            loop.append(nxt[loop[-1]])
        todo = [e for e in todo if e not in loop]
        loops.append(tuple(loop))
    return tuple(loops)


@functools.lru_cache(None)
def case_triangles(m):
    return tuple((l[0], l[i], l[i + 1]) for l in case_loops(m) for i in range(1, len(l) - 1))


def crossing_edges(m):
    return sorted(e for e in range(12) if ((m >> edge_corners(e)[0]) ^ (m >> edge_corners(e)[1])) & 1)


def vertex_ids(vol, min_weight=1.0):
    """[n_voxels * 3] int64: the rank of volume edge (voxel, axis) in tsdf_ref.extract's order, -1 where it carries no point"""
    mw = F(min_weight)
    T, valid = vol.tsdf, vol.w >= mw
    false = np.zeros_like(valid)
    cross = []
    for a, ax in enumerate((2, 1, 0)):
        B = REF._shift(T, ax, 1, T)
        cross.append(valid & REF._shift(valid, ax, 1, false) & ((T < 0) != (B < 0)))
    sel = np.stack(cross, axis=-1).reshape(-1)
    ids = np.cumsum(sel) - 1
    ids[~sel] = -1
    return ids


def extract_mesh(vol, min_weight=1.0, with_cells=False):
    """(xyz [N,3] f32, normals [N,3] f32, triangles [M,3] int32) in the specified order (+ the linear voxel index of every
    triangle's cell with with_cells)."""
    xyz, nrm = REF.extract(vol, min_weight)
    ids = vertex_ids(vol, min_weight)
    assert (ids >= 0).sum() == len(xyz)
    nx, ny, nz = vol.nx, vol.ny, vol.nz
    tris, cells = [], []
    if min(nx, ny, nz) >= 2:
        valid = vol.w >= F(min_weight)
        neg = vol.tsdf < 0
        active = np.ones((nz - 1, ny - 1, nx - 1), bool)
        case = np.zeros((nz - 1, ny - 1, nx - 1), np.int64)
        for k in range(8):
            dx, dy, dz = CORNERS[k]
            sl = (slice(dz, nz - 1 + dz), slice(dy, ny - 1 + dy), slice(dx, nx - 1 + dx))
            active &= valid[sl]
            case |= neg[sl].astype(np.int64) << k
        step = (1, nx, nx * ny)
        for z, y, x in zip(*np.nonzero(active)):             # row-major over (z, y, x): linear voxel order
            i = (z * ny + y) * nx + x
            for t in case_triangles(int(case[z, y, x])):
                row = []
                for e in t:
                    lo, _, a = edge_corners(e)
                    owner = i + int(CORNERS[lo] @ step)
                    row.append(ids[3 * owner + a])
                tris.append(row)
                cells.append(i)
    tri = np.asarray(tris, dtype=np.int64).reshape(-1, 3)
    assert (tri >= 0).all()                                  # every index a triangle names exists
    tri = tri.astype(np.int32)
    return (xyz, nrm, tri, np.asarray(cells, dtype=np.int64)) if with_cells else (xyz, nrm, tri)


# ---- shapes and checks shared by tests/test_mesh_host.py (asserted of this reference first) and tests/test_gpu_mesh.py ----------
SPHERE_R = 6.3


def sphere_volume():
    """20^3 voxels of size 1 around a sphere of radius 6.3 voxels centred on the volume, written straight into the arrays: tsdf =
    distance from the centre - radius (negative inside), all weights 1."""
    vol = REF.Volume((0.0, 0.0, 0.0), 1.0, (20, 20, 20), 3.0)
    gx, gy, gz = [c.astype(np.float64) for c in vol.centres()]
    d = np.sqrt((gx[None, None, :] - 10.0) ** 2 + (gy[None, :, None] - 10.0) ** 2 + (gz[:, None, None] - 10.0) ** 2)
    vol.tsdf = (d - SPHERE_R).astype(F)
    vol.w = np.ones_like(vol.tsdf)
    return vol


def directed_edges(tri):
    t = np.asarray(tri, dtype=np.int64)
    return np.concatenate([t[:, [0, 1]], t[:, [1, 2]], t[:, [2, 0]]])


def check_closed_genus0(n_vertices, tri):
    """every directed edge occurs once and its reverse once; V - E + F = 2; no vertex is unused"""
    e = directed_edges(tri)
    key = e[:, 0] * n_vertices + e[:, 1]
    rev = e[:, 1] * n_vertices + e[:, 0]
    assert len(np.unique(key)) == len(key)
    assert np.array_equal(np.sort(key), np.sort(rev))
    assert n_vertices - len(key) // 2 + len(tri) == 2
    assert np.array_equal(np.unique(tri), np.arange(n_vertices))


def check_sphere(xyz, tri):
    check_closed_genus0(len(xyz), tri)
    p = xyz.astype(np.float64) - 10.0
    a, b, c = p[tri[:, 0]], p[tri[:, 1]], p[tri[:, 2]]
    volume = (a * np.cross(b, c)).sum() / 6.0
    exact = 4.0 / 3.0 * np.pi * SPHERE_R ** 3
    assert volume > 0 and abs(volume - exact) <= 0.03 * exact, (volume, exact)
    n = np.cross(b - a, c - a)
    mid = (a + b + c) / 3.0
    cosine = (n * mid).sum(axis=1) / (np.linalg.norm(n, axis=1) * np.linalg.norm(mid, axis=1))
    assert cosine.min() >= np.cos(np.radians(10.0)), cosine.min()
    return volume, cosine.min()


def check_wall_mesh(s, xyz, tri):
    """the wall's triangles: every unit normal (0, 0, -1) to the wall check's tolerance (the wall's vertices share one z bit for
    bit -- tsdf depends on z alone under the identity pose -- so the normals are exact), two per cell of the covered columns"""
    p = xyz.astype(np.float64)
    n = np.cross(p[tri[:, 1]] - p[tri[:, 0]], p[tri[:, 2]] - p[tri[:, 0]])
    length = np.linalg.norm(n, axis=1)
    assert len(tri) > 0 and length.min() > 0
    assert np.abs(n / length[:, None] - np.array([0.0, 0.0, -1.0])).max() <= 2.0 ** -22
    return len(tri)


def random_volume(dims, seed, invalid=0.0):
    """values uniform in (-1, 1), f32; a fraction `invalid` of the voxels has weight 0, the rest 1"""
    rng = np.random.default_rng([seed] + list(dims))
    vol = REF.Volume((0.0, 0.0, 0.0), 1.0, dims, 3.0)
    vol.tsdf = rng.uniform(-1, 1, vol.tsdf.shape).astype(F)
    vol.tsdf[vol.tsdf == 0] = F(0.5)
    vol.w = (rng.random(vol.tsdf.shape) >= invalid).astype(F)
    return vol
