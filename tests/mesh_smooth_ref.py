"""Plain Python / NumPy restatement of the mesh smoothing specification (include/r3d.h, "Mesh smoothing"): the one-ring adjacency
and the boundary flags, the umbrella steps, and the area-weighted vertex normals, every sum in the specified order.  The sums run
over all vertices at once, but for each vertex the k-th term is added in the k-th round, so a vertex sees exactly the sequence of
fp64 operations the text writes out; adjacency_loops and the *_loops variants below are the same rules as sequential Python loops,
for the small meshes of the host tests.  Test infrastructure only."""
import numpy as np

import mesh_cc_ref as CC

F = np.float32


# ---- adjacency ----------------------------------------------------------------------------------------------------------------
def sides(tri, n_vertices):
    """[S,2] int64: both directions of every side of every valid triangle, sides with u == v dropped"""
    t = np.asarray(tri, dtype=np.int64).reshape(-1, 3)
    t = t[CC.valid_mask(t, n_vertices)]                          # the validity rule of "Mesh components", not restated
    uv = np.concatenate([t[:, [0, 1]], t[:, [1, 2]], t[:, [2, 0]]])
    uv = uv[uv[:, 0] != uv[:, 1]]
    return np.concatenate([uv, uv[:, ::-1]])


def adjacency(tri, n_vertices):
    """(row_start [N + 1] u32, neighbours [E] u32, boundary [N] u8)"""
    uv = sides(tri, n_vertices)
    key, count = np.unique(uv[:, 0] * max(n_vertices, 1) + uv[:, 1], return_counts=True)   # ascending (u, v)
    u, v = key // max(n_vertices, 1), key % max(n_vertices, 1)
    row_start = np.zeros(n_vertices + 1, np.int64)
    np.add.at(row_start, u + 1, 1)
    boundary = np.zeros(n_vertices, np.uint8)
    boundary[u[count == 1]] = 1                                  # the edge {u, v} has one side: (u, v) and (v, u) occur once each
    return np.cumsum(row_start).astype(np.uint32), v.astype(np.uint32), boundary


def adjacency_loops(tri, n_vertices):
    """the same, triangle by triangle and side by side"""
    rings = [set() for _ in range(n_vertices)]
    edge_sides = {}
    for a, b, c in np.asarray(tri, dtype=np.int64).reshape(-1, 3).tolist():
        if not all(0 <= i < n_vertices for i in (a, b, c)):
            continue
        for u, v in ((a, b), (b, c), (c, a)):
            if u == v:
                continue
            rings[u].add(v)
            rings[v].add(u)
            edge = (min(u, v), max(u, v))
            edge_sides[edge] = edge_sides.get(edge, 0) + 1
    row_start, neighbours = [0], []
    for ring in rings:
        neighbours += sorted(ring)
        row_start.append(len(neighbours))
    boundary = np.zeros(n_vertices, np.uint8)
    for (u, v), n in edge_sides.items():
        if n == 1:
            boundary[u] = boundary[v] = 1
    return np.asarray(row_start, np.uint32), np.asarray(neighbours, np.uint32), boundary


# ---- umbrella steps -------------------------------------------------------------------------------------------------------------
def smooth_factors(method="taubin", iterations=10, lam=0.5, mu=-0.53):
    return ([lam, mu] if method == "taubin" else [lam]) * iterations


def step(p, row_start, neighbours, locked, f):
    """one umbrella step of the [N,3] f32 positions; a new array"""
    rs, nb = np.asarray(row_start, np.int64), np.asarray(neighbours, np.int64)
    deg = rs[1:] - rs[:-1]
    move = deg > 0
    if locked is not None:
        move &= np.asarray(locked) == 0
    idx = np.flatnonzero(move)
    out = p.copy()
    if idx.size == 0:
        return out
    with np.errstate(all="ignore"):
        s = p[nb[rs[idx]]].astype(np.float64)                    # (double)p[j0]
        for k in range(1, int(deg[idx].max())):
            more = deg[idx] > k
            s[more] = s[more] + p[nb[rs[idx[more]] + k]].astype(np.float64)      # ... + (double)p[jk], in row order
        m = s / deg[idx].astype(np.float64)[:, None]
        own = p[idx].astype(np.float64)
        out[idx] = (own + np.float64(f) * (m - own)).astype(F)
    return out


def smooth(xyz, row_start, neighbours, locked, factors):
    """the positions after the steps of `factors`, each reading the previous step's positions"""
    p = np.array(xyz, dtype=F, copy=True).reshape(-1, 3)
    for f in factors:
        p = step(p, row_start, neighbours, locked, f)
    return p


def step_loops(p, row_start, neighbours, locked, f):
    out = p.copy()
    for i in range(len(p)):
        r0, r1 = int(row_start[i]), int(row_start[i + 1])
        if r1 == r0 or (locked is not None and locked[i]):
            continue
        with np.errstate(all="ignore"):
            for c in range(3):
                s = np.float64(p[neighbours[r0], c])
                for r in range(r0 + 1, r1):
                    s = s + np.float64(p[neighbours[r], c])
                m = s / np.float64(r1 - r0)
                out[i, c] = F(np.float64(p[i, c]) + np.float64(f) * (m - np.float64(p[i, c])))
    return out


# ---- vertex normals -------------------------------------------------------------------------------------------------------------
def face_normals(xyz, t):
    """[M,3] f64 (b - a) x (c - a) of the triangles t ([M,3] valid indices), from the f32 positions widened first"""
    p = np.asarray(xyz, dtype=F).astype(np.float64)
    a = p[t[:, 0]]
    e1, e2 = p[t[:, 1]] - a, p[t[:, 2]] - a
    return np.stack([e1[:, 1] * e2[:, 2] - e1[:, 2] * e2[:, 1],
                     e1[:, 2] * e2[:, 0] - e1[:, 0] * e2[:, 2],
                     e1[:, 0] * e2[:, 1] - e1[:, 1] * e2[:, 0]], axis=1)


def _normalise(s, fallback):
    with np.errstate(all="ignore"):
        length = np.sqrt((s[:, 0] * s[:, 0] + s[:, 1] * s[:, 1]) + s[:, 2] * s[:, 2])
        ok = (length > 0) & (length < np.inf)
        out = np.zeros((len(s), 3), F) if fallback is None else np.array(fallback, dtype=F, copy=True).reshape(-1, 3)
        out[ok] = (s[ok] / length[ok, None]).astype(F)
    return out


def vertex_normals(xyz, tri, fallback=None):
    """[N,3] f32"""
    n = len(xyz)
    t = np.asarray(tri, dtype=np.int64).reshape(-1, 3)
    t = t[CC.valid_mask(t, n)]
    s = np.zeros((n, 3), np.float64)
    with np.errstate(all="ignore"):
        fn = face_normals(xyz, t)
        corner_vertex = t.reshape(-1)                            # corner 3 t + c, ascending
        order = np.argsort(corner_vertex, kind="stable")         # by vertex; a vertex's corners stay in ascending 3 t + c
        v = corner_vertex[order]
        first = np.searchsorted(v, np.arange(n), side="left")
        count = np.searchsorted(v, np.arange(n), side="right") - first
        for k in range(int(count.max()) if n and len(v) else 0):
            idx = np.flatnonzero(count > k)
            s[idx] = s[idx] + fn[order[first[idx] + k] // 3]
    return _normalise(s, fallback)


def vertex_normals_loops(xyz, tri, fallback=None):
    n = len(xyz)
    p = np.asarray(xyz, dtype=F).astype(np.float64)
    s = np.zeros((n, 3), np.float64)
    with np.errstate(all="ignore"):
        for a, b, c in np.asarray(tri, dtype=np.int64).reshape(-1, 3).tolist():
            if not all(0 <= i < n for i in (a, b, c)):
                continue
            e1, e2 = p[b] - p[a], p[c] - p[a]
            fn = np.array([e1[1] * e2[2] - e1[2] * e2[1], e1[2] * e2[0] - e1[0] * e2[2], e1[0] * e2[1] - e1[1] * e2[0]])
            for i in (a, b, c):
                s[i] = s[i] + fn
    return _normalise(s, fallback)


def smooth_mesh(xyz, tri, method="taubin", iterations=10, lam=0.5, mu=-0.53, lock_boundary=True, normals=None):
    """(xyz, normals): the three rules chained, as mesh.smooth_mesh chains the device calls"""
    rs, nb, bd = adjacency(tri, len(xyz))
    moved = smooth(xyz, rs, nb, bd if lock_boundary else None, smooth_factors(method, iterations, lam, mu))
    return moved, vertex_normals(moved, tri, normals)


# ---- measures and meshes shared by tests/test_mesh_smooth_host.py and the GPU tests -------------------------------------------------
def enclosed_volume(xyz, tri, centre):
    p = np.asarray(xyz, dtype=np.float64) - centre
    a, b, c = p[tri[:, 0]], p[tri[:, 1]], p[tri[:, 2]]
    return float((a * np.cross(b, c)).sum() / 6.0)


def fan(n):
    """n triangles (0, k, k + 1) around the hub 0 over n + 2 vertices: the hub's row holds n + 1 neighbours"""
    k = np.arange(1, n + 1, dtype=np.int32)
    return np.stack([np.zeros(n, np.int32), k, k + 1], axis=1)


def grid(nx, ny):
    """(xyz [nx * ny, 3] f32 in the plane z = 0.25 with jittered x, y; triangles: two per cell)"""
    rng = np.random.default_rng([nx, ny])
    gx, gy = np.meshgrid(np.arange(nx, dtype=np.float64), np.arange(ny, dtype=np.float64))
    xyz = np.stack([gx + rng.uniform(-0.2, 0.2, gx.shape), gy + rng.uniform(-0.2, 0.2, gy.shape), np.full(gx.shape, 0.25)], axis=-1)
    i = (np.arange(ny - 1)[:, None] * nx + np.arange(nx - 1)[None, :]).reshape(-1)
    tri = np.concatenate([np.stack([i, i + 1, i + nx], axis=1), np.stack([i + 1, i + nx + 1, i + nx], axis=1)])
    return xyz.reshape(-1, 3).astype(F), tri.astype(np.int32)


def positions(n, seed, scale=10.0):
    """[n,3] f32 seeded positions"""
    return np.random.default_rng([seed, n]).uniform(-scale, scale, (n, 3)).astype(F)
