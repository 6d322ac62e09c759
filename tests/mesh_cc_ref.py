"""Plain Python / NumPy restatement of the mesh component specification (include/r3d.h, "Mesh components"): union-find over the
vertices, integer counts, the filter and the order-preserving compaction.  Sequential, nothing clever.  Test infrastructure only."""
import numpy as np

NO_LABEL = 0xFFFFFFFF


def valid_mask(tri, n_vertices):
    t = np.asarray(tri, dtype=np.int64).reshape(-1, 3)
    return ((t >= 0) & (t < n_vertices)).all(axis=1)


def components(tri, n_vertices):
    """(vertex_labels [N] u32, triangle_labels [M] u32, rows [K,3] u32 {label, vertices, triangles}, n_invalid)"""
    t = np.asarray(tri, dtype=np.int64).reshape(-1, 3)
    ok = valid_mask(t, n_vertices)
    parent = list(range(n_vertices))

    def find(v):
        root = v
        while parent[root] != root:
            root = parent[root]
        while parent[v] != root:
            parent[v], v = root, parent[v]
        return root

    for a, b, c in t[ok].tolist():
        for other in (b, c):
            ra, rb = find(a), find(other)
            if ra != rb:
                parent[max(ra, rb)] = min(ra, rb)                # the smaller root stays: a root is its tree's minimum
    labels = np.array([find(v) for v in range(n_vertices)], dtype=np.uint32).reshape(n_vertices)
    tri_labels = np.full(len(t), NO_LABEL, dtype=np.uint32)
    tri_labels[ok] = labels[t[ok, 0]]
    n_vert = np.bincount(labels, minlength=n_vertices) if n_vertices else np.zeros(0, np.int64)
    n_tri = np.bincount(tri_labels[ok], minlength=n_vertices) if n_vertices else np.zeros(0, np.int64)
    roots = np.flatnonzero(n_tri > 0)                            # ascending label
    rows = np.stack([roots, n_vert[roots], n_tri[roots]], axis=1).astype(np.uint32).reshape(-1, 3)
    return labels, tri_labels, rows, int((~ok).sum())


def filter_components(tri, n_vertices, vertex_labels, min_triangles=1, keep_largest=False):
    """(kept_vertices [n] u32: old index of every new vertex, triangles [m,3] int32 naming the new indices)"""
    assert min_triangles >= 1
    t = np.asarray(tri, dtype=np.int64).reshape(-1, 3)
    labels = np.asarray(vertex_labels, dtype=np.int64)
    ok = valid_mask(t, n_vertices)
    first = np.where(ok, t[:, 0], 0)
    lab = labels[first] if n_vertices else np.zeros(len(t), np.int64)
    ok &= (lab >= 0) & (lab < n_vertices)                        # a label outside the mesh is data: its triangles are invalid
    counts = np.bincount(lab[ok], minlength=max(n_vertices, 1))
    keep = ok & (counts[np.where(ok, lab, 0)] >= min_triangles)
    if keep_largest:
        best = int(np.argmax(counts)) if ok.any() else -1        # argmax returns the FIRST maximum: the smallest label
        keep &= lab == best
    kept_tri = t[keep]
    used = np.zeros(n_vertices, bool)
    used[kept_tri.reshape(-1)] = True
    kept_vertices = np.flatnonzero(used).astype(np.uint32)
    new = np.cumsum(used) - 1
    return kept_vertices, new[kept_tri].astype(np.int32).reshape(-1, 3)


def remove_small(xyz, normals, tri, min_triangles=1, keep_largest=False, colors=None):
    """the filtered mesh: (xyz, normals, triangles[, colors])"""
    n = len(xyz)
    labels = components(tri, n)[0]
    kept, out = filter_components(tri, n, labels, min_triangles, keep_largest)
    res = (np.asarray(xyz)[kept], np.asarray(normals)[kept], out)
    return res + (np.asarray(colors)[kept],) if colors is not None else res


# ---- meshes shared by tests/test_mesh_cc_host.py (which asserts their conditions of this restatement) and the GPU tests ---------
def strip(n, ids=None):
    """n triangles (i, i+1, i+2) over n + 2 vertices, renamed through ids"""
    i = np.arange(n, dtype=np.int64)
    t = np.stack([i, i + 1, i + 2], axis=1)
    return (t if ids is None else np.asarray(ids, dtype=np.int64)[t]).astype(np.int32)


def disjoint(n):
    """n triangles (3i, 3i+1, 3i+2): n components"""
    return np.arange(3 * n, dtype=np.int32).reshape(n, 3)


def fans(n_fans, per_fan):
    """n_fans fans of per_fan triangles each around the shared hub vertex 0: one component.  Fan f has its own rim vertices."""
    rows, nxt = [], 1
    for _ in range(n_fans):
        rim = np.arange(nxt, nxt + per_fan + 1)
        nxt += per_fan + 1
        rows += [(0, rim[k], rim[k + 1]) for k in range(per_fan)]
    return np.asarray(rows, dtype=np.int32), nxt
