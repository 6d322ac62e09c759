"""Clean-up of an indexed triangle mesh on the MI355X, part one -- connected components: label the connected pieces, count them, and drop the small
ones -- the clean-up between TSDFVolume.extract_triangle_mesh and cloud_io.write_ply_mesh, where a volume fused from noisy depth
carries one large surface plus floaters of a few triangles each (what users of Open3D do with cluster_connected_triangles; no
parity with Open3D is claimed: two triangles are connected here when they share a VERTEX).  Everything is integer-exact.
Semantics: include/r3d.h ("Mesh components") and DESIGN.md section 4.5j'.

Part two -- smoothing: the vertex adjacency (one-ring CSR and boundary flags), Laplacian and Taubin smoothing as a sequence of
umbrella steps, and area-weighted vertex normals of the moved mesh (what users of Open3D do with filter_smooth_taubin and
compute_vertex_normals; no parity is claimed).  Every bit is specified: include/r3d.h ("Mesh smoothing") and DESIGN.md section
4.5j''.

The *_device functions take raw device addresses and leave their results in HBM.
"""
import math
import collections
import ctypes as C

import numpy as np

from . import _lib as L
from ._args import MAX_ITEMS, count as _count
from .device import default_context

NO_LABEL = 0xFFFFFFFF   # the triangle label of an invalid triangle

MeshComponents = collections.namedtuple("MeshComponents", ["vertex_labels", "triangle_labels", "components", "n_invalid"])
MeshComponents.__doc__ = ("vertex_labels [N] uint32 (the smallest vertex index of the vertex's component), triangle_labels [M] uint32 "
                          "(the label of the triangle's first index; 0xFFFFFFFF for a triangle with an index outside [0, N)), "
                          "components [K,3] uint32 rows (label, vertices, triangles) in ascending label -- the components that have "
                          "a triangle --, n_invalid: the number of invalid triangles.")


def _triangles(triangles):
    t = np.asarray(triangles)
    if t.size == 0:
        t = np.zeros((0, 3), np.int32)
    if t.ndim != 2 or t.shape[1] != 3 or t.dtype.kind not in "iu":
        raise ValueError("triangles must be an [M,3] integer array, got %s of shape %s" % (t.dtype, list(t.shape)))
    if t.dtype != np.int32:
        if t.size and (t.min() < -2 ** 31 or t.max() > MAX_ITEMS):
            raise ValueError("triangle indices must fit int32")
        t = t.astype(np.int32)
    if len(t) > MAX_ITEMS:
        raise ValueError("a mesh takes at most 2^31 - 1 triangles")
    return np.ascontiguousarray(t)


def _min_triangles(v):
    if isinstance(v, bool) or not isinstance(v, (int, np.integer)) or not 1 <= int(v) < 2 ** 63:
        raise ValueError("min_triangles must be an integer >= 1, got %r" % (v,))
    return int(v)


def mesh_components_device(ctx, d_tri, n_triangles, n_vertices, d_vertex_labels, d_triangle_labels=None, d_components=None,
                           cap_components=0):
    """Labels into d_vertex_labels ([n_vertices] uint32) and d_triangle_labels ([n_triangles] uint32, optional), component rows
    into d_components ([cap_components][3] uint32, optional) at raw device addresses; d_tri: [n_triangles][3] int32.  Returns the
    TRUE (n_components, n_invalid); at most cap_components rows were written.  Synchronises."""
    nt, nv, cap = _count(n_triangles, "n_triangles"), _count(n_vertices, "n_vertices"), _count(cap_components, "cap_components")
    k, bad = C.c_int64(), C.c_int64()
    L.check(ctx.lib.r3d_mesh_components(ctx.handle, d_tri, nt, nv, d_vertex_labels, d_triangle_labels, d_components, cap, C.byref(k),
                                        C.byref(bad)))
    return k.value, bad.value


def remove_small_components_device(ctx, d_tri, n_triangles, n_vertices, d_vertex_labels, min_triangles=1, keep_largest=False,
                                   d_kept_vertices=None, cap_vertices=0, d_tri_out=None, cap_triangles=0):
    """The kept vertices' old indices into d_kept_vertices ([cap_vertices] uint32: the row list r3d_gather_rows takes) and the kept
    triangles, renumbered, into d_tri_out ([cap_triangles][3] int32) at raw device addresses; d_vertex_labels: what
    mesh_components_device wrote for this mesh.  Returns the TRUE (n_vertices, n_triangles) kept; at most cap_* rows each were
    written.  Synchronises."""
    nt, nv = _count(n_triangles, "n_triangles"), _count(n_vertices, "n_vertices")
    cv, ct = _count(cap_vertices, "cap_vertices"), _count(cap_triangles, "cap_triangles")
    kv, kt = C.c_int64(), C.c_int64()
    L.check(ctx.lib.r3d_mesh_filter_components(ctx.handle, d_tri, nt, nv, d_vertex_labels, _min_triangles(min_triangles),
                                               1 if keep_largest else 0, d_kept_vertices, cv, d_tri_out, ct, C.byref(kv), C.byref(kt)))
    return kv.value, kt.value


def gather_rows_device(ctx, d_xyz, n_points, d_rows, n_out, d_xyz_out):
    """d_xyz_out[k] = d_xyz[d_rows[k]] for [n][3] float32 rows (r3d_gather_rows).  Asynchronous."""
    L.check(ctx.lib.r3d_gather_rows(ctx.handle, d_xyz, int(n_points), d_rows, int(n_out), d_xyz_out))


def mesh_components(triangles, n_vertices, ctx=None):
    """MeshComponents of the mesh whose [M,3] integer `triangles` index n_vertices vertices."""
    tri, nv = _triangles(triangles), _count(n_vertices, "n_vertices")
    nt = len(tri)
    ctx = ctx or default_context()
    with ctx.buffers() as B:
        d_tri, d_vl, d_tl = B.upload(tri), B.alloc(nv * 4), B.alloc(nt * 4)
        k, bad = mesh_components_device(ctx, d_tri.ptr, nt, nv, d_vl.ptr, d_tl.ptr)
        rows = np.zeros((0, 3), np.uint32)
        if k:
            d_rows = B.alloc(k * 12)
            got = mesh_components_device(ctx, d_tri.ptr, nt, nv, d_vl.ptr, d_tl.ptr, d_rows.ptr, k)
            assert got == (k, bad), (got, k, bad)
            rows = d_rows.download_array(np.uint32, (k, 3))
        return MeshComponents(d_vl.download_array(np.uint32, (nv,)), d_tl.download_array(np.uint32, (nt,)), rows, bad)


def filter_mesh_device(ctx, d_xyz, d_normals, d_tri, n_vertices, n_triangles, min_triangles, keep_largest, B):
    """The device-resident mesh (raw addresses) filtered on the device: (d_xyz, d_normals, d_tri, kept [n] uint32 on the host,
    n, m, n_components) with the three arrays new DeviceBuffers of the caller's buffer scope B.  Positions and normals go through
    r3d_gather_rows."""
    nv, nt = n_vertices, n_triangles
    d_vl, d_kept, d_out = B.alloc(nv * 4), B.alloc(nv * 4), B.alloc(nt * 12)
    k, _ = mesh_components_device(ctx, d_tri, nt, nv, d_vl.ptr)
    n, m = remove_small_components_device(ctx, d_tri, nt, nv, d_vl.ptr, min_triangles, keep_largest, d_kept.ptr, nv, d_out.ptr, nt)
    d_xyz_out, d_nrm_out = B.alloc(n * 12), B.alloc(n * 12)
    if n:
        gather_rows_device(ctx, d_xyz, nv, d_kept.ptr, n, d_xyz_out.ptr)
        gather_rows_device(ctx, d_normals, nv, d_kept.ptr, n, d_nrm_out.ptr)
    return d_xyz_out, d_nrm_out, d_out, d_kept.download_array(np.uint32, (n,)), n, m, k


def remove_small_components(xyz, normals, triangles, min_triangles=1, keep_largest=False, colors=None, ctx=None):
    """(xyz, normals, triangles[, colors]) without the components of fewer than min_triangles triangles and, with keep_largest,
    without all but the component with the most triangles (ties: the one with the smallest vertex index); both conditions apply
    together.  Kept triangles and vertices stay in their order, triangles name the new vertex rows, vertices no kept triangle
    names are dropped.  xyz and normals: [N,3] float32; triangles: [M,3] integers (a triangle with an index outside [0, N) is
    dropped); colors: optional [N,...] rows of any dtype, gathered with the kept list.  The dtypes are kept."""
    xyz, normals = np.ascontiguousarray(xyz), np.ascontiguousarray(normals)
    if xyz.ndim != 2 or xyz.shape[1] != 3 or xyz.dtype != np.float32 or normals.shape != xyz.shape or normals.dtype != np.float32:
        raise ValueError("xyz and normals must be [N,3] float32 arrays of one shape, got %s %s and %s %s"
                         % (xyz.dtype, list(xyz.shape), normals.dtype, list(normals.shape)))
    tri_in = np.asarray(triangles)
    tri, mt = _triangles(tri_in), _min_triangles(min_triangles)
    nv, nt = _count(len(xyz), "the number of vertices"), len(tri)
    if colors is not None:
        colors = np.asarray(colors)
        if colors.ndim < 1 or len(colors) != nv:
            raise ValueError("colors must have one row per vertex (%d), got shape %s" % (nv, list(colors.shape)))
    ctx = ctx or default_context()
    with ctx.buffers() as B:
        d_xyz, d_nrm, d_tri = B.upload(xyz), B.upload(normals), B.upload(tri)
        d_x, d_n, d_t, kept, n, m, _ = filter_mesh_device(ctx, d_xyz.ptr, d_nrm.ptr, d_tri.ptr, nv, nt, mt, keep_largest, B)
        tri_dtype = tri_in.dtype if tri_in.size else np.int32
        out = (d_x.download_array(np.float32, (n, 3)), d_n.download_array(np.float32, (n, 3)),
               d_t.download_array(np.int32, (m, 3)).astype(tri_dtype, copy=False))
        return out + (colors[kept],) if colors is not None else out


# ---- smoothing (include/r3d.h "Mesh smoothing")

MAX_STEPS = 4096   # umbrella steps of one smooth_mesh_device call
METHODS = ("taubin", "laplacian")
SMOOTH_KEYS = ("method", "iterations", "lam", "mu", "lock_boundary")   # what extract_triangle_mesh(smooth=...) takes, in this order


def _finite(v, what):
    if isinstance(v, bool) or not isinstance(v, (int, float, np.integer, np.floating)) or not math.isfinite(float(v)):
        raise ValueError("%s must be a finite number, got %r" % (what, v))
    return float(v)


def smooth_factors(method="taubin", iterations=10, lam=0.5, mu=-0.53):
    """The step factors of a filter as a list of floats: [lam] * iterations for "laplacian" (mu is ignored), [lam, mu] * iterations
    for "taubin" (mu < 0 < lam < -mu: the second step undoes the shrinkage of the first)."""
    if method not in METHODS:
        raise ValueError("method must be one of %s, got %r" % (", ".join(METHODS), method))
    if isinstance(iterations, bool) or not isinstance(iterations, (int, np.integer)) or int(iterations) < 0:
        raise ValueError("iterations must be an integer >= 0, got %r" % (iterations,))
    lam = _finite(lam, "lam")
    if lam <= 0:
        raise ValueError("lam must be > 0, got %r" % (lam,))
    steps = [lam]
    if method == "taubin":
        mu = _finite(mu, "mu")
        if not (mu < 0 and -mu > lam):
            raise ValueError("mu must be negative and larger than lam in magnitude (lam %r), got %r" % (lam, mu))
        steps = [lam, mu]
    if len(steps) * int(iterations) > MAX_STEPS:
        raise ValueError("iterations gives %d steps, more than %d" % (len(steps) * int(iterations), MAX_STEPS))
    return steps * int(iterations)


def _factors(factors):
    f = np.ascontiguousarray(np.asarray(factors, np.float64).reshape(-1)) if len(factors) else np.zeros(0, np.float64)
    if len(f) > MAX_STEPS:
        raise ValueError("factors holds %d steps, more than %d" % (len(f), MAX_STEPS))
    if not np.isfinite(f).all():
        raise ValueError("factors must be finite, got %r" % (f[~np.isfinite(f)][0],))
    return f


def _positions(xyz, what="xyz"):
    a = np.ascontiguousarray(xyz)
    if a.ndim != 2 or a.shape[1] != 3 or a.dtype != np.float32:
        raise ValueError("%s must be an [N,3] float32 array, got %s of shape %s" % (what, a.dtype, list(a.shape)))
    _count(len(a), "the number of vertices")
    return a


def smooth_params(smooth):
    """extract_triangle_mesh's `smooth` argument -> the dict of smooth_mesh's keywords: a dict of them, or a tuple in the order
    (method, iterations, lam, mu, lock_boundary), both completed with smooth_mesh's defaults and checked"""
    out = {"method": "taubin", "iterations": 10, "lam": 0.5, "mu": -0.53, "lock_boundary": True}
    if isinstance(smooth, dict):
        unknown = sorted(set(smooth) - set(SMOOTH_KEYS))
        if unknown:
            raise ValueError("smooth has unknown keys %s (it takes %s)" % (unknown, ", ".join(SMOOTH_KEYS)))
        out.update(smooth)
    elif isinstance(smooth, (tuple, list)):
        if len(smooth) > len(SMOOTH_KEYS):
            raise ValueError("smooth takes at most %d values (%s), got %d" % (len(SMOOTH_KEYS), ", ".join(SMOOTH_KEYS), len(smooth)))
        out.update(zip(SMOOTH_KEYS, smooth))
    else:
        raise ValueError("smooth must be None, a dict or a tuple of (%s), got %r" % (", ".join(SMOOTH_KEYS), smooth))
    smooth_factors(out["method"], out["iterations"], out["lam"], out["mu"])
    out["lock_boundary"] = bool(out["lock_boundary"])
    return out


def mesh_adjacency_device(ctx, d_tri, n_triangles, n_vertices, d_row_start, d_neighbours=None, cap_neighbours=0, d_boundary=None):
    """The one-ring CSR of the mesh into d_row_start ([n_vertices + 1] uint32) and d_neighbours ([cap_neighbours] uint32, optional),
    the boundary flags into d_boundary ([n_vertices] uint8, optional) at raw device addresses; d_tri: [n_triangles][3] int32.
    Returns the TRUE number of neighbour entries E; at most cap_neighbours were written.  Synchronises."""
    nt, nv, cap = _count(n_triangles, "n_triangles"), _count(n_vertices, "n_vertices"), _count(cap_neighbours, "cap_neighbours")
    e = C.c_int64()
    L.check(ctx.lib.r3d_mesh_adjacency(ctx.handle, d_tri, nt, nv, d_row_start, d_neighbours, cap, d_boundary, C.byref(e)))
    return e.value


def smooth_mesh_device(ctx, d_xyz_in, d_xyz_out, n_vertices, d_row_start, d_neighbours, d_locked, factors):
    """len(factors) umbrella steps from d_xyz_in into d_xyz_out ([n_vertices][3] float32 each, not overlapping) over the adjacency
    mesh_adjacency_device wrote; d_locked: [n_vertices] uint8 or None.  Asynchronous."""
    f = _factors(factors)
    L.check(ctx.lib.r3d_mesh_smooth(ctx.handle, d_xyz_in, d_xyz_out, _count(n_vertices, "n_vertices"), d_row_start, d_neighbours, d_locked,
                                    f.ctypes.data if len(f) else None, len(f)))


def vertex_normals_device(ctx, d_xyz, n_vertices, d_tri, n_triangles, d_fallback, d_normals):
    """Area-weighted vertex normals into d_normals ([n_vertices][3] float32); d_fallback: the rows of vertices without area, or
    None for zeros.  Asynchronous."""
    L.check(ctx.lib.r3d_mesh_vertex_normals(ctx.handle, d_xyz, _count(n_vertices, "n_vertices"), d_tri, _count(n_triangles, "n_triangles"),
                                            d_fallback, d_normals))


def adjacency_buffers(ctx, d_tri, n_triangles, n_vertices, B):
    """(d_row_start, d_neighbours, d_boundary, E) as new DeviceBuffers of the buffer scope B: the two-call round trip for the cap"""
    nv = n_vertices
    d_rs, d_bd = B.alloc((nv + 1) * 4), B.alloc(nv)
    e = mesh_adjacency_device(ctx, d_tri, n_triangles, nv, d_rs.ptr, None, 0, d_bd.ptr)
    d_nb = B.alloc(e * 4)
    if e:
        got = mesh_adjacency_device(ctx, d_tri, n_triangles, nv, d_rs.ptr, d_nb.ptr, e, d_bd.ptr)
        assert got == e, (got, e)
    return d_rs, d_nb, d_bd, e


def smooth_mesh_buffers(ctx, d_xyz, d_normals, d_tri, n_vertices, n_triangles, params, B):
    """The device-resident mesh (raw addresses; d_normals the fallback or None) smoothed on the device: (d_xyz, d_normals, stats)
    with the two arrays new DeviceBuffers of the caller's buffer scope B and stats the dict {"vertices", "edges",
    "boundary_vertices", "steps"}.  params: smooth_params' dict."""
    nv, nt = n_vertices, n_triangles
    factors = smooth_factors(params["method"], params["iterations"], params["lam"], params["mu"])
    d_rs, d_nb, d_bd, e = adjacency_buffers(ctx, d_tri, nt, nv, B)
    d_out, d_nrm = B.alloc(nv * 12), B.alloc(nv * 12)
    smooth_mesh_device(ctx, d_xyz, d_out.ptr, nv, d_rs.ptr, d_nb.ptr, d_bd.ptr if params["lock_boundary"] else None, factors)
    vertex_normals_device(ctx, d_out.ptr, nv, d_tri, nt, d_normals, d_nrm.ptr)
    boundary = int(np.count_nonzero(d_bd.download_array(np.uint8, (nv,))))
    return d_out, d_nrm, {"vertices": nv, "edges": e // 2, "boundary_vertices": boundary, "steps": len(factors)}


def mesh_adjacency(triangles, n_vertices, ctx=None):
    """(row_start [N + 1] uint32, neighbours [E] uint32, boundary [N] bool) of the mesh whose [M,3] integer `triangles` index
    n_vertices vertices: row u of the CSR holds u's distinct neighbours in ascending index; boundary[u]: u lies on an edge that
    exactly one triangle side has."""
    tri, nv = _triangles(triangles), _count(n_vertices, "n_vertices")
    ctx = ctx or default_context()
    with ctx.buffers() as B:
        d_rs, d_nb, d_bd, e = adjacency_buffers(ctx, B.upload(tri).ptr, len(tri), nv, B)
        return (d_rs.download(np.uint32, nv + 1), d_nb.download_array(np.uint32, (e,)), d_bd.download_array(np.uint8, (nv,)).astype(bool))


def _upload_mesh(B, xyz, tri, rows):
    """xyz, tri and the optional [N,3] float32 `rows` in new DeviceBuffers of the buffer scope B; the last is None without rows"""
    return B.upload(xyz), B.upload(tri), None if rows is None else B.upload(rows)


def _fallback(rows, nv, what):
    if rows is None:
        return None
    rows = _positions(rows, what)
    if len(rows) != nv:
        raise ValueError("%s must have one row per vertex (%d), got %d" % (what, nv, len(rows)))
    return rows


def smooth_mesh(xyz, triangles, method="taubin", iterations=10, lam=0.5, mu=-0.53, lock_boundary=True, normals=None, ctx=None):
    """(xyz, normals) of the mesh after `iterations` rounds of Taubin (a lam step, then a mu step) or Laplacian (lam steps)
    smoothing over the one-ring of every vertex, each step moving a vertex towards (lam) or away from (mu) the mean of its
    neighbours; with lock_boundary the vertices on an open edge stay where they are.  normals: the rows that come back for vertices
    without area (isolated ones); the others get the area-weighted normals of the moved mesh.  The triangles are unchanged."""
    xyz, tri = _positions(xyz), _triangles(triangles)
    nv = len(xyz)
    normals = _fallback(normals, nv, "normals")
    params = smooth_params({"method": method, "iterations": iterations, "lam": lam, "mu": mu, "lock_boundary": lock_boundary})
    ctx = ctx or default_context()
    with ctx.buffers() as B:
        d_xyz, d_tri, d_nrm = _upload_mesh(B, xyz, tri, normals)
        d_out, d_n, _ = smooth_mesh_buffers(ctx, d_xyz.ptr, d_nrm.ptr if d_nrm else None, d_tri.ptr, nv, len(tri), params, B)
        return d_out.download_array(np.float32, (nv, 3)), d_n.download_array(np.float32, (nv, 3))


def compute_vertex_normals(xyz, triangles, fallback=None, ctx=None):
    """[N,3] float32 area-weighted vertex normals: the normalised sum of (b - a) x (c - a) over the triangles that name the
    vertex; a vertex without area gets its row of `fallback`, or zeros."""
    xyz, tri = _positions(xyz), _triangles(triangles)
    nv = len(xyz)
    fallback = _fallback(fallback, nv, "fallback")
    ctx = ctx or default_context()
    with ctx.buffers() as B:
        d_xyz, d_tri, d_fb = _upload_mesh(B, xyz, tri, fallback)
        d_n = B.alloc(nv * 12)
        vertex_normals_device(ctx, d_xyz.ptr, nv, d_tri.ptr, len(tri), d_fb.ptr if d_fb else None, d_n.ptr)
        return d_n.download_array(np.float32, (nv, 3))
