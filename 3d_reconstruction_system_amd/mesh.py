"""Connected components of an indexed triangle mesh on the MI355X: label the connected pieces, count them, and drop the small
ones -- the clean-up between TSDFVolume.extract_triangle_mesh and cloud_io.write_ply_mesh, where a volume fused from noisy depth
carries one large surface plus floaters of a few triangles each (what users of Open3D do with cluster_connected_triangles; no
parity with Open3D is claimed: two triangles are connected here when they share a VERTEX).  Everything is integer-exact.
Semantics: include/r3d.h ("Mesh components") and DESIGN.md section 4.5j'.

The *_device functions take raw device addresses and leave their results in HBM.
"""
import collections
import ctypes as C

import numpy as np

from . import _lib as L
from .device import default_context

NO_LABEL = 0xFFFFFFFF   # the triangle label of an invalid triangle
MAX_ITEMS = 2 ** 31 - 1

MeshComponents = collections.namedtuple("MeshComponents", ["vertex_labels", "triangle_labels", "components", "n_invalid"])
MeshComponents.__doc__ = ("vertex_labels [N] uint32 (the smallest vertex index of the vertex's component), triangle_labels [M] uint32 "
                          "(the label of the triangle's first index; 0xFFFFFFFF for a triangle with an index outside [0, N)), "
                          "components [K,3] uint32 rows (label, vertices, triangles) in ascending label -- the components that have "
                          "a triangle --, n_invalid: the number of invalid triangles.")


def _count(v, what, lo=0):
    if isinstance(v, bool) or not isinstance(v, (int, np.integer)) or not lo <= int(v) <= MAX_ITEMS:
        raise ValueError("%s must be an integer in [%d, 2^31 - 1], got %r" % (what, lo, v))
    return int(v)


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


def download_rows(buf, dtype, rows, width):
    """[rows, width] of dtype from a DeviceBuffer (nothing is read for 0 rows)"""
    if rows == 0:
        return np.zeros((0, width), dtype)
    return buf.download(dtype, rows * width).reshape(rows, width)


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
    bufs = []
    try:
        d_tri, d_vl, d_tl = ctx.alloc(max(tri.nbytes, 16)), ctx.alloc(max(nv * 4, 16)), ctx.alloc(max(nt * 4, 16))
        bufs += [d_tri, d_vl, d_tl]
        d_tri.upload(tri)
        k, bad = mesh_components_device(ctx, d_tri.ptr, nt, nv, d_vl.ptr, d_tl.ptr)
        rows = np.zeros((0, 3), np.uint32)
        if k:
            d_rows = ctx.alloc(k * 12)
            bufs.append(d_rows)
            got = mesh_components_device(ctx, d_tri.ptr, nt, nv, d_vl.ptr, d_tl.ptr, d_rows.ptr, k)
            assert got == (k, bad), (got, k, bad)
            rows = d_rows.download(np.uint32, 3 * k).reshape(k, 3)
        return MeshComponents(download_rows(d_vl, np.uint32, nv, 1).reshape(-1), download_rows(d_tl, np.uint32, nt, 1).reshape(-1), rows, bad)
    finally:
        for b in bufs:
            b.free()


def filter_mesh_device(ctx, d_xyz, d_normals, d_tri, n_vertices, n_triangles, min_triangles, keep_largest, bufs):
    """The device-resident mesh (raw addresses) filtered on the device: (d_xyz, d_normals, d_tri, kept [n] uint32 on the host,
    n, m, n_components) with the three arrays new DeviceBuffers (appended to bufs, the caller frees them).  Positions and normals go
    through r3d_gather_rows."""
    nv, nt = n_vertices, n_triangles
    d_vl, d_kept, d_out = ctx.alloc(max(nv * 4, 16)), ctx.alloc(max(nv * 4, 16)), ctx.alloc(max(nt * 12, 16))
    bufs += [d_vl, d_kept, d_out]
    k, _ = mesh_components_device(ctx, d_tri, nt, nv, d_vl.ptr)
    n, m = remove_small_components_device(ctx, d_tri, nt, nv, d_vl.ptr, min_triangles, keep_largest, d_kept.ptr, nv, d_out.ptr, nt)
    d_xyz_out, d_nrm_out = ctx.alloc(max(n * 12, 16)), ctx.alloc(max(n * 12, 16))
    bufs += [d_xyz_out, d_nrm_out]
    if n:
        gather_rows_device(ctx, d_xyz, nv, d_kept.ptr, n, d_xyz_out.ptr)
        gather_rows_device(ctx, d_normals, nv, d_kept.ptr, n, d_nrm_out.ptr)
    kept = download_rows(d_kept, np.uint32, n, 1).reshape(-1)
    return d_xyz_out, d_nrm_out, d_out, kept, n, m, k


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
    bufs = []
    try:
        d_xyz, d_nrm, d_tri = ctx.alloc(max(xyz.nbytes, 16)), ctx.alloc(max(normals.nbytes, 16)), ctx.alloc(max(tri.nbytes, 16))
        bufs += [d_xyz, d_nrm, d_tri]
        d_xyz.upload(xyz)
        d_nrm.upload(normals)
        d_tri.upload(tri)
        d_x, d_n, d_t, kept, n, m, _ = filter_mesh_device(ctx, d_xyz.ptr, d_nrm.ptr, d_tri.ptr, nv, nt, mt, keep_largest, bufs)
        tri_dtype = tri_in.dtype if tri_in.size else np.int32
        out = (download_rows(d_x, np.float32, n, 3), download_rows(d_n, np.float32, n, 3),
               download_rows(d_t, np.int32, m, 3).astype(tri_dtype, copy=False))
        return out + (colors[kept],) if colors is not None else out
    finally:
        for b in bufs:
            b.free()
