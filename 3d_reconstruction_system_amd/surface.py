"""A surface from an oriented cloud on the MI355X: the step behind the fused cloud.  A merged, downsampled, cleaned cloud with
oriented normals (estimate_normals) is written into a TSDF volume as the signed distance to the tangent plane of every voxel's
nearest point (Hoppe et al.; include/r3d.h "TSDF from an oriented cloud", TSDFVolume.integrate_cloud), and the volume's own
marching cubes, component filter and smoothing make the mesh.

volume_for_cloud sizes a volume around a cloud; reconstruct_surface is cloud -> mesh in one call.
"""
import numpy as np

from ._args import whole as _whole
from .tsdf import TSDFVolume, _cloud_rows, _positive_f32

MAX_MESH_VOXELS = ((1 << 32) + 4) // 5 - 1   # r3d_tsdf_extract_mesh takes volumes of fewer than 2^32 / 5 voxels


def cloud_volume_geometry(xyz, voxel_size, trunc_voxels=4, margin_voxels=None):
    """(origin [3] float64, dims (nx, ny, nz), sdf_trunc) of the volume volume_for_cloud makes: the bounding box of the cloud's
    finite points, grown by margin_voxels voxels on every side (None: trunc_voxels, so that the whole truncation band is
    inside), origin on the voxel lattice through 0.  No device is needed."""
    p = _cloud_rows(xyz, "xyz")
    vs = _positive_f32(voxel_size, "voxel_size")
    tv = _whole(trunc_voxels, "trunc_voxels", 1)
    mv = tv if margin_voxels is None else _whole(margin_voxels, "margin_voxels", 0)
    p = p[np.isfinite(p).all(axis=1)].astype(np.float64)
    if p.shape[0] == 0:
        raise ValueError("the cloud has no finite point")
    lo = np.floor(p.min(axis=0) / vs) - mv
    hi = np.floor(p.max(axis=0) / vs) + 1 + mv
    dims = tuple(int(d) for d in (hi - lo))
    n_voxels = dims[0] * dims[1] * dims[2]
    if n_voxels > MAX_MESH_VOXELS:
        raise ValueError("a volume of %d x %d x %d voxels (%d) is more than mesh extraction takes (%d): use a larger voxel_size"
                         % (dims + (n_voxels, MAX_MESH_VOXELS)))
    origin = lo * vs
    if not np.isfinite(origin.astype(np.float32)).all():
        raise ValueError("the cloud's bounding box does not fit float32")
    return origin, dims, _positive_f32(tv * vs, "sdf_trunc")


def volume_for_cloud(xyz, voxel_size, trunc_voxels=4, margin_voxels=None, color=False, ctx=None):
    """A fresh TSDFVolume around the cloud's finite points: their bounding box plus margin_voxels voxels on every side (None:
    trunc_voxels), sdf_trunc = trunc_voxels * voxel_size.  ValueError for a cloud without a finite point and for more voxels
    than mesh extraction takes (fewer than 2^32 / 5)."""
    origin, dims, trunc = cloud_volume_geometry(xyz, voxel_size, trunc_voxels, margin_voxels)
    return TSDFVolume(origin, voxel_size, dims, trunc, ctx=ctx, color=bool(color))


def reconstruct_surface(xyz, normals, voxel_size, rgb=None, trunc_voxels=4, min_component_triangles=None, keep_largest=False,
                        smooth=None, margin_voxels=None, ctx=None):
    """The triangle mesh of an oriented cloud: (xyz [V,3] float32, normals [V,3] float32, triangles [M,3] int32), and with rgb
    ([N,3] uint8, one colour per point) a fourth array, the vertices' colours [V,3] uint8 -- what
    TSDFVolume.extract_triangle_mesh returns, whose min_component_triangles, keep_largest and smooth these are.  The normals
    must point out of the surface (estimate_normals(viewpoint=...) orients them); voxel_size is the resolution of the result
    and should not be smaller than the cloud's point spacing: a voxel farther than trunc_voxels * voxel_size from every point
    stays empty, and a cell with an empty corner gets no triangle.  margin_voxels: volume_for_cloud's."""
    vol = volume_for_cloud(xyz, voxel_size, trunc_voxels, margin_voxels, color=rgb is not None, ctx=ctx)
    try:
        vol.integrate_cloud(xyz, normals, rgb)
        return vol.extract_triangle_mesh(1.0, with_colors=rgb is not None, min_component_triangles=min_component_triangles,
                                         keep_largest=keep_largest, smooth=smooth)
    finally:
        vol.close()
