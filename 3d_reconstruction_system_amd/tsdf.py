"""Dense TSDF volume on the MI355X: depth frames + poses are integrated into a truncated signed distance volume, and its zero
level set comes back as oriented surface points or as an indexed triangle mesh over those points (marching cubes) -- what users
of a depth + pose pipeline expect (Open3D's UniformTSDFVolume; no parity with Open3D is claimed).  Where fuse_frames concatenates the frames' points, the volume averages
overlapping frames.  A volume created with color=True also averages the frames' colour images and returns a colour with every
surface point / mesh vertex.  track() finds the pose of a new depth frame against the model (tracking.py), so a volume can be
built from depth frames and one pose.  Semantics: include/r3d.h (r3d_tsdf_*) and DESIGN.md sections 4.5i to 4.5o.

The volume takes the inputs camera_to_world.py already has: [F,H,W] depth, one pose-file row per frame, a pinhole camera.  Its
poses are WORLD -> CAMERA (p_cam = R p_w + t: the pose file's quaternion and t as they stand, poses_w2c), not the inverted table
fuse_frames takes.  A depth of 0 is "no measurement" here.
"""
import ctypes as C
import math

import numpy as np

from . import _lib as L
from .device import default_context, depth_code
from .fusion import REF_INTRINSICS, _as_batch
from .poses import _rotation_matrix_xyzw

CHUNK = 32   # R3D_TSDF_CHUNK: frames one integration launch applies inside the kernel


def poses_w2c(quats_xyzw, ts):
    """[F,12] float64 rows = (R row-major, t), world -> camera: the rotation of the pose file's scalar-last quaternion
    (normalised first) and its t -- the layout r3d_tsdf_integrate reads.  fuse_frames' pose_table holds the inverse rotation."""
    quats_xyzw = np.asarray(quats_xyzw, dtype=np.float64).reshape(-1, 4)
    ts = np.asarray(ts, dtype=np.float64).reshape(-1, 3)
    if len(quats_xyzw) != len(ts):
        raise ValueError("need one translation per quaternion")
    table = np.empty((len(ts), 12), dtype=np.float64)
    for k in range(len(ts)):
        table[k, :9] = _rotation_matrix_xyzw(quats_xyzw[k]).reshape(9)
        table[k, 9:] = ts[k]
    return table


def _positive_f32(v, what):
    try:
        f = float(v)
    except (TypeError, ValueError):
        raise ValueError("%s must be a finite number > 0, got %r" % (what, v))
    with np.errstate(over="ignore"):
        f32 = np.float32(f)
    if isinstance(v, bool) or not (math.isfinite(f) and f32 > 0 and np.isfinite(f32)):
        raise ValueError("%s must be a finite number > 0 (in float32), got %r" % (what, v))
    return f


def _ray_range(step, t_near, t_far, voxel_size):
    """(step, t_near, t_far) as floats: step=None means voxel_size; t_near finite and >= 0, t_far > t_near (inf allowed), in float32."""
    s = _positive_f32(voxel_size if step is None else step, "step")
    try:
        tn, tf = float(t_near), float(t_far)
    except (TypeError, ValueError):
        raise ValueError("t_near and t_far must be numbers, got %r and %r" % (t_near, t_far))
    with np.errstate(over="ignore"):
        n32, f32 = np.float32(tn), np.float32(tf)
    if isinstance(t_near, bool) or isinstance(t_far, bool) or not (np.isfinite(n32) and n32 >= 0 and f32 > n32):
        raise ValueError("need 0 <= t_near < t_far with t_near finite (in float32), got %r and %r" % (t_near, t_far))
    return s, tn, tf


def _rgb_batch(rgb, shape):
    """rgb as a contiguous [F,H,W,3] uint8 array for depth rasters of shape (F, H, W); [H,W,3] is one frame."""
    c = np.asarray(rgb)
    if c.ndim == 3:
        c = c[None]
    if c.dtype != np.uint8 or c.shape != tuple(shape) + (3,):
        raise ValueError("rgb must be uint8 of shape %s (R, G, B per pixel of every depth raster), got %s of shape %s"
                         % (list(shape) + [3], c.dtype, list(np.shape(rgb))))
    return np.ascontiguousarray(c)


def _unpack_rgba(words):
    """[N,3] uint8 (R, G, B) from the words r | g << 8 | b << 16"""
    w = np.ascontiguousarray(words, dtype=np.uint32)
    return np.stack([w & 0xff, (w >> 8) & 0xff, (w >> 16) & 0xff], axis=1).astype(np.uint8)


def _cloud_rows(a, what):
    """a as a contiguous [N,3] float32 array"""
    a = np.ascontiguousarray(a, dtype=np.float32)
    if a.ndim != 2 or a.shape[1] != 3 or a.shape[0] >= 1 << 32:
        raise ValueError("%s must be [N,3] with N < 2^32, got shape %s" % (what, list(a.shape)))
    return a


def _pose_rows(poses, n_frames):
    p = np.ascontiguousarray(poses, dtype=np.float64)
    if p.ndim != 2 or p.shape != (n_frames, 12):
        raise ValueError("poses_w2c must be [%d,12] float64 rows (R row-major, t), got shape %s" % (n_frames, p.shape))
    return p


class TSDFVolume:
    """origin [3] (the corner of voxel (0, 0, 0); its centre is origin + voxel_size / 2), voxel_size, dims = (nx, ny, nz),
    sdf_trunc: the truncation distance.  One float2 {tsdf, weight} per voxel in HBM; with color=True a second plane of one
    uint32[4] {sum_r, sum_g, sum_b, n} per voxel, and every integrate call takes the frames' colour images."""

    def __init__(self, origin, voxel_size, dims, sdf_trunc, ctx=None, color=False):
        o = np.ascontiguousarray(origin, dtype=np.float64)
        if o.shape != (3,) or not np.isfinite(o.astype(np.float32)).all():
            raise ValueError("origin must be three finite numbers, got %r" % (origin,))
        vs, tr = _positive_f32(voxel_size, "voxel_size"), _positive_f32(sdf_trunc, "sdf_trunc")
        try:
            nx, ny, nz = [int(d) for d in dims]
            exact = all(int(d) == d and not isinstance(d, bool) for d in dims)
        except (TypeError, ValueError):
            raise ValueError("dims must be three integers >= 1, got %r" % (dims,))
        if not exact or min(nx, ny, nz) < 1 or nx * ny * nz >= 1 << 31:
            raise ValueError("dims must be three integers >= 1 with a product below 2^31, got %r" % (dims,))
        self.ctx = ctx or default_context()
        self.origin, self.voxel_size, self.sdf_trunc, self.dims = o, vs, tr, (nx, ny, nz)
        self.n_voxels = nx * ny * nz
        self.color = bool(color)
        self.last_smooth = None       # what the last extract_triangle_mesh(smooth=...) did: vertices, edges, boundary vertices, steps
        h = C.c_void_p()
        create = self.ctx.lib.r3d_tsdf_create_rgb if self.color else self.ctx.lib.r3d_tsdf_create
        L.check(create(self.ctx.handle, o.ctypes.data, vs, nx, ny, nz, tr, C.byref(h)))
        self.handle = h.value
        self._bilateral = self.ctx.buffers()   # owns the two buffers of track(bilateral=): _bilateral_raster
        self._bilateral_bufs = None            # (pixels, vertex map, filtered raster) while they exist
        self.ctx.adopt(self)

    def close(self):
        if self.handle:
            self._free_bilateral()
            self.ctx.lib.r3d_tsdf_destroy(self.handle)
            self.handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def reset(self):
        """Back to the fresh volume: all zero bytes."""
        L.check(self.ctx.lib.r3d_tsdf_reset(self.handle))

    def _check_color(self, given, what):
        if given and not self.color:
            raise ValueError("%s given to a volume without colour (create it with color=True)" % what)
        if self.color and not given:
            raise ValueError("a volume with colour integrates colour images: %s is missing" % what)

    def integrate(self, depths, quats_xyzw, ts, intrinsics=REF_INTRINSICS, depth_scale=1.0, rgb=None):
        """Integrate host rasters [H,W] or [F,H,W] (uint8, uint16 or float32) seen from the pose-file rows (quats_xyzw, ts), in
        frame order.  A volume with colour takes rgb too: [H,W,3] or [F,H,W,3] uint8 (R, G, B), one image per raster.
        Synchronous."""
        self._check_color(rgb is not None, "rgb")
        d = _as_batch(depths)
        f, h, w = d.shape
        if rgb is not None:
            rgb = _rgb_batch(rgb, d.shape)
        table = poses_w2c(quats_xyzw, ts)
        if table.shape[0] != f:
            raise ValueError("%d frames but %d poses" % (f, table.shape[0]))
        if f * h * w == 0:
            return
        cam = self.ctx.camera(h, w, *intrinsics)
        if rgb is not None:
            L.check(self.ctx.lib.r3d_tsdf_integrate_rgb_host(self.handle, cam.handle, d.ctypes.data, depth_code(d.dtype), f,
                                                             float(depth_scale), table.ctypes.data, rgb.ctypes.data))
            return
        L.check(self.ctx.lib.r3d_tsdf_integrate_host(self.handle, cam.handle, d.ctypes.data, depth_code(d.dtype), f, float(depth_scale),
                                                     table.ctypes.data))

    def integrate_device(self, cam, d_depth, depth_dtype, n_frames, poses_w2c, depth_scale=1.0, d_rgb=None):
        """The same from rasters in HBM (d_depth: [n_frames][H][W] of depth_dtype at a raw device address; cam: ctx.camera(...));
        poses_w2c: [n_frames,12] host rows.  A volume with colour takes d_rgb too: [n_frames][H][W][3] uint8 at a raw device
        address.  Asynchronous on the context's stream."""
        n_frames = int(n_frames)
        if n_frames < 0:
            raise ValueError("n_frames must be >= 0, got %d" % n_frames)
        self._check_color(d_rgb is not None, "d_rgb")
        table = _pose_rows(poses_w2c, n_frames)
        if d_rgb is not None:
            L.check(self.ctx.lib.r3d_tsdf_integrate_rgb(self.handle, cam.handle, d_depth, depth_code(depth_dtype), n_frames,
                                                        float(depth_scale), table.ctypes.data, d_rgb))
            return
        L.check(self.ctx.lib.r3d_tsdf_integrate(self.handle, cam.handle, d_depth, depth_code(depth_dtype), n_frames, float(depth_scale),
                                                table.ctypes.data))

    def integrate_cloud(self, xyz, normals, rgb=None):
        """Integrate an oriented cloud as ONE frame: every voxel within sdf_trunc of its nearest point takes the signed distance
        to that point's tangent plane, truncated like a depth frame's (include/r3d.h "TSDF from an oriented cloud"; Hoppe et
        al.).  xyz, normals: [N,3] float32 (normals as estimate_normals orients them, pointing out of the surface; zero or
        non-finite rows contribute nothing, and neither do non-finite points); a volume with colour takes rgb too: [N,3] uint8.
        Composes with integrate() and with itself as running averages.  Returns the number of voxels updated.  Synchronous."""
        self._check_color(rgb is not None, "rgb")
        p, nrm = _cloud_rows(xyz, "xyz"), _cloud_rows(normals, "normals")
        if nrm.shape != p.shape:
            raise ValueError("normals must be [N,3] like the cloud, got %s for %s" % (list(nrm.shape), list(p.shape)))
        words = None
        if rgb is not None:
            c = np.asarray(rgb)
            if c.dtype != np.uint8 or c.shape != p.shape:
                raise ValueError("rgb must be [N,3] uint8 like the cloud, got %s of shape %s" % (c.dtype, list(c.shape)))
            c = c.astype(np.uint32)
            words = np.ascontiguousarray(c[:, 0] | c[:, 1] << 8 | c[:, 2] << 16)
        n = C.c_int64()
        L.check(self.ctx.lib.r3d_tsdf_integrate_cloud_host(self.handle, p.ctypes.data, nrm.ctypes.data,
                                                           None if words is None else words.ctypes.data, p.shape[0], C.byref(n)))
        return n.value

    def integrate_cloud_device(self, index, d_normals, d_rgba=None, want_count=False):
        """The same from a cloud in HBM: index is an NNIndex over it (same context), d_normals its [n][3] float32 normals in the
        cloud's row order and d_rgba (a volume with colour) its [n] uint32 words r | g << 8 | b << 16, at raw device addresses.
        Asynchronous on the context's stream; want_count: synchronises and returns the number of voxels updated."""
        self._check_color(d_rgba is not None, "d_rgba")
        n = C.c_int64()
        L.check(self.ctx.lib.r3d_tsdf_integrate_cloud(self.handle, index.handle, d_normals, d_rgba, C.byref(n) if want_count else None))
        return n.value if want_count else None

    def device_view(self):
        """(raw device address of the [n_voxels][2] float32 {tsdf, weight} array, n_voxels)."""
        p, n = C.c_void_p(), C.c_int64()
        L.check(self.ctx.lib.r3d_tsdf_volume(self.handle, C.byref(p), C.byref(n)))
        return p.value, n.value

    def volume(self):
        """(tsdf, weight): two [nz][ny][nx] float32 arrays."""
        p, n = self.device_view()
        raw = np.empty((n, 2), dtype=np.float32)
        L.check(self.ctx.lib.r3d_download(self.ctx.handle, raw.ctypes.data, p, raw.nbytes))   # synchronous
        nx, ny, nz = self.dims
        return np.ascontiguousarray(raw[:, 0]).reshape(nz, ny, nx), np.ascontiguousarray(raw[:, 1]).reshape(nz, ny, nx)

    def colors_device_view(self):
        """(raw device address of the [n_voxels][4] uint32 {sum_r, sum_g, sum_b, n} plane, n_voxels) of a volume with colour."""
        p, n = C.c_void_p(), C.c_int64()
        L.check(self.ctx.lib.r3d_tsdf_colors(self.handle, C.byref(p), C.byref(n)))
        return p.value, n.value

    def colors(self):
        """(sums [nz,ny,nx,3] uint32, n [nz,ny,nx] uint32): per voxel the sums of the red, green and blue bytes over the frames
        that touched it, and their number."""
        if not self.color:
            raise ValueError("the volume was created without colour (color=True makes one with)")
        p, n = self.colors_device_view()
        raw = np.empty((n, 4), dtype=np.uint32)
        L.check(self.ctx.lib.r3d_download(self.ctx.handle, raw.ctypes.data, p, raw.nbytes))   # synchronous
        nx, ny, nz = self.dims
        return np.ascontiguousarray(raw[:, :3]).reshape(nz, ny, nx, 3), np.ascontiguousarray(raw[:, 3]).reshape(nz, ny, nx)

    def extract_colors_device(self, min_weight, d_rgba, cap):
        """The surface points' colours into d_rgba ([cap] uint32 words r | g << 8 | b << 16 at a raw device address; None with
        cap == 0): word k is the colour of row k of extract_points_device.  Returns the TRUE number of points, of which at most
        cap words were written.  Synchronises."""
        mw, n = _positive_f32(min_weight, "min_weight"), C.c_int64()
        L.check(self.ctx.lib.r3d_tsdf_extract_colors(self.handle, mw, d_rgba, int(cap), C.byref(n)))
        return n.value

    def _extract_colors(self, mw, n):
        """[n,3] uint8: the colours of the n surface points"""
        if n == 0:
            return np.zeros((0, 3), np.uint8)
        with self.ctx.buffers() as B:
            d_rgba = B.alloc(n * 4)
            got = self.extract_colors_device(mw, d_rgba.ptr, n)
            assert got == n, (got, n)
            return _unpack_rgba(d_rgba.download(np.uint32, n))

    def extract_points_device(self, min_weight, d_xyz, d_normals, cap):
        """Surface points into d_xyz / d_normals ([cap][3] float32 device addresses; d_normals may be None); returns the TRUE
        number of points, of which at most cap rows were written.  Synchronises."""
        n = C.c_int64()
        L.check(self.ctx.lib.r3d_tsdf_extract_points(self.handle, _positive_f32(min_weight, "min_weight"), d_xyz, d_normals, int(cap),
                                                     C.byref(n)))
        return n.value

    def extract_point_cloud(self, min_weight=1.0, with_colors=False):
        """(xyz [N,3], normals [N,3]) float32: one point per volume edge whose two voxels have at least min_weight frames each and
        tsdf values of different sign, in linear voxel order (x fastest), per voxel the x, y, z edge; the normals point towards the
        cameras (zero rows where the gradient vanishes).  with_colors (a volume with colour): a third array, [N,3] uint8 R, G, B --
        the two voxels' mean colours, interpolated like the position."""
        mw = _positive_f32(min_weight, "min_weight")
        if with_colors and not self.color:
            raise ValueError("with_colors needs a volume created with color=True")
        n = self.extract_points_device(mw, None, None, 0)
        if n == 0:
            empty = (np.zeros((0, 3), np.float32), np.zeros((0, 3), np.float32))
            return empty + (np.zeros((0, 3), np.uint8),) if with_colors else empty
        with self.ctx.buffers() as B:
            d_xyz, d_nrm = B.alloc(n * 12), B.alloc(n * 12)
            got = self.extract_points_device(mw, d_xyz.ptr, d_nrm.ptr, n)
            assert got == n, (got, n)
            out = (d_xyz.download_array(np.float32, (n, 3)), d_nrm.download_array(np.float32, (n, 3)))
            return out + (self._extract_colors(mw, n),) if with_colors else out

    def extract_mesh_device(self, min_weight, d_xyz, d_normals, cap_vertices, d_tri, cap_triangles):
        """The indexed triangle mesh into d_xyz / d_normals ([cap_vertices][3] float32) and d_tri ([cap_triangles][3] int32) at raw
        device addresses (d_normals may be None; d_xyz with cap_vertices == 0 and d_tri with cap_triangles == 0 too); returns the
        TRUE (n_vertices, n_triangles), of which at most cap_* rows each were written.  The vertices are extract_points_device's
        rows.  Synchronises."""
        mw = _positive_f32(min_weight, "min_weight")
        nv, nt = C.c_int64(), C.c_int64()
        L.check(self.ctx.lib.r3d_tsdf_extract_mesh(self.handle, mw, d_xyz, d_normals, int(cap_vertices), d_tri, int(cap_triangles),
                                                   C.byref(nv), C.byref(nt)))
        return nv.value, nt.value

    def extract_triangle_mesh(self, min_weight=1.0, with_colors=False, min_component_triangles=None, keep_largest=False,
                              with_stats=False, smooth=None):
        """(xyz [N,3] float32, normals [N,3] float32, triangles [M,3] int32): marching cubes over the cells whose eight voxels
        have at least min_weight frames each.  The vertices are extract_point_cloud's rows (one per crossing volume edge, so the
        mesh is welded by construction); a triangle (a, b, c) winds so that (b - a) x (c - a) points towards the cameras, like the
        vertex normals.  with_colors (a volume with colour): a fourth array, [N,3] uint8 R, G, B, the vertices' colours --
        extract_point_cloud's.  min_component_triangles / keep_largest: the mesh is cleaned of floaters on the device before it is
        downloaded -- connected components (by shared vertex) of fewer than min_component_triangles triangles are dropped, and with
        keep_largest all but the component with the most triangles; vertices no kept triangle names go with them, and the order of
        what stays is kept (mesh.remove_small_components; include/r3d.h "Mesh components").  With neither, the call is what it was.
        with_stats (with either of the two): a last element, the dict {"components", "components_kept", "triangles",
        "triangles_kept"}.  smooth: None, or a dict / tuple of mesh.smooth_mesh's keywords (method, iterations, lam, mu,
        lock_boundary): the vertices are smoothed on the device behind the component filter and the normals become the area-weighted
        vertex normals of the moved mesh, the TSDF normals staying where a vertex has no area (include/r3d.h "Mesh smoothing");
        colours, triangles, counts and stats are untouched, and self.last_smooth is the dict {"vertices", "edges",
        "boundary_vertices", "steps"} of the run.  With smooth=None the call is what it was."""
        mw = _positive_f32(min_weight, "min_weight")
        if with_colors and not self.color:
            raise ValueError("with_colors needs a volume created with color=True")
        filtered = min_component_triangles is not None or bool(keep_largest)
        if with_stats and not filtered:
            raise ValueError("with_stats needs min_component_triangles or keep_largest")
        if filtered:
            from .mesh import _min_triangles
            min_tris = _min_triangles(1 if min_component_triangles is None else min_component_triangles)
        params = None
        if smooth is not None:
            from .mesh import smooth_factors, smooth_mesh_buffers, smooth_params
            params = smooth_params(smooth)
            self.last_smooth = {"vertices": 0, "edges": 0, "boundary_vertices": 0,
                                "steps": len(smooth_factors(params["method"], params["iterations"], params["lam"], params["mu"]))}
        n, m = self.extract_mesh_device(mw, None, None, 0, None, 0)
        if n == 0:
            empty = (np.zeros((0, 3), np.float32), np.zeros((0, 3), np.float32), np.zeros((0, 3), np.int32))
            empty = empty + (np.zeros((0, 3), np.uint8),) if with_colors else empty
            return empty + ({"components": 0, "components_kept": 0, "triangles": 0, "triangles_kept": 0},) if with_stats else empty
        with self.ctx.buffers() as B:
            d_xyz, d_nrm, d_tri = B.alloc(n * 12), B.alloc(n * 12), B.alloc(max(m, 1) * 12)
            got = self.extract_mesh_device(mw, d_xyz.ptr, d_nrm.ptr, n, d_tri.ptr if m else None, m)
            assert got == (n, m), (got, n, m)
            if filtered:
                return self._filtered_mesh(B, mw, d_xyz, d_nrm, d_tri, n, m, min_tris, bool(keep_largest), with_colors, with_stats, params)
            if params is not None:
                d_xyz, d_nrm, self.last_smooth = smooth_mesh_buffers(self.ctx, d_xyz.ptr, d_nrm.ptr, d_tri.ptr, n, m, params, B)
            out = (d_xyz.download_array(np.float32, (n, 3)), d_nrm.download_array(np.float32, (n, 3)), d_tri.download_array(np.int32, (m, 3)))
            return out + (self._extract_colors(mw, n),) if with_colors else out

    def _filtered_mesh(self, B, mw, d_xyz, d_nrm, d_tri, n, m, min_tris, keep_largest, with_colors, with_stats, params=None):
        """extract_triangle_mesh's result from the n vertices and m triangles in HBM, filtered there (mesh.filter_mesh_device) and,
        with params, smoothed behind the filter; B: the call's buffer scope"""
        from .mesh import filter_mesh_device, mesh_components_device, smooth_mesh_buffers
        d_x, d_n, d_t, kept, nk, mk, comps = filter_mesh_device(self.ctx, d_xyz.ptr, d_nrm.ptr, d_tri.ptr, n, m, min_tris, keep_largest, B)
        if params is not None:
            d_x, d_n, self.last_smooth = smooth_mesh_buffers(self.ctx, d_x.ptr, d_n.ptr, d_t.ptr, nk, mk, params, B)
        out = (d_x.download_array(np.float32, (nk, 3)), d_n.download_array(np.float32, (nk, 3)), d_t.download_array(np.int32, (mk, 3)))
        if with_colors:
            out += (self._extract_colors(mw, n)[kept],)
        if with_stats:
            kept_comps, _ = mesh_components_device(self.ctx, d_t.ptr, mk, nk, B.alloc(nk * 4).ptr)
            out += ({"components": comps, "components_kept": kept_comps, "triangles": m, "triangles_kept": mk},)
        return out

    def raycast_device(self, cam, n_views, poses_w2c, d_depth, d_vertex, d_normal, min_weight=1.0, step=None, t_near=0.0,
                       t_far=math.inf, d_rgb=None):
        """Ray-cast the volume from n_views poses (poses_w2c: [n_views,12] host rows, as integrate_device takes) through cam into
        d_depth ([n_views][H][W] float32) and d_vertex / d_normal ([n_views][H][W][3] float32, world coordinates) at raw device
        addresses; any of the three may be None.  A pixel without a surface has depth 0 and NaN vertex and normal rows.  step=None
        means voxel_size; step + voxel_size <= sdf_trunc keeps both samples that bracket the surface inside the untruncated band.
        d_rgb (a volume with colour): also the colour image, [n_views][H][W][3] uint8 R, G, B -- the hit cell's eight mean
        colours, interpolated like the tsdf; 0, 0, 0 where there is no surface.  Asynchronous on the context's stream."""
        if d_rgb is not None:
            self._check_color(True, "d_rgb")
        n_views = int(n_views)
        if n_views < 0:
            raise ValueError("n_views must be >= 0, got %d" % n_views)
        table = _pose_rows(poses_w2c, n_views)
        s, tn, tf = _ray_range(step, t_near, t_far, self.voxel_size)
        mw = _positive_f32(min_weight, "min_weight")
        if d_rgb is not None:
            L.check(self.ctx.lib.r3d_tsdf_raycast_rgb(self.handle, cam.handle, n_views, table.ctypes.data, mw, s, tn, tf, d_depth, d_vertex,
                                                      d_normal, d_rgb))
            return
        L.check(self.ctx.lib.r3d_tsdf_raycast(self.handle, cam.handle, n_views, table.ctypes.data, mw, s, tn, tf, d_depth, d_vertex, d_normal))

    def raycast(self, quats_xyzw, ts, shape, intrinsics=REF_INTRINSICS, min_weight=1.0, step=None, t_near=0.0, t_far=math.inf,
                with_colors=False):
        """(depth [F,H,W], vertices [F,H,W,3], normals [F,H,W,3]) float32: what the volume predicts for a camera of `intrinsics`
        and shape = (H, W) at the pose-file rows (quats_xyzw, ts): z-depth, the surface point in the world and the normal towards
        the camera side, from a march along every pixel's ray in steps of `step` (None: voxel_size) between the distances t_near
        and t_far, over the cells whose eight voxels have at least min_weight frames.  A pixel without a surface has depth 0 ("no
        measurement": the raster integrates back as it is) and NaN vertex and normal rows.  step + voxel_size <= sdf_trunc keeps
        both samples that bracket the surface inside the untruncated band.  The hit rows of vertices / normals are a target cloud
        with tgt_normals for icp_point_to_plane.  with_colors (a volume with colour): a fourth array, rgb [F,H,W,3] uint8 R, G, B
        -- the colour image the model predicts: the hit cell's eight mean colours, interpolated like the tsdf; 0, 0, 0 where
        there is no surface (depth 0 marks it), so depth and rgb integrate back together.  Synchronous."""
        if with_colors:
            self._check_color(True, "with_colors")
        try:
            h, w = [int(v) for v in shape]
            exact = all(int(v) == v and not isinstance(v, bool) for v in shape)
        except (TypeError, ValueError):
            raise ValueError("shape must be (H, W), two integers >= 1, got %r" % (shape,))
        if not exact or h < 1 or w < 1:
            raise ValueError("shape must be (H, W), two integers >= 1, got %r" % (shape,))
        mw = _positive_f32(min_weight, "min_weight")
        _ray_range(step, t_near, t_far, self.voxel_size)   # (raycast_device checks again: this raises before anything is allocated)
        table = poses_w2c(quats_xyzw, ts)
        f = table.shape[0]
        if f == 0:
            empty = (np.zeros((0, h, w), np.float32), np.zeros((0, h, w, 3), np.float32), np.zeros((0, h, w, 3), np.float32))
            return empty + (np.zeros((0, h, w, 3), np.uint8),) if with_colors else empty
        cam = self.ctx.camera(h, w, *intrinsics)
        n = f * h * w
        with self.ctx.buffers() as B:
            d_depth, d_vtx, d_nrm = B.alloc(n * 4), B.alloc(n * 12), B.alloc(n * 12)
            d_rgb = B.alloc(n * 3) if with_colors else None
            self.raycast_device(cam, f, table, d_depth.ptr, d_vtx.ptr, d_nrm.ptr, mw, step, t_near, t_far,
                                d_rgb=d_rgb.ptr if with_colors else None)
            out = (d_depth.download_array(np.float32, (f, h, w)), d_vtx.download_array(np.float32, (f, h, w, 3)),
                   d_nrm.download_array(np.float32, (f, h, w, 3)))
            return out + (d_rgb.download_array(np.uint8, (f, h, w, 3)),) if with_colors else out

    def _track_args(self, n_iters, dist_max, max_angle_deg, max_jump, min_weight, step, t_near, t_far):
        """(n_iters, dist_max, cos_min, max_jump, min_weight, step, t_near, t_far) as the library takes them; ValueError otherwise"""
        from .tracking import MAX_ITERS
        if isinstance(n_iters, bool) or int(n_iters) != n_iters or not 0 <= int(n_iters) <= MAX_ITERS:
            raise ValueError("n_iters must be an integer in [0, %d], got %r" % (MAX_ITERS, n_iters))
        dm = _positive_f32(2.0 * self.sdf_trunc if dist_max is None else dist_max, "dist_max")
        if max_angle_deg is None:
            cos_min = -1.0                                    # every angle passes: no source normals are computed
        else:
            try:
                ang = float(max_angle_deg)
            except (TypeError, ValueError):
                raise ValueError("max_angle_deg must be a number in [0, 180) or None, got %r" % (max_angle_deg,))
            if isinstance(max_angle_deg, bool) or not 0.0 <= ang < 180.0:
                raise ValueError("max_angle_deg must be in [0, 180) or None, got %r" % (max_angle_deg,))
            cos_min = min(1.0, max(math.cos(math.radians(ang)), math.nextafter(-1.0, 0.0)))
        try:
            mj = float(max_jump)
        except (TypeError, ValueError):
            raise ValueError("max_jump must be a number >= 0, got %r" % (max_jump,))
        if not mj >= 0.0:
            raise ValueError("max_jump must be >= 0, got %r" % (max_jump,))
        s, tn, tf = _ray_range(step, t_near, t_far, self.voxel_size)
        return int(n_iters), dm, cos_min, mj, _positive_f32(min_weight, "min_weight"), s, tn, tf

    def _check_track_color(self, pyramid_iters, photo_weight, i_max):
        """ValueError unless a colour image can take part in tracking: a volume with colour, no pyramid, a valid weight and gate"""
        self._check_color(True, "rgb")
        if pyramid_iters is not None:
            raise ValueError("rgb cannot be combined with pyramid_iters: the colour term runs at one level only (the pyramid has no "
                             "depth-consistent intensity half-sampler yet)")
        from .tracking import photo_args
        photo_args(photo_weight, i_max)

    def track_device(self, cam, d_depth, depth_dtype, pose_guess_w2c, n_iters=10, dist_max=None, max_angle_deg=None, depth_scale=1.0,
                     max_jump=0.05, min_weight=1.0, step=None, t_near=0.0, t_far=math.inf, pyramid_iters=None, d_rgb=None,
                     photo_weight=None, i_max=None, bilateral=None):
        """track() from a raster in HBM (d_depth: [H][W] of depth_dtype at a raw device address; cam: ctx.camera(...)); d_rgb: the
        frame's colour image, [H][W][3] uint8 at a raw device address, for the colour term.  bilateral: as in track(); d_depth
        itself is only read.  Synchronises (the pose is read back)."""
        if d_rgb is not None:
            self._check_track_color(pyramid_iters, photo_weight, i_max)
        if bilateral is not None:
            from .tracking import bilateral_args
            bilateral = bilateral_args(bilateral)
        levels = None
        if pyramid_iters is not None:
            from .tracking import pyramid_levels
            levels, n_iters = pyramid_levels(pyramid_iters, cam.height, cam.width), 0
        n, dm, cos_min, mj, mw, s, tn, tf = self._track_args(n_iters, dist_max, max_angle_deg, max_jump, min_weight, step, t_near, t_far)
        guess = _pose_rows(np.asarray(pose_guess_w2c, dtype=np.float64).reshape(1, -1), 1)
        if not np.isfinite(guess).all():
            raise ValueError("pose_guess_w2c must be finite")
        pose, info = np.zeros(12, dtype=np.float64), np.zeros(4, dtype=np.float64)
        if bilateral is not None:
            d_depth, depth_dtype, depth_scale = self._bilateral_raster(cam, d_depth, depth_dtype, depth_scale, bilateral), np.float32, 1.0
        if levels is not None:
            from .tracking import pyramid_intrinsics, pyramid_shape
            K = (cam.fx, cam.fy, cam.cx, cam.cy)
            cams = [cam] + [self.ctx.camera(*pyramid_shape(cam.height, cam.width, l), *pyramid_intrinsics(K, l))
                            for l in range(1, len(levels))]
            handles = (C.c_void_p * len(cams))(*[c.handle for c in cams])
            iters = (C.c_int * len(levels))(*levels)
            rms = np.zeros(max(sum(levels), 1), dtype=np.float64)
            L.check(self.ctx.lib.r3d_tsdf_track_pyramid(self.handle, handles, len(cams), iters, d_depth, depth_code(depth_dtype),
                                                        float(depth_scale), guess.ctypes.data, mw, s, tn, tf, mj, dm, cos_min,
                                                        pose.ctypes.data, info.ctypes.data, rms.ctypes.data))
            return pose, {"pairs": float(info[0]), "rms": float(info[1]), "status": int(info[2]), "iterations": int(info[3]),
                          "rms_history": rms[:sum(levels)].tolist()}
        if d_rgb is not None:
            from .tracking import photo_args
            wp, im = photo_args(photo_weight, i_max)
            info = np.zeros(6, dtype=np.float64)
            L.check(self.ctx.lib.r3d_tsdf_track_rgb(self.handle, cam.handle, d_depth, depth_code(depth_dtype), float(depth_scale), d_rgb,
                                                    guess.ctypes.data, mw, s, tn, tf, mj, dm, cos_min, wp, im, n, pose.ctypes.data,
                                                    info.ctypes.data))
            return pose, {"pairs": float(info[0]), "rms": float(info[1]), "status": int(info[2]), "iterations": int(info[3]),
                          "photo_pairs": float(info[4]), "photo_rms": float(info[5])}
        L.check(self.ctx.lib.r3d_tsdf_track(self.handle, cam.handle, d_depth, depth_code(depth_dtype), float(depth_scale),
                                            guess.ctypes.data, mw, s, tn, tf, mj, dm, cos_min, n, pose.ctypes.data, info.ctypes.data))
        return pose, {"pairs": float(info[0]), "rms": float(info[1]), "status": int(info[2]), "iterations": int(info[3])}

    def _bilateral_raster(self, cam, d_depth, depth_dtype, depth_scale, bilateral):
        """The device address of the bilateral-filtered f32 depth raster (metres) of a frame in HBM: the frame is unprojected once
        (its dtype and scale), and the z column of that vertex map is filtered (include/r3d.h "Depth bilateral filter").  Both
        buffers belong to the volume: allocated on first use, reused while the raster size holds.  Asynchronous."""
        n = cam.height * cam.width
        if self._bilateral_bufs is None or self._bilateral_bufs[0] != n:
            self._free_bilateral()
            self._bilateral_bufs = (n, self._bilateral.alloc(n * 12), self._bilateral.alloc(n * 4))
        _, vertex, raster = self._bilateral_bufs
        L.check(self.ctx.lib.r3d_unproject(self.ctx.handle, cam.handle, d_depth, depth_code(depth_dtype), 1, float(depth_scale),
                                           vertex.ptr, L.F32))
        L.check(self.ctx.lib.r3d_depth_bilateral(self.ctx.handle, vertex.ptr + 8, 3, cam.height, cam.width, *bilateral, raster.ptr))
        return raster.ptr

    def _free_bilateral(self):
        if self._bilateral_bufs is not None:
            self.ctx.sync()
            self._bilateral_bufs = None
        self._bilateral.close()

    def track(self, depth, pose_guess_w2c, intrinsics=REF_INTRINSICS, n_iters=10, dist_max=None, max_angle_deg=None, depth_scale=1.0,
              max_jump=0.05, min_weight=1.0, step=None, t_near=0.0, t_far=math.inf, pyramid_iters=None, rgb=None, photo_weight=None,
              i_max=None, bilateral=None):
        """The pose of a new depth raster [H,W] against the model, from a guess (12 doubles, world -> camera: R row-major, t --
        a row of poses_w2c): the volume is ray-cast at the guess, and n_iters iterations of projective point-to-plane ICP move
        the frame onto the predicted vertex and normal map (a source point's partner is the model pixel it projects to).
        Returns (pose [12] float64 in the same layout -- it feeds integrate_device as it is --, info): info["status"] is 0, or 1
        when a step was degenerate (fewer than 6 pairs, or the matched normals leave a freedom open): the pose is then the
        guess.  info also has "pairs" and "rms" (of the plane residual) as the last step saw them, and "iterations".
        dist_max: pairs farther apart never take part (None: 2 x sdf_trunc).  max_angle_deg: pairs whose source and model
        normals differ by more are left out; None: no source normals are computed or gated.  max_jump: the depth-edge rule of
        the source normals (and, with pyramid_iters, of the depth pyramid).  n_iters alone runs at full resolution: small
        motions only.  pyramid_iters: a sequence of iteration counts, fine to coarse, e.g. (10, 5, 4): the loop runs coarse to
        fine over a depth pyramid (every level halves the raster; the model is ray-cast at every level's camera) and follows
        larger motions; n_iters is then not used, and info gains "rms_history", the rms of every step in the order they ran
        (include/r3d.h "Depth pyramid").  rgb (a volume with colour; not with pyramid_iters): the frame's colour image [H,W,3]
        uint8; the loop then carries a photometric term next to the geometric one -- the difference between the frame's
        intensity and that of the colour image the model predicts at the guess -- which holds the freedoms that planes leave
        open (sliding along a corridor, over a wall or a floor), where depth alone ends with status 1.  photo_weight: the weight
        of a photometric pair against a geometric pair's 1, in metres^2 per intensity^2 (None: tracking.PHOTO_WEIGHT); i_max:
        pairs whose intensities differ by more are left out (None: tracking.I_MAX); info gains "photo_pairs" and "photo_rms"
        (include/r3d.h "TSDF colour tracking").  bilateral = (radius, sigma_s, sigma_r): the loop sees a bilateral-filtered copy
        of the frame instead of the frame -- a window of (2 radius + 1)^2 pixels, sigma_s in pixels, sigma_r in metres; depths
        more than 3 sigma_r apart never mix -- which keeps a sensor's depth noise out of the source normals and the residuals
        (include/r3d.h "Depth bilateral filter"); it combines with pyramid_iters and with rgb.  Synchronous."""
        if bilateral is not None:
            from .tracking import bilateral_args
            bilateral_args(bilateral)
        if rgb is not None:
            self._check_track_color(pyramid_iters, photo_weight, i_max)
            img = np.asarray(rgb)
            if img.dtype != np.uint8 or img.shape != np.shape(depth) + (3,):
                raise ValueError("rgb must be a uint8 %s image, got %s of shape %s" % (list(np.shape(depth)) + [3], img.dtype, list(img.shape)))
            img = np.ascontiguousarray(img)
        d = np.asarray(depth)
        if d.ndim != 2 or d.shape[0] < 1 or d.shape[1] < 1:
            raise ValueError("depth must be one [H,W] raster, got shape %s" % (list(d.shape),))
        if d.dtype not in (np.uint8, np.uint16, np.float32):
            raise ValueError("depth must be uint8, uint16 or float32, got %s" % d.dtype)
        d = np.ascontiguousarray(d)
        if pyramid_iters is not None:
            from .tracking import pyramid_levels
            pyramid_levels(pyramid_iters, d.shape[0], d.shape[1])
        self._track_args(0 if pyramid_iters is not None else n_iters, dist_max, max_angle_deg, max_jump, min_weight, step, t_near,
                         t_far)   # raises before anything is allocated
        guess = np.asarray(pose_guess_w2c, dtype=np.float64)
        if guess.size != 12 or not np.isfinite(guess).all():
            raise ValueError("pose_guess_w2c must be 12 finite numbers (R row-major, t), got shape %s" % (list(guess.shape),))
        cam = self.ctx.camera(d.shape[0], d.shape[1], *intrinsics)
        with self.ctx.buffers() as B:
            buf = B.upload(d)
            cbuf = None if rgb is None else B.upload(img)
            return self.track_device(cam, buf.ptr, d.dtype, guess, n_iters, dist_max, max_angle_deg, depth_scale, max_jump, min_weight,
                                     step, t_near, t_far, pyramid_iters, None if cbuf is None else cbuf.ptr, photo_weight, i_max,
                                     bilateral)

    def track_and_integrate(self, depths, first_pose_w2c, intrinsics=REF_INTRINSICS, depth_scale=1.0, rgbs=None, **track_args):
        """Reconstruct from depth rasters [F,H,W] and ONE pose: frame 0 is integrated at first_pose_w2c (12 doubles, world ->
        camera); every later frame is tracked against the model from the previous frame's pose (track(); track_args are its
        keyword arguments, pyramid_iters among them) and integrated at the pose found.  Returns the [F,12] float64 pose rows.
        Raises RuntimeError when a frame cannot be tracked (status 1); the frames before it stay integrated.  rgbs (a volume
        with colour): the frames' colour images [F,H,W,3] uint8; every frame is then tracked with the colour term (track(rgb=);
        photo_weight and i_max among track_args) and integrated with its colour.  Without rgbs: a volume without colour only.
        With bilateral= among track_args every frame is tracked on its filtered copy and integrated RAW."""
        if track_args.get("bilateral") is not None:
            from .tracking import bilateral_args
            bilateral_args(track_args["bilateral"])
        if rgbs is None and self.color:
            raise ValueError("track_and_integrate takes depth rasters only: the volume was created with color=True")
        if rgbs is not None:
            self._check_track_color(track_args.get("pyramid_iters"), track_args.get("photo_weight"), track_args.get("i_max"))
        if np.asarray(depths).dtype not in (np.uint8, np.uint16, np.float32):
            raise ValueError("depths must be uint8, uint16 or float32, got %s" % np.asarray(depths).dtype)
        d = _as_batch(depths)
        f, h, w = d.shape
        img = None if rgbs is None else _rgb_batch(rgbs, d.shape)
        first = np.asarray(first_pose_w2c, dtype=np.float64)
        if first.size != 12 or not np.isfinite(first).all():
            raise ValueError("first_pose_w2c must be 12 finite numbers (R row-major, t), got shape %s" % (list(first.shape),))
        if track_args.get("pyramid_iters") is not None:
            from .tracking import pyramid_levels
            pyramid_levels(track_args["pyramid_iters"], h, w)
        self._track_args(0 if track_args.get("pyramid_iters") is not None else track_args.get("n_iters", 10),
                         track_args.get("dist_max"), track_args.get("max_angle_deg"),
                         track_args.get("max_jump", 0.05), track_args.get("min_weight", 1.0), track_args.get("step"),
                         track_args.get("t_near", 0.0), track_args.get("t_far", math.inf))
        poses = np.zeros((f, 12), dtype=np.float64)
        if f * h * w == 0:
            return poses
        cam = self.ctx.camera(h, w, *intrinsics)
        with self.ctx.buffers() as B:
            buf = B.alloc(d[0].nbytes)
            cbuf = None if img is None else B.alloc(img[0].nbytes)
            for k in range(f):
                buf.upload(d[k])
                if cbuf is not None:
                    cbuf.upload(img[k])
                if k == 0:
                    poses[0] = first.reshape(12)
                else:
                    poses[k], info = self.track_device(cam, buf.ptr, d.dtype, poses[k - 1], depth_scale=depth_scale,
                                                       d_rgb=None if cbuf is None else cbuf.ptr, **track_args)
                    if info["status"] != 0:
                        raise RuntimeError("frame %d cannot be tracked against the model: %d pairs, the step is degenerate"
                                           % (k, int(info["pairs"])))
                self.integrate_device(cam, buf.ptr, d.dtype, 1, poses[k:k + 1], depth_scale, d_rgb=None if cbuf is None else cbuf.ptr)
            self.ctx.sync()
        return poses
