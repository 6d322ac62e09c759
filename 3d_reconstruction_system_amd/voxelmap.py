"""Occupied-voxel set on the MI355X + OctoMap ".bt" export: what the reference does point by point
through the third-party python-octomap binding (octomap/txt_transfer_octomap.py:16-36):

    tree = octomap.OcTree(0.1); tree.updateNode(xyz, True) ...; tree.updateInnerOccupancy(); tree.writeBinary(path)

`OcTree` below offers that same small surface; points are buffered on the host and inserted in bulk by the
HIP hash-set kernel, and the pruned octree is serialised on the device from the set's sorted codes (csrc/r3d_octree.hip): only the
finished records cross PCIe.  `format_bt(codes)` is the host serialiser for codes that are already in host memory (no GPU needed).
"""
import collections
import ctypes as C
import os

import numpy as np

from . import _lib as L
from ._args import colour_words as _colour_words
from .device import default_context


def format_bt(codes_sorted, resolution=0.1):
    """(.bt bytes, node count) for ascending unique 48-bit Morton codes.  Host only (no GPU needed)."""
    codes = np.ascontiguousarray(codes_sorted, dtype=np.uint64)
    lib = L.load()
    n, nodes = C.c_size_t(), C.c_int64()
    L.check(lib.r3d_octree_format_bt(codes.ctypes.data, codes.shape[0], float(resolution), None, 0, C.byref(n),
                                     C.byref(nodes)))
    buf = C.create_string_buffer(max(n.value, 1))
    L.check(lib.r3d_octree_format_bt(codes.ctypes.data, codes.shape[0], float(resolution), buf, n.value, C.byref(n),
                                     C.byref(nodes)))
    return buf.raw[:n.value], nodes.value


class VoxelSet:
    """HBM-resident hash set of occupied voxels (r3d_voxelset)."""

    def __init__(self, resolution=0.1, capacity=1 << 20, ctx=None):
        self.ctx = ctx or default_context()
        self.resolution = float(resolution)
        h = C.c_void_p()
        L.check(self.ctx.lib.r3d_voxelset_create(self.ctx.handle, self.resolution, int(capacity), C.byref(h)))
        self.handle = h.value
        self.ctx.adopt(self)

    def close(self):
        if self.handle:
            self.ctx.lib.r3d_voxelset_destroy(self.handle)
            self.handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def clear(self):
        L.check(self.ctx.lib.r3d_voxelset_clear(self.handle))

    def insert(self, xyz):
        xyz = np.ascontiguousarray(xyz, dtype=np.float32)
        if xyz.ndim != 2 or xyz.shape[1] != 3:
            raise ValueError("cloud must be [N,3]")
        L.check(self.ctx.lib.r3d_voxelset_insert_host(self.handle, xyz.ctypes.data, xyz.shape[0]))

    def insert_device(self, d_xyz, n_points):
        L.check(self.ctx.lib.r3d_voxelset_insert(self.handle, d_xyz, int(n_points)))

    def insert_codes_device(self, d_codes, n_codes):
        L.check(self.ctx.lib.r3d_voxelset_insert_codes(self.handle, d_codes, int(n_codes)))

    def union_across(self, comm):
        """Collective over a comm.Comm: afterwards this set holds the occupied voxels of EVERY rank's set (config 5: frames
        sharded, one map).  Only distinct codes cross the fabric, through the C ABI's all-gather of unequal shards."""
        L.check(self.ctx.lib.r3d_voxelset_union(self.handle, comm.handle))

    def stats(self):
        a, b, c = C.c_int64(), C.c_int64(), C.c_int64()
        L.check(self.ctx.lib.r3d_voxelset_stats(self.handle, C.byref(a), C.byref(b), C.byref(c)))
        return {"voxels": a.value, "ignored_points": b.value, "overflow": c.value}

    def codes(self):
        """Ascending unique Morton codes (uint64) of the occupied voxels."""
        n = C.c_int64()
        L.check(self.ctx.lib.r3d_voxelset_codes(self.handle, None, 0, C.byref(n)))
        out = np.empty(n.value, dtype=np.uint64)
        L.check(self.ctx.lib.r3d_voxelset_codes(self.handle, out.ctypes.data, out.shape[0], C.byref(n)))
        return out

    def format_bt(self):
        """(.bt bytes, node count) of the set, serialised on the device; equal to format_bt(self.codes(), resolution)."""
        lib = self.ctx.lib
        n, nodes = C.c_size_t(), C.c_int64()
        L.check(lib.r3d_voxelset_format_bt(self.handle, None, 0, C.byref(n), C.byref(nodes)))
        buf = C.create_string_buffer(max(n.value, 1))
        L.check(lib.r3d_voxelset_format_bt(self.handle, buf, n.value, C.byref(n), C.byref(nodes)))
        return buf.raw[:n.value], nodes.value

    def write_bt(self, path):
        """The set as an OctoMap .bt file, records streamed from the device into the file; returns the node count."""
        nodes = C.c_int64()
        L.check(self.ctx.lib.r3d_voxelset_write_bt(self.handle, os.fsencode(path), C.byref(nodes)))
        return nodes.value


def octree_records_device(d_codes, n, ctx=None):
    """(uint16 records, node count) of the pruned octree over n ascending unique Morton codes at device pointer d_codes."""
    ctx = ctx or default_context()
    n_rec, nodes = C.c_int64(), C.c_int64()
    L.check(ctx.lib.r3d_octree_records_device(ctx.handle, d_codes, int(n), None, 0, C.byref(n_rec), C.byref(nodes)))
    if n_rec.value == 0:
        return np.zeros(0, np.uint16), nodes.value
    with ctx.buffers() as B:
        d_rec = B.alloc(n_rec.value * 2)
        L.check(ctx.lib.r3d_octree_records_device(ctx.handle, d_codes, int(n), d_rec.ptr, n_rec.value, C.byref(n_rec),
                                                  C.byref(nodes)))
        return d_rec.download(np.uint16, n_rec.value), nodes.value


def _voxelize_set(xyz, resolution=0.1, ctx=None, capacity=None):
    """(VoxelSet holding the voxels hit by an [N,3] cloud, its stats); the table is sized from N (or starts at `capacity`
    slots) and is regrown on overflow."""
    xyz = np.ascontiguousarray(xyz, dtype=np.float32)
    cap = int(capacity) if capacity else max(1 << 16, 2 * xyz.shape[0])
    while True:
        vs = VoxelSet(resolution, cap, ctx)
        try:
            vs.insert(xyz)
            st = vs.stats()
        except Exception:
            vs.close()
            raise
        if st["overflow"] == 0:
            return vs, st
        vs.close()
        cap *= 4


def voxelize(xyz, resolution=0.1, ctx=None):
    """Ascending Morton codes of the voxels hit by an [N,3] cloud; the table is sized from N and regrown on overflow."""
    vs, st = _voxelize_set(xyz, resolution, ctx)
    try:
        return vs.codes(), st
    finally:
        vs.close()


VOXELGRID_RGB = 1

DownSampled = collections.namedtuple("DownSampled", ["xyz", "rgba", "counts", "codes"])
DownSampled.__doc__ = ("One row per occupied voxel in ascending Morton order: centroid xyz [M,3] float32, mean colour rgba [M] "
                       "uint32 (None without colour), point counts [M] uint32, Morton codes [M] uint64.")


def _cloud_f32(xyz):
    xyz = np.ascontiguousarray(xyz, dtype=np.float32)
    if xyz.ndim != 2 or xyz.shape[1] != 3:
        raise ValueError("cloud must be [N,3]")
    return xyz


class VoxelGrid:
    """HBM-resident voxel-grid downsampler (r3d_voxelgrid): insert points (any number of calls), extract one row per occupied
    voxel -- centroid, count, Morton code and, with colour=True, the mean colour word.  The voxels are VoxelSet's; every output
    bit is independent of how the points were split into inserts."""

    def __init__(self, resolution=0.1, capacity=1 << 20, colour=False, ctx=None):
        if not float(resolution) > 0.0:
            raise ValueError("resolution must be positive")
        if int(capacity) < 0:
            raise ValueError("capacity must be >= 0")
        self.handle = None
        self.ctx = ctx or default_context()
        self.resolution = float(resolution)
        self.colour = bool(colour)
        h = C.c_void_p()
        L.check(self.ctx.lib.r3d_voxelgrid_create(self.ctx.handle, self.resolution, int(capacity),
                                                  VOXELGRID_RGB if self.colour else 0, C.byref(h)))
        self.handle = h.value
        self.ctx.adopt(self)

    def close(self):
        if self.handle:
            self.ctx.lib.r3d_voxelgrid_destroy(self.handle)
            self.handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def clear(self):
        L.check(self.ctx.lib.r3d_voxelgrid_clear(self.handle))

    def _check_colour(self, given):
        if given and not self.colour:
            raise ValueError("rgba given to a VoxelGrid made without colour")
        if self.colour and not given:
            raise ValueError("a VoxelGrid made with colour=True needs rgba for every point")

    def insert(self, xyz, rgba=None):
        """Host arrays: xyz [N,3] (float32; other float types are converted), rgba [N] uint32 or None."""
        xyz = _cloud_f32(xyz)
        self._check_colour(rgba is not None)
        rgba = None if rgba is None else _colour_words(rgba, xyz.shape[0])
        L.check(self.ctx.lib.r3d_voxelgrid_insert_host(self.handle, xyz.ctypes.data, None if rgba is None else rgba.ctypes.data,
                                                       xyz.shape[0]))

    def insert_device(self, d_xyz, n, d_rgba=None):
        """Device pointers (ints): n float32 xyz rows and, for a colour grid, n uint32 colour words; asynchronous."""
        self._check_colour(d_rgba is not None)
        L.check(self.ctx.lib.r3d_voxelgrid_insert(self.handle, d_xyz, d_rgba, int(n)))

    def stats(self):
        a, b, c = C.c_int64(), C.c_int64(), C.c_int64()
        L.check(self.ctx.lib.r3d_voxelgrid_stats(self.handle, C.byref(a), C.byref(b), C.byref(c)))
        return {"voxels": a.value, "ignored_points": b.value, "overflow": c.value}

    def extract_device(self, d_xyz_out=None, d_rgba_out=None, d_count_out=None, d_codes_out=None, cap=0):
        """Rows into caller device buffers (pointers or None) of `cap` rows each; returns the number of voxels.  All None:
        only the count."""
        n = C.c_int64()
        L.check(self.ctx.lib.r3d_voxelgrid_extract(self.handle, d_xyz_out, d_rgba_out, d_count_out, d_codes_out, int(cap),
                                                   C.byref(n)))
        return n.value

    def extract(self):
        """DownSampled(xyz [M,3] float32, rgba [M] uint32 | None, counts [M] uint32, codes [M] uint64) on the host."""
        m = self.extract_device()
        if m == 0:
            return DownSampled(np.zeros((0, 3), np.float32), np.zeros(0, np.uint32) if self.colour else None,
                               np.zeros(0, np.uint32), np.zeros(0, np.uint64))
        with self.ctx.buffers() as B:
            d_xyz, d_cnt, d_codes = B.alloc(m * 12), B.alloc(m * 4), B.alloc(m * 8)
            d_rgba = B.alloc(m * 4) if self.colour else None
            self.extract_device(d_xyz.ptr, d_rgba.ptr if d_rgba else None, d_cnt.ptr, d_codes.ptr, m)
            return DownSampled(d_xyz.download_array(np.float32, (m, 3)), d_rgba.download(np.uint32, m) if d_rgba else None,
                               d_cnt.download(np.uint32, m), d_codes.download(np.uint64, m))


def voxel_down_sample(xyz, voxel_size, rgba=None, ctx=None):
    """One-shot voxel-grid downsampling of a host cloud: DownSampled rows, one per occupied voxel (ascending Morton code).
    The table is sized from N (2 slots per point), so it cannot overflow.  Points without a voxel key (non-finite, outside
    +-32768 voxels) are ignored."""
    xyz = _cloud_f32(xyz)
    if not float(voxel_size) > 0.0:
        raise ValueError("voxel_size must be positive")
    rgba = None if rgba is None else _colour_words(rgba, xyz.shape[0])
    vg = VoxelGrid(voxel_size, max(1 << 10, 2 * xyz.shape[0]), rgba is not None, ctx)
    try:
        vg.insert(xyz, rgba)
        return vg.extract()
    finally:
        vg.close()


class OcTree:
    """The slice of python-octomap's OcTree the reference scripts use."""

    initial_capacity = None   # table slots of the first attempt (None: sized from the number of points)

    def __init__(self, resolution):
        self.resolution = float(resolution)
        self._pending = []
        self._blocks = []
        self._set = None      # the device set of everything inserted so far (None: stale or empty)
        self._stats = None

    def _stale(self):
        if self._set is not None:
            self._set.close()
            self._set = None
        self._stats = None

    def updateNode(self, point, occupied=True):
        if not occupied:
            raise NotImplementedError("the reference only inserts hits (updateNode(point, True))")
        self._pending.append((float(point[0]), float(point[1]), float(point[2])))
        self._stale()

    def insertPointCloud(self, xyz):
        self._blocks.append(np.ascontiguousarray(xyz, dtype=np.float32).reshape(-1, 3))
        self._stale()

    def _flush(self):
        """The VoxelSet of the points inserted so far, kept on the device for size() / writeBinary(); None without points."""
        if self._stats is None:
            blocks = list(self._blocks)
            if self._pending:
                blocks.append(np.array(self._pending, dtype=np.float64).astype(np.float32))
            pts = np.concatenate(blocks) if blocks else np.zeros((0, 3), np.float32)
            if pts.shape[0]:
                self._set, self._stats = _voxelize_set(pts, self.resolution, capacity=self.initial_capacity)
            else:
                self._stats = {"voxels": 0, "ignored_points": 0, "overflow": 0}
        return self._set

    def updateInnerOccupancy(self):
        self._flush()

    def size(self):
        vs = self._flush()
        return vs.format_bt()[1] if vs is not None else 0

    def writeBinary(self, filename):
        if isinstance(filename, bytes):
            filename = filename.decode("utf-8")
        vs = self._flush()
        if vs is not None:
            vs.write_bt(filename)
        else:   # nothing inserted: the header of an empty tree (no device needed)
            with open(filename, "wb") as f:
                f.write(format_bt(np.zeros(0, np.uint64), self.resolution)[0])
        return True

    def __del__(self):
        try:
            self._stale()
        except Exception:
            pass
