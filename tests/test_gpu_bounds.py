"""GPU: stray stores, pointer offsets and aliasing at the device entry points of the C ABI.

Every buffer handed to a kernel here lives inside a GUARDED allocation (`Guarded`): one ctx.alloc of G + offset + payload + G
bytes, G = 1 MiB (more than 40 tiles of the widest kernel: a fused f64 tile is 1024 px x 24 B), filled with a seeded random
byte pattern.  The entry point sees base + G + offset.  After the call the whole allocation comes back and both bands must
still hold the pattern bit for bit -- a store one tile too far lands in a band instead of in allocator slack.  The offsets
are the ones a C consumer or a torch view with a storage offset may legally pass: naturally aligned for the element type,
not 16-byte aligned, so every "is the pointer aligned" predicate of the fused launch takes its other side.

Each case asserts (a) the guards are intact, (b) the payload equals the oracle at the existing tolerance, (c) the payload is
bit-identical to the same call with every buffer at offset 0 after its band (ctx.alloc's 256-byte alignment).  The numpy
*_host wrappers are never used: their device buffers are the library's exact-size scratch, which no band covers.

Over-reads are not probed: no buffer sits flush against the end of its allocation, so every access a kernel could make by
mistake stays inside memory this file owns.
"""
import ctypes as C
import importlib

import numpy as np
import pytest

from helpers import PKG, r3d as _r3d
from oracle import fusion_ref as O
from oracle import octomap_ref as OM
from oracle import plane_ref as OP
from test_gpu_fusion import check, make_depth
from test_gpu_icp import assert_nn_valid

pytestmark = pytest.mark.gpu

G = 1 << 20

# tile sizes of the kernels under test (csrc): r3d_fuse.hip / r3d_apply.hip / r3d_nnindex.hip kTile, r3d_textfmt.hip kTile,
# r3d_sort_dev.h kTile
FUSE_TILE = APPLY_TILE = NN_TILE = 1024
TEXT_TILE = 256
SORT_TILE = 4096


def tile_sizes(t):
    return [1, t - 1, t, t + 1, 3 * t + 17]


RASTERS = [(1, 1, 1), (1, 1, 1023), (1, 1, 1025), (1, 32, 32), (3, 37, 53), (2, 33, 1024)]


@pytest.fixture(scope="module")
def R():
    return _r3d()


@pytest.fixture(scope="module")
def L(R):
    return importlib.import_module(PKG + "._lib")


@pytest.fixture(scope="module")
def D(R):
    return importlib.import_module(PKG + ".device")


@pytest.fixture(scope="module")
def ctx(R):
    c = R.Context(0)
    yield c
    c.close()


class Guarded:
    """G + off + nbytes + G bytes of device memory in one allocation, every byte a seeded random pattern; `ptr` is the
    payload's address (base + G + off).  data != None: the payload holds those bytes instead."""

    def __init__(self, ctx, nbytes, off=0, data=None, seed=0):
        self.ctx, self.nbytes, self.off = ctx, int(nbytes), int(off)
        self.total = 2 * G + self.off + self.nbytes
        rng = np.random.default_rng([seed, self.nbytes, self.off])
        self.pattern = np.frombuffer(rng.bytes(self.total), dtype=np.uint8).copy()
        if data is not None:
            raw = np.ascontiguousarray(data).reshape(-1).view(np.uint8)
            assert raw.size == self.nbytes, (raw.size, self.nbytes)
            self.pattern[G + self.off:G + self.off + self.nbytes] = raw
        self.buf = ctx.alloc(self.total).upload(self.pattern)
        self.ptr = self.buf.ptr + G + self.off

    def bytes(self):
        """Synchronises the ctx, asserts both bands are untouched, returns a copy of the payload bytes."""
        self.ctx.sync()
        raw = self.buf.download(np.uint8, self.total)
        lo, hi = G + self.off, G + self.off + self.nbytes
        bad = np.flatnonzero(raw[:lo] != self.pattern[:lo])
        assert bad.size == 0, "%d bytes written in front of the payload, nearest at payload - %d" % (bad.size, lo - bad[-1])
        bad = np.flatnonzero(raw[hi:] != self.pattern[hi:])
        assert bad.size == 0, "%d bytes written behind the payload, first at payload end + %d" % (bad.size, bad[0])
        return raw[lo:hi].copy()

    def read(self, dtype, shape=(-1,)):
        return self.bytes().view(dtype).reshape(shape)

    def unchanged(self):
        """An input: the whole allocation, payload included, is as it was uploaded."""
        assert np.array_equal(self.bytes(), self.pattern[G + self.off:G + self.off + self.nbytes]), "input payload was written"

    def free(self):
        self.buf.free()


@pytest.fixture
def guard(ctx):
    made = []

    def make(nbytes, off=0, data=None, seed=0):
        g = Guarded(ctx, nbytes, off, data, seed)
        made.append(g)
        return g
    yield make
    for g in made:
        g.free()


def _rgba_words(rgb):
    r = rgb.reshape(-1, 3).astype(np.uint32)
    return r[:, 0] | (r[:, 1] << 8) | (r[:, 2] << 16)


def _pose(rng, frames):
    return rng.normal(size=(frames, 4)), rng.normal(size=(frames, 3)) * 10


# ---- r3d_unproject / r3d_fuse_frames -----------------------------------------------------------------------------------
DEPTH_CASES = [(np.uint8, 1), (np.uint8, 2), (np.uint8, 3), (np.uint16, 2), (np.float32, 4), (np.float32, 12)]
XYZ_OUT_CASES = [(np.float32, 4), (np.float32, 12), (np.float64, 8)]


@pytest.mark.parametrize("shape", RASTERS)
@pytest.mark.parametrize("ddtype,doff", DEPTH_CASES)
def test_unproject_and_fuse_at_offsets(R, L, D, ctx, guard, shape, ddtype, doff):
    """Depth rasters at byte offsets that switch off the dword raster loads; xyz outputs at offsets that are not 16-byte
    aligned; one workgroup per tile (fuse_blocks 0) and a 3-workgroup grid-stride walk."""
    F, H, W = shape
    n = F * H * W
    rng = np.random.default_rng([F, H, W, doff, np.dtype(ddtype).itemsize])
    d = make_depth(rng, shape, ddtype)
    q, t = _pose(rng, F)
    tab = R.pose_table(q, t)
    cam = ctx.camera(H, W, *R.REF_INTRINSICS)
    want = {"fuse": O.fuse_frames(d, q, t), "unproject": np.concatenate([O.unproject(f) for f in d])}
    dc = D.depth_code(ddtype)

    def run(which, d_depth, d_pose, odt, ooff):
        out = guard(n * 3 * np.dtype(odt).itemsize, ooff, seed=1)
        if which == "fuse":
            L.check(ctx.lib.r3d_fuse_frames(ctx.handle, cam.handle, d_depth.ptr, dc, F, 1.0, d_pose.ptr, out.ptr, D.xyz_code(odt)))
        else:
            L.check(ctx.lib.r3d_unproject(ctx.handle, cam.handle, d_depth.ptr, dc, F, 1.0, out.ptr, D.xyz_code(odt)))
        return out.read(odt, (n, 3))

    dep0, pose0 = guard(d.nbytes, 0, d), guard(tab.nbytes, 0, tab)
    dep, pose = guard(d.nbytes, doff, d, seed=2), guard(tab.nbytes, 8, tab, seed=2)
    try:
        for odt in (np.float32, np.float64):
            for which in ("fuse", "unproject"):
                ctx.set_tuning("fuse_blocks", 0)
                ref = run(which, dep0, pose0, odt, 0)
                check(ref, want[which], odt)
                for ooff in [o for dt, o in XYZ_OUT_CASES if dt == odt]:
                    for blocks in (0, 3):
                        ctx.set_tuning("fuse_blocks", blocks)
                        np.testing.assert_array_equal(run(which, dep, pose, odt, ooff), ref)
    finally:
        ctx.set_tuning("fuse_blocks", 0)
    for b in (dep0, pose0, dep, pose):
        b.unchanged()


# ---- r3d_fuse_frames_rgb ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", RASTERS)
@pytest.mark.parametrize("rgb_off", [1, 3, 8])
def test_fuse_rgb_at_offsets(R, L, D, ctx, guard, shape, rgb_off):
    """The colour plane at offsets that switch off the 16-byte LDS-staged colour loads, xyz AND rgba guarded: f32 xyz (colour
    carried by the fused kernel) and f64 xyz (rgb_expand_kernel after it), with a pose table and without one."""
    F, H, W = shape
    n = F * H * W
    rng = np.random.default_rng([F, H, W, rgb_off])
    d = make_depth(rng, shape, np.uint8)
    rgb = rng.integers(0, 256, size=shape + (3,), dtype=np.uint8)
    q, t = _pose(rng, F)
    tab = R.pose_table(q, t)
    cam = ctx.camera(H, W, *R.REF_INTRINSICS)
    want_rgba = _rgba_words(rgb)
    want = {True: O.fuse_frames(d, q, t), False: np.concatenate([O.unproject(f) for f in d])}

    def run(d_depth, d_pose, d_rgb, odt, ooff, with_pose):
        xyz = guard(n * 3 * np.dtype(odt).itemsize, ooff, seed=1)
        rgba = guard(n * 4, 4 if ooff else 0, seed=3)
        L.check(ctx.lib.r3d_fuse_frames_rgb(ctx.handle, cam.handle, d_depth.ptr, R.DEPTH_U8, F, 1.0,
                                            d_pose.ptr if with_pose else None, d_rgb.ptr, xyz.ptr, D.xyz_code(odt), rgba.ptr))
        return xyz.read(odt, (n, 3)), rgba.read(np.uint32)

    dep0, pose0, rgb0 = guard(d.nbytes, 0, d), guard(tab.nbytes, 0, tab), guard(rgb.nbytes, 0, rgb)
    dep, pose, rgbo = guard(d.nbytes, 3, d, seed=2), guard(tab.nbytes, 8, tab, seed=2), guard(rgb.nbytes, rgb_off, rgb, seed=2)
    for odt, ooff in ((np.float32, 4), (np.float64, 8)):
        for with_pose in (True, False):
            ref_xyz, ref_rgba = run(dep0, pose0, rgb0, odt, 0, with_pose)
            check(ref_xyz, want[with_pose], odt)
            np.testing.assert_array_equal(ref_rgba, want_rgba)
            xyz, rgba = run(dep, pose, rgbo, odt, ooff, with_pose)
            np.testing.assert_array_equal(xyz, ref_xyz)
            np.testing.assert_array_equal(rgba, ref_rgba)
    for b in (dep0, pose0, rgb0, dep, pose, rgbo):
        b.unchanged()


# ---- r3d_fuse_frames_voxel ----------------------------------------------------------------------------------------------
VOXEL_CASES = [(s, np.uint8, False) for s in RASTERS] + [((150, 37, 53), np.float32, True)]


@pytest.mark.parametrize("shape,ddtype,chunked", VOXEL_CASES)
def test_fuse_voxel_at_offsets(R, L, D, ctx, guard, shape, ddtype, chunked):
    """The one-launch cloud + map at offsets, xyz and rgba guarded; the set equals the oracle's set of the cloud.  The chunked
    case stages its inputs in 1 MB steps (fuse_prefetch 2, fuse_chunk_mb 1): 76 frames of 1961 pixels per step, so the second
    step's raster, colour, xyz and rgba pointers start at an odd pixel."""
    V = importlib.import_module(PKG + ".voxelmap")
    F, H, W = shape
    n = F * H * W
    rng = np.random.default_rng([F, H, W])
    d = make_depth(rng, shape, ddtype)
    rgb = rng.integers(0, 256, size=shape + (3,), dtype=np.uint8)
    q, t = _pose(rng, F)
    tab = R.pose_table(q, t)
    cam = ctx.camera(H, W, *R.REF_INTRINSICS)
    want = O.fuse_frames(d, q, t)
    doff = 4 if ddtype == np.float32 else 1

    def run(d_depth, d_pose, d_rgb, ooff):
        xyz, rgba = guard(n * 12, ooff, seed=1), guard(n * 4, ooff, seed=3)
        vs = V.VoxelSet(0.1, 1 << max(16, (2 * n).bit_length()), ctx)      # >= 2 slots per point: no overflow
        try:
            L.check(ctx.lib.r3d_fuse_frames_voxel(ctx.handle, cam.handle, d_depth.ptr, D.depth_code(ddtype), F, 1.0, d_pose.ptr,
                                                  d_rgb.ptr, xyz.ptr, rgba.ptr, vs.handle))
            cloud, words = xyz.read(np.float32, (n, 3)), rgba.read(np.uint32)
            codes, st = vs.codes(), vs.stats()
        finally:
            vs.close()
        want_codes, dropped = OM.occupied_set(cloud, 0.1)
        np.testing.assert_array_equal(codes, want_codes)
        assert st["ignored_points"] == dropped and st["overflow"] == 0
        return cloud, words

    dep0, pose0, rgb0 = guard(d.nbytes, 0, d), guard(tab.nbytes, 0, tab), guard(rgb.nbytes, 0, rgb)
    dep, pose, rgbo = guard(d.nbytes, doff, d, seed=2), guard(tab.nbytes, 8, tab, seed=2), guard(rgb.nbytes, 3, rgb, seed=2)
    try:
        if chunked:
            ctx.set_tuning("fuse_prefetch", 2)
            ctx.set_tuning("fuse_chunk_mb", 1)
        ref_xyz, ref_rgba = run(dep0, pose0, rgb0, 0)
        check(ref_xyz, want, np.float32)
        np.testing.assert_array_equal(ref_rgba, _rgba_words(rgb))
        xyz, rgba = run(dep, pose, rgbo, 4)
        np.testing.assert_array_equal(xyz, ref_xyz)
        np.testing.assert_array_equal(rgba, ref_rgba)
    finally:
        ctx.set_tuning("fuse_prefetch", 0)
        ctx.set_tuning("fuse_chunk_mb", 0)
    for b in (dep0, pose0, rgb0, dep, pose, rgbo):
        b.unchanged()


# ---- r3d_se3_apply / r3d_apply_T ----------------------------------------------------------------------------------------
XYZ_OFFSETS = {np.float32: (4, 12), np.float64: (8,)}
DTYPE_PAIRS = [(np.float32, np.float32), (np.float64, np.float64), (np.float32, np.float64), (np.float64, np.float32)]


def _transforms(R, rng):
    T = np.eye(4)
    T[:3, :3] = 1.7 * np.asarray(R.scipy_transfer(rng.normal(size=4)))
    T[:3, 3] = rng.normal(size=3) * 5
    rinv = np.asarray(R.scipy_transfer(rng.normal(size=4)))
    t = rng.normal(size=3) * 10
    pose = np.concatenate([rinv.reshape(9), t])
    return T, rinv, t, pose


def _apply(ctx, L, which, d_in, idt, n, M, d_out, odt):
    fn = ctx.lib.r3d_apply_T if which == "T" else ctx.lib.r3d_se3_apply
    return fn(ctx.handle, d_in, L.F32 if idt == np.float32 else L.F64, n, M.ctypes.data, d_out, L.F32 if odt == np.float32 else L.F64)


@pytest.mark.parametrize("n", tile_sizes(APPLY_TILE))
@pytest.mark.parametrize("idt,odt", DTYPE_PAIRS)
def test_apply_at_offsets(R, L, ctx, guard, n, idt, odt):
    rng = np.random.default_rng([n, np.dtype(idt).itemsize, np.dtype(odt).itemsize])
    p = (rng.normal(size=(n, 3)) * 50).astype(idt)
    T, rinv, t, pose = _transforms(R, rng)
    want = {"T": O.apply_T(p, T), "se3": O.se3_apply(p, rinv, t)}
    mats = {"T": np.ascontiguousarray(T), "se3": pose}
    obytes = n * 3 * np.dtype(odt).itemsize
    src0 = guard(p.nbytes, 0, p)
    try:
        for which in ("T", "se3"):
            ctx.set_tuning("apply_blocks", 0)
            out0 = guard(obytes, 0, seed=1)
            L.check(_apply(ctx, L, which, src0.ptr, idt, n, mats[which], out0.ptr, odt))
            ref = out0.read(odt, (n, 3))
            check(ref, want[which], odt)
            for ioff in XYZ_OFFSETS[idt]:
                src = guard(p.nbytes, ioff, p, seed=2)
                for ooff in XYZ_OFFSETS[odt]:
                    for blocks in (0, 3):
                        ctx.set_tuning("apply_blocks", blocks)
                        out = guard(obytes, ooff, seed=3)
                        L.check(_apply(ctx, L, which, src.ptr, idt, n, mats[which], out.ptr, odt))
                        np.testing.assert_array_equal(out.read(odt, (n, 3)), ref)
                src.unchanged()
    finally:
        ctx.set_tuning("apply_blocks", 0)
    src0.unchanged()


# ---- aliasing -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", tile_sizes(APPLY_TILE))
@pytest.mark.parametrize("dt", [np.float32, np.float64])
def test_apply_in_place_is_bitwise_the_out_of_place_call(R, L, ctx, guard, n, dt):
    """r3d.h promises in-place r3d_se3_apply / r3d_apply_T (the ICP loops move their source cloud that way, r3d_apply_T_dev
    with the step in HBM): same bits as out of place, for one tile per workgroup and a grid-stride walk."""
    rng = np.random.default_rng([n, np.dtype(dt).itemsize, 7])
    p = (rng.normal(size=(n, 3)) * 50).astype(dt)
    T, rinv, t, pose = _transforms(R, rng)
    mats = {"T": np.ascontiguousarray(T), "se3": pose}
    off = XYZ_OFFSETS[dt][-1]
    src = guard(p.nbytes, 0, p)
    d_T = guard(T.nbytes, 8, T, seed=4)
    try:
        for which in ("T", "se3"):
            ctx.set_tuning("apply_blocks", 0)
            out = guard(p.nbytes, off, seed=1)
            L.check(_apply(ctx, L, which, src.ptr, dt, n, mats[which], out.ptr, dt))
            ref = out.read(dt, (n, 3))
            for blocks in (0, 3):
                ctx.set_tuning("apply_blocks", blocks)
                buf = guard(p.nbytes, off, p, seed=2)
                L.check(_apply(ctx, L, which, buf.ptr, dt, n, mats[which], buf.ptr, dt))
                np.testing.assert_array_equal(buf.read(dt, (n, 3)), ref)
                if which == "T":
                    buf = guard(p.nbytes, off, p, seed=3)
                    code = L.F32 if dt == np.float32 else L.F64
                    L.check(ctx.lib.r3d_apply_T_dev(ctx.handle, buf.ptr, code, n, d_T.ptr, buf.ptr, code))
                    np.testing.assert_array_equal(buf.read(dt, (n, 3)), ref)
    finally:
        ctx.set_tuning("apply_blocks", 0)
    src.unchanged()
    d_T.unchanged()


@pytest.mark.parametrize("n", [1, APPLY_TILE + 1])
def test_apply_refuses_in_place_with_unequal_dtypes(R, L, ctx, guard, n):
    rng = np.random.default_rng(n)
    p64 = rng.normal(size=(n, 3)) * 50
    T = np.eye(4)
    pose = np.concatenate([np.eye(3).reshape(9), np.ones(3)])
    buf = guard(p64.nbytes, 8, p64)
    for which, M in (("T", T), ("se3", pose)):
        for idt, odt in ((np.float64, np.float32), (np.float32, np.float64)):
            assert _apply(ctx, L, which, buf.ptr, idt, n, M, buf.ptr, odt) == L.ERR_INVALID
            assert "dtype" in L.last_error()
    buf.unchanged()


@pytest.mark.parametrize("n", [1, 3, APPLY_TILE + 1])
@pytest.mark.parametrize("idt,odt", DTYPE_PAIRS)
def test_apply_refuses_partial_overlap(R, L, ctx, guard, n, idt, odt):
    """d_out one point (12 B) behind or in front of d_in, and any other overlap short of equality: R3D_ERR_INVALID, nothing
    written -- the tile-parallel kernel would make the result depend on workgroup timing.  Ranges that merely touch are two
    separate clouds and are served."""
    rng = np.random.default_rng([n, 11])
    p = (rng.normal(size=(n, 3)) * 50).astype(idt)
    T, rinv, t, pose = _transforms(R, rng)
    ib, ob = p.nbytes, n * 3 * np.dtype(odt).itemsize
    room = guard(ob + ib + ob + 32, 8, seed=5)
    lead = ob + 8
    base = room.ptr + lead                                   # the input; an output may start anywhere from base - ob on
    clash = [s for s in (-12, 12, 4 - ob, ib - 4, 4) if s != 0 and -ob < s < ib]
    L.check(ctx.lib.r3d_memcpy_h2d(ctx.handle, base, p.ctypes.data, ib))
    before = room.bytes()
    for which, M in (("T", np.ascontiguousarray(T)), ("se3", pose)):
        for s in clash:
            assert _apply(ctx, L, which, base, idt, n, M, base + s, odt) == L.ERR_INVALID, (which, s)
            assert "overlap" in L.last_error()
        np.testing.assert_array_equal(room.bytes(), before)
    # ranges that touch are two clouds: out right behind in, and right in front of it
    for s in (ib, -ob):
        L.check(_apply(ctx, L, "T", base, idt, n, np.ascontiguousarray(T), base + s, odt))
        got = room.bytes()[lead + s:lead + s + ob].view(odt).reshape(n, 3)
        check(got, O.apply_T(p, T), odt)
        np.testing.assert_array_equal(room.bytes()[lead:lead + ib], before[lead:lead + ib])


# ---- r3d_format_text_device ---------------------------------------------------------------------------------------------
def _host_rows(R, kind, xyz, aux):
    T = R.device_text
    if kind == T.TEXT_XYZ_TXT:
        return R.cloud_io.format_xyz_txt(xyz, aux)
    if kind == T.TEXT_PLY_ROWS:
        body = R.cloud_io.format_ply(xyz).split(b"end_header\n    ", 1)[1]
        return body[:-5]
    rgb = aux.reshape(len(xyz), -1)[:, :3]
    return O.format_ply_rgb(xyz, rgb).split("end_header\n    ", 1)[1][:-5].encode()


TEXT_CASES = [("xyz_txt", np.float32, "u8"), ("xyz_txt", np.float64, None), ("xyz_txt", np.float64, "u16"),
              ("ply_rows", np.float32, None), ("ply_rows", np.float64, None), ("ply_rgb", np.float32, 3), ("ply_rgb", np.float64, 4)]


@pytest.mark.parametrize("n", tile_sizes(TEXT_TILE))
@pytest.mark.parametrize("kind,dt,aux", TEXT_CASES)
def test_format_text_device_at_offsets(R, L, D, ctx, guard, n, kind, dt, aux):
    """The text goes to d_text + 1 / + 13 with text_cap == n_bytes exactly: the tile's first and last 16 bytes are byte
    stores shared with its neighbours, so a wrong end shows as a hit on a band."""
    T = R.device_text
    code = {"xyz_txt": T.TEXT_XYZ_TXT, "ply_rows": T.TEXT_PLY_ROWS, "ply_rgb": T.TEXT_PLY_ROWS_RGB}[kind]
    rng = np.random.default_rng([n, len(kind), np.dtype(dt).itemsize])
    xyz = (rng.normal(size=(n, 3)) * 10.0 ** rng.integers(-3, 5, size=(n, 1))).astype(dt)
    a_arr, a_code, a_off = None, 0, 0
    if aux == "u8":
        a_arr, a_code, a_off = rng.integers(0, 256, n, dtype=np.uint8), L.DEPTH_U8, 1
    elif aux == "u16":
        a_arr, a_code, a_off = rng.integers(0, 65536, n, dtype=np.uint16), L.DEPTH_U16, 2
    elif aux in (3, 4):
        a_arr, a_code, a_off = rng.integers(0, 256, (n, aux), dtype=np.uint8), aux, 1 if aux == 3 else 4
    want = _host_rows(R, code, xyz, a_arr)
    xoff = 4 if dt == np.float32 else 8
    x0, xo = guard(xyz.nbytes, 0, xyz), guard(xyz.nbytes, xoff, xyz, seed=2)
    a0 = guard(a_arr.nbytes, 0, a_arr) if a_arr is not None else None
    ao = guard(a_arr.nbytes, a_off, a_arr, seed=2) if a_arr is not None else None

    def run(d_xyz, d_aux, seg, toff):
        n_seg = 1 if seg <= 0 else -(-n // seg)
        offs = np.zeros(n_seg + 1, np.int64)
        total = C.c_int64(0)
        L.check(ctx.lib.r3d_format_text_device(ctx.handle, code, d_xyz.ptr, D.xyz_code(dt), n, d_aux.ptr if d_aux else None,
                                               a_code, seg, None, 0, offs.ctypes.data, C.byref(total)))
        assert total.value == len(want)
        text = guard(total.value, toff, seed=3)
        offs2 = np.zeros_like(offs)
        L.check(ctx.lib.r3d_format_text_device(ctx.handle, code, d_xyz.ptr, D.xyz_code(dt), n, d_aux.ptr if d_aux else None,
                                               a_code, seg, text.ptr, total.value, offs2.ctypes.data, C.byref(total)))
        np.testing.assert_array_equal(offs2, offs)
        return text.bytes().tobytes(), offs

    for seg in (0, 255, 256, 257):
        ref, ref_offs = run(x0, a0, seg, 0)
        assert ref == want
        rows = want.split(b"\n")[:-1]
        cuts = np.cumsum([0] + [len(r) + 1 for r in rows])
        step = n if seg <= 0 else seg
        np.testing.assert_array_equal(ref_offs, cuts[list(range(0, n, step)) + [n]])
        for toff in (1, 13):
            got, offs = run(xo, ao, seg, toff)
            assert got == ref
            np.testing.assert_array_equal(offs, ref_offs)
    for b in (x0, xo, a0, ao):
        if b is not None:
            b.unchanged()


# ---- r3d_sort_u64 -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [0, 1] + tile_sizes(SORT_TILE)[1:])
@pytest.mark.parametrize("bits", [20, 48, 64])
@pytest.mark.parametrize("keys_kind", ["random", "equal", "sorted"])
def test_sort_u64_in_place_at_offset(R, L, ctx, guard, n, bits, keys_kind):
    """Keys at +8 inside a guarded buffer, sorted in place.  Only the sort's odd digit passes scatter into the caller's buffer
    (the even ones write the library's scratch, r3d_sort.hip, which no band covers); with an odd number of passes the result is
    copied back.  So the bands see the caller-side scatter and the final copy, not every pass."""
    rng = np.random.default_rng([n, bits, len(keys_kind)])
    keys = rng.integers(0, 2 ** 63, size=n, dtype=np.uint64) * 2 + rng.integers(0, 2, size=n, dtype=np.uint64)
    if bits < 64:
        keys &= np.uint64((1 << bits) - 1)
    if keys_kind == "equal":
        keys[:] = keys[0] if n else 0
    elif keys_kind == "sorted":
        keys = np.sort(keys)
    want = np.sort(keys, kind="stable")
    outs = []
    for off in (0, 8):
        buf = guard(keys.nbytes, off, keys, seed=off)
        L.check(ctx.lib.r3d_sort_u64(ctx.handle, buf.ptr, n, bits))
        outs.append(buf.read(np.uint64))
    np.testing.assert_array_equal(outs[0], want)
    np.testing.assert_array_equal(outs[1], outs[0])


# ---- r3d_nn_index_query / r3d_icp_nn / r3d_nn_index_sort_cloud -----------------------------------------------------------
def _nn_index(ctx, L, d_tgt, n_tgt):
    h = C.c_void_p()
    L.check(ctx.lib.r3d_nn_index_create(ctx.handle, d_tgt.ptr, n_tgt, C.byref(h)))
    return h.value


@pytest.mark.parametrize("n_src", tile_sizes(NN_TILE))
def test_nn_at_offsets(R, L, ctx, guard, n_src):
    """Sources at +12, idx and d2 at +4: brute force and the culled index (presorted 0 and 1) against the oracle
    (test_gpu_icp.assert_nn_valid: its 1-ulp allowance for the oracle's emulated fma).  The warm
    start (nn_warm) is off: it reads the previous matches of a buffer at the same address as bounds."""
    rng = np.random.default_rng([n_src, 3])
    n_tgt = 2 * NN_TILE + 5
    tgt = (rng.normal(size=(n_tgt, 3)) * 4).astype(np.float32)
    src = (rng.normal(size=(n_src, 3)) * 4).astype(np.float32)
    t0 = guard(tgt.nbytes, 12, tgt)
    ix = None
    try:
        ctx.set_tuning("nn_warm", 1)
        ix = _nn_index(ctx, L, t0, n_tgt)
        refs = {}
        for soff, ooff in ((0, 0), (12, 4)):
            s = guard(src.nbytes, soff, src, seed=soff)
            for how in ("brute", "index0", "index1"):
                idx, d2 = guard(n_src * 4, ooff, seed=1), guard(n_src * 4, ooff, seed=2)
                if how == "brute":
                    L.check(ctx.lib.r3d_icp_nn(ctx.handle, s.ptr, n_src, t0.ptr, n_tgt, idx.ptr, d2.ptr))
                else:
                    L.check(ctx.lib.r3d_nn_index_query(ix, s.ptr, n_src, idx.ptr, d2.ptr, 1 if how == "index1" else 0, None))
                got = (idx.read(np.uint32), d2.read(np.float32))
                if soff == 0:
                    assert_nn_valid(src, tgt, *got)
                    refs[how] = got
                else:
                    np.testing.assert_array_equal(got[0], refs[how][0])
                    np.testing.assert_array_equal(got[1].view(np.uint32), refs[how][1].view(np.uint32))
            s.unchanged()
    finally:
        if ix:
            ctx.lib.r3d_nn_index_destroy(ix)
        ctx.set_tuning("nn_warm", 0)
    t0.unchanged()


@pytest.mark.parametrize("n", tile_sizes(NN_TILE))
def test_nn_sort_cloud_in_place_at_offset(R, L, ctx, guard, n):
    rng = np.random.default_rng([n, 5])
    tgt = (rng.normal(size=(3000, 3)) * 4).astype(np.float32)
    cloud = (rng.normal(size=(n, 3)) * 4).astype(np.float32)
    t0 = guard(tgt.nbytes, 0, tgt)
    ix = _nn_index(ctx, L, t0, tgt.shape[0])
    try:
        outs = []
        for coff, poff in ((0, 0), (12, 4)):
            c = guard(cloud.nbytes, coff, cloud, seed=coff)
            perm = guard(n * 4, poff, seed=1)
            L.check(ctx.lib.r3d_nn_index_sort_cloud(ix, c.ptr, n, perm.ptr))
            got, pm = c.read(np.float32, (n, 3)), perm.read(np.uint32)
            np.testing.assert_array_equal(np.sort(pm), np.arange(n, dtype=np.uint32))
            np.testing.assert_array_equal(got, cloud[pm])
            outs.append((got, pm))
        np.testing.assert_array_equal(outs[1][0], outs[0][0])
        np.testing.assert_array_equal(outs[1][1], outs[0][1])
    finally:
        ctx.lib.r3d_nn_index_destroy(ix)
    t0.unchanged()


# ---- r3d_normals_organized ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", RASTERS)
def test_normals_at_offset(R, L, ctx, guard, shape):
    F, H, W = shape
    n = F * H * W
    rng = np.random.default_rng([F, H, W, 9])
    jj, ii = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    depth = [(5.0 + 0.01 * ii + 0.02 * jj + 0.3 * f + rng.random((H, W)) * 0.002).astype(np.float32) for f in range(F)]
    xyz = np.concatenate([O.unproject(dp) for dp in depth]).astype(np.float32)
    want = OP.organized_normals(xyz, H, W)
    outs = []
    for off in (0, 12):
        src = guard(xyz.nbytes, off, xyz, seed=off)
        out = guard(xyz.nbytes, off, seed=1)
        L.check(ctx.lib.r3d_normals_organized(ctx.handle, src.ptr, F, H, W, C.c_float(0.05), None, out.ptr))
        outs.append(out.read(np.float32, (n, 3)))
        src.unchanged()
    np.testing.assert_array_equal(outs[0].view(np.uint32), want.view(np.uint32))
    np.testing.assert_array_equal(outs[1].view(np.uint32), outs[0].view(np.uint32))


# ---- r3d_backproject_depth_f32 / _grad, r3d_project3d_f32 / _grad ----------------------------------------------------------
def _close(got, want, tol):
    err = np.abs(got.astype(np.float64) - want) / (1.0 + np.abs(want))
    assert err.max() <= tol, err.max()


@pytest.mark.parametrize("shape", [(1, 4, 6), (2, 33, 37)])
def test_backproject_and_project3d_at_offsets(R, L, ctx, guard, shape):
    """Every input at +4, every output guarded at +4 (the float2 pixel plane at +8), d_grad_P included; fp64 numpy statements
    of the r3d.h formulas, tolerances of the torch-op tests (fp32 arithmetic, forward 1e-5 (1 + |ref|), the per-pixel gradients
    1e-5 of the largest, the per-image d_grad_P sums 2e-4 of the largest)."""
    B, H, W = shape
    hw = H * W
    eps = np.float32(1e-7)
    rng = np.random.default_rng([B, H, W])
    depth = (rng.random((B, hw)) * 80 + 0.1).astype(np.float32)
    K = np.tile(np.eye(4), (B, 1, 1))
    K[:, 0, 0], K[:, 1, 1], K[:, 0, 2], K[:, 1, 2], K[:, 0, 1] = 0.58 * W, 1.92 * H, 0.5 * W, 0.5 * H, 0.004
    inv_K = np.linalg.inv(K).astype(np.float32)
    gcam = rng.normal(size=(B, 4, hw)).astype(np.float32)
    pts = np.concatenate([rng.random((B, 2, hw)) - 0.5, rng.random((B, 1, hw)) + 1.0, np.ones((B, 1, hw))], 1).astype(np.float32)
    P = (K[:, :3, :] + rng.normal(size=(B, 3, 4)) * 0.01).astype(np.float32)
    gpix = rng.normal(size=(B, H, W, 2)).astype(np.float32)

    ys, xs = np.divmod(np.arange(hw), W)
    k64 = inv_K.astype(np.float64)
    rays = np.stack([k64[:, c, 0:1] * xs + k64[:, c, 1:2] * ys + k64[:, c, 2:3] for c in range(3)], 1)     # [B][3][hw]
    want_cam = np.concatenate([depth[:, None, :] * rays, np.ones((B, 1, hw))], 1)
    want_gdepth = (gcam[:, :3].astype(np.float64) * rays).sum(1)
    P64, x64 = P.astype(np.float64), pts.astype(np.float64)
    c = np.einsum("bck,bkp->bcp", P64, x64)
    z = c[:, 2] + float(eps)
    want_pix = np.stack([(c[:, 0] / z / (W - 1) - 0.5) * 2, (c[:, 1] / z / (H - 1) - 0.5) * 2], -1).reshape(B, H, W, 2)
    gx, gy = gpix.reshape(B, hw, 2)[..., 0].astype(np.float64), gpix.reshape(B, hw, 2)[..., 1].astype(np.float64)
    gc = np.stack([2 * gx / ((W - 1) * z), 2 * gy / ((H - 1) * z),
                   -2 * gx * c[:, 0] / ((W - 1) * z * z) - 2 * gy * c[:, 1] / ((H - 1) * z * z)], 1)              # [B][3][hw]
    want_gpts = np.einsum("bck,bcp->bkp", P64, gc)
    want_gP = np.einsum("bcp,bkp->bck", gc, x64)

    results = []
    for off in (0, 4):
        s = off // 4 + 1
        ins = [guard(a.nbytes, off, a, seed=s) for a in (depth, inv_K, gcam, pts, P, gpix)]
        d_depth, d_invK, d_gcam, d_pts, d_P, d_gpix = ins
        cam, gdep = guard(B * 4 * hw * 4, off, seed=10), guard(B * hw * 4, off, seed=11)
        pix, gpts, gP = guard(B * hw * 8, 2 * off, seed=12), guard(B * 4 * hw * 4, off, seed=13), guard(B * 12 * 4, off, seed=14)
        L.check(ctx.lib.r3d_backproject_depth_f32(ctx.handle, d_depth.ptr, d_invK.ptr, B, H, W, cam.ptr))
        L.check(ctx.lib.r3d_backproject_depth_grad_f32(ctx.handle, d_gcam.ptr, d_invK.ptr, B, H, W, gdep.ptr))
        L.check(ctx.lib.r3d_project3d_f32(ctx.handle, d_pts.ptr, d_P.ptr, B, H, W, C.c_float(eps), pix.ptr))
        L.check(ctx.lib.r3d_project3d_grad_f32(ctx.handle, d_gpix.ptr, d_pts.ptr, d_P.ptr, B, H, W, C.c_float(eps), gpts.ptr,
                                                gP.ptr))
        got = [cam.read(np.float32, (B, 4, hw)), gdep.read(np.float32, (B, hw)), pix.read(np.float32, (B, H, W, 2)),
               gpts.read(np.float32, (B, 4, hw)), gP.read(np.float32, (B, 3, 4))]
        for b in ins:
            b.unchanged()
        results.append(got)
    g_cam, g_gdep, g_pix, g_gpts, g_gP = results[0]
    _close(g_cam, want_cam, 1e-5)
    assert np.abs(g_gdep - want_gdepth).max() <= 1e-5 * np.abs(want_gdepth).max()
    _close(g_pix, want_pix, 1e-5)
    assert np.abs(g_gpts - want_gpts).max() <= 1e-5 * np.abs(want_gpts).max()
    assert np.abs(g_gP - want_gP).max() <= 2e-4 * np.abs(want_gP).max()
    for a, b in zip(results[1], results[0]):
        np.testing.assert_array_equal(a.view(np.uint32), b.view(np.uint32))
