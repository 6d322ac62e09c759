"""MI355X: the device octree serialiser (csrc/r3d_octree.hip) against the host serialiser r3d_octree_format_bt and, where the
size allows the Python oracle, against oracle/octomap_ref.write_bt_bytes.  Every comparison is exact: bytes and node counts."""
import ctypes as C
import importlib
import os
import re

import numpy as np
import pytest

from helpers import PKG, ROOT
from helpers import r3d as _r3d
from oracle import octomap_ref as OM

pytestmark = pytest.mark.gpu

G = 1 << 16
ORACLE_MAX = 60000
INVALID, NOMEM = -1, -3


def _tile():
    src = open(os.path.join(ROOT, PKG, "csrc", "r3d_octree.hip")).read()
    return int(re.search(r"constexpr int kOctreeTile = (\d+);", src).group(1))


TILE = _tile()


@pytest.fixture(scope="module")
def R():
    return _r3d()


@pytest.fixture(scope="module")
def L(R):
    return importlib.import_module(PKG + "._lib")


@pytest.fixture(scope="module")
def V(R):
    return importlib.import_module(PKG + ".voxelmap")


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
        assert self.buf.ptr % 256 == 0
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

    def unchanged(self):
        assert np.array_equal(self.bytes(), self.pattern[G + self.off:G + self.off + self.nbytes]), "payload was written"

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


def device_bt(V, L, ctx, codes, res=0.1):
    """(.bt bytes, nodes) through r3d_octree_records_device + r3d_octree_bt_header."""
    codes = np.ascontiguousarray(codes, dtype=np.uint64)
    d = ctx.alloc(max(codes.nbytes, 16))
    try:
        if codes.size:
            d.upload(codes)
        rec, nodes = V.octree_records_device(d.ptr, codes.size, ctx)
    finally:
        d.free()
    buf, n = C.create_string_buffer(256), C.c_size_t()
    L.check(ctx.lib.r3d_octree_bt_header(nodes, res, buf, 256, C.byref(n)))
    return buf.raw[:n.value] + rec.astype("<u2").tobytes(), nodes


def check_codes(V, L, ctx, codes, res=0.1):
    codes = np.ascontiguousarray(codes, dtype=np.uint64)
    assert codes.size < 2 or np.all(codes[1:] > codes[:-1])
    got, nodes = device_bt(V, L, ctx, codes, res)
    want, want_nodes = V.format_bt(codes, res)
    assert nodes == want_nodes and got == want
    if codes.size <= ORACLE_MAX:
        ref, ref_nodes = OM.write_bt_bytes(codes, res)
        assert nodes == ref_nodes and got == ref
    return got, nodes


@pytest.mark.parametrize("seed,n,spread", [(0, 1, 1.0), (1, 200, 0.3), (2, 5000, 2.0), (3, 60000, 6.0), (4, 30000, 0.5)])
def test_matches_host_and_oracle_on_clouds(V, L, ctx, seed, n, spread):
    rng = np.random.default_rng(seed)
    pts = (rng.normal(size=(n, 3)) * spread).astype(np.float32)
    codes, _ = OM.occupied_set(pts)
    check_codes(V, L, ctx, codes)


def test_single_voxel_and_empty(V, L, ctx):
    codes, _ = OM.occupied_set(np.array([[0.05, 0.05, 0.05]], np.float32))
    got, nodes = check_codes(V, L, ctx, codes)
    assert nodes == 17 and got.endswith(b"\x00\xc0" + b"\x03\x00" * 14 + b"\x02\x00")
    got, nodes = check_codes(V, L, ctx, np.zeros(0, np.uint64))
    assert nodes == 0 and got.endswith(b"size 0\nres 0.1\ndata\n")
    n_rec, n_nodes = C.c_int64(7), C.c_int64(7)
    L.check(ctx.lib.r3d_octree_records_device(ctx.handle, None, 0, None, 0, C.byref(n_rec), C.byref(n_nodes)))
    assert (n_rec.value, n_nodes.value) == (0, 0)


@pytest.mark.parametrize("size", [8, 64, 512, 4096, 8 ** 6])
def test_full_blocks_prune_and_one_missing_code_does_not(V, L, ctx, size):
    depth = 16 - round(np.log(size) / np.log(8))
    a = np.arange(size, dtype=np.uint64) + np.uint64(size * 5) + (np.uint64(3) << np.uint64(45))
    got, nodes = check_codes(V, L, ctx, a)
    assert nodes == depth + 1                                        # root + inner chain + ONE leaf
    for cut in (0, size // 2, size - 1):
        check_codes(V, L, ctx, np.delete(a, cut))
    check_codes(V, L, ctx, np.arange(2 * size, dtype=np.uint64) + np.uint64(size * 6))      # two adjacent full octants
    check_codes(V, L, ctx, np.arange(size, dtype=np.uint64) + np.uint64(size * 5 + size // 8 + 1))   # full count, not aligned
    check_codes(V, L, ctx, np.concatenate([a[:1] - np.uint64(9), a, a[-1:] + np.uint64(2)]))        # neighbours on both sides


def test_extreme_and_neighbouring_codes(V, L, ctx):
    check_codes(V, L, ctx, [0, 2 ** 48 - 1])
    check_codes(V, L, ctx, [0])
    check_codes(V, L, ctx, [2 ** 48 - 1])
    check_codes(V, L, ctx, [3, 3 + (1 << 45)])        # differ only in the top digit
    check_codes(V, L, ctx, [8, 9])                    # differ only in the bottom digit
    check_codes(V, L, ctx, list(range(8, 16)) + [17, 2 ** 47 + 3])


def test_dense_block_with_and_without_holes(V, L, ctx):
    rng = np.random.default_rng(5)
    k = np.stack(np.meshgrid(*[np.arange(32760, 32790)] * 3, indexing="ij"), -1).reshape(-1, 3)
    check_codes(V, L, ctx, np.sort(OM.morton(k)))
    check_codes(V, L, ctx, np.sort(OM.morton(k[rng.random(len(k)) < 0.97])))


@pytest.mark.parametrize("n", sorted({1, 2, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, TILE - 1, TILE, TILE + 1, 2 * TILE - 1, 2 * TILE,
                                      2 * TILE + 1, 3 * TILE + 17}))
@pytest.mark.parametrize("kind", ["sparse", "dense"])
def test_every_tile_boundary(V, L, ctx, n, kind):
    rng = np.random.default_rng(n)
    if kind == "sparse":
        codes = np.unique(rng.integers(0, 2 ** 48, size=2 * n + 8, dtype=np.uint64))[:n]
    else:   # runs of consecutive codes: full octants straddle the tile and wave boundaries
        codes = np.arange(n, dtype=np.uint64) + np.uint64(8 ** 5 * 3 + 5)
    assert codes.size == n
    check_codes(V, L, ctx, codes)


def _records(ctx, L, d_codes, n, d_out, cap):
    n_rec, nodes = C.c_int64(-1), C.c_int64(-1)
    rc = ctx.lib.r3d_octree_records_device(ctx.handle, d_codes, n, d_out, cap, C.byref(n_rec), C.byref(nodes))
    return rc, n_rec.value, nodes.value


@pytest.mark.parametrize("odd", [0, 1])
def test_guard_bands_and_offsets(V, L, ctx, guard, odd):
    rng = np.random.default_rng(11 + odd)
    codes = np.unique(np.concatenate([rng.integers(0, 2 ** 48, size=3000, dtype=np.uint64),
                                      np.arange(700, dtype=np.uint64) + np.uint64(8 ** 7)]))
    want, want_nodes = V.format_bt(codes)
    body = want[want.index(b"data\n") + 5:]
    if (len(body) // 2) % 2 != odd:        # one more lone voxel under a fresh top-level branch changes the parity or not: try a few
        for extra in range(1, 40):
            c2 = np.unique(np.append(codes, np.uint64(2 ** 48 - extra)))
            w2 = V.format_bt(c2)[0]
            if (len(w2[w2.index(b"data\n") + 5:]) // 2) % 2 == odd:
                codes = c2
                break
        want, want_nodes = V.format_bt(codes)
        body = want[want.index(b"data\n") + 5:]
    n_rec = len(body) // 2
    assert n_rec % 2 == odd
    payloads = []
    for out_off, in_off in ((0, 0), (2, 0), (0, 8), (2, 8)):
        g_in = guard(codes.nbytes, in_off, codes, seed=1)
        g_out = guard(n_rec * 2, out_off, seed=2)
        assert g_out.ptr % 4 == out_off and g_in.ptr % 16 == in_off
        rc, r, nodes = _records(ctx, L, g_in.ptr, codes.size, g_out.ptr, n_rec)
        assert rc == 0 and (r, nodes) == (n_rec, want_nodes)
        payloads.append(g_out.bytes().tobytes())
        g_in.unchanged()
    assert all(p == body for p in payloads)


def test_refusals_write_nothing(V, L, ctx, guard):
    rng = np.random.default_rng(3)
    good = np.unique(rng.integers(0, 2 ** 48, size=9000, dtype=np.uint64))
    rc0, n_rec, _ = _records(ctx, L, guard(good.nbytes, 0, good).ptr, good.size, None, 0)
    want = V.format_bt(good)[0]
    assert rc0 == 0 and n_rec == (len(want) - want.index(b"data\n") - 5) // 2

    def refused(codes, cap, needle):
        g_in = guard(codes.nbytes, 0, codes, seed=4)
        g_out = guard(n_rec * 2 + 64, 2, seed=5)
        rc, _, _ = _records(ctx, L, g_in.ptr, codes.size, g_out.ptr, cap)
        assert rc == INVALID and needle in L.last_error(), (rc, L.last_error())
        g_out.unchanged()
        g_in.unchanged()

    refused(good, n_rec - 1, "records")
    dup = good.copy()
    dup[5000] = dup[4999]
    refused(dup, n_rec + 32, "strictly ascending Morton codes (violated at index 5000)")
    desc = good.copy()
    desc[[4096, 4095]] = desc[[4095, 4096]]
    refused(desc, n_rec + 32, "(violated at index 4096)")
    big = good.copy()
    big[-1] = np.uint64(2 ** 48)
    refused(big, n_rec + 32, "Morton code above 48 bits")
    # output inside the input: refused, the input (which is the output) keeps its bytes
    g = guard(good.nbytes, 0, good, seed=6)
    rc, _, _ = _records(ctx, L, g.ptr, good.size, g.ptr + 64, n_rec)
    assert rc == INVALID and "overlap" in L.last_error()
    g.unchanged()
    # the host serialiser words the same refusals the same way
    with pytest.raises(Exception, match=r"violated at index 5000"):
        V.format_bt(dup)


def test_same_bytes_on_every_run_and_context(R, V, L, ctx):
    rng = np.random.default_rng(8)
    pts = (rng.normal(size=(300000, 3)) * 3.0).astype(np.float32)
    codes = V.voxelize(pts, 0.1, ctx)[0]
    a = device_bt(V, L, ctx, codes)
    b = device_bt(V, L, ctx, codes)
    other = R.Context(0)
    try:
        c = device_bt(V, L, other, codes)
    finally:
        other.close()
    assert a == b == c == V.format_bt(codes)


def test_voxelset_format_and_write(V, L, ctx, tmp_path):
    rng = np.random.default_rng(9)
    pts = (rng.normal(size=(20000, 3)) * 2.0).astype(np.float32)
    vs = V.VoxelSet(0.25, 1 << 17, ctx)
    try:
        vs.insert(pts)
        want = OM.write_bt_bytes(OM.occupied_set(pts, 0.25)[0], 0.25)
        assert vs.format_bt() == want == V.format_bt(vs.codes(), 0.25)
        p = tmp_path / "set.bt"
        assert vs.write_bt(str(p)) == want[1] and p.read_bytes() == want[0]
        vs.clear()
        assert vs.format_bt() == OM.write_bt_bytes(np.zeros(0, np.uint64), 0.25)
        p2 = tmp_path / "empty.bt"
        assert vs.write_bt(str(p2)) == 0 and p2.read_bytes() == OM.write_bt_bytes(np.zeros(0, np.uint64), 0.25)[0]
    finally:
        vs.close()


def test_overflowed_set_writes_no_file(V, L, ctx, tmp_path):
    rng = np.random.default_rng(10)
    pts = (rng.normal(size=(50000, 3)) * 5.0).astype(np.float32)
    vs = V.VoxelSet(0.1, 1 << 10, ctx)
    try:
        vs.insert(pts)
        assert vs.stats()["overflow"] > 0
        p = tmp_path / "never.bt"
        with pytest.raises(L.R3DError) as e:
            vs.write_bt(str(p))
        assert e.value.code == NOMEM and "overflowed" in str(e.value) and not p.exists()
        with pytest.raises(L.R3DError) as e:
            vs.format_bt()
        assert e.value.code == NOMEM
        with pytest.raises(L.R3DError) as e2:
            vs.codes()
        assert str(e2.value) == str(e.value)
    finally:
        vs.close()


def test_octree_drop_in_uses_the_device_path(V, tmp_path):
    rng = np.random.default_rng(12)
    pts = (rng.normal(size=(20000, 3)) * 1.5).astype(np.float32)
    want, want_nodes = OM.write_bt_bytes(OM.occupied_set(pts)[0])
    tree = V.OcTree(0.1)
    tree.insertPointCloud(pts[:15000])
    for p in pts[15000:]:
        tree.updateNode(p, True)
    tree.updateInnerOccupancy()
    assert tree.size() == want_nodes
    assert tree.writeBinary(str(tmp_path / "a.bt")) and (tmp_path / "a.bt").read_bytes() == want
    assert tree._set is not None                                    # the set stays on the device between size() and writeBinary()
    tree.updateNode((100.0, 100.0, 100.0), True)                    # ... until the tree changes
    assert tree.size() == OM.write_bt_bytes(OM.occupied_set(np.vstack([pts, [[100.0, 100.0, 100.0]]]).astype(np.float32))[0])[1]
    small = V.OcTree(0.1)
    small.initial_capacity = 1 << 10                                # overflows (20 000 points): regrown until everything fits
    small.insertPointCloud(pts)
    assert small.writeBinary(os.fsencode(str(tmp_path / "b.bt"))) and (tmp_path / "b.bt").read_bytes() == want
    assert small._stats["overflow"] == 0 and small._stats["voxels"] == len(OM.occupied_set(pts)[0])
    empty = V.OcTree(0.1)
    assert empty.size() == 0 and empty.writeBinary(str(tmp_path / "c.bt"))
    assert (tmp_path / "c.bt").read_bytes() == OM.write_bt_bytes(np.zeros(0, np.uint64))[0]


def _host_file(ctx, L, vs, path, res):
    codes = vs.codes()
    nodes = C.c_int64()
    L.check(ctx.lib.r3d_octree_write_bt(os.fsencode(path), codes.ctypes.data, codes.shape[0], C.c_double(res), C.byref(nodes)))
    return codes.shape[0], nodes.value


def _same_file(a, b):
    if os.path.getsize(a) != os.path.getsize(b):
        return False
    with open(a, "rb") as fa, open(b, "rb") as fb:
        while True:
            x, y = fa.read(1 << 24), fb.read(1 << 24)
            if x != y:
                return False
            if not x:
                return True


def test_surface_scan_file_equals_host_chain(R, V, L, ctx, tmp_path):
    """C5-like frames (wavy surfaces, random poses) through the one-launch fuse + voxel insert, >= 5 M voxels."""
    F, H, W, U, res = 32, 1080, 1920, 8, 0.02
    per, n = H * W, 32 * 1080 * 1920
    rng = np.random.default_rng(555)
    jj, ii = np.mgrid[0:H, 0:W]
    depth = np.stack([8.0 + 3.0 * np.sin(ii / (90.0 + 7 * k)) * np.cos(jj / (70.0 + 5 * k)) + 0.02 * rng.random((H, W))
                      for k in range(U)]).astype(np.float32)
    table = R.pose_table(rng.normal(size=(F, 4)), rng.normal(size=(F, 3)) * 10)
    cam = ctx.camera(H, W, 960.0, 960.0, 959.5, 539.5)
    d_depth, d_pose, d_xyz = ctx.alloc(n * 4), ctx.alloc(table.nbytes).upload(table), ctx.alloc(n * 12)
    vs = V.VoxelSet(res, 1 << 26, ctx)
    try:
        d_depth.upload(depth)
        for k in range(1, F // U):
            L.check(ctx.lib.r3d_memcpy_d2d(ctx.handle, d_depth.ptr + k * U * per * 4, d_depth.ptr, U * per * 4))
        R.fuse_frames_voxel_device(ctx, cam, d_depth.ptr, np.float32, F, d_pose.ptr, None, d_xyz.ptr, None, vs)
        a, b = str(tmp_path / "dev.bt"), str(tmp_path / "host.bt")
        nodes = vs.write_bt(a)
        n_codes, host_nodes = _host_file(ctx, L, vs, b, res)
        print("surface scan: %d voxels, %d nodes, %d bytes" % (n_codes, nodes, os.path.getsize(a)))
        assert n_codes >= 5_000_000 and vs.stats()["overflow"] == 0
        assert nodes == host_nodes and _same_file(a, b)
    finally:
        vs.close()
        for d in (d_depth, d_pose, d_xyz):
            d.free()


def test_c2_worst_case_file_equals_host_chain(R, V, L, ctx, tmp_path):
    """tools/voxel_export_once.py's cloud: 100 frames of 384 x 1280 random depths under random poses, ~1 voxel per point."""
    frames, H, W = 100, 384, 1280
    rng = np.random.default_rng(1234)
    depth = rng.integers(1, 256, (frames, H, W), dtype=np.uint8)
    q, t = rng.normal(size=(frames, 4)), rng.normal(size=(frames, 3)) * 10
    n = frames * H * W
    table = R.pose_table(q, t)
    cam = ctx.camera(H, W, *R.REF_INTRINSICS)
    d_depth, d_pose, d_xyz = ctx.alloc(depth.nbytes).upload(depth), ctx.alloc(table.nbytes).upload(table), ctx.alloc(n * 12)
    vs = V.VoxelSet(0.1, 1 << 27, ctx)
    try:
        R.fuse_frames_device(ctx, cam, d_depth.ptr, np.uint8, frames, d_pose.ptr, d_xyz.ptr, np.float32)
        vs.insert_device(d_xyz.ptr, n)
        a, b = str(tmp_path / "dev.bt"), str(tmp_path / "host.bt")
        nodes = vs.write_bt(a)
        n_codes, host_nodes = _host_file(ctx, L, vs, b, 0.1)
        print("C2 worst case: %d voxels, %d nodes, %d bytes" % (n_codes, nodes, os.path.getsize(a)))
        assert n_codes >= 40_000_000 and vs.stats()["overflow"] == 0
        assert nodes == host_nodes and _same_file(a, b)
    finally:
        vs.close()
        for d in (d_depth, d_pose, d_xyz):
            d.free()
