"""GPU: coloured ICP (r3d_color_gradient_knn, r3d_icp_color_accumulate, r3d_icp_iterate_color; colored_icp.py;
registration.register_colored; other_tools/colored_icp.py) against tests/color_icp_ref.py, the NumPy restatement of include/r3d.h.

Intensity, gradient, count and (float) rI are compared bit for bit (a NaN is compared as "is NaN"); the 31 sums at the rtol 1e-11
tests/test_gpu_track_color.py uses for its 31 sums, the two counts exactly; the device loop against the restatement loop at the
atol 2e-6 the tracking tests use for a device loop against its reference loop."""
import importlib
import os
import subprocess
import sys

import numpy as np
import pytest

import color_icp_ref as REF
from helpers import PKG, ROOT, r3d as _r3d
from test_gpu_bounds import Guarded

pytestmark = pytest.mark.gpu

F = np.float32
KS = (3, 8, 32)
NAN_BITS = np.uint32(0x7fc00000)


@pytest.fixture(scope="module")
def R():
    return _r3d()


@pytest.fixture(scope="module")
def L(R):
    return importlib.import_module(PKG + "._lib")


@pytest.fixture(scope="module")
def icp(R):
    return importlib.import_module(PKG + ".icp")


@pytest.fixture(scope="module")
def CI(R):
    return importlib.import_module(PKG + ".colored_icp")


@pytest.fixture(scope="module")
def ctx(R):
    c = R.Context(0)
    yield c
    c.close()


@pytest.fixture
def guard(ctx):
    made = []

    def make(nbytes, off=0, data=None, seed=0):
        made.append(Guarded(ctx, nbytes, off, data, seed))
        return made[-1]
    yield make
    for g in made:
        g.free()


def nan_bits(a):
    """f32 bit patterns with every NaN folded onto one"""
    a = np.ascontiguousarray(a, F)
    return np.where(np.isnan(a), NAN_BITS, a.view(np.uint32))


def assert_sums(got, want):
    np.testing.assert_allclose(got, want, rtol=1e-11, atol=1e-11 * max(np.abs(want).max(), 1e-300))
    assert got[0] == want[0] and got[29] == want[29], (got[0], want[0], got[29], want[29])


def garbage_alpha(rgba, seed):
    a = np.random.default_rng(seed).integers(0, 256, rgba.shape[0], dtype=np.uint32)
    return ((rgba & np.uint32(0xffffff)) | (a << 24)).astype(np.uint32)


def planar(n, seed, offset=0.0):
    """n jittered points near the plane z = 0.3 x + offset with its normal and a smooth colour"""
    rng = np.random.default_rng(seed)
    xy = rng.random((n, 2)) * max(1.0, np.sqrt(n) * 0.05)
    xyz = np.stack([xy[:, 0] + offset, xy[:, 1] + offset, 0.3 * xy[:, 0] + offset + rng.normal(0, 1e-3, n)], axis=1).astype(F)
    nrm = np.tile((np.array([-0.3, 0.0, 1.0]) / np.sqrt(1.09)).astype(F), (n, 1))
    rgba = garbage_alpha(REF.words(REF.wall_colour(xy[:, 0] * 0.3, xy[:, 1] * 0.3)), seed)
    return xyz, nrm, rgba


def make_clouds():
    out = {}
    sc = REF.wall_scene()
    out["wall"] = (sc["tgt"], sc["normals"], garbage_alpha(sc["tgt_rgba"], 1), 0.05)
    g = np.stack(np.meshgrid(*[np.arange(6)] * 3, indexing="ij"), -1).reshape(-1, 3).astype(F)
    axes = np.eye(3, dtype=F)[np.arange(216) % 3] * F(1 - 2 * ((np.arange(216) // 3) % 2))[:, None]
    rng = np.random.default_rng(5)
    out["lattice"] = (g, axes, rng.integers(0, 1 << 32, 216, dtype=np.uint64).astype(np.uint32), 1.5)
    out["offset1e4"] = planar(500, 6, 1e4) + (0.08,)
    xyz, nrm, rgba = planar(300, 7)
    xyz[100:200] = xyz[:100]                                            # exact duplicates, colours differ
    out["duplicates"] = (xyz, nrm, rgba, 0.07)
    xyz, nrm, rgba = planar(400, 8)
    xyz[rng.choice(400, 20, replace=False), rng.integers(0, 3, 20)] = np.nan
    xyz[rng.choice(400, 10, replace=False), rng.integers(0, 3, 10)] = np.inf
    xyz[7, 2] = -np.inf
    nrm = nrm.copy()
    nrm[rng.choice(400, 15, replace=False)] = 0
    nrm[rng.choice(400, 15, replace=False), rng.integers(0, 3, 15)] = np.nan
    nrm[3, 0] = np.inf
    out["nonfinite"] = (xyz, nrm, rgba, 0.06)
    for n in (1, 2, 4, 255, 257):
        out["n%d" % n] = planar(n, 20 + n) + (0.1,)
    s = F(7.97e-4)                                                      # the conditioning floor from both sides (test_color_icp_host)
    for name, v in (("floor_below", s), ("floor_above", F(1e-3))):
        out[name] = (F([[0, 0, 0], [v, 0, 0], [0, v, 0], [-v, 0, 0]]), np.tile(F([0, 0, 1]), (4, 1)),
                     REF.words(np.array([[100] * 3, [110] * 3, [90] * 3, [95] * 3], np.uint8)), None)
    return out


CLOUDS = None


def clouds():
    global CLOUDS
    if CLOUDS is None:
        CLOUDS = make_clouds()
    return CLOUDS


CLOUD_NAMES = ("wall", "lattice", "offset1e4", "duplicates", "nonfinite", "n1", "n2", "n4", "n255", "n257", "floor_below", "floor_above")


def device_gradient(ctx, L, icp, guard, xyz, nrm, rgba, k, radius, off):
    n = xyz.shape[0]
    g_xyz, g_n, g_w = guard(xyz.nbytes, 0, xyz), guard(nrm.nbytes, 0, nrm), guard(rgba.nbytes, 0, rgba)
    ix = icp.NNIndex(ctx, g_xyz.ptr, n)
    try:
        o_i, o_g, o_c = guard(n * 4, off, seed=1), guard(n * 12, off, seed=2), guard(n * 4, off, seed=3)
        got = []
        for _ in range(2):
            L.check(ctx.lib.r3d_color_gradient_knn(ix.handle, k, 0.0 if radius is None else radius, g_n.ptr, g_w.ptr, o_i.ptr, o_g.ptr,
                                                   o_c.ptr))
            got.append((o_i.read(F).copy(), o_g.read(F, (n, 3)).copy(), o_c.read(np.uint32).copy()))
        for g in (g_xyz, g_n, g_w):
            g.unchanged()
        for a, b in zip(got[0], got[1]):
            assert a.tobytes() == b.tobytes(), "a repeat gave other bits"
        return got[0]
    finally:
        ix.close()


@pytest.mark.parametrize("name", CLOUD_NAMES)
def test_gradient_bit_for_bit(ctx, L, icp, guard, name):
    xyz, nrm, rgba, radius = clouds()[name]
    n = xyz.shape[0]
    case = 0
    for k in KS:
        idx, d2 = REF.knn_lists(xyz, k)
        for rad in (None, radius):
            if rad is None and radius is not None and k == 32 and n > 1000:
                continue                                                 # the wall at k = 32 once, with its radius
            want_I, want_g, want_c = REF.gradients(xyz, nrm, rgba, idx, d2, radius=rad)
            got_I, got_g, got_c = device_gradient(ctx, L, icp, guard, xyz, nrm, rgba, k, rad, (0, 4)[case % 2])
            case += 1
            assert np.array_equal(got_c, want_c), (name, k, rad, np.flatnonzero(got_c != want_c)[:5])
            assert np.array_equal(got_I.view(np.uint32), want_I.view(np.uint32)), (name, k, rad)
            bad = np.flatnonzero((nan_bits(got_g) != nan_bits(want_g)).any(axis=1))
            assert bad.size == 0, (name, k, rad, bad[:5], got_g[bad[:2]], want_g[bad[:2]])
            if rad is None and name in ("floor_below", "floor_above") and k == 3:
                assert np.isnan(got_g[0]).all() == (name == "floor_below")
    if name == "wall":
        assert np.isfinite(got_g).all(axis=1).mean() > 0.9
    if name == "nonfinite":
        assert np.isnan(got_g).all(axis=1).sum() >= 50


# ---- r3d_icp_color_accumulate ----------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def wall():
    sc = REF.wall_scene()
    idx, d2 = REF.knn_lists(sc["tgt"], 8)
    sc["I"], sc["grad"], _ = REF.gradients(sc["tgt"], sc["normals"], sc["tgt_rgba"], idx, d2)
    sc["src_I"] = REF.intensity(sc["src_rgba"])
    return sc


def pass_inputs(wall, n_src, seed):
    """n_src sources near the wall's target (rows of the scene's source, jittered), their matches, and rows that cannot take part"""
    rng = np.random.default_rng(seed)
    rows = rng.integers(0, wall["src"].shape[0], n_src)
    src = (wall["src"][rows] + rng.normal(0, 2e-3, (n_src, 3)).astype(F)).astype(F)
    src_I = (wall["src_I"][rows] + rng.normal(0, 3, n_src).astype(F)).astype(F)
    nrm = wall["normals"].copy()
    nrm[rng.choice(nrm.shape[0], 40, replace=False)] = 0
    if n_src >= 255:
        src[5, 1] = np.nan
        src[9, 0] = np.inf
        src_I[11] = np.nan
    idx, d2 = REF.nearest(src, wall["tgt"])
    if n_src >= 255:
        idx[13] = wall["tgt"].shape[0]                                  # one past the target
        idx[14] = 0xffffffff
    return src, src_I, nrm, idx, d2


def device_pass(ctx, L, guard, wall, src, src_I, nrm, idx, d2, max_d2, w_photo, i_max, off=0):
    n, m = src.shape[0], wall["tgt"].shape[0]
    ins = [guard(a.nbytes, 0, a) for a in (src, src_I, wall["tgt"], nrm, wall["I"], wall["grad"], idx, d2)]
    o_p = guard(n * 4, off, seed=9)
    sums = np.full(31, -7.0)
    L.check(ctx.lib.r3d_icp_color_accumulate(ctx.handle, ins[0].ptr, ins[1].ptr, n, ins[2].ptr, ins[3].ptr, ins[4].ptr, ins[5].ptr, m,
                                             ins[6].ptr, ins[7].ptr, max_d2, w_photo, i_max, sums.ctypes.data, o_p.ptr))
    photo = o_p.read(F).copy()
    again = np.full(31, -7.0)
    L.check(ctx.lib.r3d_icp_color_accumulate(ctx.handle, ins[0].ptr, ins[1].ptr, n, ins[2].ptr, ins[3].ptr, ins[4].ptr, ins[5].ptr, m,
                                             ins[6].ptr, ins[7].ptr, max_d2, w_photo, i_max, again.ctypes.data, None))
    assert sums.tobytes() == again.tobytes(), "a repeat (without d_photo_out) gave other bits"
    plane = guard(29 * 8, 0, seed=4)
    L.check(ctx.lib.r3d_icp_plane_accumulate(ctx.handle, ins[0].ptr, n, ins[2].ptr, ins[3].ptr, m, ins[6].ptr, ins[7].ptr, max_d2, 0.0, 1.0,
                                             plane.ptr))
    for g in ins:
        g.unchanged()
    return sums, photo, plane.read(np.float64).copy()


@pytest.mark.parametrize("n_src", [1, 255, 257, 3072])
def test_accumulate_against_restatement(ctx, L, CI, guard, wall, n_src):
    src, src_I, nrm, idx, d2 = pass_inputs(wall, n_src, 40 + n_src)
    w = CI.photo_weight(0.968)
    for max_d2, i_max in ((-1.0, 40.0), (float(REF.WALL_MAX_D2), 6.0)):
        want = REF.accumulate(src, src_I, wall["tgt"], nrm, wall["I"], wall["grad"], idx, d2, max_d2, w, i_max)
        sums, photo, _ = device_pass(ctx, L, guard, wall, src, src_I, nrm, idx, d2, max_d2, w, i_max, off=4 if max_d2 < 0 else 0)
        assert_sums(sums, want.sums)
        assert np.array_equal(nan_bits(photo), nan_bits(want.photo)), np.flatnonzero(nan_bits(photo) != nan_bits(want.photo))[:5]
        if n_src >= 255:
            assert 0 < want.sums[29] <= want.sums[0] < n_src
    # w_photo = 0: the first 29 sums are r3d_icp_plane_accumulate's bytes (trim_q 0, gate_scale 1)
    for max_d2 in (-1.0, float(REF.WALL_MAX_D2)):
        sums, _, plane = device_pass(ctx, L, guard, wall, src, src_I, nrm, idx, d2, max_d2, 0.0, 40.0)
        assert sums[:29].tobytes() == plane.tobytes()
        assert sums[29] == REF.accumulate(src, src_I, wall["tgt"], nrm, wall["I"], wall["grad"], idx, d2, max_d2, 0.0, 40.0).sums[29]


def test_accumulate_gates_at_and_one_ulp_past(ctx, L, CI, guard, wall):
    src, src_I, nrm, idx, d2 = pass_inputs(wall, 257, 77)
    w = CI.photo_weight(0.968)
    free = REF.accumulate(src, src_I, wall["tgt"], nrm, wall["I"], wall["grad"], idx, d2, -1.0, w, 255.0)
    rows = np.flatnonzero(free.pho)
    a, b = rows[3], rows[8]
    gate = F(np.median(d2[rows]))
    d2 = d2.copy()
    d2[a], d2[b] = gate, np.nextafter(gate, F(np.inf))                  # the array is data: one pair AT the gate, one an ulp past
    want = REF.accumulate(src, src_I, wall["tgt"], nrm, wall["I"], wall["grad"], idx, d2, float(gate), w, 255.0)
    assert want.geo[a] and not want.geo[b]
    sums, photo, plane = device_pass(ctx, L, guard, wall, src, src_I, nrm, idx, d2, float(gate), w, 255.0)
    assert_sums(sums, want.sums)
    assert np.isfinite(photo[a]) and np.isnan(photo[b]) and np.array_equal(nan_bits(photo), nan_bits(want.photo))
    assert plane[0] == want.sums[0]
    # |rI| AT i_max is in, i_max one ulp (of the double) below |rI| puts that pair out and no other
    at = float(abs(free.rI[a]))
    for i_max, inside in ((at, True), (float(np.nextafter(at, 0.0)), False)):
        want = REF.accumulate(src, src_I, wall["tgt"], nrm, wall["I"], wall["grad"], idx, d2, -1.0, w, i_max)
        assert bool(want.pho[a]) == inside
        sums, photo, _ = device_pass(ctx, L, guard, wall, src, src_I, nrm, idx, d2, -1.0, w, i_max)
        assert_sums(sums, want.sums)
        assert np.isfinite(photo[a]) == inside and np.array_equal(nan_bits(photo), nan_bits(want.photo))


# ---- the loop, icp_colored, register_colored, the drop-in ------------------------------------------------------------------------
def test_icp_colored_on_the_wall(ctx, R, CI, icp, wall):
    sc = wall
    st, last = REF.loop(sc["src"], sc["src_I"], sc["tgt"], sc["normals"], sc["I"], sc["grad"], REF.WALL_ITERS, REF.WALL_MAX_D2,
                        CI.photo_weight(0.968), 40.0)
    T, info = R.icp_colored(sc["src"], sc["src_rgba"], sc["tgt"], sc["tgt_rgba"], tgt_normals=sc["normals"], max_iter=REF.WALL_ITERS,
                            max_dist=REF.WALL_MAX_DIST, ctx=ctx)
    assert info["status"] == 0 and info["photo_pairs"] > 0 and info["iterations"] == REF.WALL_ITERS
    assert info["pairs"] == last.sums[0] and info["photo_pairs"] == last.sums[29]
    np.testing.assert_allclose(T, st[:16].reshape(4, 4), atol=2e-6, rtol=0)
    before, after = REF.in_plane_error(np.eye(4), sc), REF.in_plane_error(T, sc)
    try:
        Tp, _ = icp.icp_point_to_plane(sc["src"], sc["tgt"], tgt_normals=sc["normals"], max_iter=REF.WALL_ITERS, max_dist=REF.WALL_MAX_DIST,
                                       ctx=ctx)
        plane_after = REF.in_plane_error(Tp, sc)
    except ValueError:
        plane_after = before                                             # the step is undefined on one wall: nothing moved
    print("wall: in-plane rms error before %.4e m; point-to-plane %.4e m; coloured ICP %.4e m (restatement %.4e m)"
          % (before, plane_after, after, REF.in_plane_error(st[:16].reshape(4, 4), sc)))
    assert plane_after >= 0.5 * before
    assert after <= 2 * REF.WALL_ERROR_AFTER


class ColourLoop:
    """The buffers of one r3d_icp_iterate_color loop on the wall: the source in the index's order, its intensities alongside."""

    def __init__(self, ctx, L, CI, wall, src, src_I, nrm, keep_original):
        n, m = src.shape[0], wall["tgt"].shape[0]
        self.ctx, self.L, self.n, self.keep_original = ctx, L, n, keep_original
        c = self.c = CI.Cloud(ctx, wall["tgt"])
        self.d_n, self.d_i, self.d_g = c.alloc(m * 12).upload(nrm), c.alloc(m * 4).upload(wall["I"]), c.alloc(m * 12).upload(wall["grad"])
        self.d_src, d_perm = c.alloc(n * 12).upload(src), c.alloc(n * 4)
        c.index.sort_cloud(self.d_src.ptr, n, d_perm.ptr)
        self.d_si = c.alloc(n * 4).upload(np.ascontiguousarray(src_I[d_perm.download(np.uint32, n)]))
        self.d_src0 = c.alloc(n * 12)
        L.check(ctx.lib.r3d_memcpy_d2d(ctx.handle, self.d_src0.ptr, self.d_src.ptr, n * 12))
        self.d_idx, self.d_d2, self.d_state, self.d_sums = c.alloc(n * 4), c.alloc(n * 4), c.alloc(512 * 8), c.alloc(31 * 8)
        L.check(ctx.lib.r3d_icp_state_reset(ctx.handle, self.d_state.ptr))

    def iterate(self, iters, w_photo, i_max):
        lib, h = self.ctx.lib, self.ctx.handle
        self.L.check(lib.r3d_icp_iterate_color(h, self.c.index.handle, self.d_src0.ptr if self.keep_original else None, self.d_src.ptr,
                                               self.d_si.ptr, self.n, self.d_n.ptr, self.d_i.ptr, self.d_g.ptr, self.d_idx.ptr,
                                               self.d_d2.ptr, iters, -1.0, w_photo, i_max, self.d_state.ptr, self.d_sums.ptr))
        return self.d_state.download(np.float64, 512)


@pytest.mark.parametrize("keep_original", [False, True])
def test_colour_loop_continued_with_and_without_the_original(ctx, R, L, CI, wall, keep_original):
    """r3d_icp_iterate_color called as 1, 1, 2 iterations (max_d2 = -1) on 257 sources of the wall (two partial rows), with
    d_src_orig and without.  After every call the state is the one before it advanced by the step and rms it stores itself
    (icp_state_ref.check_advance), the count is the running total, and [35] is the number of sources whose match in the d_idx left
    behind has a target normal (some normals are zeroed).  check_advance describes ONE step, and the state between the two
    iterations of the last call is never in HBM when the host can look: a twin loop on a context of its own, called 1, 1, 1 on the
    same inputs, supplies it (its first two states must be the loop's own, bit for bit).
    With the original: d_src is byte for byte what r3d_apply_T_dev makes of the original and the state's T_total -- the last
    iteration of a call moves by that very call.  Without: the last act of a call is the move by its last step, AFTER the query
    that filled d_idx and d_d2, so those describe the cloud as it was before that move (the cloud the call began with; in the last
    call the twin's cloud after its third iteration): they are what r3d_nn_index_query returns for THAT cloud -- both, bit for bit:
    the warm and the cold query are exact searches over one fp32 distance expression, the lowest target index winning ties
    (include/r3d.h, the index's contract) -- and d_src is that cloud moved by the stored step, byte for byte."""
    import icp_state_ref as SR
    n = 257
    rows = np.linspace(0, wall["src"].shape[0] - 1, n).astype(np.int64)
    src, src_I = np.ascontiguousarray(wall["src"][rows]), np.ascontiguousarray(wall["src_I"][rows])
    nrm = wall["normals"].copy()
    nrm[::7] = 0
    has = (nrm != 0).any(axis=1)
    w = CI.photo_weight(0.968)
    twin_ctx = R.Context(0)
    loop = twin = None
    try:
        loop = ColourLoop(ctx, L, CI, wall, src, src_I, nrm, keep_original)
        twin = ColourLoop(twin_ctx, L, CI, wall, src, src_I, nrm, keep_original)
        prev, total = loop.d_state.download(np.float64, 512), 0
        for k, iters in enumerate((1, 1, 2)):
            before = loop.d_src.download(np.uint8, n * 12)
            twin_state = twin.iterate(1, w, 40.0)
            if iters == 2:                                                  # the state and the cloud between the two iterations
                prev, before = twin_state, twin.d_src.download(np.uint8, n * 12)
            got = loop.iterate(iters, w, 40.0)
            if iters == 1:
                assert got.tobytes() == twin_state.tobytes(), (k, "the twin loop went another way")
                assert loop.d_src.download(np.uint8, n * 12).tobytes() == twin.d_src.download(np.uint8, n * 12).tobytes(), k
            total += iters
            SR.check_advance(prev, got, got[16:32], got[34], 0, got[35], what=k)
            assert got[32] == total and got[33] == 0.0
            idx = loop.d_idx.download(np.uint32, n)
            assert got[35] == float(has[idx].sum()) and 6 < got[35] < n, (k, got[35], has[idx].sum())
            d_want = loop.c.alloc(n * 12)
            if keep_original:
                L.check(ctx.lib.r3d_apply_T_dev(ctx.handle, loop.d_src0.ptr, L.F32, n, loop.d_state.ptr, d_want.ptr, L.F32))
            else:
                d_before, d_i2, d_d22 = loop.c.alloc(n * 12).upload(before), loop.c.alloc(n * 4), loop.c.alloc(n * 4)
                loop.c.index.query(d_before.ptr, n, d_i2.ptr, d_d22.ptr, presorted=True)
                assert np.array_equal(d_i2.download(np.uint32, n), idx), k
                assert d_d22.download(np.uint8, n * 4).tobytes() == loop.d_d2.download(np.uint8, n * 4).tobytes(), k
                L.check(ctx.lib.r3d_apply_T_dev(ctx.handle, d_before.ptr, L.F32, n, loop.d_state.ptr + 16 * 8, d_want.ptr, L.F32))
            assert loop.d_src.download(np.uint8, n * 12).tobytes() == d_want.download(np.uint8, n * 12).tobytes(), k
            prev = got
    finally:
        for c in (loop, twin):
            if c is not None:
                c.c.close()
        twin_ctx.close()


def test_register_colored_two_scales(ctx, R, wall):
    sc = wall
    T, info = R.register_colored(sc["src"], sc["src_rgba"], sc["tgt"], sc["tgt_rgba"], voxel_sizes=(0.04, 0.005), iters=(15, 20),
                                 max_dist_voxels=12.0, ctx=ctx)
    assert len(info["scales"]) == 2 and all(s["status"] == 0 and s["photo_pairs"] > 0 for s in info["scales"])
    assert info["scales"][0]["target_points"] < info["scales"][1]["target_points"] <= sc["tgt"].shape[0]
    after = REF.in_plane_error(T, sc)
    print("wall, two scales: in-plane rms error %.4e m" % after)
    assert after <= 2 * REF.WALL_ERROR_AFTER


def test_drop_in_reproduces_the_api(ctx, R, wall, tmp_path):
    sc = wall
    s_ply, t_ply, out, ref = [str(tmp_path / f) for f in ("src.ply", "tgt.ply", "T_data.txt", "T_api.txt")]
    R.cloud_io.write_ply_rgb(s_ply, sc["src"], sc["src_rgba"])
    R.cloud_io.write_ply_rgb(t_ply, sc["tgt"], sc["tgt_rgba"])
    tool = os.path.join(ROOT, PKG, "other_tools", "colored_icp.py")
    r = subprocess.run([sys.executable, tool, s_ply, t_ply, "-o", out, "--iters", "12", "--max-dist", "0.06"], capture_output=True,
                       text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    (src, sw), (tgt, tw) = R.cloud_io.read_ply_rgb(s_ply), R.cloud_io.read_ply_rgb(t_ply)
    T, info = R.icp_colored(src.astype(F), sw, tgt.astype(F), tw, max_iter=12, max_dist=0.06, ctx=ctx)
    R.write_T(ref, T)
    assert info["status"] == 0 and open(out, "rb").read() == open(ref, "rb").read()
    bad = subprocess.run([sys.executable, tool, s_ply, t_ply, "-o", str(tmp_path / "no.txt"), "--k", "40"], capture_output=True, text=True,
                         timeout=300)
    assert bad.returncode == 1 and not os.path.exists(str(tmp_path / "no.txt"))


def test_invalid_calls_write_nothing(ctx, L, icp, guard, wall):
    lib, h = ctx.lib, ctx.handle
    xyz, nrm, rgba, _ = clouds()["lattice"]
    n = xyz.shape[0]
    g_xyz, g_n, g_w = guard(xyz.nbytes, 0, xyz), guard(nrm.nbytes, 0, nrm), guard(rgba.nbytes, 0, rgba)
    o_i, o_g, o_c = guard(n * 4, 4, seed=1), guard(n * 12, 4, seed=2), guard(n * 4, 0, seed=3)
    ix = icp.NNIndex(ctx, g_xyz.ptr, n)
    try:
        f = lib.r3d_color_gradient_knn
        calls = [(None, 8, 0.0, g_n.ptr, g_w.ptr, o_i.ptr, o_g.ptr, o_c.ptr), (ix.handle, 2, 0.0, g_n.ptr, g_w.ptr, o_i.ptr, o_g.ptr, o_c.ptr),
                 (ix.handle, 33, 0.0, g_n.ptr, g_w.ptr, o_i.ptr, o_g.ptr, o_c.ptr),
                 (ix.handle, 8, float("nan"), g_n.ptr, g_w.ptr, o_i.ptr, o_g.ptr, o_c.ptr),
                 (ix.handle, 8, 0.0, None, g_w.ptr, o_i.ptr, o_g.ptr, o_c.ptr), (ix.handle, 8, 0.0, g_n.ptr, None, o_i.ptr, o_g.ptr, o_c.ptr),
                 (ix.handle, 8, 0.0, g_n.ptr, g_w.ptr, None, o_g.ptr, o_c.ptr), (ix.handle, 8, 0.0, g_n.ptr, g_w.ptr, o_i.ptr, None, o_c.ptr),
                 (ix.handle, 8, 0.0, g_n.ptr, g_w.ptr, o_g.ptr, o_g.ptr, o_c.ptr), (ix.handle, 8, 0.0, g_n.ptr, g_w.ptr, o_i.ptr, o_g.ptr, o_i.ptr),
                 (ix.handle, 8, 0.0, g_n.ptr, g_w.ptr, o_i.ptr, g_n.ptr, o_c.ptr), (ix.handle, 8, 0.0, g_n.ptr, g_w.ptr, g_w.ptr, o_g.ptr, o_c.ptr)]
        for a in calls:
            assert f(*a) == L.ERR_INVALID, a
        for g in (g_xyz, g_n, g_w, o_i, o_g, o_c):
            g.unchanged()
        # r3d_icp_color_accumulate
        src, src_I, wn, idx, d2 = pass_inputs(wall, 255, 5)
        m = wall["tgt"].shape[0]
        ins = [guard(a.nbytes, 0, a) for a in (src, src_I, wall["tgt"], wn, wall["I"], wall["grad"], idx, d2)]
        o_p = guard(255 * 4, 4, seed=5)
        sums = np.full(31, -7.0)

        def acc(src_p=ins[0].ptr, n_src=255, d2_p=ins[7].ptr, max_d2=-1.0, w=1e-5, i_max=40.0, sums_p=sums.ctypes.data, photo=o_p.ptr,
                grad=ins[5].ptr):
            return lib.r3d_icp_color_accumulate(h, src_p, ins[1].ptr, n_src, ins[2].ptr, ins[3].ptr, ins[4].ptr, grad, m, ins[6].ptr, d2_p,
                                                max_d2, w, i_max, sums_p, photo)
        for kw in (dict(src_p=None), dict(n_src=-1), dict(d2_p=None, max_d2=1.0), dict(max_d2=float("nan")), dict(w=-1.0), dict(w=float("inf")),
                   dict(w=float("nan")), dict(i_max=0.0), dict(i_max=float("inf")), dict(sums_p=None), dict(photo=ins[0].ptr),
                   dict(photo=ins[5].ptr + 4), dict(grad=None)):
            assert acc(**kw) == L.ERR_INVALID, kw
        assert (sums == -7.0).all()
        # r3d_icp_iterate_color
        tgt_ix = icp.NNIndex(ctx, ins[2].ptr, m)
        try:
            o_src, o_src0 = guard(src.nbytes, 0, src), guard(src.nbytes, 0, src)
            o_idx, o_d2, o_st, o_s = guard(255 * 4, 0, seed=6), guard(255 * 4, 4, seed=7), guard(512 * 8, 0, seed=8), guard(31 * 8, 0, seed=9)

            def it(ix_h=tgt_ix.handle, orig=o_src0.ptr, s=o_src.ptr, n_src=255, idx_p=o_idx.ptr, d2_p=o_d2.ptr, iters=2, max_d2=-1.0, w=1e-5,
                   i_max=40.0, st=o_st.ptr, so=o_s.ptr):
                return lib.r3d_icp_iterate_color(h, ix_h, orig, s, ins[1].ptr, n_src, ins[3].ptr, ins[4].ptr, ins[5].ptr, idx_p, d2_p, iters,
                                                 max_d2, w, i_max, st, so)
            for kw in (dict(ix_h=None), dict(iters=-1), dict(n_src=5), dict(orig=o_src.ptr), dict(s=None), dict(idx_p=None), dict(st=None),
                       dict(w=float("inf")), dict(w=-1e-9), dict(i_max=-1.0), dict(max_d2=float("nan")), dict(d2_p=o_idx.ptr),
                       dict(so=o_st.ptr + 64), dict(s=ins[5].ptr), dict(st=ins[3].ptr)):
                assert it(**kw) == L.ERR_INVALID, kw
            for g in ins + [o_p, o_src, o_src0, o_idx, o_d2, o_st, o_s]:
                g.unchanged()
        finally:
            tgt_ix.close()
        # the context still answers
        idx8, d28 = REF.knn_lists(xyz, 8)
        want = REF.gradients(xyz, nrm, rgba, idx8, d28)
        L.check(f(ix.handle, 8, 0.0, g_n.ptr, g_w.ptr, o_i.ptr, o_g.ptr, o_c.ptr))
        assert np.array_equal(o_c.read(np.uint32), want[2]) and np.array_equal(nan_bits(o_g.read(F, (n, 3))), nan_bits(want[1]))
        assert acc() == L.OK and sums[0] > 0
    finally:
        ix.close()
