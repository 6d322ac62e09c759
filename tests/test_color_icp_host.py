"""CPU: the coloured-ICP specification as tests/color_icp_ref.py restates it (include/r3d.h, "Coloured ICP"), and every refusal
of the Python layer and of other_tools/colored_icp.py that comes before any device use (without a device, a call that got as far
as opening one raises R3DError, not ValueError).

The wall scene, restatement loop, 20 iterations, k = 8, i_max = 40, lambda 0.968, pairs within three spacings:
    in-plane RMS error before 4.167e-02 m (about two spacings), after 1.83e-04 m (a hundredth of a spacing);
    the geometric sums alone are singular (plane_step_from_sums raises), the coloured loop ends with status 0."""
import importlib
import importlib.util
import os

import numpy as np
import pytest

import color_icp_ref as REF
from helpers import PKG, ROOT

F = np.float32
TOOL = os.path.join(ROOT, PKG, "other_tools", "colored_icp.py")


@pytest.fixture(scope="module")
def R():
    return importlib.import_module(PKG)


@pytest.fixture(scope="module")
def icp():
    return importlib.import_module(PKG + ".icp")


def grey(v):
    v = np.asarray(v, np.uint8)
    return REF.words(np.stack([v, v, v], axis=1))


def lattice_ramp(rot=None):
    """a 9 x 9 unit lattice in the plane z = 0 (turned by rot), grey value 10 + 3 x + 5 y"""
    gx, gy = np.meshgrid(np.arange(9), np.arange(9), indexing="xy")
    p = np.stack([gx.ravel(), gy.ravel(), np.zeros(81)], axis=1).astype(np.float64)
    rgba = grey(10 + 3 * gx.ravel() + 5 * gy.ravel())
    n, slope = np.array([0.0, 0.0, 1.0]), np.array([3.0, 5.0, 0.0])
    if rot is not None:
        p, n, slope = p @ rot.T, rot @ n, rot @ slope
    return p.astype(F), np.tile(n.astype(F), (81, 1)), rgba, slope


def rotation(axis, angle):
    a = np.asarray(axis, np.float64) / np.linalg.norm(axis)
    K = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    return np.eye(3) + np.sin(angle) * K + (1 - np.cos(angle)) * (K @ K)


@pytest.mark.parametrize("rot", [None, rotation((1, 2, 3), 0.7)], ids=["axis", "oblique"])
@pytest.mark.parametrize("k", [4, 8, 20])
def test_gradient_of_a_linear_ramp_is_its_slope_and_tangent(rot, k):
    """The f32 intensity of a grey byte v is v within 3 ulp(100) = 2.3e-5, the f32 coordinates of the turned lattice are within 5e-7
    of the plane: a least-squares slope over unit spacings is within 1e-4 of (3, 5, 0) turned.  g . n: the fp64 solve pins it to
    rounding level, the f32 rounding of g adds at most 2^-24 sum |g_a n_a| <= 2^-24 sqrt(3) |g|."""
    xyz, nrm, rgba, slope = lattice_ramp(rot)
    idx, d2 = REF.knn_lists(xyz, k)
    I, g, c = REF.gradients(xyz, nrm, rgba, idx, d2)
    assert (c == k).all() and np.isfinite(g).all()
    np.testing.assert_allclose(I, 10 + 3 * np.tile(np.arange(9), 9) + 5 * np.repeat(np.arange(9), 9), atol=2.3e-5, rtol=0)
    np.testing.assert_allclose(g.astype(np.float64), np.tile(slope, (81, 1)), atol=1e-4, rtol=0)
    gn = np.abs((g.astype(np.float64) * nrm.astype(np.float64)).sum(axis=1))
    assert (gn <= 2.0 ** -23 * np.linalg.norm(g.astype(np.float64), axis=1)).all(), gn.max()


def test_radius_cuts_the_list():
    xyz, nrm, rgba, _ = lattice_ramp()
    idx, d2 = REF.knn_lists(xyz, 8)
    _, g, c = REF.gradients(xyz, nrm, rgba, idx, d2, radius=1.0)        # the four axis neighbours only, fewer at the rim
    inner = (xyz[:, 0] > 0) & (xyz[:, 0] < 8) & (xyz[:, 1] > 0) & (xyz[:, 1] < 8)
    assert (c[inner] == 4).all() and (c[~inner] <= 3).all() and np.isfinite(g[inner]).all()
    corner = (c == 2)
    assert corner.sum() == 4 and np.isnan(g[corner]).all()


def test_photometric_jacobian_agrees_with_central_differences():
    """rI is linear in p, so central differences of the restatement's own rI over the six motions omega_k, v_k (p -> p + h e_k x p,
    p -> p + h e_k) give J = [p x a ; a] up to rounding: |rI| <= 60 evaluated in fp64 loses 60 * 2^-52 / h = 1.3e-8 at h = 1e-6."""
    rng = np.random.default_rng(3)
    m = 50
    p, q = rng.normal(size=(m, 3)), rng.normal(size=(m, 3))
    n = rng.normal(size=(m, 3))
    n /= np.linalg.norm(n, axis=1, keepdims=True)
    g, Iq, Ip = rng.normal(size=(m, 3)) * 20, rng.uniform(0, 255, m), rng.uniform(0, 255, m)
    _, _, a = REF.photo_term(p, q, n, Iq, g, Ip)
    J = np.concatenate([np.cross(p, a), a], axis=1)
    h = 1e-6
    for k in range(6):
        e = np.zeros(3)
        e[k % 3] = 1.0
        dp = np.cross(np.tile(e, (m, 1)), p) if k < 3 else np.tile(e, (m, 1))
        hi, lo = REF.photo_term(p + h * dp, q, n, Iq, g, Ip)[1], REF.photo_term(p - h * dp, q, n, Iq, g, Ip)[1]
        np.testing.assert_allclose((hi - lo) / (2 * h), J[:, k], atol=1e-6, rtol=1e-7)
    assert np.abs((a * n).sum(axis=1)).max() <= 1e-13 * 20 * 3          # a is tangent


def _centre_case(s, normal=(0, 0, 1)):
    """a point with three neighbours at (s, 0, 0), (0, s, 0), (-s, 0, 0): A = diag(2 s^2, s^2, 9), det = 18 s^4, tr = 9 + 3 s^2"""
    s = float(F(s))
    xyz = F([[0, 0, 0], [s, 0, 0], [0, s, 0], [-s, 0, 0]])
    rgba = grey([100, 110, 90, 95])
    idx, d2 = REF.knn_lists(xyz, 3)
    return REF.gradients(xyz, np.tile(F(normal), (4, 1)), rgba, idx, d2, details=True)


def test_no_gradient_cases():
    line = np.stack([np.arange(7), np.zeros(7), np.zeros(7)], axis=1).astype(F)
    up = np.tile(F([0, 0, 1]), (7, 1))
    rgba = grey(np.arange(7) * 9)
    idx, d2 = REF.knn_lists(line, 4)
    _, g, c = REF.gradients(line, up, rgba, idx, d2)
    assert (c == 4).all() and np.isnan(g).all()                          # collinear on the tangent plane: det == 0
    skew = line @ rotation((1, 1, 0), 0.4).T.astype(F)                   # the same line, oblique: det is rounding noise
    _, g, c, det, tr = REF.gradients(skew, (up.astype(np.float64) @ rotation((1, 1, 0), 0.4).T).astype(F), rgba, *REF.knn_lists(skew, 4),
                                     details=True)
    assert np.isnan(g).all() and (np.abs(det) <= 1e-15 * tr ** 3).all(), (det / tr ** 3)
    for n_pts in (1, 2, 3):                                              # fewer than 3 neighbours
        xyz = F([[0, 0, 0], [1, 0, 0], [0, 1, 0]])[:n_pts]
        idx, d2 = REF.knn_lists(xyz, 3)
        I, g, c = REF.gradients(xyz, up[:n_pts], rgba[:n_pts], idx, d2)
        assert (c == n_pts - 1).all() and np.isnan(g).all() and np.isfinite(I).all()
    xyz, nrm, rgba, _ = lattice_ramp()
    nrm = nrm.copy()
    nrm[10] = 0
    nrm[11, 1] = np.nan
    nrm[12, 2] = np.inf
    xyz = xyz.copy()
    xyz[40, 0] = np.nan
    idx, d2 = REF.knn_lists(xyz, 8)
    I, g, c = REF.gradients(xyz, nrm, rgba, idx, d2)
    bad = np.zeros(81, bool)
    bad[[10, 11, 12, 40]] = True
    assert np.isnan(g[bad]).all() and np.isfinite(g[~bad]).all() and c[40] == 0 and (c[~bad] == 8).all() and np.isfinite(I).all()


def test_conditioning_floor_from_both_sides():
    """det / tr^3 = 18 s^4 / (9 + 3 s^2)^3 crosses 1e-14 at s = 7.98e-4: planted well inside on both sides, and at the two
    neighbouring f32 values of s between which the answer flips."""
    _, g, _, det, tr = _centre_case(1e-3)
    assert np.isfinite(g[0]).all() and det[0] > REF.FLOOR * tr[0] ** 3
    np.testing.assert_allclose(g[0], [(110 - 95) / 2e-3, (90 - 100) / 1e-3, 0], rtol=1e-5)
    _, g, _, det, tr = _centre_case(6e-4)
    assert np.isnan(g[0]).all() and 0 < det[0] < REF.FLOOR * tr[0] ** 3
    lo, hi = F(6e-4), F(1e-3)
    while np.nextafter(lo, hi) < hi:
        mid = F(0.5) * (lo + hi)
        if np.isnan(_centre_case(mid)[1][0]).all():
            lo = mid
        else:
            hi = mid
    assert abs(float(hi) - 7.98e-4) < 2e-6
    assert np.isnan(_centre_case(lo)[1][0]).all() and np.isfinite(_centre_case(hi)[1][0]).all()


@pytest.fixture(scope="module")
def wall():
    sc = REF.wall_scene()
    idx, d2 = REF.knn_lists(sc["tgt"], 8)
    sc["I"], sc["grad"], _ = REF.gradients(sc["tgt"], sc["normals"], sc["tgt_rgba"], idx, d2)
    sc["src_I"] = REF.intensity(sc["src_rgba"])
    return sc


def test_wall_scene_geometry_is_singular_and_colour_registers_it(wall, icp, R):
    CI = importlib.import_module(PKG + ".colored_icp")
    sc = wall
    assert sc["tgt"].shape == (64 * 48, 3) and np.isfinite(sc["grad"]).mean() > 0.99
    idx, d2 = REF.nearest(sc["src"], sc["tgt"])
    geo = REF.accumulate(sc["src"], sc["src_I"], sc["tgt"], sc["normals"], sc["I"], sc["grad"], idx, d2, REF.WALL_MAX_D2, 0.0, 40.0)
    assert geo.sums[0] == sc["src"].shape[0] and geo.sums[29] > 0
    with pytest.raises(ValueError):
        icp.plane_step_from_sums(geo.sums[:29])
    st, last = REF.loop(sc["src"], sc["src_I"], sc["tgt"], sc["normals"], sc["I"], sc["grad"], REF.WALL_ITERS, REF.WALL_MAX_D2,
                        CI.photo_weight(0.968), 40.0)
    before, after = REF.in_plane_error(np.eye(4), sc), REF.in_plane_error(st[:16].reshape(4, 4), sc)
    print("wall scene, restatement: in-plane rms error before %.4e m, after %.4e m; photometric pairs %d, rms %.3f"
          % (before, after, last.sums[29], np.sqrt(last.sums[30] / last.sums[29])))
    assert st[33] == 0 and st[32] == REF.WALL_ITERS and last.sums[29] > 0
    assert 1.5 * REF.SPACING < before < 2.5 * REF.SPACING               # "about two spacings"
    assert after <= REF.WALL_ERROR_AFTER * 1.001 and after < before / 10


# ---- refusals before any device use --------------------------------------------------------------------------------------------
def test_python_layer_refuses_bad_arguments(R):
    xyz = np.zeros((10, 3), F)
    w = np.zeros(10, np.uint32)
    ok = dict(src=xyz, src_rgba=w, tgt=xyz, tgt_rgba=w, tgt_normals=np.tile(F([0, 0, 1]), (10, 1)))

    def bad(**kw):
        a = dict(ok)
        a.update(kw)
        with pytest.raises(ValueError):
            R.icp_colored(**a)

    bad(src=np.zeros((10, 2), F))
    bad(tgt=np.zeros(30, F))
    bad(src=np.zeros((5, 3), F), src_rgba=np.zeros(5, np.uint32))
    bad(src_rgba=np.zeros(9, np.uint32))
    bad(tgt_rgba=np.zeros(11, np.uint32))
    bad(src_rgba=np.zeros(10, np.int32))
    bad(tgt_rgba=np.zeros((10, 3), np.uint8))
    bad(tgt_normals=np.zeros((9, 3), F))
    bad(tgt_normals=np.zeros((10, 3), np.int32))
    for lam in (0.0, -0.1, 1.5, np.nan, "x"):
        bad(lambda_geometric=lam)
    init = np.eye(4)
    init[0, 3] = np.nan
    bad(init=init)
    bad(init=np.eye(3))
    bad(k=2)
    bad(k=33)
    bad(i_max=0.0)
    bad(i_max=np.inf)
    bad(max_dist=-1.0)
    bad(max_iter=0)
    bad(w_photo=-1.0)
    bad(w_photo=np.inf)
    nrm = ok["tgt_normals"]
    for args in ((np.zeros((10, 2), F), w, nrm), (xyz, w[:9], nrm), (xyz, w.astype(np.int64), nrm), (xyz, w, nrm[:9])):
        with pytest.raises(ValueError):
            R.colour_gradients(*args)
    for kw in (dict(k=2), dict(radius=0.0), dict(radius=np.nan)):
        with pytest.raises(ValueError):
            R.colour_gradients(xyz, w, nrm, **kw)
    for kw in (dict(voxel_sizes=(0.1, 0.05), iters=(3,)), dict(voxel_sizes=(), iters=()), dict(voxel_sizes=(0.1, -1.0), iters=(3, 3)),
               dict(voxel_sizes=(0.1,), iters=(0,)), dict(lambda_geometric=0.0), dict(init=np.full((4, 4), np.inf)), dict(k=1),
               dict(src_rgba=w[:3])):
        a = dict(src=xyz, src_rgba=w, tgt=xyz, tgt_rgba=w)
        a.update(kw)
        with pytest.raises(ValueError):
            R.register_colored(**a)
    CI = importlib.import_module(PKG + ".colored_icp")
    assert CI.photo_weight(0.968) == ((1 - 0.968) / 0.968) / 255.0 ** 2 and CI.photo_weight(1.0) == 0.0
    np.testing.assert_array_equal(CI.intensity(REF.words([[255, 0, 7]], [200])).view(np.uint32), REF.intensity(REF.words([[255, 0, 7]])).view(np.uint32))


def test_command_line_usage_errors_write_nothing(tmp_path, R):
    spec = importlib.util.spec_from_file_location("colored_icp_tool", TOOL)
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    xyz = np.random.default_rng(0).random((20, 3)).astype(F)
    col, plain, out = str(tmp_path / "c.ply"), str(tmp_path / "p.ply"), str(tmp_path / "T.txt")
    R.cloud_io.write_ply_rgb(col, xyz, REF.words(np.full((20, 3), 7, np.uint8)))
    R.cloud_io.write_ply(plain, xyz)
    back, words = R.cloud_io.read_ply_rgb(col)
    assert np.abs(back - xyz).max() <= 5.1e-5 and (words == 7 * 0x010101).all()     # the layout keeps four decimals
    with pytest.raises(ValueError):
        R.cloud_io.read_ply_rgb(plain)
    for argv in ([col, col], [col, str(tmp_path / "missing.ply"), "-o", out], [col, col, "-o", out, "--k", "2"],
                 [col, col, "-o", out, "--k", "x"], [col, col, "-o", out, "--lambda", "0"], [col, col, "-o", out, "--i-max", "-3"],
                 [col, col, "-o", out, "--voxel", "0.1", "0.05", "--iters", "3"], [col, col, "-o", out, "--voxel", "0"],
                 [col, col, "-o", out, "--iters", "0"], [col, col, "-o", out, "--init", str(tmp_path / "none.txt")],
                 [col, col, "-o", out, "--voxel", "0.1", "--max-dist", "1"], [col, "-o", out]):
        with pytest.raises(SystemExit) as e:
            tool.main(argv)
        assert e.value.code == 1, argv
    assert tool.main([plain, col, "-o", out]) == 1                      # no colour columns: refused before the device is opened
    assert not os.path.exists(out)
