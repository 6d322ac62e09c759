"""GPU: torch-facing BackprojectDepth (f4) against a plain PyTorch fp32 statement of upstream monodepth2's layer
(the formula the reference's trainer relies on, monodepth2/trainer.py:150-160, 387-390), forward and backward.
Tolerance: fp32, |err| <= 1e-5 * (1 + |ref|) -- the layer's matmul has no defined summation order.

Second half of the file: the five kernels of csrc/r3d_backproject.hip at the C ABI, in guarded buffers, against
tests/project_ref.py -- every per-pixel output BIT FOR BIT against the f32 restatement of the include/r3d.h chains, the twelve
per-image sums d_grad_P per entry against the float64 statement within project_ref.grad_P_bound (u = 2**-24 times a count of
roundings; nothing there is measured on a GPU) -- then the torch layers' plumbing: views, streams, the trainer's sequence."""
import ctypes as C
import importlib

import numpy as np
import pytest

import project_ref as PR
from helpers import PKG, r3d as _r3d

pytestmark = pytest.mark.gpu


def reference_backproject(depth, inv_K, batch, height, width):
    import torch
    ys, xs = np.meshgrid(range(height), range(width), indexing="ij")          # upstream: meshgrid(range(w), range(h), 'xy')
    pix = torch.from_numpy(np.stack([xs.reshape(-1), ys.reshape(-1), np.ones(height * width)], 0).astype(np.float32))
    pix = pix.unsqueeze(0).repeat(batch, 1, 1).to(depth.device)
    cam = torch.matmul(inv_K[:, :3, :3], pix)
    cam = depth.view(batch, 1, -1) * cam
    return torch.cat([cam, torch.ones(batch, 1, height * width, device=depth.device)], 1)


@pytest.mark.parametrize("shape", [(1, 4, 6), (3, 24, 32), (2, 192, 640), (12, 96, 320), (1, 480, 640)])
def test_backproject_depth_forward_backward(shape):
    import torch
    T = importlib.import_module(PKG + ".torch_ops")
    b, h, w = shape
    dev = torch.device("cuda", 0)
    g = torch.Generator(device="cpu").manual_seed(b * 1000 + h)
    depth = (torch.rand((b, 1, h, w), generator=g) * 80 + 0.1).to(dev).requires_grad_(True)
    K = torch.eye(4).repeat(b, 1, 1)
    K[:, 0, 0], K[:, 1, 1], K[:, 0, 2], K[:, 1, 2] = 0.58 * w, 1.92 * h, 0.5 * w, 0.5 * h
    K[:, 0, 1] = torch.rand(b, generator=g) * 0.01                            # a little skew so every entry matters
    inv_K = torch.linalg.inv(K).to(dev)
    layer = T.BackprojectDepth(b, h, w)
    out = layer(depth, inv_K)
    depth_ref = depth.detach().clone().requires_grad_(True)
    ref = reference_backproject(depth_ref, inv_K, b, h, w)
    assert out.shape == ref.shape == (b, 4, h * w) and out.dtype == torch.float32
    err = (out - ref).abs() / (1 + ref.abs())
    assert float(err.max()) <= 1e-5, float(err.max())
    assert torch.equal(out[:, 3], torch.ones_like(out[:, 3]))
    weight = torch.rand(out.shape, generator=g).to(dev)
    (out * weight).sum().backward()
    (ref * weight).sum().backward()
    gerr = (depth.grad - depth_ref.grad).abs() / (1 + depth_ref.grad.abs())
    assert depth.grad.shape == depth.shape and float(gerr.max()) <= 1e-5, float(gerr.max())


def test_backproject_depth_refuses_cpu_and_bad_shapes():
    import torch
    T = importlib.import_module(PKG + ".torch_ops")
    layer = T.BackprojectDepth(1, 4, 6)
    with pytest.raises(RuntimeError):
        layer(torch.ones(1, 1, 4, 6), torch.eye(4).unsqueeze(0))
    dev = torch.device("cuda", 0)
    with pytest.raises(ValueError):
        layer(torch.ones(1, 1, 4, 7, device=dev), torch.eye(4, device=dev).unsqueeze(0))
    with pytest.raises(TypeError):
        layer(torch.ones(1, 1, 4, 6, device=dev, dtype=torch.float64), torch.eye(4, device=dev).unsqueeze(0))


def reference_project3d(points, K, T, batch, height, width, eps=1e-7):
    """upstream monodepth2 layers.Project3D.forward, statement for statement."""
    import torch
    P = torch.matmul(K, T)[:, :3, :]
    cam_points = torch.matmul(P, points)
    pix_coords = cam_points[:, :2, :] / (cam_points[:, 2, :].unsqueeze(1) + eps)
    pix_coords = pix_coords.view(batch, 2, height, width)
    pix_coords = pix_coords.permute(0, 2, 3, 1)
    pix_coords = pix_coords / torch.tensor([width - 1, height - 1], dtype=torch.float32, device=points.device)
    return (pix_coords - 0.5) * 2


@pytest.mark.parametrize("shape", [(1, 4, 6), (3, 24, 32), (2, 192, 640), (12, 96, 320), (1, 480, 640)])
def test_project3d_forward_backward_through_the_trainer_pair(shape):
    """depth -> BackprojectDepth -> Project3D (trainer.py:387-390) with gradients into depth, K and T.
    Tolerance: fp32; forward |err| <= 1e-5 (1 + |ref|) on coordinates of O(1); the per-image K / T gradients are sums over
    H*W pixels (fp32 partials, fixed order here, rocBLAS order in the reference): <= 2e-4 of the gradient's largest entry."""
    import torch
    TO = importlib.import_module(PKG + ".torch_ops")
    b, h, w = shape
    dev = torch.device("cuda", 0)
    g = torch.Generator(device="cpu").manual_seed(b * 77 + w)
    depth0 = (torch.rand((b, 1, h, w), generator=g) * 40 + 2.0).to(dev)
    K0 = torch.eye(4).repeat(b, 1, 1)
    K0[:, 0, 0], K0[:, 1, 1], K0[:, 0, 2], K0[:, 1, 2] = 0.58 * w, 1.92 * h, 0.5 * w, 0.5 * h
    inv_K = torch.linalg.inv(K0).to(dev)
    ang = (torch.rand(b, generator=g) - 0.5) * 0.1
    T0 = torch.eye(4).repeat(b, 1, 1)
    T0[:, 0, 0], T0[:, 0, 2], T0[:, 2, 0], T0[:, 2, 2] = torch.cos(ang), torch.sin(ang), -torch.sin(ang), torch.cos(ang)
    T0[:, :3, 3] = (torch.rand((b, 3), generator=g) - 0.5) * 0.6
    weight = torch.rand((b, h, w, 2), generator=g).to(dev)
    grads = []
    for mine in (True, False):
        depth = depth0.clone().requires_grad_(True)
        K = K0.to(dev).requires_grad_(True)
        T = T0.to(dev).requires_grad_(True)
        if mine:
            pts = TO.BackprojectDepth(b, h, w)(depth, inv_K)
            pix = TO.Project3D(b, h, w)(pts, K, T)
        else:
            pts = reference_backproject(depth, inv_K, b, h, w)
            pix = reference_project3d(pts, K, T, b, h, w)
        assert pix.shape == (b, h, w, 2) and pix.dtype == torch.float32
        (pix * weight).sum().backward()
        grads.append((pix.detach(), depth.grad, K.grad, T.grad))
    (pix, gd, gK, gT), (pix_r, gd_r, gK_r, gT_r) = grads
    err = (pix - pix_r).abs() / (1 + pix_r.abs())
    assert float(err.max()) <= 1e-5, float(err.max())
    gerr = (gd - gd_r).abs() / (1e-6 + gd_r.abs().max())
    assert float(gerr.max()) <= 1e-5, float(gerr.max())
    for got, want in ((gK, gK_r), (gT, gT_r)):
        assert got.shape == want.shape == (b, 4, 4)
        assert float((got - want).abs().max()) <= 2e-4 * float(want.abs().max()), (got, want)


def test_project3d_grad_P_is_bitwise_repeatable_and_optional_outputs():
    import torch
    TO = importlib.import_module(PKG + ".torch_ops")
    b, h, w = 2, 192, 640
    dev = torch.device("cuda", 0)
    g = torch.Generator(device="cpu").manual_seed(5)
    pts = torch.rand((b, 4, h * w), generator=g).to(dev) + 1.0
    K = (torch.eye(4).repeat(b, 1, 1) * 50).to(dev).requires_grad_(True)
    T = torch.eye(4).repeat(b, 1, 1).to(dev)
    layer = TO.Project3D(b, h, w)
    weight = torch.rand((b, h, w, 2), generator=g).to(dev)
    runs = []
    for _ in range(3):
        K.grad = None
        (layer(pts, K, T) * weight).sum().backward()                # points need no gradient here: only grad_P is formed
        runs.append(K.grad.clone())
    assert torch.equal(runs[0], runs[1]) and torch.equal(runs[0], runs[2])
    pts_g = pts.clone().requires_grad_(True)
    (layer(pts_g, K.detach(), T) * weight).sum().backward()          # and the other way round
    assert pts_g.grad is not None and torch.isfinite(pts_g.grad).all()
    with pytest.raises(RuntimeError):
        layer(pts.cpu(), K.detach().cpu(), T.cpu())
    with pytest.raises(ValueError):
        TO.Project3D(b, h, w + 1)(pts, K.detach(), T)


# ======== the kernels at the C ABI: bits per pixel, a derived bound per entry of grad_P ====================================
@pytest.fixture(scope="module")
def L():
    _r3d()
    return importlib.import_module(PKG + "._lib")


@pytest.fixture(scope="module")
def ctx():
    c = _r3d().Context(0)
    yield c
    c.close()


@pytest.fixture
def guard(ctx):
    """Guarded(...) buffers of test_gpu_bounds.py (1 MiB bands of a random pattern either side, checked on every read), on
    the module's context unless another is named; freed after the test."""
    from test_gpu_bounds import Guarded
    made = []

    def make(nbytes, off=0, data=None, seed=0, on=None):
        g = Guarded(on or ctx, nbytes, off, data, seed)
        made.append(g)
        return g
    yield make
    for g in made:
        g.free()


def _cus():
    import torch
    return torch.cuda.get_device_properties(0).multi_processor_count


# (kind, index) into project_ref.shapes(CUs): the stride cases depend on the device, so they are resolved inside the test
BACK_ONLY = [("back", i) for i in range(3)]
BOTH = [("both", i) for i in range(4)] + [("fwd", 0), ("fwd", 1), ("grad", 0), ("grad", 1)]


def _shape(case):
    kind, i = case
    cus = _cus()
    shape = dict(zip(("back", "both", "fwd", "grad"), PR.shapes(cus)))[kind][i]
    B, H, W = shape
    if kind == "fwd":          # more pixels than one pass of the capped grid covers, or the case has gone stale
        assert H * W > PR.FWD_CAP_PER_CU * cus * PR.THREADS, (shape, cus)
        assert PR.trips(H * W, PR.grid_width(H * W, cus, PR.FWD_CAP_PER_CU)) == 2 + i
    if kind == "grad":
        assert H * W > PR.GRAD_CAP_PER_CU * cus * PR.THREADS, (shape, cus)
        assert PR.trips(H * W, PR.grid_width(H * W, cus)) == (2, 4)[i]
    print("case %s on %d CUs: B, H, W = %s" % (case, cus, shape))
    return shape


def _bits(got, want, what):
    assert PR.eq_bits(got, want), "%s: (mismatches, first index, got, want) = %s" % (what, PR.first_mismatch(got, want))


def _upload(guard, inp, names, on=None, off=None):
    off = off or {}
    return {n: guard(inp[n].nbytes, off.get(n, 0), inp[n], seed=1 + i, on=on) for i, n in enumerate(names)}


def _backproject(ctx, L, guard, inp, shape):
    """Both BackprojectDepth entry points on guarded buffers: cam_points [B][4][hw], grad_depth [B][hw]."""
    B, H, W = shape
    hw = H * W
    d = _upload(guard, inp, ("depth", "inv_K", "gcam"), on=ctx)
    cam, gdep = guard(B * 4 * hw * 4, seed=10, on=ctx), guard(B * hw * 4, seed=11, on=ctx)
    L.check(ctx.lib.r3d_backproject_depth_f32(ctx.handle, d["depth"].ptr, d["inv_K"].ptr, B, H, W, cam.ptr))
    L.check(ctx.lib.r3d_backproject_depth_grad_f32(ctx.handle, d["gcam"].ptr, d["inv_K"].ptr, B, H, W, gdep.ptr))
    out = cam.read(np.float32, (B, 4, hw)), gdep.read(np.float32, (B, hw))
    for b in d.values():
        b.unchanged()
    return out


def _project(ctx, L, guard, inp, shape, pix_off=0):
    """Both Project3D entry points on guarded buffers; the float2 planes (d_pix, d_grad_pix) at +pix_off bytes."""
    B, H, W = shape
    hw = H * W
    d = _upload(guard, inp, ("points", "P", "gpix"), on=ctx, off={"gpix": pix_off})
    pix, gpts, gP = guard(B * hw * 8, pix_off, seed=12, on=ctx), guard(B * 4 * hw * 4, seed=13, on=ctx), guard(B * 48, seed=14, on=ctx)
    eps = C.c_float(PR.EPS)
    L.check(ctx.lib.r3d_project3d_f32(ctx.handle, d["points"].ptr, d["P"].ptr, B, H, W, eps, pix.ptr))
    L.check(ctx.lib.r3d_project3d_grad_f32(ctx.handle, d["gpix"].ptr, d["points"].ptr, d["P"].ptr, B, H, W, eps, gpts.ptr, gP.ptr))
    out = pix.read(np.float32, (B, H, W, 2)), gpts.read(np.float32, (B, 4, hw)), gP.read(np.float32, (B, 3, 4))
    for b in d.values():
        b.unchanged()
    return out


def _check_backproject_bits(inp, shape, cam, gdep):
    B, H, W = shape
    _bits(cam, PR.cam_points_f32(inp["depth"], inp["inv_K"], H, W), "cam_points")
    assert np.array_equal(cam[:, 3].view(np.uint32), np.full((B, H * W), 0x3F800000, np.uint32)), "the ones plane is not exactly 1.0f"
    _bits(gdep, PR.grad_depth_f32(inp["gcam"], inp["inv_K"], H, W), "grad_depth")


def _check_project_bits(inp, shape, pix, gpts):
    B, H, W = shape
    _bits(pix, PR.pix_f32(inp["points"], inp["P"], H, W), "pix")
    _bits(gpts, PR.grad_points_f32(inp["gpix"], inp["points"], inp["P"], H, W), "grad_points")


def _check_grad_P(inp, shape, gP):
    """Every one of the 12 x B entries on its own: no normalisation by the largest."""
    B, H, W = shape
    a = (inp["gpix"], inp["points"], inp["P"], H, W)
    want = PR.grad_P_f64(*a)[0]
    bound = PR.grad_P_bound(*a, PR.grid_width(H * W, _cus()))
    err = np.abs(gP.astype(np.float64) - want)
    worst = np.unravel_index(np.argmax(err / bound), err.shape)
    print("grad_P %s: worst err / bound = %.3f at %s" % (shape, err[worst] / bound[worst], worst))
    assert np.all(err <= bound), (worst, gP[worst], want[worst], err[worst], bound[worst])


# ---- 1. per-pixel outputs, bit for bit ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", BACK_ONLY + BOTH)
def test_per_pixel_outputs_bit_for_bit(ctx, L, guard, case):
    shape = _shape(case)
    inp = PR.dense_inputs(*shape)
    _check_backproject_bits(inp, shape, *_backproject(ctx, L, guard, inp, shape))
    if case in BOTH:
        pix, gpts, _ = _project(ctx, L, guard, inp, shape)
        _check_project_bits(inp, shape, pix, gpts)


@pytest.mark.parametrize("pix_off", [8, 4])
def test_float2_planes_at_an_offset(ctx, L, guard, pix_off):
    """d_pix and d_grad_pix at +8 (float2-aligned, not 16-byte aligned) and at +4 (aligned for float only)."""
    shape = PR.DENSE_CASE
    inp = PR.dense_inputs(*shape)
    pix, gpts, gP = _project(ctx, L, guard, inp, shape, pix_off)
    _check_project_bits(inp, shape, pix, gpts)
    _bits(gP, _project(ctx, L, guard, inp, shape)[2], "grad_P against the call at offset 0")


# ---- 2. grad_P per entry --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", BOTH)
def test_grad_P_per_entry_repeatable_and_batch_independent(ctx, L, guard, case):
    shape = _shape(case)
    B, H, W = shape
    inp = PR.dense_inputs(*shape)
    d = _upload(guard, inp, ("points", "P", "gpix"))
    eps, runs = C.c_float(PR.EPS), []
    for r in range(3):
        gP = guard(B * 48, seed=20 + r)
        L.check(ctx.lib.r3d_project3d_grad_f32(ctx.handle, d["gpix"].ptr, d["points"].ptr, d["P"].ptr, B, H, W, eps, None, gP.ptr))
        runs.append(gP.read(np.float32, (B, 3, 4)))
    _check_grad_P(inp, shape, runs[0])
    _bits(runs[1], runs[0], "second call")
    _bits(runs[2], runs[0], "third call")
    for b in range(B if B > 1 else 0):          # the raster is the same, so are the grid width and the order of the sums
        one = {n: inp[n][b:b + 1] for n in ("points", "P", "gpix")}
        e = _upload(guard, one, ("points", "P", "gpix"))
        gP = guard(48, seed=30 + b)
        L.check(ctx.lib.r3d_project3d_grad_f32(ctx.handle, e["gpix"].ptr, e["points"].ptr, e["P"].ptr, 1, H, W, eps, None, gP.ptr))
        _bits(gP.read(np.float32, (1, 3, 4)), runs[0][b:b + 1], "image %d alone" % b)


# ---- 3. optional outputs --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", [("both", 2), ("grad", 0)])
def test_optional_outputs_give_the_bits_of_the_full_call(ctx, L, guard, case):
    shape = _shape(case)
    B, H, W = shape
    hw = H * W
    inp = PR.dense_inputs(*shape)
    _, gpts, gP = _project(ctx, L, guard, inp, shape)
    d = _upload(guard, inp, ("points", "P", "gpix"))
    eps = C.c_float(PR.EPS)
    args = (ctx.handle, d["gpix"].ptr, d["points"].ptr, d["P"].ptr, B, H, W, eps)
    only_pts, only_P = guard(B * 4 * hw * 4, seed=40), guard(B * 48, seed=41)
    L.check(ctx.lib.r3d_project3d_grad_f32(*args, only_pts.ptr, None))
    L.check(ctx.lib.r3d_project3d_grad_f32(*args, None, only_P.ptr))
    _bits(only_pts.read(np.float32, (B, 4, hw)), gpts, "grad_points without grad_P")
    _bits(only_P.read(np.float32, (B, 3, 4)), gP, "grad_P without grad_points")
    by_pts, by_P = guard(B * 4 * hw * 4, seed=42), guard(B * 48, seed=43)            # what the call with no output must not touch
    assert ctx.lib.r3d_project3d_grad_f32(*args, None, None) == L.OK
    by_pts.unchanged()
    by_P.unchanged()
    for b in d.values():
        b.unchanged()


# ---- 4. special values, bit for bit ---------------------------------------------------------------------------------------------
def _special_inputs():
    """2 x 130 raster, two images.  P_23 = -0.5 and px = py = pz = 0 at the chosen pixels make c2 = -0.5 * pw exactly:
       pixel 0   pw = 2 eps: c2 == -eps, den == 0 exactly        pixel 1 / 2   den = +1e-6 / -1e-6 (to f32 rounding)
       pixels 3, 4, 5   depth = +inf, -inf, NaN                  image 1: P_01 = NaN"""
    B, H, W = 2, 2, 130
    inp = PR.dense_inputs(B, H, W, seed=4)
    eps = PR.EPS
    inp["P"][:, 2, 3] = -0.5
    x = inp["points"]
    x[:, :3, :3] = 0.0
    x[:, 3, 0] = np.float32(2) * eps
    x[:, 3, 1] = np.float32(-2) * (np.float32(1e-6) - eps)
    x[:, 3, 2] = np.float32(-2) * (np.float32(-1e-6) - eps)
    inp["depth"][:, 3:6] = (np.inf, -np.inf, np.nan)
    inp["P"][1, 0, 1] = np.nan
    return (B, H, W), inp


def test_special_values_bit_for_bit(ctx, L, guard):
    shape, inp = _special_inputs()
    B, H, W = shape
    a = (inp["gpix"], inp["points"], inp["P"], H, W)
    c, den, inv, d = PR.chain_f32(*a)
    assert np.all(c[:, 2, 0] == -PR.EPS) and np.all(den[:, 0] == 0)                       # den == 0 exactly, in NumPy first
    assert np.all(np.abs(den[:, 1] - 1e-6) < 1e-9) and np.all(np.abs(den[:, 2] + 1e-6) < 1e-9)
    want = dict(cam=PR.cam_points_f32(inp["depth"], inp["inv_K"], H, W), gdep=PR.grad_depth_f32(inp["gcam"], inp["inv_K"], H, W),
                pix=PR.pix_f32(*a[1:]), gpts=PR.grad_points_f32(*a))
    tiny = np.finfo(np.float32).tiny
    for name, v in list(want.items()) + [("c", c), ("den", den), ("inv", inv), ("d", d)]:     # no subnormal anywhere
        f = np.isfinite(v) & (v != 0)
        assert np.all(np.abs(v[f]) >= tiny), name
    assert np.isinf(want["pix"][0, 0, 0]).all() and np.isinf(want["cam"][0, :3, 3:5]).all() and np.isnan(want["cam"][0, :3, 5]).all()
    assert not np.isnan(want["pix"][0]).any() and np.isnan(want["pix"][1, ..., 0]).all() and not np.isnan(want["pix"][1, ..., 1]).any()
    assert np.isnan(want["gpts"][0]).sum() < np.isnan(want["gpts"][1]).sum()
    cam, gdep = _backproject(ctx, L, guard, inp, shape)
    pix, gpts, _ = _project(ctx, L, guard, inp, shape)
    _check_backproject_bits(inp, shape, cam, gdep)          # eq_bits compares the NaN masks: image 0 holds no NaN that the
    _check_project_bits(inp, shape, pix, gpts)              # restatement does not predict, image 1 exactly the predicted ones


# ---- 5. limits ------------------------------------------------------------------------------------------------------------------
def test_batch_65535_runs_all_four_entry_points(ctx, L, guard):
    shape = PR.BIG_BATCH
    inp = PR.dense_inputs(*shape)
    _check_backproject_bits(inp, shape, *_backproject(ctx, L, guard, inp, shape))
    pix, gpts, gP = _project(ctx, L, guard, inp, shape)
    _check_project_bits(inp, shape, pix, gpts)
    _check_grad_P(inp, shape, gP)


def _refused(L, rc, outs):
    assert rc == L.ERR_INVALID, rc
    assert L.last_error() != ""
    for o in outs:
        o.unchanged()


def test_limits_and_refusals_write_nothing(ctx, L, guard):
    shape = (1, 2, 2)
    B, H, W = shape
    inp = PR.dense_inputs(*shape)
    d = _upload(guard, inp, ("depth", "inv_K", "gcam", "points", "P", "gpix"))
    cam, gdep, pix, gpts, gP = (guard(n, seed=50 + i) for i, n in enumerate((64, 16, 32, 64, 48)))
    outs = (cam, gdep, pix, gpts, gP)
    eps, lib, h = C.c_float(PR.EPS), ctx.lib, ctx.handle

    def calls(batch, height, width, z=None):
        """The four entry points, not yet called; z = (entry point, argument) names one pointer to pass as NULL."""
        p = lambda e, i, buf: None if z == (e, i) else buf.ptr
        return [lambda: lib.r3d_backproject_depth_f32(h, p(0, 0, d["depth"]), p(0, 1, d["inv_K"]), batch, height, width, p(0, 2, cam)),
                lambda: lib.r3d_backproject_depth_grad_f32(h, p(1, 0, d["gcam"]), p(1, 1, d["inv_K"]), batch, height, width,
                                                           p(1, 2, gdep)),
                lambda: lib.r3d_project3d_f32(h, p(2, 0, d["points"]), p(2, 1, d["P"]), batch, height, width, eps, p(2, 2, pix)),
                lambda: lib.r3d_project3d_grad_f32(h, p(3, 0, d["gpix"]), p(3, 1, d["points"]), p(3, 2, d["P"]), batch, height,
                                                   width, eps, gpts.ptr, gP.ptr)]

    for call in calls(0, H, W):                                           # batch = 0: R3D_OK, nothing written
        assert call() == L.OK
    for o in outs:
        o.unchanged()
    for call in calls(65536, H, W):                                       # one more than grid.y holds
        _refused(L, call(), outs)
    for e in range(4):                                                    # each required pointer in turn
        for i in range(3):
            _refused(L, calls(B, H, W, z=(e, i))[e](), outs)
    for height, width in ((1, 2), (2, 1)):                                # Project3D divides by (W-1) and (H-1) ...
        for call in calls(B, height, width)[2:]:
            _refused(L, call(), outs)
    for b in d.values():
        b.unchanged()
    for height, width in ((1, 2), (2, 1)):                                # ... and BackprojectDepth does not
        for call in calls(B, height, width)[:2]:
            assert call() == L.OK
    cam.bytes(), gdep.bytes()


# ---- 6. the torch layers: views, offsets, expanded gradients, and the way to K.grad and T.grad -------------------------------
def _np(t):
    return t.detach().cpu().contiguous().numpy()


def test_layers_on_views_give_the_bits_of_the_contiguous_call():
    import torch
    TO = importlib.import_module(PKG + ".torch_ops")
    dev = torch.device("cuda", 0)
    B, H, W = PR.DENSE_CASE
    hw = H * W
    inp = PR.dense_inputs(B, H, W)
    t = lambda a: torch.from_numpy(a).to(dev)
    bp, pj = TO.BackprojectDepth(B, H, W), TO.Project3D(B, H, W, eps=float(PR.EPS))
    gcam, gpix = t(inp["gcam"]), t(inp["gpix"])

    depth = t(inp["depth"]).view(B, 1, H, W).requires_grad_(True)
    cam = bp(depth, t(inp["inv_K"]))
    cam.backward(gcam)
    _bits(_np(cam), PR.cam_points_f32(inp["depth"], inp["inv_K"], H, W), "layer cam_points")
    _bits(_np(depth.grad).reshape(B, hw), PR.grad_depth_f32(inp["gcam"], inp["inv_K"], H, W), "layer grad_depth")

    big = torch.zeros((B, 1, H, 2 * W), device=dev)
    big[..., ::2] = depth.detach()
    big.requires_grad_(True)
    store = torch.zeros(1 + B * 16, device=dev)
    store[1:] = t(inp["inv_K"]).reshape(-1)
    k_twice = store[1:].view(B, 4, 4).transpose(1, 2).transpose(1, 2)                  # contiguous strides, storage offset 1
    store_t = torch.zeros(3 + B * 16, device=dev)
    store_t[3:] = t(inp["inv_K"]).transpose(1, 2).reshape(-1)
    k_once = store_t[3:].view(B, 4, 4).transpose(1, 2)                                 # the same numbers, column-major
    assert k_twice.storage_offset() == 1 and not k_once.is_contiguous() and torch.equal(k_once, k_twice)
    for k in (k_twice, k_once):
        big.grad = None
        view = big[..., ::2]
        assert not view.is_contiguous()
        out = bp(view, k)
        out.backward(gcam)
        _bits(_np(out), _np(cam), "cam_points from views")
        _bits(_np(big.grad[..., ::2]), _np(depth.grad), "grad_depth through the view")
        assert float(big.grad[..., 1::2].abs().max()) == 0.0

    K = torch.zeros((B, 4, 4), device=dev)
    K[:, :3, :], K[:, 3, 3] = t(inp["P"]), 1.0
    T = torch.eye(4, device=dev).repeat(B, 1, 1)                                       # K @ I is K exactly
    pts = t(inp["points"]).requires_grad_(True)
    pix = pj(pts, K, T)
    pix.backward(gpix)
    _bits(_np(pix), PR.pix_f32(inp["points"], inp["P"], H, W), "layer pix")
    _bits(_np(pts.grad), PR.grad_points_f32(inp["gpix"], inp["points"], inp["P"], H, W), "layer grad_points")
    flat = torch.zeros(1 + B * 4 * hw, device=dev)
    flat[1:] = pts.detach().reshape(-1)
    pts_off = flat[1:].view(B, 4, hw).detach().requires_grad_(True)
    assert pts_off.storage_offset() == 1 and pts_off.data_ptr() % 8 == 4
    pix_off = pj(pts_off, K, T)
    pix_off.backward(gpix)
    _bits(_np(pix_off), _np(pix), "pix from points at a storage offset")
    _bits(_np(pts_off.grad), _np(pts.grad), "grad_points from points at a storage offset")

    # out.sum().backward() hands the backward an expanded gradient of stride 0
    for layer, args, leaf in ((bp, (depth, t(inp["inv_K"])), depth), (pj, (pts, K, T), pts)):
        grads = []
        for expanded in (True, False):
            leaf.grad = None
            out = layer(*args)
            if expanded:
                out.sum().backward()
            else:
                out.backward(torch.ones_like(out))
            grads.append(_np(leaf.grad))
        _bits(grads[0], grads[1], "gradient from an expanded grad_output")


def test_K_and_T_gradients_are_torchs_matmul_backward_of_grad_P():
    """Project3D forms P = (K @ T)[:, :3, :] in torch, so K.grad = pad(grad_P) @ T^T and T.grad = K^T @ pad(grad_P): each
    entry a four-term dot product of f32 numbers, within 4 u sum|terms| (4 = one product and three additions on any path)
    of its float64 value -- whatever order torch's matmul adds in."""
    import torch
    TO = importlib.import_module(PKG + ".torch_ops")
    dev = torch.device("cuda", 0)
    B, H, W = PR.DENSE_CASE
    inp = PR.dense_inputs(B, H, W)
    rng = np.random.default_rng(6)
    T64 = np.eye(4) + 0.3 * rng.normal(size=(B, 4, 4))
    P4 = np.zeros((B, 4, 4))
    P4[:, :3, :], P4[:, 3, 3] = inp["P"], 1.0
    K32, T32 = (P4 @ np.linalg.inv(T64)).astype(np.float32), T64.astype(np.float32)     # K @ T is P to f32 rounding: den stays away from 0
    K, T = torch.from_numpy(K32).to(dev).requires_grad_(True), torch.from_numpy(T32).to(dev).requires_grad_(True)
    pts, gpix = torch.from_numpy(inp["points"]).to(dev), torch.from_numpy(inp["gpix"]).to(dev)
    TO.Project3D(B, H, W, eps=float(PR.EPS))(pts, K, T).backward(gpix)
    P = torch.matmul(K, T)[:, :3, :].detach().requires_grad_(True)
    TO._Project3DFn.apply(pts, P, B, H, W, float(PR.EPS)).backward(gpix)
    G = np.zeros((B, 4, 4))
    G[:, :3, :] = _np(P.grad)
    K64, T64 = K32.astype(np.float64), T32.astype(np.float64)
    for name, got, want, terms in (("K.grad", K.grad, np.einsum("bij,bkj->bik", G, T64), np.einsum("bij,bkj->bik", np.abs(G), np.abs(T64))),
                                   ("T.grad", T.grad, np.einsum("bji,bjk->bik", K64, G), np.einsum("bji,bjk->bik", np.abs(K64), np.abs(G)))):
        err = np.abs(_np(got).astype(np.float64) - want)
        assert np.all(err <= 4 * PR.U * terms), (name, float((err / (4 * PR.U * terms + 1e-300)).max()))
    assert float(K.grad[:, 3].abs().max()) == 0.0                                       # row 3 of K never reaches P


# ---- 7. streams -----------------------------------------------------------------------------------------------------------------
def test_layers_on_a_fresh_stream_give_the_bits_of_the_default_stream():
    import torch
    TO = importlib.import_module(PKG + ".torch_ops")
    dev = torch.device("cuda", 0)
    B, H, W = 2, 96, 320
    g = torch.Generator(device="cpu").manual_seed(7)
    base0 = (torch.rand((B, 1, H, W), generator=g) * 40 + 2.0).to(dev)
    K0 = torch.eye(4).repeat(B, 1, 1)
    K0[:, 0, 0], K0[:, 1, 1], K0[:, 0, 2], K0[:, 1, 2] = 0.58 * W, 1.92 * H, 0.5 * W, 0.5 * H
    inv_K, K0 = torch.linalg.inv(K0).to(dev), K0.to(dev)
    T0 = torch.eye(4).repeat(B, 1, 1)
    T0[:, :3, 3] = (torch.rand((B, 3), generator=g) - 0.5) * 0.6
    T0 = T0.to(dev)
    weight = torch.rand((B, H, W, 2), generator=g).to(dev)
    torch.cuda.synchronize()

    def run():
        base, K, T = base0.clone().requires_grad_(True), K0.clone().requires_grad_(True), T0.clone().requires_grad_(True)
        depth = (base * 1.5 + 0.25).sqrt() * 3.0 + torch.sin(base)          # produced on the current stream, consumed at once
        pts = TO.BackprojectDepth(B, H, W)(depth, inv_K)
        pix = TO.Project3D(B, H, W)(pts, K, T)
        (pix * weight).sum().backward()
        return pts.detach(), pix.detach(), base.grad, K.grad, T.grad

    default_ctx = TO._ctx_for(dev)
    first = run()
    torch.cuda.synchronize()
    s = torch.cuda.Stream(device=dev)
    with torch.cuda.stream(s):
        c = TO._ctx_for(dev)
        assert c.stream_handle() == s.cuda_stream != 0
        assert c is not default_ctx and c.handle != default_ctx.handle
        second = run()
    s.synchronize()
    assert TO._ctx_for(dev) is default_ctx
    for name, a, b in zip(("cam_points", "pix", "depth.grad", "K.grad", "T.grad"), first, second):
        _bits(_np(b), _np(a), name + " on the fresh stream")


# ---- 8. the trainer's sequence: four scales in turn on one context -----------------------------------------------------------
SCALES = [(2, 24, 80), (2, 48, 160), (2, 96, 320), (2, 192, 640)]


def _scale_buffers(c, guard, inp, shape, seed):
    B, H, W = shape
    hw = H * W
    d = _upload(guard, inp, ("depth", "inv_K", "gcam", "points", "P", "gpix"), on=c)
    sizes = dict(cam=B * 4 * hw * 4, pix=B * hw * 8, gpts=B * 4 * hw * 4, gP=B * 48, gdep=B * hw * 4)
    d.update({n: guard(sz, seed=seed + i, on=c) for i, (n, sz) in enumerate(sizes.items())})
    return d


def _forward(c, L, d, shape):
    B, H, W = shape
    L.check(c.lib.r3d_backproject_depth_f32(c.handle, d["depth"].ptr, d["inv_K"].ptr, B, H, W, d["cam"].ptr))
    L.check(c.lib.r3d_project3d_f32(c.handle, d["points"].ptr, d["P"].ptr, B, H, W, C.c_float(PR.EPS), d["pix"].ptr))


def _backward(c, L, d, shape):
    B, H, W = shape
    L.check(c.lib.r3d_project3d_grad_f32(c.handle, d["gpix"].ptr, d["points"].ptr, d["P"].ptr, B, H, W, C.c_float(PR.EPS),
                                         d["gpts"].ptr, d["gP"].ptr))
    L.check(c.lib.r3d_backproject_depth_grad_f32(c.handle, d["gcam"].ptr, d["inv_K"].ptr, B, H, W, d["gdep"].ptr))


OUTS = ("cam", "pix", "gpts", "gP", "gdep")


def test_four_scales_in_turn_on_one_context_match_each_scale_alone(ctx, L, guard):
    """All forwards, then all backwards in reverse order (what autograd makes of trainer.py:387-390 over its scales), three
    rounds without a synchronisation inside a round: the grad_P partials of all four scales pass through kWsPartials."""
    R = _r3d()
    inps = [PR.dense_inputs(*s, seed=8) for s in SCALES]
    alone = []
    for inp, shape in zip(inps, SCALES):
        with R.Context(0) as fresh:
            d = _scale_buffers(fresh, guard, inp, shape, 60)
            _forward(fresh, L, d, shape)
            _backward(fresh, L, d, shape)
            alone.append({n: d[n].read(np.uint32) for n in OUTS})
            for n in list(d):
                d.pop(n).free()
    bufs = [_scale_buffers(ctx, guard, inp, shape, 70) for inp, shape in zip(inps, SCALES)]
    for rnd in range(3):
        for d in bufs:
            for n in OUTS:                                                 # last round's results go: every round writes afresh
                L.check(ctx.lib.r3d_memset(ctx.handle, d[n].ptr, 0xA5, d[n].nbytes))
        for d, shape in zip(bufs, SCALES):
            _forward(ctx, L, d, shape)
        for d, shape in reversed(list(zip(bufs, SCALES))):
            _backward(ctx, L, d, shape)
        for i, d in enumerate(bufs):
            for n in OUTS:
                assert np.array_equal(d[n].read(np.uint32), alone[i][n]), "round %d, scale %s, %s" % (rnd, SCALES[i], n)
