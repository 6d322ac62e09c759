"""CPU: the NumPy statements of the torch-facing projection kernels (project_ref.py) against an independent derivation, and
what the GPU tests take for granted about their own inputs.

  1. The float64 functions agree with upstream monodepth2's layers, written statement for statement in CPU float64 torch, and
     with torch AUTOGRAD's gradients for depth, points and P: the hand-written gradient formulas are derived a second time.
  2. On every input set of the GPU tests (project_ref.shapes at the MI355X's 256 compute units, and the 65535-image batch)
     the f32 restatements lie within a first-order running error bound of the float64 values, the rounding count k of
     grad_P_bound covers the f32 error of the terms themselves, and the per-entry bound is tighter than the tolerance it
     replaces (2e-4 of the largest entry) -- and, on the dense case, below 1e-2 of every single entry.
  3. The float64 reference can fail: four deliberate defects each break the bound on the dense case.
"""
import numpy as np
import pytest

import project_ref as PR

U = PR.U


# ---- 1. upstream layers in float64 torch, and autograd ---------------------------------------------------------------------
def reference_backproject(depth, inv_K, batch, height, width):
    """upstream monodepth2 layers.BackprojectDepth, statement for statement (float64, CPU)."""
    import torch
    meshgrid = np.meshgrid(range(width), range(height), indexing="xy")
    id_coords = torch.from_numpy(np.stack(meshgrid, axis=0).astype(np.float64))
    ones = torch.ones(batch, 1, height * width, dtype=torch.float64)
    pix_coords = torch.unsqueeze(torch.stack([id_coords[0].view(-1), id_coords[1].view(-1)], 0), 0)
    pix_coords = pix_coords.repeat(batch, 1, 1)
    pix_coords = torch.cat([pix_coords, ones], 1)
    cam_points = torch.matmul(inv_K[:, :3, :3], pix_coords)
    cam_points = depth.view(batch, 1, -1) * cam_points
    return torch.cat([cam_points, ones], 1)


def reference_project3d(points, K, T, batch, height, width, eps):
    """upstream monodepth2 layers.Project3D.forward, statement for statement (float64, CPU)."""
    import torch
    P = torch.matmul(K, T)[:, :3, :]
    cam_points = torch.matmul(P, points)
    pix_coords = cam_points[:, :2, :] / (cam_points[:, 2, :].unsqueeze(1) + eps)
    pix_coords = pix_coords.view(batch, 2, height, width)
    pix_coords = pix_coords.permute(0, 2, 3, 1)
    pix_coords[..., 0] /= width - 1
    pix_coords[..., 1] /= height - 1
    return (pix_coords - 0.5) * 2


def _rel(got, want):
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    scale = np.maximum(np.abs(got), np.abs(want))
    return float(np.max(np.where(scale > 0, np.abs(got - want) / np.where(scale > 0, scale, 1), 0.0)))


@pytest.mark.parametrize("shape", [(1, 2, 2), PR.DENSE_CASE, (2, 5, 51)])
def test_f64_statements_agree_with_upstream_layers_and_autograd(shape):
    import torch
    B, H, W = shape
    inp = PR.dense_inputs(B, H, W)
    t64 = lambda a: torch.from_numpy(np.asarray(a, np.float32).astype(np.float64))
    eps = float(PR.EPS)

    depth = t64(inp["depth"]).view(B, 1, H, W).requires_grad_(True)
    cam = reference_backproject(depth, t64(inp["inv_K"]), B, H, W)
    assert _rel(PR.cam_points_f64(inp["depth"], inp["inv_K"], H, W), cam.detach().numpy()) <= 1e-12
    cam.backward(t64(inp["gcam"]))
    assert _rel(PR.grad_depth_f64(inp["gcam"], inp["inv_K"], H, W), depth.grad.view(B, -1).numpy()) <= 1e-12

    points = t64(inp["points"]).requires_grad_(True)
    K = torch.zeros(B, 4, 4, dtype=torch.float64)
    K[:, :3, :], K[:, 3, 3] = t64(inp["P"]), 1.0                 # K @ I, so that P itself is the leaf behind (K @ T)[:, :3, :]
    K.requires_grad_(True)
    T = torch.eye(4, dtype=torch.float64).repeat(B, 1, 1)
    pix = reference_project3d(points, K, T, B, H, W, eps)
    assert _rel(PR.pix_f64(inp["points"], inp["P"], H, W), pix.detach().numpy()) <= 1e-12
    pix.backward(t64(inp["gpix"]))
    assert _rel(PR.grad_points_f64(inp["gpix"], inp["points"], inp["P"], H, W), points.grad.numpy()) <= 1e-12
    want_P, _ = PR.grad_P_f64(inp["gpix"], inp["points"], inp["P"], H, W)
    assert _rel(want_P, K.grad[:, :3, :].numpy()) <= 1e-12
    assert float(K.grad[:, 3, :].abs().max()) == 0.0


# ---- 2. the input sets of the GPU tests ----------------------------------------------------------------------------------
def running_error(inp, H, W):
    """First-order bounds of |f32 restatement - f64 value| per entry, in the form m * u * sum|terms| applied step by step
    (the standard running error analysis: a rounding of a sum is charged against the absolute values of its terms):
      a dot product of n terms          n * u * sum|terms|             (1 for each product, n - 1 additions)
      a product or quotient a o b       |b'| E_a + |a'| E_b + u |a o b|
    Returns dict(cam, gdepth, pix, gpoints)."""
    B, hw = inp["depth"].shape[0], H * W
    k = np.abs(inp["inv_K"].astype(np.float64))
    fx, fy = PR._xy(H, W, np.float64)
    A_r = np.stack([k[:, c, 0:1] * fx + k[:, c, 1:2] * fy + k[:, c, 2:3] for c in range(3)], 1)
    z = np.abs(inp["depth"].astype(np.float64)).reshape(B, 1, hw)
    g = np.abs(inp["gcam"].astype(np.float64))[:, :3]
    out = dict(cam=4 * U * z * A_r,                                    # 3 for the ray, 1 for z * ray
               gdepth=6 * U * (g * A_r).sum(1))                        # 3 for each ray, 1 product, 2 additions
    if H < 2 or W < 2:
        return out
    x, m = inp["points"].astype(np.float64), inp["P"].astype(np.float64)
    c, den, d = PR.chain_f64(inp["gpix"], inp["points"], inp["P"], H, W)
    A = PR._c(np.abs(m), np.abs(x))                                    # sum|P_ik x_k|
    E_c = 4 * U * A
    aden = np.abs(den)
    E_den = E_c[:, 2] + U * aden
    E_pix = []
    for i, n1 in ((0, W - 1), (1, H - 1)):
        q = np.abs(c[:, i]) / aden
        E_q = E_c[:, i] / aden + q * E_den / aden + U * q
        r = c[:, i] / den / n1
        E_pix.append(2 * (E_q / n1 + U * np.abs(r) + U * np.abs(r - 0.5)))
    out["pix"] = np.stack(E_pix, -1).reshape(B, H, W, 2)
    inv = 1 / aden
    E_inv = E_den * inv * inv + U * inv
    ad = np.abs(d)
    E_d = np.empty_like(d)
    for i in (0, 1):
        gs = ad[:, i] * aden                                           # |g * gw|, 2 roundings
        E_d[:, i] = gs * E_inv + 2 * U * ad[:, i] + U * ad[:, i]
    prod = ad[:, 0] * np.abs(c[:, 0]) + ad[:, 1] * np.abs(c[:, 1])
    E_s = np.abs(c[:, 0]) * E_d[:, 0] + ad[:, 0] * E_c[:, 0] + np.abs(c[:, 1]) * E_d[:, 1] + ad[:, 1] * E_c[:, 1] + 2 * U * prod
    s = ad[:, 2] * aden
    E_d[:, 2] = inv * E_s + s * E_inv + U * ad[:, 2]
    am = np.abs(m)
    out["gpoints"] = np.einsum("bik,bip->bkp", am, E_d) + 3 * U * np.einsum("bik,bip->bkp", am, ad)
    return out


def _input_sets():
    back_only, both, fwd, grad = PR.shapes(PR.MI355X_CUS)
    return [(s, False) for s in back_only] + [(s, True) for s in both + fwd + grad + [PR.BIG_BATCH]]


@pytest.mark.parametrize("shape,project", _input_sets())
def test_input_set_rounding_sanity_and_bound_not_weaker(shape, project):
    B, H, W = shape
    inp = PR.dense_inputs(B, H, W)
    depth = inp["depth"]
    assert (depth < 0).any() or H * W < 3
    if H * W >= 2:
        assert np.array_equal(depth[:, :2].view(np.uint32), np.tile(np.array([0, 0x80000000], np.uint32), (B, 1)))
    blk = inp["inv_K"][:, :3, :3]
    assert (blk < 0).any() and (blk > 0).any() and 1e-3 * 0.999 <= np.abs(blk).min() and np.abs(blk).max() <= 1.0
    E = running_error(inp, H, W)
    # rounding sanity: restatement vs float64, m * u * sum|terms|
    assert np.all(np.abs(PR.cam_points_f32(depth, inp["inv_K"], H, W)[:, :3] - PR.cam_points_f64(depth, inp["inv_K"], H, W)[:, :3])
                  <= E["cam"])
    assert np.all(np.abs(PR.grad_depth_f32(inp["gcam"], inp["inv_K"], H, W) - PR.grad_depth_f64(inp["gcam"], inp["inv_K"], H, W))
                  <= E["gdepth"])
    if not project:
        return
    a = (inp["gpix"], inp["points"], inp["P"], H, W)
    den32 = PR.chain_f32(*a)[1]
    assert (den32 > 0).any() and (den32 < 0).any() and np.abs(den32).min() >= PR.DEN_MIN
    assert (inp["P"] < 0).any() and (inp["P"] > 0).any() and (inp["points"][:, :3] < 0).any()
    assert inp["points"][:, 3].min() >= 0.5 and inp["points"][:, 3].max() <= 2.0
    assert np.all(np.abs(PR.pix_f32(*a[1:]) - PR.pix_f64(*a[1:])) <= E["pix"])
    assert np.all(np.abs(PR.grad_points_f32(*a) - PR.grad_points_f64(*a)) <= E["gpoints"])
    # the k of the bound covers the f32 error of the terms themselves on this very set:
    #     sum_p |f32(d_i x_k) - d_i x_k| <= k u sum_p |d_i x_k|
    # (a count of roundings bounds a relative error only where no sum on the way cancels; this is that premise, checked).
    # With it, |got - want| <= [this] + n u sum|terms| + u |want| is all a correct kernel can be off by.
    want, abs_sum = PR.grad_P_f64(*a)
    d32, d64, x = PR.chain_f32(*a)[3], PR.chain_f64(*a)[2], inp["points"]
    err = np.stack([np.abs((d32[:, i] * x[:, k]).astype(np.float64) - d64[:, i] * x[:, k].astype(np.float64)).sum(-1)
                    for i in range(3) for k in range(4)], -1).reshape(B, 3, 4)
    cover = err / (U * abs_sum)
    assert np.all(cover <= PR.K_ROUNDINGS[None, :, None]), cover.max((0, 2))
    # the new bound is never weaker than the old one
    width = PR.grid_width(H * W, PR.MI355X_CUS)
    bound = PR.grad_P_bound(*a, width)
    assert np.all(bound < 2e-4 * np.abs(want).max()), float((bound / np.abs(want).max()).max())
    if shape == PR.DENSE_CASE:
        assert np.all(bound < 1e-2 * np.abs(want)), float((bound / np.abs(want)).max())


def test_stride_cases_take_the_trips_they_are_named_for():
    cus = PR.MI355X_CUS
    _, _, fwd, grad = PR.shapes(cus)
    for (B, H, W), want in zip(fwd, (2, 3)):
        assert H * W > PR.FWD_CAP_PER_CU * cus * PR.THREADS
        assert PR.trips(H * W, PR.grid_width(H * W, cus, PR.FWD_CAP_PER_CU)) == want and (H * W) % PR.THREADS
    for (B, H, W), want in zip(grad, (2, 4)):
        assert H * W > PR.GRAD_CAP_PER_CU * cus * PR.THREADS
        assert PR.trips(H * W, PR.grid_width(H * W, cus)) == want and (H * W) % PR.THREADS


def test_eq_bits():
    a = np.array([1.0, -0.0, np.nan, np.inf], np.float32)
    b = a.copy()
    b.view(np.uint32)[2] = 0xFFC00001                                  # another NaN: sign and payload are not compared
    assert PR.eq_bits(b, a) and PR.first_mismatch(b, a) == (0,)
    b[1] = 0.0
    assert not PR.eq_bits(b, a) and PR.first_mismatch(b, a)[:2] == (1, 1)
    b[1], b[3] = -0.0, np.nan
    assert not PR.eq_bits(b, a)
    assert not PR.eq_bits(np.nextafter(a, np.float32(2)), a)


# ---- 3. the references can fail ------------------------------------------------------------------------------------------
def _dense():
    B, H, W = PR.DENSE_CASE
    inp = PR.dense_inputs(B, H, W)
    a = (inp["gpix"], inp["points"], inp["P"], H, W)
    return inp, a, PR.grad_P_f64(*a)[0], PR.grad_P_bound(*a, PR.grid_width(H * W, PR.MI355X_CUS))


def _swapped_P(inp):
    P = inp["P"].copy()
    P[:, 0, 1], P[:, 1, 0] = inp["P"][:, 1, 0], inp["P"][:, 0, 1]
    return P


def _pw_one(inp):
    x = inp["points"].copy()
    x[:, 3] = 1.0
    return x


MUTATIONS = {
    "two P entries swapped": lambda inp, H, W: PR.grad_P_f64(inp["gpix"], inp["points"], _swapped_P(inp), H, W)[0],
    "pw forced to 1": lambda inp, H, W: PR.grad_P_f64(inp["gpix"], _pw_one(inp), inp["P"], H, W)[0],
    "gw and gh exchanged": lambda inp, H, W: PR.grad_P_f64(inp["gpix"], inp["points"], inp["P"], W, H)[0],
    "a dropped d2 term": lambda inp, H, W: PR.grad_P_f64(inp["gpix"], inp["points"], inp["P"], H, W, drop_d1c1=True)[0],
}


@pytest.mark.parametrize("name", sorted(MUTATIONS))
def test_mutated_reference_breaks_the_bound_on_the_dense_case(name):
    inp, a, want, bound = _dense()
    _, H, W = PR.DENSE_CASE
    assert H != W
    mutant = MUTATIONS[name](inp, H, W)
    assert mutant.shape == want.shape
    assert np.any(np.abs(mutant - want) > bound), name
