"""CPU: the depth bilateral filter's weight tables (r3d_bilateral_weights: host only, no GPU) against np.exp, the argument errors
of both C entries and of their Python wrappers, the properties of tests/bilateral_ref.py (the NumPy restatement of include/r3d.h
"Depth bilateral filter" the GPU tests compare with), and what the filter is for: on a noisy frame of the room scene the organised
normals are closer to the clean frame's with the filter than without (the figures: DESIGN.md section 4.5q)."""
import ctypes as C
import importlib

import numpy as np
import pytest

import bilateral_ref as BR
import pyramid_ref as PR
from helpers import PKG

F = np.float32


@pytest.fixture(scope="module")
def L():
    return importlib.import_module(PKG + "._lib")


@pytest.fixture(scope="module")
def tracking():
    return importlib.import_module(PKG + ".tracking")


def bits(a):
    return np.ascontiguousarray(a, dtype=F).view(np.uint32)


def ulps(a, b):
    """distance in f32 steps between two arrays of non-negative finite floats"""
    return np.abs(bits(a).astype(np.int64) - bits(b).astype(np.int64))


@pytest.mark.parametrize("radius,sigma_s,sigma_r", [(0, 1.0, 1.0), (1, 0.5, 0.01), (3, 2.0, 0.05), (8, 4.5, 0.1), (8, 0.3, 7.0), (5, 1e3, 1e-3)])
def test_weights_against_numpy(tracking, radius, sigma_s, sigma_r):
    spatial, rng, cut, inv_step = tracking.bilateral_weights(radius, sigma_s, sigma_r)
    want_s, want_r, want_cut, want_inv = BR.weights(radius, sigma_s, sigma_r)
    assert spatial.shape == (2 * radius + 1, 2 * radius + 1) and spatial.dtype == F and rng.shape == (256,) and rng.dtype == F
    # exp is not correctly rounded everywhere: one f32 step between two libms, no more
    assert ulps(spatial, want_s).max() <= 1 and ulps(rng, want_r).max() <= 1
    assert rng[0] == 1.0 and spatial[radius, radius] == 1.0
    assert F(cut) == want_cut == F(3.0 * sigma_r) and F(inv_step) == want_inv == F(256.0 / (3.0 * sigma_r))
    assert np.all(np.diff(rng) < 0) and rng[255] > 0                    # the left edges of the bins of exp(-t^2 / 2) on [0, 3)
    assert np.array_equal(spatial, spatial.T) and np.array_equal(spatial, spatial[::-1, ::-1])
    # the same numbers on a repeat
    again = tracking.bilateral_weights(radius, sigma_s, sigma_r)
    assert again[0].tobytes() == spatial.tobytes() and again[1].tobytes() == rng.tobytes() and again[2:] == (cut, inv_step)


def test_argument_errors_without_gpu(L, tracking):
    lib = L.load()
    spatial, rng = np.full(17 * 17, 7.0, dtype=F), np.full(256, 7.0, dtype=F)
    cut, inv_step = C.c_float(7.0), C.c_float(7.0)
    good = dict(r=3, ss=2.0, sr=0.05, sp=spatial.ctypes.data, rg=rng.ctypes.data, cut=C.addressof(cut), inv=C.addressof(inv_step))
    order = ["r", "ss", "sr", "sp", "rg", "cut", "inv"]
    inf, nan = float("inf"), float("nan")
    bad = [dict(r=-1), dict(r=-1, ss=0.0, sr=0.0), dict(r=9), dict(r=1 << 30), dict(ss=0.0), dict(ss=-1.0), dict(ss=inf), dict(ss=nan), dict(sr=0.0), dict(sr=-0.05),
           dict(sr=inf), dict(sr=nan), dict(sr=1e-40), dict(sr=1e39), dict(sp=None), dict(rg=None), dict(cut=None), dict(inv=None)]
    for b in bad:
        a = {**good, **b}
        assert lib.r3d_bilateral_weights(*[a[k] for k in order]) == L.ERR_INVALID, b
    assert np.all(spatial == 7.0) and np.all(rng == 7.0) and cut.value == 7.0 and inv_step.value == 7.0
    assert lib.r3d_bilateral_weights(*[good[k] for k in order]) == L.OK
    assert np.all(spatial[:49] != 7.0) and np.all(spatial[49:] == 7.0) and cut.value == F(0.15)
    # the device call refuses a NULL context before it looks at anything else
    assert lib.r3d_depth_bilateral(None, rng.ctypes.data, 1, 4, 4, 1, 1.0, 1.0, spatial.ctypes.data) == L.ERR_INVALID
    # the wrappers raise ValueError for the same calls, before a device is asked for
    for args in [(-1, 1.0, 1.0), (9, 1.0, 1.0), (1.5, 1.0, 1.0), (True, 1.0, 1.0), ("1", 1.0, 1.0), (1, 0.0, 1.0), (1, nan, 1.0), (1, 1.0, 0.0),
                 (1, 1.0, inf), (1, 1.0, 1e-40), (1, None, 1.0)]:
        with pytest.raises(ValueError):
            tracking.bilateral_weights(*args)
        with pytest.raises(ValueError):
            tracking.depth_bilateral(np.ones((4, 4), F), *args)
    for depth in (np.ones((4, 4), np.float64), np.ones(4, F), np.ones((0, 4), F), np.ones((2, 2, 2), F)):
        with pytest.raises(ValueError):
            tracking.depth_bilateral(depth, 1, 1.0, 1.0)


def dirty(h, w, seed):
    rng = np.random.default_rng([seed, h, w])
    d = rng.uniform(0.5, 4.0, size=(h, w)).astype(F)
    kind = rng.random((h, w))
    for k, bad in enumerate([0.0, -1.5, np.nan, np.inf, -np.inf]):
        d[(kind >= 0.02 * k) & (kind < 0.02 * (k + 1))] = bad
    return d


def test_reference_properties():
    d = dirty(13, 21, 1)
    ok = BR.valid(d)
    assert 0 < (~ok).sum() < ok.sum()
    # radius 0 is the identity on valid pixels; invalid centres give 0 at every radius
    out0 = BR.depth_bilateral(d, 0, *BR.weights(0, 1.0, 1.0))
    assert np.array_equal(bits(out0[ok]), bits(d[ok])) and np.all(bits(out0[~ok]) == 0)
    for r in (1, 3, 8):
        out = BR.depth_bilateral(d, r, *BR.weights(r, 2.0, 0.5))
        assert np.all(bits(out[~ok]) == 0) and np.isfinite(out).all() and np.all(out[ok] > 0)
        assert (out[ok] != d[ok]).any()
    # a step of 1.0 | 2.0 comes back bit for bit with sigma_r = 0.1: cut = 0.3 m is below the 1 m step, and with every
    # contributing depth the same power of two each product w d and the quotient are exact
    step = np.where(np.arange(40)[None, :] < 17, F(1.0), F(2.0)) * np.ones((9, 1), F)
    for r in (0, 1, 2, 5, 8):
        assert np.array_equal(bits(BR.depth_bilateral(step, r, *BR.weights(r, 1.7, 0.1))), bits(step)), r
    # ... and with a cut above the step the two sides do mix
    assert (BR.depth_bilateral(step, 2, *BR.weights(2, 1.7, 0.5)) != step).any()
    # invalid neighbours are skipped: a valid pixel surrounded by invalid ones keeps its depth, and a hole changes the mean of
    # its neighbours only through the taps it removes
    lone = np.full((5, 5), np.nan, dtype=F)
    lone[2, 2] = F(1.25)
    lone[0, 0], lone[4, 4], lone[0, 4] = F(0.0), F(-3.0), F(np.inf)
    out = BR.depth_bilateral(lone, 2, *BR.weights(2, 1.0, 1.0))
    assert out[2, 2] == F(1.25) and np.count_nonzero(out) == 1
    flat = np.full((5, 5), F(2.0))                                      # a power of two: every weighted mean is exact
    flat[2, 3] = np.nan
    out = BR.depth_bilateral(flat, 1, *BR.weights(1, 1.0, 1.0))
    assert out[2, 3] == 0 and np.all(out[np.isfinite(flat)] == F(2.0))
    # the tap order is part of the restatement: a by-hand 1 x 3 case, dx = -1, 0, 1
    sp, rg, cut, inv = BR.weights(1, 1.0, 1.0)
    row = np.array([[1.0, 1.5, 2.25]], dtype=F)
    num, den = F(0.0), F(0.0)
    for dx in (-1, 0, 1):
        a = np.abs(row[0, 1 + dx] - row[0, 1])
        w = sp[1, 1 + dx] * rg[min(255, int(a * inv))]
        num, den = num + w * row[0, 1 + dx], den + w
    assert bits(BR.depth_bilateral(row, 1, sp, rg, cut, inv))[0, 1] == bits(num / den)


def test_filter_brings_the_normals_of_a_noisy_frame_closer_to_the_clean_ones():
    """The room frame of bilateral_ref.room_frame with 0.5 % z noise (seed 7), filter (3, 2.0, 0.05).  Measured: the mean angle
    between the organised normals (max_jump 0.05) of the noisy frame and of the clean frame is 20.29 degrees without the filter
    and 12.14 degrees with it, over the 11844 / 11843 pixels where both have a normal.  The condition is `smaller`; the figures are
    printed."""
    s = BR.room_frame()
    K = s["K"]
    clean = BR.normals_organized(PR.unproject(s["clean"], K), BR.MAX_JUMP)
    raw = BR.normals_organized(PR.unproject(s["noisy"], K), BR.MAX_JUMP)
    filtered_depth = BR.depth_bilateral(s["noisy"], BR.FILTER[0], *BR.weights(*BR.FILTER))
    filtered = BR.normals_organized(PR.unproject(filtered_depth, K), BR.MAX_JUMP)
    angle_raw, n_raw = BR.mean_normal_angle_deg(raw, clean)
    angle_filtered, n_filtered = BR.mean_normal_angle_deg(filtered, clean)
    print("mean normal angle to the clean frame: %.3f degrees raw (%d px), %.3f degrees filtered (%d px)"
          % (angle_raw, n_raw, angle_filtered, n_filtered))
    assert n_raw > 0.9 * s["H"] * s["W"] and n_filtered > 0.9 * s["H"] * s["W"]
    assert angle_filtered < angle_raw
    # the filter moved depths by the noise's size, not more: it smooths, it does not reshape
    assert np.abs(filtered_depth - s["clean"]).mean() < np.abs(s["noisy"] - s["clean"]).mean()
