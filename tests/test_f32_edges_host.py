"""CPU: the cases of tests/f32_edge_cases.py bite.  Before tests/test_gpu_f32_edges.py compares anything with the device, this file
asserts of the restatements alone, case by case, that (a) the expected bits differ from what flush-to-zero arithmetic gives --
subnormal inputs flushed to signed zero and the restatement run again, and where the case rests on subnormal intermediates (d2 of
the searches, the normal's squared length, the filter's weight products) those flushed too; (b) at least a quarter of the compared
elements are subnormal or computed from a subnormal operand; (c) no case is degenerate: voxels pass, points and triangles are
found, rays hit, the lists are full.  The counts each case records are in DESIGN.md ("f32 edges").  Also here: the bilateral
filter's host table against np.exp where its entries are subnormal, and the committed build recipe's floating-point options."""
import importlib
import os
import re

import numpy as np
import pytest

import f32_edge_cases as E
import outliers_ref as OREF
from helpers import PKG, ROOT
from oracle import icp_ref as OI

F = np.float32


def quarter(part, whole):
    return 4 * part >= whole


# ---- case 1 ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(E.NN_SCALES))
def test_nn_cases(name):
    c = E.nn_case(name)
    f = c["facts"]
    # the integer answer is the restatement's (oracle/icp_ref.py evaluates the header's expression; its argmin takes the lowest row)
    with np.errstate(over="ignore", invalid="ignore"):
        d = OI.pair_d2(c["src"], c["tgt"])
    d[~np.isfinite(d)] = np.inf
    oi = np.argmin(d, axis=1)
    od = d[np.arange(len(oi)), oi]
    oi = np.where(np.isfinite(od), oi, 0)
    assert np.array_equal(oi, c["idx"]) and np.array_equal(E.bits(od), E.bits(c["d2"]))
    assert f["ties"] > 0 and f["zero"] > 0
    if name == "tiny":
        assert f["pairs_subnormal"] + (d == 0).sum() == f["pairs"]            # EVERY non-zero d2 is subnormal
        assert f["subnormal"] == f["n"] - f["zero"] and quarter(f["subnormal"], f["n"])
        assert f["ftz_differs"] == f["n"]           # flushed, every pair ties at 0: row 0 wins everywhere, and no source has row 0
        assert (c["idx"] != 0).all()
    elif name == "huge":
        assert f["inf"] == f["n"] - f["zero"] and quarter(f["inf"], f["n"])   # every non-zero d2 overflows
        assert np.isinf(d[d != 0]).all()
        assert (c["idx"][np.isinf(c["d2"])] == 0).all()
    else:
        assert f["inf"] == 0 and f["subnormal"] == 0 and np.isinf(d).any()    # the winners are finite, far pairs overflow
        assert c["d2"].max() >= 2.0 ** 122


@pytest.mark.parametrize("k", E.KNN_KS)
@pytest.mark.parametrize("name", list(E.NN_SCALES))
def test_knn_cases(name, k):
    c = E.knn_case(name, k)
    f = c["facts"]
    ri, rd = OREF.knn_brute(c["xyz"], k)
    assert np.array_equal(ri, c["idx"]) and np.array_equal(E.bits(rd), E.bits(c["d2"]))
    if name == "tiny":
        assert f["full_rows"] == len(c["idx"]) and quarter(f["subnormal"], f["n"]) and f["subnormal"] + f["zero"] == f["n"]
        assert f["ftz_differs"] >= f["n"] - 1
    elif name == "huge":
        assert f["inf"] + f["zero"] == f["n"] and f["zero"] > 0 and quarter(f["inf"], f["n"])
    else:
        assert f["full_rows"] == len(c["idx"]) or k == 32                      # the 32nd neighbour of some rows is past 2^128
        assert f["full_rows"] > 0 and f["subnormal"] == 0


# ---- case 2 ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dims,dtype", E.TSDF_CASES, ids=lambda v: "x".join(map(str, v)) if isinstance(v, tuple) else v.__name__)
def test_tsdf_cases(dims, dtype):
    f = E.tsdf_case(dims, dtype)["facts"]
    assert f["passed"] > 0 and f["points"] > 0 and 0 < f["seen"] < f["voxels"]
    assert f["vs_subnormal"] and f["tr_subnormal"] and f["scale_subnormal"]
    assert f["pcz_subnormal"] > 0 and f["pcz_normal"] > 0                      # pc.z straddles 2^-126
    assert quarter(f["pcz_subnormal"], f["pcz_subnormal"] + f["pcz_normal"]) and quarter(f["xyz_subnormal"], f["xyz_n"])
    assert f["ftz_passed"] == 0 and f["ftz_volume_differs"] and f["ftz_points_differ"]    # flushed, the volume has no extent


# ---- case 3 ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dims", E.VOLUME_DIMS, ids=lambda d: "x".join(map(str, d)))
def test_volume_cases(dims):
    c = E.volume_case(dims)
    f = c["facts"]
    t = c["vol"].tsdf
    for v in (E.DENORM_MIN, E.TINY - E.DENORM_MIN, E.TINY, E.FLT_MAX / 2, F(0.75) * E.FLT_MAX):
        assert (t == v).any() and (t == -v).any(), v
    assert ((t == 0) & np.signbit(t)).any() and ((t == 0) & ~np.signbit(t)).any()
    assert f["points"] > 0 and f["triangles"] > 0
    assert f["crossings_both_subnormal"] > 0 and f["crossings_negative_zero"] > 0
    assert f["difference_overflows"] > 0 and f["difference_is_flt_max"] > 0
    assert f["sq_length_subnormal"] > 0 and f["sq_length_zero"] > 0
    assert f["unit_normals_from_subnormal_length"] == f["sq_length_subnormal"] and f["zero_normals"] > 0
    assert quarter(f["crossings_with_subnormal"], f["points"]) and quarter(f["sq_length_subnormal"], f["points"])
    assert f["ftz_count_differs"] and f["ftz_normals_differ_by_squares_alone"] >= f["sq_length_subnormal"]


@pytest.mark.parametrize("dims", E.VOLUME_DIMS, ids=lambda d: "x".join(map(str, d)))
def test_raycast_cases(dims):
    f = E.raycast_case(dims)["facts"]
    assert f["hits"] > 0 and f["misses"] > 0
    assert quarter(f["hits_in_cells_with_subnormal"], f["hits"])
    assert f["ftz_depth_differs"] + f["ftz_hit_mask_differs"] > 0 and f["ftz_normal_differs"] > 0


# ---- case 4 ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("h,w", E.RASTERS)
def test_depth_half_cases(h, w):
    f = E.half_case(h, w)["facts"]
    assert f["subnormal"] > 0 and f["inf"] > 0 and quarter(f["from_subnormal"], f["outputs"]) and quarter(f["ftz_differs"], f["outputs"])


def test_bilateral_table_where_it_is_subnormal():
    """r3d_bilateral_weights (host only) against np.exp: the same entries subnormal, the same entries zero, one f32 step at the most
    between two libms (as tests/test_bilateral_host.py allows of the normal entries)"""
    tracking = importlib.import_module(PKG + ".tracking")
    radius, ss, sr = E.BILATERAL
    spatial, rng, cut, inv_step = tracking.bilateral_weights(radius, ss, sr)
    want_s, want_r, want_cut, want_inv = E.bilateral_tables()
    d2 = np.add.outer(np.arange(-radius, radius + 1) ** 2, np.arange(-radius, radius + 1) ** 2)
    assert np.array_equal(E.is_sub(want_s), (d2 >= 88) & (d2 <= 103)) and np.array_equal(want_s == 0, d2 >= 104)
    assert np.array_equal(E.is_sub(spatial), E.is_sub(want_s)) and np.array_equal(spatial == 0, want_s == 0)
    assert np.abs(E.bits(spatial).astype(np.int64) - E.bits(want_s).astype(np.int64)).max() <= 1
    assert np.abs(E.bits(rng).astype(np.int64) - E.bits(want_r).astype(np.int64)).max() <= 1 and not E.is_sub(rng).any()
    assert F(cut) == want_cut and F(inv_step) == want_inv and np.isfinite(want_inv) and want_inv > 0


@pytest.mark.parametrize("h,w", E.RASTERS)
def test_bilateral_cases(h, w):
    f = E.bilateral_facts(E.edge_depth(h, w), E.bilateral_tables())
    assert f["table_subnormal"] > 0 and f["table_zero"] > 0 and f["inf"] > 0
    assert quarter(f["centre_subnormal"], f["outputs"])
    assert quarter(f["ftz_differs"], f["outputs"]) and f["ftz_differs_by_table_alone"] > 0


# ---- case 5 ---------------------------------------------------------------------------------------------------------------------
def test_project_case():
    f = E.project_case()["facts"]
    assert all(f["inputs_subnormal"][k] > 0 for k in ("depth", "gcam", "points", "gpix"))
    assert f["den_subnormal"] > 0 and f["d_subnormal"] > 0
    assert f["from_subnormal_fraction"] >= 0.25
    for name in ("cam", "gdep", "pix", "gpts"):
        assert quarter(f[name]["ftz_differs"], f[name]["n"]), (name, f[name])
    assert f["cam"]["subnormal"] > 0 and f["gdep"]["subnormal"] > 0 and f["gpts"]["subnormal"] > 0


# ---- case 6 ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", E.APPLY_KS)
def test_apply_cases(k):
    x = E.apply_points()
    f = E.apply_facts(x, k)
    assert (x != 0).all() and quarter(f["in_subnormal"], f["n"]) and quarter(f["ftz_differs"], f["n"])
    assert f["out_subnormal"] > 0
    if k == 0:
        assert f["inexact"] == 0 and np.array_equal(E.bits(E.apply_expect(x, 0)), E.bits(x[:, list(E.PERM)]))
    if k == 1:
        assert f["ties"] > 0 and f["rounds_up_to_tiny"] > 0
    if k == 30:
        assert f["inexact"] > 0 and f["ties"] > 0
    if k == -1:
        assert f["inf"] > 0


def test_halving_ties_go_to_even():
    """the expectation itself: 1.5, 2.5 and 3.5 units of 2^-149 become 2, 2 and 4; (2^-125 - 2^-149) / 2 becomes 2^-126"""
    x = (np.array([[3, 5, 7]], dtype=np.float64) * 2.0 ** -149).astype(F)
    want = E.apply_expect(x, 1)
    assert np.array_equal(want[0].astype(np.float64) / 2.0 ** -149, np.array([2.0, 2.0, 4.0])[list(E.PERM)])
    up = E.apply_expect(np.full((1, 3), 2.0 ** -125 - 2.0 ** -149, F), 1)
    assert (up == E.TINY).all()


@pytest.mark.parametrize("k", E.APPLY_KS)
def test_unproject_cases(k):
    d = E.unproject_depth()
    f = E.unproject_facts(d, k)
    assert quarter(f["from_subnormal"], f["n"]) and quarter(f["ftz_differs"], f["n"]) and f["out_subnormal"] > 0
    if k == -1:
        assert f["inf"] > 0


# ---- the build recipe ---------------------------------------------------------------------------------------------------------
FORBIDDEN = re.compile(r"fast-math|ffast|unsafe-fp|unsafe-math|finite-math|denormal|flush|ftz|daz|reciprocal-math|associative-math|"
                       r"fp-model|approx-func|no-signed-zeros|-Ofast|correctly-rounded|fp32-denorm|contract=(?!off)", re.I)


def test_build_recipe_keeps_ieee_f32():
    """csrc/Makefile: one set of flags for every object, -ffp-contract=off among them, and nothing that licenses fast or unsafe
    arithmetic, flushes denormals or unrounds division and square root -- in any variable or rule"""
    path = os.path.join(ROOT, PKG, "csrc", "Makefile")
    text = open(path).read()
    code = "\n".join(line.split("#", 1)[0] for line in text.splitlines())
    flags = [m.group(1) for m in re.finditer(r"^CXXFLAGS\s*[:+?]?=\s*(.*)$", code, re.M)]
    assert len(flags) == 1 and "-ffp-contract=off" in flags[0].split()
    assert not FORBIDDEN.search(code), FORBIDDEN.search(code).group(0)
    rules = re.findall(r"^\t\$\(HIPCC\) (.*-c .*)$", code, re.M)
    assert len(rules) == 2 and all(r.startswith("$(CXXFLAGS) ") for r in rules)       # every object: exactly the common flags
    assert not re.search(r"^\s*(override\s+)?\S*FLAGS\S*\s*\+=", code, re.M)             # no per-object additions
    assert not re.search(r"^build/\S+\s*:\s*\S*FLAGS", code, re.M)                       # no target-specific variables
    # build() runs this Makefile and passes no flags of its own
    entry = open(os.path.join(ROOT, "__graft_entry__.py")).read()
    assert "CXXFLAGS" not in entry and "HIPCC_COMPILE_FLAGS_APPEND" not in entry
