"""GPU: the mesh smoothing entry points among the others on one context, in the manner of tests/test_gpu_consistency_call_order.py.
They keep their keys and ping-pong arrays in a workspace of their own, but their three sorts take the shared kWsCounts of the
context, where every other entry point leaves foreign data and expects none of its own to survive.  The case below is checked
against the restatement and returns its outputs as bytes; it must give the bytes a fresh context gives behind every case of the
catalogue (tests/call_order_cases.py, read here, not extended) that sorts, compacts or handles meshes, and those cases must give
their own fresh-context bytes behind it."""
import numpy as np
import pytest

import call_order_cases as CAT
import mesh_smooth_ref as MS
from helpers import r3d as _r3d
from test_gpu_call_order import base as catalogue_base, fresh
from test_mesh_cc_host import volume_mesh
from test_mesh_smooth_host import bits

pytestmark = pytest.mark.gpu

# the catalogue's cases that use kWsSpare / kWsCounts (sorts, compactions, pose tables) and the mesh cases
OTHERS = [n for n in ("sort", "nn_build_query", "knn_sor_ror_select", "voxelset", "voxelgrid", "fuse_host", "tsdf", "select",
                      "feature_match", "mesh_components", "mesh_distance") if n in CAT.CASES]
SHARERS = [n for n in ("sort", "tsdf", "select", "knn_sor_ror_select", "voxelgrid", "mesh_distance") if n in CAT.CASES]
_WANT = {}


def smoothing(ctx, scale=1):
    """adjacency, Taubin steps and normals of a reference mesh through the host-array layer; every output against the restatement"""
    R = _r3d()
    key = ((16, 16, 17), 86, 0.0) if scale > 1 else ((9, 8, 7), 5, 0.0)
    xyz, nrm, tri = volume_mesh(key)
    if key not in _WANT:
        _WANT[key] = MS.adjacency(tri, len(xyz)) + MS.smooth_mesh(xyz, tri, "taubin", 3, normals=nrm)
    rs, nb, bd, moved, normals = _WANT[key]
    got = R.mesh_adjacency(tri, len(xyz), ctx=ctx)
    assert np.array_equal(got[0], rs) and np.array_equal(got[1], nb) and np.array_equal(got[2], bd.astype(bool))
    out = R.smooth_mesh(xyz, tri, iterations=3, normals=nrm, ctx=ctx)
    assert np.array_equal(bits(out[0]), bits(moved)) and np.array_equal(bits(out[1]), bits(normals))
    return b"".join(np.ascontiguousarray(a).tobytes() for a in got + out)


@pytest.fixture(scope="module")
def alone():
    c = fresh()
    try:
        return smoothing(c)
    finally:
        c.close()


@pytest.mark.parametrize("other", OTHERS)
def test_behind_and_in_front_of_the_sharing_cases(alone, other):
    c = fresh()
    try:
        CAT.CASES[other](c)
        assert smoothing(c) == alone, "smoothing differs behind %s" % other
        assert CAT.CASES[other](c) == catalogue_base(other), "%s differs behind smoothing" % other
    finally:
        c.close()


def test_small_behind_large(alone):
    c = fresh()
    try:
        for other in SHARERS:
            CAT.CASES[other](c, 4)
        smoothing(c, 4)
        assert smoothing(c) == alone, "behind the large instances"
        assert smoothing(c) == alone, "on its second run behind the large instances"
    finally:
        c.close()
