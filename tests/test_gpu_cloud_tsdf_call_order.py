"""GPU: r3d_tsdf_integrate_cloud among the other entry points on one context, in the manner of tests/test_gpu_call_order.py.  It
claims shared workspaces of the context (kWsSpare for the block bitmap, kWsCounts for the compaction's counters) and calls
r3d_nn_index_create and r3d_nn_index_query, which take kWsIn, kWsOut, kWsSpare, kWsCounts, kWsPartials and kWsMisc -- where every other
entry point leaves foreign data and expects none of its own to survive.  The case below is checked against the restatement and
returns its outputs as bytes; it must give the bytes a fresh context gives behind every case of the catalogue
(tests/call_order_cases.py, read here, not extended), and every case of the catalogue must give its own fresh-context bytes behind
it."""
import numpy as np
import pytest

import call_order_cases as CAT
import cloud_tsdf_ref as CT
from helpers import r3d as _r3d
from test_gpu_call_order import base as catalogue_base, fresh
from test_gpu_cloud_tsdf import GEO, planes, random_cloud

pytestmark = pytest.mark.gpu

NAMES = list(CAT.CASES)
# the cases whose entry points take the workspaces this one and its NN query take: their large instances grow them and fill them
SHARERS = [n for n in ("nn_build_query", "knn_sor_ror_select", "normals_knn", "tsdf", "select", "voxelgrid", "fuse_host") if n in CAT.CASES]
_WANT = {}


def cloud_tsdf(ctx, scale=1):
    """two clouds with colour through the host call (its own index) into one volume, in chunks of 9 blocks; planes and counts
    against the restatement"""
    R = _r3d()
    n = 1500 * scale
    origin, vs, dims, tr = GEO
    if n not in _WANT:
        rng = np.random.default_rng(91)
        clouds = [random_cloud(n, (-1.0, -0.85, -0.65), (1.0, 0.85, 0.65), 91) + (rng.integers(0, 256, (n, 3), dtype=np.uint8),),
                  random_cloud(n // 3, (-0.5, -0.85, -0.65), (1.0, 0.85, 0.65), 92) + (rng.integers(0, 256, (n // 3, 3), dtype=np.uint8),)]
        nv = dims[0] * dims[1] * dims[2]
        vol, col, counts = np.zeros((nv, 2), np.float32), np.zeros((nv, 4), np.uint32), []
        for xyz, nrm, rgb in clouds:
            c = rgb.astype(np.uint32)
            vol, col, touched = CT.integrate_cloud(vol, origin, vs, dims, tr, xyz, nrm, col, c[:, 0] | c[:, 1] << 8 | c[:, 2] << 16)
            counts.append(touched)
        _WANT[n] = (clouds, vol, col, counts)
    clouds, want, want_col, counts = _WANT[n]
    V = R.TSDFVolume(origin, vs, dims, tr, ctx=ctx, color=True)
    ctx.set_tuning("tsdf_cloud_chunk", 9)
    try:
        got = [V.integrate_cloud(*cloud) for cloud in clouds]
        vol, col = planes(V)
    finally:
        ctx.set_tuning("tsdf_cloud_chunk", 0)
        V.close()
    assert got == counts and np.array_equal(vol.view(np.uint32), want.view(np.uint32)) and np.array_equal(col, want_col)
    return vol.tobytes() + col.tobytes()


@pytest.fixture(scope="module")
def alone():
    c = fresh()
    try:
        return cloud_tsdf(c)
    finally:
        c.close()


@pytest.mark.parametrize("other", NAMES)
def test_behind_and_in_front_of_every_case(alone, other):
    c = fresh()
    try:
        CAT.CASES[other](c)
        assert cloud_tsdf(c) == alone, "cloud_tsdf differs behind %s" % other
        assert CAT.CASES[other](c) == catalogue_base(other), "%s differs behind cloud_tsdf" % other
    finally:
        c.close()


def test_small_behind_large(alone):
    c = fresh()
    try:
        for other in SHARERS:
            CAT.CASES[other](c, 4)
        cloud_tsdf(c, 4)
        assert cloud_tsdf(c) == alone, "behind the large instances"
        assert cloud_tsdf(c) == alone, "on its second run behind the large instances"
    finally:
        c.close()
