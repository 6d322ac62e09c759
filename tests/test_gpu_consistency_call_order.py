"""GPU: the depth consistency entry points among the others on one context, in the manner of tests/test_gpu_call_order.py.  They
claim shared workspaces of the context (kWsSpare for the relative pose rows, kWsIn / kWsOut for the host call's staging, kWsCounts
for the compaction's counters), where every other entry point leaves foreign data and expects none of its own to survive.  The
case below is checked against the restatement and returns its outputs as bytes; it must give the bytes a fresh context gives
behind every case of the catalogue (tests/call_order_cases.py, read here, not extended), and every case of the catalogue must give
its own fresh-context bytes behind it."""
import numpy as np
import pytest

import call_order_cases as CAT
import consistency_ref as CR
from helpers import r3d as _r3d
from test_gpu_call_order import base as catalogue_base, fresh
from test_gpu_consistency import scene

pytestmark = pytest.mark.gpu

NAMES = list(CAT.CASES)
# the cases whose entry points stage through the workspaces this one takes: their large instances grow them and fill them
SHARERS = [n for n in ("fuse_host", "fuse_rgb_host", "apply_host", "tsdf", "select", "knn_sor_ror_select", "voxelgrid") if n in CAT.CASES]
_WANT = {}


def consistency(ctx, scale=1):
    """the host call with a wide and a narrow source table, then the filtered cloud; every output against the restatement"""
    R = _r3d()
    h, w = (48, 64) if scale > 1 else (24, 32)
    if (h, w) not in _WANT:
        d, q, t, K = scene(R, 4, h, w, seed=7)
        poses = R.poses_w2c(q, t)
        tables = (np.array([[(r + 1 + k % 3) % 4 for k in range(16)] for r in range(4)], np.int32), R.window_sources(4, 1))
        _WANT[(h, w)] = (d, q, t, K, tables, [CR.depth_consistency(d, poses, src, K, 0.03, 1, 0) for src in tables])
    d, q, t, K, tables, wants = _WANT[(h, w)]
    out = []
    for src, (votes, keep, filtered) in zip(tables, wants):
        cons, viol, kept, got = R.depth_consistency(d, q, t, K, sources=src, rel_tol=0.03, min_consistent=1, ctx=ctx)
        assert np.array_equal(cons, votes[..., 0]) and np.array_equal(viol, votes[..., 1]) and np.array_equal(kept, keep.astype(bool))
        assert np.array_equal(got.view(np.uint32), filtered.view(np.uint32))
        out += [cons, viol, kept, got]
    xyz, kept2 = R.fuse_frames_consistent(d, q, t, K, radius=1, rel_tol=0.03, min_consistent=1, ctx=ctx)
    assert np.array_equal(kept2, out[-2]) and 0 < len(xyz) < d.size
    assert np.array_equal(xyz.view(np.uint32), R.fuse_frames(d, q, t, K, ctx=ctx)[kept2.ravel()].view(np.uint32))
    return b"".join(np.ascontiguousarray(a).tobytes() for a in out + [xyz])


@pytest.fixture(scope="module")
def alone():
    c = fresh()
    try:
        return consistency(c)
    finally:
        c.close()


@pytest.mark.parametrize("other", NAMES)
def test_behind_and_in_front_of_every_case(alone, other):
    c = fresh()
    try:
        CAT.CASES[other](c)
        assert consistency(c) == alone, "consistency differs behind %s" % other
        assert CAT.CASES[other](c) == catalogue_base(other), "%s differs behind consistency" % other
    finally:
        c.close()


def test_small_behind_large(alone):
    c = fresh()
    try:
        for other in SHARERS:
            CAT.CASES[other](c, 4)
        consistency(c, 4)
        assert consistency(c) == alone, "behind the large instances"
        assert consistency(c) == alone, "on its second run behind the large instances"
    finally:
        c.close()
