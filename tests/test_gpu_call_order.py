"""GPU: results against call order.  One r3d_ctx carries fourteen grow-only workspaces that some twenty-five source files claim by
name (enum r3d_workspace), and facts about what they hold (select_ws, loop_*, the bilateral table key, the per-device record of cached inputs).
Every case of tests/call_order_cases.py is run behind every other case, behind larger instances of all of them, interleaved
on two contexts of one device and on a caller's stream: each result must be the BYTES the case gives on a context of its own
(BASE).  Nothing here has a tolerance; the comparison with each module's restatement is inside the case, to that module's bound.

Per-test times of the first full run on an MI355X (135 tests of this file and test_gpu_feature_match.py in 32 s): the first
test to run a size computes that size's restatements once for the whole session -- test_after_every_other_case[fuse_host]
3.2 s, test_small_behind_large[fuse_host] 14.3 s (7.4 s since the large cloud's k-NN lists come from the tree); every
other test_after_every_other_case 0.18 .. 0.59 s, every other test_small_behind_large 0.11 .. 0.13 s,
test_two_contexts_of_one_device_interleaved 0.16 s, test_caller_stream_context 0.08 s,
test_loops_do_not_continue_across_foreign_calls 0.03 s each.
"""
import importlib

import numpy as np
import pytest

import call_order_cases as CAT
from helpers import PKG, r3d as _r3d

pytestmark = pytest.mark.gpu

NAMES = list(CAT.CASES)
_BASE = {}


def fresh():
    return _r3d().Context(0)


def base(case):
    if case not in _BASE:
        c = fresh()
        try:
            _BASE[case] = CAT.CASES[case](c)
        finally:
            c.close()
    return _BASE[case]


def same(got, case, what):
    want = base(case)
    if got == want:
        return
    a, b = np.frombuffer(got, np.uint8), np.frombuffer(want, np.uint8)
    n = min(a.size, b.size)
    bad = np.flatnonzero(a[:n] != b[:n])
    raise AssertionError("%s differs %s: %d and %d bytes, first differing byte at offset %d"
                         % (case, what, a.size, b.size, int(bad[0]) if bad.size else n))


@pytest.mark.parametrize("case", NAMES)
def test_after_every_other_case(case):
    for order in (NAMES, NAMES[::-1]):
        c = fresh()
        try:
            for other in order:
                if other == case:
                    continue
                CAT.CASES[other](c)
                same(CAT.CASES[case](c), case, "behind %s" % other)
        finally:
            c.close()


@pytest.mark.parametrize("case", NAMES)
def test_small_behind_large(case):
    c = fresh()
    try:
        for other in NAMES:
            if other != case:
                CAT.CASES[other](c, 4)
        same(CAT.CASES[case](c), case, "behind the large instances of every other case")
        same(CAT.CASES[case](c), case, "on its second run behind the large instances")
    finally:
        c.close()


def test_two_contexts_of_one_device_interleaved():
    a, b = fresh(), fresh()
    try:
        for i, name in enumerate(NAMES):
            nxt = NAMES[(i + 1) % len(NAMES)]
            same(CAT.CASES[name](a), name, "on context A, step %d" % i)
            same(CAT.CASES[nxt](b), nxt, "on context B, step %d" % i)
    finally:
        a.close()
        b.close()


def test_caller_stream_context():
    import torch
    s = torch.cuda.Stream(device=torch.device("cuda", 0))
    c = _r3d().Context(0, stream=s.cuda_stream)
    try:
        assert c.stream_handle() == s.cuda_stream != 0
        for name in NAMES:
            same(CAT.CASES[name](c), name, "on a caller's stream")
    finally:
        c.close()
        s.synchronize()


FOREIGN = ["textfmt", "segment_plane", "knn_sor_ror_select", "register_ransac", "track"]


def _loop(kind, c, between=None, rewrite=None, halves=(2, 2)):
    """the catalogue's loop on context c in two calls with `between` (a callable) in the middle; rewrite: new source rows put
    at the same address through r3d_memcpy_h2d between the halves, the state reset with them.  (state bytes, source bytes)"""
    icp, L = importlib.import_module(PKG + ".icp"), importlib.import_module(PKG + "._lib")
    if kind == "icp_loop":
        src, tgt = CAT.icp_pair()
        dev = icp.IcpDevice(src, tgt, c, True)
        dev.sort_source()                                           # before any rewrite: both runs rewrite rows of one order
        step = dev.iterate
    else:
        src, tgt, shape, T0, _ = CAT.plane_scene()
        dev = icp.PlaneIcpDevice(src, tgt, shape, ctx=c, init=T0)
        step = dev.iterate
    try:
        dev.state_reset()
        if halves[0]:
            step(halves[0])
        if between:
            between()
        if rewrite is not None:
            new = np.ascontiguousarray(rewrite(dev), np.float32)
            L.check(c.lib.r3d_memcpy_h2d(c.handle, dev.d_src.ptr, new.ctypes.data, new.nbytes))
            c.sync()
            dev.state_reset()
        step(halves[1])
        return dev.d_state.download(np.float64, 512).tobytes(), dev.d_src.download(np.float32, dev.n * 3).tobytes()
    finally:
        dev.free()


@pytest.mark.parametrize("kind", ["icp_loop", "plane_icp_loop"])
def test_loops_do_not_continue_across_foreign_calls(kind):
    c = fresh()
    try:
        whole = _loop(kind, c, halves=(0, 4))
        assert _loop(kind, c) == whole, "2 + 2 iterations differ from 4"
        for foreign in FOREIGN:
            got = _loop(kind, c, between=lambda: CAT.CASES[foreign](c))
            assert got[0] == whole[0], "%s: the state differs with %s between the halves" % (kind, foreign)
            assert got[1] == whole[1], "%s: the source differs with %s between the halves" % (kind, foreign)

        # the source rewritten at the same address between the halves: a cold loop on the new points
        def other_points(dev):
            rows = dev.d_src.download(np.float32, dev.n * 3).reshape(-1, 3)
            return rows[::-1] * np.float32(1.001) + np.float32(0.01)
        captured = {}

        def rewrite(dev):
            captured["rows"] = other_points(dev)
            return captured["rows"]
        warm = _loop(kind, c, rewrite=rewrite, halves=(2, 2))
        other = fresh()
        try:
            cold = _loop(kind, other, rewrite=lambda dev: captured["rows"], halves=(0, 2))
        finally:
            other.close()
        assert warm == cold, "%s: a rewritten source gives another result than a cold loop on the new points" % kind
    finally:
        c.close()
