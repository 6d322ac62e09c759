"""The cases whose fp64 sums and ICP states are pinned bit for bit (tests/golden/sums_bits.json): one function per family of
sums, used unchanged by the recorder (tests/golden/make_sums_bits.py) and by the test (tests/test_gpu_sums_bits.py).  Every
input comes from the repository's own seeded generators.  A function returns (bits, facts): `bits` maps a name to a hex string
of raw words, `facts` holds what the recorder checks before it writes (pair counts, statuses) so that no degenerate case is
ever pinned."""
import importlib

import numpy as np

from helpers import PKG
from oracle import icp_ref as OI

STATE_DOUBLES = 512


def words(a):
    """hex of the raw uint64 words of a float64 array, 16 digits per word"""
    return "".join("%016x" % int(w) for w in np.ascontiguousarray(a, dtype=np.float64).reshape(-1).view(np.uint64))


def state_words(st):
    """All STATE_DOUBLES words of an ICP state; the all-zero tail (unused history) is cut off the string, which loses nothing
    because the length is fixed."""
    assert st.shape == (STATE_DOUBLES,)
    s = words(st)
    while s.endswith("0" * 16):
        s = s[:-16]
    return s


def f32_word(v):
    return "%08x" % int(np.float32(v).view(np.uint32))


def state_facts(st):
    return {"status": float(st[33]), "iterations": float(st[32]), "pairs": float(st[35])}


def compute_units():
    import torch
    return int(torch.cuda.get_device_properties(0).multi_processor_count)


def _median_gate(d2):
    """the upper median of the squared match distances, as the f32 the kernel compares with"""
    return np.float32(np.sort(d2)[len(d2) // 2])


def icp_separate(ctx, n_tgt, n_src):
    """18 sums, brute-force NN then the separate gather pass (accumulate_kernel + finish): ungated and gated at the median d2.
    ceil(n_src / 256) partial rows, capped at 4 x compute units."""
    icp = importlib.import_module(PKG + ".icp")
    src, tgt, _, _ = OI.synthetic_pair(n_tgt=n_tgt, n_src=n_src, noise=0.01)
    assert src.shape[0] == n_src
    dev = icp.IcpDevice(src, tgt, ctx=ctx, culled=False)
    try:
        dev.nn()
        gate = _median_gate(dev.d_d2.download(np.float32, dev.n))
        ungated, gated = dev.sums(), dev.sums(max_d2=float(gate))
    finally:
        dev.free()
    bits = {"gate_f32": f32_word(gate), "sums_ungated": words(ungated), "sums_gated": words(gated)}
    return bits, {"n": n_src, "pairs": [float(ungated[0]), float(gated[0])], "rows": -(-n_src // 256)}


def icp_fused(ctx):
    """18 sums taken in the NN index's query kernels: the cold LDS-tile kernel and (nn_warm = 3: whenever the previous matches
    bound the search, as in a loop's later iterations) the wave-local warm kernel; then 3 device-resident iterations, whose first
    query runs the tile kernel and whose second and third run the warm kernel.  Ungated and gated at the median d2."""
    icp = importlib.import_module(PKG + ".icp")
    src, tgt, _, _ = OI.synthetic_pair(n_tgt=20000, n_src=15000, noise=0.01)
    bits, pairs, states = {}, [], []
    dev = icp.IcpDevice(src, tgt, ctx=ctx)
    try:
        dev.nn()
        gate = _median_gate(dev.d_d2.download(np.float32, dev.n))
        bits["gate_f32"] = f32_word(gate)
    finally:
        dev.free()
    for name, max_d2 in (("ungated", -1.0), ("gated", float(gate))):
        dev = icp.IcpDevice(src, tgt, ctx=ctx)
        try:
            ctx.set_tuning("nn_warm", 1)
            cold = dev.nn_sums(max_d2=max_d2)
            ctx.set_tuning("nn_warm", 3)
            warm = dev.nn_sums(max_d2=max_d2)
            ctx.set_tuning("nn_warm", 0)
            dev.state_reset()
            dev.iterate(3, max_d2=max_d2)
            st = dev.d_state.download(np.float64, STATE_DOUBLES)
        finally:
            ctx.set_tuning("nn_warm", 0)
            dev.free()
        bits["sums_cold_" + name], bits["sums_warm_" + name], bits["state_" + name] = words(cold), words(warm), state_words(st)
        pairs += [float(cold[0]), float(warm[0])]
        states.append(state_facts(st))
    return bits, {"n": src.shape[0], "pairs": pairs, "states": states}


PLANE_PARAMS = [(0.0, 1.0, -1.0), (0.5, 1.0, -1.0), (0.5, 20.0, -1.0), (0.8, 4.0, 0.09)]     # test_gpu_plane_icp.py's four


def plane(ctx, trim_q, gate_scale, max_d2):
    """29 sums of the point-to-plane loop over test_gpu_plane_icp.py's matched_state (96 x 128 source: 48 partial rows), and the
    state after 3 iterations with the same parameters."""
    from test_gpu_plane_icp import matched_state
    icp = importlib.import_module(PKG + ".icp")
    S = importlib.import_module(PKG + ".synthetic")
    _, _, dev, _, _, _ = matched_state(icp, S, ctx)
    try:
        sums = dev.sums(trim_q, gate_scale, max_d2)
        dev.iterate(3, trim_q, gate_scale, max_d2)
        st = dev.d_state.download(np.float64, STATE_DOUBLES)
        n = dev.n
    finally:
        dev.free()
    return {"sums": words(sums), "state": state_words(st)}, {"n": n, "pairs": [float(sums[0])], "states": [state_facts(st)]}


def track(ctx, h, w):
    """29 sums of frame-to-model tracking over tests/track_ref.py's analytic case (one partial row per 1024 pixels), and the
    state after 3 iterations."""
    import track_ref as TR
    tracking = importlib.import_module(PKG + ".tracking")
    case = TR.analytic_case(h, w, 2.0, 1.0, (0.03, 0.02, -0.04))
    dev = tracking.TrackDevice(case["src_vertex"], case["model_vertex"], case["model_normal"], case["model_row"],
                               TR.inverse_pose(case["model_row"]), case["K"], ctx=ctx)
    try:
        sums, _, _ = dev.sums(0.5)
        dev.iterate(3, 0.5)
        st = dev.d_state.download(np.float64, STATE_DOUBLES)
    finally:
        dev.free()
    return {"sums": words(sums), "state": state_words(st)}, {"n": h * w, "pairs": [float(sums[0])], "states": [state_facts(st)],
                                                              "rows": -(-h * w // 1024)}


def ransac(ctx):
    """10 sums of the RANSAC refit: one plane of segment_ref.noisy_plane (20 000 points, 30 % outliers); every float the wrapper
    returns for the refined plane, and the inlier mask."""
    import segment_ref as SR
    seg = importlib.import_module(PKG + ".segmentation")
    xyz, _ = SR.noisy_plane(n=20_000, seed=3)
    p = seg.segment_plane(xyz, distance_threshold=0.01, num_hypotheses=1024, seed=5, ctx=ctx)
    mask = np.zeros(xyz.shape[0], dtype=np.uint8)
    mask[p.rows] = 1
    bits = {"plane": words(p.plane), "centroid": words(p.centroid), "eigenvalues": words(p.eigenvalues),
            "counts": "%x.%x.%x" % (int(p.best_hypothesis), int(p.best_count), int(p.n_valid)), "inlier_mask": np.packbits(mask).tobytes().hex()}
    return bits, {"n": xyz.shape[0], "pairs": [float(len(p.rows))], "finite": bool(np.isfinite(p.plane).all())}


# name -> (function, arguments).  The separate path's second case strides the finish: 274 rows, so finish threads 0..17 fold two
# rows each.  (oracle.icp_ref.synthetic_pair draws the source from the target's rows, so 70 000 sources need 70 000 targets.)
CASES = {"icp_separate_59_rows": (icp_separate, (20000, 15000)),
         "icp_separate_274_rows": (icp_separate, (70000, 70000)),
         "icp_fused": (icp_fused, ()),
         "track_3_rows": (track, (48, 64)),
         "track_300_rows": (track, (480, 640)),
         "ransac_refit": (ransac, ())}
CASES.update({"plane_%g_%g_%g" % p: (plane, p) for p in PLANE_PARAMS})


def run(name, ctx):
    fn, args = CASES[name]
    return fn(ctx, *args)
