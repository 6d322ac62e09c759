"""NumPy restatement of include/r3d.h "Depth consistency", written from the header text: the fp64 relative pose of the host side and
the per-pixel rule with every operation on np.float32 in the written order (NumPy neither fuses a multiply with an add nor
reorders).  Vectorised over the pixels of a frame; frames and slots are loops, in slot order.  Test infrastructure: the product
never imports it.
"""
import numpy as np

F32 = np.float32


def relative_pose64(poses, r, s):
    """(Rsr [3,3], tsr [3]) in fp64 from the [F,12] world -> camera rows: Rsr = R_s R_r^T and tsr = t_s - Rsr t_r, every element a
    left-to-right sum of three products (Python floats: IEEE doubles, no fused multiply-add)."""
    Rr, tr = [float(v) for v in poses[r][:9]], [float(v) for v in poses[r][9:]]
    Rs, ts = [float(v) for v in poses[s][:9]], [float(v) for v in poses[s][9:]]
    R, t = np.zeros((3, 3)), np.zeros(3)
    for i in range(3):
        row = [(Rs[3 * i] * Rr[3 * j] + Rs[3 * i + 1] * Rr[3 * j + 1]) + Rs[3 * i + 2] * Rr[3 * j + 2] for j in range(3)]
        R[i] = row
        t[i] = ts[i] - ((row[0] * tr[0] + row[1] * tr[1]) + row[2] * tr[2])
    return R, t


def relative_row(poses, r, s):
    """the twelve numbers rounded once to f32: (R [9], t [3])"""
    R, t = relative_pose64(poses, r, s)
    return R.reshape(9).astype(F32), t.astype(F32)


def depth_consistency(depths, poses, sources, K, rel_tol, min_consistent=2, max_violations=0, depth_scale=1.0, with_in_view=False):
    """(votes [F,H,W,2] uint8, keep [F,H,W] uint8, filtered [F,H,W] float32) of rasters [F,H,W] (uint8, uint16 or float32), [F,12]
    float64 world -> camera rows, an [F,S] integer table (-1 = empty slot) and K = (fx, fy, cx, cy).  with_in_view: a fourth array,
    [F,H,W] uint8 -- the filled slots in which the pixel's point has p.z > 0 and falls inside the raster (steps 2 and 3 passed),
    whatever the source's depth there; not an output of the library, the semantic test counts with it."""
    depths = np.asarray(depths)
    poses = np.asarray(poses, dtype=np.float64)
    sources = np.asarray(sources)
    f, h, w = depths.shape
    fx, fy, cx, cy = [F32(v) for v in K]
    scale, tol_rel, wf, hf = F32(depth_scale), F32(rel_tol), F32(w), F32(h)
    votes = np.zeros((f, h, w, 2), np.uint8)
    keep = np.zeros((f, h, w), np.uint8)
    filtered = np.zeros((f, h, w), F32)
    in_view = np.zeros((f, h, w), np.uint8)
    u = np.broadcast_to(np.arange(w, dtype=F32)[None, :], (h, w))
    v = np.broadcast_to(np.arange(h, dtype=F32)[:, None], (h, w))
    with np.errstate(all="ignore"):
        for r in range(f):
            Z = depths[r].astype(F32) * scale
            valid = (Z > 0) & (Z < np.inf)
            x = ((u - cx) / fx) * Z
            y = ((v - cy) / fy) * Z
            cons = np.zeros((h, w), np.int32)
            viol = np.zeros((h, w), np.int32)
            seen = np.zeros((h, w), np.int32)
            for s in sources[r]:
                s = int(s)
                if s < 0:
                    continue
                R, t = relative_row(poses, r, s)
                px = ((R[0] * x + R[1] * y) + R[2] * Z) + t[0]
                py = ((R[3] * x + R[4] * y) + R[5] * Z) + t[1]
                pz = ((R[6] * x + R[7] * y) + R[8] * Z) + t[2]
                ok = valid & (pz > 0)
                ui = np.floor((fx * (px / pz) + cx) + F32(0.5))
                vi = np.floor((fy * (py / pz) + cy) + F32(0.5))
                ok &= (ui >= 0) & (ui < wf) & (vi >= 0) & (vi < hf)          # NaN fails every comparison
                seen += ok
                iu = np.where(ok, ui, 0).astype(np.int64)
                iv = np.where(ok, vi, 0).astype(np.int64)
                d = depths[s][iv, iu].astype(F32) * scale
                ok &= (d > 0) & (d < np.inf)
                diff = d - pz
                tol = tol_rel * pz
                agree = np.abs(diff) <= tol
                cons += ok & agree
                viol += ok & ~agree & (diff > 0)
            kept = valid & (cons >= min_consistent) & (viol <= max_violations)
            votes[r, ..., 0], votes[r, ..., 1] = cons, viol
            keep[r] = kept
            filtered[r] = np.where(kept, Z, F32(0))
            in_view[r] = seen
    assert filtered.dtype == F32
    return (votes, keep, filtered, in_view) if with_in_view else (votes, keep, filtered)
