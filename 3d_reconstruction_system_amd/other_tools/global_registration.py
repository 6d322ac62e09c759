#!/usr/bin/env python3
"""Register two clouds on the MI355X without a starting pose: FPFH features, mutual matching, RANSAC, optional ICP.

    python global_registration.py SOURCE TARGET --voxel V [--out-T T_data.txt] [--out-ply MOVED.ply] [--refine]
                                  [--hypotheses H] [--rounds R] [--seed S] [--k K] [--feature-radius F]
                                  [--source-viewpoint X Y Z] [--target-viewpoint X Y Z]

SOURCE / TARGET: PLY clouds (anything cloud_io.read_ply reads) or the reference's camera txt files (X,Y,Z per line).  The 4x4
that moves SOURCE onto TARGET is written to --out-T in the format transfer_T_icp.py reads (get_T), and printed; --out-ply gets
the moved source as a binary PLY.  The viewpoints say where each cloud was seen from in its own frame (a single-view scan in its
camera frame: 0 0 0); clouds turned far against each other need them.
"""
import argparse
import math
import os
import sys

if __package__ in (None, ""):
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "transfer"))
    import _common  # type: ignore
else:
    from ..transfer import _common


def parse_args(argv):
    p = argparse.ArgumentParser(description="Global registration of two point clouds (FPFH + RANSAC).")
    p.add_argument("source", help="cloud to move (.ply or .txt)")
    p.add_argument("target", help="cloud to move it onto (.ply or .txt)")
    p.add_argument("--voxel", required=True, metavar="V", help="voxel size both clouds are downsampled to")
    p.add_argument("--out-T", default="T_data.txt", metavar="PATH", help="where the 4x4 goes (default T_data.txt)")
    p.add_argument("--out-ply", metavar="PATH", help="write the moved source here")
    p.add_argument("--refine", action="store_true", help="finish with point-to-plane ICP")
    p.add_argument("--hypotheses", default="65536", metavar="H")
    p.add_argument("--rounds", default="4", metavar="R")
    p.add_argument("--seed", default="0", metavar="S")
    p.add_argument("--k", default="32", metavar="K")
    p.add_argument("--feature-radius", default="5", metavar="F", help="feature radius in voxels")
    p.add_argument("--source-viewpoint", nargs=3, metavar=("X", "Y", "Z"))
    p.add_argument("--target-viewpoint", nargs=3, metavar=("X", "Y", "Z"))
    args = p.parse_args(argv)

    def number(text, kind, what):
        try:
            return kind(text)
        except ValueError:
            p.error("%s must be %s, got %r" % (what, "an integer" if kind is int else "a number", text))

    args.voxel, args.feature_radius = number(args.voxel, float, "V"), number(args.feature_radius, float, "F")
    for v, what in ((args.voxel, "V"), (args.feature_radius, "F")):
        if not (math.isfinite(v) and v > 0.0):
            p.error("%s must be finite and positive, got %r" % (what, v))
    args.hypotheses, args.rounds = number(args.hypotheses, int, "H"), number(args.rounds, int, "R")
    args.seed, args.k = number(args.seed, int, "S"), number(args.k, int, "K")
    if not 1 <= args.hypotheses <= 65536:
        p.error("H must be in [1, 65536], got %d" % args.hypotheses)
    if args.rounds < 1:
        p.error("R must be at least 1, got %d" % args.rounds)
    if not 0 <= args.seed < 1 << 64:
        p.error("S must be in [0, 2^64), got %d" % args.seed)
    if not 3 <= args.k <= 32:
        p.error("K must be in [3, 32], got %d" % args.k)
    for name in ("source_viewpoint", "target_viewpoint"):
        v = getattr(args, name)
        if v is not None:
            v = tuple(number(c, float, "X Y Z") for c in v)
            if not all(math.isfinite(c) for c in v):
                p.error("X Y Z must be finite, got %r" % (v,))
            setattr(args, name, v)
    for path in (args.source, args.target):
        if not os.path.isfile(path):
            p.error("input file %r does not exist" % path)
    return args


def read_cloud(r3d, path):
    if path.lower().endswith(".ply"):
        return r3d.cloud_io.read_ply(path).astype("float32")
    return r3d.cloud_io.read_xyz_txt(path).astype("float32")


def main(argv=None):
    args = parse_args(sys.argv[1:] if argv is None else argv)
    r3d = _common.package()
    reg = __import__(r3d.__name__ + ".registration", fromlist=["register_global"])
    src, tgt = read_cloud(r3d, args.source), read_cloud(r3d, args.target)
    try:
        T, info = reg.register_global(src, tgt, args.voxel, k=args.k, feature_radius=args.feature_radius, num_hypotheses=args.hypotheses,
                                      rounds=args.rounds, seed=args.seed, refine=args.refine, src_viewpoint=args.source_viewpoint,
                                      tgt_viewpoint=args.target_viewpoint, ctx=_common.context())
    except ValueError as e:
        print("no registration: %s" % e, file=sys.stderr)
        return 1
    r3d.write_T(args.out_T, T)
    if args.out_ply:
        r3d.cloud_io.write_ply_binary(args.out_ply, r3d.apply_T(src, T, ctx=_common.context()))
    ran = info["ransac"]
    print("%d / %d points after downsampling, %d correspondences, %d inliers (rms %.4g)"
          % (info["source_down"].shape[0], info["target_down"].shape[0], info["correspondences"].shape[0], ran.n_inliers, ran.rms))
    for row in T:
        print(" ".join("%.9g" % v for v in row))
    return 0


if __name__ == "__main__":
    sys.exit(main())
