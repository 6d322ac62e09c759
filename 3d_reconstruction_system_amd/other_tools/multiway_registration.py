#!/usr/bin/env python3
"""Put N clouds into the frame of the first one on the MI355X: pairwise ICP along the sequence, global registration of the loop
candidates (every pair two or more apart), a pose graph with robust loop closures.

    python multiway_registration.py CLOUD CLOUD [CLOUD ...] --voxel-size V [--out-dir D]

CLOUD: PLY clouds (anything cloud_io.read_ply reads) or the reference's camera txt files (X,Y,Z per line), in sequence order:
cloud k + 1 must overlap cloud k.  D (default .) receives T_<k>.txt per cloud -- the 4x4 that moves cloud k into the frame of
cloud 0, in the format transfer_T_icp.py reads (get_T) -- and merged.ply, all moved clouds in one binary PLY.  When two
consecutive clouds cannot be registered nothing is written and the exit status is 1.
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
    p = argparse.ArgumentParser(description="Multiway registration of a sequence of point clouds (ICP + FPFH/RANSAC + pose graph).")
    p.add_argument("clouds", nargs="+", metavar="CLOUD", help="clouds in sequence order (.ply or .txt)")
    p.add_argument("--voxel-size", required=True, metavar="V", help="voxel size every cloud is downsampled to")
    p.add_argument("--out-dir", default=".", metavar="D", help="where T_<k>.txt and merged.ply go (default .)")
    args = p.parse_args(argv)
    try:
        args.voxel_size = float(args.voxel_size)
    except ValueError:
        p.error("V must be a number, got %r" % args.voxel_size)
    if not (math.isfinite(args.voxel_size) and args.voxel_size > 0.0):
        p.error("V must be finite and positive, got %r" % args.voxel_size)
    if len(args.clouds) < 2:
        p.error("need at least two clouds")
    for path in args.clouds:
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
    import numpy as np
    clouds = [read_cloud(r3d, path) for path in args.clouds]
    try:
        poses, graph, info = r3d.register_multiway(clouds, args.voxel_size, ctx=_common.context())
    except ValueError as e:
        print("no registration: %s" % e, file=sys.stderr)
        return 1
    os.makedirs(args.out_dir, exist_ok=True)
    moved = []
    for k, (cloud, T) in enumerate(zip(clouds, poses)):
        r3d.write_T(os.path.join(args.out_dir, "T_%d.txt" % k), T)
        moved.append(r3d.apply_T(cloud, T, ctx=_common.context()))
    r3d.cloud_io.write_ply_binary(os.path.join(args.out_dir, "merged.ply"), np.concatenate(moved))
    rep = info["report"]
    print("%d clouds, %d edges (%d loop closures, %d pruned, %d candidates rejected); cost %.6g -> %.6g in %d iterations"
          % (len(clouds), len(graph.edges), sum(1 for e in graph.edges if e[4]), rep["pruned"], len(info["rejected"]),
             rep["initial_cost"], rep["final_cost"], rep["iterations"]))
    return 0


if __name__ == "__main__":
    sys.exit(main())
