#!/usr/bin/env python3
"""RANSAC plane segmentation of a PLY cloud on the MI355X: plane after plane is peeled off the cloud.

    python segment_planes.py IN.ply OUT.ply [--threshold T] [--hypotheses H] [--max-planes P] [--min-inliers M] [--seed S]

IN.ply: any PLY cloud_io.read_ply reads (xyz only).  OUT.ply: every input point in its input order, coloured by its plane (a
fixed palette, grey for points on no plane), in the reference's coloured ASCII layout.  Prints one `a b c d count` line per
plane: unit normal, offset (a x + b y + c z + d = 0) and the number of points within T of it.
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

PALETTE = [(230, 25, 75), (60, 180, 75), (0, 130, 200), (255, 225, 25), (245, 130, 48), (145, 30, 180), (70, 240, 240),
           (240, 50, 230), (210, 245, 60), (0, 128, 128), (170, 110, 40), (128, 0, 0)]
GREY = (128, 128, 128)


def parse_args(argv):
    p = argparse.ArgumentParser(description="RANSAC plane segmentation of a PLY point cloud.")
    p.add_argument("input", help="input PLY (ASCII reference layout or binary float32)")
    p.add_argument("output", help="output PLY, coloured by plane")
    p.add_argument("--threshold", type=float, default=0.01, help="distance to the plane that still counts as on it (default 0.01)")
    p.add_argument("--hypotheses", type=int, default=1024, help="three-point samples per plane, 1..65536 (default 1024)")
    p.add_argument("--max-planes", type=int, default=6, help="stop after this many planes (default 6)")
    p.add_argument("--min-inliers", type=int, default=100, help="stop at the first plane with fewer points (default 100)")
    p.add_argument("--seed", type=int, default=0, help="sampler seed (default 0)")
    args = p.parse_args(argv)
    if not (math.isfinite(args.threshold) and args.threshold > 0.0):
        p.error("--threshold must be finite and positive, got %r" % args.threshold)
    if not 1 <= args.hypotheses <= 65536:
        p.error("--hypotheses must be in [1, 65536], got %d" % args.hypotheses)
    if args.max_planes < 0:
        p.error("--max-planes must be >= 0, got %d" % args.max_planes)
    if args.min_inliers < 1:
        p.error("--min-inliers must be >= 1, got %d" % args.min_inliers)
    if not 0 <= args.seed < 1 << 64:
        p.error("--seed must be in [0, 2^64), got %d" % args.seed)
    if not os.path.isfile(args.input):
        p.error("input file %r does not exist" % args.input)
    return args


def main(argv=None):
    import numpy as np
    args = parse_args(sys.argv[1:] if argv is None else argv)
    r3d = _common.package()
    seg = __import__(r3d.__name__ + ".segmentation", fromlist=["segment_planes"])
    xyz = r3d.cloud_io.read_ply(args.input).astype("float32")
    planes, labels, counts = seg.segment_planes(xyz, args.threshold, args.hypotheses, args.max_planes, args.min_inliers, args.seed,
                                                ctx=_common.context())
    colours = np.array(PALETTE + [GREY], np.uint8)
    rgb = colours[np.where(labels < 0, len(PALETTE), labels % len(PALETTE))]
    r3d.cloud_io.write_ply_rgb(args.output, xyz, rgb)
    for (a, b, c, d), k in zip(planes, counts):
        print("%.9g %.9g %.9g %.9g %d" % (a, b, c, d, k))


if __name__ == "__main__":
    main()
