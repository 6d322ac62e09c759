#!/usr/bin/env python3
"""Normals of a PLY cloud on the MI355X (k nearest neighbours, covariance and eigenvector in one GPU launch).

    python estimate_normals.py IN.ply OUT.ply --k K [--radius R] [--viewpoint X Y Z]

Every point gets the unit normal of the plane through its K nearest neighbours (those within R when --radius is given),
turned towards --viewpoint when given, otherwise so that its largest component is positive.  IN.ply: any PLY
cloud_io.read_ply reads (xyz only); OUT.ply: binary little-endian, float x y z nx ny nz per vertex, in the input order
(cloud_io.read_ply_normals reads it back).  A point without a plane keeps a zero normal.
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
    p = argparse.ArgumentParser(description="Estimate oriented normals of a PLY point cloud.")
    p.add_argument("input", help="input PLY (ASCII reference layout or binary float32)")
    p.add_argument("output", help="output PLY (binary, with normals)")
    p.add_argument("--k", required=True, metavar="K", help="neighbours per point (3..32)")
    p.add_argument("--radius", metavar="R", help="use only the neighbours within R")
    p.add_argument("--viewpoint", nargs=3, metavar=("X", "Y", "Z"), help="turn every normal towards this position")
    args = p.parse_args(argv)

    def number(text, kind, what):
        try:
            return kind(text)
        except ValueError:
            p.error("%s must be %s, got %r" % (what, "an integer" if kind is int else "a number", text))

    args.k = number(args.k, int, "K")
    if not 3 <= args.k <= 32:
        p.error("K must be in [3, 32], got %d" % args.k)
    if args.radius is not None:
        args.radius = number(args.radius, float, "R")
        if not (math.isfinite(args.radius) and args.radius > 0.0):
            p.error("R must be finite and positive, got %r" % args.radius)
    if args.viewpoint is not None:
        args.viewpoint = tuple(number(v, float, "X Y Z") for v in args.viewpoint)
        if not all(math.isfinite(v) for v in args.viewpoint):
            p.error("X Y Z must be finite, got %r" % (args.viewpoint,))
    if not os.path.isfile(args.input):
        p.error("input file %r does not exist" % args.input)
    return args


def main(argv=None):
    args = parse_args(sys.argv[1:] if argv is None else argv)
    r3d = _common.package()
    normals = __import__(r3d.__name__ + ".normals", fromlist=["estimate_normals"])
    xyz = r3d.cloud_io.read_ply(args.input).astype("float32")
    out = normals.estimate_normals(xyz, args.k, radius=args.radius, viewpoint=args.viewpoint, ctx=_common.context())
    r3d.cloud_io.write_ply_normals(args.output, xyz, out.normals)
    print("%d points, %d without a normal" % (xyz.shape[0], int((out.normals == 0).all(axis=1).sum())))


if __name__ == "__main__":
    main()
