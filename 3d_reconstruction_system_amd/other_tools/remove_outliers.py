#!/usr/bin/env python3
"""Statistical or radius outlier removal of a PLY cloud on the MI355X (exact k nearest neighbours on the GPU).

    python remove_outliers.py IN.ply OUT.ply --statistical K RATIO [--binary]
    python remove_outliers.py IN.ply OUT.ply --radius N R [--binary]

--statistical K RATIO: keep a point iff it has K neighbours and its mean distance to them is at most mean + RATIO * std over
all such points.  --radius N R: keep a point iff at least N other points lie within R.  IN.ply: any PLY cloud_io.read_ply reads
(xyz only); OUT.ply: the kept points in their input order, in the reference's ASCII layout or binary with --binary.
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
    p = argparse.ArgumentParser(description="Statistical or radius outlier removal of a PLY point cloud.")
    p.add_argument("input", help="input PLY (ASCII reference layout or binary float32)")
    p.add_argument("output", help="output PLY")
    mode = p.add_mutually_exclusive_group(required=True)
    mode.add_argument("--statistical", nargs=2, metavar=("K", "RATIO"),
                      help="K neighbours (1..32), keep mean distance <= mean + RATIO * std")
    mode.add_argument("--radius", nargs=2, metavar=("N", "R"), help="keep points with at least N neighbours within R")
    p.add_argument("--binary", action="store_true", help="write a binary little-endian PLY instead of the ASCII layout")
    args = p.parse_args(argv)

    def number(text, kind, what):
        try:
            return kind(text)
        except ValueError:
            p.error("%s must be %s, got %r" % (what, "an integer" if kind is int else "a number", text))

    if args.statistical:
        k, ratio = number(args.statistical[0], int, "K"), number(args.statistical[1], float, "RATIO")
        if not 1 <= k <= 32:
            p.error("K must be in [1, 32], got %d" % k)
        if not (math.isfinite(ratio) and ratio > 0.0):
            p.error("RATIO must be finite and positive, got %r" % ratio)
        args.params = (k, ratio)
    else:
        n, r = number(args.radius[0], int, "N"), number(args.radius[1], float, "R")
        if n < 1:
            p.error("N must be >= 1, got %d" % n)
        if not (math.isfinite(r) and r > 0.0):
            p.error("R must be finite and positive, got %r" % r)
        args.params = (n, r)
    if not os.path.isfile(args.input):
        p.error("input file %r does not exist" % args.input)
    return args


def main(argv=None):
    args = parse_args(sys.argv[1:] if argv is None else argv)
    r3d = _common.package()
    outliers = __import__(r3d.__name__ + ".outliers", fromlist=["remove_statistical_outlier"])
    xyz = r3d.cloud_io.read_ply(args.input).astype("float32")
    if args.statistical:
        out = outliers.remove_statistical_outlier(xyz, args.params[0], args.params[1], ctx=_common.context())
    else:
        out = outliers.remove_radius_outlier(xyz, args.params[0], args.params[1], ctx=_common.context())
    if args.binary:
        r3d.cloud_io.write_ply_binary(args.output, out.xyz)
    else:
        r3d.cloud_io.write_ply(args.output, out.xyz)
    n, kept = xyz.shape[0], out.xyz.shape[0]
    print("%d -> %d (%d removed)" % (n, kept, n - kept))


if __name__ == "__main__":
    main()
