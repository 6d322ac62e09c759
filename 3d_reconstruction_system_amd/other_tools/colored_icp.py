#!/usr/bin/env python3
"""Register two coloured clouds on the MI355X with coloured ICP (geometry + colour: works on one wall, a floor, a corridor).

    python colored_icp.py SRC.ply TGT.ply [--init T.txt] [--voxel V [V ...]] [--iters N [N ...]] [--max-dist D] [--k K]
                          [--i-max I] [--lambda L] -o T_data.txt

SRC.ply / TGT.ply: ASCII PLYs in the reference's coloured layout (x y z red green blue alpha per row, what write_ply_rgb and
pixel_to_camera.py write; cloud_io.read_ply_rgb).  --init: a 4x4 in the format transfer_T_icp.py reads (get_T).  Without --voxel
the clouds are registered as they are (icp_colored, --iters one number, default 30); with --voxel, coarse to fine over those
voxel sizes (register_colored, --iters one number per size).  The 4x4 that moves SRC onto TGT is written to -o in get_T's format
and printed.  On a usage error, and when a step was undefined (status 1), the exit code is 1 and nothing is written.
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


class _Parser(argparse.ArgumentParser):
    def error(self, message):
        self.print_usage(sys.stderr)
        print("%s: error: %s" % (self.prog, message), file=sys.stderr)
        raise SystemExit(1)


def parse_args(argv):
    p = _Parser(description="Coloured ICP of two coloured point clouds.")
    p.add_argument("source", help="coloured cloud to move (.ply)")
    p.add_argument("target", help="coloured cloud to move it onto (.ply)")
    p.add_argument("-o", "--out-T", required=True, metavar="PATH", help="where the 4x4 goes")
    p.add_argument("--init", metavar="T.txt", help="rough pose, a 4x4 text file")
    p.add_argument("--voxel", nargs="+", metavar="V", help="voxel sizes, coarse to fine")
    p.add_argument("--iters", nargs="+", metavar="N", help="iterations (one per voxel size)")
    p.add_argument("--max-dist", metavar="D", help="pairs farther apart never take part (without --voxel)")
    p.add_argument("--k", default="8", metavar="K")
    p.add_argument("--i-max", default="40", metavar="I")
    p.add_argument("--lambda", dest="lam", default="0.968", metavar="L", help="weight of the geometric term, in (0, 1]")
    args = p.parse_args(argv)

    def number(text, kind, what):
        try:
            return kind(text)
        except ValueError:
            p.error("%s must be %s, got %r" % (what, "an integer" if kind is int else "a number", text))

    def positive(text, what):
        v = number(text, float, what)
        if not (math.isfinite(v) and v > 0.0):
            p.error("%s must be finite and positive, got %r" % (what, v))
        return v

    args.voxel = None if args.voxel is None else [positive(v, "V") for v in args.voxel]
    n_scales = 1 if args.voxel is None else len(args.voxel)
    args.iters = [30] * n_scales if args.iters is None else [number(v, int, "N") for v in args.iters]
    if len(args.iters) != n_scales or any(i < 1 for i in args.iters):
        p.error("--iters needs %d integer(s) >= 1, got %r" % (n_scales, args.iters))
    args.max_dist = None if args.max_dist is None else positive(args.max_dist, "D")
    if args.max_dist is not None and args.voxel is not None:
        p.error("--max-dist goes without --voxel (the scales set their own gate)")
    args.k, args.i_max, args.lam = number(args.k, int, "K"), positive(args.i_max, "I"), number(args.lam, float, "L")
    if not 3 <= args.k <= 32:
        p.error("K must be in [3, 32], got %d" % args.k)
    if not 0.0 < args.lam <= 1.0:
        p.error("L must be in (0, 1], got %r" % args.lam)
    for path in (args.source, args.target) + ((args.init,) if args.init else ()):
        if not os.path.isfile(path):
            p.error("input file %r does not exist" % path)
    return args


def main(argv=None):
    args = parse_args(sys.argv[1:] if argv is None else argv)
    r3d = _common.package()
    try:
        (src, src_w), (tgt, tgt_w) = r3d.cloud_io.read_ply_rgb(args.source), r3d.cloud_io.read_ply_rgb(args.target)
        init = None if args.init is None else r3d.get_T(args.init)
    except ValueError as e:
        print("colored_icp.py: error: %s" % e, file=sys.stderr)
        return 1
    src, tgt = src.astype("float32"), tgt.astype("float32")
    try:
        if args.voxel is None:
            T, info = r3d.icp_colored(src, src_w, tgt, tgt_w, init=init, max_iter=args.iters[0], max_dist=args.max_dist,
                                      lambda_geometric=args.lam, i_max=args.i_max, k=args.k, ctx=_common.context())
        else:
            T, info = r3d.register_colored(src, src_w, tgt, tgt_w, voxel_sizes=args.voxel, iters=args.iters, init=init, k=args.k,
                                           i_max=args.i_max, lambda_geometric=args.lam, ctx=_common.context())
            info = info["scales"][-1]
    except ValueError as e:
        print("no registration: %s" % e, file=sys.stderr)
        return 1
    if info["status"]:
        print("no registration: a step was undefined (geometry and colour together leave a freedom open, or too few pairs)",
              file=sys.stderr)
        return 1
    r3d.write_T(args.out_T, T)
    print("%d geometric / %d photometric pairs, rms %.4g, photometric rms %.4g, %d iterations"
          % (info["pairs"], info["photo_pairs"], info["rms"], info["photo_rms"], info["iterations"]))
    for row in T:
        print(" ".join("%.9g" % v for v in row))
    return 0


if __name__ == "__main__":
    sys.exit(main())
