#!/usr/bin/env python3
"""Compare a reconstruction with the truth on the MI355X: the step the reference's readme leaves to CloudCompare.

    python compare_clouds.py RECON TRUTH --threshold T [--signed] [--hist BINS,WIDTH] [--ply OUT --ply-max D]

RECON and TRUTH: an `x,y,z` text cloud (cloud_io.read_xyz_txt), a PLY cloud (cloud_io.read_ply) or a PLY with faces in
cloud_io.write_ply_mesh's layout (read_ply_mesh).  The samples of a mesh are its vertices; distances go to the nearest triangle
of a mesh and to the nearest point of a cloud.  Prints ONE JSON line: accuracy and completeness (n, mean, rms, max, within),
precision, recall and f_score at the threshold, and the Chamfer distance (the sum of the two mean distances).
--signed (TRUTH must be a mesh): also the signed accuracy distances' mean, min and max (face-normal sign of the nearest triangle).
--hist BINS,WIDTH: also the histogram of the accuracy distances, BINS bins of WIDTH, the last one open.
--ply OUT: the reconstruction's samples coloured by their distance to the truth, blue (0) to red (--ply-max and beyond).
"""
import argparse
import json
import os
import sys

if __package__ in (None, ""):
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "transfer"))
    import _common  # type: ignore
else:
    from ..transfer import _common


def file_kind(path):
    """'txt', 'ply' or 'ply_mesh' (a PLY whose header announces faces), from the file's first bytes"""
    with open(path, "rb") as f:
        head = f.read(4096)
    if not head.startswith(b"ply"):
        return "txt"
    end = head.find(b"end_header")
    header = head if end < 0 else head[:end]
    for line in header.split(b"\n"):
        words = line.split()
        if len(words) == 3 and words[:2] == [b"element", b"face"] and int(words[2]) > 0:
            return "ply_mesh"
    return "ply"


def parse_hist(text):
    try:
        bins, width = text.split(",")
        bins, width = int(bins), float(width)
    except ValueError:
        raise argparse.ArgumentTypeError("expected BINS,WIDTH, got %r" % text) from None
    if not 1 <= bins <= 4096 or not 0.0 < width < float("inf"):
        raise argparse.ArgumentTypeError("BINS must be in [1, 4096] and WIDTH positive, got %r" % text)
    return bins, width


def parse_args(argv):
    p = argparse.ArgumentParser(description="Accuracy, completeness, F-score and Chamfer distance of a reconstruction against the truth.")
    p.add_argument("recon", help="reconstructed cloud or mesh (txt, PLY, PLY with faces)")
    p.add_argument("truth", help="true cloud or mesh (txt, PLY, PLY with faces)")
    p.add_argument("--threshold", type=float, required=True, help="distance below which a sample counts as correct / covered")
    p.add_argument("--signed", action="store_true", help="also report signed accuracy distances (TRUTH must be a mesh)")
    p.add_argument("--hist", type=parse_hist, default=None, metavar="BINS,WIDTH", help="also the histogram of the accuracy distances")
    p.add_argument("--ply", default=None, metavar="OUT", help="write the reconstruction's samples coloured by distance")
    p.add_argument("--ply-max", type=float, default=None, metavar="D", help="distance shown in full red (default: the threshold)")
    args = p.parse_args(argv)
    if not args.threshold >= 0.0:
        p.error("--threshold must be >= 0, got %r" % args.threshold)
    if args.ply_max is not None and args.ply is None:
        p.error("--ply-max needs --ply")
    if args.ply is not None:
        if args.ply_max is None:
            args.ply_max = args.threshold
        if not 0.0 < args.ply_max < float("inf"):
            p.error("--ply-max must be positive and finite, got %r" % args.ply_max)
    for path in (args.recon, args.truth):
        if not os.path.isfile(path):
            p.error("input file %r does not exist" % path)
    return args


def load(r3d, path):
    """an [N,3] cloud, or (vertices, triangles) for a PLY with faces"""
    kind = file_kind(path)
    if kind == "txt":
        return r3d.cloud_io.read_xyz_txt(path)
    if kind == "ply":
        return r3d.cloud_io.read_ply(path)
    xyz, _, tri = r3d.cloud_io.read_ply_mesh(path)
    return (xyz, tri)


def report(r3d, recon, truth, args, ctx):
    """the dict the tool prints, and the accuracy distances"""
    E = _common.module("evaluation")
    out, d_acc, _ = E.evaluate_reconstruction(recon, truth, args.threshold, ctx=ctx, return_distances=True)
    if args.signed:
        if not isinstance(truth, tuple):
            raise SystemExit("--signed needs a TRUTH with faces")
        samples = recon[0] if isinstance(recon, tuple) else recon
        sd, _ = E.cloud_to_mesh_distance(samples, truth[0], truth[1], signed=True, ctx=ctx)
        st = E.distance_stats(sd, ctx=ctx)
        out["signed_accuracy"] = {"n": st["n"], "mean": st["mean"], "min": st["min"], "max": st["max"]}
    if args.hist:
        st = E.distance_stats(d_acc, bin_width=args.hist[1], n_bins=args.hist[0], ctx=ctx)
        out["hist"] = {"bin_width": args.hist[1], "counts": [int(c) for c in st["hist"]]}
    return out, d_acc


def main(argv=None):
    args = parse_args(sys.argv[1:] if argv is None else argv)
    r3d = _common.package()
    ctx = _common.context()
    recon, truth = load(r3d, args.recon), load(r3d, args.truth)
    out, d_acc = report(r3d, recon, truth, args, ctx)
    if args.ply:
        E = _common.module("evaluation")
        samples = recon[0] if isinstance(recon, tuple) else recon
        r3d.cloud_io.write_ply_rgb(args.ply, samples, E.distance_colors(d_acc, args.ply_max, ctx=ctx))
    print(json.dumps(out, sort_keys=True))


if __name__ == "__main__":
    main()
