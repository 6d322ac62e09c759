#!/usr/bin/env python3
"""Cloud fusion of a drop-in working directory with multi-view depth consistency filtering on the MI355X: the cloud
camera_to_world.py fuses, without the pixels that the neighbouring frames' depth maps contradict (floaters, sky, smeared edges).

    python fuse_consistent.py [--radius R] [--rel-tol T] [--min-consistent N] [--max-violations M] [--color-dir DIR] [--out PATH]

Run from a directory holding ./camera_pose/image_colmap_simi_2.txt and ./depth/ (the inputs of camera_to_world.py; the same
environment overrides apply: R3D_FX .. R3D_CY, R3D_POSE_SCALE, R3D_DEVICE).  Every frame asks the R frames before and after it in the
pose file (default 2) where each of its pixels lies in them: a neighbour whose depth there agrees within T (relative to the depth,
default 0.01) votes for the pixel, one that sees farther votes against it.  A pixel stays with at least N votes for it (default 2)
and at most M against it (default 0); a pixel without a depth never stays.  T has to cover the depth noise and, on slanted
surfaces, the half pixel of the nearest-pixel lookup.  Writes ./ply/fused_consistent.ply (or PATH) in the reference's PLY layout, the
kept points in the order camera_to_world.py emits them, and prints "frames F pixels P kept K dropped D -> path".
--color-dir DIR reads the colour image DIR/<frame name> of every frame (the size of the depth maps) and writes the coloured PLY of
the reference layout.  camera_to_world.py itself is unchanged: it keeps writing every pixel.
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

POSE_FILE = './camera_pose/image_colmap_simi_2.txt'
OUT_FILE = './ply/fused_consistent.ply'


def add_rule_arguments(p):
    p.add_argument("--radius", type=int, default=2, help="frames before and after a frame that are its sources (1..8, default 2)")
    p.add_argument("--rel-tol", type=float, default=0.01, help="relative depth difference that still agrees (default 0.01)")
    p.add_argument("--min-consistent", type=int, default=2, help="agreeing sources a pixel needs (0..255, default 2)")
    p.add_argument("--max-violations", type=int, default=0, help="sources that may see past a pixel (0..255, default 0)")


def check_rule(p, radius, rel_tol, min_consistent, max_violations):
    if not 1 <= radius <= 8:
        p.error("the radius must be in 1..8, got %r" % radius)
    if not (math.isfinite(rel_tol) and rel_tol > 0.0):
        p.error("the relative tolerance must be finite and > 0, got %r" % rel_tol)
    if not (0 <= min_consistent <= 255 and 0 <= max_violations <= 255):
        p.error("the vote thresholds must be in 0..255, got %r and %r" % (min_consistent, max_violations))


def parse_args(argv):
    p = argparse.ArgumentParser(description="Fuse ./depth/ + the pose file into a cloud without multi-view inconsistent pixels.")
    add_rule_arguments(p)
    p.add_argument("--color-dir", metavar="DIR", default=None, help="attach the colour images DIR/<frame name> and write a coloured PLY")
    p.add_argument("--out", metavar="PATH", default=OUT_FILE, help="the PLY to write (default %s)" % OUT_FILE)
    args = p.parse_args(argv)
    check_rule(p, args.radius, args.rel_tol, args.min_consistent, args.max_violations)
    return args


def main(argv=None):
    args = parse_args(sys.argv[1:] if argv is None else argv)
    r3d = _common.package()
    if not os.path.isfile(POSE_FILE):
        sys.exit("fuse_consistent.py: %s not found (run from the data directory)" % POSE_FILE)
    names, quats, ts = r3d.read_pose_file(POSE_FILE)
    if not names:
        sys.exit("fuse_consistent.py: %s lists no frames" % POSE_FILE)
    ts = ts * _common.pose_scale()
    depths = r3d.cloud_io.read_depth_batch([os.path.join('./depth/', n) for n in names])
    rgb = None
    if args.color_dir is not None:
        paths = [os.path.join(args.color_dir, n) for n in names]
        for path in paths:
            if not os.path.isfile(path):
                sys.exit("fuse_consistent.py: colour image %s not found (--color-dir needs one image per frame of the pose file)" % path)
        rgb = r3d.cloud_io.read_rgb_batch(paths)
        if rgb.shape[1:3] != depths.shape[-2:]:
            sys.exit("fuse_consistent.py: the colour images are %d x %d, the depth maps %d x %d" % (rgb.shape[1:3] + depths.shape[-2:]))
    _common.stamp("read %d frames" % len(names))
    got = r3d.fuse_frames_consistent(depths, quats, ts, intrinsics=_common.intrinsics(), radius=args.radius, rel_tol=args.rel_tol,
                                     min_consistent=args.min_consistent, max_violations=args.max_violations, rgb=rgb,
                                     ctx=_common.context())
    _common.stamp("filter + fuse")
    xyz, keep = got[0], got[-1]
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    if rgb is None:
        r3d.cloud_io.write_ply(args.out, xyz)
    else:
        r3d.cloud_io.write_ply_rgb(args.out, xyz, got[1])
    print("frames %d pixels %d kept %d dropped %d -> %s" % (len(names), keep.size, len(xyz), keep.size - len(xyz), args.out))


if __name__ == "__main__":
    main()
