#!/usr/bin/env python3
"""Voxel-grid downsampling of a PLY cloud on the MI355X: one point per occupied voxel, at the centroid of its points.

    python voxel_down_sample.py IN.ply OUT.ply [--voxel-size 0.1] [--binary]

IN.ply: any PLY cloud_io.read_ply reads (the reference's ASCII layout that camera_to_world.py writes, or a binary float32
one).  OUT.ply: the centroids in the reference's ASCII layout, or as a binary little-endian PLY with --binary.  Points that
have no voxel (non-finite, beyond +-32768 voxels from the origin) are ignored and counted.
"""
import argparse
import os
import sys

if __package__ in (None, ""):
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "transfer"))
    import _common  # type: ignore
else:
    from ..transfer import _common


def parse_args(argv):
    p = argparse.ArgumentParser(description="Voxel-grid downsampling of a PLY point cloud (one centroid per occupied voxel).")
    p.add_argument("input", help="input PLY (ASCII reference layout or binary float32)")
    p.add_argument("output", help="output PLY")
    p.add_argument("--voxel-size", type=float, default=0.1, help="voxel edge length, in the cloud's unit (default 0.1)")
    p.add_argument("--binary", action="store_true", help="write a binary little-endian PLY instead of the ASCII layout")
    args = p.parse_args(argv)
    if not args.voxel_size > 0.0:
        p.error("--voxel-size must be positive, got %r" % args.voxel_size)
    if not os.path.isfile(args.input):
        p.error("input file %r does not exist" % args.input)
    return args


def main(argv=None):
    args = parse_args(sys.argv[1:] if argv is None else argv)
    r3d = _common.package()
    voxelmap = __import__(r3d.__name__ + ".voxelmap", fromlist=["VoxelGrid"])
    xyz = r3d.cloud_io.read_ply(args.input).astype("float32")
    vg = voxelmap.VoxelGrid(args.voxel_size, max(1 << 10, 2 * xyz.shape[0]), ctx=_common.context())
    try:
        vg.insert(xyz)
        ignored = vg.stats()["ignored_points"]
        out = vg.extract()
    finally:
        vg.close()
    if args.binary:
        r3d.cloud_io.write_ply_binary(args.output, out.xyz)
    else:
        r3d.cloud_io.write_ply(args.output, out.xyz)
    print("%d points -> %d voxels (%d ignored)" % (xyz.shape[0], out.xyz.shape[0], ignored))


if __name__ == "__main__":
    main()
