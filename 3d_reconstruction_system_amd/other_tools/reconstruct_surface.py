#!/usr/bin/env python3
"""A triangle mesh from an oriented point cloud on the MI355X: the step behind the fused cloud.

    python reconstruct_surface.py CLOUD.ply OUT.ply --voxel-size V [--trunc-voxels N] [--knn K --viewpoint X,Y,Z]
                                  [--mesh-min-component N] [--mesh-largest] [--mesh-smooth METHOD,ITERATIONS[,LAM[,MU]]]

CLOUD.ply is a binary PLY with normals (cloud_io.write_ply_normals' layout: float x y z nx ny nz, with or without uchar red
green blue -- what estimate_normals.py and integrate_tsdf.py write), the normals pointing out of the surface.  Every voxel (edge
V) within N voxels (default 4) of the cloud takes the signed distance to the tangent plane of its nearest point, and OUT.ply gets
the marching-cubes mesh of that field (cloud_io.write_ply_mesh's layout), with the nearest points' colours when the cloud has them.
A PLY WITHOUT normals (the reference's ASCII layout, or write_ply_binary's) gets them estimated from its K nearest neighbours
(--knn, default 20) and oriented towards --viewpoint, a position the surface was seen from; without --viewpoint such a file is
refused: an orientation cannot be guessed.  Normals that the file has are used as they stand: --knn and --viewpoint do not
replace them.  --mesh-min-component / --mesh-largest / --mesh-smooth are integrate_tsdf.py's.
Prints "points P voxels NX NY NZ touched T vertices V triangles M -> OUT.ply".
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
    p = argparse.ArgumentParser(description="Reconstruct the surface of an oriented point cloud as a triangle mesh.")
    p.add_argument("cloud", metavar="CLOUD.ply")
    p.add_argument("out", metavar="OUT.ply")
    p.add_argument("--voxel-size", type=float, required=True, help="edge of a voxel: the resolution of the mesh")
    p.add_argument("--trunc-voxels", type=int, default=4, help="truncation distance in voxels (default 4)")
    p.add_argument("--knn", type=int, default=None, help="for a cloud without normals: neighbours per normal (default 20)")
    p.add_argument("--viewpoint", metavar="X,Y,Z", default=None,
                   help="for a cloud without normals: a position the surface was seen from; the normals point towards it")
    p.add_argument("--mesh-min-component", type=int, metavar="N", default=None, help="drop connected pieces of fewer than N triangles")
    p.add_argument("--mesh-largest", action="store_true", help="keep only the connected piece with the most triangles")
    p.add_argument("--mesh-smooth", metavar="METHOD,ITERATIONS[,LAM[,MU]]", default=None,
                   help="smooth the mesh (taubin or laplacian) and recompute its vertex normals, e.g. taubin,10")
    args = p.parse_args(argv)
    if not (math.isfinite(args.voxel_size) and args.voxel_size > 0.0):
        p.error("--voxel-size must be finite and positive, got %r" % args.voxel_size)
    if args.trunc_voxels < 1:
        p.error("--trunc-voxels must be >= 1, got %r" % args.trunc_voxels)
    if args.knn is not None and not 3 <= args.knn <= 32:
        p.error("--knn must be in 3..32, got %r" % args.knn)
    if args.knn is not None and args.viewpoint is None:
        p.error("--knn needs --viewpoint: estimated normals have no orientation without one")
    if args.viewpoint is not None:
        try:
            args.viewpoint = [float(v) for v in args.viewpoint.split(",")]
            if len(args.viewpoint) != 3 or not all(math.isfinite(v) for v in args.viewpoint):
                raise ValueError
        except ValueError:
            p.error("--viewpoint takes X,Y,Z (three finite numbers), got %r" % (args.viewpoint,))
    if args.mesh_min_component is not None and args.mesh_min_component < 1:
        p.error("--mesh-min-component must be >= 1, got %r" % args.mesh_min_component)
    if args.mesh_smooth is not None:
        try:
            parts = args.mesh_smooth.split(",")
            if len(parts) not in (2, 3, 4):
                raise ValueError
            smooth = {"method": parts[0], "iterations": int(parts[1])}
            smooth.update(zip(("lam", "mu"), (float(v) for v in parts[2:])))
        except ValueError:
            p.error("--mesh-smooth takes METHOD,ITERATIONS[,LAM[,MU]] (a name, an integer, up to two numbers), got %r" % args.mesh_smooth)
        try:
            args.mesh_smooth = _common.package().mesh.smooth_params(smooth)
        except ValueError as e:
            p.error("--mesh-smooth: %s" % e)
    return args


def read_cloud(r3d, args):
    """(xyz, normals, rgb or None) of the input: the file's normals, or estimated ones oriented to --viewpoint"""
    import numpy as np
    try:
        return r3d.cloud_io.read_ply_normals(args.cloud, with_colors=True)      # the file's normals stand, whatever --viewpoint says
    except ValueError as e:
        # only "this PLY has another layout" sends the file to the plain reader; a PLY with normals that is broken says so
        if "must start with float x y z nx ny nz" not in str(e) and "not a binary little-endian PLY" not in str(e):
            sys.exit("reconstruct_surface.py: %s" % e)
        try:
            xyz, rgb = np.ascontiguousarray(r3d.cloud_io.read_ply(args.cloud), dtype=np.float32), None
        except ValueError as plain:
            sys.exit("reconstruct_surface.py: %s" % plain)
    if args.viewpoint is None:
        sys.exit("reconstruct_surface.py: %s has no normals and no --viewpoint was given: the orientation of a surface cannot be "
                 "guessed (give --viewpoint X,Y,Z, or write oriented normals with estimate_normals.py)" % args.cloud)
    est = r3d.estimate_normals(xyz, k=20 if args.knn is None else args.knn, viewpoint=args.viewpoint, ctx=_common.context())
    return xyz, est.normals, rgb


def main(argv=None):
    args = parse_args(sys.argv[1:] if argv is None else argv)
    r3d = _common.package()
    if not os.path.isfile(args.cloud):
        sys.exit("reconstruct_surface.py: %s not found" % args.cloud)
    xyz, normals, rgb = read_cloud(r3d, args)
    try:
        vol = r3d.volume_for_cloud(xyz, args.voxel_size, args.trunc_voxels, color=rgb is not None, ctx=_common.context())
    except ValueError as e:
        sys.exit("reconstruct_surface.py: %s" % e)
    touched = vol.integrate_cloud(xyz, normals, rgb)
    mesh = vol.extract_triangle_mesh(1.0, with_colors=rgb is not None, min_component_triangles=args.mesh_min_component,
                                     keep_largest=args.mesh_largest, smooth=args.mesh_smooth)
    dims = vol.dims
    vol.close()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    r3d.cloud_io.write_ply_mesh(args.out, *mesh)
    print("points %d voxels %d %d %d touched %d vertices %d triangles %d -> %s"
          % (len(xyz), dims[0], dims[1], dims[2], touched, len(mesh[0]), len(mesh[2]), args.out))


if __name__ == "__main__":
    main()
