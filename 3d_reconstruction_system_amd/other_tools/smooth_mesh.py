#!/usr/bin/env python3
"""Smooth a mesh PLY on the MI355X: python smooth_mesh.py IN.ply OUT.ply [METHOD,ITERATIONS[,LAM[,MU]]] (default taubin,10).  IN is a
PLY in cloud_io.write_ply_mesh's layout (what integrate_tsdf.py --mesh writes); OUT gets the moved vertices, the area-weighted
vertex normals of the moved mesh, and the faces and colours of IN.  Open edges stay where they are (mesh.smooth_mesh)."""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
r3d = __import__(os.path.basename(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))

if __name__ == "__main__":
    if len(sys.argv) not in (3, 4):
        sys.exit(__doc__)
    parts = (sys.argv[3] if len(sys.argv) == 4 else "taubin,10").split(",")
    kw = dict(zip(("method", "iterations", "lam", "mu"), [parts[0], int(parts[1])] + [float(v) for v in parts[2:]]))
    xyz, normals, tri, rgb = r3d.cloud_io.read_ply_mesh(sys.argv[1], with_colors=True)
    xyz, normals = r3d.smooth_mesh(xyz, tri, normals=normals, **kw)
    r3d.cloud_io.write_ply_mesh(sys.argv[2], xyz, normals, tri, rgb)
    print("vertices %d triangles %d -> %s" % (len(xyz), len(tri), sys.argv[2]))
