#!/usr/bin/env python3
"""TSDF integration of a drop-in working directory on the MI355X: the frames camera_to_world.py fuses into a cloud are averaged in a
truncated signed distance volume instead, and the volume's zero level set is written as oriented surface points.

    python integrate_tsdf.py --voxel-size S --trunc T [--origin X Y Z] [--dims NX NY NZ] [--margin M] [--min-weight W]
                             [--mesh [--mesh-min-component N] [--mesh-largest]
                                     [--mesh-smooth METHOD,ITERATIONS[,LAM[,MU]] [--mesh-smooth-free-boundary]]]
                             [--consistency RADIUS,REL_TOL,MIN[,MAX_VIOL]]
                             [--raycast] [--color-dir DIR] [--raycast-color] [--track [--track-pyramid N0,N1,..] [--track-bilateral R,SIGMA_S,SIGMA_R] [--track-color [--photo-weight W] [--track-max-jump D]]]

Run from a directory holding ./camera_pose/image_colmap_simi_2.txt and ./depth/ (the inputs of camera_to_world.py; the same
environment overrides apply: R3D_FX .. R3D_CY, R3D_POSE_SCALE, R3D_DEVICE).  Writes ./ply/tsdf_surface.ply: binary PLY, float
x y z nx ny nz, the normals pointing towards the cameras.  Without --origin / --dims the volume is the bounding box of the camera
centres padded by M on every side (default M = 16 T), cut into voxels of S.  A depth of 0 is "no measurement".
--mesh also writes ./ply/tsdf_mesh.ply: the same vertices plus the marching-cubes triangles over them (a face element MeshLab
shades), and prints a second line "triangles M -> path".
--mesh-min-component N / --mesh-largest (with --mesh) clean the mesh of floaters on the device before it is written: connected
pieces (triangles that share a vertex) of fewer than N triangles are dropped, and with --mesh-largest all but the piece with the
most triangles; vertices no kept triangle names go with them, so the mesh file then has fewer vertices than the surface file.
A line "components C kept K triangles kept M dropped D" is printed in front of the "triangles" line.
--mesh-smooth METHOD,ITERATIONS[,LAM[,MU]] (with --mesh) smooths the mesh on the device, behind the component filter, before it
is written: METHOD taubin (ITERATIONS times a LAM step then a MU step; defaults 0.5 and -0.53; the surface does not shrink) or
laplacian (ITERATIONS LAM steps), e.g. taubin,10.  Every step moves a vertex towards (or, for MU, away from) the mean of its
neighbours; the vertices on an open edge stay where they are unless --mesh-smooth-free-boundary is given.  The normals of the mesh
file are then the area-weighted vertex normals of the moved mesh; faces, colours and counts are as without the flag.  A line
"smoothed vertices N edges E boundary B steps S" is printed in front of the "triangles" line.
--consistency RADIUS,REL_TOL,MIN[,MAX_VIOL] (not with --track: it needs every pose) runs the multi-view depth consistency filter
over the depth maps first and integrates the filtered rasters instead of the raw ones: a pixel stays when at least MIN of the
RADIUS frames before and after its own see a surface within REL_TOL (relative) of where it says one is and at most MAX_VIOL
(default 0) see past it, e.g. 2,0.01,2; a floater no longer carves the volume.  A line "consistency kept K of P pixels" is printed.
--raycast also casts the volume from every pose of the pose file at the input rasters' size and writes the depth the model
predicts (float32, 0 = no surface) to ./raycast/<frame name>.npy, and prints a further line "raycast F frames -> ./raycast/".
--color-dir DIR reads the colour image DIR/<frame name> of every frame (the size of the depth maps), integrates colour with the
depth and adds uchar red green blue to the vertices of both PLY files.
--raycast-color (with --color-dir) also casts the colour image the model predicts from every pose of the pose file at the input
rasters' size and writes it (uint8 [H,W,3], R, G, B; 0, 0, 0 = no surface) to ./raycast_color/<frame name>.npy, and prints a
further line "raycast colour F frames -> ./raycast_color/".
--track reconstructs from the depth maps and ONE pose: only the first row of the pose file is used (its names still list the
frames).  A pose file that is missing or lists no frame gives the identity as the first pose and the files of ./depth/ in
sorted order as the frames (--origin / --dims are then the caller's to choose around a camera at the origin).  Every later
frame is tracked against the model from the previous frame's pose (projective point-to-plane ICP on the ray-cast maps: small
motions between frames) and integrated at the pose found.  The estimated poses are written to
./camera_pose/image_colmap_simi_2_tracked.txt in the pose file's own format, and a further line "tracked F frames -> path" is
printed.  Without --origin / --dims the volume is then built around the first camera centre alone.  Not with --color-dir, unless:
--track-color (with --track and --color-dir; not with --track-pyramid) tracks every frame with a photometric term next to the
geometric one -- the frame's colour image against the one the model predicts -- and integrates the colour images, so the PLY
files carry colour.  It holds what planes alone leave open: sliding along a corridor, over a wall or a floor.
--photo-weight W is the weight of a photometric pair against a geometric pair's 1, in (length unit)^2 per intensity^2 (default:
tracking.PHOTO_WEIGHT, chosen for metres); --track-max-jump D the depth step, in length units, across which no image gradient
is taken (default 0.05, for metres).  Both scale with the unit of the depth maps.
--track-pyramid N0,N1,.. (with --track) tracks coarse to fine over a depth pyramid: N0 iterations at full size, N1 on the halved
rasters and so on, e.g. 10,5,4; the coarse levels run first and let the loop follow larger motions between frames.
--track-bilateral R,SIGMA_S,SIGMA_R (with --track; combines with --track-pyramid and --track-color) tracks every frame on a
bilateral-filtered copy of its depth map -- a window of (2 R + 1)^2 pixels, SIGMA_S in pixels, SIGMA_R in length units; depths
more than 3 SIGMA_R apart never mix -- which keeps sensor noise out of the normals and residuals; the raw maps are integrated.
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
OUT_FILE = './ply/tsdf_surface.ply'
MESH_FILE = './ply/tsdf_mesh.ply'
RAYCAST_DIR = './raycast/'
RAYCAST_COLOR_DIR = './raycast_color/'
TRACKED_FILE = './camera_pose/image_colmap_simi_2_tracked.txt'


def parse_args(argv):
    p = argparse.ArgumentParser(description="Integrate ./depth/ + the pose file into a TSDF volume and write its surface points.")
    p.add_argument("--voxel-size", type=float, required=True, help="edge of a voxel, in the depth maps' unit")
    p.add_argument("--trunc", type=float, required=True, help="truncation distance of the signed distance (a few voxels)")
    p.add_argument("--origin", type=float, nargs=3, metavar=("X", "Y", "Z"), help="corner of voxel (0, 0, 0)")
    p.add_argument("--dims", type=int, nargs=3, metavar=("NX", "NY", "NZ"), help="voxels per axis")
    p.add_argument("--margin", type=float, default=None,
                   help="padding of the camera centres' bounding box when --origin / --dims are not given (default 16 x --trunc)")
    p.add_argument("--min-weight", type=float, default=1.0, help="frames a voxel needs to count (default 1)")
    p.add_argument("--mesh", action="store_true", help="also write the triangle mesh of the surface to %s" % MESH_FILE)
    p.add_argument("--mesh-min-component", type=int, metavar="N", default=None,
                   help="with --mesh: drop the connected pieces of the mesh that have fewer than N triangles")
    p.add_argument("--mesh-largest", action="store_true", help="with --mesh: keep only the connected piece with the most triangles")
    p.add_argument("--mesh-smooth", metavar="METHOD,ITERATIONS[,LAM[,MU]]", default=None,
                   help="with --mesh: smooth the mesh (taubin or laplacian) and recompute its vertex normals, e.g. taubin,10")
    p.add_argument("--mesh-smooth-free-boundary", action="store_true",
                   help="with --mesh-smooth: move the vertices on open edges too (default: they stay)")
    p.add_argument("--consistency", metavar="RADIUS,REL_TOL,MIN[,MAX_VIOL]", default=None,
                   help="integrate the depth maps filtered by multi-view consistency: sources RADIUS frames either side, relative "
                        "tolerance, agreeing sources needed, sources that may see past a pixel (default 0), e.g. 2,0.01,2")
    p.add_argument("--raycast", action="store_true",
                   help="also ray-cast the volume from every pose and write the predicted depth to %s<frame name>.npy" % RAYCAST_DIR)
    p.add_argument("--color-dir", metavar="DIR", default=None,
                   help="integrate the colour images DIR/<frame name> too and write the colours into the PLY files")
    p.add_argument("--raycast-color", action="store_true",
                   help="with --color-dir: also ray-cast the colour image from every pose and write it to %s<frame name>.npy"
                   % RAYCAST_COLOR_DIR)
    p.add_argument("--track", action="store_true",
                   help="use only the first pose of the pose file, estimate the others by tracking and write them to %s" % TRACKED_FILE)
    p.add_argument("--track-pyramid", metavar="N0,N1,..", default=None,
                   help="with --track: iterations per pyramid level, fine to coarse (e.g. 10,5,4): track coarse to fine")
    p.add_argument("--track-bilateral", metavar="R,SIGMA_S,SIGMA_R", default=None,
                   help="with --track: track on a bilateral-filtered copy of every frame (window radius in pixels, sigma in pixels, "
                        "sigma in length units, e.g. 3,2.0,0.03); the raw frames are integrated")
    p.add_argument("--track-color", action="store_true",
                   help="with --track and --color-dir: track with the colour term too and integrate the colour images")
    p.add_argument("--photo-weight", type=float, default=None,
                   help="with --track-color: weight of a photometric pair, (length unit)^2 per intensity^2 (default: for metres)")
    p.add_argument("--track-max-jump", type=float, default=None,
                   help="with --track-color: depth step across which no image gradient is taken (default 0.05)")
    args = p.parse_args(argv)
    if (args.mesh_min_component is not None or args.mesh_largest) and not args.mesh:
        p.error("--mesh-min-component and --mesh-largest need --mesh")
    if args.mesh_min_component is not None and args.mesh_min_component < 1:
        p.error("--mesh-min-component must be >= 1, got %r" % args.mesh_min_component)
    if args.mesh_smooth is not None and not args.mesh:
        p.error("--mesh-smooth needs --mesh")
    if args.mesh_smooth_free_boundary and args.mesh_smooth is None:
        p.error("--mesh-smooth-free-boundary needs --mesh-smooth")
    if args.mesh_smooth is not None:
        try:
            parts = args.mesh_smooth.split(",")
            if len(parts) not in (2, 3, 4):
                raise ValueError
            smooth = {"method": parts[0], "iterations": int(parts[1])}
            smooth.update(zip(("lam", "mu"), (float(v) for v in parts[2:])))
        except ValueError:
            p.error("--mesh-smooth takes METHOD,ITERATIONS[,LAM[,MU]] (a name, an integer, up to two numbers), got %r" % args.mesh_smooth)
        smooth["lock_boundary"] = not args.mesh_smooth_free_boundary
        try:
            args.mesh_smooth = _common.package().mesh.smooth_params(smooth)
        except ValueError as e:
            p.error("--mesh-smooth: %s" % e)
    if (args.photo_weight is not None or args.track_max_jump is not None) and not args.track_color:
        p.error("--photo-weight and --track-max-jump need --track-color")
    if args.track_pyramid is not None:
        if not args.track:
            p.error("--track-pyramid needs --track")
        try:
            args.track_pyramid = [int(v) for v in args.track_pyramid.split(",")]
        except ValueError:
            p.error("--track-pyramid takes integers separated by commas, got %r" % args.track_pyramid)
        if not 1 <= len(args.track_pyramid) <= 8 or min(args.track_pyramid) < 0:
            p.error("--track-pyramid takes 1 to 8 iteration counts >= 0, got %r" % (args.track_pyramid,))
    if args.track_bilateral is not None:
        if not args.track:
            p.error("--track-bilateral needs --track")
        try:
            r, sigma_s, sigma_r = args.track_bilateral.split(",")
            args.track_bilateral = (int(r), float(sigma_s), float(sigma_r))
        except ValueError:
            p.error("--track-bilateral takes R,SIGMA_S,SIGMA_R (an integer and two numbers), got %r" % args.track_bilateral)
        if not (0 <= args.track_bilateral[0] <= 8 and 0.0 < args.track_bilateral[1] < math.inf and 0.0 < args.track_bilateral[2] < math.inf):
            p.error("--track-bilateral takes a radius in 0..8 and two finite sigmas > 0, got %r" % (args.track_bilateral,))
    if args.consistency is not None:
        if args.track:
            p.error("--consistency needs the pose of every frame (not with --track)")
        try:
            parts = args.consistency.split(",")
            if len(parts) not in (3, 4):
                raise ValueError
            args.consistency = (int(parts[0]), float(parts[1]), int(parts[2]), int(parts[3]) if len(parts) == 4 else 0)
        except ValueError:
            p.error("--consistency takes RADIUS,REL_TOL,MIN[,MAX_VIOL] (an integer, a number, one or two integers), got %r" % args.consistency)
        radius, rel_tol, min_c, max_v = args.consistency
        if not (1 <= radius <= 8 and math.isfinite(rel_tol) and rel_tol > 0.0 and 0 <= min_c <= 255 and 0 <= max_v <= 255):
            p.error("--consistency takes a radius in 1..8, a finite tolerance > 0 and vote thresholds in 0..255, got %r" % (args.consistency,))
    if args.track_color and not (args.track and args.color_dir is not None):
        p.error("--track-color needs --track and the colour images (--color-dir)")
    if args.track_color and args.track_pyramid is not None:
        p.error("--track-color runs at one level only (not with --track-pyramid)")
    if args.track and args.color_dir is not None and not args.track_color:
        p.error("--track takes depth maps only (not with --color-dir, unless --track-color)")
    if args.raycast_color and args.color_dir is None:
        p.error("--raycast-color needs the colour images (--color-dir)")
    for name in ("voxel_size", "trunc", "min_weight"):
        v = getattr(args, name)
        if not (math.isfinite(v) and v > 0.0):
            p.error("--%s must be finite and positive, got %r" % (name.replace("_", "-"), v))
    if args.margin is not None and not (math.isfinite(args.margin) and args.margin >= 0.0):
        p.error("--margin must be finite and >= 0, got %r" % args.margin)
    if (args.origin is None) != (args.dims is None):
        p.error("--origin and --dims go together")
    if args.dims is not None and (min(args.dims) < 1 or args.dims[0] * args.dims[1] * args.dims[2] >= 1 << 31):
        p.error("--dims must be >= 1 each with a product below 2^31, got %r" % (args.dims,))
    return args


def default_volume(w2c, voxel_size, margin):
    """(origin, dims): the bounding box of the camera centres -R^T t, padded by margin on every side."""
    import numpy as np
    R, t = w2c[:, :9].reshape(-1, 3, 3), w2c[:, 9:]
    centres = -np.einsum("fba,fb->fa", R, t)
    lo, hi = centres.min(axis=0) - margin, centres.max(axis=0) + margin
    dims = [max(1, int(math.ceil((hi[a] - lo[a]) / voxel_size))) for a in range(3)]
    return lo, dims


def raycast_depth(r3d, vol, quats, ts, shape, min_weight):
    """[F,H,W] float32: the depth the volume predicts at every pose -- the depth map alone (4 bytes per pixel on the device and
    over the bus, not the 28 of all three maps), one launch's worth of views at a time."""
    import numpy as np
    h, w = shape
    table = r3d.poses_w2c(quats, ts)
    cam = vol.ctx.camera(h, w, *_common.intrinsics())
    out = np.empty((len(table), h, w), np.float32)
    chunk = 32
    with vol.ctx.buffers() as B:
        buf = B.alloc(min(chunk, len(table)) * h * w * 4)
        for lo in range(0, len(table), chunk):
            n = min(chunk, len(table) - lo)
            vol.raycast_device(cam, n, table[lo:lo + n], buf.ptr, None, None, min_weight=min_weight)
            out[lo:lo + n] = buf.download_array(np.float32, (n, h, w))
    return out


def raycast_color(r3d, vol, quats, ts, shape, min_weight):
    """[F,H,W,3] uint8: the colour image the volume predicts at every pose -- that image alone (3 bytes per pixel), one launch's
    worth of views at a time."""
    import numpy as np
    h, w = shape
    table = r3d.poses_w2c(quats, ts)
    cam = vol.ctx.camera(h, w, *_common.intrinsics())
    out = np.empty((len(table), h, w, 3), np.uint8)
    chunk = 32
    with vol.ctx.buffers() as B:
        buf = B.alloc(min(chunk, len(table)) * h * w * 3)
        for lo in range(0, len(table), chunk):
            n = min(chunk, len(table) - lo)
            vol.raycast_device(cam, n, table[lo:lo + n], None, None, None, min_weight=min_weight, d_rgb=buf.ptr)
            out[lo:lo + n] = buf.download_array(np.uint8, (n, h, w, 3))
    return out


def quat_xyzw(R):
    """scalar-last unit quaternion of a rotation matrix (Shepperd's method: the largest of w, x, y, z first)"""
    import numpy as np
    t = np.trace(R)
    cand = [t, R[0, 0], R[1, 1], R[2, 2]]
    k = int(np.argmax(cand))
    if k == 0:
        w = math.sqrt(1.0 + t) / 2.0
        q = [(R[2, 1] - R[1, 2]) / (4 * w), (R[0, 2] - R[2, 0]) / (4 * w), (R[1, 0] - R[0, 1]) / (4 * w), w]
    else:
        a = k - 1
        b, c = (a + 1) % 3, (a + 2) % 3
        x = math.sqrt(1.0 + R[a, a] - R[b, b] - R[c, c]) / 2.0
        q = [0.0, 0.0, 0.0, (R[c, b] - R[b, c]) / (4 * x)]
        q[a], q[b], q[c] = x, (R[b, a] + R[a, b]) / (4 * x), (R[c, a] + R[a, c]) / (4 * x)
    return np.array(q)


def write_tracked(path, names, rows, scale):
    """the rows (world -> camera, R row-major then t) as a pose file read_pose_file parses; t is divided by the pose scale again"""
    header = "id,tx,ty,tz,qx,qy,qz,qw,name,tail"
    if os.path.isfile(POSE_FILE):
        with open(POSE_FILE, 'r') as f:
            header = f.readline().rstrip("\n") or header
    with open(path, 'w') as f:
        f.write(header + "\n")
        for k, (name, row) in enumerate(zip(names, rows)):
            q, t = quat_xyzw(row[:9].reshape(3, 3)), row[9:] / scale
            f.write(",".join([str(k + 1)] + [repr(float(v)) for v in t] + [repr(float(v)) for v in q] + [name, "tracked"]) + "\n")


def read_colors(r3d, color_dir, names, shape):
    """[F,H,W,3] uint8: DIR/<frame name> of every frame, at the depth maps' size; exits with a message otherwise."""
    paths = [os.path.join(color_dir, n) for n in names]
    for path in paths:
        if not os.path.isfile(path):
            sys.exit("integrate_tsdf.py: colour image %s not found (--color-dir needs one image per frame of the pose file)" % path)
    try:
        rgb = r3d.cloud_io.read_rgb_batch(paths)
    except (ValueError, r3d.R3DError) as e:
        sys.exit("integrate_tsdf.py: the colour images in %s cannot be read as one batch (they must all have the depth maps' size): %s"
                 % (color_dir, e))
    if rgb.shape[1:3] != tuple(shape):
        sys.exit("integrate_tsdf.py: the colour images are %d x %d, the depth maps %d x %d" % (rgb.shape[1:3] + tuple(shape)))
    return rgb


def main(argv=None):
    args = parse_args(sys.argv[1:] if argv is None else argv)
    r3d = _common.package()
    if not os.path.isfile(POSE_FILE) and not args.track:
        sys.exit("integrate_tsdf.py: %s not found (run from the data directory)" % POSE_FILE)
    names, quats, ts = r3d.read_pose_file(POSE_FILE) if os.path.isfile(POSE_FILE) else ([], None, None)
    if not names and args.track and os.path.isdir('./depth/'):
        import numpy as np
        names = sorted(n for n in os.listdir('./depth/') if os.path.isfile(os.path.join('./depth/', n)))
        quats, ts = np.tile([0.0, 0.0, 0.0, 1.0], (len(names), 1)), np.zeros((len(names), 3))   # row 0 is the identity; the rest unused
    if not names:
        sys.exit("integrate_tsdf.py: %s lists no frames" % POSE_FILE)
    ts = ts * _common.pose_scale()
    if args.origin is None:
        margin = 16.0 * args.trunc if args.margin is None else args.margin
        known = r3d.poses_w2c(quats, ts)
        origin, dims = default_volume(known[:1] if args.track else known, args.voxel_size, margin)
        if dims[0] * dims[1] * dims[2] >= 1 << 31:
            sys.exit("integrate_tsdf.py: the default volume has %d x %d x %d voxels; choose a larger --voxel-size or give --origin / --dims"
                     % tuple(dims))
    else:
        origin, dims = args.origin, args.dims
    depths = r3d.cloud_io.read_depth_batch([os.path.join('./depth/', n) for n in names])
    rgb = read_colors(r3d, args.color_dir, names, depths.shape[-2:]) if args.color_dir is not None else None
    _common.stamp("read %d frames" % len(names))
    if args.consistency is not None:
        radius, rel_tol, min_c, max_v = args.consistency
        keep, depths = r3d.depth_consistency(depths, quats, ts, intrinsics=_common.intrinsics(), radius=radius, rel_tol=rel_tol,
                                             min_consistent=min_c, max_violations=max_v, ctx=_common.context())[2:]
        print("consistency kept %d of %d pixels" % (int(keep.sum()), keep.size))
        _common.stamp("consistency")
    tracked = None
    if args.track:
        vol = r3d.TSDFVolume(origin, args.voxel_size, dims, args.trunc, ctx=_common.context(), color=args.track_color)
        try:
            tracked = vol.track_and_integrate(depths, r3d.poses_w2c(quats[:1], ts[:1])[0], intrinsics=_common.intrinsics(),
                                              min_weight=args.min_weight, pyramid_iters=args.track_pyramid,
                                              bilateral=args.track_bilateral, rgbs=rgb if args.track_color else None,
                                              **({"photo_weight": args.photo_weight, "max_jump": 0.05 if args.track_max_jump is None
                                                  else args.track_max_jump} if args.track_color else {}))
        except (RuntimeError, ValueError) as e:
            sys.exit("integrate_tsdf.py: --track: %s" % e)
        quats = [quat_xyzw(row[:9].reshape(3, 3)) for row in tracked]
        ts = tracked[:, 9:]
    elif rgb is None:
        vol = r3d.TSDFVolume(origin, args.voxel_size, dims, args.trunc, ctx=_common.context())
        vol.integrate(depths, quats, ts, intrinsics=_common.intrinsics())
    else:
        vol = r3d.TSDFVolume(origin, args.voxel_size, dims, args.trunc, ctx=_common.context(), color=True)
        vol.integrate(depths, quats, ts, intrinsics=_common.intrinsics(), rgb=rgb)
    _common.stamp("integrate")
    colors, mesh_stats = None, None
    clean = args.mesh and (args.mesh_min_component is not None or args.mesh_largest)
    smooth = args.mesh_smooth if args.mesh else None
    if rgb is None:
        xyz, normals = vol.extract_point_cloud(args.min_weight)
        mesh = vol.extract_triangle_mesh(args.min_weight, smooth=smooth) if args.mesh and not clean else None
    else:
        xyz, normals, colors = vol.extract_point_cloud(args.min_weight, with_colors=True)
        mesh = vol.extract_triangle_mesh(args.min_weight, smooth=smooth)[:3] + (colors,) if args.mesh and not clean else None   # the vertices are the points
    if clean:
        got = vol.extract_triangle_mesh(args.min_weight, with_colors=rgb is not None, min_component_triangles=args.mesh_min_component,
                                        keep_largest=args.mesh_largest, with_stats=True, smooth=smooth)
        mesh, mesh_stats = got[:-1], got[-1]
    cast = raycast_depth(r3d, vol, quats, ts, depths.shape[-2:], args.min_weight) if args.raycast else None
    cast_rgb = raycast_color(r3d, vol, quats, ts, depths.shape[-2:], args.min_weight) if args.raycast_color else None
    vol.close()
    _common.stamp("extract")
    os.makedirs(os.path.dirname(OUT_FILE), exist_ok=True)
    r3d.cloud_io.write_ply_normals(OUT_FILE, xyz, normals, rgb=colors)
    print("origin %.9g %.9g %.9g dims %d %d %d voxel %.9g trunc %.9g frames %d points %d -> %s"
          % (origin[0], origin[1], origin[2], dims[0], dims[1], dims[2], args.voxel_size, args.trunc, len(names), len(xyz), OUT_FILE))
    if mesh is not None:
        r3d.cloud_io.write_ply_mesh(MESH_FILE, *mesh)
        if mesh_stats is not None:
            print("components %d kept %d triangles kept %d dropped %d" % (mesh_stats["components"], mesh_stats["components_kept"],
                                                                          mesh_stats["triangles_kept"],
                                                                          mesh_stats["triangles"] - mesh_stats["triangles_kept"]))
        if smooth is not None:
            print("smoothed vertices %(vertices)d edges %(edges)d boundary %(boundary_vertices)d steps %(steps)d" % vol.last_smooth)
        print("triangles %d -> %s" % (len(mesh[2]), MESH_FILE))
    if cast is not None:
        import numpy as np
        os.makedirs(RAYCAST_DIR, exist_ok=True)
        for name, raster in zip(names, cast):
            np.save(os.path.join(RAYCAST_DIR, name + ".npy"), raster)
        print("raycast %d frames -> %s" % (len(names), RAYCAST_DIR))
    if cast_rgb is not None:
        import numpy as np
        os.makedirs(RAYCAST_COLOR_DIR, exist_ok=True)
        for name, image in zip(names, cast_rgb):
            np.save(os.path.join(RAYCAST_COLOR_DIR, name + ".npy"), image)
        print("raycast colour %d frames -> %s" % (len(names), RAYCAST_COLOR_DIR))
    if tracked is not None:
        os.makedirs(os.path.dirname(TRACKED_FILE), exist_ok=True)
        write_tracked(TRACKED_FILE, names, tracked, _common.pose_scale())
        print("tracked %d frames -> %s" % (len(names), TRACKED_FILE))


if __name__ == "__main__":
    main()
