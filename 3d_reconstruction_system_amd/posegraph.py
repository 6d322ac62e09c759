"""Multiway registration on the MI355X: the information matrix and quality of a registered pair, a pose graph with robust loop
closures and the recipe that puts N clouds into one frame -- what users of Open3D call get_information_matrix_from_point_clouds,
evaluate_registration, PoseGraph and global_optimization for, between "register pairs" and "integrate everything" (no parity with
Open3D is claimed).  Semantics: include/r3d.h (r3d_registration_sums, r3d_information_from_sums, r3d_posegraph_optimize) and
DESIGN.md section 4.5s.

Conventions: the pose X_i of node i maps cloud i into the frame of cloud 0; an edge (s, t, T) says p_t = T p_s, the T that
register_global and icp_point_to_plane(src=s, tgt=t) return.  The pair sums run on the GPU; the information matrix and the
pose-graph solver are host fp64 code of the library and need none.
"""
import ctypes as C
import math

import numpy as np

from . import _lib as L
from ._args import positive as _check_positive
from .device import default_context
from .icp import NNIndex
from .outliers import _cloud

SUMS = 11             # R3D_REGISTRATION_SUMS
MAX_NODES = 512       # R3D_POSEGRAPH_MAX_NODES
REPORT_DOUBLES = 8    # R3D_POSEGRAPH_REPORT_DOUBLES


# ---- pair sums, information matrix, quality ---------------------------------------------------------------------------------

def registration_sums_device(ctx, d_src, n_src, d_tgt, n_tgt, d_idx, d_d2, max_dist):
    """The 11 pair sums (r3d_registration_sums) of a source cloud ALREADY moved by the pose under test: d_src [n_src][3] float32,
    d_idx / d_d2 what NNIndex.query wrote for it against d_tgt [n_tgt][3] float32; pairs farther apart than max_dist stay out.
    Returns a float64 array.  Synchronous."""
    max_dist = _check_positive(max_dist, "max_dist")
    sums = np.zeros(SUMS, np.float64)
    L.check(ctx.lib.r3d_registration_sums(ctx.handle, d_src, int(n_src), d_tgt, int(n_tgt), d_idx, d_d2, max_dist * max_dist,
                                          sums.ctypes.data))
    return sums


def information_from_sums(sums, n_src):
    """(info [6,6] float64, fitness, rmse) of the 11 pair sums (r3d_information_from_sums; host arithmetic, no GPU)."""
    sums = np.ascontiguousarray(sums, dtype=np.float64).reshape(-1)
    if sums.shape[0] != SUMS:
        raise ValueError("need %d sums, got %d" % (SUMS, sums.shape[0]))
    info, fit, rmse = np.zeros((6, 6), np.float64), C.c_double(), C.c_double()
    L.check(L.load().r3d_information_from_sums(sums.ctypes.data, int(n_src), info.ctypes.data, C.byref(fit), C.byref(rmse)))
    return info, fit.value, rmse.value


def _rigid(T, what):
    T = np.array(T, dtype=np.float64)
    if T.shape != (4, 4) or not np.isfinite(T).all():
        raise ValueError("%s must be a finite 4x4 matrix" % what)
    if T[3].tolist() != [0.0, 0.0, 0.0, 1.0]:
        raise ValueError("the bottom row of %s must be 0 0 0 1" % what)
    return np.ascontiguousarray(T)


def _pair_sums(src, tgt, T, max_dist, ctx):
    """(sums, n_src): T applied to src on the device, the nearest neighbours through an NNIndex over tgt (or tgt itself when it
    is one) and the pair sums."""
    src, T, max_dist = _cloud(src), _rigid(T, "T"), _check_positive(max_dist, "max_dist")
    n = src.shape[0]
    index = tgt if isinstance(tgt, NNIndex) else None
    if index is None:
        tgt = _cloud(tgt)
        if tgt.shape[0] < 1:
            raise ValueError("the target cloud is empty")
    if n == 0:
        return np.zeros(SUMS, np.float64), 0
    ctx = index.ctx if index is not None else (ctx or default_context())
    with ctx.buffers() as B:
        if index is None:
            index = B.adopt(NNIndex(ctx, B.upload(tgt).ptr, tgt.shape[0]))
        d_src, d_idx, d_d2 = B.upload(src), B.alloc(n * 4), B.alloc(n * 4)
        L.check(ctx.lib.r3d_apply_T(ctx.handle, d_src.ptr, L.F32, n, T.ctypes.data, d_src.ptr, L.F32))
        index.query(d_src.ptr, n, d_idx.ptr, d_d2.ptr)
        return registration_sums_device(ctx, d_src.ptr, n, index.d_tgt, index.n, d_idx.ptr, d_d2.ptr, max_dist), n


def evaluate_registration(src, tgt, T, max_dist, ctx=None):
    """(fitness, rmse, n_pairs) of the pose T (tgt ~ T src): the share of the source points that have a target point within
    max_dist once moved, the rms of those distances and their number.  tgt: an [M,3] cloud, or a ready icp.NNIndex over one (its
    context is used; many sources against one target build the index once)."""
    sums, n = _pair_sums(src, tgt, T, max_dist, ctx)
    _, fitness, rmse = information_from_sums(sums, n)
    return fitness, rmse, int(sums[0])


def registration_information(src, tgt, T, max_dist, ctx=None):
    """(info [6,6] float64, fitness, rmse): the information matrix, in the order (rotation, translation), of the pose T
    (tgt ~ T src) over the pairs within max_dist -- how firmly the overlap holds each of the six freedoms, the weight of this
    pair's edge in a PoseGraph.  info[5,5] is the pair count.  tgt as in evaluate_registration."""
    sums, n = _pair_sums(src, tgt, T, max_dist, ctx)
    return information_from_sums(sums, n)


# ---- pose graph -------------------------------------------------------------------------------------------------------------

class PoseGraph:
    """Node poses [N,4,4] (X_i maps cloud i into the frame of cloud 0; node 0 is fixed) and edges (s, t, T, info, uncertain) with
    p_t = T p_s.  optimize() moves the poses to the least-squares compromise of the edges; uncertain edges (loop closures that may
    be wrong) are weighted down by how badly they fit, and pruned when their weight ends below the threshold."""

    def __init__(self, poses):
        poses = np.array(poses, dtype=np.float64)
        if poses.ndim != 3 or poses.shape[1:] != (4, 4) or not 1 <= poses.shape[0] <= MAX_NODES:
            raise ValueError("poses must be [N,4,4] with 1 <= N <= %d, got %r" % (MAX_NODES, poses.shape))
        self.poses = np.stack([_rigid(X, "pose %d" % i) for i, X in enumerate(poses)])
        self.edges = []
        self.edge_weights = np.zeros(0, np.float64)
        self.pruned = np.zeros(0, bool)

    def add_edge(self, s, t, T, info, uncertain=False):
        """p_t = T p_s with the information matrix info [6,6] (registration_information); uncertain: a loop closure."""
        n = self.poses.shape[0]
        for v in (s, t):
            if isinstance(v, bool) or not isinstance(v, (int, np.integer)) or not 0 <= int(v) < n:
                raise ValueError("an edge joins two of the nodes 0..%d, got %r" % (n - 1, v))
        if int(s) == int(t):
            raise ValueError("an edge joins two different nodes, got %d twice" % s)
        if not isinstance(uncertain, (bool, np.bool_)):
            raise ValueError("uncertain must be True or False, got %r" % (uncertain,))
        T = _rigid(T, "T")
        info = np.array(info, dtype=np.float64)
        if info.shape != (6, 6) or not np.isfinite(info).all():
            raise ValueError("info must be a finite 6x6 matrix")
        if np.abs(info - info.T).max() > 1e-9 * np.abs(info).max():
            raise ValueError("info must be symmetric")
        if (np.diag(info) < 0).any():
            raise ValueError("info has a negative diagonal entry")
        self.edges.append((int(s), int(t), T, np.ascontiguousarray(info), bool(uncertain)))

    def _connected(self):
        n = self.poses.shape[0]
        seen, todo = {0}, [0]
        while todo:
            a = todo.pop()
            for s, t, _, _, _ in self.edges:
                b = t if s == a else s if t == a else None
                if b is not None and b not in seen:
                    seen.add(b)
                    todo.append(b)
        return sorted(set(range(n)) - seen)

    def optimize(self, max_correspondence_distance, preference_loop_closure=1.0, prune_threshold=0.25, max_iters=100):
        """Levenberg-Marquardt over the poses of nodes 1..N-1 (r3d_posegraph_optimize; host fp64, no GPU).  self.poses,
        self.edge_weights ([M] float64, 0 for pruned edges) and self.pruned ([M] bool) are updated; returns the report:
        initial_cost, final_cost, iterations, pruned, max_iters_reached.  preference_loop_closure=inf: no robust weights."""
        dist = _check_positive(max_correspondence_distance, "max_correspondence_distance")
        try:
            pref, thr = float(preference_loop_closure), float(prune_threshold)
        except (TypeError, ValueError):
            raise ValueError("preference_loop_closure and prune_threshold must be numbers")
        if not pref > 0.0:
            raise ValueError("preference_loop_closure must be > 0 (inf: no robust weights), got %r" % (preference_loop_closure,))
        if not math.isfinite(thr):
            raise ValueError("prune_threshold must be finite, got %r" % (prune_threshold,))
        if isinstance(max_iters, bool) or not isinstance(max_iters, (int, np.integer)) or int(max_iters) < 0:
            raise ValueError("max_iters must be an integer >= 0, got %r" % (max_iters,))
        self.poses = np.stack([_rigid(X, "pose %d" % i) for i, X in enumerate(self.poses)])
        loose = self._connected()
        if loose:
            raise ValueError("no path of edges connects node %d to node 0" % loose[0])
        n, m = self.poses.shape[0], len(self.edges)
        nodes = np.ascontiguousarray([(s, t) for s, t, _, _, _ in self.edges], dtype=np.int32).reshape(m, 2)
        Ts = np.ascontiguousarray([e[2] for e in self.edges], dtype=np.float64).reshape(m, 16)
        infos = np.ascontiguousarray([e[3] for e in self.edges], dtype=np.float64).reshape(m, 36)
        unc = np.ascontiguousarray([e[4] for e in self.edges], dtype=np.uint8).reshape(m)
        poses = np.ascontiguousarray(self.poses, dtype=np.float64).copy()
        w, rep = np.zeros(max(m, 1), np.float64), np.zeros(REPORT_DOUBLES, np.float64)
        L.check(L.load().r3d_posegraph_optimize(n, poses.ctypes.data, m, nodes.ctypes.data if m else None, Ts.ctypes.data if m else None,
                                                infos.ctypes.data if m else None, unc.ctypes.data if m else None, dist, pref, thr,
                                                int(max_iters), w.ctypes.data, rep.ctypes.data))
        self.poses, self.edge_weights = poses, w[:m].copy()
        self.pruned = (unc != 0) & (self.edge_weights == 0.0) if int(rep[3]) else np.zeros(m, bool)
        return {"initial_cost": float(rep[0]), "final_cost": float(rep[1]), "iterations": int(rep[2]), "pruned": int(rep[3]),
                "max_iters_reached": bool(rep[4])}


# ---- the recipe ----------------------------------------------------------------------------------------------------------------

def _loop_pairs(loop_pairs, n):
    if loop_pairs is None:
        return []
    if isinstance(loop_pairs, str):
        if loop_pairs != "all":
            raise ValueError("loop_pairs must be 'all', None or a list of (s, t) pairs, got %r" % (loop_pairs,))
        return [(s, t) for t in range(n) for s in range(t + 2, n)]
    out = []
    for pair in loop_pairs:
        try:
            s, t = pair
        except (TypeError, ValueError):
            raise ValueError("loop_pairs holds (s, t) pairs, got %r" % (pair,))
        for v in (s, t):
            if isinstance(v, bool) or not isinstance(v, (int, np.integer)) or not 0 <= int(v) < n:
                raise ValueError("a loop pair joins two of the clouds 0..%d, got %r" % (n - 1, pair))
        if int(s) == int(t):
            raise ValueError("a loop pair joins two different clouds, got %r" % (pair,))
        out.append((int(s), int(t)))
    return out


def register_multiway(clouds, voxel_size, loop_pairs="all", min_fitness=0.3, viewpoints=None, seed=0, ctx=None):
    """(poses [N,4,4], graph, info): poses[i] maps cloud i into the frame of cloud 0.
    Every cloud is voxel-downsampled to voxel_size and gets normals once (32 neighbours within 5 x voxel_size, turned towards
    viewpoints[i] when given: [N,3], where each cloud was seen from in its own frame).  Consecutive clouds (i + 1 -> i) become
    certain edges: icp.icp_point_to_plane from the identity with max_dist = 15 x voxel_size, then again with 1.5 x voxel_size.
    loop_pairs ('all': every (s, t) with s >= t + 2; None; or a list of (s, t)) are candidates for uncertain edges:
    register_global(refine=True) on the downsampled clouds, kept when the fitness at 1.5 x voxel_size is at least min_fitness.  The
    information matrix of every edge is registration_information at 1.5 x voxel_size.  The node poses start as the chained odometry
    and are optimised with max_correspondence_distance = 1.5 x voxel_size.
    info: "down" (the downsampled clouds), "odometry" ([N,4,4], the chained poses), "edges" ((s, t, uncertain, fitness, rmse) per
    edge), "rejected" ((s, t, reason) per candidate that raised or fell below min_fitness), "report" (PoseGraph.optimize).
    The chain must hold: a consecutive pair that cannot be registered -- its point-to-plane step is undefined because the overlap
    is one plane, parallel walls or nothing -- raises ValueError naming the pair and the stage."""
    from . import voxelmap
    from .icp import icp_point_to_plane
    from .normals import estimate_normals
    from .registration import _check_seed, _viewpoint, register_global
    clouds = [_cloud(c) for c in clouds]
    n = len(clouds)
    if not 1 <= n <= MAX_NODES:
        raise ValueError("need 1 <= N <= %d clouds, got %d" % (MAX_NODES, n))
    vs, seed = _check_positive(voxel_size, "voxel_size"), _check_seed(seed)
    try:
        min_fitness = float(min_fitness)
    except (TypeError, ValueError):
        raise ValueError("min_fitness must be a number, got %r" % (min_fitness,))
    if not 0.0 <= min_fitness <= 1.0:
        raise ValueError("min_fitness must be in [0, 1], got %r" % (min_fitness,))
    if viewpoints is None:
        views = [None] * n
    else:
        if len(viewpoints) != n:
            raise ValueError("viewpoints must have one row per cloud")
        views = [_viewpoint(v, "a viewpoint") for v in viewpoints]
    candidates = _loop_pairs(loop_pairs, n)
    ctx = ctx or default_context()
    fine, coarse = 1.5 * vs, 15.0 * vs
    down, nrm = [], []
    for cloud, view in zip(clouds, views):
        d = np.ascontiguousarray(voxelmap.voxel_down_sample(cloud, vs, ctx=ctx).xyz, dtype=np.float32)
        if d.shape[0] < 3:
            raise ValueError("a cloud has fewer than 3 occupied voxels at voxel_size %g" % vs)
        down.append(d)
        nrm.append(estimate_normals(d, 32, radius=5.0 * vs, viewpoint=view, ctx=ctx).normals)
    odometry = np.tile(np.eye(4), (n, 1, 1))
    found = []                                            # (s, t, T, uncertain)
    for i in range(n - 1):
        T = None
        for stage, gate in (("coarse", coarse), ("fine", fine)):
            try:
                T, _ = icp_point_to_plane(down[i + 1], down[i], tgt_normals=nrm[i], init=T, max_dist=gate, ctx=ctx)
            except ValueError as e:
                raise ValueError("clouds %d and %d cannot be registered (%s stage, max_dist %g): %s" % (i + 1, i, stage, gate, e))
        odometry[i + 1] = odometry[i] @ T
        found.append((i + 1, i, T, False))
    rejected = []
    for s, t in candidates:
        try:
            T, _ = register_global(down[s], down[t], vs, seed=seed, refine=True, src_viewpoint=views[s], tgt_viewpoint=views[t], ctx=ctx)
            fitness, _, _ = evaluate_registration(down[s], down[t], T, fine, ctx=ctx)
        except (ValueError, L.R3DError) as e:
            rejected.append((s, t, str(e)))
            continue
        if fitness < min_fitness:
            rejected.append((s, t, "fitness %.3f below %.3f" % (fitness, min_fitness)))
            continue
        found.append((s, t, T, True))
    graph, edges = PoseGraph(odometry), []
    for s, t, T, uncertain in found:
        lam, fitness, rmse = registration_information(down[s], down[t], T, fine, ctx=ctx)
        graph.add_edge(s, t, T, lam, uncertain)
        edges.append((s, t, uncertain, fitness, rmse))
    report = graph.optimize(max_correspondence_distance=fine)
    return graph.poses.copy(), graph, {"down": down, "odometry": odometry, "edges": edges, "rejected": rejected, "report": report}
