"""ctypes binding of include/posegraph/vcr_hip_posegraph.h and the Python API on top of it: multiway
registration after Open3D's global_optimization -- a pose graph optimised by Levenberg-Marquardt with the line process over its
uncertain edges and the pruning pass, the whole loop of a graph in one launch (vcr_posegraph_optimize_f64) --, the graph of K
clouds built from batched pairwise refinements (pose_graph_from_clouds) and the two together (register_multiway).

Like ``robust``, the header extends include/vcr_hip.h without touching it and this module keeps its own STRUCTS / SIGNATURES
maps, applied once to ``native.lib()`` on first use.  No CPU fallback, as everywhere."""
from __future__ import annotations

import ctypes as C
import math
import torch

from . import extension, native
from .native import VcrHipError, ptr
from .score import f64p

i32p = C.c_void_p
MAX_NODES, MAX_EDGES, MAX_TRIALS = 128, 65536, 4096
FORM_LDS, FORM_GLOBAL = 1, 2
# Open3D's GlobalOptimizationConvergenceCriteria, by its names
CRITERIA = {"max_iteration": 100, "max_iteration_lm": 20, "min_relative_increment": 1e-6, "min_relative_residual_increment": 1e-6,
            "min_right_term": 1e-6, "min_residual": 1e-6, "lower_scale_factor": 1.0 / 3.0, "upper_scale_factor": 2.0 / 3.0}


class PosegraphArgs(native._Sized):
    _fields_ = [("struct_bytes", C.c_uint32), ("G", C.c_int), ("K", C.c_int), ("E", C.c_int), ("R", f64p), ("t", f64p),
                ("src", i32p), ("dst", i32p), ("R_edge", f64p), ("t_edge", f64p), ("information", f64p), ("uncertain", i32p),
                ("anchor", C.c_int), ("prune", C.c_int), ("max_correspondence_distance", C.c_double),
                ("edge_prune_threshold", C.c_double), ("max_iteration", C.c_int), ("max_iteration_lm", C.c_int),
                ("min_relative_increment", C.c_double), ("min_relative_residual_increment", C.c_double),
                ("min_right_term", C.c_double), ("min_residual", C.c_double), ("lower_scale_factor", C.c_double),
                ("upper_scale_factor", C.c_double), ("variant", C.c_int), ("R_out", f64p), ("t_out", f64p), ("weight", f64p),
                ("kept", i32p), ("residual", f64p), ("iterations", i32p), ("converged", i32p), ("trials", i32p), ("H", f64p),
                ("b", f64p), ("residual0", f64p), ("l0", f64p), ("delta0", f64p), ("lambda0", f64p)]


STRUCTS = {"vcr_posegraph_args": PosegraphArgs}

_A = C.POINTER(PosegraphArgs)
_intp = C.POINTER(C.c_int)
# name -> (restype, [argtypes]): the prototypes of include/posegraph/vcr_hip_posegraph.h (tests/test_posegraph_cpu.py holds them to it)
SIGNATURES = {"vcr_posegraph_optimize_workspace_bytes": (C.c_size_t, [_A, C.c_int]),
              "vcr_posegraph_optimize_f64": (C.c_int, [_A, C.c_void_p, C.c_size_t, C.c_void_p]),
              "vcr_posegraph_optimize_form": (C.c_int, [_A, C.c_int, _intp, _intp]),
              "vcr_posegraph_check_edges": (C.c_int, [_intp, _intp, C.c_int, C.c_int, C.c_int])}

lib = extension.typed_lib(SIGNATURES)                      # native.lib() with this module's entry points typed (once)

_API = "optimize_pose_graph"


def form_args(G, K, E, variant=0, **kw):
    """Args with every mandatory pointer set to a placeholder (never dereferenced on the host) and the default criteria."""
    a = PosegraphArgs(G=G, K=K, E=E, R=0x1000, t=0x2000, src=0x3000, dst=0x4000, R_edge=0x5000, t_edge=0x6000, information=0x7000,
                      uncertain=0x8000, anchor=0, prune=1, max_correspondence_distance=0.05, edge_prune_threshold=0.25,
                      variant=variant, R_out=0x9000, t_out=0xa000, weight=0xb000, kept=0xc000, residual=0xd000, iterations=0xe000,
                      converged=0xf000, **CRITERIA)
    for k, v in kw.items():
        setattr(a, k, v)
    return a


def posegraph_form(K, G=1, E=0, variant=0):
    """vcr_posegraph_optimize_form and _workspace_bytes (host only): (FORM_LDS or FORM_GLOBAL, bytes of LDS a workgroup asks for,
    workspace bytes)."""
    L = lib()
    a = form_args(G, K, E, variant)
    f, n = C.c_int(0), C.c_int(0)
    native.check(L.vcr_posegraph_optimize_form(C.byref(a), 0, C.byref(f), C.byref(n)), "vcr_posegraph_optimize_form")
    return f.value, n.value, L.vcr_posegraph_optimize_workspace_bytes(C.byref(a), 0)


def check_criteria(criteria, api=_API):
    """-> CRITERIA with the caller's entries over it, checked: the rules of vcr_posegraph_args."""
    c = dict(CRITERIA)
    if criteria is not None:
        if not isinstance(criteria, dict) or set(criteria) - set(CRITERIA):
            raise VcrHipError(f"{api}: criteria must be a dict with keys among {sorted(CRITERIA)}, got {criteria!r}")
        c.update(criteria)
    for k in ("max_iteration", "max_iteration_lm"):
        if int(c[k]) != c[k] or not 0 <= c[k] <= MAX_TRIALS:
            raise VcrHipError(f"{api}: {k} must be an integer in [0, {MAX_TRIALS}], got {c[k]!r}")
        c[k] = int(c[k])
    if c["max_iteration"] * c["max_iteration_lm"] > MAX_TRIALS:
        raise VcrHipError(f"{api}: max_iteration * max_iteration_lm must not exceed {MAX_TRIALS} (the launch stays bounded), got "
                          f"{c['max_iteration']} * {c['max_iteration_lm']}")
    for k in ("min_relative_increment", "min_relative_residual_increment", "min_right_term", "min_residual"):
        c[k] = float(c[k])
        if not c[k] >= 0.0:
            raise VcrHipError(f"{api}: {k} must be >= 0, got {c[k]}")
    for k in ("lower_scale_factor", "upper_scale_factor"):
        c[k] = float(c[k])
        if not (math.isfinite(c[k]) and c[k] > 0.0):
            raise VcrHipError(f"{api}: {k} must be finite and > 0, got {c[k]}")
    return c


def _nonneg(api, name, v):
    if v is None:
        raise VcrHipError(f"{api}: {name} has no default -- it is the distance within which your pairwise registrations matched "
                          "points, in the clouds' unit")
    try:
        v = float(v)
    except (TypeError, ValueError):
        v = float("nan")
    if not (math.isfinite(v) and v >= 0.0):
        raise VcrHipError(f"{api}: {name} must be finite and >= 0, got {v}")
    return v


def check_edges(src, dst, K, api=_API):
    """HOST edge lists (int tensors or sequences, [E] or [G,E]) -> (src, dst) as contiguous int32 CPU tensors, refused
    (vcr_posegraph_check_edges) where an edge names a node >= K or itself; src < 0 is a blank."""
    s = torch.as_tensor(src, dtype=torch.int32).contiguous()
    d = torch.as_tensor(dst, dtype=torch.int32).contiguous()
    if s.shape != d.shape or s.dim() not in (1, 2):
        raise VcrHipError(f"{api}: src and dst must both be [E] or [G, E], got {tuple(s.shape)} and {tuple(d.shape)}")
    G, E = (1, s.shape[0]) if s.dim() == 1 else s.shape
    if E and lib().vcr_posegraph_check_edges(C.cast(s.data_ptr(), _intp), C.cast(d.data_ptr(), _intp), max(G, 1), K, E) != 0:
        bad = ((s >= 0) & ((s >= K) | (d < 0) | (d >= K) | (s == d))).nonzero()[0].tolist()
        raise VcrHipError(f"{api}: edge {bad} names a node outside [0, {K}) or joins a node to itself "
                          f"(src {int(s[tuple(bad)])}, dst {int(d[tuple(bad)])}); src < 0 marks a blank")
    return s, d


def _take(api, name, x, shape, dtype, dev):
    """x as a contiguous `shape` tensor of dtype: it has that shape, or, for one graph, the shape without the leading 1."""
    if not torch.is_tensor(x) or not (tuple(x.shape) == shape or (shape[0] == 1 and tuple(x.shape) == shape[1:])):
        raise VcrHipError(f"{api}: {name} must be {list(shape[1:])} for one graph or {list(shape)} for a batch, got "
                          f"{tuple(x.shape) if torch.is_tensor(x) else type(x).__name__}")
    if x.device != dev:
        raise VcrHipError(f"{api}: {name} must live on the device of the poses (there is no CPU fallback)")
    return x.reshape(shape).to(dtype).contiguous()


@native._guarded
def optimize(R, t, src, dst, R_edge, t_edge, information, uncertain, max_correspondence_distance=None, anchor=0, prune=True,
             edge_prune_threshold=0.25, criteria=None, variant=0, want_system=False, guard=0, prefill=None):
    """vcr_posegraph_optimize_f64 on device tensors -> the header's outputs as a dict.  want_system: also "H", "b", "residual0",
    "l0", "delta0", "lambda0" and "trials".  guard / prefill (tests): as refine.refine's; the workspace is prefilled too."""
    if not torch.is_tensor(R) or R.dim() not in (3, 4) or tuple(R.shape[-2:]) != (3, 3):
        raise VcrHipError(f"{_API}: R must be [K, 3, 3] or [G, K, 3, 3], got {tuple(R.shape) if torch.is_tensor(R) else type(R).__name__}")
    batched = R.dim() == 4
    G, K = (R.shape[0], R.shape[1]) if batched else (1, R.shape[0])
    if G < 1 or K < 1:
        raise VcrHipError(f"{_API}: a graph needs at least one node, got R {tuple(R.shape)}")
    if K > MAX_NODES:
        raise VcrHipError(f"{_API}: at most {MAX_NODES} nodes a graph (a dense solve; sparse solves are not built), got {K}")
    mcd = _nonneg(_API, "max_correspondence_distance", max_correspondence_distance)
    thr = _nonneg(_API, "edge_prune_threshold", edge_prune_threshold)
    c = check_criteria(criteria)
    anchor = int(anchor)
    if not 0 <= anchor < K:
        raise VcrHipError(f"{_API}: anchor must be a node in [0, {K}), got {anchor}")
    if int(variant) not in (0, FORM_LDS, FORM_GLOBAL):
        raise VcrHipError(f"{_API}: variant must be 0, {FORM_LDS} (LDS) or {FORM_GLOBAL} (global memory), got {variant}")
    if not R.is_cuda:
        raise VcrHipError(f"{_API} runs on the MI355X HIP path only; move the graph to cuda (there is no CPU fallback by design)")
    dev = R.device
    if not (torch.is_tensor(src) and src.is_cuda and torch.is_tensor(dst) and dst.is_cuda):
        src, dst = check_edges(src, dst, K)                 # host lists: refused here; device tensors: blanks on the device
        src, dst = src.to(dev, non_blocking=True), dst.to(dev, non_blocking=True)
    if src.dim() not in (1, 2):
        raise VcrHipError(f"{_API}: src must be [E] or [G, E], got {tuple(src.shape)}")
    E = src.shape[-1]
    if E > MAX_EDGES or G * max(E, 1) >= 1 << 31:
        raise VcrHipError(f"{_API}: at most {MAX_EDGES} edge slots a graph and G * E < 2^31, got G = {G}, E = {E}")
    R = _take(_API, "R", R, (G, K, 3, 3), torch.float64, dev)
    t = _take(_API, "t", t, (G, K, 3), torch.float64, dev)
    src = _take(_API, "src", src, (G, E), torch.int32, dev)
    dst = _take(_API, "dst", dst, (G, E), torch.int32, dev)
    R_edge = _take(_API, "R_edge", R_edge, (G, E, 3, 3), torch.float64, dev)
    t_edge = _take(_API, "t_edge", t_edge, (G, E, 3), torch.float64, dev)
    information = _take(_API, "information", information, (G, E, 6, 6), torch.float64, dev)
    uncertain = _take(_API, "uncertain", uncertain, (G, E), torch.int32, dev)
    out, raw = extension.outputs(dev, guard, prefill)
    o = {"R": out("R", G * K * 9, torch.float64).view(G, K, 3, 3), "t": out("t", G * K * 3, torch.float64).view(G, K, 3),
         "weight": out("weight", G * E, torch.float64).view(G, E), "kept": out("kept", G * E, torch.int32).view(G, E),
         "residual": out("residual", G * 2, torch.float64).view(G, 2), "iterations": out("iterations", G * 2, torch.int32).view(G, 2),
         "converged": out("converged", G, torch.int32)}
    if want_system:
        o.update({"trials": out("trials", G * 2, torch.int32).view(G, 2),
                  "H": out("H", G * 36 * K * K, torch.float64).view(G, 6 * K, 6 * K), "b": out("b", G * 6 * K, torch.float64).view(G, 6 * K),
                  "residual0": out("residual0", G, torch.float64), "l0": out("l0", G * E, torch.float64).view(G, E),
                  "delta0": out("delta0", G * 6 * K, torch.float64).view(G, 6 * K), "lambda0": out("lambda0", G, torch.float64)})
    a = PosegraphArgs(G, K, E, ptr(R), ptr(t), ptr(src), ptr(dst), ptr(R_edge), ptr(t_edge), ptr(information), ptr(uncertain),
                      anchor, 1 if prune else 0, mcd, thr, c["max_iteration"], c["max_iteration_lm"], c["min_relative_increment"],
                      c["min_relative_residual_increment"], c["min_right_term"], c["min_residual"], c["lower_scale_factor"],
                      c["upper_scale_factor"], int(variant), ptr(o["R"]), ptr(o["t"]), ptr(o["weight"]), ptr(o["kept"]),
                      ptr(o["residual"]), ptr(o["iterations"]), ptr(o["converged"]), ptr(o.get("trials")), ptr(o.get("H")),
                      ptr(o.get("b")), ptr(o.get("residual0")), ptr(o.get("l0")), ptr(o.get("delta0")), ptr(o.get("lambda0")))
    L = lib()
    need = L.vcr_posegraph_optimize_workspace_bytes(C.byref(a), 0)
    if need == 0:                                            # refused: let the entry point say why
        native.check(L.vcr_posegraph_optimize_f64(C.byref(a), None, 0, native.stream_ptr()), "vcr_posegraph_optimize_f64")
        raise VcrHipError("vcr_posegraph_optimize_workspace_bytes: 0 for arguments vcr_posegraph_optimize_f64 accepts")
    ws = torch.empty(need + 256, dtype=torch.uint8, device=dev)
    if prefill is not None:
        ws.fill_(prefill)
    at = ws.data_ptr() + (-ws.data_ptr()) % 256
    native.check(L.vcr_posegraph_optimize_f64(C.byref(a), at, need, native.stream_ptr()), "vcr_posegraph_optimize_f64")
    if not batched:
        o = {k: v[0] for k, v in o.items()}
    if guard or prefill is not None:
        o["_raw"] = raw
    return o


def optimize_pose_graph(R, t, src, dst, R_edge, t_edge, information, uncertain, max_correspondence_distance=None, anchor=0,
                        prune=True, edge_prune_threshold=0.25, criteria=None):
    """Put the K nodes of a pose graph into one frame so that its pairwise poses agree with each other, and drop the pairwise
    poses that are wrong -- multiway registration after Open3D's global_optimization (GlobalOptimizationLevenbergMarquardt,
    the line process over uncertain edges, the pruning pass; not bit for bit Open3D's: DESIGN.md section 4.32 is the
    definition).  Device tensors, [K,...] for one graph or [G,K,...] for a batch of G (fp32 poses are widened):
      R, t                  [K,3,3], [K,3]     the initial poses, node frame -> world
      src, dst              int [E]            an edge's nodes; src < 0 marks a blank slot (how a batch pads).  Given as HOST
                                               tensors or lists they are checked here (a node >= K, src == dst: VcrHipError);
                                               given as device tensors such an edge is a blank -- nothing waits for the device
      R_edge, t_edge        [E,3,3], [E,3]     X_e: the SOURCE node's frame -> the TARGET node's (``refine_registration``'s R, t
                                               for the pair (source cloud, target cloud))
      information           [E,6,6]            ``information_matrix``'s, rotation first
      uncertain             [E]                non-zero: a loop closure the line process may switch off; 0: odometry
    max_correspondence_distance: the cap your pairwise registrations matched within (no default); it scales the line process:
    an uncertain edge whose residual r^T info r reaches mu = cap^2 * mean(info[5][5]) weighs a quarter.
    anchor: the node that does not move.  prune: after a first pass, drop every uncertain edge whose weight fell below
    edge_prune_threshold and optimise again.  criteria: a dict over ``posegraph.CRITERIA`` (Open3D's names and defaults;
    upper_scale_factor is taken and not used).
    Returns a dict: R, t float64 the optimised poses; weight float64 [E] the last line-process weight (NaN on a blank); kept
    int32 [E] 1 on an edge that survived; residual float64 [2] at the start and at the end; iterations int32 [2] outer
    iterations of each pass; converged int32.  One launch a call, no host synchronisation.
    Where it is weak: a dense solve -- at most 128 nodes a graph, and one workgroup a graph, so a single large graph uses one
    compute unit of 256 (SLAM-sized graphs want a sparse solver, not built).  The line process can only drop an edge that
    disagrees with the rest: two wrong closures that agree with each other survive, and with few or weak odometry edges a
    wrong closure can win.  A singular system (a node no certain path reaches once closures are dropped is still held by
    lambda, but an information matrix of zeros or NaN is not) stops the graph with the poses it has, converged = 0."""
    return optimize(R, t, src, dst, R_edge, t_edge, information, uncertain, max_correspondence_distance, anchor, prune,
                    edge_prune_threshold, criteria)


def all_pairs(K):
    return [(i, j) for i in range(K) for j in range(i + 1, K)]


def chain_poses(R_edge, t_edge, odometry):
    """The initial poses from the odometry edges, on the device in fp64: T_0 = I, T_{i+1} = T_i X_{i,i+1}^-1, where
    odometry[i] is the edge slot of (i, i+1).  -> R [K,3,3], t [K,3] float64."""
    Re, te = R_edge.double(), t_edge.double()
    Rs, ts = [torch.eye(3, dtype=torch.float64, device=Re.device)], [torch.zeros(3, dtype=torch.float64, device=Re.device)]
    for e in odometry:
        Rinv = Re[e].T
        Rs.append(Rs[-1] @ Rinv)
        ts.append(ts[-1] - Rs[-1] @ te[e])                   # T X^-1 = (R R_e^T, t - R R_e^T t_e)
    return torch.stack(Rs), torch.stack(ts)


def pose_graph_from_clouds(clouds, max_dist_coarse, max_dist_fine, method="point_to_plane", pairs=None, search="scan",
                           max_iterations=30, normal_k=20, cell=None):
    """The pose graph of K overlapping clouds [K,3,N] (device; clouds in neighbouring order overlap), in the shape of Open3D's
    multiway-registration tutorial: every pair i < j (or the given ``pairs``, a host list of (i, j) with i < j that holds every
    (i, i+1)) is gathered into ONE batch of P pairs, source i, target j; one ``refine_registration`` call at max_dist_coarse
    starts from the identity, one at max_dist_fine from its result, one ``information_matrix`` call at max_dist_fine follows.
    Edges (i, i+1) are certain (odometry), all others uncertain; the initial poses chain the odometry, T_0 = I,
    T_{i+1} = T_i X_{i,i+1}^-1, on the device.  method, search, cell, max_iterations, normal_k: ``refine_registration``'s.
    Returns a dict: R, t float64 the initial poses; src, dst int32 [P] (device) and "pairs" (the host list); R_edge, t_edge
    float32; information float64 [P,6,6]; uncertain int32 [P]; fitness, inlier_rmse of each pair at the fine cap.  No host
    synchronisation.
    Where it is weak: K (K - 1) / 2 refinements grow with the square of K -- give ``pairs`` where you know which clouds overlap;
    a pair that does not overlap still yields an edge (few inliers, a small information matrix), which the optimiser must
    then drop; colours and robust losses are not taken."""
    from .refine import refine_registration
    from .robust import information_matrix
    api = "pose_graph_from_clouds"
    extension.check_cloud(api, "clouds", clouds)
    K = clouds.shape[0]
    if not 2 <= K <= MAX_NODES:
        raise VcrHipError(f"{api}: 2 ... {MAX_NODES} clouds, got {K}")
    coarse, fine = _nonneg(api, "max_dist_coarse", max_dist_coarse), _nonneg(api, "max_dist_fine", max_dist_fine)
    pairs = all_pairs(K) if pairs is None else [(int(i), int(j)) for i, j in pairs]
    if any(not 0 <= i < j < K for i, j in pairs) or len(set(pairs)) != len(pairs):
        raise VcrHipError(f"{api}: pairs must be distinct (i, j) with 0 <= i < j < {K}")
    at = {p: n for n, p in enumerate(pairs)}
    if any((i, i + 1) not in at for i in range(K - 1)):
        raise VcrHipError(f"{api}: pairs must hold every odometry pair (i, i + 1)")
    if not clouds.is_cuda:
        raise VcrHipError(f"{api} runs on the MI355X HIP path only; move the clouds to cuda (there is no CPU fallback by design)")
    dev = clouds.device
    s_host, d_host = check_edges([i for i, _ in pairs], [j for _, j in pairs], K, api)
    src_i, dst_i = s_host.to(dev, non_blocking=True), d_host.to(dev, non_blocking=True)
    clouds = clouds.contiguous().float()
    src_c, tgt_c = clouds.index_select(0, src_i.long()), clouds.index_select(0, dst_i.long())
    kw = dict(max_iterations=max_iterations, method=method, normal_k=normal_k, search=search, cell=cell)
    c = refine_registration(src_c, tgt_c, None, None, coarse, **kw)
    f = refine_registration(src_c, tgt_c, c["R"], c["t"], fine, **kw)
    info = information_matrix(src_c, tgt_c, f["R"], f["t"], fine, search=search, cell=cell)
    R0, t0 = chain_poses(f["R"], f["t"], [at[(i, i + 1)] for i in range(K - 1)])
    uncertain = torch.tensor([0 if j == i + 1 else 1 for i, j in pairs], dtype=torch.int32).to(dev, non_blocking=True)
    return {"R": R0, "t": t0, "src": src_i, "dst": dst_i, "pairs": pairs, "R_edge": f["R"], "t_edge": f["t"], "information": info,
            "uncertain": uncertain, "fitness": f["fitness"], "inlier_rmse": f["inlier_rmse"]}


def register_multiway(clouds, max_dist_coarse, max_dist_fine, method="point_to_plane", pairs=None, search="scan", anchor=0,
                      prune=True, edge_prune_threshold=0.25, criteria=None, **kw):
    """Register K overlapping clouds [K,3,N] into the frame of cloud ``anchor``: ``pose_graph_from_clouds`` and then
    ``optimize_pose_graph`` with max_correspondence_distance = max_dist_fine.  Returns a dict: R, t float64 [K,3,3], [K,3] (cloud
    i's frame -> the common frame: R[i] @ clouds[i] + t[i][:, None]), kept int32 [P], "optimized" (``optimize_pose_graph``'s
    dict) and "graph" (``pose_graph_from_clouds``'s).  Their weaknesses are this call's."""
    g = pose_graph_from_clouds(clouds, max_dist_coarse, max_dist_fine, method, pairs, search, **kw)
    o = optimize_pose_graph(g["R"], g["t"], g["src"], g["dst"], g["R_edge"], g["t_edge"], g["information"], g["uncertain"],
                            max_dist_fine, anchor, prune, edge_prune_threshold, criteria)
    return {"R": o["R"], "t": o["t"], "kept": o["kept"], "optimized": o, "graph": g}
