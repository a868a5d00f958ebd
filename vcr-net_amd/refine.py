"""ctypes binding of include/vcr_hip_refine.h and the Python API on top of it: refining a registration on the FULL clouds
 -- a trimmed point-to-point ICP (Open3D's registration_icp with a correspondence-distance cap) by
vcr_refine_f32: per cloud its own stop, on the device, no host synchronisation inside the loop.

Like ``score``, the header extends include/vcr_hip.h without touching it and this module keeps its own STRUCTS / SIGNATURES
maps, applied once to ``native.lib()`` on first use.  No CPU fallback, as everywhere."""
from __future__ import annotations

import ctypes as C
import math
import torch

from . import extension, native
from .native import VcrHipError, f32p, ptr
from .score import i32p, f64p, variant  # noqa: F401  (the search's forms are the score's: VCR_NN_SCORE_VARIANT)

MAX_ITERATIONS = 4096


class RefineArgs(native._Sized):
    _fields_ = [("struct_bytes", C.c_uint32), ("src", f32p), ("tgt", f32p), ("B", C.c_int), ("Ns", C.c_int), ("Nt", C.c_int),
                ("R", f32p), ("t", f32p), ("max_dist", C.c_float), ("max_iterations", C.c_int), ("rel_fitness", C.c_float),
                ("rel_rmse", C.c_float), ("R_out", f32p), ("t_out", f32p), ("fitness", f32p), ("rmse", f32p), ("R_ba", f32p),
                ("t_ba", f32p), ("inliers", i32p), ("sum_d2", f64p), ("iterations", i32p), ("converged", i32p),
                ("nn_idx", i32p), ("nn_d2", f32p), ("variant", C.c_int)]


STRUCTS = {"vcr_refine_args": RefineArgs}

# name -> (restype, [argtypes]): the prototypes of include/vcr_hip_refine.h (tests/test_refine_cpu.py holds them to it)
SIGNATURES = extension.workspace_signatures("vcr_refine", RefineArgs)

lib = extension.typed_lib(SIGNATURES)                      # native.lib() with this module's entry points typed (once)


def refine_form(B, Ns, Nt, cu_count=256, variant=0, max_iterations=30):
    """vcr_refine_form (host only with an explicit cu_count): (source points per lane, target splits, workspace bytes) of the
    search vcr_refine_f32 would run for [B,3,Ns] against [B,3,Nt] on a device of cu_count compute units."""
    a = RefineArgs(src=0x1000, tgt=0x2000, B=B, Ns=Ns, Nt=Nt, max_iterations=max_iterations, R_out=0x3000, t_out=0x4000,
                   fitness=0x5000, rmse=0x6000, variant=variant)                  # (never dereferenced on the host)
    return extension.form(lib(), "vcr_refine", a, cu_count)


def _cloud(name, x):
    extension.check_cloud("refine_registration", name, x)


def _threshold(name, v):
    v = float(v)
    if not (math.isfinite(v) and v >= 0.0):
        raise VcrHipError(f"refine_registration: {name} must be finite and >= 0, got {v}")
    return v


@native._guarded
def refine(src, tgt, R=None, t=None, max_dist=0.0, max_iterations=30, rel_fitness=1e-6, rel_rmse=1e-6, variant=0, want_nn=True,
           guard=0, prefill=None, tgt_normals=None, src_normals=None, epsilon=None, search="scan", cell=None, order=0):
    """vcr_refine_f32 on src [B,3,Ns], tgt [B,3,Nt] (device, fp32) from the pose (R [B,3,3], t [B,3]; both None = identity)
    -> dict of R [B,3,3], t [B,3], R_ba, t_ba, fitness, rmse float32 [B], inliers, iterations, converged int32 [B], sum_d2
    float64 [B], nn_idx int32 / nn_d2 [B,Ns] (want_nn).
    guard / prefill (tests): every output is a view of a buffer with `guard` more elements behind it, all of it -- and the
    workspace -- filled with the byte `prefill` before the launch; the buffers come back under "_raw".
    tgt_normals [B,3,Nt]: vcr_refine_plane_f32 instead -- the same loop with the point-to-plane fit (plane.refine_plane checks
    them and calls this).  With src_normals [B,3,Ns] and epsilon as well: vcr_refine_gicp_f32, the plane-to-plane fit
    (gicp.refine_gicp checks them and calls this).
    search="grid": the entry point's grid sibling instead (include/vcr_hip_gridnn.h; variant must be 0), with cell (None: the
    automatic edge) and order (0 = the plan's, 1 = the source's cell order, 2 = index order) as its vcr_grid_nn_args."""
    from . import gridnn
    gridnn.check_search("refine_registration", search)
    cell = gridnn.check_cell("refine_registration", cell)
    extension.check_pair("refine_registration", src, tgt, R, t)
    max_dist = _threshold("max_dist", max_dist)
    rel_fitness, rel_rmse = _threshold("rel_fitness", rel_fitness), _threshold("rel_rmse", rel_rmse)
    max_iterations = int(max_iterations)
    if max_iterations < 0:
        raise VcrHipError(f"refine_registration: max_iterations must be >= 0, got {max_iterations}")
    dev, B, Ns, Nt, src, tgt, R, t = extension.take_pair("refine_registration", src, tgt, R, t)
    out, raw = extension.outputs(dev, guard, prefill)
    o = {"R": out("R", B * 9, torch.float32).view(B, 3, 3), "t": out("t", B * 3, torch.float32).view(B, 3),
         "R_ba": out("R_ba", B * 9, torch.float32).view(B, 3, 3), "t_ba": out("t_ba", B * 3, torch.float32).view(B, 3),
         "fitness": out("fitness", B, torch.float32), "rmse": out("rmse", B, torch.float32),
         "inliers": out("inliers", B, torch.int32), "sum_d2": out("sum_d2", B, torch.float64),
         "iterations": out("iterations", B, torch.int32), "converged": out("converged", B, torch.int32)}
    if want_nn:
        o["nn_idx"], o["nn_d2"] = out("nn_idx", B * Ns, torch.int32).view(B, Ns), out("nn_d2", B * Ns, torch.float32).view(B, Ns)
    Args, L, entry = RefineArgs, lib(), "vcr_refine"
    if src_normals is not None:
        from . import gicp
        Args, L, entry = gicp.RefineGicpArgs, gicp.lib(), "vcr_refine_gicp"
    elif tgt_normals is not None:
        from . import plane
        Args, L, entry = plane.RefinePlaneArgs, plane.lib(), "vcr_refine_plane"
    a = Args(ptr(src), ptr(tgt), B, Ns, Nt, ptr(R), ptr(t), max_dist, max_iterations, rel_fitness, rel_rmse,
             ptr(o["R"]), ptr(o["t"]), ptr(o["fitness"]), ptr(o["rmse"]), ptr(o["R_ba"]), ptr(o["t_ba"]),
             ptr(o["inliers"]), ptr(o["sum_d2"]), ptr(o["iterations"]), ptr(o["converged"]),
             ptr(o.get("nn_idx")), ptr(o.get("nn_d2")), int(variant))
    if tgt_normals is not None:
        a.tgt_normals = ptr(tgt_normals)
    if src_normals is not None:
        a.src_normals, a.epsilon = ptr(src_normals), epsilon
    if search == "grid":
        extension.call_with_workspace(gridnn.lib(), gridnn.entry_of(entry), a, dev, prefill, second=gridnn.grid_args(cell, order))
    else:
        extension.call_with_workspace(L, entry, a, dev, prefill)
    if guard or prefill is not None:
        o["_raw"] = raw
    return o


METHODS = ("point_to_point", "point_to_plane", "generalized")


def refine_registration(src, tgt, R=None, t=None, max_dist=0.0, max_iterations=30, rel_fitness=1e-6, rel_rmse=1e-6,
                        want_nn=False, method="point_to_point", tgt_normals=None, normal_k=20, src_normals=None, epsilon=1e-3,
                        centre=False, search="scan", cell=None):
    """Improve the pose (R, t) on the FULL clouds: src [B,3,Ns], tgt [B,3,Nt] (Ns != Nt allowed, each up to 131 072 points;
    device tensors).  An ICP: every round matches each moved source point to its nearest target point, keeps the pairs within
    max_dist and solves the best rigid update for them; a cloud stops on its own when fitness and inlier RMSE both change by
    less than rel_fitness / rel_rmse, when too few pairs are left, or after max_iterations updates.
    method "point_to_point" (the default): the update pulls every point onto its neighbour (at least three pairs).
    method "point_to_plane": the update pulls every point onto its neighbour's tangent plane, so the clouds may slide along the
    surface -- fewer rounds where they are different samplings of one surface (at least six pairs, and normals that span:
    a flat target stops at once).  tgt_normals [B,3,Nt] are the target's unit normals; None: estimate_normals(tgt, normal_k).
    method "generalized": plane to plane (generalized ICP) -- every residual is weighed by the local surfaces of BOTH clouds,
    each point's covariance epsilon along its normal and 1 across it: the fit for two independent samplings of one surface (at
    least three pairs that are not collinear).  src_normals [B,3,Ns], tgt_normals [B,3,Nt] are unit normals of either sign;
    None: estimate_normals(cloud, normal_k).  Covariances of the caller's own are not taken.
    Returns a dict:
      R, t           float32 [B,3,3], [B,3]   the refined pose (src -> tgt);  R_ba, t_ba: its inverse
      fitness, inlier_rmse, inliers           of the refined pose, exactly score_registration(src, tgt, R, t, max_dist)'s
      iterations     int32 [B]                updates applied;  converged  int32 [B]: 1 = stopped by the rel_* test
      nn_idx, nn_d2 (want_nn)                 int64 / float32 [B,Ns], as score_registration's
    R = t = None: start from the identity.
    centre: False works in the caller's frame.  The six-unknown fits ("point_to_plane", "generalized") turn about the frame's
    origin, and estimate_normals' search cancels in fp32 far from it: on a cloud whose distance from the origin is a hundred
    times its extent they lose every inlier from a start a few degrees off.  True moves the source and
    the target each to its own centre first (``centred``: the mean of the finite coordinates), a pair (c_src, c_tgt) of [B,3]
    tensors to the centres given -- before anything else, the normals estimated inside included --, runs the method there,
    carries R, t, R_ba, t_ba back (``uncentred_pose``) and takes fitness, inlier_rmse, inliers, nn_idx and nn_d2 from the
    caller's clouds at the returned pose.
    search: "scan" (the default) tests every source point against every target point.  "grid" walks the target's uniform grid
     and stops at max_dist: the same inliers, fitness, inlier_rmse, poses, iterations and converged,
    bit for bit; the one difference is that a source point without a target point within max_dist reports nn_idx = -1,
    nn_d2 = +inf where the scan reports the far neighbour it found.  Measured (DESIGN.md section 4.20,
    profiles/gridnn_bench.txt): it wins from about 16 384 points for one cloud and 4 096 points a cloud for sixteen (x5-x10 an
    evaluation, x12-x25 a round at 131 072 points) and loses below; it loses on clouds that fill little of their bounding box
    (tight clusters); with many source points without a partner inside the target's box its advantage falls from x7-x9.5 at
    max_dist <= 1 automatic grid edge to x3-x5 at 4 edges and x1.2-x1.7 at 8: take it for max_dist up to about four edges.
    cell: None for the target's automatic edge, otherwise the cells' edge -- it changes the time and never the result.
    It serves every round of the three methods and the closing evaluation of centre."""
    from . import gridnn
    gridnn.check_search("refine_registration", search)
    gridnn.check_cell("refine_registration", cell)
    if method not in METHODS:
        raise VcrHipError(f"refine_registration: method must be one of {METHODS}, got {method!r}")
    if method != "generalized" and (src_normals is not None or epsilon != 1e-3):
        raise VcrHipError("refine_registration: src_normals and epsilon are read by method='generalized' only")
    if centre is not False and centre is not None:
        extension.check_pair("refine_registration", src, tgt, R, t)
        return _refine_centred(src, tgt, R, t, max_dist, centre, want_nn,
                               dict(max_iterations=max_iterations, rel_fitness=rel_fitness, rel_rmse=rel_rmse, method=method,
                                    tgt_normals=tgt_normals, normal_k=normal_k, src_normals=src_normals, epsilon=epsilon,
                                    search=search, cell=cell))
    if method == "generalized":
        from . import gicp, plane
        _cloud("src", src)
        _cloud("tgt", tgt)
        epsilon = gicp.check_epsilon(epsilon)
        if tgt_normals is None:
            tgt_normals = plane.estimate_normals(tgt, normal_k)
        if src_normals is None:
            src_normals = plane.estimate_normals(src, normal_k)
        f = gicp.refine_gicp(src, tgt, src_normals, tgt_normals, R, t, max_dist, max_iterations, rel_fitness, rel_rmse,
                             want_nn=want_nn, epsilon=epsilon, search=search, cell=cell)
    elif method == "point_to_plane":
        from . import plane
        _cloud("src", src)
        _cloud("tgt", tgt)
        if tgt_normals is None:
            tgt_normals = plane.estimate_normals(tgt, normal_k)
        f = plane.refine_plane(src, tgt, tgt_normals, R, t, max_dist, max_iterations, rel_fitness, rel_rmse, want_nn=want_nn,
                               search=search, cell=cell)
    else:
        if tgt_normals is not None:
            raise VcrHipError("refine_registration: tgt_normals are read by method='point_to_plane' only")
        f = refine(src, tgt, R, t, max_dist, max_iterations, rel_fitness, rel_rmse, want_nn=want_nn, search=search, cell=cell)
    res = {"R": f["R"], "t": f["t"], "R_ba": f["R_ba"], "t_ba": f["t_ba"], "fitness": f["fitness"], "inlier_rmse": f["rmse"],
           "inliers": f["inliers"], "iterations": f["iterations"], "converged": f["converged"]}
    if want_nn:
        res["nn_idx"], res["nn_d2"] = f["nn_idx"].long(), f["nn_d2"]
    return res


def uncentre_refined(res, src, tgt, c_src, c_tgt, max_dist, want_nn=False, search="scan", cell=None):
    """refine_registration's dict from clouds centred at c_src, c_tgt -> the same in the caller's frame: the poses carried back,
    the evaluation taken again on the caller's clouds (src, tgt) at the pose returned."""
    from .centre import uncentred_pose
    from .score import score_registration
    out = dict(res)
    _, out["t"] = uncentred_pose(res["R"], res["t"], c_src, c_tgt)
    _, out["t_ba"] = uncentred_pose(res["R_ba"], res["t_ba"], c_tgt, c_src)
    out.update(score_registration(src, tgt, out["R"], out["t"], max_dist, want_nn=want_nn, search=search, cell=cell))
    return out


def _refine_centred(src, tgt, R, t, max_dist, centre, want_nn, kw):
    from .centre import centred_pose, take_centres
    src_c, c_src, tgt_c, c_tgt = take_centres("refine_registration", centre, src, tgt)
    if R is not None:
        native.same_device(src, tgt, R, t)
        if tuple(R.shape) != (src.shape[0], 3, 3) or tuple(t.shape) != (src.shape[0], 3):
            raise VcrHipError(f"refine_registration: R must be [B, 3, 3] and t [B, 3] with B = {src.shape[0]}, got "
                              f"{tuple(R.shape)} and {tuple(t.shape)}")
        R, t = R.contiguous().float(), t.contiguous().float()
    R_c, t_c = centred_pose(R, t, c_src, c_tgt)
    res = refine_registration(src_c, tgt_c, R_c, t_c, max_dist, want_nn=False, centre=False, **kw)
    return uncentre_refined(res, src, tgt, c_src, c_tgt, max_dist, want_nn, search=kw["search"], cell=kw["cell"])
