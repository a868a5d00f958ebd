"""ctypes binding of include/robust/vcr_hip_robust.h and the Python API on top of it: the
point-to-plane refinement with a robust weight per pair (vcr_refine_robust_f32: Open3D's
TransformationEstimationPointToPlane(kernel) with HuberLoss, CauchyLoss, GMLoss, TukeyLoss) and the information matrix of a
registered pair (vcr_information_f32: get_information_matrix_from_point_clouds), each with its grid sibling.

Like ``colored``, the header extends include/vcr_hip.h without touching it and this module keeps its own STRUCTS / SIGNATURES
maps, applied once to ``native.lib()`` on first use.  No CPU fallback, as everywhere."""
from __future__ import annotations

import ctypes as C
import math
import torch

from . import extension, gridnn, native, plane, refine
from .native import VcrHipError, f32p, ptr
from .score import f64p

LOSSES = ("l2", "huber", "cauchy", "gm", "tukey")          # VCR_LOSS_*: a loss' value is its index


class RefineRobustArgs(native._Sized):
    _fields_ = list(plane.RefinePlaneArgs._fields_) + [("loss", C.c_int), ("k", C.c_float)]   # vcr_refine_plane_args' fields lead


class InformationArgs(native._Sized):
    _fields_ = list(refine.RefineArgs._fields_) + [("information", f64p)]      # vcr_refine_args' fields lead


STRUCTS = {"vcr_refine_robust_args": RefineRobustArgs, "vcr_information_args": InformationArgs}

# name -> (restype, [argtypes]): the prototypes of include/robust/vcr_hip_robust.h (tests/test_robust_cpu.py holds them to it)
SIGNATURES = {**extension.workspace_signatures("vcr_refine_robust", RefineRobustArgs),
              **extension.workspace_signatures2("vcr_refine_robust_grid", RefineRobustArgs, gridnn.GridNnArgs),
              **extension.workspace_signatures("vcr_information", InformationArgs),
              **extension.workspace_signatures2("vcr_information_grid", InformationArgs, gridnn.GridNnArgs)}

lib = extension.typed_lib(SIGNATURES)                      # native.lib() with this module's entry points typed (once)

_API = "refine_registration_robust"
_INFO = "information_matrix"


def _form_args(B, Ns, Nt, variant, max_iterations, loss=4, k=0.01):
    return RefineRobustArgs(src=0x1000, tgt=0x2000, B=B, Ns=Ns, Nt=Nt, max_iterations=max_iterations, R_out=0x3000, t_out=0x4000,
                            fitness=0x5000, rmse=0x6000, variant=variant, tgt_normals=0x7000, loss=loss,
                            k=k)                           # (never dereferenced on the host)


def refine_robust_form(B, Ns, Nt, cu_count=256, variant=0, max_iterations=30):
    """vcr_refine_robust_form (host only with an explicit cu_count): (source points per lane, target splits, workspace bytes),
    as refine.refine_form."""
    return extension.form(lib(), "vcr_refine_robust", _form_args(B, Ns, Nt, variant, max_iterations), cu_count)


def refine_robust_grid_form(B, Ns, Nt, order=0, cell=0.0, cu_count=256, max_iterations=30):
    """vcr_refine_robust_grid_form (host only): as gridnn.refine_grid_form."""
    L = lib()
    a, g = _form_args(B, Ns, Nt, 0, max_iterations), gridnn.grid_args(cell, order)
    cells, taken, queries = C.c_int(0), C.c_int(0), C.c_int(0)
    native.check(L.vcr_refine_robust_grid_form(C.byref(a), C.byref(g), cu_count, C.byref(cells), C.byref(taken), C.byref(queries)),
                 "vcr_refine_robust_grid_form")
    return cells.value, taken.value, queries.value, L.vcr_refine_robust_grid_workspace_bytes(C.byref(a), C.byref(g), cu_count)


def information_form(B, Ns, Nt, cu_count=256, variant=0):
    """vcr_information_form (host only with an explicit cu_count): as refine.refine_form."""
    a = InformationArgs(src=0x1000, tgt=0x2000, B=B, Ns=Ns, Nt=Nt, R_out=0x3000, t_out=0x4000, fitness=0x5000, rmse=0x6000,
                        variant=variant, information=0x7000)                       # (never dereferenced on the host)
    return extension.form(lib(), "vcr_information", a, cu_count)


def check_loss(loss, k, api=_API):
    """-> (VCR_LOSS_* value, k as a float): loss is one of LOSSES, k finite and > 0 (the caller's: there is no default)."""
    if loss not in LOSSES:
        raise VcrHipError(f"{api}: loss must be one of {LOSSES}, got {loss!r}")
    if k is None:
        raise VcrHipError(f"{api}: k has no default -- it is the noise scale of your sensor, in the clouds' unit")
    try:
        kf = float(k)
    except (TypeError, ValueError):
        kf = float("nan")
    if not (math.isfinite(kf) and kf > 0.0):
        raise VcrHipError(f"{api}: k must be finite and > 0, got {k!r}")
    return LOSSES.index(loss), kf


def _threshold(api, name, v):
    v = float(v)
    if not (math.isfinite(v) and v >= 0.0):
        raise VcrHipError(f"{api}: {name} must be finite and >= 0, got {v}")
    return v


def _normals(api, tgt_normals, tgt):
    if not torch.is_tensor(tgt_normals) or tuple(tgt_normals.shape) != tuple(tgt.shape):
        raise VcrHipError(f"{api}: tgt_normals must be [B, 3, Nt] like tgt {tuple(tgt.shape)}, got "
                          f"{tuple(tgt_normals.shape) if torch.is_tensor(tgt_normals) else type(tgt_normals).__name__}")
    if not tgt_normals.is_cuda or tgt_normals.device != tgt.device:
        raise VcrHipError(f"{api}: tgt_normals must live on the device of the clouds (there is no CPU fallback)")
    return tgt_normals.contiguous().float()


def _outputs(out, B, Ns, want_nn):
    o = {"R": out("R", B * 9, torch.float32).view(B, 3, 3), "t": out("t", B * 3, torch.float32).view(B, 3),
         "R_ba": out("R_ba", B * 9, torch.float32).view(B, 3, 3), "t_ba": out("t_ba", B * 3, torch.float32).view(B, 3),
         "fitness": out("fitness", B, torch.float32), "rmse": out("rmse", B, torch.float32),
         "inliers": out("inliers", B, torch.int32), "sum_d2": out("sum_d2", B, torch.float64),
         "iterations": out("iterations", B, torch.int32), "converged": out("converged", B, torch.int32)}
    if want_nn:
        o["nn_idx"], o["nn_d2"] = out("nn_idx", B * Ns, torch.int32).view(B, Ns), out("nn_d2", B * Ns, torch.float32).view(B, Ns)
    return o


@native._guarded
def refine_robust(src, tgt, tgt_normals, R=None, t=None, max_dist=0.0, loss="tukey", k=None, max_iterations=30, rel_fitness=1e-6,
                  rel_rmse=1e-6, variant=0, want_nn=True, guard=0, prefill=None, search="scan", cell=None, order=0):
    """vcr_refine_robust_f32: plane.refine_plane's arguments and dict, with the loss (one of LOSSES) and its scale k behind
    max_dist.  search="grid": vcr_refine_robust_grid_f32, as refine.refine's."""
    gridnn.check_search(_API, search)
    cell = gridnn.check_cell(_API, cell)
    extension.check_pair(_API, src, tgt, R, t)
    loss, k = check_loss(loss, k)
    max_dist = _threshold(_API, "max_dist", max_dist)
    rel_fitness, rel_rmse = _threshold(_API, "rel_fitness", rel_fitness), _threshold(_API, "rel_rmse", rel_rmse)
    max_iterations = int(max_iterations)
    if max_iterations < 0:
        raise VcrHipError(f"{_API}: max_iterations must be >= 0, got {max_iterations}")
    tgt_normals = _normals(_API, tgt_normals, tgt)
    dev, B, Ns, Nt, src, tgt, R, t = extension.take_pair(_API, src, tgt, R, t)
    out, raw = extension.outputs(dev, guard, prefill)
    o = _outputs(out, B, Ns, want_nn)
    a = RefineRobustArgs(ptr(src), ptr(tgt), B, Ns, Nt, ptr(R), ptr(t), max_dist, max_iterations, rel_fitness, rel_rmse,
                         ptr(o["R"]), ptr(o["t"]), ptr(o["fitness"]), ptr(o["rmse"]), ptr(o["R_ba"]), ptr(o["t_ba"]),
                         ptr(o["inliers"]), ptr(o["sum_d2"]), ptr(o["iterations"]), ptr(o["converged"]),
                         ptr(o.get("nn_idx")), ptr(o.get("nn_d2")), int(variant), ptr(tgt_normals), loss, k)
    if search == "grid":
        extension.call_with_workspace(lib(), "vcr_refine_robust_grid", a, dev, prefill, second=gridnn.grid_args(cell, order))
    else:
        extension.call_with_workspace(lib(), "vcr_refine_robust", a, dev, prefill)
    if guard or prefill is not None:
        o["_raw"] = raw
    return o


@native._guarded
def information(src, tgt, R=None, t=None, max_dist=0.0, variant=0, want_nn=True, guard=0, prefill=None, search="scan", cell=None,
                order=0):
    """vcr_information_f32 on src [B,3,Ns], tgt [B,3,Nt] (device, fp32) under the pose (R, t; both None = identity) ->
    refine.refine's dict (the pose given, the evaluation at it, iterations = converged = 0) plus "information", float64
    [B,6,6].  guard / prefill (tests) and search / cell / order: as refine.refine's."""
    gridnn.check_search(_INFO, search)
    cell = gridnn.check_cell(_INFO, cell)
    extension.check_pair(_INFO, src, tgt, R, t)
    max_dist = _threshold(_INFO, "max_dist", max_dist)
    dev, B, Ns, Nt, src, tgt, R, t = extension.take_pair(_INFO, src, tgt, R, t)
    out, raw = extension.outputs(dev, guard, prefill)
    o = _outputs(out, B, Ns, want_nn)
    o["information"] = out("information", B * 36, torch.float64).view(B, 6, 6)
    a = InformationArgs(ptr(src), ptr(tgt), B, Ns, Nt, ptr(R), ptr(t), max_dist, 0, 0.0, 0.0,
                        ptr(o["R"]), ptr(o["t"]), ptr(o["fitness"]), ptr(o["rmse"]), ptr(o["R_ba"]), ptr(o["t_ba"]),
                        ptr(o["inliers"]), ptr(o["sum_d2"]), ptr(o["iterations"]), ptr(o["converged"]),
                        ptr(o.get("nn_idx")), ptr(o.get("nn_d2")), int(variant), ptr(o["information"]))
    if search == "grid":
        extension.call_with_workspace(lib(), "vcr_information_grid", a, dev, prefill, second=gridnn.grid_args(cell, order))
    else:
        extension.call_with_workspace(lib(), "vcr_information", a, dev, prefill)
    if guard or prefill is not None:
        o["_raw"] = raw
    return o


def refine_registration_robust(src, tgt, R=None, t=None, max_dist=0.0, loss="tukey", k=None, max_iterations=30, rel_fitness=1e-6,
                               rel_rmse=1e-6, want_nn=False, tgt_normals=None, normal_k=20, centre=False, search="scan", cell=None):
    """Improve the pose (R, t) on the FULL clouds point to plane, with a robust kernel: src [B,3,Ns], tgt [B,3,Nt] device
    tensors -- Open3D's registration_icp with TransformationEstimationPointToPlane(kernel).  ``refine_registration``'s loop,
    stops and dict with method="point_to_plane"'s fit, in which every pair is weighed by its own residual r, the distance of
    the moved point from its neighbour's tangent plane: pairs that lie within max_dist and are still wrong -- a second surface
    behind the first, an object that moved, sensor ghosts -- pull a least-squares fit along, and pull this one the less the
    farther off they are.
    loss: "l2" (w = 1: method="point_to_plane" itself, bit for bit), "huber" (w = k / |r| beyond k), "cauchy"
    (w = 1 / (1 + (r / k)^2)), "gm" (w = k / (k + r^2)^2) or "tukey" (w = (1 - (r / k)^2)^2 within k, 0 beyond).
    k: the noise scale of YOUR sensor, in the clouds' unit -- residuals up to about k count as noise, those far beyond as
    wrong.  There is no honest default: k=None raises.
    tgt_normals [B,3,Nt]: the target's unit normals; None: estimate_normals(tgt, normal_k).  centre, search and cell: as
    ``refine_registration``'s.
    Returns ``refine_registration``'s dict.  fitness, inlier_rmse and inliers are the GEOMETRIC figures of the refined pose,
    exactly score_registration(src, tgt, R, t, max_dist)'s, not the weighted residual.
    Where it is weak: "tukey" and "gm" redescend -- a pair far from the surface gets next to no pull --, so from a poor start,
    where the good pairs are far off too, they lose the pose (measured: Tukey at k = 0.02 from 6 degrees and 0.04 off diverges
    on two clouds of four).  Run "l2" or "cauchy" first and start them from its result.  A k below the noise throws the good
    pairs away (with every weight zero the cloud stops at once, converged = 0); a k far above it is least squares again."""
    gridnn.check_search(_API, search)
    gridnn.check_cell(_API, cell)
    check_loss(loss, k)
    extension.check_pair(_API, src, tgt, R, t)
    kw = dict(loss=loss, k=k, max_iterations=max_iterations, rel_fitness=rel_fitness, rel_rmse=rel_rmse, tgt_normals=tgt_normals,
              normal_k=normal_k, search=search, cell=cell)
    if centre is not False and centre is not None:
        from .centre import centred_pose, take_centres
        src_c, c_src, tgt_c, c_tgt = take_centres(_API, centre, src, tgt)
        if R is not None:
            native.same_device(src, tgt, R, t)
            if tuple(R.shape) != (src.shape[0], 3, 3) or tuple(t.shape) != (src.shape[0], 3):
                raise VcrHipError(f"{_API}: R must be [B, 3, 3] and t [B, 3] with B = {src.shape[0]}, got "
                                  f"{tuple(R.shape)} and {tuple(t.shape)}")
            R, t = R.contiguous().float(), t.contiguous().float()
        R_c, t_c = centred_pose(R, t, c_src, c_tgt)
        res = refine_registration_robust(src_c, tgt_c, R_c, t_c, max_dist, want_nn=False, centre=False, **kw)
        return refine.uncentre_refined(res, src, tgt, c_src, c_tgt, max_dist, want_nn, search=search, cell=cell)
    if tgt_normals is None:
        tgt_normals = plane.estimate_normals(tgt, normal_k)
    f = refine_robust(src, tgt, tgt_normals, R, t, max_dist, loss, k, max_iterations, rel_fitness, rel_rmse, want_nn=want_nn,
                      search=search, cell=cell)
    res = {"R": f["R"], "t": f["t"], "R_ba": f["R_ba"], "t_ba": f["t_ba"], "fitness": f["fitness"], "inlier_rmse": f["rmse"],
           "inliers": f["inliers"], "iterations": f["iterations"], "converged": f["converged"]}
    if want_nn:
        res["nn_idx"], res["nn_d2"] = f["nn_idx"].long(), f["nn_d2"]
    return res


def information_matrix(src, tgt, R=None, t=None, max_dist=0.0, search="scan", cell=None, want_score=False):
    """The 6 x 6 information matrix of the pair under the pose (R, t) -> float64 [B,6,6]: Open3D's
    get_information_matrix_from_point_clouds, the weight of the pair's edge in a pose graph (multiway registration).  Over the
    source points with a target point within max_dist, each with its nearest one q: the sum of G^T G, G = [ -[q]x | I ] --
    rotation first, translation behind; the lower right block is the number of inliers on the diagonal.  One search and nine
    sums on the device; no pair within max_dist gives the zero matrix.
    search and cell: as ``score_registration``'s.  want_score: also ``score_registration``'s dict at that pose, from the same
    search -- returned as (information, dict).
    Where it is weak: it counts pairs and where they lie and knows nothing of how well they fit -- a wrong pose with many pairs
    within max_dist weighs as much as a right one; and its rotation block is taken about the frame's origin, as Open3D's, so
    it grows with the square of the target's distance from it."""
    f = information(src, tgt, R, t, max_dist, want_nn=False, search=search, cell=cell)
    if not want_score:
        return f["information"]
    return f["information"], {"fitness": f["fitness"], "inlier_rmse": f["rmse"], "inliers": f["inliers"]}
