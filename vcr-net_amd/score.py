"""ctypes binding of include/vcr_hip_score.h and the Python API on top of it: scoring a registration on the FULL clouds
 -- per source point the nearest target point, per cloud fitness and inlier RMSE (Open3D's
evaluate_registration) -- by vcr_nn_score_f32, without an Ns x Nt matrix.

The header extends include/vcr_hip.h without touching it, and so does this module for ``native``: its own STRUCTS / SIGNATURES
maps, in the same shape, applied once to ``native.lib()`` on first use.  No CPU fallback, as everywhere."""
from __future__ import annotations

import ctypes as C
import math
import torch

from . import extension, native
from .native import VcrHipError, f32p, ptr

MAX_N = 131072
QUERIES_PER_LANE = (1, 2, 4)
MAX_SPLITS = 128


i32p = f64p = C.c_void_p                                   # device pointers travel as integers, like f32p: the names say what they point to


class NnScoreArgs(native._Sized):
    _fields_ = [("struct_bytes", C.c_uint32), ("src", f32p), ("tgt", f32p), ("B", C.c_int), ("Ns", C.c_int), ("Nt", C.c_int),
                ("R", f32p), ("t", f32p), ("max_dist", C.c_float), ("nn_idx", i32p), ("nn_d2", f32p), ("inliers", i32p),
                ("sum_d2", f64p), ("fitness", f32p), ("rmse", f32p), ("variant", C.c_int)]


STRUCTS = {"vcr_nn_score_args": NnScoreArgs}

# name -> (restype, [argtypes]): the prototypes of include/vcr_hip_score.h (tests/test_nnscore_cpu.py holds them to it)
SIGNATURES = extension.workspace_signatures("vcr_nn_score", NnScoreArgs)

lib = extension.typed_lib(SIGNATURES)                      # native.lib() with this module's entry points typed (once)


def variant(queries_per_lane: int = 0, target_splits: int = 0) -> int:
    """vcr_nn_score_args.variant that forces a form (VCR_NN_SCORE_VARIANT): 0 leaves that half to the plan."""
    return int(queries_per_lane) | (int(target_splits) << 8)


def nn_score_form(B, Ns, Nt, cu_count=256, variant=0):
    """vcr_nn_score_form (host only with an explicit cu_count): (source points per lane, target splits, workspace bytes)
    vcr_nn_score_f32 would run [B,3,Ns] against [B,3,Nt] with on a device of cu_count compute units."""
    a = NnScoreArgs(0x1000, 0x2000, B, Ns, Nt, None, None, 0.0, None, None, None, None, 0x3000, 0x4000, variant)   # (never dereferenced on the host)
    return extension.form(lib(), "vcr_nn_score", a, cu_count)


@native._guarded
def nn_score(src, tgt, R=None, t=None, max_dist=0.0, variant=0, want_nn=True, guard=0, prefill=None, search="scan", cell=None,
             order=0):
    """vcr_nn_score_f32 on src [B,3,Ns], tgt [B,3,Nt] (device, fp32) under the pose (R [B,3,3], t [B,3]; both None = identity)
    -> dict of nn_idx int32 [B,Ns], nn_d2 [B,Ns] (want_nn), inliers int32 [B], sum_d2 float64 [B], fitness, rmse float32 [B].
    guard / prefill (tests): every output is a view of a buffer with `guard` more elements behind it, all of it filled with the
    byte `prefill` before the launch; the buffers come back under "_raw".
    search="grid": vcr_nn_score_grid_f32 instead (include/vcr_hip_gridnn.h; variant must be 0), with cell (None: the automatic
    edge) and order (0 = the plan's, 1 = the source's cell order, 2 = index order) as its vcr_grid_nn_args; the workspace is
    prefilled too."""
    from . import gridnn
    gridnn.check_search("score_registration", search)
    cell = gridnn.check_cell("score_registration", cell)
    extension.check_pair("score_registration", src, tgt, R, t)
    max_dist = float(max_dist)
    if not (math.isfinite(max_dist) and max_dist >= 0.0):
        raise VcrHipError(f"score_registration: max_dist must be finite and >= 0, got {max_dist}")
    dev, B, Ns, Nt, src, tgt, R, t = extension.take_pair("score_registration", src, tgt, R, t)
    out, raw = extension.outputs(dev, guard, prefill)
    o = {}
    if want_nn:
        o["nn_idx"], o["nn_d2"] = out("nn_idx", B * Ns, torch.int32).view(B, Ns), out("nn_d2", B * Ns, torch.float32).view(B, Ns)
    o["inliers"], o["sum_d2"] = out("inliers", B, torch.int32), out("sum_d2", B, torch.float64)
    o["fitness"], o["rmse"] = out("fitness", B, torch.float32), out("rmse", B, torch.float32)
    a = NnScoreArgs(ptr(src), ptr(tgt), B, Ns, Nt, ptr(R), ptr(t), max_dist, ptr(o.get("nn_idx")), ptr(o.get("nn_d2")),
                    ptr(o["inliers"]), ptr(o["sum_d2"]), ptr(o["fitness"]), ptr(o["rmse"]), int(variant))
    if search == "grid":
        extension.call_with_workspace(gridnn.lib(), "vcr_nn_score_grid", a, dev, prefill, second=gridnn.grid_args(cell, order))
    else:
        extension.call_with_workspace(lib(), "vcr_nn_score", a, dev)
    if guard or prefill is not None:
        o["_raw"] = raw
    return o


def score_registration(src, tgt, R=None, t=None, max_dist=0.0, symmetric=False, want_nn=False, search="scan", cell=None):
    """How good is the pose (R, t) for the FULL clouds?  src [B,3,Ns], tgt [B,3,Nt] (Ns != Nt allowed, each up to 131 072
    points; device tensors): every source point is moved by the pose and matched to its nearest target point.  Returns a dict:
      fitness      float32 [B]   the fraction of source points within max_dist of the target
      inlier_rmse  float32 [B]   the RMS distance of those points to their neighbours (0 without inliers)
      inliers      int32 [B]     their number
      nn_idx, nn_d2 (want_nn)    int64 / float32 [B,Ns]: the neighbour (the lowest index among equals; -1 when no target point
                                 is at a finite distance) and the squared distance to it
    symmetric: also tgt -> src under the inverse pose (native.pose_step's R_ba, t_ba), as fitness_ba, inlier_rmse_ba,
    inliers_ba.  R = t = None: the identity.
    search: "scan" (the default) tests every source point against every target point.  "grid" walks the target's uniform grid
     and stops at max_dist: the same inliers, fitness, inlier_rmse and poses, bit for bit; the one
    difference is that a source point without a target point within max_dist reports nn_idx = -1, nn_d2 = +inf where the scan
    reports the far neighbour it found.  Measured (DESIGN.md section 4.20,
    profiles/gridnn_bench.txt): it wins from about 16 384 points for one cloud and 4 096 points a cloud for sixteen (x5-x10 an
    evaluation, x12-x25 a round at 131 072 points) and loses below; it loses on clouds that fill little of their bounding box
    (tight clusters); with many source points without a partner inside the target's box its advantage falls from x7-x9.5 at
    max_dist <= 1 automatic grid edge to x3-x5 at 4 edges and x1.2-x1.7 at 8: take it for max_dist up to about four edges.
    cell: None for the target's automatic edge, otherwise the cells' edge -- it changes the time and never the result.
    With symmetric, the way back is searched the same way (on the source's grid; a forced cell serves both)."""
    f = nn_score(src, tgt, R, t, max_dist, want_nn=want_nn, search=search, cell=cell)
    res = {"fitness": f["fitness"], "inlier_rmse": f["rmse"], "inliers": f["inliers"]}
    if want_nn:
        res["nn_idx"], res["nn_d2"] = f["nn_idx"].long(), f["nn_d2"]
    if symmetric:
        R_ba = t_ba = None
        if R is not None:
            _, _, _, R_ba, t_ba = native.pose_step(R, t)
        g = nn_score(tgt, src, R_ba, t_ba, max_dist, want_nn=False, search=search, cell=cell)
        res.update(fitness_ba=g["fitness"], inlier_rmse_ba=g["rmse"], inliers_ba=g["inliers"])
    return res
