"""ctypes binding of include/vcr_hip_outlier.h and the Python API on top of it: removing a cloud's stray
points on the device -- Open3D's remove_statistical_outlier (vcr_outlier_stat_f32, on the library's kNN) and
remove_radius_outlier (vcr_outlier_radius_f32, a brute-force count, or its grid sibling of ``radius``) -- the step between ``voxel_down_sample`` and
``estimate_normals``.

The header extends include/vcr_hip.h without touching it, and so does this module for ``native``: its own STRUCTS / SIGNATURES
maps, in the same shape, applied once to ``native.lib()`` on first use.  No CPU fallback, as everywhere."""
from __future__ import annotations

import ctypes as C
import math
import operator
import torch

from . import extension, grid, native
from .native import VcrHipError, f32p, ptr
from .score import f64p, i32p

MAX_N = 131072
MAX_SPLITS = 128
MAX_K = 62                                                 # the kNN's limit: nb_neighbors <= MAX_K + 1


class StatArgs(native._Sized):
    _fields_ = [("struct_bytes", C.c_uint32), ("xyz4", f32p), ("idx", i32p), ("B", C.c_int), ("N", C.c_int), ("k", C.c_int),
                ("std_ratio", C.c_float), ("points", f32p), ("count", i32p), ("index", i32p), ("mean_dist", f32p),
                ("valid", i32p), ("stats", f64p)]


class RadiusArgs(native._Sized):
    _fields_ = [("struct_bytes", C.c_uint32), ("xyz", f32p), ("B", C.c_int), ("N", C.c_int), ("radius", C.c_float),
                ("nb_points", C.c_int), ("points", f32p), ("count", i32p), ("index", i32p), ("neighbours", i32p),
                ("variant", C.c_int)]


STRUCTS = {"vcr_outlier_stat_args": StatArgs, "vcr_outlier_radius_args": RadiusArgs}

# name -> (restype, [argtypes]): the prototypes of include/vcr_hip_outlier.h (tests/test_outlier_cpu.py holds them to it); the
# statistical filter has no form to report
SIGNATURES = {**{n: s for n, s in extension.workspace_signatures("vcr_outlier_stat", StatArgs).items() if not n.endswith("_form")},
              **extension.workspace_signatures("vcr_outlier_radius", RadiusArgs)}

lib = extension.typed_lib(SIGNATURES)                      # native.lib() with this module's entry points typed (once)


def variant(splits: int = 0) -> int:
    """vcr_outlier_radius_args.variant that forces the scan's number of segments (VCR_NN_SCORE_VARIANT's encoding): 0 = the
    plan's."""
    return int(splits) << 8


def radius_form(B, N, cu_count=256, variant=0):
    """vcr_outlier_radius_form (host only with an explicit cu_count): (points per lane, segments of the scan, workspace bytes)
    vcr_outlier_radius_f32 would run [B,3,N] with on a device of cu_count compute units."""
    a = RadiusArgs(0x1000, B, N, 1.0, 0, 0x2000, 0x3000, None, None, variant)   # (never dereferenced on the host)
    return extension.form(lib(), "vcr_outlier_radius", a, cu_count)


def _integer(v):
    """v as an int; None if it is not an integer (a float is none)."""
    try:
        return operator.index(v)
    except TypeError:
        return None


def _on_device(api, x):
    if not x.is_cuda:
        raise VcrHipError(f"{api} runs on the MI355X HIP path only; move the cloud to cuda (there is no CPU fallback by design)")


@native._guarded
def stat_filter(xyz4, idx, std_ratio, want_trace=True, guard=0, prefill=None):
    """vcr_outlier_stat_f32 on xyz4 [B,N,4] rows (native.to_rows4) and idx int32 [B,N,k] (native.knn on those rows) -> dict of
    points float32 [B,3,N] (the kept points in ascending index order, NaN behind them), count int32 [B], index int32 [B,N]
    (-1 behind the kept) and, with want_trace, mean_dist float32 [B,N], valid int32 [B] and stats float64 [B,3] (mu, sigma,
    thr).  guard / prefill (tests): as voxel.voxel_grid's -- the buffers come back under "_raw"."""
    api = "remove_statistical_outlier"
    if not (torch.is_tensor(xyz4) and xyz4.dim() == 3 and xyz4.shape[2] == 4 and xyz4.dtype == torch.float32):
        raise VcrHipError(f"{api}: xyz4 must be float32 [B, N, 4] rows")
    B, N, _ = xyz4.shape
    if not (torch.is_tensor(idx) and idx.dtype == torch.int32 and idx.dim() == 3 and tuple(idx.shape[:2]) == (B, N)):
        raise VcrHipError(f"{api}: idx must be int32 [B, N, k] with B, N = {B}, {N}")
    _on_device(api, xyz4)
    std_ratio = float(std_ratio)
    if not (math.isfinite(std_ratio) and std_ratio >= 0.0):
        raise VcrHipError(f"{api}: std_ratio must be finite and >= 0, got {std_ratio}")
    k = idx.shape[2]
    dev = native.same_device(xyz4, idx)
    xyz4, idx = xyz4.contiguous(), idx.contiguous()
    out, raw = extension.outputs(dev, guard, prefill)
    o = {"points": out("points", B * 3 * N, torch.float32).view(B, 3, N), "count": out("count", B, torch.int32),
         "index": out("index", B * N, torch.int32).view(B, N)}
    if want_trace:
        o["mean_dist"] = out("mean_dist", B * N, torch.float32).view(B, N)
        o["valid"] = out("valid", B, torch.int32)
        o["stats"] = out("stats", B * 3, torch.float64).view(B, 3)
    a = StatArgs(ptr(xyz4), ptr(idx), B, N, k, std_ratio, ptr(o["points"]), ptr(o["count"]), ptr(o["index"]),
                 ptr(o.get("mean_dist")), ptr(o.get("valid")), ptr(o.get("stats")))
    extension.call_with_workspace(lib(), "vcr_outlier_stat", a, dev, prefill)
    if guard or prefill is not None:
        o["_raw"] = raw
    return o


@native._guarded
def radius_filter(xyz, radius, nb_points, variant=0, want_trace=True, guard=0, prefill=None):
    """vcr_outlier_radius_f32 on xyz [B,3,N] (device, fp32) -> dict of points float32 [B,3,N], count int32 [B], index int32
    [B,N] as stat_filter's and, with want_trace, neighbours int32 [B,N]: the points within radius of every point, itself
    included.  guard / prefill (tests): as voxel.voxel_grid's."""
    api = "remove_radius_outlier"
    extension.check_cloud(api, "xyz", xyz)
    _on_device(api, xyz)
    radius = float(radius)
    if not (math.isfinite(radius) and radius > 0.0):
        raise VcrHipError(f"{api}: radius must be finite and > 0, got {radius}")
    if _integer(nb_points) is None or nb_points < 0:
        raise VcrHipError(f"{api}: nb_points must be an integer >= 0, got {nb_points}")
    dev = xyz.device
    B, _, N = xyz.shape
    xyz = xyz.contiguous().float()
    out, raw = extension.outputs(dev, guard, prefill)
    o = {"points": out("points", B * 3 * N, torch.float32).view(B, 3, N), "count": out("count", B, torch.int32),
         "index": out("index", B * N, torch.int32).view(B, N)}
    if want_trace:
        o["neighbours"] = out("neighbours", B * N, torch.int32).view(B, N)
    a = RadiusArgs(ptr(xyz), B, N, radius, int(nb_points), ptr(o["points"]), ptr(o["count"]), ptr(o["index"]),
                   ptr(o.get("neighbours")), int(variant))
    extension.call_with_workspace(lib(), "vcr_outlier_radius", a, dev, prefill)
    if guard or prefill is not None:
        o["_raw"] = raw
    return o


def remove_statistical_outlier(xyz, nb_neighbors=20, std_ratio=2.0, search="knn"):
    """xyz [B,3,N] (device tensor, up to 131 072 points a cloud) without the points whose mean distance to their nb_neighbors
    nearest points (the point itself among them, as Open3D counts) lies more than std_ratio standard deviations above the
    cloud's mean of those distances: Open3D's remove_statistical_outlier, in fp64 on the device.  A point AT the threshold is
    kept (Open3D drops it; a lattice would lose every point), and so is a point among its own copies (mean distance 0).
    2 <= nb_neighbors <= 63 and nb_neighbors <= N.  Returns (points, count, index) without a host synchronisation:
      points  float32 [B,3,N]  cloud b's count[b] kept points in ascending index order, NaN behind them
      count   int32 [B]
      index   int32 [B,N]      the kept points' indices, -1 behind them
    ``voxel.unpad(points, count)`` cuts the clouds to their sizes.  A point with a NaN or infinite coordinate is dropped and
    does not enter the statistics.
    The neighbours are the library's kNN (native.knn on the points' rows, ties broken exactly), whose distance is the expansion
    2 x.y - |x|^2 - |y|^2 in fp32: for a cloud far from the origin relative to its spacing it cancels, and the neighbours are
    then not the nearest.  Centre such a cloud first (the filter does not change under a translation):
    ``vcrnet_amd.centred(xyz)`` returns xyz - c and the centre c it took.
    search: "knn" is that search.  "grid" takes the nb_neighbors - 1 other points from ``search_knn``
    instead: distances of differences, so no centring is needed, and the point itself excluded by its index.  The faster one
    for large clouds."""
    api = "remove_statistical_outlier"
    extension.check_cloud(api, "xyz", xyz)
    grid.check_search(api, search)
    _on_device(api, xyz)
    if _integer(nb_neighbors) is None or not 2 <= nb_neighbors <= MAX_K + 1:
        raise VcrHipError(f"{api}: nb_neighbors must be an integer in [2, {MAX_K + 1}], got {nb_neighbors}")
    N = xyz.shape[2]
    if nb_neighbors > N:
        raise VcrHipError(f"{api}: nb_neighbors = {nb_neighbors} needs at least as many points, got N = {N}")
    std_ratio = float(std_ratio)
    if not (math.isfinite(std_ratio) and std_ratio >= 0.0):
        raise VcrHipError(f"{api}: std_ratio must be finite and >= 0, got {std_ratio}")
    xyz4 = native.to_rows4(xyz)
    k = int(nb_neighbors) - 1
    idx = native.knn(xyz4, None, k) if search == "knn" else grid.search_knn(xyz, k)
    o = stat_filter(xyz4, idx, std_ratio, want_trace=False)
    return o["points"], o["count"], o["index"]


def remove_radius_outlier(xyz, nb_points, radius, search="scan"):
    """xyz [B,3,N] (device tensor, up to 131 072 points a cloud) without the points that have no more than nb_points points
    (themselves included, as Open3D counts) within radius: Open3D's remove_radius_outlier.  The distances are differences
    (dx^2 + dy^2 + dz^2 in fp32, a point ON the sphere counts), so a cloud far from the origin needs no centring.  Returns
    (points, count, index) as remove_statistical_outlier, without a host synchronisation; ``voxel.unpad(points, count)`` cuts
    the clouds to their sizes.  A point with a NaN or infinite coordinate is dropped and counted by nobody.
    search: "scan" compares every point with every point.  "grid" counts on the cloud's uniform grid instead (DESIGN.md section
    4.22: cells of the radius' edge, 27 of them a point where the cloud is no denser than its grid) and returns the same bits;
    it needs a radius whose fp32 square is finite."""
    if search not in ("scan", "grid"):
        raise VcrHipError(f'remove_radius_outlier: search must be "scan" or "grid", got {search!r}')
    if search == "grid":
        from . import radius as radius_search               # (it imports this module: resolved on first use)
        o = radius_search.radius_filter_grid(xyz, radius, nb_points, want_trace=False)
    else:
        o = radius_filter(xyz, radius, nb_points, want_trace=False)
    return o["points"], o["count"], o["index"]


def filter_by(spec, xyz):
    """register_sampled's ``outlier=`` on one batch: ("statistical", nb_neighbors, std_ratio) or ("radius", nb_points, radius)
    -> (points, count, index).  The radius filter takes an optional fourth element, "grid": its ``search=``."""
    ok = isinstance(spec, (tuple, list)) and len(spec) >= 1 and spec[0] in ("statistical", "radius")
    if not (ok and (len(spec) == 3 or (spec[0] == "radius" and len(spec) == 4 and spec[3] == "grid"))):
        raise VcrHipError('register_sampled: outlier must be ("statistical", nb_neighbors, std_ratio) or '
                          f'("radius", nb_points, radius), got {spec!r}')
    if spec[0] == "statistical":
        return remove_statistical_outlier(xyz, spec[1], spec[2])
    return remove_radius_outlier(xyz, spec[1], spec[2], *spec[3:])
