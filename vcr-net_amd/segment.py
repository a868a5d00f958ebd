"""ctypes binding of include/segment/vcr_hip_segment.h and the Python API on top of it: the dominant
plane of a cloud by RANSAC -- vcr_plane_ransac_f32 and its host-only vcr_plane_ransac_form -- and vcr_plane_split_f32, which
compacts a cloud into the plane's points and the rest through the outlier filters' tail.  ``segment_plane`` is Open3D's call of
that name, ``split_by_plane`` its two ``select_by_index`` in one, ``segment_planes`` peels planes one after the other.

Like ``dbscan``, the header extends include/vcr_hip.h without touching it and this module keeps its own STRUCTS / SIGNATURES
maps, applied once to ``native.lib()`` on first use.  No CPU fallback, as everywhere."""
from __future__ import annotations

import ctypes as C
import math
import torch

from . import extension, native
from .native import VcrHipError, f32p, ptr
from .score import i32p

MAX_N = 131072                                             # VCR_PLANE_MAX_N
MAX_TRIALS = 1 << 20                                       # VCR_PLANE_MAX_TRIALS
FORMS = {"trial": 1, "point": 2}                           # VCR_PLANE_TRIAL / VCR_PLANE_POINT: what ``variant`` forces
MAX_SPLITS = 512                                           # VCR_PLANE_MAX_SPLITS
POINT_PER_LANE = 4                                         # VCR_PLANE_POINT_PER_LANE
POINT_MIN_N = 8192                                         # VCR_PLANE_POINT_MIN_N: the POINT form from this many points a cloud
POINT_MIN_T = 4096                                         # VCR_PLANE_POINT_MIN_T: ... or this many trials
FILL = 4                                                   # VCR_PLANE_FILL
TRIAL_MIN_RANGE = 64                                       # VCR_PLANE_TRIAL_MIN_RANGE
_INT32_LIMIT = 1 << 31

f64p = C.c_void_p


class PlaneRansacArgs(native._Sized):
    _fields_ = [("struct_bytes", C.c_uint32), ("xyz", f32p), ("mask", i32p), ("B", C.c_int), ("N", C.c_int),
                ("distance_threshold", C.c_float), ("ransac_n", C.c_int), ("trials", C.c_int), ("seed", C.c_uint32),
                ("variant", C.c_int), ("plane", f32p), ("inlier", i32p), ("count", i32p), ("point", f32p), ("best_trial", i32p),
                ("candidates", i32p), ("trial_status", i32p), ("trial_picks", i32p), ("trial_plane", f32p), ("trial_count", i32p),
                ("refit_sums", f64p)]


class PlaneSplitArgs(native._Sized):
    _fields_ = [("struct_bytes", C.c_uint32), ("xyz", f32p), ("inlier", i32p), ("B", C.c_int), ("N", C.c_int),
                ("plane_points", f32p), ("plane_count", i32p), ("rest_points", f32p), ("rest_count", i32p), ("plane_index", i32p),
                ("rest_index", i32p)]


STRUCTS = {"vcr_plane_ransac_args": PlaneRansacArgs, "vcr_plane_split_args": PlaneSplitArgs}

# name -> (restype, [argtypes]): the prototypes of include/segment/vcr_hip_segment.h (tests/test_segment_cpu.py holds them to it);
# the split has no form to report
SIGNATURES = {**extension.workspace_signatures("vcr_plane_ransac", PlaneRansacArgs),
              **{n: s for n, s in extension.workspace_signatures("vcr_plane_split", PlaneSplitArgs).items()
                 if not n.endswith("_form")}}

lib = extension.typed_lib(SIGNATURES)                      # native.lib() with this module's entry points typed (once)


def variant_code(api, variant):
    """0 (the plan), "trial" / "point", or (form, splits) -> the header's form | splits << 8."""
    if isinstance(variant, tuple) and len(variant) == 2:
        form, splits = variant
    else:
        form, splits = variant, 0
    if form in FORMS:
        form = FORMS[form]
    ok = not isinstance(form, bool) and form in (0, 1, 2) and isinstance(splits, int) and not isinstance(splits, bool)
    if not ok or not 0 <= splits <= MAX_SPLITS or (form == 0 and splits != 0):
        raise VcrHipError(f'{api}: variant must be 0 (the plan), "trial", "point" or (form, splits) with splits in '
                          f"[0, {MAX_SPLITS}], got {variant!r}")
    return int(form) | splits << 8


def form(B, N, trials, cu_count=256, variant=0):
    """vcr_plane_ransac_form and _workspace_bytes (host only): (the count launch's form, its splits, workspace bytes)."""
    a = PlaneRansacArgs(0x1000, None, B, N, 0.0, 3, trials, 0, variant_code("segment.form", variant), 0x2000, 0x3000, 0x4000)
    return extension.form(lib(), "vcr_plane_ransac", a, cu_count)     # (the pointers are never dereferenced on the host)


def _threshold(api, v):
    if isinstance(v, bool) or not isinstance(v, (int, float)) or not (v >= 0) or math.isinf(v) or math.isinf(C.c_float(v).value):
        raise VcrHipError(f"{api}: distance_threshold must be finite and >= 0, got {v!r}")
    return float(v)


def _cloud(api, xyz):
    extension.check_cloud(api, "xyz", xyz)
    B, _, N = xyz.shape
    if not 1 <= N <= MAX_N:
        raise VcrHipError(f"{api}: a cloud must have 1 ... {MAX_N} points, got {N}")
    if B < 1 or B * N >= _INT32_LIMIT:
        raise VcrHipError(f"{api}: B must be at least 1 and B * N below 2^31, got B = {B}, N = {N}")
    return B, N


def _flags(api, name, t, B, N):
    if not (torch.is_tensor(t) and t.dtype == torch.int32 and tuple(t.shape) == (B, N)):
        raise VcrHipError(f"{api}: {name} must be int32 [B, N] with B, N = {B}, {N}")


def _on_device(api, xyz):
    if not xyz.is_cuda:
        raise VcrHipError(f"{api} runs on the MI355X HIP path only; move the cloud to cuda (there is no CPU fallback by design)")


@native._guarded
def plane_ransac(xyz, distance_threshold, ransac_n=3, num_iterations=1000, seed=0, mask=None, want_trials=False, variant=0,
                 guard=0, prefill=None, api="segment.plane_ransac"):
    """vcr_plane_ransac_f32 on xyz float32 [B,3,N] -> dict of plane float32 [B,4], inlier int32 [B,N], count int32 [B], point
    float32 [B,3], best_trial int32 [B], candidates int32 [B], refit_sums float64 [B,9] and, with want_trials, trial_status
    int32 [B,T], trial_picks int32 [B,T,3], trial_plane float32 [B,T,8] and trial_count int32 [B,T] (the header's layouts).
    variant: 0 for the plan, "trial" / "point" to force the count's form, (form, splits) to force both.  guard / prefill (tests):
    as voxel.voxel_grid's -- the buffers come back under "_raw", and the workspace is prefilled too."""
    B, N = _cloud(api, xyz)
    thr = _threshold(api, distance_threshold)
    if isinstance(ransac_n, bool) or ransac_n != 3:
        raise VcrHipError(f"{api}: ransac_n must be 3 (the plane through three points), got {ransac_n!r}")
    T = num_iterations
    if isinstance(T, bool) or not isinstance(T, int) or not 1 <= T <= MAX_TRIALS:
        raise VcrHipError(f"{api}: num_iterations must be an integer in [1, {MAX_TRIALS}], got {T!r}")
    if B * T >= 1 << 29:
        raise VcrHipError(f"{api}: B * num_iterations must be below 2^29, got B = {B}, num_iterations = {T}")
    if isinstance(seed, bool) or not isinstance(seed, int) or not 0 <= seed < 1 << 32:
        raise VcrHipError(f"{api}: seed must be an integer in [0, 2^32), got {seed!r}")
    if mask is not None:
        _flags(api, "mask", mask, B, N)
    v = variant_code(api, variant)
    _on_device(api, xyz)
    dev = native.same_device(xyz, mask)
    xyz = xyz.contiguous().float()
    mask = None if mask is None else mask.contiguous()
    out, raw = extension.outputs(dev, guard, prefill)
    o = {"plane": out("plane", B * 4, torch.float32).view(B, 4), "inlier": out("inlier", B * N, torch.int32).view(B, N),
         "count": out("count", B, torch.int32), "point": out("point", B * 3, torch.float32).view(B, 3),
         "best_trial": out("best_trial", B, torch.int32), "candidates": out("candidates", B, torch.int32),
         "refit_sums": out("refit_sums", B * 9, torch.float64).view(B, 9)}
    if want_trials:
        o["trial_status"] = out("trial_status", B * T, torch.int32).view(B, T)
        o["trial_picks"] = out("trial_picks", B * T * 3, torch.int32).view(B, T, 3)
        o["trial_plane"] = out("trial_plane", B * T * 8, torch.float32).view(B, T, 8)
        o["trial_count"] = out("trial_count", B * T, torch.int32).view(B, T)
    a = PlaneRansacArgs(ptr(xyz), ptr(mask), B, N, thr, 3, T, seed, v, ptr(o["plane"]), ptr(o["inlier"]), ptr(o["count"]),
                        ptr(o["point"]), ptr(o["best_trial"]), ptr(o["candidates"]), ptr(o.get("trial_status")),
                        ptr(o.get("trial_picks")), ptr(o.get("trial_plane")), ptr(o.get("trial_count")), ptr(o["refit_sums"]))
    extension.call_with_workspace(lib(), "vcr_plane_ransac", a, dev, prefill)
    if guard or prefill is not None:
        o["_raw"] = raw
    return o


@native._guarded
def split_rows(xyz, inlier, want_index=True, guard=0, prefill=None):
    """vcr_plane_split_f32 on xyz float32 [B,3,N] and inlier int32 [B,N] -> dict of plane_points / rest_points float32 [B,3,N],
    plane_count / rest_count int32 [B] and plane_index / rest_index int32 [B,N], as outlier.radius_filter's."""
    api = "split_by_plane"
    B, N = _cloud(api, xyz)
    _flags(api, "inlier", inlier, B, N)
    _on_device(api, xyz)
    dev = native.same_device(xyz, inlier)
    xyz, inlier = xyz.contiguous().float(), inlier.contiguous()
    out, raw = extension.outputs(dev, guard, prefill)
    o = {}
    for side in ("plane", "rest"):
        o[side + "_points"] = out(side + "_points", B * 3 * N, torch.float32).view(B, 3, N)
        o[side + "_count"] = out(side + "_count", B, torch.int32)
        if want_index:
            o[side + "_index"] = out(side + "_index", B * N, torch.int32).view(B, N)
    a = PlaneSplitArgs(ptr(xyz), ptr(inlier), B, N, ptr(o["plane_points"]), ptr(o["plane_count"]), ptr(o["rest_points"]),
                       ptr(o["rest_count"]), ptr(o.get("plane_index")), ptr(o.get("rest_index")))
    extension.call_with_workspace(lib(), "vcr_plane_split", a, dev, prefill)
    if guard or prefill is not None:
        o["_raw"] = raw
    return o


def segment_plane(xyz, distance_threshold, ransac_n=3, num_iterations=1000, seed=0, mask=None):
    """The dominant plane of every cloud of xyz [B,3,N] (device tensor, up to 131 072 points a cloud) by RANSAC: Open3D's
    segment_plane(distance_threshold, ransac_n=3, num_iterations) with probability = 1 (all trials run).  Returns
      plane   float32 [B,4]  (a, b, c, d) with a x + b y + c z + d = 0 and (a, b, c) of unit length: the least-squares plane of
                             the best trial's inliers, as Open3D returns it
      inlier  int32 [B,N]    1 for a point within distance_threshold of the best trial's plane, else 0
      count   int32 [B]      their number
    A trial draws three points by the hash of (seed, trial) -- ``ransac_correspondences``' draws --, the best trial is the one
    with the most inliers, the lowest number among equals: the result is a function of the cloud and the seed alone, the same
    bits in every batch.  Distances are taken from coordinate differences in fp32, so a cloud far from the origin needs no
    centring.  A point with a NaN or infinite coordinate, or with mask 0 (mask: optional int32 [B,N]), is neither drawn nor
    counted.  A cloud without three candidates that span a plane comes back with a NaN plane and count 0.  No host
    synchronisation."""
    o = plane_ransac(xyz, distance_threshold, ransac_n, num_iterations, seed, mask, api="segment_plane")
    return o["plane"], o["inlier"], o["count"]


def split_by_plane(xyz, inlier):
    """xyz [B,3,N] cut along ``segment_plane``'s inlier flags: ((points, count, index), (points, count, index)), the plane's
    points and all the others, each as ``remove_radius_outlier`` returns them -- compacted in ascending index order, NaN (index
    -1) behind count, without a host synchronisation; ``voxel.unpad(points, count)`` cuts the clouds to their sizes.  Open3D's
    select_by_index(inliers) and select_by_index(inliers, invert=True) in one call."""
    o = split_rows(xyz, inlier)
    return ((o["plane_points"], o["plane_count"], o["plane_index"]), (o["rest_points"], o["rest_count"], o["rest_index"]))


def segment_planes(xyz, distance_threshold, max_planes, min_inliers, num_iterations=1000, seed=0):
    """Up to max_planes planes of every cloud, one after the other: round k runs ``segment_plane`` with seed + k on the points no
    earlier plane took.  Returns (labels int32 [B,N]: the plane a point belongs to, -1 for none; planes float32 [B,K,4]; counts
    int32 [B,K]).  A cloud whose k-th plane has fewer than min_inliers inliers stops there: that row of planes and the rows
    behind it are NaN, their counts 0, and its remaining points stay -1; the other clouds go on.  K calls with torch plumbing
    on device tensors between them: no host synchronisation."""
    api = "segment_planes"
    B, N = _cloud(api, xyz)
    for name, v, low in (("max_planes", max_planes, 1), ("min_inliers", min_inliers, 0)):
        if isinstance(v, bool) or not isinstance(v, int) or v < low:
            raise VcrHipError(f"{api}: {name} must be an integer >= {low}, got {v!r}")
    if isinstance(seed, bool) or not isinstance(seed, int) or not 0 <= seed or seed + max_planes > 1 << 32:
        raise VcrHipError(f"{api}: seed must be an integer >= 0 with seed + max_planes <= 2^32, got {seed!r}")
    _threshold(api, distance_threshold)
    _on_device(api, xyz)
    K = max_planes
    labels = torch.full((B, N), -1, dtype=torch.int32, device=xyz.device)
    planes = torch.full((B, K, 4), float("nan"), dtype=torch.float32, device=xyz.device)
    counts = torch.zeros((B, K), dtype=torch.int32, device=xyz.device)
    live = torch.ones((B, 1), dtype=torch.bool, device=xyz.device)
    for k in range(K):
        mask = ((labels < 0) & live).to(torch.int32)
        o = plane_ransac(xyz, distance_threshold, 3, num_iterations, seed + k, mask, api=api)
        live = live & (o["count"] >= max(min_inliers, 1)).view(B, 1)
        take = live & (o["inlier"] > 0)
        labels = torch.where(take, torch.full_like(labels, k), labels)
        planes[:, k] = torch.where(live, o["plane"], planes[:, k])
        counts[:, k] = torch.where(live.view(B), o["count"], counts[:, k])
    return labels, planes, counts
