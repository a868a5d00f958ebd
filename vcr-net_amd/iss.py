"""ctypes binding of include/keypoint/vcr_hip_iss.h and the Python API on top of it: keypoints by
Intrinsic Shape Signatures on the device, over the ragged CSR rows ``search_radius`` returns -- vcr_rows_iss_saliency_f32 (the
eigenvalue test of every neighbourhood's covariance), vcr_rows_iss_nms_f32 (the suppression of every point a neighbour beats) with
its host-only vcr_rows_iss_form, and vcr_iss_select_f32, which compacts a cloud to its keypoints through the outlier filters' tail.
``compute_iss_keypoints`` is Open3D's call of that name, ``model_resolution`` its ComputeModelResolution.

Like ``rows`` and ``dbscan``, the header extends include/vcr_hip.h without touching it and this module keeps its own STRUCTS /
SIGNATURES maps, applied once to ``native.lib()`` on first use.  No CPU fallback, as everywhere."""
from __future__ import annotations

import ctypes as C
import math
import torch

from . import extension, native, radius
from .native import VcrHipError, f32p, ptr
from .score import i32p

MAX_N = 131072
FORMS = {"lane": 1, "wave": 2}                             # VCR_ISS_LANE / VCR_ISS_WAVE: what ``variant`` forces
WAVE_NMS = 131072                                          # VCR_ISS_WAVE_NMS: the row length the suppression's wave form starts at
NOT_SERVED = -2                                            # VCR_ISS_NOT_SERVED
_INT32_LIMIT = 1 << 31

i64p = C.c_void_p
f64p = C.c_void_p


class RowsIssSaliencyArgs(native._Sized):
    _fields_ = [("struct_bytes", C.c_uint32), ("xyz4", f32p), ("idx", i32p), ("row_start", i64p), ("total", i64p), ("B", C.c_int),
                ("N", C.c_int), ("capacity", C.c_int), ("min_neighbors", C.c_int), ("gamma_21", C.c_double),
                ("gamma_32", C.c_double), ("saliency", f64p), ("eigen", f64p)]


class RowsIssNmsArgs(native._Sized):
    _fields_ = [("struct_bytes", C.c_uint32), ("idx", i32p), ("row_start", i64p), ("total", i64p), ("saliency", f64p),
                ("d2", f32p), ("B", C.c_int), ("N", C.c_int), ("capacity", C.c_int), ("min_neighbors", C.c_int),
                ("r2_nm", C.c_float), ("variant", C.c_int), ("keypoint", i32p)]


class IssSelectArgs(native._Sized):
    _fields_ = [("struct_bytes", C.c_uint32), ("xyz", f32p), ("keypoint", i32p), ("B", C.c_int), ("N", C.c_int), ("points", f32p),
                ("count", i32p), ("index", i32p)]


STRUCTS = {"vcr_rows_iss_saliency_args": RowsIssSaliencyArgs, "vcr_rows_iss_nms_args": RowsIssNmsArgs,
           "vcr_iss_select_args": IssSelectArgs}

_int, _intp = C.c_int, C.POINTER(C.c_int)

# name -> (restype, [argtypes]): the prototypes of include/keypoint/vcr_hip_iss.h (tests/test_iss_cpu.py holds them to it)
SIGNATURES = {"vcr_rows_iss_saliency_f32": (_int, [C.POINTER(RowsIssSaliencyArgs), C.c_void_p]),
              "vcr_rows_iss_nms_f32": (_int, [C.POINTER(RowsIssNmsArgs), C.c_void_p]),
              "vcr_rows_iss_form": (_int, [_int, _int, _int, _int, _int, _intp]),
              "vcr_iss_select_workspace_bytes": (C.c_size_t, [C.POINTER(IssSelectArgs), _int]),
              "vcr_iss_select_f32": (_int, [C.POINTER(IssSelectArgs), C.c_void_p, C.c_size_t, C.c_void_p])}

lib = extension.typed_lib(SIGNATURES)                      # native.lib() with this module's entry points typed (once)


def form(B, N, capacity, cu_count=256, variant=0):
    """vcr_rows_iss_form (host only): the suppression's form, 1 = a lane a row, 2 = a wave a row."""
    f = C.c_int(0)
    native.check(lib().vcr_rows_iss_form(B, N, capacity, cu_count, variant, C.byref(f)), "vcr_rows_iss_form")
    return f.value


def check_min_neighbors(api, min_neighbors):
    if isinstance(min_neighbors, bool) or not isinstance(min_neighbors, int) or min_neighbors < 1:
        raise VcrHipError(f"{api}: min_neighbors must be an integer >= 1, got {min_neighbors!r}")
    return min_neighbors


def check_gamma(api, name, gamma):
    try:
        g = float(gamma)
    except (TypeError, ValueError):
        g = float("nan")
    if isinstance(gamma, bool) or not (math.isfinite(g) and g > 0.0):
        raise VcrHipError(f"{api}: {name} must be finite and > 0, got {gamma!r}")
    return g


def check_arguments(api, salient_radius=None, non_max_radius=None, gamma_21=0.975, gamma_32=0.975, min_neighbors=5,
                    border_radius=None, normal_radius=None, border_angle=90.0, **_):
    """What compute_iss_keypoints asks of its numbers, under the caller's name -> (gamma_21, gamma_32) as floats."""
    if border_radius is None and normal_radius is not None:
        raise VcrHipError(f"{api}: normal_radius belongs to border_radius, which is None")
    if border_radius is not None:
        from .border import check_threshold
        check_threshold(api, "border_angle", border_angle)
    for name, r in (("salient_radius", salient_radius), ("non_max_radius", non_max_radius), ("border_radius", border_radius),
                    ("normal_radius", normal_radius)):
        if r is not None:
            try:
                radius._radius(api, r)
            except VcrHipError as e:
                raise VcrHipError(str(e).replace("radius must", name + " must", 1)) from None
    g = check_gamma(api, "gamma_21", gamma_21), check_gamma(api, "gamma_32", gamma_32)
    check_min_neighbors(api, min_neighbors)
    return g


def _variant(api, variant):
    if variant in FORMS:
        return FORMS[variant]
    if isinstance(variant, bool) or variant not in (0, 1, 2):
        raise VcrHipError(f'{api}: variant must be 0 (the plan), "lane" or "wave", got {variant!r}')
    return int(variant)


def _rows(api, idx, row_start, total, B, N):
    """The CSR triple of B clouds of N points -> capacity."""
    if not (torch.is_tensor(idx) and idx.dtype == torch.int32 and idx.dim() == 2 and idx.shape[0] == B):
        raise VcrHipError(f"{api}: idx must be int32 [B, capacity] with B = {B}")
    capacity = idx.shape[1]
    if B * N >= _INT32_LIMIT or B * capacity >= _INT32_LIMIT:
        raise VcrHipError(f"{api}: B * N and B * capacity must be below 2^31, got B = {B}, N = {N}, capacity = {capacity}")
    if not (torch.is_tensor(row_start) and row_start.dtype == torch.int64 and tuple(row_start.shape) == (B, N + 1)):
        raise VcrHipError(f"{api}: row_start must be int64 [B, N + 1] with B, N = {B}, {N}")
    if not (torch.is_tensor(total) and total.dtype == torch.int64 and tuple(total.shape) == (B,)):
        raise VcrHipError(f"{api}: total must be int64 [B] with B = {B}")
    return capacity


@native._guarded
def saliency_rows(xyz4, idx, row_start, total, gamma_21=0.975, gamma_32=0.975, min_neighbors=5, want_eigen=False, guard=0,
                  prefill=None):
    """vcr_rows_iss_saliency_f32 on xyz4 [B,N,4] rows (native.to_rows4) and the CSR rows idx int32 [B,capacity], row_start int64
    [B,N+1], total int64 [B] (``search_radius`` on the same cloud, or any caller's) -> dict of saliency float64 [B,N] (the
    smallest eigenvalue where the point passes both ratio tests and has min_neighbors points, itself included; 0 elsewhere; NaN
    over a cloud that is not served) and, with want_eigen, eigen float64 [B,N,3].
    guard / prefill (tests): as voxel.voxel_grid's -- the buffers come back under "_raw"."""
    api = "iss.saliency_rows"
    if not (torch.is_tensor(xyz4) and xyz4.dim() == 3 and xyz4.shape[2] == 4 and xyz4.dtype == torch.float32
            and xyz4.shape[0] >= 1):
        raise VcrHipError(f"{api}: xyz4 must be float32 [B, N, 4] rows")
    B, N, _ = xyz4.shape
    if not 1 <= N <= MAX_N:
        raise VcrHipError(f"{api}: a cloud must have 1 ... {MAX_N} points, got {N}")
    capacity = _rows(api, idx, row_start, total, B, N)
    g21, g32 = check_gamma(api, "gamma_21", gamma_21), check_gamma(api, "gamma_32", gamma_32)
    check_min_neighbors(api, min_neighbors)
    dev = native.same_device(xyz4, idx, row_start, total)
    xyz4, idx, row_start, total = xyz4.contiguous(), idx.contiguous(), row_start.contiguous(), total.contiguous()
    given = ptr(idx) if B * capacity > 0 else None          # (an empty tensor has no address to give)
    xyz4_p = ptr(xyz4)
    out, raw = extension.outputs(dev, guard, prefill)
    o = {"saliency": out("saliency", B * N, torch.float64).view(B, N)}
    if want_eigen:
        o["eigen"] = out("eigen", B * N * 3, torch.float64).view(B, N, 3)
    a = RowsIssSaliencyArgs(xyz4_p, given, ptr(row_start), ptr(total), B, N, capacity, min_neighbors, g21, g32,
                            ptr(o["saliency"]), ptr(o.get("eigen")))
    native.check(lib().vcr_rows_iss_saliency_f32(C.byref(a), native.stream_ptr()), "vcr_rows_iss_saliency_f32")
    if guard or prefill is not None:
        o["_raw"] = raw
    return o


@native._guarded
def nms_rows(idx, row_start, total, saliency, min_neighbors=5, d2=None, r2_nm=None, variant=0, guard=0, prefill=None):
    """vcr_rows_iss_nms_f32 on the CSR rows and saliency float64 [B,N] -> dict of keypoint int32 [B,N]: 1 where the point's
    saliency is above 0, its used entries and itself are min_neighbors at least and none of them has a larger saliency; 0
    elsewhere; -2 over a cloud that is not served or holds a NaN saliency.  d2 float32 [B,capacity] with r2_nm (a float, compared
    in fp32): a row's used entries are its leading ones with d2 <= r2_nm; without them all of the row.
    variant: 0 for the plan's form, "lane" or "wave" to force one.  guard / prefill: as above."""
    api = "iss.nms_rows"
    if not (torch.is_tensor(saliency) and saliency.dtype == torch.float64 and saliency.dim() == 2 and saliency.shape[0] >= 1):
        raise VcrHipError(f"{api}: saliency must be float64 [B, N]")
    B, N = saliency.shape
    if not 1 <= N <= MAX_N:
        raise VcrHipError(f"{api}: a cloud must have 1 ... {MAX_N} points, got {N}")
    capacity = _rows(api, idx, row_start, total, B, N)
    check_min_neighbors(api, min_neighbors)
    if (d2 is None) != (r2_nm is None):
        raise VcrHipError(f"{api}: give both d2 and r2_nm, or neither (the whole row)")
    r2 = 0.0
    if d2 is not None:
        if not (torch.is_tensor(d2) and d2.dtype == torch.float32 and tuple(d2.shape) == (B, capacity)):
            raise VcrHipError(f"{api}: d2 must be None or float32 [B, capacity] with B, capacity = {B}, {capacity}")
        try:
            r2 = float(r2_nm)
        except (TypeError, ValueError):
            r2 = float("nan")
        if not r2 >= 0.0:
            raise VcrHipError(f"{api}: r2_nm must be >= 0, got {r2_nm!r}")
    v = _variant(api, variant)
    dev = native.same_device(idx, row_start, total, saliency, d2)
    idx, row_start, total, saliency = idx.contiguous(), row_start.contiguous(), total.contiguous(), saliency.contiguous()
    d2 = None if d2 is None else d2.contiguous()
    has = B * capacity > 0                                  # (an empty tensor has no address to give)
    idx_p, d2_p = (ptr(idx) if has else None), (ptr(d2) if has and d2 is not None else None)
    sal_p = ptr(saliency)
    out, raw = extension.outputs(dev, guard, prefill)
    o = {"keypoint": out("keypoint", B * N, torch.int32).view(B, N)}
    a = RowsIssNmsArgs(idx_p, ptr(row_start), ptr(total), sal_p, d2_p, B, N, capacity, min_neighbors, r2, v, ptr(o["keypoint"]))
    native.check(lib().vcr_rows_iss_nms_f32(C.byref(a), native.stream_ptr()), "vcr_rows_iss_nms_f32")
    if guard or prefill is not None:
        o["_raw"] = raw
    return o


@native._guarded
def select(xyz, keypoint, want_index=True, guard=0, prefill=None):
    """vcr_iss_select_f32 on xyz float32 [B,3,N] and keypoint int32 [B,N] (``nms_rows``) -> dict of points float32 [B,3,N], count
    int32 [B] and index int32 [B,N], as outlier.radius_filter's: the points whose flag is above 0 in ascending index order."""
    api = "iss.select"
    extension.check_cloud(api, "xyz", xyz)
    B, _, N = xyz.shape
    if not (torch.is_tensor(keypoint) and keypoint.dtype == torch.int32 and tuple(keypoint.shape) == (B, N)):
        raise VcrHipError(f"{api}: keypoint must be int32 [B, N] with B, N = {B}, {N}")
    if not 1 <= N <= MAX_N:
        raise VcrHipError(f"{api}: a cloud must have 1 ... {MAX_N} points, got {N}")
    if B < 1 or B * N >= _INT32_LIMIT:
        raise VcrHipError(f"{api}: B must be at least 1 and B * N below 2^31, got B = {B}, N = {N}")
    if not xyz.is_cuda:
        raise VcrHipError(f"{api} runs on the MI355X HIP path only; move the cloud to cuda (there is no CPU fallback by design)")
    dev = native.same_device(xyz, keypoint)
    xyz, keypoint = xyz.contiguous().float(), keypoint.contiguous()
    out, raw = extension.outputs(dev, guard, prefill)
    o = {"points": out("points", B * 3 * N, torch.float32).view(B, 3, N), "count": out("count", B, torch.int32)}
    if want_index:
        o["index"] = out("index", B * N, torch.int32).view(B, N)
    a = IssSelectArgs(ptr(xyz), ptr(keypoint), B, N, ptr(o["points"]), ptr(o["count"]), ptr(o.get("index")))
    extension.call_with_workspace(lib(), "vcr_iss_select", a, dev, prefill)
    if guard or prefill is not None:
        o["_raw"] = raw
    return o


def model_resolution(xyz):
    """Open3D's ComputeModelResolution for every cloud of xyz [B,3,N] (device tensor, N >= 2): float64 [B] on the device, the
    mean over the cloud's finite points of the distance to their nearest other point -- sqrt of ``search_knn(xyz, 1)``'s d2
    widened to fp64.  No host synchronisation.  The sum is torch's: equal to numpy's to rounding, not to the bit."""
    api = "model_resolution"
    radius._cloud(api, xyz)
    if xyz.shape[2] < 2:
        raise VcrHipError(f"{api}: a nearest other point needs at least 2 points, got N = {xyz.shape[2]}")
    radius._on_device(api, xyz)
    from .grid import search_knn
    xyz = xyz.contiguous().float()
    _, d2 = search_knn(xyz, 1, want_d2=True)
    finite = torch.isfinite(xyz).all(dim=1)
    dist = torch.where(finite, d2[:, :, 0].double().sqrt(), torch.zeros((), dtype=torch.float64, device=xyz.device))
    return dist.sum(dim=1) / finite.sum(dim=1).double()


def _search(api, xyz, r, want_d2, capacity, cell):
    """search_radius with its refusals under this call's name."""
    try:
        return radius.search_radius(xyz, r, want_d2=want_d2, capacity=capacity, cell=cell)
    except VcrHipError as e:
        raise VcrHipError(str(e).replace("search_radius", api, 1)) from None


def _border_near(api, xyz, xyz4, searched, border_radius, normal_radius, border_angle, normals, capacity, cell):
    """PCL's border rule -> near int32 [B,N]: 1 where a boundary point lies within border_radius of the point, itself included.
    The boundary is ``border``'s at border_radius over ALL the points within it and its default of 3 points a neighbourhood.
    searched: None, or (radius, idx, row_start, total, d2) of a search already made: with normals given and border_radius within
    that radius, the three passes read the d2 prefix of those rows and nothing is searched."""
    from . import border, rows
    br, br2 = radius._radius(api, border_radius)
    thr = border.radians(border_angle)
    if normals is not None and searched is not None and br <= searched[0]:
        _, idx, row_start, total, d2 = searched
        flag, _ = border.boundary_rows(xyz4, normals, idx, row_start, total, 3, thr, d2=d2, r2=br2)
        return border.near_rows(flag, idx, row_start, total, d2=d2, r2=br2)["near"]
    idx, row_start, total = _search(api, xyz, br, False, capacity, cell)
    if normals is None:
        nr = br if normal_radius is None else float(normal_radius)
        over = (idx, row_start, total) if nr == br else _search(api, xyz, nr, False, capacity, cell)
        normals = rows.normals(xyz4, *over, want_curvature=False)[0]
    flag, _ = border.boundary_rows(xyz4, normals, idx, row_start, total, 3, thr)
    return border.near_rows(flag, idx, row_start, total)["near"]


def _without_border(sal, near):
    """The saliency with 0 where the point is near the boundary, NaN over a cloud whose boundary was not served (the suppression
    voids it)."""
    zero, nan = torch.zeros((), dtype=sal.dtype, device=sal.device), torch.full((), float("nan"), dtype=sal.dtype, device=sal.device)
    sal = torch.where(near > 0, zero, sal)
    return torch.where(near < 0, nan, sal)


def compute_iss_keypoints(xyz, salient_radius=None, non_max_radius=None, gamma_21=0.975, gamma_32=0.975, min_neighbors=5,
                          capacity=None, cell=None, want_flag=False, want_saliency=False, border_radius=None, normal_radius=None,
                          border_angle=90.0, normals=None):
    """ISS keypoints of every cloud of xyz [B,3,N] (device tensor, up to 131 072 points a cloud): Open3D's
    compute_iss_keypoints(salient_radius, non_max_radius, gamma_21, gamma_32, min_neighbors).  Returns (points, count, index) as
    ``remove_radius_outlier`` returns them -- the keypoints compacted in ascending index order, NaN / -1 behind count[b];
    ``voxel.unpad(points, count)`` cuts the clouds to their sizes -- then, where asked:
      flag      int32 [B,N]    1 for a keypoint, 0 for any other point, -2 over a cloud that was not served
      saliency  float64 [B,N]  the smallest eigenvalue l0 of the point's neighbourhood covariance where it is salient, else 0
    A point is salient where its neighbourhood within salient_radius, itself included, holds min_neighbors points and the
    covariance's eigenvalues l0 <= l1 <= l2 satisfy l1 / l2 < gamma_21 and l0 / l1 < gamma_32; a salient point is a keypoint
    where no point within non_max_radius is more salient (and that neighbourhood holds min_neighbors points too).  The
    neighbourhoods are ``search_radius``' -- distances of differences in fp32, a point ON the sphere counts -- and the covariance
    is taken of the fp32 differences to the point in fp64, so a cloud far from the origin needs no centring.  The result is
    defined to the bit (include/keypoint/vcr_hip_iss.h); against Open3D's float64 arithmetic it can differ at a point whose ratio
    lies within about 1e-5 of its gamma or whose saliency ties a neighbour's that closely.
    Explicit radii run the whole batch as one: ONE search at the larger radius where non_max_radius <= salient_radius (the
    rows ascend in distance: the suppression reads a prefix of them), two searches otherwise.  capacity=None costs
    ``search_radius``' one host synchronisation a search, capacity=int none: a cloud whose rows exceed it comes back with count 0,
    every flag -2 and every saliency NaN.  cell: the search grid's edge, as ``search_radius``' (it never changes the result).
    A radius of None is Open3D's default, 6 (salient) and 4 (non-max) times ``model_resolution``, rounded to fp32 per cloud:
    that reads the resolutions back -- one more host synchronisation -- and, because ``search_radius`` takes one radius a call,
    runs a batch of B > 1 cloud by cloud.  It needs N >= 2.
    border_radius (None changes nothing: the same launches, the same bits) is PCL's rule against the rim of
    a partial scan, whose half-empty neighbourhoods look salient: a point with a boundary point (``compute_boundary_points`` at
    border_radius over all the points within it, border_angle in degrees) within border_radius of it, itself included, is not
    salient -- its saliency is 0 before the suppression, and in what want_saliency returns.  normals [B,3,N] serve the boundary;
    None estimates them over normal_radius (default border_radius).  With normals given and border_radius <= the larger radius
    searched already, the boundary reads a prefix of those rows; otherwise it costs one search more (two where normal_radius
    differs)."""
    api = "compute_iss_keypoints"
    radius._cloud(api, xyz)
    g21, g32 = check_arguments(api, salient_radius, non_max_radius, gamma_21, gamma_32, min_neighbors, border_radius, normal_radius,
                               border_angle)
    B, _, N = xyz.shape
    if border_radius is not None:
        from .border import check_normals
        check_normals(api, normals, B, N)
    elif normals is not None:
        raise VcrHipError(f"{api}: normals belong to border_radius, which is None")
    if (salient_radius is None or non_max_radius is None) and N < 2:
        raise VcrHipError(f"{api}: the default radii come from model_resolution, which needs at least 2 points, got N = {N}")
    radius._on_device(api, xyz)
    xyz = xyz.contiguous().float()
    if salient_radius is None or non_max_radius is None:
        res = model_resolution(xyz).cpu()                   # the host synchronisation of the default radii
        per = []
        for b in range(B):
            sr = float(torch.tensor(6.0 * float(res[b]), dtype=torch.float32)) if salient_radius is None else salient_radius
            nr = float(torch.tensor(4.0 * float(res[b]), dtype=torch.float32)) if non_max_radius is None else non_max_radius
            per.append(compute_iss_keypoints(xyz[b:b + 1], sr, nr, g21, g32, min_neighbors, capacity, cell, True, True,
                                             border_radius, normal_radius, border_angle,
                                             None if normals is None else normals[b:b + 1]))
        got = tuple(torch.cat([p[j] for p in per]) for j in range(5))
    else:
        sr, nr = float(salient_radius), float(non_max_radius)
        xyz4 = native.to_rows4(xyz)
        if border_radius is not None and normals is not None:
            native.same_device(xyz, normals)
            normals = normals.contiguous().float()
        if nr <= sr:
            idx, row_start, total, d2 = _search(api, xyz, sr, True, capacity, cell)
            sal = saliency_rows(xyz4, idx, row_start, total, g21, g32, min_neighbors)["saliency"]
            if border_radius is not None:
                sal = _without_border(sal, _border_near(api, xyz, xyz4, (sr, idx, row_start, total, d2), border_radius,
                                                        normal_radius, border_angle, normals, capacity, cell))
            flag = nms_rows(idx, row_start, total, sal, min_neighbors, d2=d2, r2_nm=radius._radius(api, nr)[1])["keypoint"]
        else:
            sal = saliency_rows(xyz4, *_search(api, xyz, sr, False, capacity, cell), g21, g32, min_neighbors)["saliency"]
            if border_radius is not None:
                sal = _without_border(sal, _border_near(api, xyz, xyz4, None, border_radius, normal_radius, border_angle, normals,
                                                        capacity, cell))
            flag = nms_rows(*_search(api, xyz, nr, False, capacity, cell), sal, min_neighbors)["keypoint"]
        o = select(xyz, flag)
        got = (o["points"], o["count"], o["index"], flag, sal)
    return got[:3] + ((got[3],) if want_flag else ()) + ((got[4],) if want_saliency else ())
