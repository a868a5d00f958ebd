"""ctypes binding of include/border/vcr_hip_border.h and the Python API on top of it: the points on the rim
of a scanned surface, on the device, over the ragged CSR rows ``search_radius`` returns -- vcr_border_angles_f32 (every neighbour's
angle in the point's tangent frame), vcr_border_gap_f32 (the largest angular gap around the point, and the flag) with its host-only
vcr_border_form, and vcr_border_near_f32 (the flags spread once over rows).  ``compute_boundary_points`` is Open3D's call of that
name; ``compute_iss_keypoints(border_radius=...)`` uses the spreading for PCL's border rule.

Like ``rows`` and ``iss``, the header extends include/vcr_hip.h without touching it and this module keeps its own STRUCTS /
SIGNATURES maps, applied once to ``native.lib()`` on first use.  No CPU fallback, as everywhere."""
from __future__ import annotations

import ctypes as C
import math
import torch

from . import extension, native
from . import radius as rad
from .iss import _rows, check_min_neighbors
from .native import VcrHipError, f32p, ptr
from .score import i32p

MAX_N = 131072
FORMS = {"lane": 1, "wave": 2}                             # VCR_BORDER_LANE / VCR_BORDER_WAVE: what ``variant`` forces
CHUNK = 256                                                # VCR_BORDER_CHUNK: angles of a row the wave form holds in LDS at a time
WAVE_GAP = 10                                              # VCR_BORDER_WAVE_GAP: the row length the gap's wave form starts at
NOT_SERVED = -2                                            # VCR_BORDER_NOT_SERVED
TWO_PI = float.fromhex("0x1.921fb54442d18p+2")             # the double 0x401921FB54442D18

i64p = C.c_void_p
f64p = C.c_void_p


class BorderAnglesArgs(native._Sized):
    _fields_ = [("struct_bytes", C.c_uint32), ("xyz4", f32p), ("normals", f32p), ("idx", i32p), ("row_start", i64p),
                ("total", i64p), ("B", C.c_int), ("N", C.c_int), ("capacity", C.c_int), ("angle", f64p), ("frame", i32p),
                ("d2", f32p), ("r2", C.c_float)]


class BorderGapArgs(native._Sized):
    _fields_ = [("struct_bytes", C.c_uint32), ("angle", f64p), ("row_start", i64p), ("total", i64p), ("frame", i32p), ("d2", f32p),
                ("B", C.c_int), ("N", C.c_int), ("capacity", C.c_int), ("min_neighbors", C.c_int), ("angle_threshold", C.c_double),
                ("r2", C.c_float), ("variant", C.c_int), ("gap", f64p), ("flag", i32p)]


class BorderNearArgs(native._Sized):
    _fields_ = [("struct_bytes", C.c_uint32), ("flag", i32p), ("idx", i32p), ("row_start", i64p), ("total", i64p), ("d2", f32p),
                ("B", C.c_int), ("N", C.c_int), ("capacity", C.c_int), ("r2", C.c_float), ("near", i32p)]


STRUCTS = {"vcr_border_angles_args": BorderAnglesArgs, "vcr_border_gap_args": BorderGapArgs,
           "vcr_border_near_args": BorderNearArgs}

_int, _intp = C.c_int, C.POINTER(C.c_int)

# name -> (restype, [argtypes]): the prototypes of include/border/vcr_hip_border.h (tests/test_border_cpu.py holds them to it)
SIGNATURES = {"vcr_border_angles_f32": (_int, [C.POINTER(BorderAnglesArgs), C.c_void_p]),
              "vcr_border_gap_f32": (_int, [C.POINTER(BorderGapArgs), C.c_void_p]),
              "vcr_border_form": (_int, [_int, _int, _int, _int, _int, _intp]),
              "vcr_border_near_f32": (_int, [C.POINTER(BorderNearArgs), C.c_void_p])}

lib = extension.typed_lib(SIGNATURES)                      # native.lib() with this module's entry points typed (once)


def form(B, N, capacity, cu_count=256, variant=0):
    """vcr_border_form (host only): the gap pass's form, 1 = a lane a row, 2 = a wave a row."""
    f = C.c_int(0)
    native.check(lib().vcr_border_form(B, N, capacity, cu_count, variant, C.byref(f)), "vcr_border_form")
    return f.value


def _variant(api, variant):
    if variant in FORMS:
        return FORMS[variant]
    if isinstance(variant, bool) or variant not in (0, 1, 2):
        raise VcrHipError(f'{api}: variant must be 0 (the plan), "lane" or "wave", got {variant!r}')
    return int(variant)


def _points(api, N):
    if not 1 <= N <= MAX_N:
        raise VcrHipError(f"{api}: a cloud must have 1 ... {MAX_N} points, got {N}")


def _prefix(api, d2, r2, B, capacity):
    """The optional (d2, r2) pair -> r2 as a float (0.0 without them)."""
    if (d2 is None) != (r2 is None):
        raise VcrHipError(f"{api}: give both d2 and r2, or neither (the whole row)")
    if d2 is None:
        return 0.0
    if not (torch.is_tensor(d2) and d2.dtype == torch.float32 and tuple(d2.shape) == (B, capacity)):
        raise VcrHipError(f"{api}: d2 must be None or float32 [B, capacity] with B, capacity = {B}, {capacity}")
    try:
        v = float(r2)
    except (TypeError, ValueError):
        v = float("nan")
    if not v >= 0.0:
        raise VcrHipError(f"{api}: r2 must be >= 0, got {r2!r}")
    return v


def check_threshold(api, name, angle):
    """An angle threshold (radians or degrees alike): a finite number >= 0 -> float."""
    try:
        a = float(angle)
    except (TypeError, ValueError):
        a = float("nan")
    if isinstance(angle, bool) or not (math.isfinite(a) and a >= 0.0):
        raise VcrHipError(f"{api}: {name} must be finite and >= 0, got {angle!r}")
    return a


def radians(degrees):
    """The threshold the C side takes for an angle in degrees: degrees * (pi / 180), both factors doubles."""
    return float(degrees) * (math.pi / 180.0)


@native._guarded
def angles_rows(xyz4, normals, idx, row_start, total, d2=None, r2=None, want_frame=False, guard=0, prefill=None):
    """vcr_border_angles_f32 on xyz4 [B,N,4] rows (native.to_rows4), normals float32 [B,3,N] and the CSR rows idx int32
    [B,capacity], row_start int64 [B,N+1], total int64 [B] (``search_radius`` on the same cloud, or any caller's) -> dict of angle
    float64 [B,capacity] (every entry's angle in its point's tangent frame, in [-pi, pi]; NaN in a slot that does not count and
    behind the rows) and, with want_frame, frame int32 [B,N] (1 where the point has a frame, 0 where not, -2 over a cloud that is
    not served).  d2 float32 [B,capacity] with r2 (a float, compared in fp32): a row is its leading entries with d2 <= r2.
    guard / prefill (tests): as voxel.voxel_grid's -- the buffers come back under "_raw"."""
    api = "border.angles_rows"
    if not (torch.is_tensor(xyz4) and xyz4.dim() == 3 and xyz4.shape[2] == 4 and xyz4.dtype == torch.float32
            and xyz4.shape[0] >= 1):
        raise VcrHipError(f"{api}: xyz4 must be float32 [B, N, 4] rows")
    B, N, _ = xyz4.shape
    _points(api, N)
    if not (torch.is_tensor(normals) and normals.dtype == torch.float32 and tuple(normals.shape) == (B, 3, N)):
        raise VcrHipError(f"{api}: normals must be float32 [B, 3, N] with B, N = {B}, {N}")
    capacity = _rows(api, idx, row_start, total, B, N)
    v = _prefix(api, d2, r2, B, capacity)
    dev = native.same_device(xyz4, normals, idx, row_start, total, d2)
    xyz4, normals, idx = xyz4.contiguous(), normals.contiguous(), idx.contiguous()
    row_start, total = row_start.contiguous(), total.contiguous()
    d2 = None if d2 is None else d2.contiguous()
    has = B * capacity > 0                                  # (an empty tensor has no address to give)
    xyz4_p = ptr(xyz4)
    out, raw = extension.outputs(dev, guard, prefill)
    o = {"angle": out("angle", B * capacity, torch.float64).view(B, capacity)}
    if want_frame:
        o["frame"] = out("frame", B * N, torch.int32).view(B, N)
    a = BorderAnglesArgs(xyz4_p, ptr(normals), ptr(idx) if has else None, ptr(row_start), ptr(total), B, N, capacity,
                         ptr(o["angle"]) if has else None, ptr(o.get("frame")), ptr(d2) if has and d2 is not None else None, v)
    native.check(lib().vcr_border_angles_f32(C.byref(a), native.stream_ptr()), "vcr_border_angles_f32")
    if guard or prefill is not None:
        o["_raw"] = raw
    return o


@native._guarded
def gap_rows(angle, row_start, total, min_neighbors=3, angle_threshold=math.pi / 2, frame=None, d2=None, r2=None, variant=0,
             guard=0, prefill=None):
    """vcr_border_gap_f32 on angle float64 [B,capacity] (``angles_rows``) and the CSR offsets -> dict of gap float64 [B,N] (the
    largest angular gap between the row's counted angles in radians, the one across +-pi included; 0 where the row and the point
    are fewer than min_neighbors or no angle counts; NaN where frame is given and 0, and over a cloud that is not served) and flag
    int32 [B,N]: 1 where gap > angle_threshold (RADIANS here), else 0; -2 over a cloud that is not served.  frame int32 [B,N]:
    ``angles_rows``' output.  d2 / r2: as ``angles_rows``' -- the row's length is its used entries'.
    variant: 0 for the plan's form, "lane" or "wave" to force one.  guard / prefill: as above."""
    api = "border.gap_rows"
    if not (torch.is_tensor(angle) and angle.dtype == torch.float64 and angle.dim() == 2 and angle.shape[0] >= 1):
        raise VcrHipError(f"{api}: angle must be float64 [B, capacity]")
    B, capacity = angle.shape
    if not (torch.is_tensor(row_start) and row_start.dtype == torch.int64 and row_start.dim() == 2
            and row_start.shape[0] == B and row_start.shape[1] >= 2):
        raise VcrHipError(f"{api}: row_start must be int64 [B, N + 1] with B = {B}")
    N = row_start.shape[1] - 1
    _points(api, N)
    if B * N >= rad._INT32_LIMIT or B * capacity >= rad._INT32_LIMIT:
        raise VcrHipError(f"{api}: B * N and B * capacity must be below 2^31, got B = {B}, N = {N}, capacity = {capacity}")
    if not (torch.is_tensor(total) and total.dtype == torch.int64 and tuple(total.shape) == (B,)):
        raise VcrHipError(f"{api}: total must be int64 [B] with B = {B}")
    check_min_neighbors(api, min_neighbors)
    thr = check_threshold(api, "angle_threshold", angle_threshold)
    if frame is not None and not (torch.is_tensor(frame) and frame.dtype == torch.int32 and tuple(frame.shape) == (B, N)):
        raise VcrHipError(f"{api}: frame must be None or int32 [B, N] with B, N = {B}, {N}")
    r = _prefix(api, d2, r2, B, capacity)
    v = _variant(api, variant)
    dev = native.same_device(angle, row_start, total, frame, d2)
    angle, row_start, total = angle.contiguous(), row_start.contiguous(), total.contiguous()
    frame = None if frame is None else frame.contiguous()
    d2 = None if d2 is None else d2.contiguous()
    has = B * capacity > 0
    rs_p = ptr(row_start)
    out, raw = extension.outputs(dev, guard, prefill)
    o = {"gap": out("gap", B * N, torch.float64).view(B, N), "flag": out("flag", B * N, torch.int32).view(B, N)}
    a = BorderGapArgs(ptr(angle) if has else None, rs_p, ptr(total), ptr(frame), ptr(d2) if has and d2 is not None else None, B, N,
                      capacity, min_neighbors, thr, r, v, ptr(o["gap"]), ptr(o["flag"]))
    native.check(lib().vcr_border_gap_f32(C.byref(a), native.stream_ptr()), "vcr_border_gap_f32")
    if guard or prefill is not None:
        o["_raw"] = raw
    return o


@native._guarded
def near_rows(flag, idx, row_start, total, d2=None, r2=None, guard=0, prefill=None):
    """vcr_border_near_f32 on flag int32 [B,N] (``gap_rows``) and the CSR rows -> dict of near int32 [B,N]: 1 where the point's
    flag or a used entry's is above 0, else 0; -2 over a cloud that is not served or whose flags are -2.  d2 float32 [B,capacity]
    with r2: a row's used entries are its leading ones with d2 <= r2; without them all of the row.  guard / prefill: as above."""
    api = "border.near_rows"
    if not (torch.is_tensor(flag) and flag.dtype == torch.int32 and flag.dim() == 2 and flag.shape[0] >= 1):
        raise VcrHipError(f"{api}: flag must be int32 [B, N]")
    B, N = flag.shape
    _points(api, N)
    capacity = _rows(api, idx, row_start, total, B, N)
    v = _prefix(api, d2, r2, B, capacity)
    dev = native.same_device(flag, idx, row_start, total, d2)
    flag, idx, row_start, total = flag.contiguous(), idx.contiguous(), row_start.contiguous(), total.contiguous()
    d2 = None if d2 is None else d2.contiguous()
    has = B * capacity > 0
    flag_p = ptr(flag)
    out, raw = extension.outputs(dev, guard, prefill)
    o = {"near": out("near", B * N, torch.int32).view(B, N)}
    a = BorderNearArgs(flag_p, ptr(idx) if has else None, ptr(row_start), ptr(total), ptr(d2) if has and d2 is not None else None,
                       B, N, capacity, v, ptr(o["near"]))
    native.check(lib().vcr_border_near_f32(C.byref(a), native.stream_ptr()), "vcr_border_near_f32")
    if guard or prefill is not None:
        o["_raw"] = raw
    return o


def check_normals(api, normals, B, N):
    if normals is not None and not (torch.is_tensor(normals) and tuple(normals.shape) == (B, 3, N)):
        raise VcrHipError(f"{api}: normals must be None or a [B, 3, N] tensor with B, N = {B}, {N}, got "
                          f"{tuple(normals.shape) if torch.is_tensor(normals) else type(normals).__name__}")


def _search(api, xyz, r, max_nn, want_d2, capacity, cell):
    """search_radius with its refusals under this call's name; a cap no row can reach is no cap."""
    if max_nn is not None and max_nn + 1 > xyz.shape[2]:
        max_nn = None
    try:
        return rad.search_radius(xyz, r, max_nn=max_nn, want_d2=want_d2, capacity=capacity, cell=cell)
    except VcrHipError as e:
        raise VcrHipError(str(e).replace("search_radius", api, 1)) from None


def boundary_rows(xyz4, normals, idx, row_start, total, min_neighbors, threshold, d2=None, r2=None):
    """The two passes on given rows -> (flag int32 [B,N], gap float64 [B,N]); threshold in radians."""
    a = angles_rows(xyz4, normals, idx, row_start, total, d2=d2, r2=r2, want_frame=True)
    g = gap_rows(a["angle"], row_start, total, min_neighbors, threshold, frame=a["frame"], d2=d2, r2=r2)
    return g["flag"], g["gap"]


def check_arguments(api, radius=None, max_nn=30, angle_threshold=90.0, min_neighbors=3):
    """What compute_boundary_points asks of its numbers, under the caller's name -> the threshold in radians."""
    if radius is None:
        raise VcrHipError(f"{api}: radius has no default: give the neighbourhood's radius")
    rad._radius(api, radius)
    if max_nn is not None and (isinstance(max_nn, bool) or not isinstance(max_nn, int) or not 1 <= max_nn <= rad.MAX_NN):
        raise VcrHipError(f"{api}: max_nn must be None or an integer in [1, {rad.MAX_NN}], got {max_nn!r}")
    deg = check_threshold(api, "angle_threshold", angle_threshold)
    check_min_neighbors(api, min_neighbors)
    return radians(deg)


def compute_boundary_points(xyz, normals=None, radius=None, max_nn=30, angle_threshold=90.0, min_neighbors=3, capacity=None,
                            cell=None, want_flag=False, want_gap=False):
    """The points on the rim of every cloud of xyz [B,3,N] (device tensor, up to 131 072 points a cloud): Open3D's
    compute_boundary_points(radius, max_nn, angle_threshold).  Returns (points, count, index) as ``remove_radius_outlier``
    returns them -- the boundary points compacted in ascending index order, NaN / -1 behind count[b]; ``voxel.unpad(points,
    count)`` cuts the clouds to their sizes -- then, where asked:
      flag  int32 [B,N]    1 for a boundary point, 0 for any other point, -2 over a cloud that was not served
      gap   float64 [B,N]  the largest angular gap around the point in RADIANS; NaN where the point has no frame
    A point's neighbours (``search_radius``' hybrid rows: within `radius`, the nearest max_nn of them; max_nn counts OTHER points,
    Open3D's is ours + 1; None takes all) are projected on the plane across its normal; the point is on the boundary where the
    largest gap between the directions of two neighbours that follow each other around it exceeds angle_threshold (DEGREES, as
    Open3D's; the comparison is strict).  A point whose row and itself are fewer than min_neighbors is never one.
    `radius` has no default.  normals [B,3,N] of any length; None estimates them on the same rows (``rows.normals``).
    Everything but the one atan2 a neighbour is defined to the bit (include/border/vcr_hip_border.h).
    ONE search a call.  capacity=None costs ``search_radius``' one host synchronisation, capacity=int none: a cloud whose rows
    exceed it comes back with count 0, every flag -2 and every gap NaN.  cell: the search grid's edge (it never changes the
    result)."""
    api = "compute_boundary_points"
    from . import iss, rows
    rad._cloud(api, xyz)
    B, _, N = xyz.shape
    check_normals(api, normals, B, N)
    thr = check_arguments(api, radius, max_nn, angle_threshold, min_neighbors)
    xyz = xyz.contiguous().float()                          # (the search refuses a capacity, a cell and a cloud off the device)
    idx, row_start, total = _search(api, xyz, radius, max_nn, False, capacity, cell)
    xyz4 = native.to_rows4(xyz)
    if normals is None:
        normals = rows.normals(xyz4, idx, row_start, total, want_curvature=False)[0]
    else:
        native.same_device(xyz, normals)
        normals = normals.contiguous().float()
    flag, gap = boundary_rows(xyz4, normals, idx, row_start, total, min_neighbors, thr)
    o = iss.select(xyz, flag)
    return (o["points"], o["count"], o["index"]) + ((flag,) if want_flag else ()) + ((gap,) if want_gap else ())
