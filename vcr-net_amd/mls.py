"""ctypes binding of include/smooth/vcr_hip_mls.h and the Python API on top of it: moving least squares
smoothing on the device, over the ragged CSR rows ``search_radius`` returns -- vcr_mls_weights_f32 (the origin of every point's fit
and every neighbour's Gaussian weight) and vcr_mls_fit_f32 (the weighted quadratic over the tangent plane, its 6 x 6 solve and the
projection).  ``smooth_mls`` is PCL's MovingLeastSquares with the SIMPLE projection.

Like ``border``, the header extends include/vcr_hip.h without touching it and this module keeps its own STRUCTS / SIGNATURES maps,
applied once to ``native.lib()`` on first use.  No CPU fallback, as everywhere."""
from __future__ import annotations

import ctypes as C
import math
import torch

from . import extension, native
from . import radius as rad
from .border import _search, check_normals
from .iss import _rows, check_min_neighbors
from .native import VcrHipError, f32p, ptr
from .score import i32p

MAX_N = 131072
FORMS = {"plain": 1, "transpose": 2}                       # VCR_MLS_PLAIN / VCR_MLS_TRANSPOSE: what ``variant`` forces
NOT_SERVED = -2                                            # VCR_MLS_NOT_SERVED
TERMS = 6                                                  # VCR_MLS_TERMS

i64p = C.c_void_p
f64p = C.c_void_p


class MlsWeightsArgs(native._Sized):
    _fields_ = [("struct_bytes", C.c_uint32), ("xyz4", f32p), ("normals", f32p), ("idx", i32p), ("row_start", i64p),
                ("total", i64p), ("B", C.c_int), ("N", C.c_int), ("capacity", C.c_int), ("sqr_gauss_param", C.c_double),
                ("weight", f64p), ("origin", f64p), ("w_self", f64p), ("frame", i32p)]


class MlsFitArgs(native._Sized):
    _fields_ = [("struct_bytes", C.c_uint32), ("xyz4", f32p), ("normals", f32p), ("idx", i32p), ("row_start", i64p),
                ("total", i64p), ("weight", f64p), ("origin", f64p), ("w_self", f64p), ("frame", i32p), ("B", C.c_int),
                ("N", C.c_int), ("capacity", C.c_int), ("order", C.c_int), ("min_neighbors", C.c_int), ("variant", C.c_int),
                ("points", f32p), ("fit", i32p), ("normals_out", f32p), ("coeffs", f64p)]


STRUCTS = {"vcr_mls_weights_args": MlsWeightsArgs, "vcr_mls_fit_args": MlsFitArgs}

# name -> (restype, [argtypes]): the prototypes of include/smooth/vcr_hip_mls.h (tests/test_mls_cpu.py holds them to it)
SIGNATURES = {"vcr_mls_weights_f32": (C.c_int, [C.POINTER(MlsWeightsArgs), C.c_void_p]),
              "vcr_mls_fit_f32": (C.c_int, [C.POINTER(MlsFitArgs), C.c_void_p])}

lib = extension.typed_lib(SIGNATURES)                      # native.lib() with this module's entry points typed (once)


def _variant(api, variant):
    if variant in FORMS:
        return FORMS[variant]
    if isinstance(variant, bool) or variant not in (0, 1, 2):
        raise VcrHipError(f'{api}: variant must be 0 (the plan), "plain" or "transpose", got {variant!r}')
    return int(variant)


def check_order(api, order):
    if isinstance(order, bool) or not isinstance(order, int) or order not in (1, 2):
        raise VcrHipError(f"{api}: order must be 1 (the plane) or 2 (the quadratic), got {order!r}")
    return int(order)


def check_gauss(api, sqr_gauss_param):
    """h2 as a float: finite and > 0."""
    try:
        h2 = float(sqr_gauss_param)
    except (TypeError, ValueError):
        h2 = float("nan")
    if isinstance(sqr_gauss_param, bool) or not (math.isfinite(h2) and h2 > 0.0):
        raise VcrHipError(f"{api}: sqr_gauss_param must be None or finite and > 0, got {sqr_gauss_param!r}")
    return h2


def _cloud_rows(api, xyz4, normals, idx, row_start, total):
    """The inputs both stages share -> (B, N, capacity)."""
    if not (torch.is_tensor(xyz4) and xyz4.dim() == 3 and xyz4.shape[2] == 4 and xyz4.dtype == torch.float32
            and xyz4.shape[0] >= 1):
        raise VcrHipError(f"{api}: xyz4 must be float32 [B, N, 4] rows")
    B, N, _ = xyz4.shape
    if not 1 <= N <= MAX_N:
        raise VcrHipError(f"{api}: a cloud must have 1 ... {MAX_N} points, got {N}")
    if not (torch.is_tensor(normals) and normals.dtype == torch.float32 and tuple(normals.shape) == (B, 3, N)):
        raise VcrHipError(f"{api}: normals must be float32 [B, 3, N] with B, N = {B}, {N}")
    return B, N, _rows(api, idx, row_start, total, B, N)


@native._guarded
def weights_rows(xyz4, normals, idx, row_start, total, sqr_gauss_param, guard=0, prefill=None):
    """vcr_mls_weights_f32 on xyz4 [B,N,4] rows (native.to_rows4), normals float32 [B,3,N] and the CSR rows idx int32
    [B,capacity], row_start int64 [B,N+1], total int64 [B] (``search_radius`` on the same cloud, or any caller's) -> dict of
    weight float64 [B,capacity] (every entry's Gaussian weight; +0.0 in a skipped slot, NaN behind the rows, over a point without
    a frame and over a cloud that is not served), origin float64 [B,N,3] (the point's projection on the plane through its
    neighbourhood's mean, relative to the point), w_self float64 [B,N] and frame int32 [B,N] (1 / 0; -2 not served).
    guard / prefill (tests): as voxel.voxel_grid's -- the buffers come back under "_raw"."""
    api = "mls.weights_rows"
    B, N, capacity = _cloud_rows(api, xyz4, normals, idx, row_start, total)
    h2 = check_gauss(api, sqr_gauss_param)
    dev = native.same_device(xyz4, normals, idx, row_start, total)
    xyz4, normals, idx = xyz4.contiguous(), normals.contiguous(), idx.contiguous()
    row_start, total = row_start.contiguous(), total.contiguous()
    has = B * capacity > 0                                  # (an empty tensor has no address to give)
    xyz4_p = ptr(xyz4)
    out, raw = extension.outputs(dev, guard, prefill)
    o = {"weight": out("weight", B * capacity, torch.float64).view(B, capacity),
         "origin": out("origin", B * N * 3, torch.float64).view(B, N, 3), "w_self": out("w_self", B * N, torch.float64).view(B, N),
         "frame": out("frame", B * N, torch.int32).view(B, N)}
    a = MlsWeightsArgs(xyz4_p, ptr(normals), ptr(idx) if has else None, ptr(row_start), ptr(total), B, N, capacity, h2,
                       ptr(o["weight"]) if has else None, ptr(o["origin"]), ptr(o["w_self"]), ptr(o["frame"]))
    native.check(lib().vcr_mls_weights_f32(C.byref(a), native.stream_ptr()), "vcr_mls_weights_f32")
    if guard or prefill is not None:
        o["_raw"] = raw
    return o


@native._guarded
def fit_rows(xyz4, normals, idx, row_start, total, weight, origin, w_self, frame, order=2, min_neighbors=3, want_normals=True,
             want_coeffs=True, variant=0, guard=0, prefill=None):
    """vcr_mls_fit_f32 on the inputs of ``weights_rows`` and weight float64 [B,capacity], origin float64 [B,N,3], w_self float64
    [B,N], frame int32 [B,N] AS GIVEN (``weights_rows``' or any caller's) -> dict of points float32 [B,3,N], fit int32 [B,N] (2 =
    on the quadratic, 1 = on the plane alone, 0 = left where it was, -2 = not served) and, where asked, normals float32 [B,3,N] and
    coeffs float64 [B,N,6].  variant: 0 for the plan's combine, "plain" or "transpose" to force one (the same bits).
    guard / prefill: as above."""
    api = "mls.fit_rows"
    B, N, capacity = _cloud_rows(api, xyz4, normals, idx, row_start, total)
    for name, t, dtype, shape in (("weight", weight, torch.float64, (B, capacity)), ("origin", origin, torch.float64, (B, N, 3)),
                                  ("w_self", w_self, torch.float64, (B, N)), ("frame", frame, torch.int32, (B, N))):
        if not (torch.is_tensor(t) and t.dtype == dtype and tuple(t.shape) == shape):
            raise VcrHipError(f"{api}: {name} must be {str(dtype).replace('torch.', '')} {list(shape)}")
    order = check_order(api, order)
    check_min_neighbors(api, min_neighbors)
    v = _variant(api, variant)
    dev = native.same_device(xyz4, normals, idx, row_start, total, weight, origin, w_self, frame)
    xyz4, normals, idx = xyz4.contiguous(), normals.contiguous(), idx.contiguous()
    row_start, total = row_start.contiguous(), total.contiguous()
    weight, origin, w_self, frame = weight.contiguous(), origin.contiguous(), w_self.contiguous(), frame.contiguous()
    has = B * capacity > 0
    xyz4_p = ptr(xyz4)
    out, raw = extension.outputs(dev, guard, prefill)
    o = {"points": out("points", B * 3 * N, torch.float32).view(B, 3, N), "fit": out("fit", B * N, torch.int32).view(B, N)}
    if want_normals:
        o["normals"] = out("normals", B * 3 * N, torch.float32).view(B, 3, N)
    if want_coeffs:
        o["coeffs"] = out("coeffs", B * N * TERMS, torch.float64).view(B, N, TERMS)
    a = MlsFitArgs(xyz4_p, ptr(normals), ptr(idx) if has else None, ptr(row_start), ptr(total), ptr(weight) if has else None,
                   ptr(origin), ptr(w_self), ptr(frame), B, N, capacity, order, min_neighbors, v, ptr(o["points"]), ptr(o["fit"]),
                   ptr(o.get("normals")), ptr(o.get("coeffs")))
    native.check(lib().vcr_mls_fit_f32(C.byref(a), native.stream_ptr()), "vcr_mls_fit_f32")
    if guard or prefill is not None:
        o["_raw"] = raw
    return o


def smooth_rows(xyz4, normals, idx, row_start, total, sqr_gauss_param, order=2, min_neighbors=3, want_normals=True,
                want_coeffs=True, variant=0):
    """The two stages on given rows -> ``fit_rows``' dict."""
    a = weights_rows(xyz4, normals, idx, row_start, total, sqr_gauss_param)
    return fit_rows(xyz4, normals, idx, row_start, total, a["weight"], a["origin"], a["w_self"], a["frame"], order, min_neighbors,
                    want_normals, want_coeffs, variant)


def check_arguments(api, radius, order=2, max_nn=None, sqr_gauss_param=None, min_neighbors=3):
    """What smooth_mls asks of its numbers, under the caller's name -> h2 as a float."""
    if radius is None:
        raise VcrHipError(f"{api}: radius has no default: give the neighbourhood's radius")
    r, _ = rad._radius(api, radius)
    check_order(api, order)
    if max_nn is not None and (isinstance(max_nn, bool) or not isinstance(max_nn, int) or not 1 <= max_nn <= rad.MAX_NN):
        raise VcrHipError(f"{api}: max_nn must be None or an integer in [1, {rad.MAX_NN}], got {max_nn!r}")
    check_min_neighbors(api, min_neighbors)
    return r * r if sqr_gauss_param is None else check_gauss(api, sqr_gauss_param)     # (the product of two doubles: PCL's default)


def smooth_mls(xyz, radius=None, normals=None, order=2, max_nn=None, sqr_gauss_param=None, min_neighbors=3, capacity=None,
               cell=None, want_normals=False, want_coeffs=False):
    """Every point of every cloud of xyz [B,3,N] (device tensor, up to 131 072 points a cloud) moved onto the surface its
    neighbourhood describes: PCL's MovingLeastSquares (polynomial order 1 or 2, SIMPLE projection).  Returns (points float32
    [B,3,N], fit int32 [B,N]) -- the count and the order are the input's, nothing is compacted -- then, where asked:
      normals  float32 [B,3,N]  the fitted surface's normal at the projected point, on the side of the input normal
      coeffs   float64 [B,N,6]  the polynomial's coefficients of (1, v, v^2, u, uv, u^2) over the tangent plane
    fit: 2 = projected on the quadratic, 1 = projected on the plane alone (order=1, fewer than six points, or a neighbourhood
    that does not determine a quadratic), 0 = left where it was (fewer than min_neighbors points, the point itself included, or no
    usable normal), -2 = the cloud was not served.
    A point's neighbours are ``search_radius``' rows (within `radius`; max_nn cuts them to the nearest max_nn OTHER points, None
    takes all); they are weighted by exp(-d^2 / sqr_gauss_param), d the distance to the point's projection on the plane through
    their mean; sqr_gauss_param=None is radius * radius in double, PCL's default.  `radius` has no default.  normals [B,3,N] of any
    length; None estimates them on the same rows (``rows.normals``).  Everything but the one exp a neighbour is defined to the bit
    (include/smooth/vcr_hip_mls.h).
    ONE search a call.  capacity=None costs ``search_radius``' one host synchronisation, capacity=int none: a cloud whose rows
    exceed it comes back NaN with every fit -2, and the rest of the batch is unaffected.  cell: the search grid's edge (it never
    changes the result)."""
    api = "smooth_mls"
    from . import rows
    rad._cloud(api, xyz)
    B, _, N = xyz.shape
    check_normals(api, normals, B, N)
    h2 = check_arguments(api, radius, order, max_nn, sqr_gauss_param, min_neighbors)
    xyz = xyz.contiguous().float()                          # (the search refuses a capacity, a cell and a cloud off the device)
    idx, row_start, total = _search(api, xyz, radius, max_nn, False, capacity, cell)
    xyz4 = native.to_rows4(xyz)
    if normals is None:
        normals = rows.normals(xyz4, idx, row_start, total, want_curvature=False)[0]
    else:
        native.same_device(xyz, normals)
        normals = normals.contiguous().float()
    o = smooth_rows(xyz4, normals, idx, row_start, total, h2, order, min_neighbors, want_normals, want_coeffs)
    return (o["points"], o["fit"]) + ((o["normals"],) if want_normals else ()) + ((o["coeffs"],) if want_coeffs else ())
