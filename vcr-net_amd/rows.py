"""ctypes binding of include/ext/vcr_hip_rows.h: normals and FPFH over neighbourhoods given as ragged CSR
rows -- (idx, row_start, total), what ``search_radius`` returns -- instead of a fixed-width idx [B,N,k]: vcr_rows_normals_f32,
vcr_rows_spfh_f32 and vcr_rows_fpfh_f32, and the host-only vcr_rows_form.  ``estimate_normals``, ``compute_fpfh_feature`` and
``register_features`` reach them through ``search="radius"``.

Like ``radius``, the header extends include/vcr_hip.h without touching it and this module keeps its own STRUCTS / SIGNATURES maps,
applied once to ``native.lib()`` on first use.  No CPU fallback, as everywhere."""
from __future__ import annotations

import ctypes as C
import torch

from . import extension, native
from .native import VcrHipError, f32p, ptr
from .score import i32p

MAX_N = 131072
SPFH_WORDS = 36                                            # VCR_ROWS_SPFH_WORDS: three groups of 11 counts and c_i
BINS = 11
FORMS = {"lane": 1, "wave": 2}                             # VCR_ROWS_LANE / VCR_ROWS_WAVE: what ``variant`` forces
WAVE_SPFH = 24                                             # VCR_ROWS_WAVE_SPFH / _FPFH: the row length the wave form starts at
WAVE_FPFH = 131072

i64p = C.c_void_p
u32p = C.c_void_p


class RowsNormalsArgs(native._Sized):
    _fields_ = [("struct_bytes", C.c_uint32), ("xyz4", f32p), ("idx", i32p), ("row_start", i64p), ("total", i64p), ("B", C.c_int),
                ("N", C.c_int), ("capacity", C.c_int), ("max_nn", C.c_int), ("viewpoint", f32p), ("normals", f32p),
                ("curvature", f32p)]


class RowsSpfhArgs(native._Sized):
    _fields_ = [("struct_bytes", C.c_uint32), ("xyz4", f32p), ("normals", f32p), ("idx", i32p), ("row_start", i64p),
                ("total", i64p), ("B", C.c_int), ("N", C.c_int), ("capacity", C.c_int), ("max_nn", C.c_int), ("variant", C.c_int),
                ("spfh", u32p)]


class RowsFpfhArgs(native._Sized):
    _fields_ = [("struct_bytes", C.c_uint32), ("xyz4", f32p), ("idx", i32p), ("row_start", i64p), ("total", i64p), ("spfh", u32p),
                ("B", C.c_int), ("N", C.c_int), ("capacity", C.c_int), ("max_nn", C.c_int), ("variant", C.c_int), ("fpfh", f32p)]


STRUCTS = {"vcr_rows_normals_args": RowsNormalsArgs, "vcr_rows_spfh_args": RowsSpfhArgs, "vcr_rows_fpfh_args": RowsFpfhArgs}

_int, _intp = C.c_int, C.POINTER(C.c_int)

# name -> (restype, [argtypes]): the prototypes of include/ext/vcr_hip_rows.h (tests/test_rows_cpu.py holds them to it)
SIGNATURES = {"vcr_rows_normals_f32": (_int, [C.POINTER(RowsNormalsArgs), C.c_void_p]),
              "vcr_rows_spfh_f32": (_int, [C.POINTER(RowsSpfhArgs), C.c_void_p]),
              "vcr_rows_fpfh_f32": (_int, [C.POINTER(RowsFpfhArgs), C.c_void_p]),
              "vcr_rows_form": (_int, [_int, _int, _int, _int, _int, _int, _intp, _intp])}

lib = extension.typed_lib(SIGNATURES)                      # native.lib() with this module's entry points typed (once)


def form(B, N, capacity, max_nn=0, cu_count=256, variant=0):
    """vcr_rows_form (host only): (the first pass's form, the second pass's), 1 = a lane a row, 2 = a wave a row."""
    s, f = C.c_int(0), C.c_int(0)
    native.check(lib().vcr_rows_form(B, N, capacity, max_nn, cu_count, variant, C.byref(s), C.byref(f)), "vcr_rows_form")
    return s.value, f.value


def _take(api, xyz4, idx, row_start, total, max_nn):
    """-> (B, N, capacity, max_nn as the C side takes it) of xyz4 [B,N,4] and the CSR triple."""
    if not (torch.is_tensor(xyz4) and xyz4.dim() == 3 and xyz4.shape[2] == 4 and xyz4.dtype == torch.float32):
        raise VcrHipError(f"{api}: xyz4 must be float32 [B, N, 4] rows")
    B, N, _ = xyz4.shape
    if not (torch.is_tensor(idx) and idx.dtype == torch.int32 and idx.dim() == 2 and idx.shape[0] == B):
        raise VcrHipError(f"{api}: idx must be int32 [B, capacity] with B = {B}")
    if not (torch.is_tensor(row_start) and row_start.dtype == torch.int64 and tuple(row_start.shape) == (B, N + 1)):
        raise VcrHipError(f"{api}: row_start must be int64 [B, N + 1] with B, N = {B}, {N}")
    if not (torch.is_tensor(total) and total.dtype == torch.int64 and tuple(total.shape) == (B,)):
        raise VcrHipError(f"{api}: total must be int64 [B] with B = {B}")
    return B, N, idx.shape[1], check_max_nn(api, max_nn)


def check_max_nn(api, max_nn):
    """None (the whole row) -> 0; otherwise an integer >= 1, as it is."""
    if max_nn is None:
        return 0
    if isinstance(max_nn, bool) or not isinstance(max_nn, int) or max_nn < 1:
        raise VcrHipError(f"{api}: max_nn must be None or an integer >= 1, got {max_nn!r}")
    return max_nn


def _variant(api, variant):
    if variant in FORMS:
        return FORMS[variant]
    if variant not in (0, 1, 2):
        raise VcrHipError(f'{api}: variant must be 0 (the plan), "lane" or "wave", got {variant!r}')
    return int(variant)


@native._guarded
def normals(xyz4, idx, row_start, total, max_nn=None, viewpoint=None, want_curvature=True, guard=0, prefill=None):
    """vcr_rows_normals_f32 on xyz4 [B,N,4] rows (native.to_rows4) and the CSR rows idx int32 [B,capacity], row_start int64
    [B,N+1], total int64 [B] (``search_radius`` on the same cloud) -> (normals float32 [B,3,N], curvature float32 [B,N] or
    None).  max_nn: None for the whole row, m for its first min(n_i, m) entries.  viewpoint [B,3]: the normals look at it.
    guard / prefill (tests): as plane.normals' -- the raw buffers come back as a third element."""
    B, N, capacity, m = _take("rows.normals", xyz4, idx, row_start, total, max_nn)
    dev = native.same_device(xyz4, idx, row_start, total, viewpoint)
    xyz4, idx, row_start, total = xyz4.contiguous(), idx.contiguous(), row_start.contiguous(), total.contiguous()
    if viewpoint is not None:
        if tuple(viewpoint.shape) != (B, 3):
            raise VcrHipError(f"rows.normals: viewpoint must be [B, 3] with B = {B}, got {tuple(viewpoint.shape)}")
        viewpoint = viewpoint.contiguous().float()
    out, raw = extension.outputs(dev, guard, prefill)
    nrm = out("normals", B * 3 * N, torch.float32).view(B, 3, N)
    cur = out("curvature", B * N, torch.float32).view(B, N) if want_curvature else None
    a = RowsNormalsArgs(ptr(xyz4), ptr(idx), ptr(row_start), ptr(total), B, N, capacity, m, ptr(viewpoint), ptr(nrm), ptr(cur))
    native.check(lib().vcr_rows_normals_f32(C.byref(a), native.stream_ptr()), "vcr_rows_normals_f32")
    return (nrm, cur, raw) if guard or prefill is not None else (nrm, cur)


@native._guarded
def spfh(xyz4, normals, idx, row_start, total, max_nn=None, variant=0, guard=0, prefill=None):
    """vcr_rows_spfh_f32 on xyz4 [B,N,4], normals float32 [B,3,N] and the CSR rows -> int32 [B,N,3,12] (the header's uint32
    words): per point and group the counts of 11 bins and the number of counted pairs.  variant: 0 for the plan's form, "lane"
    or "wave" to force one.  guard / prefill (tests): the raw buffers come back as a second element."""
    B, N, capacity, m = _take("rows.spfh", xyz4, idx, row_start, total, max_nn)
    if not (torch.is_tensor(normals) and normals.dtype == torch.float32 and tuple(normals.shape) == (B, 3, N)):
        raise VcrHipError(f"rows.spfh: normals must be float32 [B, 3, N] with B, N = {B}, {N}")
    v = _variant("rows.spfh", variant)
    dev = native.same_device(xyz4, normals, idx, row_start, total)
    xyz4, normals, idx = xyz4.contiguous(), normals.contiguous(), idx.contiguous()
    row_start, total = row_start.contiguous(), total.contiguous()
    out, raw = extension.outputs(dev, guard, prefill)
    hist = out("spfh", B * N * SPFH_WORDS, torch.int32).view(B, N, 3, 12)
    a = RowsSpfhArgs(ptr(xyz4), ptr(normals), ptr(idx), ptr(row_start), ptr(total), B, N, capacity, m, v, ptr(hist))
    native.check(lib().vcr_rows_spfh_f32(C.byref(a), native.stream_ptr()), "vcr_rows_spfh_f32")
    return (hist, raw) if guard or prefill is not None else hist


@native._guarded
def fpfh(xyz4, idx, row_start, total, spfh, max_nn=None, variant=0, guard=0, prefill=None):
    """vcr_rows_fpfh_f32 on xyz4 [B,N,4], the CSR rows and spfh int32 [B,N,3,12] (``spfh`` above, for the same rows and max_nn)
    -> float32 [B,33,N].  variant, guard / prefill: as ``spfh``'s."""
    B, N, capacity, m = _take("rows.fpfh", xyz4, idx, row_start, total, max_nn)
    if not (torch.is_tensor(spfh) and spfh.dtype == torch.int32 and tuple(spfh.shape) == (B, N, 3, 12)):
        raise VcrHipError(f"rows.fpfh: spfh must be int32 [B, N, 3, 12] with B, N = {B}, {N}")
    v = _variant("rows.fpfh", variant)
    dev = native.same_device(xyz4, idx, row_start, total, spfh)
    xyz4, idx, spfh = xyz4.contiguous(), idx.contiguous(), spfh.contiguous()
    row_start, total = row_start.contiguous(), total.contiguous()
    out, raw = extension.outputs(dev, guard, prefill)
    feat = out("fpfh", B * 3 * BINS * N, torch.float32).view(B, 3 * BINS, N)
    a = RowsFpfhArgs(ptr(xyz4), ptr(idx), ptr(row_start), ptr(total), ptr(spfh), B, N, capacity, m, v, ptr(feat))
    native.check(lib().vcr_rows_fpfh_f32(C.byref(a), native.stream_ptr()), "vcr_rows_fpfh_f32")
    return (feat, raw) if guard or prefill is not None else feat


def radius_arguments(api, search, radius, max_nn, capacity):
    """What the public calls ask of (search, radius, max_nn, capacity) in front of everything else.  -> True under
    search="radius" (max_nn is then None or an integer >= 1), False otherwise (the caller goes on to grid.check_search)."""
    if search != "radius":
        if max_nn is not None or capacity is not None:
            raise VcrHipError(f'{api}: max_nn and capacity belong to search="radius", got search={search!r}')
        return False
    if radius is None:
        raise VcrHipError(f'{api}: search="radius" needs a radius')
    check_max_nn(api, max_nn)
    return True
