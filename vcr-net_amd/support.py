"""ctypes binding of include/support/vcr_hip_support.h: normals and FPFH at M CENTRES over a SUPPORT cloud
of N points -- rows whose row i belongs to centre i (any position) and whose entries index the support, what
``search_radius(xyz, r, queries=q)`` returns: vcr_support_normals_f32, vcr_support_spfh_f32, vcr_support_needed_f32,
vcr_support_fpfh_f32 and the host-only vcr_support_form.  ``estimate_normals``, ``compute_fpfh_feature`` and ``register_features``
reach them through ``queries=`` / ``query_index=`` / ``describe="keypoints"``; ``plan`` is the one place that picks between the
two ways to get the support's histograms.

Like ``rows``, the header extends include/vcr_hip.h without touching it and this module keeps its own STRUCTS / SIGNATURES maps,
applied once to ``native.lib()`` on first use.  No CPU fallback, as everywhere."""
from __future__ import annotations

import ctypes as C
import torch

from . import extension, native
from .native import VcrHipError, f32p, ptr
from .rows import check_max_nn
from .score import i32p

MAX_N = 131072                                             # VCR_SUPPORT_MAX_N: N, M and R
SPFH_WORDS = 36                                            # VCR_SUPPORT_SPFH_WORDS
BINS = 11
FORMS = {"lane": 1, "wave": 2}                             # VCR_SUPPORT_LANE / VCR_SUPPORT_WAVE: what ``variant`` forces
WAVE_SPFH = 24                                             # VCR_SUPPORT_WAVE_SPFH: the row length the wave form starts at
WAVE_CENTRES = 32768                                       # VCR_SUPPORT_WAVE_CENTRES: ... and B * M up to which it is taken anyway
COVERAGE_PCT = 0                                           # VCR_SUPPORT_COVERAGE_PCT: "needed" up to this bound on the coverage
PLANS = ("all", "needed")

i64p = C.c_void_p
u32p = C.c_void_p


class SupportNormalsArgs(native._Sized):
    _fields_ = [("struct_bytes", C.c_uint32), ("xyz4", f32p), ("c4", f32p), ("idx", i32p), ("row_start", i64p), ("total", i64p),
                ("self", i32p), ("B", C.c_int), ("N", C.c_int), ("M", C.c_int), ("capacity", C.c_int), ("max_nn", C.c_int),
                ("viewpoint", f32p), ("normals", f32p), ("curvature", f32p)]


class SupportSpfhArgs(native._Sized):
    _fields_ = [("struct_bytes", C.c_uint32), ("xyz4", f32p), ("normals", f32p), ("c4", f32p), ("centre_normals", f32p),
                ("idx", i32p), ("row_start", i64p), ("total", i64p), ("self", i32p), ("B", C.c_int), ("N", C.c_int), ("M", C.c_int),
                ("capacity", C.c_int), ("max_nn", C.c_int), ("variant", C.c_int), ("spfh", u32p)]


class SupportNeededArgs(native._Sized):
    _fields_ = [("struct_bytes", C.c_uint32), ("xyz4", f32p), ("c4", f32p), ("idx", i32p), ("row_start", i64p), ("total", i64p),
                ("self", i32p), ("B", C.c_int), ("N", C.c_int), ("M", C.c_int), ("capacity", C.c_int), ("max_nn", C.c_int),
                ("points", f32p), ("count", i32p), ("index", i32p), ("slot", i32p)]


class SupportFpfhArgs(native._Sized):
    _fields_ = [("struct_bytes", C.c_uint32), ("xyz4", f32p), ("c4", f32p), ("idx", i32p), ("row_start", i64p), ("total", i64p),
                ("self", i32p), ("slot", i32p), ("support_spfh", u32p), ("centre_spfh", u32p), ("B", C.c_int), ("N", C.c_int),
                ("M", C.c_int), ("R", C.c_int), ("capacity", C.c_int), ("max_nn", C.c_int), ("fpfh", f32p)]


STRUCTS = {"vcr_support_normals_args": SupportNormalsArgs, "vcr_support_spfh_args": SupportSpfhArgs,
           "vcr_support_needed_args": SupportNeededArgs, "vcr_support_fpfh_args": SupportFpfhArgs}

_int, _intp = C.c_int, C.POINTER(C.c_int)

# name -> (restype, [argtypes]): the prototypes of include/support/vcr_hip_support.h (tests/test_support_cpu.py holds them to it)
SIGNATURES = {"vcr_support_normals_f32": (_int, [C.POINTER(SupportNormalsArgs), C.c_void_p]),
              "vcr_support_spfh_f32": (_int, [C.POINTER(SupportSpfhArgs), C.c_void_p]),
              "vcr_support_needed_workspace_bytes": (C.c_size_t, [C.POINTER(SupportNeededArgs), _int]),
              "vcr_support_needed_f32": (_int, [C.POINTER(SupportNeededArgs), C.c_void_p, C.c_size_t, C.c_void_p]),
              "vcr_support_fpfh_f32": (_int, [C.POINTER(SupportFpfhArgs), C.c_void_p]),
              "vcr_support_form": (_int, [_int, _int, _int, _int, _int, _int, _int, _intp])}

lib = extension.typed_lib(SIGNATURES)                      # native.lib() with this module's entry points typed (once)


def form(B, N, M, capacity, max_nn=0, cu_count=256, variant=0):
    """vcr_support_form (host only): the first pass's form, 1 = a lane a centre, 2 = a wave a centre: the wave form where
    B * M <= WAVE_CENTRES or est = capacity / M (cut at max_nn) >= WAVE_SPFH."""
    s = C.c_int(0)
    native.check(lib().vcr_support_form(B, N, M, capacity, max_nn, cu_count, variant, C.byref(s)), "vcr_support_form")
    return s.value


def plan(N, M, capacity=None, max_nn=None, normals_given=True, support=None):
    """THE one place that picks how compute_fpfh_feature(queries=) gets the support's histograms (host only): "all" -- a self
    search of the whole support and its histograms --, or "needed" -- only the points the centres' rows hold.  support forces
    either ("needed" without given normals is refused: estimating them would take neighbours of neighbours of neighbours).
    None decides: "all" where the normals are estimated; otherwise by the bound on the coverage the host can see,
    min(N, est * M) / N with est = capacity / M cut at max_nn, "needed" up to COVERAGE_PCT per cent; without a capacity there
    is no est, and "all" is taken.  As measured (profiles/support_bench.txt) "needed" won at no coverage from 9 % up, at M =
    N / 100 included, so COVERAGE_PCT is 0 and None means "all" wherever a centre has a row."""
    if support is not None and (not isinstance(support, str) or support not in PLANS):
        raise VcrHipError(f'compute_fpfh_feature: support must be None, "all" or "needed", got {support!r}')
    if support == "needed" and not normals_given:
        raise VcrHipError('compute_fpfh_feature: support="needed" needs the support\'s normals (normals=None would estimate them '
                          'from neighbours of neighbours of neighbours); give normals or take support="all"')
    if support is not None:
        return support
    if not normals_given:
        return "all"
    first = capacity[0] if isinstance(capacity, tuple) else capacity
    if first is None:
        return "all"
    est = first // M
    if max_nn:
        est = min(est, max_nn)
    return "needed" if min(N, est * M) * 100 <= COVERAGE_PCT * N else "all"


def _variant(api, variant):
    if variant in FORMS:
        return FORMS[variant]
    if isinstance(variant, bool) or variant not in (0, 1, 2):
        raise VcrHipError(f'{api}: variant must be 0 (the plan), "lane" or "wave", got {variant!r}')
    return int(variant)


def _take(api, xyz4, c4, idx, row_start, total, self_index, max_nn):
    """-> (B, N, M, capacity, max_nn as the C side takes it) of xyz4 [B,N,4], c4 [B,M,4], the CSR triple over the centres and
    the optional self_index int32 [B,M]."""
    if not (torch.is_tensor(xyz4) and xyz4.dim() == 3 and xyz4.shape[2] == 4 and xyz4.dtype == torch.float32):
        raise VcrHipError(f"{api}: xyz4 must be float32 [B, N, 4] rows")
    B, N, _ = xyz4.shape
    if not (torch.is_tensor(c4) and c4.dim() == 3 and c4.shape[2] == 4 and c4.dtype == torch.float32 and c4.shape[0] == B):
        raise VcrHipError(f"{api}: c4 must be float32 [B, M, 4] rows with B = {B}")
    M = c4.shape[1]
    if not (torch.is_tensor(idx) and idx.dtype == torch.int32 and idx.dim() == 2 and idx.shape[0] == B):
        raise VcrHipError(f"{api}: idx must be int32 [B, capacity] with B = {B}")
    if not (torch.is_tensor(row_start) and row_start.dtype == torch.int64 and tuple(row_start.shape) == (B, M + 1)):
        raise VcrHipError(f"{api}: row_start must be int64 [B, M + 1] with B, M = {B}, {M}")
    if not (torch.is_tensor(total) and total.dtype == torch.int64 and tuple(total.shape) == (B,)):
        raise VcrHipError(f"{api}: total must be int64 [B] with B = {B}")
    if self_index is not None and not (torch.is_tensor(self_index) and self_index.dtype == torch.int32
                                       and tuple(self_index.shape) == (B, M)):
        raise VcrHipError(f"{api}: self_index must be None or int32 [B, M] with B, M = {B}, {M}")
    return B, N, M, idx.shape[1], check_max_nn(api, max_nn)


def _c(*tensors):
    return [None if t is None else t.contiguous() for t in tensors]


def _idx_ptr(idx):
    return ptr(idx) if idx.numel() else None                # (an empty tensor has no address to give: capacity 0)


@native._guarded
def normals(xyz4, c4, idx, row_start, total, self_index=None, max_nn=None, viewpoint=None, want_curvature=True, guard=0,
            prefill=None):
    """vcr_support_normals_f32 on the support's rows xyz4 [B,N,4], the centres' rows c4 [B,M,4] (native.to_rows4) and the CSR
    rows over the centres idx int32 [B,capacity], row_start int64 [B,M+1], total int64 [B] (``search_radius(queries=)``) ->
    (normals float32 [B,3,M], curvature float32 [B,M] or None).  self_index int32 [B,M]: which support point a centre is, -1 for
    none (None: -1 everywhere).  max_nn: None for the whole row, m to end behind its m-th neighbour entry.  viewpoint [B,3].
    guard / prefill (tests): as rows.normals' -- the raw buffers come back as a third element."""
    B, N, M, capacity, m = _take("support.normals", xyz4, c4, idx, row_start, total, self_index, max_nn)
    dev = native.same_device(xyz4, c4, idx, row_start, total, self_index, viewpoint)
    xyz4, c4, idx, row_start, total, self_index = _c(xyz4, c4, idx, row_start, total, self_index)
    if viewpoint is not None:
        if tuple(viewpoint.shape) != (B, 3):
            raise VcrHipError(f"support.normals: viewpoint must be [B, 3] with B = {B}, got {tuple(viewpoint.shape)}")
        viewpoint = viewpoint.contiguous().float()
    out, raw = extension.outputs(dev, guard, prefill)
    nrm = out("normals", B * 3 * M, torch.float32).view(B, 3, M)
    cur = out("curvature", B * M, torch.float32).view(B, M) if want_curvature else None
    a = SupportNormalsArgs(ptr(xyz4), ptr(c4), _idx_ptr(idx), ptr(row_start), ptr(total), ptr(self_index), B, N, M, capacity, m,
                           ptr(viewpoint), ptr(nrm), ptr(cur))
    native.check(lib().vcr_support_normals_f32(C.byref(a), native.stream_ptr()), "vcr_support_normals_f32")
    return (nrm, cur, raw) if guard or prefill is not None else (nrm, cur)


@native._guarded
def spfh(xyz4, normals, c4, centre_normals, idx, row_start, total, self_index=None, max_nn=None, variant=0, guard=0, prefill=None):
    """vcr_support_spfh_f32: the centres' simplified histograms over their used neighbour entries -> int32 [B,M,3,12] (the
    header's uint32 words).  normals float32 [B,3,N] the support's, centre_normals float32 [B,3,M] the centres'.  variant: 0 for
    the plan's form, "lane" or "wave" to force one.  guard / prefill (tests): the raw buffers come back as a second element."""
    B, N, M, capacity, m = _take("support.spfh", xyz4, c4, idx, row_start, total, self_index, max_nn)
    if not (torch.is_tensor(normals) and normals.dtype == torch.float32 and tuple(normals.shape) == (B, 3, N)):
        raise VcrHipError(f"support.spfh: normals must be float32 [B, 3, N] with B, N = {B}, {N}")
    if not (torch.is_tensor(centre_normals) and centre_normals.dtype == torch.float32 and tuple(centre_normals.shape) == (B, 3, M)):
        raise VcrHipError(f"support.spfh: centre_normals must be float32 [B, 3, M] with B, M = {B}, {M}")
    v = _variant("support.spfh", variant)
    dev = native.same_device(xyz4, normals, c4, centre_normals, idx, row_start, total, self_index)
    xyz4, normals, c4, centre_normals, idx, row_start, total, self_index = _c(xyz4, normals, c4, centre_normals, idx, row_start,
                                                                            total, self_index)
    out, raw = extension.outputs(dev, guard, prefill)
    hist = out("spfh", B * M * SPFH_WORDS, torch.int32).view(B, M, 3, 12)
    a = SupportSpfhArgs(ptr(xyz4), ptr(normals), ptr(c4), ptr(centre_normals), _idx_ptr(idx), ptr(row_start), ptr(total),
                        ptr(self_index), B, N, M, capacity, m, v, ptr(hist))
    native.check(lib().vcr_support_spfh_f32(C.byref(a), native.stream_ptr()), "vcr_support_spfh_f32")
    return (hist, raw) if guard or prefill is not None else hist


@native._guarded
def needed(xyz4, c4, idx, row_start, total, self_index=None, max_nn=None, guard=0, prefill=None):
    """vcr_support_needed_f32: the support points the second pass will read -> dict of points float32 [B,3,N] (ascending by index,
    NaN behind the count), count int32 [B], index int32 [B,N] (-1 behind the count) and slot int32 [B,N] (a point's rank among
    the needed, -1 where it is not).  guard / prefill (tests): the raw buffers come back under "_raw"."""
    B, N, M, capacity, m = _take("support.needed", xyz4, c4, idx, row_start, total, self_index, max_nn)
    dev = native.same_device(xyz4, c4, idx, row_start, total, self_index)
    xyz4, c4, idx, row_start, total, self_index = _c(xyz4, c4, idx, row_start, total, self_index)
    out, raw = extension.outputs(dev, guard, prefill)
    o = {"points": out("points", B * 3 * N, torch.float32).view(B, 3, N), "count": out("count", B, torch.int32),
         "index": out("index", B * N, torch.int32).view(B, N), "slot": out("slot", B * N, torch.int32).view(B, N)}
    a = SupportNeededArgs(ptr(xyz4), ptr(c4), _idx_ptr(idx), ptr(row_start), ptr(total), ptr(self_index), B, N, M, capacity, m,
                          ptr(o["points"]), ptr(o["count"]), ptr(o["index"]), ptr(o["slot"]))
    L = lib()
    need = L.vcr_support_needed_workspace_bytes(C.byref(a), 0)
    if need == 0:                                            # refused: let the entry point say why
        native.check(L.vcr_support_needed_f32(C.byref(a), None, 0, native.stream_ptr()), "vcr_support_needed_f32")
        raise VcrHipError("vcr_support_needed_workspace_bytes: 0 for arguments vcr_support_needed_f32 accepts")
    ws = torch.empty(need + 256, dtype=torch.uint8, device=dev)
    if prefill is not None:
        ws.fill_(prefill)
    off = (-ws.data_ptr()) % 256
    native.check(L.vcr_support_needed_f32(C.byref(a), ws.data_ptr() + off, need, native.stream_ptr()), "vcr_support_needed_f32")
    if guard or prefill is not None:
        o["_raw"] = raw
    return o


@native._guarded
def fpfh(xyz4, c4, idx, row_start, total, support_spfh, centre_spfh, self_index=None, slot=None, max_nn=None, guard=0,
         prefill=None):
    """vcr_support_fpfh_f32: the weighted sum over the centres' used neighbour entries -> float32 [B,33,M].  support_spfh int32
    [B,R,3,12]: the support's histogram rows, support point j's at row slot[b,j] (slot int32 [B,N]; None: the identity, R = N);
    centre_spfh int32 [B,M,3,12]: the centres' own (``spfh`` above, for the same rows and max_nn).  guard / prefill: as
    ``spfh``'s."""
    B, N, M, capacity, m = _take("support.fpfh", xyz4, c4, idx, row_start, total, self_index, max_nn)
    if not (torch.is_tensor(support_spfh) and support_spfh.dtype == torch.int32 and support_spfh.dim() == 4
            and support_spfh.shape[0] == B and tuple(support_spfh.shape[2:]) == (3, 12)):
        raise VcrHipError(f"support.fpfh: support_spfh must be int32 [B, R, 3, 12] with B = {B}")
    R = support_spfh.shape[1]
    if not (torch.is_tensor(centre_spfh) and centre_spfh.dtype == torch.int32 and tuple(centre_spfh.shape) == (B, M, 3, 12)):
        raise VcrHipError(f"support.fpfh: centre_spfh must be int32 [B, M, 3, 12] with B, M = {B}, {M}")
    if slot is not None and not (torch.is_tensor(slot) and slot.dtype == torch.int32 and tuple(slot.shape) == (B, N)):
        raise VcrHipError(f"support.fpfh: slot must be None or int32 [B, N] with B, N = {B}, {N}")
    if slot is None and R != N:
        raise VcrHipError(f"support.fpfh: without a slot support_spfh must hold a row a support point, got R = {R}, N = {N}")
    dev = native.same_device(xyz4, c4, idx, row_start, total, support_spfh, centre_spfh, self_index, slot)
    xyz4, c4, idx, row_start, total, support_spfh, centre_spfh, self_index, slot = _c(
        xyz4, c4, idx, row_start, total, support_spfh, centre_spfh, self_index, slot)
    out, raw = extension.outputs(dev, guard, prefill)
    feat = out("fpfh", B * 3 * BINS * M, torch.float32).view(B, 3 * BINS, M)
    a = SupportFpfhArgs(ptr(xyz4), ptr(c4), _idx_ptr(idx), ptr(row_start), ptr(total), ptr(self_index), ptr(slot),
                        ptr(support_spfh), ptr(centre_spfh), B, N, M, R, capacity, m, ptr(feat))
    native.check(lib().vcr_support_fpfh_f32(C.byref(a), native.stream_ptr()), "vcr_support_fpfh_f32")
    return (feat, raw) if guard or prefill is not None else feat


# ------------------------------------------------------------------------------------------------------- the public calls' path

def query_arguments(api, xyz, queries, query_index):
    """What the public calls ask of (queries, query_index) behind the cloud's own checks -> (B, N, M)."""
    B, _, N = xyz.shape
    if queries is not None:
        extension.check_cloud(api, "queries", queries)
        if queries.shape[0] != B:
            raise VcrHipError(f"{api}: xyz and queries must hold the same number of clouds, got {B} and {queries.shape[0]}")
    M = queries.shape[2] if queries is not None else None
    if query_index is not None:
        if not (torch.is_tensor(query_index) and query_index.dtype == torch.int32 and query_index.dim() == 2
                and query_index.shape[0] == B and (M is None or query_index.shape[1] == M)):
            raise VcrHipError(f"{api}: query_index must be int32 [B, M] with B = {B}" + ("" if M is None else f", M = {M}"))
        M = query_index.shape[1]
    if not 1 <= M <= MAX_N:
        raise VcrHipError(f"{api}: queries must have 1 ... {MAX_N} points, got {M}")
    if not 1 <= N <= MAX_N:
        raise VcrHipError(f"{api}: a cloud must have 1 ... {MAX_N} points, got {N}")
    return B, N, M


def gather_positions(xyz, query_index):
    """xyz [B,3,N], query_index int32 [B,M] -> [B,3,M]: the indexed points, NaN where the index is outside [0, N)."""
    N = xyz.shape[2]
    ok = (query_index >= 0) & (query_index < N)
    at = torch.where(ok, query_index, torch.zeros_like(query_index)).long()
    got = torch.gather(xyz.float(), 2, at[:, None, :].expand(-1, 3, -1))
    return torch.where(ok[:, None, :], got, torch.full_like(got, float("nan")))


def _capacities(api, capacity):
    """capacity: None, an int for both searches or a pair (the queries' rows, the needed points' rows) -> the pair."""
    pair = capacity if isinstance(capacity, tuple) else (capacity, capacity)
    ok = len(pair) == 2 and all(c is None or (isinstance(c, int) and not isinstance(c, bool) and c >= 0) for c in pair)
    if not ok:
        raise VcrHipError(f"{api}: capacity must be None, an integer >= 0 or a pair of them (the queries' rows, the needed "
                          f"points' rows), got {capacity!r}")
    return pair


def query_normals_of(xyz, queries, radius, max_nn=None, capacity=None, viewpoint=None, want_curvature=False):
    """estimate_normals(queries=): call 1 over the query rows with no self index -- a point at the query's position is a point
    of its neighbourhood."""
    from .radius import search_radius
    csr = search_radius(xyz, radius, capacity=capacity, queries=queries)
    nrm, cur = normals(native.to_rows4(xyz), native.to_rows4(queries), *csr, max_nn=max_nn, viewpoint=viewpoint,
                       want_curvature=want_curvature)
    return (nrm, cur) if want_curvature else nrm


def _void(feat, *fits):
    """feat [B,33,M] with NaN over the clouds whose rows did not fit in a search (total > capacity): a device `where`."""
    bad = None
    for total, capacity in fits:
        over = total > capacity
        bad = over if bad is None else bad | over
    return torch.where(bad.view(-1, 1, 1), torch.full_like(feat, float("nan")), feat)


def fpfh_at(api, xyz, nrm, radius, max_nn, capacity, queries, query_index, query_normals, support, variant=0):
    """compute_fpfh_feature(queries= / query_index=): the two plans; they return the same bits."""
    from . import rows
    from .radius import search_radius
    B, N, M = query_arguments(api, xyz, queries, query_index)
    cq, cn = _capacities(api, capacity)
    which = plan(N, M, capacity=cq, max_nn=max_nn, normals_given=nrm is not None, support=support)
    if nrm is not None and (not torch.is_tensor(nrm) or tuple(nrm.shape) != (B, 3, N)):
        raise VcrHipError(f"{api}: normals must be [B, 3, N] like xyz {tuple(xyz.shape)}, got "
                          f"{tuple(nrm.shape) if torch.is_tensor(nrm) else type(nrm).__name__}")
    if query_normals is not None and (not torch.is_tensor(query_normals) or tuple(query_normals.shape) != (B, 3, M)):
        raise VcrHipError(f"{api}: query_normals must be [B, 3, M] with B, M = {B}, {M}")
    tensors = [t for t in (xyz, nrm, queries, query_index, query_normals) if t is not None]
    if not all(t.is_cuda for t in tensors):
        raise VcrHipError(f"{api} runs on the MI355X HIP path only; move the cloud, the queries and their normals to cuda "
                          "(there is no CPU fallback by design)")
    xyz = xyz.contiguous().float()
    if query_index is not None:
        query_index = query_index.contiguous()
    if queries is None:
        queries = gather_positions(xyz, query_index)
    queries = queries.contiguous().float()
    xyz4, c4 = native.to_rows4(xyz), native.to_rows4(queries)
    q_csr = search_radius(xyz, radius, capacity=cq, queries=queries)
    fits = [(q_csr[2], q_csr[0].shape[1])]
    if which == "all":
        s_csr = search_radius(xyz, radius, capacity=cn)
        fits.append((s_csr[2], s_csr[0].shape[1]))
        nrm = rows.normals(xyz4, *s_csr, max_nn=max_nn, want_curvature=False)[0] if nrm is None else nrm.contiguous().float()
        support_spfh, slot = rows.spfh(xyz4, nrm, *s_csr, max_nn=max_nn), None
    else:
        nrm = nrm.contiguous().float()
        need = needed(xyz4, c4, *q_csr, self_index=query_index, max_nn=max_nn)
        n_csr = search_radius(xyz, radius, capacity=cn, queries=need["points"])    # (the padding is NaN: those rows are empty)
        fits.append((n_csr[2], n_csr[0].shape[1]))
        n4 = native.to_rows4(need["points"])
        at = need["index"].clamp(min=0).long()
        n_nrm = torch.gather(nrm, 2, at[:, None, :].expand(-1, 3, -1)).contiguous()
        support_spfh = spfh(xyz4, nrm, n4, n_nrm, *n_csr, self_index=need["index"], max_nn=max_nn, variant=variant)
        slot = need["slot"]
    if query_normals is None:
        est = normals(xyz4, c4, *q_csr, max_nn=max_nn, want_curvature=False)[0]
        if query_index is None:
            query_normals = est
        else:                                                # a query with an index takes the support's normal there
            ok = (query_index >= 0) & (query_index < N)
            at = torch.where(ok, query_index, torch.zeros_like(query_index)).long()
            query_normals = torch.where(ok[:, None, :], torch.gather(nrm, 2, at[:, None, :].expand(-1, 3, -1)), est)
    query_normals = query_normals.contiguous().float()
    centre_spfh = spfh(xyz4, nrm, c4, query_normals, *q_csr, self_index=query_index, max_nn=max_nn, variant=variant)
    feat = fpfh(xyz4, c4, *q_csr, support_spfh, centre_spfh, self_index=query_index, slot=slot, max_nn=max_nn)
    return _void(feat, *fits)
