"""ctypes binding of include/query/vcr_hip_query.h and the Python API on top of it: neighbours of ANY
query positions in a cloud, searched on the cloud's uniform grid -- the k nearest points of every query (vcr_query_knn_f32) and
all points within a radius of it as rows of varying length in CSR form (vcr_query_radius_f32), both in (d2, index) order with d2
in difference form and no self exclusion: a query is a position, not an index.

``grid.search_knn(..., queries=)`` and ``radius.search_radius(..., queries=)`` run these; ``compute_point_cloud_distance`` is
Open3D's call of that name on the k = 1 search.

The header extends include/vcr_hip.h without touching it, and so does this module for ``native``: its own STRUCTS / SIGNATURES
maps, in the same shape, applied once to ``native.lib()`` on first use.  No CPU fallback, as everywhere."""
from __future__ import annotations

import ctypes as C
import math
import torch

from . import extension, native
from .native import VcrHipError, f32p, ptr
from .score import i32p

MAX_N = 131072                                             # VCR_QUERY_MAX_N: points a cloud, and queries a cloud
MAX_K = 62                                                 # VCR_QUERY_MAX_K
CHUNK = 128                                                # VCR_QUERY_CHUNK: keys of a row the ordering stages at a time
ORDERS = {"cell": 1, "index": 2}                           # the order the queries are served in (the structs' variant)
_INT32_LIMIT = 1 << 31

i64p = C.c_void_p


class QueryKnnArgs(native._Sized):
    _fields_ = [("struct_bytes", C.c_uint32), ("xyz", f32p), ("queries", f32p), ("B", C.c_int), ("N", C.c_int), ("M", C.c_int),
                ("k", C.c_int), ("cell", C.c_float), ("idx", i32p), ("d2", f32p), ("variant", C.c_int)]


class QueryRadiusArgs(native._Sized):
    _fields_ = [("struct_bytes", C.c_uint32), ("xyz", f32p), ("queries", f32p), ("B", C.c_int), ("N", C.c_int), ("M", C.c_int),
                ("radius", C.c_float), ("cell", C.c_float), ("capacity", C.c_int), ("count", i32p), ("row_start", i64p),
                ("total", i64p), ("idx", i32p), ("d2", f32p), ("variant", C.c_int)]


STRUCTS = {"vcr_query_knn_args": QueryKnnArgs, "vcr_query_radius_args": QueryRadiusArgs}

# name -> (restype, [argtypes]): the prototypes of include/query/vcr_hip_query.h (tests/test_query_cpu.py holds them to it)
SIGNATURES = {**extension.workspace_signatures("vcr_query_knn", QueryKnnArgs),
              **extension.workspace_signatures("vcr_query_radius", QueryRadiusArgs)}

lib = extension.typed_lib(SIGNATURES)                      # native.lib() with this module's entry points typed (once)


def knn_form(B, N, M, k, cu_count=256, variant=0):
    """vcr_query_knn_form (host only): (cells per cloud, the queries' order, workspace bytes) of vcr_query_knn_f32."""
    a = QueryKnnArgs(0x1000, 0x2000, B, N, M, k, 0.0, 0x3000, None, variant)     # (never dereferenced on the host)
    return extension.form(lib(), "vcr_query_knn", a, cu_count)


def radius_form(B, N, M, capacity=0, with_idx=True, cu_count=256, variant=0, radius=1.0, cell=0.0):
    """vcr_query_radius_form (host only): (cells per cloud, the queries' order, workspace bytes) of vcr_query_radius_f32."""
    a = QueryRadiusArgs(0x1000, 0x2000, B, N, M, radius, cell, capacity, 0x3000, 0x4000, 0x5000, 0x6000 if with_idx else None,
                        None, variant)                      # (never dereferenced on the host)
    return extension.form(lib(), "vcr_query_radius", a, cu_count)


def _pair(api, xyz, queries, names=("xyz", "queries")):
    """What can be said of the points and the queries before any other argument is looked at."""
    extension.check_cloud(api, names[0], xyz)
    extension.check_cloud(api, names[1], queries)
    B, _, N = xyz.shape
    M = queries.shape[2]
    if queries.shape[0] != B:
        raise VcrHipError(f"{api}: {names[0]} and {names[1]} must hold the same number of clouds, got {B} and "
                          f"{queries.shape[0]}")
    for name, n in zip(names, (N, M)):
        if not 1 <= n <= MAX_N:
            raise VcrHipError(f"{api}: {name} must have 1 ... {MAX_N} points a cloud, got {n}")
    if B < 1 or B * N >= _INT32_LIMIT or B * M >= _INT32_LIMIT:
        raise VcrHipError(f"{api}: B must be at least 1 and B * N, B * M below 2^31, got B = {B}, N = {N}, M = {M}")


def _cell(api, cell, default):
    cell = float(cell)
    if not (math.isfinite(cell) and cell >= 0.0):
        raise VcrHipError(f"{api}: cell must be None ({default}) or finite and > 0, got {cell}")
    return cell


def _on_device(api, xyz, queries):
    if not (xyz.is_cuda and queries.is_cuda):
        raise VcrHipError(f"{api} runs on the MI355X HIP path only; move the clouds to cuda (there is no CPU fallback by design)")
    return native.same_device(xyz, queries)


@native._guarded
def grid_knn(xyz, queries, k, cell=0.0, want_d2=True, variant=0, guard=0, prefill=None):
    """vcr_query_knn_f32 on the points xyz [B,3,N] and the positions queries [B,3,M] (device, fp32) -> dict of idx int32 [B,M,k]
    and, with want_d2, d2 float32 [B,M,k]: per query its k nearest points in (d2, index) order, -1 and +inf where there are fewer.
    cell: 0 for the automatic grid, otherwise the cells' edge; variant: 0 the plan's, 1 the queries in cell order, 2 in index
    order (the result depends on neither).
    guard / prefill (tests): as voxel.voxel_grid's -- the buffers come back under "_raw"."""
    api = "search_knn"
    _pair(api, xyz, queries)
    cell = _cell(api, cell, "the automatic grid")
    dev = _on_device(api, xyz, queries)
    B, _, N = xyz.shape
    M = queries.shape[2]
    k = int(k)
    xyz, queries = xyz.contiguous().float(), queries.contiguous().float()
    out, raw = extension.outputs(dev, guard, prefill)
    o = {"idx": out("idx", B * M * max(k, 0), torch.int32).view(B, M, max(k, 0))}
    if want_d2:
        o["d2"] = out("d2", B * M * max(k, 0), torch.float32).view(B, M, max(k, 0))
    a = QueryKnnArgs(ptr(xyz), ptr(queries), B, N, M, k, cell, ptr(o["idx"]), ptr(o.get("d2")), int(variant))
    extension.call_with_workspace(lib(), "vcr_query_knn", a, dev, prefill)
    if guard or prefill is not None:
        o["_raw"] = raw
    return o


@native._guarded
def grid_radius(xyz, queries, radius, capacity=0, want_idx=True, want_d2=True, cell=0.0, variant=0, guard=0, prefill=None):
    """vcr_query_radius_f32 on the points xyz [B,3,N] and the positions queries [B,3,M] (device, fp32) -> dict of count int32
    [B,M], row_start int64 [B,M+1], total int64 [B] and, with want_idx, idx int32 [B,capacity] (with want_d2 also d2 float32
    [B,capacity]): cloud b's rows where total[b] <= capacity, -1 / +inf behind them and over a cloud that does not fit.
    want_idx=False is the count-only call (capacity 0).  cell: 0 for the radius, otherwise the cells' edge; variant as grid_knn's.
    guard / prefill (tests): as voxel.voxel_grid's -- the buffers come back under "_raw"."""
    from .radius import _radius
    api = "search_radius"
    _pair(api, xyz, queries)
    radius, _ = _radius(api, radius)
    cell = _cell(api, cell, "the radius")
    capacity = int(capacity)
    dev = _on_device(api, xyz, queries)
    B, _, N = xyz.shape
    M = queries.shape[2]
    xyz, queries = xyz.contiguous().float(), queries.contiguous().float()
    out, raw = extension.outputs(dev, guard, prefill)
    o = {"count": out("count", B * M, torch.int32).view(B, M),
         "row_start": out("row_start", B * (M + 1), torch.int64).view(B, M + 1), "total": out("total", B, torch.int64)}
    cap = max(capacity, 0)
    if want_idx:
        o["idx"] = out("idx", B * cap, torch.int32).view(B, cap)
        if want_d2:
            o["d2"] = out("d2", B * cap, torch.float32).view(B, cap)
    # (an empty tensor has no address to give: capacity 0 is the count-only call)
    given = want_idx and B * cap > 0
    a = QueryRadiusArgs(ptr(xyz), ptr(queries), B, N, M, radius, cell, capacity, ptr(o["count"]), ptr(o["row_start"]),
                        ptr(o["total"]), ptr(o["idx"]) if given else None, ptr(o.get("d2")) if given else None, int(variant))
    extension.call_with_workspace(lib(), "vcr_query_radius", a, dev, prefill)
    if guard or prefill is not None:
        o["_raw"] = raw
    return o


def compute_point_cloud_distance(src, tgt, want_index=False):
    """For every point of src [B,3,Ns] the distance to its nearest point of tgt [B,3,Nt] (device tensors, up to 131 072 points a
    cloud each): Open3D's compute_point_cloud_distance, float32 [B,Ns].  No cap, no host synchronisation.
    The value is the square root of ``search_knn(tgt, 1, want_d2=True, queries=src)``'s d2 -- the coordinates' DIFFERENCES in
    fp32, so clouds far from the origin need no centring -- and +inf for a source point with a NaN or infinite coordinate, or
    where tgt has no finite point.  want_index: also the neighbour's index in tgt, int32 [B,Ns] (-1 there), as a tuple
    (distance, index); among points at the same distance the lowest index."""
    api = "compute_point_cloud_distance"
    _pair(api, tgt, src, ("tgt", "src"))
    _on_device(api, tgt, src)
    o = grid_knn(tgt, src, 1, want_d2=True)
    dist = torch.sqrt(o["d2"][:, :, 0])
    return (dist, o["idx"][:, :, 0].contiguous()) if want_index else dist
