"""ctypes binding of include/vcr_hip_grid.h and the Python API on top of it: the exact k nearest neighbours of every point among
its cloud's other points, searched on a uniform grid by vcr_grid_knn_f32 -- the k smallest (d2, j) with
d2 in difference form, so the result holds for a cloud anywhere in space, and a point is never its own neighbour.

The header extends include/vcr_hip.h without touching it, and so does this module for ``native``: its own STRUCTS / SIGNATURES
maps, in the same shape, applied once to ``native.lib()`` on first use.  No CPU fallback, as everywhere."""
from __future__ import annotations

import ctypes as C
import math
import torch

from . import extension, native
from .native import VcrHipError, f32p, ptr
from .score import i32p

MAX_N = 131072
MAX_K = 62
QUERIES = 256                                              # VCR_GRID_QUERIES: the queries a workgroup serves
SEARCHES = ("knn", "grid")                                 # what the consumers' ``search=`` takes


def cells(N: int) -> int:
    """VCR_GRID_CELLS(N): the cells one cloud's grid may have."""
    return 2 * int(N) + 64


class GridKnnArgs(native._Sized):
    _fields_ = [("struct_bytes", C.c_uint32), ("xyz", f32p), ("B", C.c_int), ("N", C.c_int), ("k", C.c_int), ("cell", C.c_float),
                ("idx", i32p), ("d2", f32p), ("variant", C.c_int)]


STRUCTS = {"vcr_grid_knn_args": GridKnnArgs}

# name -> (restype, [argtypes]): the prototypes of include/vcr_hip_grid.h (tests/test_grid_cpu.py holds them to it)
SIGNATURES = extension.workspace_signatures("vcr_grid_knn", GridKnnArgs)

lib = extension.typed_lib(SIGNATURES)                      # native.lib() with this module's entry points typed (once)


def variant(order: int = 0) -> int:
    """vcr_grid_knn_args.variant: 1 serves the queries in cell order (the plan's), 2 in index order; 0 = the plan's."""
    return int(order)


def grid_form(B, N, k, cu_count=256, variant=0):
    """vcr_grid_knn_form (host only): (cells per cloud, queries per workgroup, workspace bytes) of vcr_grid_knn_f32 on [B,3,N]."""
    a = GridKnnArgs(0x1000, B, N, k, 0.0, 0x2000, None, variant)                 # (never dereferenced on the host)
    return extension.form(lib(), "vcr_grid_knn", a, cu_count)


def check_search(api, search):
    if search not in SEARCHES:
        raise VcrHipError(f'{api}: search must be "knn" or "grid", got {search!r}')


@native._guarded
def grid_knn(xyz, k, cell=0.0, want_d2=True, variant=0, guard=0, prefill=None):
    """vcr_grid_knn_f32 on xyz [B,3,N] (device, fp32) -> dict of idx int32 [B,N,k] and, with want_d2, d2 float32 [B,N,k]: per
    point its k nearest other points in (d2, index) order, the query's own index and +inf where there are fewer.
    cell: 0 for the automatic grid, otherwise the cells' edge (the result does not depend on it).
    guard / prefill (tests): as voxel.voxel_grid's -- the buffers come back under "_raw"."""
    api = "search_knn"
    extension.check_cloud(api, "xyz", xyz)
    cell = float(cell)
    if not (math.isfinite(cell) and cell >= 0.0):
        raise VcrHipError(f"{api}: cell must be None (the automatic grid) or finite and > 0, got {cell}")
    if not xyz.is_cuda:
        raise VcrHipError(f"{api} runs on the MI355X HIP path only; move the cloud to cuda (there is no CPU fallback by design)")
    dev = xyz.device
    B, _, N = xyz.shape
    k = int(k)
    xyz = xyz.contiguous().float()
    out, raw = extension.outputs(dev, guard, prefill)
    o = {"idx": out("idx", B * N * max(k, 0), torch.int32).view(B, N, max(k, 0))}
    if want_d2:
        o["d2"] = out("d2", B * N * max(k, 0), torch.float32).view(B, N, max(k, 0))
    a = GridKnnArgs(ptr(xyz), B, N, k, cell, ptr(o["idx"]), ptr(o.get("d2")), int(variant))
    extension.call_with_workspace(lib(), "vcr_grid_knn", a, dev, prefill)
    if guard or prefill is not None:
        o["_raw"] = raw
    return o


def search_knn(xyz, k, want_d2=False, cell=None, queries=None):
    """The k nearest neighbours of every point of xyz [B,3,N] (device tensor, up to 131 072 points a cloud) among the cloud's
    other points, exactly: int32 [B,N,k], per point in ascending order of (distance, index); with want_d2 also the squared
    distances, float32 [B,N,k], as a tuple (idx, d2).  No host synchronisation.  1 <= k <= 62 and k + 1 <= N.
    The distance is dx^2 + dy^2 + dz^2 of the coordinates' DIFFERENCES in fp32 (fmaf(dz, dz, fmaf(dy, dy, dx * dx))), so a cloud
    far from the origin needs no centring: moving a cloud by a translation that is exact in fp32 returns the same bits.  A point
    is excluded from its own row by its index: copies of it are neighbours at distance 0.  A point with a NaN or infinite
    coordinate is nobody's neighbour, and its own row -- like every slot a row cannot fill -- holds its own index and +inf.
    The search walks a uniform grid built on the device; cell forces the grid's edge (None: chosen from
    the cloud's bounds), which changes the time and never the result.
    queries=[B,3,M] (device tensor, up to 131 072 positions a cloud) asks about THOSE positions instead of the cloud's own
    points: int32 [B,M,k] (and float32 [B,M,k]), the k nearest points of xyz to every query in the same order and arithmetic
    (DESIGN.md section 4.28).  A query is a position, not an index: a point that coincides with it is its first neighbour at
    distance 0.  k may exceed N: a slot a row cannot fill -- and every slot of a query with a NaN or infinite coordinate --
    holds -1 and +inf.  E.g. carrying labels from a down-sampled cloud back to the full one:
        down, count, _ = voxel_down_sample(full, voxel)        # (NaN behind count[b]: in nobody's row)
        labels, _ = cluster_dbscan(down, eps, min_points)
        nearest = search_knn(down, 1, queries=full)[:, :, 0]
        full_labels = torch.where(nearest >= 0, labels.gather(1, nearest.clamp(min=0).long()), -1)"""
    api = "search_knn"
    extension.check_cloud(api, "xyz", xyz)
    if isinstance(k, bool) or not isinstance(k, int) or not 1 <= k <= MAX_K:
        raise VcrHipError(f"{api}: k must be an integer in [1, {MAX_K}], got {k!r}")
    if queries is not None:
        return _search_queries(api, xyz, queries, k, want_d2, cell)
    N = xyz.shape[2]
    if k + 1 > N:
        raise VcrHipError(f"{api}: k + 1 = {k + 1} neighbours need at least as many points, got N = {N}")
    if N > MAX_N:
        raise VcrHipError(f"{api}: a cloud must have 1 ... {MAX_N} points, got {N}")
    if cell is not None:
        cell = float(cell)
        if not (math.isfinite(cell) and cell > 0.0):
            raise VcrHipError(f"{api}: cell must be None (the automatic grid) or finite and > 0, got {cell}")
    o = grid_knn(xyz, k, 0.0 if cell is None else cell, want_d2=want_d2)
    return (o["idx"], o["d2"]) if want_d2 else o["idx"]


def _search_queries(api, xyz, queries, k, want_d2, cell):
    """search_knn's cross search: the rows of the positions `queries` among the points xyz (query.grid_knn)."""
    from . import query
    query._pair(api, xyz, queries)
    if cell is not None:
        cell = float(cell)
        if not (math.isfinite(cell) and cell > 0.0):
            raise VcrHipError(f"{api}: cell must be None (the automatic grid) or finite and > 0, got {cell}")
    o = query.grid_knn(xyz, queries, k, 0.0 if cell is None else cell, want_d2=want_d2)
    return (o["idx"], o["d2"]) if want_d2 else o["idx"]
