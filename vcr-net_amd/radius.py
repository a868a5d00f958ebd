"""ctypes binding of include/vcr_hip_radius.h and the Python API on top of it: ALL points within a radius
of every point of a cloud, searched on the cloud's uniform grid by vcr_grid_radius_f32 -- rows of varying length in CSR form,
ascending in (d2, index), d2 in difference form -- and the grid sibling of the radius outlier filter,
vcr_outlier_radius_grid_f32, which ``outlier.remove_radius_outlier(search="grid")`` runs.

The header extends include/vcr_hip.h without touching it, and so does this module for ``native``: its own STRUCTS / SIGNATURES
maps, in the same shape, applied once to ``native.lib()`` on first use.  No CPU fallback, as everywhere."""
from __future__ import annotations

import ctypes as C
import math
import torch

from . import extension, grid, gridnn, native, outlier
from .native import VcrHipError, f32p, ptr
from .score import i32p

MAX_N = 131072
MAX_NN = grid.MAX_K                                        # the hybrid search's cap: search_knn's k
CHUNK = 128                                                # VCR_RADIUS_CHUNK: keys of a row the wave form stages at a time
QUERIES = grid.QUERIES
SEARCHES = ("scan", "grid")                                # what remove_radius_outlier's ``search=`` takes
ORDER_FORMS = {"wave": 1, "lane": 2}                       # the ordering's forms (vcr_grid_radius_args.variant bits 4-7)
_INT32_LIMIT = 1 << 31

i64p = C.c_void_p


class GridRadiusArgs(native._Sized):
    _fields_ = [("struct_bytes", C.c_uint32), ("xyz", f32p), ("B", C.c_int), ("N", C.c_int), ("radius", C.c_float),
                ("cell", C.c_float), ("capacity", C.c_int), ("count", i32p), ("row_start", i64p), ("total", i64p),
                ("idx", i32p), ("d2", f32p), ("variant", C.c_int)]


NEW_STRUCTS = {"vcr_grid_radius_args": GridRadiusArgs}     # what the header itself defines
STRUCTS = {**NEW_STRUCTS, "vcr_outlier_radius_args": outlier.RadiusArgs, **gridnn.NEW_STRUCTS}

_int, _intp = C.c_int, C.POINTER(C.c_int)

# name -> (restype, [argtypes]): the prototypes of include/vcr_hip_radius.h (tests/test_radius_cpu.py holds them to it); the
# search's _form reports three ints
SIGNATURES = {**extension.workspace_signatures("vcr_grid_radius", GridRadiusArgs),
              **extension.workspace_signatures2("vcr_outlier_radius_grid", outlier.RadiusArgs, gridnn.GridNnArgs)}
SIGNATURES["vcr_grid_radius_form"] = (_int, [C.POINTER(GridRadiusArgs), _int, _intp, _intp, _intp])

lib = extension.typed_lib(SIGNATURES)                      # native.lib() with this module's entry points typed (once)


def variant(order: int = 0, form: int = 0) -> int:
    """vcr_grid_radius_args.variant (VCR_RADIUS_VARIANT): order 1 serves the queries in cell order (the plan's), 2 in index
    order; form 1 orders a row by a wave, 2 by a lane; 0 = the plan's."""
    return int(order) | int(form) << 4


def radius_form(B, N, capacity=0, with_idx=True, cu_count=256, variant=0, radius=1.0, cell=0.0):
    """vcr_grid_radius_form (host only): (cells per cloud, queries per workgroup, the ordering's form, workspace bytes) of
    vcr_grid_radius_f32 on [B,3,N] with `capacity` slots a cloud."""
    a = GridRadiusArgs(0x1000, B, N, radius, cell, capacity, 0x2000, 0x3000, 0x4000, 0x5000 if with_idx else None, None,
                       variant)                             # (never dereferenced on the host)
    L = lib()
    cells, queries, form = C.c_int(0), C.c_int(0), C.c_int(0)
    native.check(L.vcr_grid_radius_form(C.byref(a), cu_count, C.byref(cells), C.byref(queries), C.byref(form)),
                 "vcr_grid_radius_form")
    return cells.value, queries.value, form.value, L.vcr_grid_radius_workspace_bytes(C.byref(a), cu_count)


def filter_grid_form(B, N, order=0, cell=0.0, cu_count=256, radius=1.0):
    """vcr_outlier_radius_grid_form (host only): (cells per cloud, order taken, queries per workgroup, workspace bytes)."""
    a = outlier.RadiusArgs(0x1000, B, N, radius, 0, 0x2000, 0x3000, None, None, 0)
    return gridnn.form("vcr_outlier_radius_grid", a, gridnn.grid_args(cell, order), cu_count)


def _radius(api, radius):
    """The radius as a float whose fp32 square is finite."""
    try:
        r = float(radius)
    except (TypeError, ValueError):
        r = float("nan")
    r2 = float(torch.tensor(r, dtype=torch.float32) * torch.tensor(r, dtype=torch.float32)) if math.isfinite(r) else r
    if not (math.isfinite(r) and r > 0.0 and math.isfinite(r2)):
        raise VcrHipError(f"{api}: radius must be finite and > 0 with a finite square in fp32, got {radius!r}")
    return r, r2


def _cloud(api, xyz):
    extension.check_cloud(api, "xyz", xyz)
    N = xyz.shape[2]
    if not 1 <= N <= MAX_N:
        raise VcrHipError(f"{api}: a cloud must have 1 ... {MAX_N} points, got {N}")
    if xyz.shape[0] < 1 or xyz.shape[0] * N >= _INT32_LIMIT:
        raise VcrHipError(f"{api}: B must be at least 1 and B * N below 2^31, got B = {xyz.shape[0]}, N = {N}")


def _on_device(api, x):
    if not x.is_cuda:
        raise VcrHipError(f"{api} runs on the MI355X HIP path only; move the cloud to cuda (there is no CPU fallback by design)")


@native._guarded
def grid_radius(xyz, radius, capacity=0, want_idx=True, want_d2=True, cell=0.0, variant=0, guard=0, prefill=None):
    """vcr_grid_radius_f32 on xyz [B,3,N] (device, fp32) -> dict of count int32 [B,N], row_start int64 [B,N+1], total int64 [B]
    and, with want_idx, idx int32 [B,capacity] (with want_d2 also d2 float32 [B,capacity]): cloud b's rows where total[b] <=
    capacity, -1 / +inf behind them and over a cloud that does not fit.  want_idx=False is the count-only call (capacity 0).
    cell: 0 for the radius, otherwise the cells' edge (the result does not depend on it).
    guard / prefill (tests): as voxel.voxel_grid's -- the buffers come back under "_raw"."""
    api = "search_radius"
    extension.check_cloud(api, "xyz", xyz)
    radius, _ = _radius(api, radius)
    cell = float(cell)
    if not (math.isfinite(cell) and cell >= 0.0):
        raise VcrHipError(f"{api}: cell must be None (the radius) or finite and > 0, got {cell}")
    capacity = int(capacity)
    _on_device(api, xyz)
    dev = xyz.device
    B, _, N = xyz.shape
    xyz = xyz.contiguous().float()
    out, raw = extension.outputs(dev, guard, prefill)
    o = {"count": out("count", B * N, torch.int32).view(B, N),
         "row_start": out("row_start", B * (N + 1), torch.int64).view(B, N + 1), "total": out("total", B, torch.int64)}
    cap = max(capacity, 0)
    if want_idx:
        o["idx"] = out("idx", B * cap, torch.int32).view(B, cap)
        if want_d2:
            o["d2"] = out("d2", B * cap, torch.float32).view(B, cap)
    # (an empty tensor has no address to give: capacity 0 is the count-only call)
    given = want_idx and B * cap > 0
    a = GridRadiusArgs(ptr(xyz), B, N, radius, cell, capacity, ptr(o["count"]), ptr(o["row_start"]), ptr(o["total"]),
                       ptr(o["idx"]) if given else None, ptr(o.get("d2")) if given else None, int(variant))
    extension.call_with_workspace(lib(), "vcr_grid_radius", a, dev, prefill)
    if guard or prefill is not None:
        o["_raw"] = raw
    return o


@native._guarded
def radius_filter_grid(xyz, radius, nb_points, cell=0.0, order=0, want_trace=True, guard=0, prefill=None):
    """vcr_outlier_radius_grid_f32 on xyz [B,3,N] (device, fp32) -> outlier.radius_filter's dict, bit for bit, with the count
    taken on the cloud's grid.  cell: 0 for the radius; order: 0 / 1 cell order, 2 index order."""
    api = "remove_radius_outlier"
    extension.check_cloud(api, "xyz", xyz)
    radius, _ = _radius(api, radius)
    if outlier._integer(nb_points) is None or nb_points < 0:
        raise VcrHipError(f"{api}: nb_points must be an integer >= 0, got {nb_points}")
    _on_device(api, xyz)
    dev = xyz.device
    B, _, N = xyz.shape
    xyz = xyz.contiguous().float()
    out, raw = extension.outputs(dev, guard, prefill)
    o = {"points": out("points", B * 3 * N, torch.float32).view(B, 3, N), "count": out("count", B, torch.int32),
         "index": out("index", B * N, torch.int32).view(B, N)}
    if want_trace:
        o["neighbours"] = out("neighbours", B * N, torch.int32).view(B, N)
    a = outlier.RadiusArgs(ptr(xyz), B, N, radius, int(nb_points), ptr(o["points"]), ptr(o["count"]), ptr(o["index"]),
                           ptr(o.get("neighbours")), 0)
    extension.call_with_workspace(lib(), "vcr_outlier_radius_grid", a, dev, prefill, second=gridnn.grid_args(cell, order))
    if guard or prefill is not None:
        o["_raw"] = raw
    return o


def _hybrid(xyz, r2, m, want_d2, cell, capacity, queries=None):
    """The first min(n_i, m) entries of every radius row, from search_knn's rows cut at r2 and compacted to CSR by torch ops."""
    api = "search_radius"
    idx, d2 = grid.search_knn(xyz, m, want_d2=True, cell=cell, queries=queries)
    B, N, _ = idx.shape
    hit = d2 <= r2                                          # (a short row's slots hold +inf; the rows ascend: a prefix)
    count = hit.sum(dim=2)
    row_start = torch.zeros(B, N + 1, dtype=torch.int64, device=idx.device)
    torch.cumsum(count, dim=1, out=row_start[:, 1:])
    total = row_start[:, N].clone()
    if capacity is None:
        capacity = int(total.max())                        # the ONE host synchronisation
    if B * capacity >= _INT32_LIMIT:
        raise VcrHipError(f"{api}: B * capacity = {B * capacity} slots are beyond 2^31")
    # every slot is written once: a hit of a cloud that fits goes to its place, everything else to a slot behind the end
    flat_idx = torch.full((B * capacity + 1,), -1, dtype=torch.int32, device=idx.device)
    flat_d2 = torch.full((B * capacity + 1,), float("inf"), dtype=torch.float32, device=idx.device) if want_d2 else None
    fits = (total <= capacity).view(B, 1, 1)
    place = (torch.arange(B, device=idx.device).view(B, 1, 1) * capacity + row_start[:, :N, None]
             + torch.arange(m, device=idx.device).view(1, 1, m))
    place = torch.where(hit & fits, place, torch.full_like(place, B * capacity)).reshape(-1)
    spill = torch.full((1,), -1, dtype=torch.int32, device=idx.device)
    flat_idx.scatter_(0, place, torch.where(hit & fits, idx, spill).reshape(-1))
    out_idx = flat_idx[:B * capacity].view(B, capacity)
    if not want_d2:
        return out_idx, row_start, total
    flat_d2.scatter_(0, place, torch.where(hit & fits, d2, torch.full_like(d2, float("inf"))).reshape(-1))
    return out_idx, row_start, total, flat_d2[:B * capacity].view(B, capacity)


def search_radius(xyz, radius, max_nn=None, want_d2=False, cell=None, capacity=None, queries=None):
    """ALL points within radius of every point of xyz [B,3,N] (device tensor, up to 131 072 points a cloud) among the cloud's
    other points, exactly: Open3D's search_radius_vector_3d for every point at once.  Returns (idx, row_start, total), with
    want_d2 (idx, row_start, total, d2):
      row_start  int64 [B,N+1]      point i's neighbours are idx[b, row_start[b, i] : row_start[b, i + 1]]
      total      int64 [B]          = row_start[:, N]: the neighbours of cloud b, all rows together
      idx        int32 [B,capacity] every row in ascending order of (distance, index); -1 behind total[b]
      d2         float32 [B,capacity] the squared distances; +inf behind total[b]
    The distance is that of ``search_knn``: dx^2 + dy^2 + dz^2 of the coordinates' DIFFERENCES in fp32, so a cloud far from the
    origin needs no centring.  A point ON the sphere (d2 <= radius * radius, the fp32 product) is a neighbour; a point is
    excluded from its own row by its index, so copies of it are neighbours at distance 0; a point with a NaN or infinite
    coordinate has an empty row and is in nobody's row.
    capacity=None: the rows are counted first, the largest total is read back -- ONE host synchronisation -- and the search
    runs again with exactly that capacity: the grid is built and the cloud is counted twice.  capacity=int: one call and no
    synchronisation; a cloud whose total exceeds it comes back with every idx -1 (d2 +inf) and its true row_start and total --
    compare total with capacity.
    max_nn=m (1 <= m <= 62, m + 1 <= N): Open3D's hybrid search without the point itself -- every row cut to its first
    min(n_i, m) entries, row_start and total those of the cut rows.  It is served from ``search_knn(xyz, m)``.
    The rows are ordered by a rank sort whose cost is quadratic in a row's length: meant for neighbourhoods.
    The search walks a uniform grid built on the device whose edge is the radius; cell forces another
    edge, which changes the time and never the result.
    queries=[B,3,M] (device tensor, up to 131 072 positions a cloud) asks about THOSE positions instead of the cloud's own
    points: the same outputs with M for N -- row_start is [B,M+1], row i holds the points of xyz within
    radius of query i.  A query is a position, not an index: nothing is excluded, and a point that coincides with a query heads
    its row at distance 0.  A query with a NaN or infinite coordinate has an empty row.  max_nn=m needs no m + 1 <= N there."""
    api = "search_radius"
    _cloud(api, xyz)
    if queries is not None:
        from . import query
        query._pair(api, xyz, queries)
    radius, r2 = _radius(api, radius)
    B, _, N = xyz.shape
    if max_nn is not None:
        if isinstance(max_nn, bool) or not isinstance(max_nn, int) or not 1 <= max_nn <= MAX_NN:
            raise VcrHipError(f"{api}: max_nn must be None or an integer in [1, {MAX_NN}], got {max_nn!r}")
        if queries is None and max_nn + 1 > N:
            raise VcrHipError(f"{api}: max_nn + 1 = {max_nn + 1} neighbours need at least as many points, got N = {N}")
    if capacity is not None:
        if isinstance(capacity, bool) or not isinstance(capacity, int) or capacity < 0:
            raise VcrHipError(f"{api}: capacity must be None or an integer >= 0, got {capacity!r}")
        if B * capacity >= _INT32_LIMIT:
            raise VcrHipError(f"{api}: B * capacity = {B * capacity} slots are beyond 2^31")
    if cell is not None:
        try:
            cell = float(cell)
        except (TypeError, ValueError):
            cell = float("nan")
        if not (math.isfinite(cell) and cell > 0.0):
            raise VcrHipError(f"{api}: cell must be None (the radius) or finite and > 0, got {cell!r}")
    _on_device(api, xyz)
    if queries is not None:
        query._on_device(api, xyz, queries)
    if max_nn is not None:
        return _hybrid(xyz, r2, max_nn, want_d2, cell, capacity, queries)
    cell = 0.0 if cell is None else cell
    if queries is None:
        search = grid_radius
    else:
        def search(xyz, *a, **kw):
            return query.grid_radius(xyz, queries, *a, **kw)
    if capacity is None:
        counted = search(xyz, radius, 0, want_idx=False, cell=cell)
        capacity = int(counted["total"].max())             # the ONE host synchronisation
        if B * capacity >= _INT32_LIMIT:
            raise VcrHipError(f"{api}: the rows need B * {capacity} slots, beyond 2^31: search the clouds one at a time")
    o = search(xyz, radius, capacity, want_idx=True, want_d2=want_d2, cell=cell)
    return (o["idx"], o["row_start"], o["total"], o["d2"]) if want_d2 else (o["idx"], o["row_start"], o["total"])
