"""ctypes binding of include/cluster/vcr_hip_dbscan.h and the Python API on top of it: DBSCAN on the
device as the connected components of the core points' graph, over the ragged CSR rows ``search_radius`` returns --
vcr_rows_dbscan_f32 and its host-only vcr_rows_dbscan_form -- and vcr_cluster_largest_f32, which compacts a cloud to its largest
cluster through the outlier filters' tail.  ``cluster_dbscan`` is Open3D's call of that name; ``largest_cluster`` is the form in
which a registration pipeline uses it.

Like ``rows``, the header extends include/vcr_hip.h without touching it and this module keeps its own STRUCTS / SIGNATURES maps,
applied once to ``native.lib()`` on first use.  No CPU fallback, as everywhere."""
from __future__ import annotations

import ctypes as C
import torch

from . import extension, native, radius
from .native import VcrHipError, f32p, ptr
from .score import i32p

MAX_N = 131072
FORMS = {"lane": 1, "wave": 2}                             # VCR_DBSCAN_LANE / VCR_DBSCAN_WAVE: what ``variant`` forces
WAVE_HOOK = 131072                                         # VCR_DBSCAN_WAVE_HOOK / _LABEL: the row length the wave form starts at
WAVE_LABEL = 131072                                        # (no row is that long: as measured, only ``variant`` reaches the wave forms)
NOISE, NOT_SERVED = -1, -2                                 # VCR_DBSCAN_NOISE / VCR_DBSCAN_NOT_SERVED
_INT32_LIMIT = 1 << 31

i64p = C.c_void_p


class RowsDbscanArgs(native._Sized):
    _fields_ = [("struct_bytes", C.c_uint32), ("xyz", f32p), ("idx", i32p), ("row_start", i64p), ("total", i64p), ("B", C.c_int),
                ("N", C.c_int), ("capacity", C.c_int), ("min_points", C.c_int), ("variant", C.c_int), ("labels", i32p),
                ("n_clusters", i32p), ("core", i32p), ("sizes", i32p)]


class ClusterLargestArgs(native._Sized):
    _fields_ = [("struct_bytes", C.c_uint32), ("xyz", f32p), ("labels", i32p), ("sizes", i32p), ("B", C.c_int), ("N", C.c_int),
                ("points", f32p), ("count", i32p), ("index", i32p)]


STRUCTS = {"vcr_rows_dbscan_args": RowsDbscanArgs, "vcr_cluster_largest_args": ClusterLargestArgs}

# name -> (restype, [argtypes]): the prototypes of include/cluster/vcr_hip_dbscan.h (tests/test_dbscan_cpu.py holds them to it);
# the compaction has no form to report
SIGNATURES = {**extension.workspace_signatures("vcr_rows_dbscan", RowsDbscanArgs),
              **{n: s for n, s in extension.workspace_signatures("vcr_cluster_largest", ClusterLargestArgs).items()
                 if not n.endswith("_form")}}

lib = extension.typed_lib(SIGNATURES)                      # native.lib() with this module's entry points typed (once)


def form(B, N, capacity, min_points=1, cu_count=256, variant=0):
    """vcr_rows_dbscan_form and _workspace_bytes (host only): (the hook's form, the labels' form, workspace bytes), 1 = a lane
    a row, 2 = a wave a row."""
    a = RowsDbscanArgs(None, 0x1000, 0x2000, 0x3000, B, N, capacity, min_points, variant, 0x4000, 0x5000, None, None)
    L = lib()                                               # (the pointers are never dereferenced on the host)
    h, lb = C.c_int(0), C.c_int(0)
    native.check(L.vcr_rows_dbscan_form(C.byref(a), cu_count, C.byref(h), C.byref(lb)), "vcr_rows_dbscan_form")
    return h.value, lb.value, L.vcr_rows_dbscan_workspace_bytes(C.byref(a), cu_count)


def check_min_points(api, min_points):
    if isinstance(min_points, bool) or not isinstance(min_points, int) or min_points < 1:
        raise VcrHipError(f"{api}: min_points must be an integer >= 1, got {min_points!r}")
    return min_points


def _variant(api, variant):
    if variant in FORMS:
        return FORMS[variant]
    if isinstance(variant, bool) or variant not in (0, 1, 2):
        raise VcrHipError(f'{api}: variant must be 0 (the plan), "lane" or "wave", got {variant!r}')
    return int(variant)


@native._guarded
def cluster_rows(idx, row_start, total, N, min_points, xyz=None, want_core=False, want_sizes=False, variant=0, guard=0,
                 prefill=None):
    """vcr_rows_dbscan_f32 on the CSR rows idx int32 [B,capacity], row_start int64 [B,N+1], total int64 [B] (``search_radius``,
    or any caller's) -> dict of labels int32 [B,N] (the cluster from 0, -1 noise, -2 a cloud that is not served), n_clusters
    int32 [B] (-1 likewise) and, where asked, core int32 [B,N] (1 / 0) and sizes int32 [B,N] (slot c the members of cluster c,
    border points included).  xyz [B,3,N] float32: a point with a non-finite coordinate is never core and always -1.
    variant: 0 for the plan's forms, "lane" or "wave" to force one.  guard / prefill (tests): as voxel.voxel_grid's -- the
    buffers come back under "_raw", and the workspace is prefilled too."""
    api = "dbscan.cluster_rows"
    if isinstance(N, bool) or not isinstance(N, int) or not 1 <= N <= MAX_N:
        raise VcrHipError(f"{api}: N must be an integer in [1, {MAX_N}], got {N!r}")
    if not (torch.is_tensor(idx) and idx.dtype == torch.int32 and idx.dim() == 2 and idx.shape[0] >= 1):
        raise VcrHipError(f"{api}: idx must be int32 [B, capacity]")
    B, capacity = idx.shape
    if B * N >= _INT32_LIMIT or B * capacity >= _INT32_LIMIT:
        raise VcrHipError(f"{api}: B * N and B * capacity must be below 2^31, got B = {B}, N = {N}, capacity = {capacity}")
    if not (torch.is_tensor(row_start) and row_start.dtype == torch.int64 and tuple(row_start.shape) == (B, N + 1)):
        raise VcrHipError(f"{api}: row_start must be int64 [B, N + 1] with B, N = {B}, {N}")
    if not (torch.is_tensor(total) and total.dtype == torch.int64 and tuple(total.shape) == (B,)):
        raise VcrHipError(f"{api}: total must be int64 [B] with B = {B}")
    if xyz is not None and not (torch.is_tensor(xyz) and xyz.dtype == torch.float32 and tuple(xyz.shape) == (B, 3, N)):
        raise VcrHipError(f"{api}: xyz must be None or float32 [B, 3, N] with B, N = {B}, {N}")
    check_min_points(api, min_points)
    v = _variant(api, variant)
    dev = native.same_device(idx, row_start, total, xyz)
    idx, row_start, total = idx.contiguous(), row_start.contiguous(), total.contiguous()
    given = ptr(idx) if B * capacity > 0 else None          # (an empty tensor has no address to give)
    xyz = None if xyz is None else xyz.contiguous()
    xyz_p = ptr(xyz)
    out, raw = extension.outputs(dev, guard, prefill)
    o = {"labels": out("labels", B * N, torch.int32).view(B, N), "n_clusters": out("n_clusters", B, torch.int32)}
    if want_core:
        o["core"] = out("core", B * N, torch.int32).view(B, N)
    if want_sizes:
        o["sizes"] = out("sizes", B * N, torch.int32).view(B, N)
    a = RowsDbscanArgs(xyz_p, given, ptr(row_start), ptr(total), B, N, capacity, min_points, v, ptr(o["labels"]),
                       ptr(o["n_clusters"]), ptr(o.get("core")), ptr(o.get("sizes")))
    extension.call_with_workspace(lib(), "vcr_rows_dbscan", a, dev, prefill)
    if guard or prefill is not None:
        o["_raw"] = raw
    return o


@native._guarded
def largest_rows(xyz, labels, sizes, want_index=True, guard=0, prefill=None):
    """vcr_cluster_largest_f32 on xyz float32 [B,3,N], labels and sizes int32 [B,N] (``cluster_rows`` with want_sizes) -> dict
    of points float32 [B,3,N], count int32 [B] and index int32 [B,N], as outlier.radius_filter's.  guard / prefill: as above."""
    api = "largest_cluster"
    extension.check_cloud(api, "xyz", xyz)
    B, _, N = xyz.shape
    for name, t in (("labels", labels), ("sizes", sizes)):
        if not (torch.is_tensor(t) and t.dtype == torch.int32 and tuple(t.shape) == (B, N)):
            raise VcrHipError(f"{api}: {name} must be int32 [B, N] with B, N = {B}, {N}")
    if not 1 <= N <= MAX_N:
        raise VcrHipError(f"{api}: a cloud must have 1 ... {MAX_N} points, got {N}")
    if B < 1 or B * N >= _INT32_LIMIT:
        raise VcrHipError(f"{api}: B must be at least 1 and B * N below 2^31, got B = {B}, N = {N}")
    if not xyz.is_cuda:
        raise VcrHipError(f"{api} runs on the MI355X HIP path only; move the cloud to cuda (there is no CPU fallback by design)")
    dev = native.same_device(xyz, labels, sizes)
    xyz, labels, sizes = xyz.contiguous().float(), labels.contiguous(), sizes.contiguous()
    out, raw = extension.outputs(dev, guard, prefill)
    o = {"points": out("points", B * 3 * N, torch.float32).view(B, 3, N), "count": out("count", B, torch.int32)}
    if want_index:
        o["index"] = out("index", B * N, torch.int32).view(B, N)
    a = ClusterLargestArgs(ptr(xyz), ptr(labels), ptr(sizes), B, N, ptr(o["points"]), ptr(o["count"]), ptr(o.get("index")))
    extension.call_with_workspace(lib(), "vcr_cluster_largest", a, dev, prefill)
    if guard or prefill is not None:
        o["_raw"] = raw
    return o


def cluster_dbscan(xyz, eps, min_points, capacity=None, cell=None, want_core=False, want_sizes=False):
    """DBSCAN on every cloud of xyz [B,3,N] (device tensor, up to 131 072 points a cloud): Open3D's cluster_dbscan(eps,
    min_points), scikit-learn's DBSCAN(eps, min_samples).  Returns (labels, n_clusters), then core and sizes where asked:
      labels      int32 [B,N]  the point's cluster, from 0; -1 for noise
      n_clusters  int32 [B]
      core        int32 [B,N]  1 for a core point: one with at least min_points points within eps, itself included
      sizes       int32 [B,N]  slot c holds the number of members of cluster c, border points included; 0 behind n_clusters
    The clusters are the connected components of the core points under "within eps"; they are numbered by their lowest core
    index, ascending.  A border point (not core, within eps of a core point) takes the lowest label among the core points
    within its reach; that is where the sequential algorithm of Open3D and scikit-learn puts it too, so the labels are theirs.
    The neighbourhoods are ``search_radius(xyz, eps)``'s -- distances of differences in fp32, a point ON the sphere counts,
    copies of a point are neighbours at distance 0 -- so a cloud far from the origin needs no centring.  A point with a NaN or
    infinite coordinate is noise and nobody's neighbour.
    capacity=None costs ``search_radius``'s one host synchronisation; capacity=int (the slots of idx a cloud gets) none: a
    cloud whose neighbours, all rows together, exceed it comes back with every label -2 and n_clusters -1, the other clouds
    unaffected.  cell: the search grid's edge, as ``search_radius``'s (it never changes the result)."""
    api = "cluster_dbscan"
    radius._cloud(api, xyz)
    radius._radius(api, eps)
    check_min_points(api, min_points)
    idx, row_start, total = _search(api, xyz, eps, capacity, cell)
    o = cluster_rows(idx, row_start, total, xyz.shape[2], min_points, xyz=xyz.contiguous().float(), want_core=want_core,
                     want_sizes=want_sizes)
    return (o["labels"], o["n_clusters"]) + ((o["core"],) if want_core else ()) + ((o["sizes"],) if want_sizes else ())


def _search(api, xyz, eps, capacity, cell):
    """search_radius with its refusals under this call's name."""
    try:
        return radius.search_radius(xyz, eps, capacity=capacity, cell=cell)
    except VcrHipError as e:
        raise VcrHipError(str(e).replace("search_radius", api, 1)) from None


def largest_cluster(xyz, labels, sizes):
    """xyz [B,3,N] cut to the members of its largest cluster -- ``cluster_dbscan``'s labels and sizes (want_sizes=True) --
    the lowest label among clusters of equal size: (points, count, index) as ``remove_radius_outlier`` returns them, compacted
    in ascending index order without a host synchronisation; ``voxel.unpad(points, count)`` cuts the clouds to their sizes.
    A cloud with no cluster (or one that was not served) gives count 0."""
    o = largest_rows(xyz, labels, sizes)
    return o["points"], o["count"], o["index"]
