"""ctypes binding of include/vcr_hip_fpfh.h and the Python API on top of it: a 33-bin Fast Point Feature
Histogram per point on the device -- Open3D's compute_fpfh_feature -- from the library's kNN and its normals: the simplified
histograms (vcr_spfh_f32) and their weighted sum over the neighbours (vcr_fpfh_f32).

Like ``plane`` and ``outlier``, the header extends include/vcr_hip.h without touching it and this module keeps its own STRUCTS /
SIGNATURES maps, applied once to ``native.lib()`` on first use.  No CPU fallback, as everywhere."""
from __future__ import annotations

import ctypes as C
import math
import torch

from . import extension, grid, native, plane, rows
from .native import VcrHipError, f32p, ptr
from .score import i32p

MAX_K = 62
BINS = 11                                                  # per group; three groups
ROW_BYTES = 48                                             # an SPFH row: three groups of 16 bytes
u8p = C.c_void_p                                           # device pointers travel as integers, like f32p


class SpfhArgs(native._Sized):
    _fields_ = [("struct_bytes", C.c_uint32), ("xyz4", f32p), ("normals", f32p), ("idx", i32p), ("B", C.c_int), ("N", C.c_int),
                ("k", C.c_int), ("radius", C.c_float), ("spfh", u8p)]


class FpfhArgs(native._Sized):
    _fields_ = [("struct_bytes", C.c_uint32), ("xyz4", f32p), ("idx", i32p), ("spfh", u8p), ("B", C.c_int), ("N", C.c_int),
                ("k", C.c_int), ("radius", C.c_float), ("fpfh", f32p)]


STRUCTS = {"vcr_spfh_args": SpfhArgs, "vcr_fpfh_args": FpfhArgs}

# name -> (restype, [argtypes]): the prototypes of include/vcr_hip_fpfh.h (tests/test_fpfh_cpu.py holds them to it)
SIGNATURES = {"vcr_spfh_f32": (C.c_int, [C.POINTER(SpfhArgs), C.c_void_p]),
              "vcr_fpfh_f32": (C.c_int, [C.POINTER(FpfhArgs), C.c_void_p])}

lib = extension.typed_lib(SIGNATURES)                      # native.lib() with this module's entry points typed (once)


def _rows_and_idx(api, xyz4, idx):
    if not (torch.is_tensor(xyz4) and xyz4.dim() == 3 and xyz4.shape[2] == 4 and xyz4.dtype == torch.float32):
        raise VcrHipError(f"{api}: xyz4 must be float32 [B, N, 4] rows")
    B, N, _ = xyz4.shape
    if not (torch.is_tensor(idx) and idx.dtype == torch.int32 and idx.dim() == 3 and tuple(idx.shape[:2]) == (B, N)):
        raise VcrHipError(f"{api}: idx must be int32 [B, N, k] with B, N = {B}, {N}")
    return B, N, idx.shape[2]


@native._guarded
def spfh(xyz4, normals, idx, radius=0.0, guard=0, prefill=None):
    """vcr_spfh_f32 on xyz4 [B,N,4] rows (native.to_rows4), normals float32 [B,3,N] (plane.normals) and idx int32 [B,N,k]
    (native.knn on those rows) -> uint8 [B,N,48]: per point three groups of 16 bytes -- the counts of 11 bins, the number of
    counted pairs, four zeros.  radius: 0 for the plain kNN neighbourhood, otherwise neighbours further away are dropped.
    guard / prefill (tests): as plane.normals' -- the raw buffers come back as a second element."""
    B, N, k = _rows_and_idx("spfh", xyz4, idx)
    if not (torch.is_tensor(normals) and normals.dtype == torch.float32 and tuple(normals.shape) == (B, 3, N)):
        raise VcrHipError(f"spfh: normals must be float32 [B, 3, N] with B, N = {B}, {N}")
    dev = native.same_device(xyz4, normals, idx)
    xyz4, normals, idx = xyz4.contiguous(), normals.contiguous(), idx.contiguous()
    out, raw = extension.outputs(dev, guard, prefill)
    hist = out("spfh", B * N * ROW_BYTES, torch.uint8).view(B, N, ROW_BYTES)
    a = SpfhArgs(ptr(xyz4), ptr(normals), ptr(idx), B, N, k, float(radius), ptr(hist))
    native.check(lib().vcr_spfh_f32(C.byref(a), native.stream_ptr()), "vcr_spfh_f32")
    return (hist, raw) if guard or prefill is not None else hist


@native._guarded
def fpfh(xyz4, idx, spfh, radius=0.0, guard=0, prefill=None):
    """vcr_fpfh_f32 on xyz4 [B,N,4], idx int32 [B,N,k] and spfh uint8 [B,N,48] (``spfh`` above, for the same rows, neighbours and
    radius) -> float32 [B,33,N].  guard / prefill (tests): as ``spfh``'s."""
    B, N, k = _rows_and_idx("fpfh", xyz4, idx)
    if not (torch.is_tensor(spfh) and spfh.dtype == torch.uint8 and tuple(spfh.shape) == (B, N, ROW_BYTES)):
        raise VcrHipError(f"fpfh: spfh must be uint8 [B, N, {ROW_BYTES}] with B, N = {B}, {N}")
    dev = native.same_device(xyz4, idx, spfh)
    xyz4, idx, spfh = xyz4.contiguous(), idx.contiguous(), spfh.contiguous()
    out, raw = extension.outputs(dev, guard, prefill)
    feat = out("fpfh", B * 3 * BINS * N, torch.float32).view(B, 3 * BINS, N)
    a = FpfhArgs(ptr(xyz4), ptr(idx), ptr(spfh), B, N, k, float(radius), ptr(feat))
    native.check(lib().vcr_fpfh_f32(C.byref(a), native.stream_ptr()), "vcr_fpfh_f32")
    return (feat, raw) if guard or prefill is not None else feat


def compute_fpfh_feature(xyz, normals=None, k=30, radius=None, want_normals=False, want_idx=False, search="knn", max_nn=None,
                         capacity=None, queries=None, query_index=None, query_normals=None, support=None):
    """The 33-bin Fast Point Feature Histogram of every point of xyz [B,3,N] (device tensor, up to 131 072 points a cloud) from
    its k nearest neighbours: Open3D's compute_fpfh_feature, in fp64 on the device.  Returns float32 [B,33,N] -- three groups
    of 11 bins, each group of a point summing to 200 where the point and a neighbour have pairs to count; with want_normals
    also the normals used, float32 [B,3,N]; with want_idx also the neighbours, int32 [B,N,k] -- as a tuple in that order.
    normals [B,3,N] (device): the points' normals; None estimates them with ``estimate_normals`` from the SAME k neighbours (one
    search serves both).  radius: None for the plain kNN neighbourhood; a positive number drops the neighbours further away
    than it (Open3D's hybrid search with max_nn = k + 1).  1 <= k <= 62 and k + 1 <= N.
    The neighbours are the library's kNN (native.knn on the points' rows, ties broken exactly), whose distance is the expansion
    2 x.y - |x|^2 - |y|^2 in fp32: for a cloud far from the origin relative to its spacing it cancels, and the neighbours are
    then not the nearest.  Centre such a cloud first (the features do not change under a translation):
    ``vcrnet_amd.centred(xyz)`` returns xyz - c and the centre c it took.
    search: "knn" is that search.  "grid" takes the neighbours (the normals' too) from ``search_knn``
    instead: distances of differences, so no centring is needed, and the point itself excluded by its index.  The faster one
    for large clouds.
    search="radius" (DESIGN.md section 4.23): the neighbourhood is ALL points within `radius` (``search_radius``, rows of any
    length: Open3D's KDTreeSearchParamRadius), or with max_nn=m (any integer >= 1) the nearest min(n_i, m) of them -- Open3D's
    KDTreeSearchParamHybrid(radius, max_nn = m + 1), without the 62 of k.  ONE ``search_radius(xyz, radius, capacity=capacity)``
    serves the normals (where they are not given) and both passes; k is not read; want_idx returns the (idx, row_start, total)
    triple.  max_nn and capacity belong to this search alone.
    queries / query_index (search="radius" alone): the features of M CENTRES over xyz as the SUPPORT
    cloud -> float32 [B,33,M]; PCL's setInputCloud(centres) + setSearchSurface(xyz).  queries [B,3,M] are positions, points of
    the cloud or not (voxel centroids over the full-resolution cloud, say).  query_index int32 [B,M] says which support point
    each query is, -1 for none; given without queries it gathers the positions, NaN where it is -1 --
    ``compute_iss_keypoints``' index can be passed directly, and a NaN centre's feature is NaN.  A query with an index has that
    point left out of its own neighbourhood, as in the self form: max_nn=m is "the nearest m OTHER points"; a query without one
    counts a point at its position in its simplified histogram (and skips it, at distance 0, in the weighted sum).
    query_normals [B,3,M]: the centres' normals; None takes the support's normal at the index where there is one and estimates
    the others from the query's own row.  With queries = xyz and query_index = arange the result is the self form's, bit for
    bit; a subset of indices returns the self form's columns.
    support: how the neighbours' histograms are obtained.  "all": one self search of the whole support and its histograms;
    only the centres' passes are M-sized.  "needed": the histograms of the points in the centres' rows alone -- the query
    search, a compaction of the needed points, a second query search from them --; it needs given `normals`.  None picks
    (``support.plan``).  Both return the same bits.  capacity there: None (one synchronisation a search), an int for both
    searches or a pair (the queries' rows, the needed points' or the support's rows): no synchronisation; a cloud whose rows
    did not fit in either search comes back all NaN and nothing raises.  want_normals and want_idx are not served there."""
    api = "compute_fpfh_feature"
    extension.check_cloud(api, "xyz", xyz)
    if queries is not None or query_index is not None or query_normals is not None or support is not None:
        from . import support as at
        if search != "radius":
            raise VcrHipError(f'{api}: queries, query_index, query_normals and support belong to search="radius", got '
                              f"search={search!r}")
        if queries is None and query_index is None:
            raise VcrHipError(f"{api}: query_normals and support belong to queries= or query_index=; neither is given")
        if want_normals or want_idx:
            raise VcrHipError(f"{api}: want_normals and want_idx are not served with queries= or query_index=")
        if radius is None:
            raise VcrHipError(f'{api}: search="radius" needs a radius')
        rows.check_max_nn(api, max_nn)
        return at.fpfh_at(api, xyz, normals, radius, max_nn, capacity, queries, query_index, query_normals, support)
    if rows.radius_arguments(api, search, radius, max_nn, capacity):
        return _compute_fpfh_radius(api, xyz, normals, radius, max_nn, capacity, want_normals, want_idx)
    grid.check_search(api, search)
    k = int(k)
    B, _, N = xyz.shape
    if k < 1 or k > MAX_K:
        raise VcrHipError(f"{api}: k must be in [1, {MAX_K}], got {k}")
    if k + 1 > N:
        raise VcrHipError(f"{api}: k + 1 = {k + 1} neighbours need at least as many points, got N = {N}")
    if normals is not None and (not torch.is_tensor(normals) or tuple(normals.shape) != (B, 3, N)):
        raise VcrHipError(f"{api}: normals must be [B, 3, N] like xyz {tuple(xyz.shape)}, got "
                          f"{tuple(normals.shape) if torch.is_tensor(normals) else type(normals).__name__}")
    if radius is not None:
        radius = float(radius)
        if not (math.isfinite(radius) and radius > 0.0):
            raise VcrHipError(f"{api}: radius must be positive and finite (None: the k nearest neighbours alone), got {radius}")
    if not xyz.is_cuda or (normals is not None and not normals.is_cuda):
        raise VcrHipError(f"{api} runs on the MI355X HIP path only; move the cloud and its normals to cuda "
                          "(there is no CPU fallback by design)")
    r = 0.0 if radius is None else radius
    if normals is None:
        normals, idx = plane.estimate_normals(xyz, k, want_idx=True, search=search)   # its search is this call's
        xyz4 = native.to_rows4(xyz)
    else:
        normals = normals.contiguous().float()
        xyz4 = native.to_rows4(xyz)
        idx = native.knn(xyz4, None, k) if search == "knn" else grid.search_knn(xyz, k)
    feat = fpfh(xyz4, idx, spfh(xyz4, normals, idx, r), r)
    res = (feat,) + ((normals,) if want_normals else ()) + ((idx,) if want_idx else ())
    return res[0] if len(res) == 1 else res


def _compute_fpfh_radius(api, xyz, normals, radius, max_nn, capacity, want_normals, want_idx):
    """compute_fpfh_feature(search="radius"): one search_radius, the rows' normals where none are given, the rows' two passes."""
    from .radius import search_radius
    B, _, N = xyz.shape
    if normals is not None and (not torch.is_tensor(normals) or tuple(normals.shape) != (B, 3, N)):
        raise VcrHipError(f"{api}: normals must be [B, 3, N] like xyz {tuple(xyz.shape)}, got "
                          f"{tuple(normals.shape) if torch.is_tensor(normals) else type(normals).__name__}")
    if not xyz.is_cuda or (normals is not None and not normals.is_cuda):
        raise VcrHipError(f"{api} runs on the MI355X HIP path only; move the cloud and its normals to cuda "
                          "(there is no CPU fallback by design)")
    csr = search_radius(xyz, radius, capacity=capacity)
    xyz4 = native.to_rows4(xyz)
    normals = rows.normals(xyz4, *csr, max_nn=max_nn, want_curvature=False)[0] if normals is None else normals.contiguous().float()
    feat = rows.fpfh(xyz4, *csr, rows.spfh(xyz4, normals, *csr, max_nn=max_nn), max_nn=max_nn)
    res = (feat,) + ((normals,) if want_normals else ()) + ((csr,) if want_idx else ())
    return res[0] if len(res) == 1 else res
