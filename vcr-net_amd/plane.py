"""ctypes binding of include/vcr_hip_plane.h and the Python API on top of it: a normal per point on
the device (vcr_normals_f32: Open3D's estimate_normals with a kNN search) and the point-to-plane refinement that needs them
(vcr_refine_plane_f32: registration_icp with TransformationEstimationPointToPlane, vcr_refine_f32's loop with another fit).

Like ``score`` and ``refine``, the header extends include/vcr_hip.h without touching it and this module keeps its own STRUCTS /
SIGNATURES maps, applied once to ``native.lib()`` on first use.  No CPU fallback, as everywhere."""
from __future__ import annotations

import ctypes as C
import torch

from . import extension, grid, native, refine, rows
from .native import VcrHipError, f32p, ptr
from .score import i32p

MAX_K = 62


class NormalsArgs(native._Sized):
    _fields_ = [("struct_bytes", C.c_uint32), ("xyz4", f32p), ("idx", i32p), ("B", C.c_int), ("N", C.c_int), ("k", C.c_int),
                ("viewpoint", f32p), ("normals", f32p), ("curvature", f32p)]


class RefinePlaneArgs(native._Sized):
    _fields_ = list(refine.RefineArgs._fields_) + [("tgt_normals", f32p)]      # vcr_refine_args' fields lead, in its order


STRUCTS = {"vcr_normals_args": NormalsArgs, "vcr_refine_plane_args": RefinePlaneArgs}

# name -> (restype, [argtypes]): the prototypes of include/vcr_hip_plane.h (tests/test_plane_cpu.py holds them to it)
SIGNATURES = {"vcr_normals_f32": (C.c_int, [C.POINTER(NormalsArgs), C.c_void_p]),
              **extension.workspace_signatures("vcr_refine_plane", RefinePlaneArgs)}

lib = extension.typed_lib(SIGNATURES)                      # native.lib() with this module's entry points typed (once)


def refine_plane_form(B, Ns, Nt, cu_count=256, variant=0, max_iterations=30):
    """vcr_refine_plane_form (host only with an explicit cu_count): (source points per lane, target splits, workspace bytes),
    as refine.refine_form."""
    a = RefinePlaneArgs(src=0x1000, tgt=0x2000, B=B, Ns=Ns, Nt=Nt, max_iterations=max_iterations, R_out=0x3000, t_out=0x4000,
                        fitness=0x5000, rmse=0x6000, variant=variant, tgt_normals=0x7000)   # (never dereferenced on the host)
    return extension.form(lib(), "vcr_refine_plane", a, cu_count)


@native._guarded
def normals(xyz4, idx, viewpoint=None, want_curvature=True, guard=0, prefill=None):
    """vcr_normals_f32 on xyz4 [B,N,4] rows (native.to_rows4) and idx int32 [B,N,k] (native.knn on those rows) ->
    (normals float32 [B,3,N], curvature float32 [B,N] or None).  viewpoint [B,3]: the normals look at it.
    guard / prefill (tests): as refine.refine's -- the raw buffers come back as a third element."""
    if not (torch.is_tensor(xyz4) and xyz4.dim() == 3 and xyz4.shape[2] == 4 and xyz4.dtype == torch.float32):
        raise VcrHipError("normals: xyz4 must be float32 [B, N, 4] rows")
    B, N, _ = xyz4.shape
    if not (torch.is_tensor(idx) and idx.dtype == torch.int32 and idx.dim() == 3 and tuple(idx.shape[:2]) == (B, N)):
        raise VcrHipError(f"normals: idx must be int32 [B, N, k] with B, N = {B}, {N}")
    k = idx.shape[2]
    dev = native.same_device(xyz4, idx, viewpoint)
    xyz4, idx = xyz4.contiguous(), idx.contiguous()
    if viewpoint is not None:
        if tuple(viewpoint.shape) != (B, 3):
            raise VcrHipError(f"normals: viewpoint must be [B, 3] with B = {B}, got {tuple(viewpoint.shape)}")
        viewpoint = viewpoint.contiguous().float()
    out, raw = extension.outputs(dev, guard, prefill)
    nrm = out("normals", B * 3 * N, torch.float32).view(B, 3, N)
    cur = out("curvature", B * N, torch.float32).view(B, N) if want_curvature else None
    a = NormalsArgs(ptr(xyz4), ptr(idx), B, N, k, ptr(viewpoint), ptr(nrm), ptr(cur))
    native.check(lib().vcr_normals_f32(C.byref(a), native.stream_ptr()), "vcr_normals_f32")
    return (nrm, cur, raw) if guard or prefill is not None else (nrm, cur)


def estimate_normals(xyz, k=20, viewpoint=None, want_curvature=False, want_idx=False, search="knn", radius=None, max_nn=None,
                     capacity=None, queries=None):
    """A unit normal per point of xyz [B,3,N] (device tensor) from its k nearest neighbours: the eigenvector of the smallest
    eigenvalue of the covariance of the point and those neighbours (Open3D's estimate_normals with a kNN search), in fp64 on
    the device.  Returns normals float32 [B,3,N]; with want_curvature also the surface variation lambda0 / (lambda0 + lambda1 +
    lambda2), float32 [B,N]; with want_idx also the neighbours, int32 [B,N,k] -- as a tuple in that order.
    viewpoint [B,3]: every normal looks at it (n . (viewpoint - x) >= 0); None: the component of largest magnitude is positive.
    No orientation is propagated between points here: ``orient_normals_consistent_tangent_plane`` does that.
    The neighbours are the library's kNN (native.knn on the points' rows, ties broken exactly), whose distance is the expansion
    2 x.y - |x|^2 - |y|^2 in fp32: for a cloud far from the origin relative to its spacing it cancels, and the neighbours are
    then not the nearest.  Centre such a cloud first (normals do not change under a translation):
    ``vcrnet_amd.centred(xyz)`` returns xyz - c and the centre c it took.
    search: "knn" is that search.  "grid" takes the neighbours from ``search_knn`` instead: distances
    of differences, so no centring is needed, and the point itself excluded by its index (among copies of a point the brute
    force drops whichever of them came first).  The faster one for large clouds.
    search="radius" (DESIGN.md section 4.23): the neighbours are ALL points within `radius` (``search_radius(xyz, radius,
    capacity=capacity)``, rows of any length; Open3D's KDTreeSearchParamRadius), or with max_nn=m (any integer >= 1) the nearest
    min(n_i, m) of them: Open3D's KDTreeSearchParamHybrid(radius, max_nn = m + 1) -- m counts OTHER points, as ``search_radius``
    does.  k is not read.  A point with fewer than two neighbours gets (0, 0, 1), curvature 0.  capacity: ``search_radius``'s
    (None reads the rows' total back once; an integer is one call without a synchronisation, and a cloud whose rows exceed it
    comes back NaN).  want_idx then returns the (idx, row_start, total) triple in idx's place.  radius, max_nn and capacity
    belong to this search alone.
    queries=[B,3,M] (search="radius" alone): the normals of the surface xyz AT those positions -> [B,3,M]
    (with want_curvature also [B,M]), each from the points within `radius` of the query (``search_radius(queries=)``), the
    viewpoint rule taken at the query's position.  A query is a position, not an index: a point at the query's position is a
    point of its neighbourhood, max_nn=m keeps the nearest m points, and fewer than three points give (0, 0, 1), curvature 0.
    A query with a NaN or infinite coordinate gets NaN.  want_idx is not served there."""
    if not torch.is_tensor(xyz) or xyz.dim() != 3 or xyz.shape[1] != 3:
        raise VcrHipError(f"estimate_normals: xyz must be a [B, 3, N] point cloud, got "
                          f"{tuple(xyz.shape) if torch.is_tensor(xyz) else type(xyz).__name__}")
    if queries is not None:
        return _estimate_normals_queries(xyz, search, radius, max_nn, capacity, viewpoint, want_curvature, want_idx, queries)
    if rows.radius_arguments("estimate_normals", search, radius, max_nn, capacity):
        return _estimate_normals_radius(xyz, radius, max_nn, capacity, viewpoint, want_curvature, want_idx)
    if radius is not None:
        raise VcrHipError(f'estimate_normals: radius belongs to search="radius", got search={search!r}')
    grid.check_search("estimate_normals", search)
    if not xyz.is_cuda:
        raise VcrHipError("estimate_normals runs on the MI355X HIP path only; move the cloud to cuda "
                          "(there is no CPU fallback by design)")
    k = int(k)
    N = xyz.shape[2]
    if k < 1 or k > MAX_K:
        raise VcrHipError(f"estimate_normals: k must be in [1, {MAX_K}], got {k}")
    if k + 1 > N:
        raise VcrHipError(f"estimate_normals: k + 1 = {k + 1} neighbours need at least as many points, got N = {N}")
    if viewpoint is not None and (not torch.is_tensor(viewpoint) or tuple(viewpoint.shape) != (xyz.shape[0], 3)
                                  or not viewpoint.is_cuda):
        raise VcrHipError(f"estimate_normals: viewpoint must be a device tensor [B, 3] with B = {xyz.shape[0]}")
    xyz4 = native.to_rows4(xyz)
    idx = native.knn(xyz4, None, k) if search == "knn" else grid.search_knn(xyz, k)
    nrm, cur = normals(xyz4, idx, viewpoint, want_curvature=want_curvature)
    res = (nrm,) + ((cur,) if want_curvature else ()) + ((idx,) if want_idx else ())
    return res[0] if len(res) == 1 else res


def _estimate_normals_queries(xyz, search, radius, max_nn, capacity, viewpoint, want_curvature, want_idx, queries):
    """estimate_normals(queries=): one search_radius from the queries, then vcr_support_normals_f32 on its rows."""
    from . import support
    api = "estimate_normals"
    if search != "radius":
        raise VcrHipError(f'{api}: queries belongs to search="radius", got search={search!r}')
    rows.radius_arguments(api, search, radius, max_nn, capacity)
    if want_idx:
        raise VcrHipError(f"{api}: want_idx is not served with queries=")
    B, _, _ = support.query_arguments(api, xyz, queries, None)
    if capacity is not None and (isinstance(capacity, bool) or not isinstance(capacity, int) or capacity < 0):
        raise VcrHipError(f"{api}: capacity must be None or an integer >= 0, got {capacity!r}")
    if not (xyz.is_cuda and queries.is_cuda):
        raise VcrHipError(f"{api} runs on the MI355X HIP path only; move the cloud and the queries to cuda "
                          "(there is no CPU fallback by design)")
    if viewpoint is not None and (not torch.is_tensor(viewpoint) or tuple(viewpoint.shape) != (B, 3) or not viewpoint.is_cuda):
        raise VcrHipError(f"{api}: viewpoint must be a device tensor [B, 3] with B = {B}")
    return support.query_normals_of(xyz, queries, radius, max_nn, capacity, viewpoint, want_curvature)


def _estimate_normals_radius(xyz, radius, max_nn, capacity, viewpoint, want_curvature, want_idx):
    """estimate_normals(search="radius"): one search_radius, then vcr_rows_normals_f32 on its rows."""
    from .radius import search_radius
    if not xyz.is_cuda:
        raise VcrHipError("estimate_normals runs on the MI355X HIP path only; move the cloud to cuda "
                          "(there is no CPU fallback by design)")
    if viewpoint is not None and (not torch.is_tensor(viewpoint) or tuple(viewpoint.shape) != (xyz.shape[0], 3)
                                  or not viewpoint.is_cuda):
        raise VcrHipError(f"estimate_normals: viewpoint must be a device tensor [B, 3] with B = {xyz.shape[0]}")
    csr = search_radius(xyz, radius, capacity=capacity)
    nrm, cur = rows.normals(native.to_rows4(xyz), *csr, max_nn=max_nn, viewpoint=viewpoint, want_curvature=want_curvature)
    res = (nrm,) + ((cur,) if want_curvature else ()) + ((csr,) if want_idx else ())
    return res[0] if len(res) == 1 else res


def refine_plane(src, tgt, tgt_normals, R=None, t=None, max_dist=0.0, max_iterations=30, rel_fitness=1e-6, rel_rmse=1e-6,
                 variant=0, want_nn=True, guard=0, prefill=None, search="scan", cell=None, order=0):
    """vcr_refine_plane_f32: refine.refine's arguments and dict, with tgt_normals [B,3,Nt] (device, fp32) behind tgt.
    search="grid": vcr_refine_plane_grid_f32, as refine.refine's."""
    from . import gridnn
    gridnn.check_search("refine_registration", search)
    gridnn.check_cell("refine_registration", cell)
    refine._cloud("tgt", tgt)
    if not torch.is_tensor(tgt_normals) or tuple(tgt_normals.shape) != tuple(tgt.shape):
        raise VcrHipError(f"refine_registration: tgt_normals must be [B, 3, Nt] like tgt {tuple(tgt.shape)}, got "
                          f"{tuple(tgt_normals.shape) if torch.is_tensor(tgt_normals) else type(tgt_normals).__name__}")
    if not tgt_normals.is_cuda or tgt_normals.device != tgt.device:
        raise VcrHipError("refine_registration: tgt_normals must live on the device of the clouds (there is no CPU fallback)")
    return refine.refine(src, tgt, R, t, max_dist, max_iterations, rel_fitness, rel_rmse, variant, want_nn, guard, prefill,
                         tgt_normals=tgt_normals.contiguous().float(), search=search, cell=cell, order=order)
