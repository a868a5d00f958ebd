"""ctypes binding of include/colored/vcr_hip_colored.h and the Python API on top of it: the colour
gradients of a cloud (vcr_color_gradient_f32) and the refinement by colour and shape that reads them (vcr_refine_colored_f32:
Open3D's registration_colored_icp, vcr_refine_f32's loop with a fourth fit), with its grid sibling.

Like ``gicp``, the header extends include/vcr_hip.h without touching it and this module keeps its own STRUCTS / SIGNATURES
maps, applied once to ``native.lib()`` on first use.  No CPU fallback, as everywhere."""
from __future__ import annotations

import ctypes as C
import math
import torch

from . import extension, gridnn, native, plane, refine
from .native import VcrHipError, f32p, ptr
from .score import i32p

LAMBDA_GEOMETRIC = 0.968                                   # Open3D's default
MAX_K = plane.MAX_K


class ColorGradientArgs(native._Sized):
    _fields_ = [("struct_bytes", C.c_uint32), ("xyz4", f32p), ("idx", i32p), ("B", C.c_int), ("N", C.c_int), ("k", C.c_int),
                ("normals", f32p), ("intensity", f32p), ("radius", C.c_float), ("gradient", f32p)]


class RefineColoredArgs(native._Sized):
    _fields_ = list(plane.RefinePlaneArgs._fields_) + [("tgt_gradient", f32p), ("tgt_intensity", f32p), ("src_intensity", f32p),
                                                       ("lambda_geometric", C.c_float)]   # vcr_refine_args' fields lead


STRUCTS = {"vcr_color_gradient_args": ColorGradientArgs, "vcr_refine_colored_args": RefineColoredArgs}

# name -> (restype, [argtypes]): the prototypes of include/colored/vcr_hip_colored.h (tests/test_colored_cpu.py holds them to it)
SIGNATURES = {"vcr_color_gradient_f32": (C.c_int, [C.POINTER(ColorGradientArgs), C.c_void_p]),
              **extension.workspace_signatures("vcr_refine_colored", RefineColoredArgs),
              **extension.workspace_signatures2("vcr_refine_colored_grid", RefineColoredArgs, gridnn.GridNnArgs)}

lib = extension.typed_lib(SIGNATURES)                      # native.lib() with this module's entry points typed (once)

_API = "refine_registration_colored"


def _form_args(B, Ns, Nt, variant, max_iterations):
    return RefineColoredArgs(src=0x1000, tgt=0x2000, B=B, Ns=Ns, Nt=Nt, max_iterations=max_iterations, R_out=0x3000, t_out=0x4000,
                             fitness=0x5000, rmse=0x6000, variant=variant, tgt_normals=0x7000, tgt_gradient=0x8000,
                             tgt_intensity=0x9000, src_intensity=0xa000,
                             lambda_geometric=LAMBDA_GEOMETRIC)   # (never dereferenced on the host)


def refine_colored_form(B, Ns, Nt, cu_count=256, variant=0, max_iterations=30):
    """vcr_refine_colored_form (host only with an explicit cu_count): (source points per lane, target splits, workspace bytes),
    as refine.refine_form."""
    return extension.form(lib(), "vcr_refine_colored", _form_args(B, Ns, Nt, variant, max_iterations), cu_count)


def refine_colored_grid_form(B, Ns, Nt, order=0, cell=0.0, cu_count=256, max_iterations=30):
    """vcr_refine_colored_grid_form (host only): as gridnn.refine_grid_form."""
    L = lib()
    a, g = _form_args(B, Ns, Nt, 0, max_iterations), gridnn.grid_args(cell, order)
    cells, taken, queries = C.c_int(0), C.c_int(0), C.c_int(0)
    native.check(L.vcr_refine_colored_grid_form(C.byref(a), C.byref(g), cu_count, C.byref(cells), C.byref(taken), C.byref(queries)),
                 "vcr_refine_colored_grid_form")
    return cells.value, taken.value, queries.value, L.vcr_refine_colored_grid_workspace_bytes(C.byref(a), C.byref(g), cu_count)


def check_lambda(lambda_geometric, api=_API):
    lam = float(lambda_geometric)
    if not (math.isfinite(lam) and 0.0 <= lam <= 1.0):
        raise VcrHipError(f"{api}: lambda_geometric must be finite and in [0, 1], got {lam}")
    return lam


def intensity(api, name, colors, cloud_name, cloud):
    """colors [B,3,N] RGB -> ((r + g) + b) / 3 in fp32; [B,N] is an intensity already.  The shape first, then the device."""
    B, _, N = cloud.shape
    if not torch.is_tensor(colors) or tuple(colors.shape) not in ((B, 3, N), (B, N)):
        raise VcrHipError(f"{api}: {name} must be [B, 3, N] RGB or [B, N] intensities for {cloud_name} {tuple(cloud.shape)}, got "
                          f"{tuple(colors.shape) if torch.is_tensor(colors) else type(colors).__name__}")
    if not colors.is_cuda or colors.device != cloud.device:
        raise VcrHipError(f"{api}: {name} must live on the device of the clouds (there is no CPU fallback)")
    c = colors.float()
    if c.dim() == 3:
        # (a tensor divisor: the division is IEEE's; by a Python scalar torch multiplies by the reciprocal)
        c = ((c[:, 0] + c[:, 1]) + c[:, 2]) / torch.full((), 3.0, dtype=torch.float32, device=c.device)
    return c.contiguous()


def _like_cloud(api, name, x, cloud_name, cloud):
    if not torch.is_tensor(x) or tuple(x.shape) != tuple(cloud.shape):
        raise VcrHipError(f"{api}: {name} must be [B, 3, N] like {cloud_name} {tuple(cloud.shape)}, got "
                          f"{tuple(x.shape) if torch.is_tensor(x) else type(x).__name__}")
    if not x.is_cuda or x.device != cloud.device:
        raise VcrHipError(f"{api}: {name} must live on the device of the clouds (there is no CPU fallback)")
    return x.contiguous().float()


def _radius(api, radius):
    if radius is None:
        return 0.0
    r = float(radius)
    if not (math.isfinite(r) and r > 0.0):
        raise VcrHipError(f"{api}: radius must be None or finite and > 0, got {radius!r}")
    return r


@native._guarded
def color_gradient(xyz4, idx, normals, inten, radius=0.0, guard=0, prefill=None):
    """vcr_color_gradient_f32 on xyz4 [B,N,4] rows (native.to_rows4), idx int32 [B,N,k], normals [B,3,N] and intensities [B,N]
    -> gradient float32 [B,3,N].  guard / prefill (tests): as plane.normals' -- the raw buffers come back as a second element."""
    if not (torch.is_tensor(xyz4) and xyz4.dim() == 3 and xyz4.shape[2] == 4 and xyz4.dtype == torch.float32):
        raise VcrHipError("color_gradient: xyz4 must be float32 [B, N, 4] rows")
    B, N, _ = xyz4.shape
    if not (torch.is_tensor(idx) and idx.dtype == torch.int32 and idx.dim() == 3 and tuple(idx.shape[:2]) == (B, N)):
        raise VcrHipError(f"color_gradient: idx must be int32 [B, N, k] with B, N = {B}, {N}")
    if not (torch.is_tensor(normals) and tuple(normals.shape) == (B, 3, N) and normals.dtype == torch.float32):
        raise VcrHipError(f"color_gradient: normals must be float32 [B, 3, N] with B, N = {B}, {N}")
    if not (torch.is_tensor(inten) and tuple(inten.shape) == (B, N) and inten.dtype == torch.float32):
        raise VcrHipError(f"color_gradient: the intensities must be float32 [B, N] with B, N = {B}, {N}")
    dev = native.same_device(xyz4, idx, normals, inten)
    xyz4, idx, normals, inten = xyz4.contiguous(), idx.contiguous(), normals.contiguous(), inten.contiguous()
    out, raw = extension.outputs(dev, guard, prefill)
    grad = out("gradient", B * 3 * N, torch.float32).view(B, 3, N)
    a = ColorGradientArgs(ptr(xyz4), ptr(idx), B, N, idx.shape[2], ptr(normals), ptr(inten), float(radius), ptr(grad))
    native.check(lib().vcr_color_gradient_f32(C.byref(a), native.stream_ptr()), "vcr_color_gradient_f32")
    return (grad, raw) if guard or prefill is not None else grad


def compute_color_gradient(xyz, normals, colors, k=20, radius=None, search="knn", idx=None):
    """The colour gradient of every point of xyz [B,3,N] (device tensor) in its tangent plane -> float32 [B,3,N]: the
    least-squares slope of the intensity over the point's k nearest neighbours projected into the plane of its unit normal
    (normals [B,3,N]), orthogonal to the normal -- what Open3D's colored ICP precomputes for its target.
    colors: [B,3,N] RGB, read as the intensity ((r + g) + b) / 3, or [B,N] intensities.
    radius: None takes all k neighbours; a radius keeps those within it (Open3D's KDTreeSearchParamHybrid(2 r, 30) is
    radius = 2 r, k = 29).  A point left with fewer than three neighbours, with a non-finite colour in its row or with collinear
    neighbours gets an exact zero.
    search: "knn" (the brute force on the rows) or "grid" (``search_knn``), as ``estimate_normals``; idx int32 [B,N,k]: rows of
    the caller's own instead (k and search are not read; entries outside [0, N) and the point itself are skipped)."""
    api = "compute_color_gradient"
    extension.check_cloud(api, "xyz", xyz)
    from . import grid
    grid.check_search(api, search)
    radius = _radius(api, radius)
    if not xyz.is_cuda:
        raise VcrHipError(f"{api} runs on the MI355X HIP path only; move the cloud to cuda (there is no CPU fallback by design)")
    normals = _like_cloud(api, "normals", normals, "xyz", xyz)
    inten = intensity(api, "colors", colors, "xyz", xyz)
    N = xyz.shape[2]
    xyz4 = native.to_rows4(xyz)
    if idx is None:
        k = int(k)
        if k < 1 or k > MAX_K:
            raise VcrHipError(f"{api}: k must be in [1, {MAX_K}], got {k}")
        if k + 1 > N:
            raise VcrHipError(f"{api}: k + 1 = {k + 1} neighbours need at least as many points, got N = {N}")
        idx = native.knn(xyz4, None, k) if search == "knn" else grid.search_knn(xyz, k)
    elif not (torch.is_tensor(idx) and idx.dim() == 3 and tuple(idx.shape[:2]) == (xyz.shape[0], N) and idx.is_cuda
              and 1 <= idx.shape[2] <= MAX_K):
        raise VcrHipError(f"{api}: idx must be a device tensor [B, N, k] with 1 <= k <= {MAX_K}")
    return color_gradient(xyz4, idx.int(), normals, inten, radius)


@native._guarded
def refine_colored(src, tgt, src_intensity, tgt_intensity, tgt_normals, tgt_gradient, R=None, t=None, max_dist=0.0,
                   max_iterations=30, rel_fitness=1e-6, rel_rmse=1e-6, variant=0, want_nn=True, guard=0, prefill=None,
                   lambda_geometric=LAMBDA_GEOMETRIC, search="scan", cell=None, order=0):
    """vcr_refine_colored_f32: refine.refine's arguments and dict, with the intensities [B,Ns], [B,Nt] and the target's normals
    and gradients [B,3,Nt] (device, fp32).  search="grid": vcr_refine_colored_grid_f32, as refine.refine's."""
    gridnn.check_search(_API, search)
    cell = gridnn.check_cell(_API, cell)
    extension.check_pair(_API, src, tgt, R, t)
    max_dist = _threshold("max_dist", max_dist)
    rel_fitness, rel_rmse = _threshold("rel_fitness", rel_fitness), _threshold("rel_rmse", rel_rmse)
    max_iterations = int(max_iterations)
    if max_iterations < 0:
        raise VcrHipError(f"{_API}: max_iterations must be >= 0, got {max_iterations}")
    lam = check_lambda(lambda_geometric)
    tgt_normals = _like_cloud(_API, "tgt_normals", tgt_normals, "tgt", tgt)
    tgt_gradient = _like_cloud(_API, "tgt_gradient", tgt_gradient, "tgt", tgt)
    src_intensity = intensity(_API, "src_colors", src_intensity, "src", src)
    tgt_intensity = intensity(_API, "tgt_colors", tgt_intensity, "tgt", tgt)
    dev, B, Ns, Nt, src, tgt, R, t = extension.take_pair(_API, src, tgt, R, t)
    out, raw = extension.outputs(dev, guard, prefill)
    o = {"R": out("R", B * 9, torch.float32).view(B, 3, 3), "t": out("t", B * 3, torch.float32).view(B, 3),
         "R_ba": out("R_ba", B * 9, torch.float32).view(B, 3, 3), "t_ba": out("t_ba", B * 3, torch.float32).view(B, 3),
         "fitness": out("fitness", B, torch.float32), "rmse": out("rmse", B, torch.float32),
         "inliers": out("inliers", B, torch.int32), "sum_d2": out("sum_d2", B, torch.float64),
         "iterations": out("iterations", B, torch.int32), "converged": out("converged", B, torch.int32)}
    if want_nn:
        o["nn_idx"], o["nn_d2"] = out("nn_idx", B * Ns, torch.int32).view(B, Ns), out("nn_d2", B * Ns, torch.float32).view(B, Ns)
    a = RefineColoredArgs(ptr(src), ptr(tgt), B, Ns, Nt, ptr(R), ptr(t), max_dist, max_iterations, rel_fitness, rel_rmse,
                          ptr(o["R"]), ptr(o["t"]), ptr(o["fitness"]), ptr(o["rmse"]), ptr(o["R_ba"]), ptr(o["t_ba"]),
                          ptr(o["inliers"]), ptr(o["sum_d2"]), ptr(o["iterations"]), ptr(o["converged"]),
                          ptr(o.get("nn_idx")), ptr(o.get("nn_d2")), int(variant), ptr(tgt_normals), ptr(tgt_gradient),
                          ptr(tgt_intensity), ptr(src_intensity), lam)
    if search == "grid":
        extension.call_with_workspace(lib(), "vcr_refine_colored_grid", a, dev, prefill, second=gridnn.grid_args(cell, order))
    else:
        extension.call_with_workspace(lib(), "vcr_refine_colored", a, dev, prefill)
    if guard or prefill is not None:
        o["_raw"] = raw
    return o


def _threshold(name, v):
    v = float(v)
    if not (math.isfinite(v) and v >= 0.0):
        raise VcrHipError(f"{_API}: {name} must be finite and >= 0, got {v}")
    return v


def refine_registration_colored(src, tgt, src_colors, tgt_colors, R=None, t=None, max_dist=0.0, max_iterations=30,
                                rel_fitness=1e-6, rel_rmse=1e-6, lambda_geometric=LAMBDA_GEOMETRIC, tgt_normals=None, normal_k=20,
                                gradient_k=20, gradient_radius=None, tgt_gradient=None, want_nn=False, centre=False,
                                search="scan", cell=None):
    """Improve the pose (R, t) on the FULL clouds by colour and shape: src [B,3,Ns], tgt [B,3,Nt] device tensors with a colour
    per point -- Open3D's registration_colored_icp (Park, Zhou, Koltun, ICCV 2017).  ``refine_registration``'s loop, stops and
    dict, with a fit of two residuals a pair: the point-to-plane distance, weighed lambda_geometric, and the difference
    between the source point's intensity and the target's intensity continued along its tangent plane by its colour gradient,
    weighed 1 - lambda_geometric.  The second one pulls the source ALONG the surface until the colours agree: it holds the pose
    where the shape does not -- walls, floors, table tops, gently curved scans --, where method="point_to_plane" stops at once
    or slides (at least six pairs).
    src_colors, tgt_colors: [B,3,N] RGB, read as the intensity ((r + g) + b) / 3, or [B,N] intensities.
    tgt_normals [B,3,Nt]: the target's unit normals; None: estimate_normals(tgt, normal_k).  tgt_gradient [B,3,Nt]: the target's
    colour gradients; None: compute_color_gradient(tgt, the normals in use, tgt_colors, gradient_k, gradient_radius).
    lambda_geometric in [0, 1] (Open3D's 0.968): at 1 the colours are not read and the result is method="point_to_plane"'s.
    Returns ``refine_registration``'s dict.  fitness, inlier_rmse and inliers are the GEOMETRIC figures of the refined pose,
    exactly score_registration(src, tgt, R, t, max_dist)'s; Open3D reports the joint (geometric and photometric) residual as
    inlier_rmse.  centre, search and cell: as ``refine_registration``'s; colours do not move with the centring.
    Where it is weak: the gradient is a least-squares slope over gradient_k neighbours, so texture finer than the point
    spacing, or none at all (one colour on a plane is singular and stops), gives it nothing to hold on to; a colour that is not
    finite at an inlier makes that cloud's pose NaN."""
    gridnn.check_search(_API, search)
    gridnn.check_cell(_API, cell)
    lam = check_lambda(lambda_geometric)
    extension.check_pair(_API, src, tgt, R, t)
    kw = dict(max_iterations=max_iterations, rel_fitness=rel_fitness, rel_rmse=rel_rmse, lambda_geometric=lam,
              tgt_normals=tgt_normals, normal_k=normal_k, gradient_k=gradient_k, gradient_radius=gradient_radius,
              tgt_gradient=tgt_gradient, search=search, cell=cell)
    if centre is not False and centre is not None:
        from .centre import centred_pose, take_centres
        src_c, c_src, tgt_c, c_tgt = take_centres(_API, centre, src, tgt)
        if R is not None:
            native.same_device(src, tgt, R, t)
            if tuple(R.shape) != (src.shape[0], 3, 3) or tuple(t.shape) != (src.shape[0], 3):
                raise VcrHipError(f"{_API}: R must be [B, 3, 3] and t [B, 3] with B = {src.shape[0]}, got "
                                  f"{tuple(R.shape)} and {tuple(t.shape)}")
            R, t = R.contiguous().float(), t.contiguous().float()
        R_c, t_c = centred_pose(R, t, c_src, c_tgt)
        res = refine_registration_colored(src_c, tgt_c, src_colors, tgt_colors, R_c, t_c, max_dist, want_nn=False, centre=False, **kw)
        return refine.uncentre_refined(res, src, tgt, c_src, c_tgt, max_dist, want_nn, search=search, cell=cell)
    src_i = intensity(_API, "src_colors", src_colors, "src", src)
    tgt_i = intensity(_API, "tgt_colors", tgt_colors, "tgt", tgt)
    if tgt_normals is None:
        tgt_normals = plane.estimate_normals(tgt, normal_k)
    tgt_normals = _like_cloud(_API, "tgt_normals", tgt_normals, "tgt", tgt)
    if tgt_gradient is None:
        tgt_gradient = compute_color_gradient(tgt, tgt_normals, tgt_i, gradient_k, gradient_radius)
    f = refine_colored(src, tgt, src_i, tgt_i, tgt_normals, tgt_gradient, R, t, max_dist, max_iterations, rel_fitness, rel_rmse,
                       want_nn=want_nn, lambda_geometric=lam, search=search, cell=cell)
    res = {"R": f["R"], "t": f["t"], "R_ba": f["R_ba"], "t_ba": f["t_ba"], "fitness": f["fitness"], "inlier_rmse": f["rmse"],
           "inliers": f["inliers"], "iterations": f["iterations"], "converged": f["converged"]}
    if want_nn:
        res["nn_idx"], res["nn_d2"] = f["nn_idx"].long(), f["nn_d2"]
    return res
