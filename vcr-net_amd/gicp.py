"""ctypes binding of include/vcr_hip_gicp.h and the Python API on top of it: the plane-to-plane
refinement (vcr_refine_gicp_f32: Open3D's registration_generalized_icp with covariances built from the normals of both clouds,
vcr_refine_f32's loop with a third fit).

Like ``plane``, the header extends include/vcr_hip.h without touching it and this module keeps its own STRUCTS / SIGNATURES
maps, applied once to ``native.lib()`` on first use.  No CPU fallback, as everywhere."""
from __future__ import annotations

import ctypes as C
import math
import torch

from . import extension, native, plane, refine
from .native import VcrHipError, f32p

EPSILON = 1e-3                                             # Open3D's default


class RefineGicpArgs(native._Sized):
    _fields_ = list(plane.RefinePlaneArgs._fields_) + [("src_normals", f32p), ("epsilon", C.c_float)]   # vcr_refine_args' fields lead


STRUCTS = {"vcr_refine_gicp_args": RefineGicpArgs}

# name -> (restype, [argtypes]): the prototypes of include/vcr_hip_gicp.h (tests/test_gicp_cpu.py holds them to it)
SIGNATURES = extension.workspace_signatures("vcr_refine_gicp", RefineGicpArgs)

lib = extension.typed_lib(SIGNATURES)                      # native.lib() with this module's entry points typed (once)


def refine_gicp_form(B, Ns, Nt, cu_count=256, variant=0, max_iterations=30):
    """vcr_refine_gicp_form (host only with an explicit cu_count): (source points per lane, target splits, workspace bytes),
    as refine.refine_form."""
    a = RefineGicpArgs(src=0x1000, tgt=0x2000, B=B, Ns=Ns, Nt=Nt, max_iterations=max_iterations, R_out=0x3000, t_out=0x4000,
                       fitness=0x5000, rmse=0x6000, variant=variant, tgt_normals=0x7000, src_normals=0x8000,
                       epsilon=EPSILON)                     # (never dereferenced on the host)
    return extension.form(lib(), "vcr_refine_gicp", a, cu_count)


def check_epsilon(epsilon):
    epsilon = float(epsilon)
    if not (math.isfinite(epsilon) and 0.0 < epsilon <= 1.0):
        raise VcrHipError(f"refine_registration: epsilon must be finite, > 0 and <= 1, got {epsilon}")
    return epsilon


def _normals(src, tgt, src_normals, tgt_normals):
    """plane.refine_plane's checks of tgt_normals, for both clouds: the shapes first, then the devices."""
    pairs = (("tgt_normals", tgt_normals, "tgt", tgt), ("src_normals", src_normals, "src", src))
    for name, nrm, cloud_name, cloud in pairs:
        refine._cloud(cloud_name, cloud)
        if not torch.is_tensor(nrm) or tuple(nrm.shape) != tuple(cloud.shape):
            raise VcrHipError(f"refine_registration: {name} must be [B, 3, N{cloud_name[0]}] like {cloud_name} {tuple(cloud.shape)}, "
                              f"got {tuple(nrm.shape) if torch.is_tensor(nrm) else type(nrm).__name__}")
    for name, nrm, _, cloud in pairs:
        if not nrm.is_cuda or nrm.device != cloud.device:
            raise VcrHipError(f"refine_registration: {name} must live on the device of the clouds (there is no CPU fallback)")
    return src_normals.contiguous().float(), tgt_normals.contiguous().float()


def refine_gicp(src, tgt, src_normals, tgt_normals, R=None, t=None, max_dist=0.0, max_iterations=30, rel_fitness=1e-6,
                rel_rmse=1e-6, variant=0, want_nn=True, guard=0, prefill=None, epsilon=EPSILON, search="scan", cell=None, order=0):
    """vcr_refine_gicp_f32: refine.refine's arguments and dict, with src_normals [B,3,Ns] and tgt_normals [B,3,Nt] (device,
    fp32, unit vectors of either sign) behind the clouds and epsilon, the covariance along a normal.
    search="grid": vcr_refine_gicp_grid_f32, as refine.refine's."""
    from . import gridnn
    gridnn.check_search("refine_registration", search)
    gridnn.check_cell("refine_registration", cell)
    src_normals, tgt_normals = _normals(src, tgt, src_normals, tgt_normals)
    return refine.refine(src, tgt, R, t, max_dist, max_iterations, rel_fitness, rel_rmse, variant, want_nn, guard, prefill,
                         tgt_normals=tgt_normals, src_normals=src_normals, epsilon=check_epsilon(epsilon), search=search, cell=cell,
                         order=order)
