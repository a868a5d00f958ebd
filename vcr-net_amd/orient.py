"""ctypes binding of include/orient/vcr_hip_orient.h and the Python API on top of it: a cloud's normals
oriented consistently on the device -- the minimum spanning forest of the neighbour graph under the weight 1 - |n_i . n_j|
(Boruvka's rounds), the signs carried along its trees, the top point of every tree looking up.
``orient_normals_consistent_tangent_plane`` is Open3D's call of that name.

Like ``dbscan``, the header extends include/vcr_hip.h without touching it and this module keeps its own STRUCTS / SIGNATURES maps,
applied once to ``native.lib()`` on first use.  No CPU fallback, as everywhere."""
from __future__ import annotations

import ctypes as C
import torch

from . import extension, native
from .native import VcrHipError, f32p, ptr
from .score import i32p

MAX_N = 131072
FORMS = {"rounds": 1, "one_launch": 2}                     # VCR_ORIENT_ROUNDS / VCR_ORIENT_ONE_LAUNCH: what ``variant`` forces
BUILT = ("rounds",)                                        # the one-launch form is not built: VCR_EUNSUPPORTED
_INT32_LIMIT = 1 << 31


class OrientTangentArgs(native._Sized):
    _fields_ = [("struct_bytes", C.c_uint32), ("xyz", f32p), ("normals", f32p), ("idx", i32p), ("B", C.c_int), ("N", C.c_int),
                ("k", C.c_int), ("variant", C.c_int), ("oriented", f32p), ("flip", i32p), ("ref", i32p), ("n_trees", i32p)]


STRUCTS = {"vcr_orient_tangent_args": OrientTangentArgs}

# name -> (restype, [argtypes]): the prototypes of include/orient/vcr_hip_orient.h (tests/test_orient_cpu.py holds them to it);
# there is no form to report
SIGNATURES = {n: s for n, s in extension.workspace_signatures("vcr_orient_tangent", OrientTangentArgs).items()
              if not n.endswith("_form")}

lib = extension.typed_lib(SIGNATURES)                      # native.lib() with this module's entry points typed (once)


def _variant(api, variant):
    if variant in FORMS:
        return FORMS[variant]
    if isinstance(variant, bool) or variant not in (0, 1, 2):
        raise VcrHipError(f'{api}: variant must be 0 (the plan), "rounds" or "one_launch", got {variant!r}')
    return int(variant)


def _checks(api, xyz, normals, idx):
    """Shapes and dtypes first, the device last: every refusal can be met without one."""
    extension.check_cloud(api, "xyz", xyz)
    B, _, N = xyz.shape
    if not (torch.is_tensor(normals) and normals.dtype == torch.float32 and tuple(normals.shape) == (B, 3, N)):
        raise VcrHipError(f"{api}: normals must be float32 [B, 3, N] like xyz {tuple(xyz.shape)}, got "
                          f"{(tuple(normals.shape), normals.dtype) if torch.is_tensor(normals) else type(normals).__name__}")
    if not 1 <= N <= MAX_N:
        raise VcrHipError(f"{api}: a cloud must have 1 ... {MAX_N} points, got {N}")
    if idx is not None:
        if not (torch.is_tensor(idx) and idx.dtype == torch.int32 and idx.dim() == 3 and tuple(idx.shape[:2]) == (B, N)
                and idx.shape[2] >= 1):
            raise VcrHipError(f"{api}: idx must be None or int32 [B, N, k] with B, N = {B}, {N} and k >= 1, got "
                              f"{(tuple(idx.shape), idx.dtype) if torch.is_tensor(idx) else type(idx).__name__}")
        if B * N * idx.shape[2] >= _INT32_LIMIT:
            raise VcrHipError(f"{api}: B * N * k must be below 2^31, got B = {B}, N = {N}, k = {idx.shape[2]}")
    if B < 1 or B * N >= _INT32_LIMIT:
        raise VcrHipError(f"{api}: B must be at least 1 and B * N below 2^31, got B = {B}, N = {N}")
    if not (xyz.is_cuda and normals.is_cuda and (idx is None or idx.is_cuda)):
        raise VcrHipError(f"{api} runs on the MI355X HIP path only; move the cloud, its normals and idx to cuda "
                          "(there is no CPU fallback by design)")


@native._guarded
def orient_tangent(xyz, normals, idx, want_flip=False, want_ref=False, want_trees=False, variant=0, guard=0, prefill=None,
                   api="orient.orient_tangent"):
    """vcr_orient_tangent_f32 on xyz, normals float32 [B,3,N] and idx int32 [B,N,k] (device) -> dict of oriented float32
    [B,3,N] and, where asked, flip int32 [B,N] (1 where the normal was negated), ref int32 [B,N] (the reference point of the
    point's tree) and n_trees int32 [B].  variant: 0 for the plan's form, "rounds" or "one_launch" to force one (the latter is
    not built and is refused).  guard / prefill (tests): as voxel.voxel_grid's -- the buffers come back under "_raw", and the
    workspace is prefilled too."""
    if idx is None:
        raise VcrHipError(f"{api}: idx must be int32 [B, N, k]")
    v = _variant(api, variant)
    _checks(api, xyz, normals, idx)
    dev = native.same_device(xyz, normals, idx)
    xyz, normals, idx = xyz.contiguous().float(), normals.contiguous(), idx.contiguous()
    B, _, N = xyz.shape
    out, raw = extension.outputs(dev, guard, prefill)
    o = {"oriented": out("oriented", B * 3 * N, torch.float32).view(B, 3, N)}
    if want_flip:
        o["flip"] = out("flip", B * N, torch.int32).view(B, N)
    if want_ref:
        o["ref"] = out("ref", B * N, torch.int32).view(B, N)
    if want_trees:
        o["n_trees"] = out("n_trees", B, torch.int32)
    a = OrientTangentArgs(ptr(xyz), ptr(normals), ptr(idx), B, N, idx.shape[2], v, ptr(o["oriented"]), ptr(o.get("flip")),
                          ptr(o.get("ref")), ptr(o.get("n_trees")))
    extension.call_with_workspace(lib(), "vcr_orient_tangent", a, dev, prefill)
    if guard or prefill is not None:
        o["_raw"] = raw
    return o


def orient_normals_consistent_tangent_plane(xyz, normals, k=12, idx=None, want_flip=False, want_ref=False, want_trees=False):
    """The normals [B,3,N] of xyz [B,3,N] (float32 device tensors, up to 131 072 points a cloud) with their signs made
    consistent along the surface: Open3D's orient_normals_consistent_tangent_plane (Hoppe et al. 1992).  Every pair of
    neighbours is an edge of weight 1 - |n_i . n_j|; signs are carried along the minimum spanning forest of that graph -- across
    an edge whose two normals look apart (n_i . n_j < 0) the sign changes -- and in every tree the point with the largest z
    ends with n_z >= 0.  Returns the oriented normals float32 [B,3,N] (each the input's or its exact negative), then where asked:
      flip      int32 [B,N]  1 where the normal was negated
      ref       int32 [B,N]  the top point of the point's tree
      n_trees   int32 [B]    the number of trees: 1 where the neighbour graph is connected
    The graph: idx=None takes ``search_knn(xyz, min(k, N - 1))``; a given idx int32 [B,N,k'] (``search_knn``'s, ``native.knn``'s
    or the caller's own; any k' >= 1) is used as it is and k is not read.  Rows need not be symmetric; an entry outside [0, N)
    or equal to its row's index is ignored.  No host synchronisation; the result is a function of the inputs alone, bit for bit
    (include/orient/vcr_hip_orient.h states the order of edges that makes the forest unique).
    Where it is weak: a kNN graph may fall into several components, and each is then oriented ON ITS OWN, by its own top point
    (Open3D joins them by the edges of a Delaunay triangulation; this library does not) -- ask for n_trees, and raise k where it
    is not 1.  ONE global sign per tree remains a convention ("the top looks up"): two scans of one surface in different poses may
    come out opposite, which ``register_features(orient="tangent")`` settles by trying both.  Across a sharp edge, or between two
    sheets closer together than the neighbours' spacing, the propagation can cross and orient a whole region the wrong way."""
    api = "orient_normals_consistent_tangent_plane"
    if idx is None and (isinstance(k, bool) or not isinstance(k, int) or k < 1):
        raise VcrHipError(f"{api}: k must be an integer >= 1, got {k!r}")
    _checks(api, xyz, normals, idx)
    if idx is None:
        B, _, N = xyz.shape
        if N == 1:                                          # no other point: a row of ignored entries
            idx = torch.full((B, 1, 1), -1, dtype=torch.int32, device=xyz.device)
        else:
            idx = _search(api, xyz, min(k, N - 1))
    o = orient_tangent(xyz, normals, idx, want_flip=want_flip, want_ref=want_ref, want_trees=want_trees, api=api)
    res = (o["oriented"],) + ((o["flip"],) if want_flip else ()) + ((o["ref"],) if want_ref else ()) \
        + ((o["n_trees"],) if want_trees else ())
    return res[0] if len(res) == 1 else res


def _search(api, xyz, k):
    """search_knn with its refusals under this call's name."""
    from .grid import search_knn
    try:
        return search_knn(xyz, k)
    except VcrHipError as e:
        raise VcrHipError(str(e).replace("search_knn", api, 1)) from None
