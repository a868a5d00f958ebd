"""ctypes binding of include/ndt/vcr_hip_ndt.h and the Python API on top of it: the Normal Distributions
Transform -- a voxel map of Gaussians built once from the target (vcr_ndt_map_f32), the score of a scan at a pose with its exact
gradient and Hessian (vcr_ndt_derivatives_f32) and Levenberg-Marquardt on it in one call (vcr_ndt_f32).

Like ``consistency``, the header extends include/vcr_hip.h without touching it and this module keeps its own STRUCTS /
SIGNATURES maps, applied once to ``native.lib()`` on first use.  No CPU fallback, as everywhere."""
from __future__ import annotations

import ctypes as C
import math
import torch

from . import extension, native
from .native import VcrHipError, f32p, ptr
from .score import i32p

MAX_N = 131072
VALUES = 29                                                 # f, hits, g (6), the upper triangle of H (21)
STATE_BYTES = 512
STATUS = ("converged", "max iterations", "max trials", "no hits", "not finite")
f64p = C.c_void_p                                           # (a device pointer travels as an integer, like f32p)
u64p = C.c_void_p


class NdtMapArgs(native._Sized):
    _fields_ = [("struct_bytes", C.c_uint32), ("tgt", f32p), ("B", C.c_int), ("Nt", C.c_int), ("resolution", C.c_float),
                ("min_points", C.c_int), ("min_eig_ratio", C.c_double), ("mean", f64p), ("inv_cov", f64p), ("valid", i32p),
                ("count", i32p), ("voxel_points", i32p), ("origin", f64p), ("table_keys", u64p), ("table_vals", i32p)]


class NdtArgs(native._Sized):
    _fields_ = [("struct_bytes", C.c_uint32), ("src", f32p), ("Ns", C.c_int), ("R", f32p), ("t", f32p), ("neighbors", C.c_int),
                ("d1", C.c_double), ("d2", C.c_double), ("variant", C.c_int), ("e_stage", f64p), ("voxel_stage", i32p),
                ("score", f64p), ("hits", i32p), ("g", f64p), ("H", f64p), ("max_iterations", C.c_int), ("max_trials", C.c_int),
                ("rot_epsilon", C.c_double), ("trans_epsilon", C.c_double), ("R_out", f32p), ("t_out", f32p), ("R_ba", f32p),
                ("t_ba", f32p), ("probability", f64p), ("iterations", i32p), ("trials", i32p), ("converged", i32p),
                ("status", i32p), ("trace", f64p)]


STRUCTS = {"vcr_ndt_map_args": NdtMapArgs, "vcr_ndt_args": NdtArgs}

# name -> (restype, [argtypes]): the prototypes of the header (tests/test_ndt_cpu.py holds them to it)
SIGNATURES = dict(extension.workspace_signatures("vcr_ndt_map", NdtMapArgs))
SIGNATURES.update(extension.workspace_signatures2("vcr_ndt_derivatives", NdtMapArgs, NdtArgs))
SIGNATURES.update(extension.workspace_signatures2("vcr_ndt", NdtMapArgs, NdtArgs))
SIGNATURES["vcr_ndt_table_slots"] = (C.c_int, [C.c_int])

lib = extension.typed_lib(SIGNATURES)                      # native.lib() with this module's entry points typed (once)


def constants(outlier_ratio, resolution):
    """PCL's (d1, d2) from the outlier ratio o and the voxel edge h, in fp64 on the host: c1 = 10 (1 - o), c2 = o / h^3,
    d3 = -log(c2), d1 = -log(c1 + c2) - d3, d2 = -2 log((-log(c1 exp(-1/2) + c2) - d3) / d1).  h is the fp32 the kernels see."""
    o = float(outlier_ratio)
    h = float(torch.tensor(float(resolution), dtype=torch.float32).item())
    c1 = 10.0 * (1.0 - o)
    c2 = o / (h * h * h)
    d3 = -math.log(c2)
    d1 = -math.log(c1 + c2) - d3
    d2 = -2.0 * math.log((-math.log(c1 * math.exp(-0.5) + c2) - d3) / d1)
    return d1, d2


def table_slots(Nt):
    """vcr_ndt_table_slots: 2^ceil(log2(2 Nt + 2)), the lookup slots a cloud of Nt points reserves."""
    return int(lib().vcr_ndt_table_slots(int(Nt)))


class NdtMap:
    """What vcr_ndt_map_f32 built from tgt [B,3,Nt] at `resolution`: per voxel number mean float64 [B,3,Nt], inv_cov float64
    [B,6,Nt] (entries 00, 01, 02, 11, 12, 22), valid int32 [B,Nt], voxel_points int32 [B,Nt]; per cloud count int32 [B] (-1:
    too fine) and origin float64 [B,3]; table_keys int64 / table_vals int32 [B, table_slots(Nt)], the lookup from a packed cell
    to a voxel number.  It outlives the call: many scans can be matched against one map."""
    FIELDS = ("mean", "inv_cov", "valid", "count", "voxel_points", "origin", "table_keys", "table_vals")

    def __init__(self, resolution, min_points, min_eig_ratio, **tensors):
        self.resolution, self.min_points, self.min_eig_ratio = float(resolution), int(min_points), float(min_eig_ratio)
        for k in self.FIELDS:
            setattr(self, k, tensors[k])
        self.B, self.Nt = tuple(self.valid.shape)

    @property
    def device(self):
        return self.valid.device

    def args(self, tgt=None):
        return NdtMapArgs(ptr(tgt), self.B, self.Nt, self.resolution, self.min_points, self.min_eig_ratio,
                          *(ptr(getattr(self, k)) for k in self.FIELDS))


def _map_values(api, resolution, min_points, min_eig_ratio):
    if resolution is None:
        raise VcrHipError(f"{api}: resolution has no default: give the voxel's edge")
    resolution, min_eig_ratio = float(resolution), float(min_eig_ratio)
    if not (math.isfinite(resolution) and resolution > 0.0):
        raise VcrHipError(f"{api}: resolution must be finite and > 0, got {resolution}")
    if isinstance(min_points, bool) or not isinstance(min_points, int) or min_points < 3:
        raise VcrHipError(f"{api}: min_points must be an integer >= 3, got {min_points!r}")
    if not 0.0 < min_eig_ratio <= 1.0:
        raise VcrHipError(f"{api}: min_eig_ratio must be in (0, 1], got {min_eig_ratio}")
    return resolution, min_points, min_eig_ratio


def _check_tgt(api, tgt):
    extension.check_cloud(api, "tgt", tgt)
    if tgt.dtype != torch.float32:
        raise VcrHipError(f"{api}: tgt must be float32, got {tgt.dtype}")
    if tgt.shape[0] < 1 or not 1 <= tgt.shape[2] <= MAX_N:
        raise VcrHipError(f"{api}: tgt must hold at least one cloud of 1 ... {MAX_N} points, got {tuple(tgt.shape)}")


def map_form(B, Nt, resolution=1.0, min_points=6, min_eig_ratio=0.01, cu_count=256):
    """vcr_ndt_map_form and _workspace_bytes (host only with an explicit cu_count): (lanes per voxel, table slots per cloud,
    workspace bytes) of vcr_ndt_map_f32 on [B,3,Nt]."""
    a = NdtMapArgs(0x1000, B, Nt, resolution, min_points, min_eig_ratio, *([0x2000] * 8))
    return extension.form(lib(), "vcr_ndt_map", a, cu_count)


def _ndt_map(tgt, resolution, min_points, min_eig_ratio, guard, prefill, api):
    _check_tgt(api, tgt)
    resolution, min_points, min_eig_ratio = _map_values(api, resolution, min_points, min_eig_ratio)
    if not tgt.is_cuda:
        raise VcrHipError(f"{api} runs on the MI355X HIP path only; move tgt to cuda (there is no CPU fallback by design)")
    dev = tgt.device
    tgt = tgt.contiguous()
    B, _, Nt = tgt.shape
    T = table_slots(Nt)
    out, raw = extension.outputs(dev, guard, prefill)
    m = NdtMap(resolution, min_points, min_eig_ratio,
               mean=out("mean", B * 3 * Nt, torch.float64).view(B, 3, Nt), inv_cov=out("inv_cov", B * 6 * Nt, torch.float64).view(B, 6, Nt),
               valid=out("valid", B * Nt, torch.int32).view(B, Nt), count=out("count", B, torch.int32),
               voxel_points=out("voxel_points", B * Nt, torch.int32).view(B, Nt), origin=out("origin", B * 3, torch.float64).view(B, 3),
               table_keys=out("table_keys", B * T, torch.int64).view(B, T), table_vals=out("table_vals", B * T, torch.int32).view(B, T))
    extension.call_with_workspace(lib(), "vcr_ndt_map", m.args(tgt), dev, prefill)
    if guard or prefill is not None:
        m._raw = raw
    return m


def _scoped(fn, tensors, *run):
    """native._guarded's device scope by hand: the table of staged calls in tests/stream_cases.py is closed, and these calls'
    side-stream and capture tests live in tests/test_hip_ndt.py."""
    first = next((x for x in tensors if torch.is_tensor(x) and x.is_cuda), None)
    if first is None:
        return fn(*run)
    with torch.cuda.device(first.device):
        return fn(*run)


def ndt_map(tgt, resolution, min_points=6, min_eig_ratio=0.01, guard=0, prefill=None):
    """The map of the Normal Distributions Transform: tgt [B,3,Nt] (float32 device tensor) on a voxel grid of edge `resolution`
    (voxel_down_sample's grid, word for word) becomes one Gaussian per voxel -- the fp64 mean of its members, their two-pass
    covariance, and the inverse covariance from the normals' Jacobi sweeps with every eigenvalue below `min_eig_ratio` times
    the largest raised to that (PCL: 0.01).  A voxel with fewer than `min_points` members (PCL: 6), with a covariance that is
    zero or not finite, is not valid and is never scored.  Returns an ``NdtMap``; every bit of it but the lookup table's
    slots is defined by include/ndt/vcr_hip_ndt.h.  guard / prefill (tests): as ``match.feat_nn``'s."""
    return _scoped(_ndt_map, (tgt,), tgt, resolution, min_points, min_eig_ratio, guard, prefill, "ndt_map")


def _take_map(api, map_or_tgt, resolution, min_points, min_eig_ratio):
    """-> (NdtMap or None, tgt or None): what the caller gave, checked as far as it goes without a device."""
    if isinstance(map_or_tgt, NdtMap):
        if resolution is not None and float(resolution) != map_or_tgt.resolution:
            raise VcrHipError(f"{api}: resolution {resolution} is not the map's ({map_or_tgt.resolution})")
        return map_or_tgt, None
    _check_tgt(api, map_or_tgt)
    _map_values(api, resolution, min_points, min_eig_ratio)
    return None, map_or_tgt


def _check_scan(api, src, B, R, t, neighbors, outlier_ratio):
    extension.check_cloud(api, "src", src)
    if src.dtype != torch.float32:
        raise VcrHipError(f"{api}: src must be float32, got {src.dtype}")
    if src.shape[0] != B:
        raise VcrHipError(f"{api}: src and the map must hold the same number of clouds, got {src.shape[0]} and {B}")
    if not 1 <= src.shape[2] <= MAX_N:
        raise VcrHipError(f"{api}: src must hold 1 ... {MAX_N} points, got {src.shape[2]}")
    if (R is None) != (t is None):
        raise VcrHipError(f"{api}: give both R and t, or neither (the identity)")
    if R is not None and not (torch.is_tensor(R) and torch.is_tensor(t) and tuple(R.shape) == (B, 3, 3) and tuple(t.shape) == (B, 3)
                              and R.dtype == torch.float32 and t.dtype == torch.float32):
        raise VcrHipError(f"{api}: R must be float32 [B, 3, 3] and t float32 [B, 3] with B = {B}")
    if neighbors not in (1, 7) or isinstance(neighbors, bool):
        raise VcrHipError(f"{api}: neighbors must be 1 (the point's cell) or 7 (and its six face neighbours), got {neighbors!r}")
    outlier_ratio = float(outlier_ratio)
    if not 0.0 < outlier_ratio < 1.0:
        raise VcrHipError(f"{api}: outlier_ratio must be in (0, 1), got {outlier_ratio}")
    return outlier_ratio


def _need_cuda(api, *tensors):
    if not all(x.is_cuda for x in tensors if x is not None):
        raise VcrHipError(f"{api} runs on the MI355X HIP path only; move the clouds, the pose and the map to cuda "
                          "(there is no CPU fallback by design)")


def _derivatives(src, map_or_tgt, R, t, neighbors, outlier_ratio, resolution, min_points, min_eig_ratio, want_stages, variant, guard,
                 prefill, api):
    m, tgt = _take_map(api, map_or_tgt, resolution, min_points, min_eig_ratio)
    B = m.B if m is not None else tgt.shape[0]
    outlier_ratio = _check_scan(api, src, B, R, t, neighbors, outlier_ratio)
    if variant not in (0, 1):
        raise VcrHipError(f"{api}: variant must be 0 (the plan) or 1 (a lane per point), got {variant!r}")
    _need_cuda(api, src, R, t, tgt, *(() if m is None else (m.valid,)))
    if m is None:
        m = _ndt_map(tgt, resolution, min_points, min_eig_ratio, 0, None, api)
    dev = native.same_device(src, R, t, m.valid)
    src = src.contiguous()
    R, t = (None, None) if R is None else (R.contiguous(), t.contiguous())
    Ns = src.shape[2]
    d1, d2 = constants(outlier_ratio, m.resolution)
    out, raw = extension.outputs(dev, guard, prefill)
    o = {"score": out("score", B, torch.float64), "hits": out("hits", B, torch.int32), "g": out("g", B * 6, torch.float64).view(B, 6),
         "H": out("H", B * 21, torch.float64).view(B, 21)}
    if want_stages:
        o["e"] = out("e", B * Ns * 7, torch.float64).view(B, Ns, 7)
        o["voxel"] = out("voxel", B * Ns * 7, torch.int32).view(B, Ns, 7)
    a = NdtArgs(ptr(src), Ns, ptr(R), ptr(t), neighbors, d1, d2, int(variant), ptr(o.get("e")), ptr(o.get("voxel")), ptr(o["score"]),
                ptr(o["hits"]), ptr(o["g"]), ptr(o["H"]))
    extension.call_with_workspace(lib(), "vcr_ndt_derivatives", m.args(), dev, prefill, second=a)
    o["probability"] = (-d1) * (-o["score"]) / float(Ns)
    if guard or prefill is not None:
        o["_raw"] = raw
    return o


def ndt_derivatives(src, map_or_tgt, R=None, t=None, neighbors=7, outlier_ratio=0.55, resolution=None, min_points=6,
                    min_eig_ratio=0.01, want_stages=False, variant=0, guard=0, prefill=None):
    """The NDT score of the scan src [B,3,Ns] at the pose (R, t) (None: the identity) against an ``NdtMap`` (or a target
    [B,3,Nt], whose map is built first with `resolution`, `min_points`, `min_eig_ratio`), with its exact gradient and Hessian in
    the chart (euler(x) R, euler(x) t + x[3:6]) at x = 0 (x[0:3] the rotations about x, y, z; x[3:6] the translation).  Returns
    a dict: score float64 [B] (f = -sum e: lower is better), hits int32 [B] (source points that met a valid voxel), g float64
    [B,6], H float64 [B,21] (the upper triangle by rows), probability float64 [B]; with want_stages also e float64 [B,Ns,7] and
    voxel int32 [B,Ns,7] per (point, cell) in the order own, -x, +x, -y, +y, -z, +z."""
    return _scoped(_derivatives, (src, R, t), src, map_or_tgt, R, t, neighbors, outlier_ratio, resolution, min_points, min_eig_ratio,
                   want_stages, variant, guard, prefill, "ndt_derivatives")


def hessian(H21):
    """[..., 21] (the upper triangle by rows) -> the symmetric [..., 6, 6]."""
    iu = torch.triu_indices(6, 6, device=H21.device)
    full = H21.new_zeros(H21.shape[:-1] + (6, 6))
    full[..., iu[0], iu[1]] = H21
    full[..., iu[1], iu[0]] = H21
    return full


def _ndt(src, tgt, R, t, resolution, neighbors, outlier_ratio, max_iterations, rot_epsilon, trans_epsilon, min_points, min_eig_ratio, map,
         max_trials, want_trace, variant, guard, prefill, api):
    if map is not None and not isinstance(map, NdtMap):
        raise VcrHipError(f"{api}: map must be an NdtMap (ndt_map's result), got {type(map).__name__}")
    if map is None and resolution is None:
        raise VcrHipError(f"{api}: resolution has no default: give the voxel's edge (or map=)")
    m, tgt_ = _take_map(api, map if map is not None else tgt, resolution, min_points, min_eig_ratio)
    B = m.B if m is not None else tgt_.shape[0]
    outlier_ratio = _check_scan(api, src, B, R, t, neighbors, outlier_ratio)
    for name, v in (("max_iterations", max_iterations), ("max_trials", max_trials)):
        if v is not None and (isinstance(v, bool) or not isinstance(v, int) or v < 0 or v > 1 << 20):
            raise VcrHipError(f"{api}: {name} must be an integer in [0, 2^20], got {v!r}")
    if max_iterations is None:
        raise VcrHipError(f"{api}: max_iterations must be an integer in [0, 2^20], got None")
    h = m.resolution if m is not None else float(resolution)
    rot_epsilon = float(rot_epsilon)
    trans_epsilon = 1e-6 * h if trans_epsilon is None else float(trans_epsilon)
    if not (rot_epsilon >= 0.0 and trans_epsilon >= 0.0):
        raise VcrHipError(f"{api}: rot_epsilon and trans_epsilon must be >= 0, got {rot_epsilon} and {trans_epsilon}")
    if variant not in (0, 1):
        raise VcrHipError(f"{api}: variant must be 0 (the plan) or 1 (a lane per point), got {variant!r}")
    max_trials = 4 * max_iterations if max_trials is None else max_trials
    _need_cuda(api, src, R, t, tgt_, *(() if m is None else (m.valid,)))
    if m is None:
        m = _ndt_map(tgt_, resolution, min_points, min_eig_ratio, 0, None, api)
    dev = native.same_device(src, R, t, m.valid)
    src = src.contiguous()
    R, t = (None, None) if R is None else (R.contiguous(), t.contiguous())
    Ns = src.shape[2]
    d1, d2 = constants(outlier_ratio, m.resolution)
    out, raw = extension.outputs(dev, guard, prefill)
    o = {"R": out("R", B * 9, torch.float32).view(B, 3, 3), "t": out("t", B * 3, torch.float32).view(B, 3),
         "R_ba": out("R_ba", B * 9, torch.float32).view(B, 3, 3), "t_ba": out("t_ba", B * 3, torch.float32).view(B, 3),
         "score": out("score", B, torch.float64), "probability": out("probability", B, torch.float64),
         "hits": out("hits", B, torch.int32), "g": out("g", B * 6, torch.float64).view(B, 6),
         "H": out("H", B * 21, torch.float64).view(B, 21)}
    for name in ("iterations", "trials", "converged", "status"):
        o[name] = out(name, B, torch.int32)
    if want_trace:
        o["trace"] = out("trace", B * (max_trials + 1), torch.float64).view(B, max_trials + 1)
    a = NdtArgs(ptr(src), Ns, ptr(R), ptr(t), neighbors, d1, d2, int(variant), None, None, ptr(o["score"]), ptr(o["hits"]), ptr(o["g"]),
                ptr(o["H"]), max_iterations, max_trials, rot_epsilon, trans_epsilon, ptr(o["R"]), ptr(o["t"]), ptr(o["R_ba"]),
                ptr(o["t_ba"]), ptr(o["probability"]), ptr(o["iterations"]), ptr(o["trials"]), ptr(o["converged"]), ptr(o["status"]),
                ptr(o.get("trace")))
    extension.call_with_workspace(lib(), "vcr_ndt", m.args(), dev, prefill, second=a)
    if guard or prefill is not None:
        o["_raw"] = raw
    return o


def refine_registration_ndt(src, tgt, R=None, t=None, resolution=None, neighbors=7, outlier_ratio=0.55, max_iterations=30,
                            rot_epsilon=1e-6, trans_epsilon=None, min_points=6, min_eig_ratio=0.01, map=None, max_trials=None,
                            want_trace=False, variant=0, guard=0, prefill=None):
    """Refine a registration by the Normal Distributions Transform (P2D-NDT; PCL's NormalDistributionsTransform): the scan src
    [B,3,Ns] against the voxel map of tgt [B,3,Nt] at `resolution` (no default), from the pose (R, t) (None: the identity).
    Levenberg-Marquardt on the score with its exact gradient and Hessian, every round enqueued in one call without a host
    synchronisation: a trial that lowers the score is accepted, any other raises the damping.  It stops on an accepted step
    below `rot_epsilon` (rad) and `trans_epsilon` (None: 1e-6 * resolution), after `max_iterations` accepted steps or
    `max_trials` rounds (None: 4 * max_iterations), or when fewer than three points meet a valid voxel.  `map=` takes
    ndt_map's result (tgt may then be None), so many scans match one map without rebuilding it.  Returns a dict: R [B,3,3],
    t [B,3], R_ba, t_ba (the inverse), iterations, converged int32 [B] as refine_registration's; score, probability float64
    [B], hits, trials, status int32 [B] (``ndt.STATUS`` names them), g float64 [B,6], H float64 [B,21] at the returned
    pose; with want_trace also trace float64 [B, max_trials + 1]: the score every round accepted, NaN where it accepted none."""
    return _scoped(_ndt, (src, tgt, R, t), src, tgt, R, t, resolution, neighbors, outlier_ratio, max_iterations, rot_epsilon,
                   trans_epsilon, min_points, min_eig_ratio, map, max_trials, want_trace, variant, guard, prefill,
                   "refine_registration_ndt")


def ndt_form(B, Ns, Nt, neighbors=7, max_iterations=30, max_trials=None, loop=True, cu_count=256, variant=0):
    """vcr_ndt_form / vcr_ndt_derivatives_form and _workspace_bytes (host only with an explicit cu_count): (lanes per point,
    workgroups per cloud, launches, workspace bytes)."""
    m = NdtMapArgs(None, B, Nt, 1.0, 6, 0.01, *([0x2000] * 8))
    o = 0x3000                                               # (never dereferenced on the host)
    max_trials = 4 * max_iterations if max_trials is None else max_trials
    a = NdtArgs(0x1000, Ns, None, None, neighbors, -1.0, 1.0, variant, None, None, o, o, o, o, max_iterations, max_trials, 1e-6, 1e-6,
                o, o)
    entry = "vcr_ndt" if loop else "vcr_ndt_derivatives"
    q, s, n = C.c_int(0), C.c_int(0), C.c_int(0)
    native.check(getattr(lib(), entry + "_form")(C.byref(m), C.byref(a), cu_count, C.byref(q), C.byref(s), C.byref(n)), entry + "_form")
    return q.value, s.value, n.value, getattr(lib(), entry + "_workspace_bytes")(C.byref(m), C.byref(a), cu_count)
