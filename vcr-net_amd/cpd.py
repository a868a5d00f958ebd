"""ctypes binding of include/cpd/vcr_hip_cpd.h and the Python API on top of it: rigid Coherent Point
Drift -- the soft assignment of every source point to every target point at a pose and a variance (vcr_cpd_expectation_f32) and
the EM loop on it in one call (vcr_cpd_f32).

Like ``ndt``, the header extends include/vcr_hip.h without touching it and this module keeps its own STRUCTS / SIGNATURES maps,
applied once to ``native.lib()`` on first use.  No CPU fallback, as everywhere."""
from __future__ import annotations

import collections
import ctypes as C
import math
import torch

from . import extension, native
from .native import VcrHipError, f32p, ptr
from .score import i32p

MAX_N = 131072
TILE, SEGMENT = 256, 4096
STATE_BYTES = 256
FORMS = 6                                                   # 1 ... 3: LDS tiles, 1 / 2 / 4 points a lane; 4 ... 6: scalar loads
STATUS = ("converged", "max iterations", "collapsed", "no mass", "not finite")
VARIANTS = tuple(f + 8 * g for g in range(3) for f in range(FORMS + 1))
f64p = C.c_void_p                                           # (a device pointer travels as an integer, like f32p)


class CpdArgs(native._Sized):
    _fields_ = [("struct_bytes", C.c_uint32), ("src", f32p), ("tgt", f32p), ("B", C.c_int), ("M", C.c_int), ("N", C.c_int),
                ("R", f32p), ("t", f32p), ("sigma2", C.c_double), ("sigma2_dev", f64p), ("scale", C.c_double), ("scale_dev", f64p),
                ("w", C.c_double), ("variant", C.c_int), ("Pt1", f64p), ("P1", f64p), ("PX", f64p), ("Np", f64p), ("e_stage", f32p),
                ("max_iterations", C.c_int), ("with_scaling", C.c_int), ("tolerance", C.c_double), ("sigma2_floor", C.c_double),
                ("R_out", f32p), ("t_out", f32p), ("R_ba", f32p), ("t_ba", f32p), ("scale_out", f64p), ("sigma2_out", f64p),
                ("iterations", i32p), ("status", i32p), ("trace", f64p)]


STRUCTS = {"vcr_cpd_args": CpdArgs}

_intp = C.POINTER(C.c_int)
# name -> (restype, [argtypes]): the prototypes of the header (tests/test_cpd_cpu.py holds them to it)
SIGNATURES = {}
for _entry in ("vcr_cpd_expectation", "vcr_cpd"):
    SIGNATURES[_entry + "_workspace_bytes"] = (C.c_size_t, [C.POINTER(CpdArgs), C.c_int])
    SIGNATURES[_entry + "_f32"] = (C.c_int, [C.POINTER(CpdArgs), C.c_void_p, C.c_size_t, C.c_void_p])
    SIGNATURES[_entry + "_form"] = (C.c_int, [C.POINTER(CpdArgs), C.c_int, _intp, _intp, _intp])

lib = extension.typed_lib(SIGNATURES)                      # native.lib() with this module's entry points typed (once)

CpdExpectation = collections.namedtuple("CpdExpectation", ("Pt1", "P1", "PX", "Np", "e"), defaults=(None,))


def _scoped(fn, tensors, *run):
    """native._guarded's device scope by hand: the table of staged calls in tests/stream_cases.py is closed, and these calls'
    side-stream and capture tests live in tests/test_hip_cpd.py."""
    first = next((x for x in tensors if torch.is_tensor(x) and x.is_cuda), None)
    if first is None:
        return fn(*run)
    with torch.cuda.device(first.device):
        return fn(*run)


def _check_clouds(api, src, tgt, R, t):
    extension.check_cloud(api, "src", src)
    extension.check_cloud(api, "tgt", tgt)
    for name, x in (("src", src), ("tgt", tgt)):
        if x.dtype != torch.float32:
            raise VcrHipError(f"{api}: {name} must be float32, got {x.dtype}")
        if x.shape[0] < 1 or not 1 <= x.shape[2] <= MAX_N:
            raise VcrHipError(f"{api}: {name} must hold at least one cloud of 1 ... {MAX_N} points, got {tuple(x.shape)}")
    B = src.shape[0]
    if tgt.shape[0] != B:
        raise VcrHipError(f"{api}: src and tgt must hold the same number of clouds, got {B} and {tgt.shape[0]}")
    if (R is None) != (t is None):
        raise VcrHipError(f"{api}: give both R and t, or neither (the identity)")
    if R is not None and not (torch.is_tensor(R) and torch.is_tensor(t) and tuple(R.shape) == (B, 3, 3) and tuple(t.shape) == (B, 3)
                              and R.dtype == torch.float32 and t.dtype == torch.float32):
        raise VcrHipError(f"{api}: R must be float32 [B, 3, 3] and t float32 [B, 3] with B = {B}")
    return B


def _per_cloud(api, name, v, B, default=None):
    """-> (host value, device tensor or None) of an fp64 given per call (a number) or per cloud (a float64 tensor [B])."""
    if v is None and default is not None:
        return default, None
    if torch.is_tensor(v):
        if v.dtype != torch.float64 or tuple(v.shape) != (B,):
            raise VcrHipError(f"{api}: {name} must be a number or a float64 tensor [B] with B = {B}, got {v.dtype} {tuple(v.shape)}")
        return 0.0, v
    if isinstance(v, bool) or not isinstance(v, (int, float)) or not (math.isfinite(v) and v > 0.0):
        raise VcrHipError(f"{api}: {name} must be finite and > 0, got {v!r}")
    return float(v), None


def _check_w(api, w):
    if isinstance(w, bool) or not isinstance(w, (int, float)) or not 0.0 <= w < 1.0:
        raise VcrHipError(f"{api}: w must be in [0, 1), got {w!r}")
    return float(w)


def _check_variant(api, variant):
    if isinstance(variant, bool) or not isinstance(variant, int) or variant not in VARIANTS:
        raise VcrHipError(f"{api}: variant must be 0 (the plan) or f + 8 g with f in 0 ... {FORMS} and g in 0 ... 2, got {variant!r}")
    return variant


def _need_cuda(api, *tensors):
    if not all(x.is_cuda for x in tensors if x is not None):
        raise VcrHipError(f"{api} runs on the MI355X HIP path only; move the clouds, the pose and the state to cuda "
                          "(there is no CPU fallback by design)")


def _expectation(src, tgt, sigma2, R, t, scale, w, want_e, variant, guard, prefill, api):
    B = _check_clouds(api, src, tgt, R, t)
    s2, s2_dev = _per_cloud(api, "sigma2", sigma2, B)
    sc, sc_dev = _per_cloud(api, "scale", scale, B, default=1.0)
    w = _check_w(api, w)
    variant = _check_variant(api, variant)
    _need_cuda(api, src, tgt, R, t, s2_dev, sc_dev)
    dev = native.same_device(src, tgt, R, t, s2_dev, sc_dev)
    src, tgt = src.contiguous(), tgt.contiguous()
    R, t = (None, None) if R is None else (R.contiguous(), t.contiguous())
    s2_dev = None if s2_dev is None else s2_dev.contiguous()
    sc_dev = None if sc_dev is None else sc_dev.contiguous()
    M, N = src.shape[2], tgt.shape[2]
    out, raw = extension.outputs(dev, guard, prefill)
    o = {"Pt1": out("Pt1", B * N, torch.float64).view(B, N), "P1": out("P1", B * M, torch.float64).view(B, M),
         "PX": out("PX", B * 3 * M, torch.float64).view(B, 3, M), "Np": out("Np", B, torch.float64)}
    if want_e:
        o["e"] = out("e", B * M * N, torch.float32).view(B, M, N)
    a = CpdArgs(ptr(src), ptr(tgt), B, M, N, ptr(R), ptr(t), s2, ptr(s2_dev), sc, ptr(sc_dev), w, variant, ptr(o["Pt1"]), ptr(o["P1"]),
                ptr(o["PX"]), ptr(o["Np"]), ptr(o.get("e")))
    extension.call_with_workspace(lib(), "vcr_cpd_expectation", a, dev, prefill)
    res = CpdExpectation(o["Pt1"], o["P1"], o["PX"], o["Np"], o.get("e"))
    return (res, raw) if guard or prefill is not None else res


def cpd_expectation(src, tgt, sigma2, R=None, t=None, scale=None, w=0.0, want_e=False, variant=0, guard=0, prefill=None):
    """The E-step of Coherent Point Drift: the source src [B,3,M] moved by (scale R, t) (None: 1, the identity) carries an
    isotropic Gaussian mixture of variance `sigma2`; a uniform component of weight `w` in [0, 1) takes what nothing explains.
    sigma2 and scale are numbers, or float64 device tensors [B] (one per cloud, as coherent_point_drift returns them).  Returns
    ``CpdExpectation``: Pt1 float64 [B,N] (how much of each target point the mixture explains), P1 float64 [B,M] (each source
    point's mass), PX float64 [B,3,M] (its mass-weighted target: ``PX / P1`` is the virtual corresponding point), Np float64 [B];
    with want_e also e float32 [B,M,N], the unnormalised weights (small shapes only).  Every bit but the hardware's exp2 is
    defined by include/cpd/vcr_hip_cpd.h; every `variant` returns the same bits.  guard / prefill (tests): as
    ``match.feat_nn``'s; the raw buffers come back beside the result."""
    return _scoped(_expectation, (src, tgt, R, t), src, tgt, sigma2, R, t, scale, w, want_e, variant, guard, prefill, "cpd_expectation")


def _cpd(src, tgt, R, t, w, max_iterations, tolerance, with_scaling, sigma2, sigma2_floor, want_trace, variant, guard, prefill, api):
    B = _check_clouds(api, src, tgt, R, t)
    w = _check_w(api, w)
    if isinstance(max_iterations, bool) or not isinstance(max_iterations, int) or not 0 <= max_iterations <= 1 << 20:
        raise VcrHipError(f"{api}: max_iterations must be an integer in [0, 2^20], got {max_iterations!r}")
    if isinstance(tolerance, bool) or not isinstance(tolerance, (int, float)) or not tolerance >= 0.0:
        raise VcrHipError(f"{api}: tolerance must be >= 0, got {tolerance!r}")
    s2, s2_dev = (0.0, None) if sigma2 is None else _per_cloud(api, "sigma2", sigma2, B)
    if sigma2_floor is not None and (isinstance(sigma2_floor, bool) or not isinstance(sigma2_floor, (int, float))
                                     or not (math.isfinite(sigma2_floor) and sigma2_floor > 0.0)):
        raise VcrHipError(f"{api}: sigma2_floor must be finite and > 0 (None: 1e-8 of the start's sigma2), got {sigma2_floor!r}")
    fl = 0.0 if sigma2_floor is None else float(sigma2_floor)
    variant = _check_variant(api, variant)
    _need_cuda(api, src, tgt, R, t, s2_dev)
    dev = native.same_device(src, tgt, R, t, s2_dev)
    src, tgt = src.contiguous(), tgt.contiguous()
    R, t = (None, None) if R is None else (R.contiguous(), t.contiguous())
    s2_dev = None if s2_dev is None else s2_dev.contiguous()
    M, N = src.shape[2], tgt.shape[2]
    out, raw = extension.outputs(dev, guard, prefill)
    o = {"R": out("R", B * 9, torch.float32).view(B, 3, 3), "t": out("t", B * 3, torch.float32).view(B, 3),
         "R_ba": out("R_ba", B * 9, torch.float32).view(B, 3, 3), "t_ba": out("t_ba", B * 3, torch.float32).view(B, 3),
         "scale": out("scale", B, torch.float64), "sigma2": out("sigma2", B, torch.float64), "Np": out("Np", B, torch.float64),
         "iterations": out("iterations", B, torch.int32), "status": out("status", B, torch.int32),
         "Pt1": out("Pt1", B * N, torch.float64).view(B, N), "P1": out("P1", B * M, torch.float64).view(B, M),
         "PX": out("PX", B * 3 * M, torch.float64).view(B, 3, M)}
    if want_trace:
        o["trace"] = out("trace", B * (max_iterations + 1), torch.float64).view(B, max_iterations + 1)
    a = CpdArgs(ptr(src), ptr(tgt), B, M, N, ptr(R), ptr(t), s2, ptr(s2_dev), 1.0, None, w, variant, ptr(o["Pt1"]), ptr(o["P1"]),
                ptr(o["PX"]), ptr(o["Np"]), None, max_iterations, 1 if with_scaling else 0, float(tolerance), fl, ptr(o["R"]), ptr(o["t"]),
                ptr(o["R_ba"]), ptr(o["t_ba"]), ptr(o["scale"]), ptr(o["sigma2"]), ptr(o["iterations"]), ptr(o["status"]),
                ptr(o.get("trace")))
    extension.call_with_workspace(lib(), "vcr_cpd", a, dev, prefill)
    if guard or prefill is not None:
        o["_raw"] = raw
    return o


def coherent_point_drift(src, tgt, R=None, t=None, w=0.1, max_iterations=50, tolerance=1e-4, with_scaling=False, sigma2=None,
                         sigma2_floor=None, want_trace=False, variant=0, guard=0, prefill=None):
    """Register src [B,3,M] to tgt [B,3,N] (float32 device tensors) by rigid Coherent Point Drift (Myronenko & Song 2010), from
    the pose (R, t) (None: the identity): EM on an isotropic Gaussian mixture on the moved source with a uniform component of
    weight `w` -- every round an O(M N) soft assignment and a closed-form rotation, translation and (with_scaling) scale;
    the variance shrinks by itself from sigma2 (None: the mean squared distance of all pairs).  Every round is enqueued in one
    call without a host synchronisation.  It stops when sigma2 moves by no more than `tolerance` of itself (status 0), after
    `max_iterations` updates (1), when sigma2 falls to `sigma2_floor` (None: 1e-8 of the start's; 2: the clouds coincide), when
    no mass is left (3) or on a non-finite sum (4) -- ``cpd.STATUS`` names them.  Returns a dict: R [B,3,3], t [B,3], R_ba,
    t_ba (the inverse of the rigid part) float32; scale, sigma2, Np float64 [B]; iterations, status int32 [B]; Pt1, P1, PX: the
    soft correspondences at the returned state, bit for bit ``cpd_expectation``'s; with want_trace also trace float64
    [B, max_iterations + 1]: sigma2 after every update, NaN behind the stop.  It is coarse (sigma2 settles at the sampling
    distance): follow it with ``refine_registration``."""
    return _scoped(_cpd, (src, tgt, R, t), src, tgt, R, t, w, max_iterations, tolerance, with_scaling, sigma2, sigma2_floor, want_trace,
                   variant, guard, prefill, "coherent_point_drift")


def cpd_form(B, M, N, loop=True, cu_count=256, variant=0, max_iterations=50):
    """vcr_cpd_form / vcr_cpd_expectation_form and _workspace_bytes (host only with an explicit cu_count): (form, the workgroups
    pass 1's segments are dealt to, pass 2's, workspace bytes)."""
    o = 0x3000                                               # (never dereferenced on the host)
    a = CpdArgs(0x1000, 0x2000, B, M, N, None, None, 1.0, None, 1.0, None, 0.1, variant, o, o, o, o, None, max_iterations, 0, 1e-4, 0.0,
                o, o)
    entry = "vcr_cpd" if loop else "vcr_cpd_expectation"
    f, s1, s2 = C.c_int(0), C.c_int(0), C.c_int(0)
    native.check(getattr(lib(), entry + "_form")(C.byref(a), cu_count, C.byref(f), C.byref(s1), C.byref(s2)), entry + "_form")
    return f.value, s1.value, s2.value, getattr(lib(), entry + "_workspace_bytes")(C.byref(a), cu_count)
