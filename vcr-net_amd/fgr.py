"""ctypes binding of include/vcr_hip_fgr.h and the Python API on top of it: Fast Global Registration
over a correspondence array (vcr_fgr_f32) -- Open3D's registration_fgr_based_on_feature_matching behind its matching -- the
global method beside ``match``'s RANSAC that has no trial budget.

Like ``match``, the header extends include/vcr_hip.h without touching it and this module keeps its own STRUCTS / SIGNATURES maps,
applied once to ``native.lib()`` on first use.  No CPU fallback, as everywhere."""
from __future__ import annotations

import ctypes as C
import math
import torch

from . import extension, native
from .native import VcrHipError, f32p, ptr
from .score import f64p, i32p

MAX_N = 131072
MAX_TRIALS = 1 << 20
MAX_ITERATIONS = 1024
MIN_ENTRIES = 10
DEFAULTS = dict(tuple_scale=0.95, max_tuples=1000, iterations=64, division_factor=1.4, mu_floor=0.025, decrease_mu=True,
                tuple_trials=None, seed=0)


class FgrArgs(native._Sized):
    _fields_ = [("struct_bytes", C.c_uint32), ("src", f32p), ("tgt", f32p), ("corr", i32p), ("B", C.c_int), ("Ns", C.c_int),
                ("Nt", C.c_int), ("tuple_scale", C.c_float), ("tuple_trials", C.c_int), ("max_tuples", C.c_int), ("seed", C.c_uint32),
                ("iterations", C.c_int), ("decrease_mu", C.c_int), ("division_factor", C.c_double), ("mu_floor", C.c_double),
                ("R_out", f32p), ("t_out", f32p), ("pairs", i32p), ("tuples", i32p), ("used", i32p), ("status", i32p),
                ("tuple_list", i32p), ("norm", f64p), ("pose64", f64p), ("sums", f64p), ("mu", f64p)]


STRUCTS = {"vcr_fgr_args": FgrArgs}

# name -> (restype, [argtypes]): the prototypes of include/vcr_hip_fgr.h (tests/test_fgr_cpu.py holds them to it)
SIGNATURES = dict(vcr_fgr_workspace_bytes=(C.c_size_t, [C.POINTER(FgrArgs), C.c_int]),
                  vcr_fgr_f32=(C.c_int, [C.POINTER(FgrArgs), C.c_void_p, C.c_size_t, C.c_void_p]))

lib = extension.typed_lib(SIGNATURES)                      # native.lib() with this module's entry points typed (once)


def _fgr_checks(api, src, tgt, corr, tuple_scale, max_tuples, iterations, division_factor, mu_floor, tuple_trials, seed,
                given_corr=True):
    """What the call refuses before any launch -- shapes, dtypes and values first, the device last.  given_corr False: corr is
    not looked at (register_features computes it).  -> the values as the struct takes them."""
    extension.check_cloud(api, "src", src)
    extension.check_cloud(api, "tgt", tgt)
    if src.shape[0] != tgt.shape[0]:
        raise VcrHipError(f"{api}: src and tgt must hold the same number of clouds, got {src.shape[0]} and {tgt.shape[0]}")
    if src.dtype != torch.float32 or tgt.dtype != torch.float32:
        raise VcrHipError(f"{api}: src and tgt must be float32, got {src.dtype} and {tgt.dtype}")
    B, _, Ns = src.shape
    if min(Ns, tgt.shape[2]) < 1 or max(Ns, tgt.shape[2]) > MAX_N:
        raise VcrHipError(f"{api}: a cloud must hold 1 ... {MAX_N} points, got {Ns} and {tgt.shape[2]}")
    if given_corr and not (torch.is_tensor(corr) and corr.dtype == torch.int32 and tuple(corr.shape) == (B, Ns)):
        raise VcrHipError(f"{api}: corr must be int32 [B, Ns] = [{B}, {Ns}] (match_features' result), got "
                          f"{(tuple(corr.shape), corr.dtype) if torch.is_tensor(corr) else type(corr).__name__}")
    tuple_scale, division_factor, mu_floor = float(tuple_scale), float(division_factor), float(mu_floor)
    tuple_trials = min(100 * Ns, MAX_TRIALS) if tuple_trials is None else int(tuple_trials)
    max_tuples, iterations, seed = int(max_tuples), int(iterations), int(seed)
    if not 0.0 <= tuple_scale <= 1.0:
        raise VcrHipError(f"{api}: tuple_scale must be 0 (no tuple test) or in (0, 1], got {tuple_scale}")
    if tuple_trials < 1 or tuple_trials > MAX_TRIALS:
        raise VcrHipError(f"{api}: tuple_trials must be in [1, {MAX_TRIALS}], got {tuple_trials}")
    if max_tuples < 1 or max_tuples >= 1 << 31:
        raise VcrHipError(f"{api}: max_tuples must be in [1, 2^31), got {max_tuples}")
    if iterations < 0 or iterations > MAX_ITERATIONS:
        raise VcrHipError(f"{api}: iterations must be in [0, {MAX_ITERATIONS}], got {iterations}")
    if not (math.isfinite(division_factor) and division_factor > 1.0):
        raise VcrHipError(f"{api}: division_factor must be finite and > 1, got {division_factor}")
    if not (math.isfinite(mu_floor) and mu_floor > 0.0):
        raise VcrHipError(f"{api}: mu_floor must be finite and > 0, got {mu_floor}")
    if not 0 <= seed < 1 << 32:
        raise VcrHipError(f"{api}: seed must be in [0, 2^32), got {seed}")
    if B * tuple_trials >= 1 << 29:
        raise VcrHipError(f"{api}: B * tuple_trials must stay below 2^29, got {B} * {tuple_trials}")
    if not (src.is_cuda and tgt.is_cuda and (not given_corr or corr.is_cuda)):
        raise VcrHipError(f"{api} runs on the MI355X HIP path only; move the clouds and corr to cuda "
                          "(there is no CPU fallback by design)")
    return tuple_scale, max_tuples, iterations, division_factor, mu_floor, tuple_trials, seed


@native._guarded
def fgr(src, tgt, corr, tuple_scale=0.95, max_tuples=1000, iterations=64, division_factor=1.4, mu_floor=0.025, decrease_mu=True,
        tuple_trials=None, seed=0, want_stages=False, guard=0, prefill=None, api="fgr"):
    """vcr_fgr_f32 on src [B,3,Ns], tgt [B,3,Nt] (device, fp32) and corr int32 [B,Ns] -> dict of R [B,3,3], t [B,3], pairs,
    tuples, used, status int32 [B]; with want_stages also tuple_list int32 [B,3K], norm [B,7], pose64 [B,12], sums [B,27],
    mu [B] (float64).  guard / prefill (tests): as ``match.feat_nn``'s."""
    tuple_scale, K, iterations, division_factor, mu_floor, T, seed = _fgr_checks(
        api, src, tgt, corr, tuple_scale, max_tuples, iterations, division_factor, mu_floor, tuple_trials, seed)
    dev = native.same_device(src, tgt, corr)
    src, tgt, corr = src.contiguous(), tgt.contiguous(), corr.contiguous()
    B, _, Ns = src.shape
    Nt = tgt.shape[2]
    out, raw = extension.outputs(dev, guard, prefill)
    o = {"R": out("R", B * 9, torch.float32).view(B, 3, 3), "t": out("t", B * 3, torch.float32).view(B, 3)}
    for name in ("pairs", "tuples", "used", "status"):
        o[name] = out(name, B, torch.int32)
    if want_stages:
        o["tuple_list"] = out("tuple_list", B * 3 * K, torch.int32).view(B, 3 * K)
        for name, n in (("norm", 7), ("pose64", 12), ("sums", 27), ("mu", 1)):
            o[name] = out(name, B * n, torch.float64).view(B, n)
        o["mu"] = o["mu"].view(B)
    args = FgrArgs(ptr(src), ptr(tgt), ptr(corr), B, Ns, Nt, tuple_scale, T, K, seed, iterations, int(bool(decrease_mu)),
                   division_factor, mu_floor, ptr(o["R"]), ptr(o["t"]), ptr(o["pairs"]), ptr(o["tuples"]), ptr(o["used"]),
                   ptr(o["status"]), ptr(o.get("tuple_list")), ptr(o.get("norm")), ptr(o.get("pose64")), ptr(o.get("sums")),
                   ptr(o.get("mu")))
    extension.call_with_workspace(lib(), "vcr_fgr", args, dev, prefill)
    if guard or prefill is not None:
        o["_raw"] = raw
    return o


def fast_global_registration(src, tgt, corr, tuple_scale=0.95, max_tuples=1000, iterations=64, division_factor=1.4,
                             mu_floor=0.025, decrease_mu=True, tuple_trials=None, seed=0):
    """A pose from correspondences without trials: src [B,3,Ns], tgt [B,3,Nt] (float32 device tensors), corr int32 [B,Ns]
    (match_features' result: the partner of every source point, -1 = none).  Open3D's Fast Global Registration behind its
    matching: up to `tuple_trials` (None: min(100 Ns, 2^20)) triples of pairs are drawn by a hash of (seed, trial) and the first
    `max_tuples` whose three edge lengths agree within `tuple_scale` on both sides are kept (0: no test, all pairs are used);
    both clouds are centred and scaled to the unit ball; `iterations` Gauss-Newton steps then minimise the kept pairs' distances
    under the weight (mu / (d^2 + mu))^2, mu starting at 1 and divided by `division_factor` every fourth iteration while above
    `mu_floor` (decrease_mu).  The cost does not grow with the share of wrong pairs, and the result is a function of the inputs
    and the seed.  Returns a dict:
      R, t      float32 [B,3,3], [B,3]   the pose src -> tgt; the identity with fewer than 10 entries to optimise (status 1),
                                         NaN for a cloud with a non-finite coordinate or no extent (status 2)
      pairs     int32 [B]                the source points with a partner;  tuples: the kept triples;  used: the entries
                                         optimised (3 tuples, or pairs without the tuple test)
      status    int32 [B]                0, 1, 2 as above; + 16 where an iteration met a singular system (an identity update)."""
    o = fgr(src, tgt, corr, tuple_scale, max_tuples, iterations, division_factor, mu_floor, decrease_mu, tuple_trials, seed,
            api="fast_global_registration")
    return {k: o[k] for k in ("R", "t", "pairs", "tuples", "used", "status")}
