"""ctypes binding of include/consistency/vcr_hip_consistency.h and the Python API on top of it: a pose
from mostly wrong correspondences by pairwise length-consistency voting (vcr_consistency_f32) -- the global method beside
``match``'s RANSAC and ``fgr`` that needs neither draws nor a fair share of right matches.

Like ``fgr``, the header extends include/vcr_hip.h without touching it and this module keeps its own STRUCTS / SIGNATURES maps,
applied once to ``native.lib()`` on first use.  No CPU fallback, as everywhere."""
from __future__ import annotations

import ctypes as C
import math
import torch

from . import extension, native
from .native import VcrHipError, f32p, ptr
from .score import i32p
from .score import variant as _form_variant             # (VCR_NN_SCORE_VARIANT's encoding serves the degree pass's two fields)

MAX_N = 131072
MAX_KEEP = 4096
PAIRS_PER_LANE = (1, 2, 4)
MAX_SPLITS = 128
PRETEST_ON, PRETEST_OFF = 0x10, 0x20
DEFAULTS = dict(tau=None, keep=1024, seeds=64, ratio=0.5, min_length=0.0)
u64p = C.c_void_p                                           # (a device pointer travels as an integer, like f32p)
STAGES = ("deg", "kept", "adj", "seed_status", "seed_members", "seed_inliers", "seed_pose", "member")


class ConsistencyArgs(native._Sized):
    _fields_ = [("struct_bytes", C.c_uint32), ("src", f32p), ("tgt", f32p), ("corr", i32p), ("B", C.c_int), ("Ns", C.c_int),
                ("Nt", C.c_int), ("tau", C.c_float), ("min_length", C.c_float), ("max_dist", C.c_float), ("ratio", C.c_float),
                ("keep", C.c_int), ("seeds", C.c_int), ("R_out", f32p), ("t_out", f32p), ("best_seed", i32p), ("inliers", i32p),
                ("pairs", i32p), ("deg", i32p), ("kept", i32p), ("adj", u64p), ("seed_status", i32p), ("seed_members", i32p),
                ("seed_inliers", i32p), ("seed_pose", f32p), ("member", u64p), ("variant", C.c_int), ("stop_after", C.c_int)]


STRUCTS = {"vcr_consistency_args": ConsistencyArgs}

# name -> (restype, [argtypes]): the prototypes of the header (tests/test_consistency_cpu.py holds them to it)
SIGNATURES = dict(extension.workspace_signatures("vcr_consistency", ConsistencyArgs))
SIGNATURES["vcr_consistency_form"] = (C.c_int, [C.POINTER(ConsistencyArgs), C.c_int] + 3 * [C.POINTER(C.c_int)])

lib = extension.typed_lib(SIGNATURES)                      # native.lib() with this module's entry points typed (once)


def variant(pairs_per_lane=0, splits=0, pretest=None):
    """vcr_consistency_args.variant that forces a form of the degree pass: 0 / None leaves that part to the plan."""
    return _form_variant(pairs_per_lane, splits) | (0 if pretest is None else PRETEST_ON if pretest else PRETEST_OFF)


def consistency_form(B, Ns, Nt, keep=1024, seeds=64, cu_count=256, variant=0, stages=False, want_pretest=False):
    """vcr_consistency_form (host only with an explicit cu_count): (pairs per lane, splits of the streamed side, workspace
    bytes) of the degree pass vcr_consistency_f32 would run on [B,3,Ns] against [B,3,Nt] on a device of cu_count compute units;
    want_pretest: a fourth entry, whether the pre-test runs.  stages: with every optional output given (they leave the
    workspace)."""
    o = 0x4000 if stages else None                           # (never dereferenced on the host)
    a = ConsistencyArgs(0x1000, 0x2000, 0x3000, B, Ns, Nt, 0.01, 0.0, 0.01, 0.5, keep, seeds, 0x4000, 0x4000, None, None, None,
                        o, o, o, o, o, o, o, o, variant, 0)
    q, s, pre = C.c_int(0), C.c_int(0), C.c_int(0)
    native.check(lib().vcr_consistency_form(C.byref(a), cu_count, C.byref(q), C.byref(s), C.byref(pre)), "vcr_consistency_form")
    form = (q.value, s.value, lib().vcr_consistency_workspace_bytes(C.byref(a), cu_count))
    return form + (bool(pre.value),) if want_pretest else form


def _checks(api, src, tgt, corr, max_dist, tau, keep, seeds, ratio, min_length, given_corr=True):
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
    max_dist = float(max_dist)
    if not (math.isfinite(max_dist) and max_dist >= 0.0):
        raise VcrHipError(f"{api}: max_dist must be finite and >= 0, got {max_dist}")
    tau = max_dist if tau is None else float(tau)
    if not (math.isfinite(tau) and tau >= 0.0):
        raise VcrHipError(f"{api}: tau must be finite and >= 0, got {tau}")
    min_length, ratio = float(min_length), float(ratio)
    if not (math.isfinite(min_length) and min_length >= 0.0):
        raise VcrHipError(f"{api}: min_length must be finite and >= 0, got {min_length}")
    if not 0.0 <= ratio <= 1.0:
        raise VcrHipError(f"{api}: ratio must be in [0, 1], got {ratio}")
    for name, v in (("keep", keep), ("seeds", seeds)):
        if isinstance(v, bool) or not isinstance(v, int):
            raise VcrHipError(f"{api}: {name} must be an integer, got {v!r}")
    if keep < 64 or keep > MAX_KEEP or keep % 64:
        raise VcrHipError(f"{api}: keep must be a multiple of 64 in [64, {MAX_KEEP}], got {keep}")
    if seeds < 1 or seeds > keep:
        raise VcrHipError(f"{api}: seeds must be in [1, keep] = [1, {keep}], got {seeds}")
    if B * keep >= 1 << 30:
        raise VcrHipError(f"{api}: B * keep must stay below 2^30, got {B} * {keep}")
    if not (src.is_cuda and tgt.is_cuda and (not given_corr or corr.is_cuda)):
        raise VcrHipError(f"{api} runs on the MI355X HIP path only; move the clouds and corr to cuda "
                          "(there is no CPU fallback by design)")
    return max_dist, tau, keep, seeds, ratio, min_length


def _consistency(src, tgt, corr, max_dist, tau=None, keep=1024, seeds=64, ratio=0.5, min_length=0.0, want_stages=False, variant=0,
                 stop_after=0, guard=0, prefill=None, api="consistency"):
    max_dist, tau, keep, seeds, ratio, min_length = _checks(api, src, tgt, corr, max_dist, tau, keep, seeds, ratio, min_length)
    dev = native.same_device(src, tgt, corr)
    src, tgt, corr = src.contiguous(), tgt.contiguous(), corr.contiguous()
    B, _, Ns = src.shape
    Nt = tgt.shape[2]
    W = keep // 64
    out, raw = extension.outputs(dev, guard, prefill)
    o = {"pairs": out("pairs", B, torch.int32)}
    if stop_after == 0:
        o.update(R=out("R", B * 9, torch.float32).view(B, 3, 3), t=out("t", B * 3, torch.float32).view(B, 3),
                 best_seed=out("best_seed", B, torch.int32), inliers=out("inliers", B, torch.int32))
    if want_stages or stop_after >= 1:
        o["deg"] = out("deg", B * Ns, torch.int32).view(B, Ns)
    if want_stages or stop_after == 2:
        o["kept"] = out("kept", B * keep, torch.int32).view(B, keep)
    if want_stages and stop_after == 0:
        o["adj"] = out("adj", B * keep * W, torch.int64).view(B, keep, W)
        for name in ("seed_status", "seed_members", "seed_inliers"):
            o[name] = out(name, B * seeds, torch.int32).view(B, seeds)
        o["seed_pose"] = out("seed_pose", B * seeds * 12, torch.float32).view(B, seeds, 12)
        o["member"] = out("member", B * seeds * W, torch.int64).view(B, seeds, W)
    args = ConsistencyArgs(ptr(src), ptr(tgt), ptr(corr), B, Ns, Nt, tau, min_length, max_dist, ratio, keep, seeds, ptr(o.get("R")),
                           ptr(o.get("t")), ptr(o.get("best_seed")), ptr(o.get("inliers")), ptr(o["pairs"]), ptr(o.get("deg")),
                           ptr(o.get("kept")), ptr(o.get("adj")), ptr(o.get("seed_status")), ptr(o.get("seed_members")),
                           ptr(o.get("seed_inliers")), ptr(o.get("seed_pose")), ptr(o.get("member")), int(variant), int(stop_after))
    extension.call_with_workspace(lib(), "vcr_consistency", args, dev, prefill)
    if guard or prefill is not None:
        o["_raw"] = raw
    return o


def consistency(src, tgt, corr, max_dist, tau=None, keep=1024, seeds=64, ratio=0.5, min_length=0.0, want_stages=False, variant=0,
                stop_after=0, guard=0, prefill=None, api="consistency"):
    """vcr_consistency_f32 on src [B,3,Ns], tgt [B,3,Nt] (device, fp32) and corr int32 [B,Ns] -> dict of R [B,3,3], t [B,3],
    best_seed, inliers, pairs int32 [B]; with want_stages also deg int32 [B,Ns], kept int32 [B,keep], adj int64 [B,keep,keep/64]
    (the words' bits), seed_status, seed_members, seed_inliers int32 [B,seeds], seed_pose float32 [B,seeds,12], member int64
    [B,seeds,keep/64].  stop_after 1: pairs and deg alone; 2: pairs, deg and kept.  variant: the degree pass's form
    (``score.variant``).  guard / prefill (tests): as ``match.feat_nn``'s."""
    # native._guarded's device scope by hand: the table of staged calls in tests/stream_cases.py is closed, and this call's
    # side-stream and capture tests live in tests/test_hip_consistency.py
    first = next((x for x in (src, tgt, corr) if torch.is_tensor(x) and x.is_cuda), None)
    run = (src, tgt, corr, max_dist, tau, keep, seeds, ratio, min_length, want_stages, variant, stop_after, guard, prefill, api)
    if first is None:
        return _consistency(*run)
    with torch.cuda.device(first.device):
        return _consistency(*run)


def consistency_registration(src, tgt, corr, max_dist, tau=None, keep=1024, seeds=64, ratio=0.5, min_length=0.0,
                             want_stages=False):
    """A pose from correspondences of which MOST may be wrong: src [B,3,Ns], tgt [B,3,Nt] (float32 device tensors), corr int32
    [B,Ns] (match_features' result: the partner of every source point, -1 = none).  A rigid motion keeps distances, so two right
    pairs agree in the length between their source points and between their partners, within `tau` (None: max_dist); two
    unrelated pairs almost never do.  Every pair's degree is the number of pairs it agrees with (both lengths at least
    `min_length`); the `keep` pairs of highest degree -- the lower index among equals -- are kept; each of the first `seeds` of
    them proposes the kept pairs it agrees with and shares at least `ratio` times its best partner's common neighbours with
    (SC2-PCR's second-order measure), fits them rigidly and counts ALL pairs within max_dist under that pose.  No draws and no
    trial budget: the result is a function of the inputs alone.  Returns a dict:
      R, t         float32 [B,3,3], [B,3]   the best seed's pose (src -> tgt); the identity when no seed is valid
      inliers      int32 [B]                its count;  pairs int32 [B]: the number of source points with a partner
      best_seed    int32 [B]                its rank among the kept pairs, -1 when no seed is valid
      deg, kept, adj, seed_status, seed_members, seed_inliers, seed_pose, member (want_stages): as
      include/consistency/vcr_hip_consistency.h states them."""
    o = consistency(src, tgt, corr, max_dist, tau, keep, seeds, ratio, min_length, want_stages, api="consistency_registration")
    return {k: o[k] for k in ("R", "t", "inliers", "pairs", "best_seed") + (STAGES if want_stages else ())}


def correspondence_consistency(src, tgt, corr, tau, min_length=0.0):
    """The vote alone: int32 [B,Ns], per source point the number of OTHER pairs of corr whose two lengths to it agree within
    tau (and are at least min_length each); -1 for a source point without a partner."""
    if tau is None:
        raise VcrHipError("correspondence_consistency: tau must be finite and >= 0, got None")
    return consistency(src, tgt, corr, 0.0, tau, 64, 1, 0.5, min_length, stop_after=1, api="correspondence_consistency")["deg"]


def prune_correspondences(src, tgt, corr, tau, keep, min_length=0.0):
    """corr with -1 at every source point that is not among the `keep` pairs of highest degree (correspondence_consistency's;
    the lower index among equals): ransac_correspondences or fast_global_registration can then run on the survivors.  keep is a
    multiple of 64 in [64, 4096]."""
    if tau is None:
        raise VcrHipError("prune_correspondences: tau must be finite and >= 0, got None")
    o = consistency(src, tgt, corr, 0.0, tau, keep, 1, 0.5, min_length, stop_after=2, api="prune_correspondences")
    kept = o["kept"]
    B, Ns = corr.shape
    stays = torch.zeros((B, Ns + 1), dtype=torch.bool, device=corr.device)
    stays.scatter_(1, torch.where(kept >= 0, kept, torch.full_like(kept, Ns)).long(), True)      # (a slot behind P goes behind the end)
    return torch.where(stays[:, :Ns], corr, torch.full_like(corr, -1))
