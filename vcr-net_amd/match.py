"""ctypes binding of include/vcr_hip_match.h and the Python API on top of it: a pose from features
alone -- the nearest neighbour across two clouds in the 33-d FPFH space (vcr_feat_nn_f32) and a RANSAC over the resulting
correspondences (vcr_ransac_f32), Open3D's registration_ransac_based_on_feature_matching on the device.

Like ``fpfh``, the header extends include/vcr_hip.h without touching it and this module keeps its own STRUCTS / SIGNATURES maps,
applied once to ``native.lib()`` on first use.  No CPU fallback, as everywhere."""
from __future__ import annotations

import ctypes as C
import math
import torch

from . import extension, native
from .native import VcrHipError, f32p, ptr
from .score import i32p, variant  # noqa: F401  (VCR_NN_SCORE_VARIANT's encoding serves vcr_feat_nn_args.variant too)

FEAT_C = 33
MAX_N = 131072
MAX_TRIALS = 1 << 20
QUERIES_PER_LANE = (1, 2, 4)
MAX_SPLITS = 128


class FeatNnArgs(native._Sized):
    _fields_ = [("struct_bytes", C.c_uint32), ("a", f32p), ("b", f32p), ("B", C.c_int), ("C", C.c_int), ("Ns", C.c_int),
                ("Nt", C.c_int), ("nn_idx", i32p), ("nn_d2", f32p), ("mutual", C.c_int), ("rev_idx", i32p), ("variant", C.c_int)]


class RansacArgs(native._Sized):
    _fields_ = [("struct_bytes", C.c_uint32), ("src", f32p), ("tgt", f32p), ("corr", i32p), ("B", C.c_int), ("Ns", C.c_int),
                ("Nt", C.c_int), ("max_dist", C.c_float), ("similarity", C.c_float), ("trials", C.c_int), ("seed", C.c_uint32),
                ("R_out", f32p), ("t_out", f32p), ("best_trial", i32p), ("inliers", i32p), ("pairs", i32p),
                ("trial_status", i32p), ("trial_picks", i32p), ("trial_pose", f32p), ("trial_inliers", i32p)]


STRUCTS = {"vcr_feat_nn_args": FeatNnArgs, "vcr_ransac_args": RansacArgs}

# name -> (restype, [argtypes]): the prototypes of include/vcr_hip_match.h (tests/test_match_cpu.py holds them to it)
SIGNATURES = dict(extension.workspace_signatures("vcr_feat_nn", FeatNnArgs),
                  vcr_ransac_workspace_bytes=(C.c_size_t, [C.POINTER(RansacArgs), C.c_int]),
                  vcr_ransac_f32=(C.c_int, [C.POINTER(RansacArgs), C.c_void_p, C.c_size_t, C.c_void_p]))

lib = extension.typed_lib(SIGNATURES)                      # native.lib() with this module's entry points typed (once)


def feat_nn_form(B, Ns, Nt, cu_count=256, variant=0, mutual=False):
    """vcr_feat_nn_form (host only with an explicit cu_count): (rows of a per lane, splits of b, workspace bytes)
    vcr_feat_nn_f32 would search [B,33,Ns] in [B,33,Nt] with on a device of cu_count compute units."""
    a = FeatNnArgs(0x1000, 0x2000, B, FEAT_C, Ns, Nt, 0x3000, None, int(bool(mutual)), None, variant)   # (never dereferenced on the host)
    return extension.form(lib(), "vcr_feat_nn", a, cu_count)


def _features(api, name, x):
    if not (torch.is_tensor(x) and x.dim() == 3 and x.dtype == torch.float32):
        raise VcrHipError(f"{api}: {name} must be a float32 [B, {FEAT_C}, N] feature tensor, got "
                          f"{(tuple(x.shape), x.dtype) if torch.is_tensor(x) else type(x).__name__}")
    if x.shape[1] != FEAT_C:
        raise VcrHipError(f"{api}: {name} must have {FEAT_C} channels (compute_fpfh_feature's), got {x.shape[1]}")
    if x.shape[2] < 1 or x.shape[2] > MAX_N:
        raise VcrHipError(f"{api}: {name} must hold 1 ... {MAX_N} points, got {x.shape[2]}")


def _feature_pair(api, a, b):
    """Shapes, dtypes and widths first, the device last: every refusal can be met without one."""
    _features(api, "src_feat", a)
    _features(api, "tgt_feat", b)
    if a.shape[0] != b.shape[0]:
        raise VcrHipError(f"{api}: src_feat and tgt_feat must hold the same number of clouds, got {a.shape[0]} and {b.shape[0]}")
    if not (a.is_cuda and b.is_cuda):
        raise VcrHipError(f"{api} runs on the MI355X HIP path only; move the features to cuda (there is no CPU fallback by design)")


@native._guarded
def feat_nn(a, b, mutual=False, want_d2=True, want_rev=False, variant=0, guard=0, prefill=None, api="feat_nn"):
    """vcr_feat_nn_f32 on a [B,33,Ns], b [B,33,Nt] (device, fp32) -> dict of nn_idx int32 [B,Ns], nn_d2 float32 [B,Ns] (want_d2),
    rev_idx int32 [B,Nt] (want_rev: the b -> a search).  mutual: nn_idx keeps j only where rev_idx[j] == i, -1 elsewhere.
    guard / prefill (tests): every output is a view of a buffer with `guard` more elements behind it, all of it -- and the
    workspace -- filled with the byte `prefill` before the launch; the buffers come back under "_raw"."""
    _feature_pair(api, a, b)
    dev = native.same_device(a, b)
    a, b = a.contiguous(), b.contiguous()
    B, _, Ns = a.shape
    Nt = b.shape[2]
    out, raw = extension.outputs(dev, guard, prefill)
    o = {"nn_idx": out("nn_idx", B * Ns, torch.int32).view(B, Ns)}
    if want_d2:
        o["nn_d2"] = out("nn_d2", B * Ns, torch.float32).view(B, Ns)
    if want_rev:
        o["rev_idx"] = out("rev_idx", B * Nt, torch.int32).view(B, Nt)
    args = FeatNnArgs(ptr(a), ptr(b), B, FEAT_C, Ns, Nt, ptr(o["nn_idx"]), ptr(o.get("nn_d2")), int(bool(mutual)),
                      ptr(o.get("rev_idx")), int(variant))
    extension.call_with_workspace(lib(), "vcr_feat_nn", args, dev, prefill)
    if guard or prefill is not None:
        o["_raw"] = raw
    return o


def _ransac_checks(api, src, tgt, corr, max_dist, trials, similarity, seed, given_corr=True):
    """What the RANSAC refuses before any launch -- shapes, dtypes and values first, the device last.  given_corr False: corr is
    not looked at (register_features computes it)."""
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
    max_dist, similarity, trials, seed = float(max_dist), float(similarity), int(trials), int(seed)
    if not (math.isfinite(max_dist) and max_dist >= 0.0):
        raise VcrHipError(f"{api}: max_dist must be finite and >= 0, got {max_dist}")
    if not 0.0 <= similarity <= 1.0:
        raise VcrHipError(f"{api}: similarity must be 0 (no edge-length test) or in (0, 1], got {similarity}")
    if trials < 1 or trials > MAX_TRIALS:
        raise VcrHipError(f"{api}: trials must be in [1, {MAX_TRIALS}], got {trials}")
    if not 0 <= seed < 1 << 32:
        raise VcrHipError(f"{api}: seed must be in [0, 2^32), got {seed}")
    if not (src.is_cuda and tgt.is_cuda and (not given_corr or corr.is_cuda)):
        raise VcrHipError(f"{api} runs on the MI355X HIP path only; move the clouds and corr to cuda "
                          "(there is no CPU fallback by design)")
    return max_dist, similarity, trials, seed


@native._guarded
def ransac(src, tgt, corr, max_dist, trials=100000, similarity=0.9, seed=0, want_trials=False, guard=0, prefill=None,
           api="ransac"):
    """vcr_ransac_f32 on src [B,3,Ns], tgt [B,3,Nt] (device, fp32) and corr int32 [B,Ns] (the target index per source point;
    outside [0, Nt): none) -> dict of R [B,3,3], t [B,3], best_trial, inliers, pairs int32 [B]; with want_trials also
    trial_status int32 [B,T], trial_picks int32 [B,T,3], trial_pose float32 [B,T,12], trial_inliers int32 [B,T].
    guard / prefill (tests): as ``feat_nn``'s."""
    max_dist, similarity, T, seed = _ransac_checks(api, src, tgt, corr, max_dist, trials, similarity, seed)
    dev = native.same_device(src, tgt, corr)
    src, tgt, corr = src.contiguous(), tgt.contiguous(), corr.contiguous()
    B, _, Ns = src.shape
    Nt = tgt.shape[2]
    out, raw = extension.outputs(dev, guard, prefill)
    o = {"R": out("R", B * 9, torch.float32).view(B, 3, 3), "t": out("t", B * 3, torch.float32).view(B, 3)}
    for name in ("best_trial", "inliers", "pairs"):
        o[name] = out(name, B, torch.int32)
    if want_trials:
        o["trial_status"] = out("trial_status", B * T, torch.int32).view(B, T)
        o["trial_picks"] = out("trial_picks", B * T * 3, torch.int32).view(B, T, 3)
        o["trial_pose"] = out("trial_pose", B * T * 12, torch.float32).view(B, T, 12)
        o["trial_inliers"] = out("trial_inliers", B * T, torch.int32).view(B, T)
    args = RansacArgs(ptr(src), ptr(tgt), ptr(corr), B, Ns, Nt, max_dist, similarity, T, seed, ptr(o["R"]), ptr(o["t"]),
                      ptr(o["best_trial"]), ptr(o["inliers"]), ptr(o["pairs"]), ptr(o.get("trial_status")),
                      ptr(o.get("trial_picks")), ptr(o.get("trial_pose")), ptr(o.get("trial_inliers")))
    extension.call_with_workspace(lib(), "vcr_ransac", args, dev, prefill)
    if guard or prefill is not None:
        o["_raw"] = raw
    return o


def match_features(src_feat, tgt_feat, mutual=False, want_d2=False):
    """For every point of the source its nearest point of the target IN FEATURE SPACE: src_feat [B,33,Ns], tgt_feat [B,33,Nt]
    (float32 device tensors, compute_fpfh_feature's; Ns != Nt allowed, each up to 131 072) -> int32 [B,Ns], the target index;
    among equally near target points the lowest index, -1 for a source row without a finite distance.  The distance is the sum
    of the 33 squared differences in fp32, one fmaf chain in channel order.  mutual: a pair (i, j) is kept only where i is also
    the nearest source point of j; the others are -1.  want_d2: also the squared feature distances, float32 [B,Ns]."""
    f = feat_nn(src_feat, tgt_feat, mutual=mutual, want_d2=want_d2, api="match_features")
    return (f["nn_idx"], f["nn_d2"]) if want_d2 else f["nn_idx"]


def ransac_correspondences(src, tgt, corr, max_dist, trials=100000, similarity=0.9, seed=0, want_trials=False):
    """A pose from correspondences: src [B,3,Ns], tgt [B,3,Nt] (float32 device tensors), corr int32 [B,Ns] (match_features'
    result: the partner of every source point, -1 = none).  Open3D's registration_ransac_based_on_feature_matching with
    ransac_n = 3 and its edge-length (similarity; 0 = off) and distance (max_dist) checkers: every trial draws three pairs by
    a hash of (seed, trial), solves their rigid fit and counts the pairs within max_dist of their partner under it.  ALL
    `trials` run (no early stop), a trial with a repeated pick is dropped, and the winner is the highest count, the lowest
    trial among equals -- the result is a function of the inputs and the seed.  Returns a dict:
      R, t         float32 [B,3,3], [B,3]   the best trial's pose (src -> tgt); the identity when no trial is valid
      inliers      int32 [B]                its count;  pairs int32 [B]: the number of source points with a partner
      best_trial   int32 [B]                -1 when no trial is valid
      trial_status, trial_picks, trial_pose, trial_inliers (want_trials): per trial, as include/vcr_hip_match.h states them."""
    return ransac(src, tgt, corr, max_dist, trials, similarity, seed, want_trials, api="ransac_correspondences")


def register_features(src, tgt, max_dist, k=30, radius=None, mutual=True, trials=100000, similarity=0.9, seed=0, refine=None,
                      refine_method="point_to_point", src_normals=None, tgt_normals=None, method="ransac", fgr=None,
                      centre=False, search="knn", nn_search="scan", max_nn=None, keypoints=None, iss=None, describe="all",
                      consistency=None, capacity=None, orient=None, orient_k=12):
    """Register two clouds of any two sizes with neither a network nor a starting pose: src [B,3,Ns], tgt [B,3,Nt] (float32
    device tensors).  compute_fpfh_feature(k, radius) on both, match_features(mutual), ransac_correspondences(max_dist,
    trials, similarity, seed), then score_registration at max_dist on the FULL clouds (Open3D's closing evaluation).
    refine: a correspondence cap; refine_registration(method=refine_method, max_dist=refine) then runs from the RANSAC's pose.
    src_normals, tgt_normals [B,3,N]: the clouds' normals for the features; None estimates them (estimate_normals, from the
    features' own search).  An estimated normal's SIGN is arbitrary, and the feature of a point changes with it: two copies of
    one surface match far better with normals oriented alike than with estimated ones -- on the test's surface 99.7 % of the
    one-way matches are the true partner against 18 % at 600 points.  Two remedies: normals oriented
    towards a sensor position where one is known (``estimate_normals(viewpoint=)``), or orient="tangent" where none is -- a
    registered scan, a merged cloud, a mesh sample.
    orient: None uses the normals as they are.  "tangent" (DESIGN.md section 4.26): every side whose normals are ESTIMATED has
    them oriented by ``orient_normals_consistent_tangent_plane(k=orient_k)`` before its features are computed; given normals
    are used as they are.  That leaves one global sign per cloud, so where at least one side was estimated the chain --
    features, matching, RANSAC or FGR, score -- runs TWICE, once with the source's normals as oriented and once with all of
    them negated, and per cloud the run with the higher fitness is kept on the device -- where the fitness is equal the one
    with the lower inlier_rmse (two runs that both end with every point an inlier differ there by orders of magnitude), and
    the oriented run among equals --: every key of the dict is selected per cloud, `flipped` bool [B] says which run it was,
    and refine runs once, from the kept pose.
    The second run costs the source's features, the matching, the RANSAC or FGR and a score again (DESIGN.md section 4.26
    states it as measured).
    method: "ransac", or "fgr": fast_global_registration (``fgr``) takes the RANSAC's place -- no trial
    budget; trials, similarity and seed are not used, `fgr` is a dict of its keywords (tuple_scale, max_tuples, iterations,
    division_factor, mu_floor, decrease_mu, tuple_trials, seed).  The score and refine work from its pose in the same way.
    "consistency": consistency_registration (``consistency``) takes the RANSAC's place -- pairwise
    length-consistency voting, for matches of which most are wrong; trials, similarity and seed are not used, `consistency` is
    a dict of its keywords (tau, keep, seeds, ratio, min_length).
    Returns a dict: fitness, inlier_rmse, inliers (the score of the global pose); R, t, best_trial, pairs and ransac_inliers
    (the RANSAC's; its `inliers` under that name) -- with "fgr": R, t, pairs, tuples, used, status; with "consistency": R, t,
    pairs, best_seed, consistency_inliers --; corr int32 [B,Ns]; and with refine, `refined`: refine_registration's dict.
    centre: False works in the caller's frame; True, or a pair (c_src, c_tgt) of [B,3] tensors, runs the whole chain --
    features, matching, RANSAC or FGR, score and refine -- on the clouds moved each to its own centre (``centred``), carries every
    pose back (``uncentred_pose``) and takes every score on the caller's clouds.  For clouds far from the origin relative to their
    extent: the features' and the normals' search cancels there in fp32.  ransac_inliers stays the
    RANSAC's own count.
    search: handed to both compute_fpfh_feature calls: "knn" is the brute-force search on the points' rows, "grid" takes the
    features' and the normals' neighbours from ``search_knn`` -- distances of differences, so the
    features need no centring, and a point excluded from its own row by its index.  It means the feature stages' kNN and
    nothing more.  "radius" (DESIGN.md section 4.23): the features and their normals over ALL points within `radius`, or the
    nearest max_nn of them (any max_nn >= 1: Open3D's hybrid search); radius, max_nn and capacity go to both
    compute_fpfh_feature calls as they are, and k is not read.
    ``nn_search``: the ``search`` of the score and refine steps: "scan" (the default) or "grid", the target's uniform grid
     -- the same poses and scores bit for bit, faster on large clouds.
    keypoints: None matches every source point.  "iss" (DESIGN.md section 4.27): ``compute_iss_keypoints(src, **iss)`` -- `iss` a
    dict of its keywords (salient_radius, non_max_radius, gamma_21, gamma_32, min_neighbors, capacity, cell, and border_radius,
    normal_radius, border_angle, normals of its rule against the scan's rim) -- picks the source's
    keypoints, and directly behind match_features corr[b, i] becomes -1 where source point i is not one: the RANSAC or FGR
    draws from the keypoints' pairs alone.  The features are still computed on the whole clouds and the target is searched
    whole; the score and refine steps use every point.  Under orient="tangent" both runs take the same mask.
    describe: "all" is that path.  "keypoints" (needs keypoints="iss" and search="radius") computes the
    SOURCE's features at the keypoints alone -- ``compute_fpfh_feature(src, ..., query_index=index)`` with
    ``compute_iss_keypoints``' index, the count left on the device: the padded slots are NaN centres with empty rows and NaN
    features, which never win a match.  Given normals, and under orient="tangent" the oriented ones, are the whole cloud's.
    match_features runs on those [B,33,Ns] columns against the whole target and its result is scattered to corr [B,Ns], -1
    elsewhere.  With mutual=False every key equals describe="all" bit for bit.  With mutual=True the reverse search runs among
    the KEYPOINTS' features alone: a pair (i, j) is kept where keypoint i is the nearest KEYPOINT of j, not the nearest source
    point -- a different definition, and the one a keypoint pipeline means; "all" asks more of a pair and keeps fewer.  The
    target side stays whole."""
    from . import grid, gridnn, rows
    feat = dict(k=k, radius=radius, search=search)          # what both compute_fpfh_feature calls take
    if rows.radius_arguments("register_features", search, radius, max_nn, capacity):
        feat.update(max_nn=max_nn, capacity=capacity)
    else:
        grid.check_search("register_features", search)
    gridnn.check_search("register_features", nn_search, "nn_search")
    if orient not in (None, "tangent"):
        raise VcrHipError(f'register_features: orient must be None or "tangent", got {orient!r}')
    if isinstance(orient_k, bool) or not isinstance(orient_k, int) or orient_k < 1:
        raise VcrHipError(f"register_features: orient_k must be an integer >= 1, got {orient_k!r}")
    iss = _keypoint_arguments("register_features", keypoints, iss)
    if describe not in ("all", "keypoints") or not isinstance(describe, str):
        raise VcrHipError(f'register_features: describe must be "all" or "keypoints", got {describe!r}')
    if describe == "keypoints" and (keypoints != "iss" or search != "radius"):
        raise VcrHipError(f'register_features: describe="keypoints" needs keypoints="iss" and search="radius", got '
                          f"keypoints={keypoints!r}, search={search!r}")
    if centre is not False and centre is not None:
        return _register_centred(src, tgt, max_dist, centre, refine,
                                 dict(k=k, radius=radius, mutual=mutual, trials=trials, similarity=similarity, seed=seed,
                                      refine=refine, refine_method=refine_method, src_normals=src_normals,
                                      tgt_normals=tgt_normals, method=method, fgr=fgr, consistency=consistency, search=search,
                                      nn_search=nn_search,
                                      max_nn=max_nn, capacity=capacity, orient=orient, orient_k=orient_k,
                                      keypoints=keypoints, iss=iss or None, describe=describe))
    from .fpfh import compute_fpfh_feature
    from .refine import refine_registration
    from .score import score_registration
    api = "register_features"
    if refine is not None and not (math.isfinite(float(refine)) and float(refine) >= 0.0):
        raise VcrHipError(f"{api}: refine must be None or a finite correspondence cap >= 0, got {refine}")
    if method not in ("ransac", "fgr", "consistency"):
        raise VcrHipError(f'{api}: method must be "ransac" or "fgr" or "consistency", got {method!r}')
    if fgr is not None and method != "fgr":
        raise VcrHipError(f'{api}: fgr= holds the keywords of method="fgr"; the method is "{method}"')
    if consistency is not None and method != "consistency":
        raise VcrHipError(f'{api}: consistency= holds the keywords of method="consistency"; the method is "{method}"')
    if method == "fgr":
        return _register_fgr(api, src, tgt, max_dist, feat, mutual, refine, refine_method, src_normals, tgt_normals, fgr, nn_search,
                             orient, orient_k, keypoints, iss, describe)
    if method == "consistency":
        return _register_consistency(api, src, tgt, max_dist, feat, mutual, refine, refine_method, src_normals, tgt_normals,
                                     consistency, nn_search, orient, orient_k, keypoints, iss, describe)
    _ransac_checks(api, src, tgt, None, max_dist, trials, similarity, seed, given_corr=False)
    keep, index = _keypoint_mask(src, keypoints, iss, describe)

    def tail(src_feat, tgt_feat):
        corr = _placed(match_features(src_feat, tgt_feat, mutual=mutual), keep, index)
        r = ransac_correspondences(src, tgt, corr, max_dist, trials, similarity, seed)
        res = dict(score_registration(src, tgt, r["R"], r["t"], max_dist, search=nn_search))
        res.update(R=r["R"], t=r["t"], best_trial=r["best_trial"], pairs=r["pairs"], ransac_inliers=r["inliers"], corr=corr)
        return res
    res = _both_signs(src, tgt, src_normals, tgt_normals, feat, orient, orient_k, tail, index)
    if refine is not None:
        res["refined"] = refine_registration(src, tgt, res["R"], res["t"], float(refine), method=refine_method, search=nn_search)
    return res


ISS_KEYWORDS = ("salient_radius", "non_max_radius", "gamma_21", "gamma_32", "min_neighbors", "capacity", "cell", "border_radius",
                "normal_radius", "border_angle", "normals")


def _keypoint_arguments(api, keypoints, iss):
    """What register_features asks of (keypoints, iss) in front of everything else -> iss as a dict."""
    if keypoints not in (None, "iss") or isinstance(keypoints, bool):
        raise VcrHipError(f'{api}: keypoints must be None or "iss", got {keypoints!r}')
    if iss is not None and (not isinstance(iss, dict) or set(iss) - set(ISS_KEYWORDS)):
        raise VcrHipError(f"{api}: iss must be None or a dict with keys among {sorted(ISS_KEYWORDS)}, got "
                          f"{sorted(iss) if isinstance(iss, dict) else type(iss).__name__}")
    if iss is not None and keypoints is None:
        raise VcrHipError(f'{api}: iss= holds the keywords of keypoints="iss"; keypoints is None')
    iss = {} if iss is None else dict(iss)
    if keypoints is not None:
        from .iss import check_arguments
        check_arguments(api, **iss)
    return iss


def _keypoint_mask(src, keypoints, iss, describe="all"):
    """-> (bool [B,Ns]: the source points that keep their match, None where every point does; with describe="keypoints" the
    keypoints' index int32 [B,Ns], -1 behind the count, else None)."""
    if keypoints is None:
        return None, None
    from .iss import compute_iss_keypoints
    try:
        got = compute_iss_keypoints(src, want_flag=True, **iss)
        return got[3] > 0, (got[2] if describe == "keypoints" else None)
    except VcrHipError as e:
        raise VcrHipError(str(e).replace("compute_iss_keypoints", 'register_features (keypoints="iss")', 1)) from None


def _masked(corr, keep):
    """match_features' corr with -1 (no partner) where keep is False: a device `where`."""
    return corr if keep is None else torch.where(keep, corr, torch.full_like(corr, -1))


def _placed(corr, keep, index):
    """corr [B,Ns] in the source's numbering: match_features' result masked (index None: it already is in that numbering), or
    -- the matches of the keypoints' columns -- scattered to the keypoints' indices, -1 elsewhere and for slots behind the count."""
    if index is None:
        return _masked(corr, keep)
    B, Ns = index.shape
    ok = index >= 0
    at = torch.where(ok, index, torch.full_like(index, Ns)).long()       # (a padded slot goes behind the end)
    out = torch.full((B, Ns + 1), -1, dtype=corr.dtype, device=corr.device)
    out.scatter_(1, at, torch.where(ok, corr, torch.full_like(corr, -1)))
    return out[:, :Ns].contiguous()


def _estimated_normals(xyz, feat):
    """The normals compute_fpfh_feature(xyz, None, **feat) estimates for itself, bit for bit: the same call on the same search."""
    from .plane import estimate_normals
    if feat["search"] == "radius":
        return estimate_normals(xyz, search="radius", radius=feat["radius"], max_nn=feat["max_nn"], capacity=feat["capacity"])
    return estimate_normals(xyz, feat["k"], search=feat["search"])


def _both_signs(src, tgt, src_normals, tgt_normals, feat, orient, orient_k, tail, src_index=None):
    """The features of both clouds (feat: the keywords of both compute_fpfh_feature calls) and tail(src_feat, tgt_feat) -> the
    result's dict: matching, RANSAC or FGR, score.  orient="tangent": a side without given normals has them estimated and
    oriented first; where there is such a side the tail runs a second time on the features of the source's normals negated, and
    every entry is taken per cloud from the run with the higher fitness -- the lower inlier_rmse where the fitness is equal --,
    the first among equals; `flipped` bool [B].  src_index: describe="keypoints" -- the source's features at those indices alone."""
    from .fpfh import compute_fpfh_feature
    at = {} if src_index is None else dict(query_index=src_index)
    if orient is None:
        return tail(compute_fpfh_feature(src, src_normals, **feat, **at), compute_fpfh_feature(tgt, tgt_normals, **feat))
    from .orient import orient_normals_consistent_tangent_plane
    twice = src_normals is None or tgt_normals is None
    if src_normals is None:
        src_normals = orient_normals_consistent_tangent_plane(src, _estimated_normals(src, feat), k=orient_k)
    if tgt_normals is None:
        tgt_normals = orient_normals_consistent_tangent_plane(tgt, _estimated_normals(tgt, feat), k=orient_k)
    src_feat, tgt_feat = compute_fpfh_feature(src, src_normals, **feat, **at), compute_fpfh_feature(tgt, tgt_normals, **feat)
    res = tail(src_feat, tgt_feat)
    flipped = torch.zeros(src.shape[0], dtype=torch.bool, device=res["fitness"].device)
    if twice:
        other = tail(compute_fpfh_feature(src, -src_normals, **feat, **at), tgt_feat)
        # fitness first, then the lower inlier_rmse (Open3D's order of two RANSAC results): on clean copies BOTH runs can end
        # with every point an inlier -- a few correct matches among many wrong ones still find a pose -- and the fitness ties
        flipped = (other["fitness"] > res["fitness"]) | ((other["fitness"] == res["fitness"])
                                                         & (other["inlier_rmse"] < res["inlier_rmse"]))
        for key, a in res.items():
            res[key] = torch.where(flipped.view((-1,) + (1,) * (a.dim() - 1)), other[key], a)
    res["flipped"] = flipped
    return res


def _register_fgr(api, src, tgt, max_dist, feat, mutual, refine, refine_method, src_normals, tgt_normals, kw, nn_search="scan",
                  orient=None, orient_k=12, keypoints=None, iss=None, describe="all"):
    """register_features with method="fgr": the same chain with fast_global_registration in the RANSAC's place.  feat: the
    keywords of both compute_fpfh_feature calls."""
    from . import fgr as F
    from .fpfh import compute_fpfh_feature
    from .refine import refine_registration
    from .score import score_registration
    kw = {} if kw is None else kw
    if not isinstance(kw, dict) or set(kw) - set(F.DEFAULTS):
        raise VcrHipError(f"{api}: fgr must be None or a dict with keys among {sorted(F.DEFAULTS)}, got "
                          f"{sorted(kw) if isinstance(kw, dict) else type(kw).__name__}")
    kw = dict(F.DEFAULTS, **kw)
    max_dist = float(max_dist)
    if not (math.isfinite(max_dist) and max_dist >= 0.0):
        raise VcrHipError(f"{api}: max_dist must be finite and >= 0, got {max_dist}")
    F._fgr_checks(api, src, tgt, None, kw["tuple_scale"], kw["max_tuples"], kw["iterations"], kw["division_factor"], kw["mu_floor"],
                  kw["tuple_trials"], kw["seed"], given_corr=False)
    keep, index = _keypoint_mask(src, keypoints, iss, describe)

    def tail(src_feat, tgt_feat):
        corr = _placed(match_features(src_feat, tgt_feat, mutual=mutual), keep, index)
        r = F.fast_global_registration(src, tgt, corr, **kw)
        res = dict(score_registration(src, tgt, r["R"], r["t"], max_dist, search=nn_search))
        res.update(R=r["R"], t=r["t"], pairs=r["pairs"], tuples=r["tuples"], used=r["used"], status=r["status"], corr=corr)
        return res
    res = _both_signs(src, tgt, src_normals, tgt_normals, feat, orient, orient_k, tail, index)
    if refine is not None:
        res["refined"] = refine_registration(src, tgt, res["R"], res["t"], float(refine), method=refine_method, search=nn_search)
    return res


def _register_consistency(api, src, tgt, max_dist, feat, mutual, refine, refine_method, src_normals, tgt_normals, kw,
                          nn_search="scan", orient=None, orient_k=12, keypoints=None, iss=None, describe="all"):
    """register_features with method="consistency": the same chain with consistency_registration in the RANSAC's place.  feat:
    the keywords of both compute_fpfh_feature calls."""
    from . import consistency as K
    from .refine import refine_registration
    from .score import score_registration
    kw = {} if kw is None else kw
    if not isinstance(kw, dict) or set(kw) - set(K.DEFAULTS):
        raise VcrHipError(f"{api}: consistency must be None or a dict with keys among {sorted(K.DEFAULTS)}, got "
                          f"{sorted(kw) if isinstance(kw, dict) else type(kw).__name__}")
    kw = dict(K.DEFAULTS, **kw)
    K._checks(api, src, tgt, None, max_dist, kw["tau"], kw["keep"], kw["seeds"], kw["ratio"], kw["min_length"], given_corr=False)
    keep, index = _keypoint_mask(src, keypoints, iss, describe)

    def tail(src_feat, tgt_feat):
        corr = _placed(match_features(src_feat, tgt_feat, mutual=mutual), keep, index)
        r = K.consistency_registration(src, tgt, corr, max_dist, **kw)
        res = dict(score_registration(src, tgt, r["R"], r["t"], float(max_dist), search=nn_search))
        res.update(R=r["R"], t=r["t"], pairs=r["pairs"], best_seed=r["best_seed"], consistency_inliers=r["inliers"], corr=corr)
        return res
    res = _both_signs(src, tgt, src_normals, tgt_normals, feat, orient, orient_k, tail, index)
    if refine is not None:
        res["refined"] = refine_registration(src, tgt, res["R"], res["t"], float(refine), method=refine_method, search=nn_search)
    return res


def _register_centred(src, tgt, max_dist, centre, refine, kw):
    """register_features(centre=...): the chain on the centred clouds, the poses and scores in the caller's frame."""
    from .centre import take_centres, uncentred_pose
    from .refine import uncentre_refined
    from .score import score_registration
    api = "register_features"
    extension.check_cloud(api, "src", src)
    extension.check_cloud(api, "tgt", tgt)
    src_c, c_src, tgt_c, c_tgt = take_centres(api, centre, src, tgt)
    res = register_features(src_c, tgt_c, max_dist, centre=False, **kw)
    _, res["t"] = uncentred_pose(res["R"], res["t"], c_src, c_tgt)
    res.update(score_registration(src, tgt, res["R"], res["t"], float(max_dist), search=kw["nn_search"]))
    if "refined" in res:
        res["refined"] = uncentre_refined(res["refined"], src, tgt, c_src, c_tgt, float(refine), search=kw["nn_search"])
    return res
