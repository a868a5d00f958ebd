"""include/consistency/vcr_hip_consistency.h without a GPU: the boundary -- the header as C and as
C++, the prototypes, the struct's layout, the error codes, the host-only plan and workspace queries, the build's lists, the
kernels' resources --, the numpy restatement (tests/consistency_restated.py) on the planted recipe and under the symmetries
the definition promises, and what the four Python calls refuse."""
import ctypes
import os
import subprocess

import numpy as np
import pytest
import torch

import boundary
import consistency_restated as cr
import match_restated as mr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INCLUDE = os.path.join(ROOT, "include")
HEADER = os.path.join(INCLUDE, "consistency", "vcr_hip_consistency.h")
EINVAL, EWORKSPACE, EUNSUPPORTED = -1, -2, -3
ENTRY_POINTS = {"vcr_consistency_f32", "vcr_consistency_workspace_bytes", "vcr_consistency_form"}
KERNELS = {"consistency_pairs_kernel", "consistency_degree_kernel<1, false>", "consistency_degree_kernel<2, false>",
           "consistency_degree_kernel<4, false>", "consistency_degree_kernel<1, true>", "consistency_degree_kernel<2, true>",
           "consistency_degree_kernel<4, true>", "consistency_merge_kernel", "rs_hist_kernel<9, 4>", "rs_scan_kernel<9>",
           "rs_scatter_kernel<9, 4>", "consistency_kept_kernel", "consistency_adj_kernel", "consistency_seed_kernel",
           "consistency_count_kernel", "consistency_best_kernel"}
PLANTED = ((300, 0.10), (1000, 0.05), (2000, 0.02), (4000, 0.01))       # (M, share of right pairs)
TAU, KEEP, SEEDS = 0.01, 512, 32


@pytest.fixture(scope="module")
def lib():
    import vcrnet_amd  # noqa: F401
    from vcrnet_amd import build, consistency
    build.build()
    return consistency.lib()


# ----------------------------------------------------------------------------------------------------------------- the boundary

@pytest.mark.parametrize("language,compiler", [("c", "gcc"), ("c++", "g++")])
def test_the_header_compiles_as_c_and_as_cpp(language, compiler, tmp_path):
    src = tmp_path / ("use." + ("c" if language == "c" else "cpp"))
    src.write_text('#include "consistency/vcr_hip_consistency.h"\n'
                   "int main(void) { vcr_consistency_args a; a.struct_bytes = sizeof a; return a.struct_bytes == 0; }\n")
    r = subprocess.run([compiler, "-x", language, "-Wall", "-Werror", "-pedantic", "-fsyntax-only", "-I", INCLUDE, str(src)],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr


def test_signatures_match_the_header_and_the_library_exports_them(lib):
    from vcrnet_amd import consistency
    boundary.check_signatures(HEADER, consistency, lib, ENTRY_POINTS)


def test_args_match_the_c_layout(tmp_path):
    import vcrnet_amd  # noqa: F401
    from vcrnet_amd import consistency
    boundary.check_layout(HEADER, consistency, tmp_path)
    A = consistency.ConsistencyArgs
    assert A.best_seed.offset == A.t_out.offset + 8           # where the mandatory part ends


def test_the_call_lives_beside_the_other_headers_not_in_them(lib):
    """No other public header mentions it, the ABI version and vcr_hip.h's prototypes are where they were; the header enters
    the digest of consistency.o alone; the pair list, the draws' hash and the count's distance are one text for the three
    global methods, and ransac.hip keeps nothing of its own of them."""
    from vcrnet_amd import build, consistency, fgr, match, native
    for d, _, files in os.walk(INCLUDE):
        for f in files:
            if os.path.join(d, f) != HEADER:
                assert "vcr_consistency" not in open(os.path.join(d, f)).read(), f
    assert lib.vcr_abi_version() == native.ABI_VERSION == 27
    for other in (native, match, fgr):
        assert not set(consistency.SIGNATURES) & set(other.SIGNATURES) and not set(consistency.STRUCTS) & set(other.STRUCTS)
    assert not set(consistency.SIGNATURES) & set(native.PUBLIC)
    assert build.CONSISTENCY_HEADERS == [HEADER] and build.OWN_HEADERS["consistency.hip"] is build.CONSISTENCY_HEADERS
    assert [k for k, v in build.OWN_HEADERS.items() if HEADER in v] == ["consistency.hip"]
    assert "#define VCR_CONSISTENCY_MAX_KEEP %d" % consistency.MAX_KEEP in open(HEADER).read()
    assert (consistency.MAX_N, consistency.MAX_SPLITS) == (match.MAX_N, match.MAX_SPLITS)
    csrc = os.path.join(ROOT, "vcr-net_amd", "csrc")
    for f, kernel in (("ransac.hip", "ransac_pairs_kernel"), ("consistency.hip", "consistency_pairs_kernel")):
        text = open(os.path.join(csrc, f)).read()
        assert '#include "corr_pairs.h"' in text and "float rs_d2(" not in text and "rs_d2(P, " in text, f
        assert "void %s(RsPairs p) { rs_pairs_body(p); }" % kernel in text, f
    assert open(os.path.join(csrc, "corr_pairs.h")).read().count("float rs_d2(") == 1


def _cs(**kw):
    from vcrnet_amd import consistency
    a = consistency.ConsistencyArgs()
    a.src, a.tgt, a.corr, a.R_out, a.t_out = 0x1000, 0x2000, 0x3000, 0x4000, 0x5000   # (never dereferenced on the host)
    v = dict(B=2, Ns=1000, Nt=900, tau=0.01, min_length=0.0, max_dist=0.02, ratio=0.5, keep=512, seeds=32)
    v.update(kw)
    for k, x in v.items():
        setattr(a, k, x)
    return a


def test_argument_errors_return_their_codes_without_a_gpu(lib):
    from vcrnet_amd import consistency

    def codes(a):
        rc = lib.vcr_consistency_f32(ctypes.byref(a), 0x10000, 1 << 40, None)
        assert lib.vcr_consistency_workspace_bytes(ctypes.byref(a), 256) == 0
        assert lib.vcr_consistency_form(ctypes.byref(a), 256, None, None, None) == rc
        return rc
    assert lib.vcr_consistency_f32(None, None, 0, None) == EINVAL and lib.vcr_consistency_workspace_bytes(None, 256) == 0
    for field in ("src", "tgt", "corr", "R_out", "t_out"):
        a = _cs()
        setattr(a, field, None)
        assert codes(a) == EINVAL, field
    nan, inf = float("nan"), float("inf")
    for kw in (dict(B=0), dict(Ns=0), dict(Nt=0), dict(B=-1), dict(tau=-0.1), dict(tau=nan), dict(tau=inf), dict(max_dist=-1.0),
               dict(max_dist=nan), dict(max_dist=inf), dict(min_length=-1.0), dict(min_length=nan), dict(min_length=inf),
               dict(ratio=-0.1), dict(ratio=1.1), dict(ratio=nan), dict(keep=0), dict(keep=63), dict(keep=100), dict(keep=4160),
               dict(seeds=0), dict(seeds=513), dict(variant=3), dict(variant=8), dict(variant=129 << 8), dict(variant=1 << 16), dict(variant=0x30), dict(variant=0x31), dict(variant=0x40),
               dict(stop_after=-1), dict(stop_after=3)):
        assert codes(_cs(**kw)) == EINVAL, kw
    for kw in (dict(Ns=131073), dict(Nt=131073), dict(B=16384, Ns=131072), dict(B=1 << 21)):
        assert codes(_cs(**kw)) == EUNSUPPORTED, kw
    size = ctypes.sizeof(consistency.ConsistencyArgs)
    for bad in (0, consistency.ConsistencyArgs.best_seed.offset - 8, size + 8):
        a = _cs()
        a.struct_bytes = bad
        assert codes(a) == EINVAL, bad
    # the degrees and the kept pairs alone need no pose
    for stop in (1, 2):
        a = _cs(stop_after=stop)
        a.R_out = a.t_out = None
        assert lib.vcr_consistency_workspace_bytes(ctypes.byref(a), 256) > 0


def test_the_plan_and_the_workspace_are_host_only_queries(lib):
    """With an explicit cu_count nothing touches a device.  The plan is the feature search's rule on (B, Ns, Ns): the most pairs
    per lane that leave 16 workgroups a CU within reach, then the streamed side cut into segments of at least 64 until they
    exist; a forced form is what it says."""
    from vcrnet_amd import consistency
    form, variant = consistency.consistency_form, consistency.variant

    def plan(B, Ns, cu):                                      # restated from the header's words and seg_scan.h's
        fill = 16 * cu
        most = max(1, min(Ns // 64, 128))
        for Q in (4, 2, 1):
            groups = B * -(-Ns // (256 * Q))
            if groups * most >= fill or Q == 1:
                return Q, (1 if groups >= fill else min(-(-fill // groups), most))
    for B, Ns, cu in ((16, 1024, 256), (16, 16384, 256), (1, 131072, 256), (1, 100, 256), (3, 5000, 104), (1, 131072, 1),
                      (64, 131072, 256)):
        q, s, ws = form(B, Ns, Ns, cu_count=cu)
        assert (q, s) == plan(B, Ns, cu), (B, Ns, cu, q, s)
        assert ws > 0 and ws % 256 == 0
    for Q in (1, 2, 4):
        for S in (1, 5, 128):
            for pre in (False, True):
                assert form(2, 3000, 2000, variant=variant(Q, S, pre), want_pretest=True)[::3] == (Q, pre)
                assert form(2, 3000, 2000, variant=variant(Q, S, pre))[:2] == (Q, S)
    assert form(2, 3000, 2000, variant=variant(2, 0))[0] == 2
    # the plan runs the pre-test from two pairs a lane (profiles/consistency_bench.txt: it wins there and loses at one), a
    # forced pair count included; forcing it moves neither Q nor S
    assert (variant(), variant(pretest=True), variant(pretest=False)) == (0, 0x10, 0x20)
    for B, Ns in ((16, 1024), (16, 16384), (1, 131072), (1, 100)):
        planned = form(B, Ns, Ns, want_pretest=True)
        assert planned[3] is (planned[0] >= 2), (B, Ns, planned)
        for pre in (False, True):
            assert form(B, Ns, Ns, variant=variant(pretest=pre), want_pretest=True) == planned[:3] + (pre,)
    assert [form(2, 3000, 2000, variant=variant(Q), want_pretest=True)[3] for Q in (1, 2, 4)] == [False, True, True]
    assert form(16, 1024, 1024, want_pretest=True)[::3] == (1, False) and form(16, 16384, 16384, want_pretest=True)[::3] == (4, True)
    text = open(HEADER).read()
    assert "#define VCR_CONSISTENCY_PRETEST_ON 0x10" in text and "#define VCR_CONSISTENCY_PRETEST_OFF 0x20" in text
    # the workspace: every part, 256-B aligned, and the optional outputs take their parts out of it
    up = lambda v: (v + 255) & ~255                                               # noqa: E731
    B, Ns, keep, seeds = 2, 1000, 512, 32
    q, s, ws = form(B, Ns, 900, keep, seeds, cu_count=256)
    W, nt, nseg = keep // 64, -(-Ns // 1024), -(-Ns // 1024)
    fixed = (up(B * Ns * 32) + 3 * up(B * 4) + up(s * B * Ns * 4) + 2 * up(B * Ns * 8) + 2 * up(B * Ns * 4) + up(B * nt * 512 * 4)
             + up(B * 512 * 4) + up(B * keep * 32) + up(B * nseg * seeds * 4))
    assert ws == fixed + up(B * keep * W * 8) + up(B * seeds * 4) + up(B * seeds * 48)
    assert form(B, Ns, 900, keep, seeds, cu_count=256, stages=True)[2] == fixed
    a = _cs()
    assert lib.vcr_consistency_workspace_bytes(ctypes.byref(a), 256) == ws
    assert lib.vcr_consistency_workspace_bytes(ctypes.byref(a), -1) == 0
    assert lib.vcr_consistency_f32(ctypes.byref(a), None, ws, None) == EINVAL
    assert lib.vcr_consistency_f32(ctypes.byref(a), 0x10008, ws, None) == EINVAL
    a.struct_bytes = consistency.ConsistencyArgs.best_seed.offset                # the mandatory part alone
    assert lib.vcr_consistency_workspace_bytes(ctypes.byref(a), 256) == ws


def test_the_new_kernels_use_no_scratch():
    import vcrnet_amd  # noqa: F401
    from vcrnet_amd import build
    build.build()
    res = build.kernel_resources()
    names = list(res)
    dem = subprocess.run(["c++filt"], input="\n".join(names), capture_output=True, text=True, check=True).stdout.splitlines()
    mine = {d.replace("(anonymous namespace)::", "").replace("void ", "").split("(")[0]: res[n]
            for n, d in zip(names, dem) if res[n]["file"] == "consistency.hip"}
    assert set(mine) == KERNELS
    for d, v in mine.items():
        print(d, v)
        assert v.get("scratch", 0) == 0 and v.get("vgpr_spill", 0) == 0, (d, v)
    for Q in (1, 2, 4):                                       # the hot path: registers alone, eight waves a SIMD
        for pre in ("false", "true"):
            deg = mine["consistency_degree_kernel<%d, %s>" % (Q, pre)]
            assert deg["lds"] == 0 and deg["occupancy"] == 8, (Q, pre, deg)
    # a seed's workgroup: two rows of bits, w[r][.] of 4096 columns, four wave maxima
    assert mine["consistency_seed_kernel"]["lds"] <= 2 * 64 * 8 + 4096 * 4 + 16 + 16


# ------------------------------------------------------------------------------------------------------------- the restatement

def pose_error(o, c):
    """(the angle of R R_planted^T in degrees -- by its skew part: an arccos of a cosine that close to 1 resolves 0.02 degrees --,
    the largest |dt|)."""
    E = o["R"].astype(np.float64) @ c["R"].T
    sine = 0.5 * np.linalg.norm([E[2, 1] - E[1, 2], E[0, 2] - E[2, 0], E[1, 0] - E[0, 1]])
    return float(np.degrees(np.arctan2(sine, (np.trace(E) - 1) / 2))), float(np.abs(o["t"].astype(np.float64) - c["t"]).max())


@pytest.mark.parametrize("M,share", PLANTED)
def test_the_restatement_recovers_the_planted_pose(M, share):
    """Down to one right pair in a hundred: every right pair is kept, the best seed is one, its members are exactly the right
    pairs, and the pose is the planted one to fp32 -- where 100 000 RANSAC trials would draw three right pairs 0.1 times."""
    c = mr.planted(M, share)
    o = cr.consistency(c["src"], c["tgt"], c["corr"], TAU, TAU, KEEP, SEEDS)
    good = np.nonzero(c["good"])[0]
    kept = o["pl"][o["order"]]
    bs = o["best_seed"]
    assert o["pairs"] == M and len(kept) == min(M, KEEP) and np.isin(good, kept).all()
    assert bs >= 0 and c["good"][kept[bs]] and o["status"][bs] == 0
    assert np.array_equal(np.sort(kept[o["member"][bs]]), good)
    assert o["inliers"] >= len(good) and o["n"][bs] == len(good)
    deg, dt = pose_error(o, c)
    print(f"consistency restated M {M} share {share}: best seed {bs}, {o['n'][bs]} members, {o['inliers']} inliers, "
          f"rotation {deg:.2e} deg, |dt| {dt:.2e}; degrees of the right pairs {o['deg'][np.isin(o['pl'], good)].min()} ... , "
          f"of the others at most {o['deg'][~np.isin(o['pl'], good)].max()}")
    # the partners and the pose are rounded to fp32, 6e-8 a coordinate at most: 3.5e-7 rad and 2e-7 leave a factor of three
    assert deg <= 2e-5 and dt <= 2e-7, (deg, dt)


def test_the_restatement_at_its_edges():
    c = mr.planted(40, 0.5, extra=5)
    none = cr.consistency(c["src"], c["tgt"], np.full(45, -1), TAU, keep=64, seeds=8)
    assert (none["pairs"], none["best_seed"], none["inliers"]) == (0, -1, 0) and (none["status"] == 1).all()
    assert np.array_equal(none["R"], np.eye(3, dtype=np.float32)) and not none["t"].any() and (none["count"] == -1).all()
    two = c["corr"].copy()
    two[np.nonzero(c["good"])[0][2:]] = -1
    two[~c["good"]] = -1
    o = cr.consistency(c["src"], c["tgt"], two, TAU, keep=64, seeds=8)
    assert o["pairs"] == 2 and (o["deg"] == 1).all() and (o["n"][:2] == 2).all() and o["best_seed"] == -1
    three = c["corr"].copy()
    three[np.nonzero(c["good"])[0][3:]] = -1
    three[~c["good"]] = -1
    o = cr.consistency(c["src"], c["tgt"], three, TAU, keep=64, seeds=8)
    assert o["pairs"] == 3 and (o["deg"] == 2).all() and o["best_seed"] == 0 and o["inliers"] == 3 and (o["status"][3:] == 1).all()
    # equal degrees keep the lower position; the words' layout
    assert cr.kept_order(np.asarray([3, 5, 3, 5, 0]), 64).tolist() == [1, 3, 0, 2, 4]
    assert cr.kept_order(np.asarray([3, 5, 3, 5, 0]), 2).tolist() == [1, 3]
    bits = np.zeros(130, bool)
    bits[[0, 63, 64, 129]] = True
    words = cr.pack(bits, 192)
    assert words.tolist() == [1 | 1 << 63, 1, 2] and np.array_equal(cr.unpack(words, 130), bits)
    # the sum order: 64 chains, then the butterfly -- not the running sum
    e = 2.0 ** -53
    v = np.asarray([1.0, e, e, e] + [0.0] * 60 + [e], np.float64)     # rank 64 joins chain 0: 1 + e rounds to 1 there
    assert cr.chain_sum(v, np.ones(65, bool)) == 1.0 + 2 * e and np.cumsum(v)[-1] == 1.0     # (1 + e) + (e + e), exactly 1 + 4 e
    assert cr.chain_sum(v, ~np.isin(np.arange(65), (1, 3))) == 1.0    # a rank that is no member adds nothing: 1 + e twice


def test_the_degree_is_symmetric_in_the_roles_of_the_two_clouds():
    c = mr.planted(300, 0.1)
    pl, P, Q = cr.rows(c["src"], c["tgt"], c["corr"])
    deg = cr.degree(P, Q, TAU, 0.05)
    back = np.full(300, -1, np.int64)
    back[c["corr"][pl]] = pl                                  # the target's partner: the recipe's corr is one to one
    pl2, P2, Q2 = cr.rows(c["tgt"], c["src"], back)
    deg2 = cr.degree(P2, Q2, TAU, 0.05)
    assert np.array_equal(cr.deg_by_source(deg2, pl2, 300)[c["corr"][pl]], deg) and deg.max() >= 29


def test_the_degree_follows_a_permutation_and_ignores_an_exact_translation():
    c = mr.planted(300, 0.1, extra=7)
    lattice = lambda x: (np.round(x * 4096) / 4096).astype(np.float32)            # noqa: E731  (2^-12: a shift by integers is exact)
    src, tgt = lattice(c["src"]), lattice(c["tgt"])
    pl, P, Q = cr.rows(src, tgt, c["corr"])
    deg = cr.deg_by_source(cr.degree(P, Q, TAU), pl, 307)
    assert (deg[300:] == -1).all() and (deg[:300] >= 0).all()
    perm = np.random.RandomState(3).permutation(307)
    pl2, P2, Q2 = cr.rows(src[:, perm], tgt, c["corr"][perm])
    assert np.array_equal(cr.deg_by_source(cr.degree(P2, Q2, TAU), pl2, 307), deg[perm])
    moved_s = src + np.asarray([[3], [-2], [1]], np.float32)
    moved_t = tgt + np.asarray([[-1], [4], [2]], np.float32)
    assert np.array_equal(moved_s - np.asarray([[3], [-2], [1]], np.float32), src)
    pl3, P3, Q3 = cr.rows(moved_s, moved_t, c["corr"])
    assert np.array_equal(cr.deg_by_source(cr.degree(P3, Q3, TAU), pl3, 307), deg)


# ------------------------------------------------------------------------------------------------------------ the Python layer

def test_python_entry_points_refuse_what_they_cannot_run():
    import vcrnet_amd
    from vcrnet_amd import consistency, native
    for name in ("consistency_registration", "correspondence_consistency", "prune_correspondences"):
        assert getattr(vcrnet_amd, name) is getattr(consistency, name) and name in vcrnet_amd.__all__
    E = native.VcrHipError
    src, tgt, corr = torch.zeros(2, 3, 50), torch.zeros(2, 3, 40), torch.zeros(2, 50, dtype=torch.int32)
    calls = ((lambda s, t, c, **k: vcrnet_amd.consistency_registration(s, t, c, 0.05, **k), (src, tgt, corr), True, True),
             (lambda s, t, **k: vcrnet_amd.register_features(s, t, 0.05, method="consistency", consistency=k), (src, tgt), True, True),
             (lambda s, t, c, **k: vcrnet_amd.correspondence_consistency(s, t, c, k.pop("tau", 0.05), **k), (src, tgt, corr),
              False, False),
             (lambda s, t, c, **k: vcrnet_amd.prune_correspondences(s, t, c, k.pop("tau", 0.05), k.pop("keep", 64), **k),
              (src, tgt, corr), True, False))
    for fn, args, has_keep, has_seeds in calls:
        with pytest.raises(E, match="no CPU fallback"):      # (the last refusal: everything else was in order)
            fn(*args)
        with pytest.raises(E, match="no CPU fallback"):
            fn(*args, tau=0.0, min_length=0.5)
        with pytest.raises(E, match=r"src must be a \[B, 3, N\]"):
            fn(src.transpose(1, 2), *args[1:])
        with pytest.raises(E, match=r"tgt must be a \[B, 3, N\]"):
            fn(args[0], torch.zeros(2, 40, 3), *args[2:])
        with pytest.raises(E, match="same number of clouds"):
            fn(args[0], tgt[:1], *args[2:])
        with pytest.raises(E, match="must be float32"):
            fn(src.double(), *args[1:])
        with pytest.raises(E, match="1 ... 131072 points"):
            fn(args[0], torch.zeros(2, 3, 0), *args[2:])
        for bad in (-0.1, float("nan"), float("inf")):
            with pytest.raises(E, match="tau must be finite and >= 0"):
                fn(*args, tau=bad)
            with pytest.raises(E, match="min_length must be finite and >= 0"):
                fn(*args, min_length=bad)
        if has_keep:
            for bad in (0, 63, 100, 4160, 64.0, True):
                with pytest.raises(E, match="keep must be"):
                    fn(*args, keep=bad)
        if has_seeds:
            with pytest.raises(E, match="no CPU fallback"):
                fn(*args, keep=4096, seeds=4096, ratio=1.0)
            for bad in (0, 129, -1):
                with pytest.raises(E, match=r"seeds must be in \[1, keep\]"):
                    fn(*args, keep=128, seeds=bad)
            for bad in (-0.1, 1.1, float("nan")):
                with pytest.raises(E, match=r"ratio must be in \[0, 1\]"):
                    fn(*args, ratio=bad)
    for fn in (vcrnet_amd.consistency_registration, ):
        with pytest.raises(E, match=r"corr must be int32 \[B, Ns\]"):
            fn(src, tgt, corr.long(), 0.05)
        with pytest.raises(E, match=r"corr must be int32 \[B, Ns\]"):
            fn(src, tgt, corr[:, :40], 0.05)
        for bad in (-1.0, float("nan"), float("inf")):
            with pytest.raises(E, match="max_dist must be finite and >= 0"):
                fn(src, tgt, corr, bad)
    for fn in (vcrnet_amd.correspondence_consistency, lambda *a: vcrnet_amd.prune_correspondences(*a, 64)):
        with pytest.raises(E, match="tau must be finite and >= 0, got None"):
            fn(src, tgt, corr, None)
    with pytest.raises(E, match=r"B \* keep must stay below 2\^30"):
        vcrnet_amd.consistency_registration(torch.zeros(1 << 18, 3, 1), torch.zeros(1 << 18, 3, 1),
                                            torch.zeros(1 << 18, 1, dtype=torch.int32), 0.05, keep=4096)
    # register_features: the method's name and its dict
    with pytest.raises(E, match='method must be "ransac" or "fgr" or "consistency", got \'sc2\''):
        vcrnet_amd.register_features(src, tgt, 0.05, method="sc2")
    with pytest.raises(E, match="consistency must be None or a dict with keys among"):
        vcrnet_amd.register_features(src, tgt, 0.05, method="consistency", consistency=dict(trials=5))
    with pytest.raises(E, match="consistency must be None or a dict"):
        vcrnet_amd.register_features(src, tgt, 0.05, method="consistency", consistency=[1])
    with pytest.raises(E, match='consistency= holds the keywords of method="consistency"; the method is "ransac"'):
        vcrnet_amd.register_features(src, tgt, 0.05, consistency={})
    with pytest.raises(E, match='fgr= holds the keywords of method="fgr"; the method is "consistency"'):
        vcrnet_amd.register_features(src, tgt, 0.05, method="consistency", fgr={})
    with pytest.raises(E, match='fgr= holds the keywords of method="fgr"; the method is "ransac"'):
        vcrnet_amd.register_features(src, tgt, 0.05, fgr={})
    with pytest.raises(E, match="no CPU fallback"):
        vcrnet_amd.register_features(src, tgt, 0.05, method="consistency", refine=0.05, centre=True, keypoints=None)
