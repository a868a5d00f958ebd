"""Feature matching and the RANSAC over its correspondences, without a GPU: the boundary of include/vcr_hip_match.h (prototypes
against vcrnet_amd.match.SIGNATURES, the structs against gcc's layout, the exported symbols), every argument error of both
calls and of the three Python functions, the host-only queries, the resource remarks of the new kernels, and the numpy
restatement (tests/match_restated.py): its exact fmaf against a fractions.Fraction one, the quality of the draws, and the
RANSAC recipe's planted counts."""
import ctypes
import os
import subprocess
from fractions import Fraction

import numpy as np
import pytest
import torch

import boundary
import match_restated as mr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INCLUDE = os.path.join(ROOT, "include")
HEADER = os.path.join(INCLUDE, "vcr_hip_match.h")
OTHERS = ("vcr_hip.h", "vcr_hip_score.h", "vcr_hip_refine.h", "vcr_hip_plane.h", "vcr_hip_voxel.h", "vcr_hip_outlier.h",
          "vcr_hip_gicp.h", "vcr_hip_fpfh.h")
EINVAL, EWORKSPACE, EUNSUPPORTED = -1, -2, -3
ENTRY_POINTS = {"vcr_feat_nn_f32", "vcr_feat_nn_form", "vcr_feat_nn_workspace_bytes", "vcr_ransac_f32", "vcr_ransac_workspace_bytes"}
# waves per SIMD, as DESIGN section 4.15 records them from the build's resource remarks
OCCUPANCY = {"featnn_rows_kernel": 8, "featnn_scan_kernel<1>": 8, "featnn_scan_kernel<2>": 6, "featnn_scan_kernel<4>": 3,
             "featnn_merge_kernel": 8, "featnn_mutual_kernel": 8,
             "ransac_pairs_kernel": 8, "ransac_trial_kernel": 4, "ransac_count_kernel": 8, "ransac_best_kernel": 8}


@pytest.fixture(scope="module")
def lib():
    import vcrnet_amd  # noqa: F401
    from vcrnet_amd import build, match
    build.build()
    return match.lib()


def test_signatures_match_the_header_and_the_library_exports_them(lib):
    from vcrnet_amd import match
    boundary.check_signatures(HEADER, match, lib, ENTRY_POINTS)


def test_args_match_the_c_layout(tmp_path):
    import vcrnet_amd  # noqa: F401
    from vcrnet_amd import match
    boundary.check_layout(HEADER, match, tmp_path)


def test_the_other_boundaries_are_where_they_were(lib, monkeypatch):
    """The two calls live beside the eight headers, not in them: none mentions them, ABI 27, the same 51 prototypes; the new
    header is taken into the digests through a list of its own."""
    from vcrnet_amd import build, fpfh, gicp, match, native, outlier, plane, refine, score, voxel
    for h in OTHERS:
        text = open(os.path.join(INCLUDE, h)).read()
        assert "vcr_feat_nn" not in text and "vcr_ransac" not in text, h
    assert len(native.PUBLIC) == 51 and lib.vcr_abi_version() == native.ABI_VERSION == 27
    for other in (native, score, refine, plane, voxel, outlier, gicp, fpfh):
        assert not set(match.SIGNATURES) & set(other.SIGNATURES) and not set(match.STRUCTS) & set(other.STRUCTS)
    assert not set(match.SIGNATURES) & set(native.PUBLIC)
    assert build.MATCH_HEADERS == [HEADER]
    assert HEADER not in (build.PUBLIC_HEADERS + build.LATER_HEADERS + build.OUTLIER_HEADERS + build.GICP_HEADERS
                          + build.FPFH_HEADERS)
    full = build.sources_sha16()
    monkeypatch.setattr(build, "MATCH_HEADERS", [])
    assert build.sources_sha16() != full
    monkeypatch.undo()
    text = open(HEADER).read()
    for name, value in (("VCR_FEAT_NN_C", match.FEAT_C), ("VCR_RANSAC_MAX_TRIALS", match.MAX_TRIALS)):
        assert "#define %s %d " % (name, value) in text, name
    assert (match.FEAT_C, match.MAX_TRIALS, match.MAX_N) == (33, 2 ** 20, 131072)


def _nn(B=2, C=33, Ns=100, Nt=90, mutual=0, variant=0):
    from vcrnet_amd import match
    a = match.FeatNnArgs()
    a.a, a.b, a.nn_idx, a.nn_d2, a.rev_idx = 0x1000, 0x2000, 0x3000, 0x4000, 0x5000   # (never dereferenced: every call is refused)
    a.B, a.C, a.Ns, a.Nt, a.mutual, a.variant = B, C, Ns, Nt, mutual, variant
    return a


def _rs(B=2, Ns=100, Nt=90, max_dist=0.05, similarity=0.9, trials=1000, seed=7):
    from vcrnet_amd import match
    a = match.RansacArgs()
    a.src, a.tgt, a.corr, a.R_out, a.t_out = 0x1000, 0x2000, 0x3000, 0x4000, 0x5000
    a.B, a.Ns, a.Nt, a.max_dist, a.similarity, a.trials, a.seed = B, Ns, Nt, max_dist, similarity, trials, seed
    return a


def test_feat_nn_argument_errors_return_their_codes_without_a_gpu(lib):
    from vcrnet_amd import match
    q, s = ctypes.c_int(-7), ctypes.c_int(-7)

    def codes(a):
        """The three entry points agree: the call's code (its argument checks come before the workspace's), the form's, 0 bytes."""
        rc = lib.vcr_feat_nn_f32(ctypes.byref(a), 0x10000, 1 << 40, None)
        assert lib.vcr_feat_nn_form(ctypes.byref(a), 256, ctypes.byref(q), ctypes.byref(s)) == rc
        assert lib.vcr_feat_nn_workspace_bytes(ctypes.byref(a), 256) == 0
        return rc
    assert lib.vcr_feat_nn_f32(None, None, 0, None) == EINVAL and lib.vcr_feat_nn_workspace_bytes(None, 256) == 0
    for field in ("a", "b", "nn_idx"):
        a = _nn()
        setattr(a, field, None)
        assert codes(a) == EINVAL, field
    for kw in (dict(B=0), dict(Ns=0), dict(Nt=0), dict(B=-1), dict(Ns=-3), dict(variant=3), dict(variant=8), dict(variant=129 << 8),
               dict(variant=1 << 4), dict(variant=1 << 16)):
        assert codes(_nn(**kw)) == EINVAL, kw
    for kw in (dict(C=32), dict(C=34), dict(C=3), dict(C=64), dict(C=0), dict(Ns=131073), dict(Nt=131073), dict(B=16384, Ns=131072),
               dict(B=16384, Nt=131072)):
        assert codes(_nn(**kw)) == EUNSUPPORTED, kw
    size = ctypes.sizeof(match.FeatNnArgs)
    for bad in (0, match.FeatNnArgs.variant.offset - 4, size + 8):
        a = _nn()
        a.struct_bytes = bad
        assert codes(a) == EINVAL, bad
    a = _nn()
    a.struct_bytes = match.FeatNnArgs.variant.offset           # an older caller without the tail: variant reads as 0
    assert lib.vcr_feat_nn_workspace_bytes(ctypes.byref(a), 256) == lib.vcr_feat_nn_workspace_bytes(ctypes.byref(_nn()), 256) > 0
    # accepted arguments: a missing, misaligned or short workspace is the call's to refuse (no device is touched before)
    ok = _nn()
    need = lib.vcr_feat_nn_workspace_bytes(ctypes.byref(ok), 256)
    assert need > 0 and lib.vcr_feat_nn_f32(ctypes.byref(ok), None, need, None) == EINVAL
    assert lib.vcr_feat_nn_f32(ctypes.byref(ok), 0x10008, need, None) == EINVAL
    assert lib.vcr_feat_nn_form(ctypes.byref(ok), -1, None, None) == EINVAL and lib.vcr_feat_nn_workspace_bytes(ctypes.byref(ok), -1) == 0


def test_the_form_query_works_without_a_device():
    """The plan: the most rows per lane (4, 2, 1) that leave enough workgroups within reach of the splits; forced forms come back
    as forced; the
    workspace holds the searched side's rows, both sides' with a reverse search, and the candidates of every split."""
    from vcrnet_amd import match
    up = lambda v: (v + 255) & ~255                                               # noqa: E731
    for B, Ns, Nt in ((1, 1, 1), (2, 1000, 777), (16, 16384, 16384), (1, 131072, 131072), (64, 131072, 1000)):
        q, s, need = match.feat_nn_form(B, Ns, Nt, 256)
        assert q in (1, 2, 4) and 1 <= s <= 128 and (Nt + s - 1) // s >= min(Nt, 64), (B, Ns, Nt, q, s)
        assert need == up(B * Nt * 144) + 2 * up(4 * s * B * Ns)
        assert match.feat_nn_form(B, Ns, Nt, 256) == (q, s, need)
    assert match.feat_nn_form(64, 131072, 1000, 256)[:2] == (4, 1)               # the source alone fills the device
    assert match.feat_nn_form(16, 1024, 1024, 256)[:2] == (1, 16) and match.feat_nn_form(16, 16384, 16384, 256)[:2] == (4, 16)
    assert match.feat_nn_form(1, 131072, 131072, 256)[:2] == (4, 32)              # (the three shapes of profiles/match_bench.txt)
    assert match.feat_nn_form(1, 300, 4000, 256)[0] == 1 and match.feat_nn_form(1, 300, 4000, 256)[1] > 1
    for fq in match.QUERIES_PER_LANE:
        for fs in (1, 2, 7, match.MAX_SPLITS):
            q, s, need = match.feat_nn_form(3, 257, 300, 256, match.variant(fq, fs))
            assert (q, s) == (fq, fs) and need == up(3 * 300 * 144) + 2 * up(4 * fs * 3 * 257)
    # a reverse search: the source's rows too, candidates for the larger of the two directions, the reverse result
    q, s, need = match.feat_nn_form(3, 257, 300, 256, match.variant(1, 2), mutual=True)
    assert need == up(3 * 300 * 144) + up(3 * 257 * 144) + 2 * up(4 * 2 * 3 * 300) + up(4 * 3 * 300)


def test_ransac_argument_errors_return_their_codes_without_a_gpu(lib):
    from vcrnet_amd import match

    def codes(a):
        rc = lib.vcr_ransac_f32(ctypes.byref(a), 0x10000, 1 << 40, None)
        assert lib.vcr_ransac_workspace_bytes(ctypes.byref(a), 256) == 0
        return rc
    assert lib.vcr_ransac_f32(None, None, 0, None) == EINVAL and lib.vcr_ransac_workspace_bytes(None, 256) == 0
    for field in ("src", "tgt", "corr", "R_out", "t_out"):
        a = _rs()
        setattr(a, field, None)
        assert codes(a) == EINVAL, field
    nan, inf = float("nan"), float("inf")
    for kw in (dict(B=0), dict(Ns=0), dict(Nt=0), dict(B=-1), dict(trials=0), dict(trials=-5), dict(max_dist=-0.1), dict(max_dist=nan),
               dict(max_dist=inf), dict(similarity=-0.1), dict(similarity=1.5), dict(similarity=nan)):
        assert codes(_rs(**kw)) == EINVAL, kw
    for kw in (dict(trials=2 ** 20 + 1), dict(Ns=131073), dict(Nt=131073), dict(B=16384, Ns=131072), dict(B=512, trials=2 ** 20)):
        assert codes(_rs(**kw)) == EUNSUPPORTED, kw
    size = ctypes.sizeof(match.RansacArgs)
    for bad in (0, match.RansacArgs.best_trial.offset - 8, size + 8):
        a = _rs()
        a.struct_bytes = bad
        assert codes(a) == EINVAL, bad
    a = _rs()
    a.struct_bytes = match.RansacArgs.best_trial.offset       # the mandatory part alone
    up = lambda v: (v + 255) & ~255                                               # noqa: E731
    BT = 2 * 1000
    want = up(2 * 100 * 32) + 2 * up(2 * 4) + up(BT * 4) + up(BT * 4) + up(BT * 48) + up(BT * 4)
    assert lib.vcr_ransac_workspace_bytes(ctypes.byref(a), 256) == lib.vcr_ransac_workspace_bytes(ctypes.byref(_rs()), 0) == want
    full = _rs()
    full.trial_status, full.trial_pose, full.trial_inliers = 0x6000, 0x7000, 0x8000      # the caller's arrays replace the workspace's
    assert lib.vcr_ransac_workspace_bytes(ctypes.byref(full), 256) == up(2 * 100 * 32) + 2 * up(2 * 4) + up(BT * 4)
    ok = _rs()
    assert lib.vcr_ransac_f32(ctypes.byref(ok), None, want, None) == EINVAL
    assert lib.vcr_ransac_f32(ctypes.byref(ok), 0x10008, want, None) == EINVAL
    assert lib.vcr_ransac_f32(ctypes.byref(ok), 0x10000, want - 1, None) == EWORKSPACE
    full.trial_pose = 0x7008                                  # a pose is read and written 16 B at a time
    assert lib.vcr_ransac_f32(ctypes.byref(full), 0x10000, want, None) == EINVAL
    for kw in (dict(similarity=0.0), dict(similarity=1.0), dict(max_dist=0.0), dict(trials=2 ** 20, B=1), dict(trials=1)):
        assert lib.vcr_ransac_workspace_bytes(ctypes.byref(_rs(**kw)), 256) > 0, kw


def test_the_new_kernels_use_no_scratch_and_keep_their_occupancy():
    import vcrnet_amd  # noqa: F401
    from vcrnet_amd import build
    build.build()
    res = build.kernel_resources()
    names = list(res)
    dem = subprocess.run(["c++filt"], input="\n".join(names), capture_output=True, text=True, check=True).stdout.splitlines()
    mine = {d.replace("(anonymous namespace)::", "").replace("void ", "").split("(")[0]: res[n]
            for n, d in zip(names, dem) if res[n]["file"] in ("featnn.hip", "ransac.hip")}
    assert set(mine) == set(OCCUPANCY)
    for d, v in mine.items():
        assert v.get("scratch", 0) == 0 and v.get("vgpr_spill", 0) == 0 and v.get("sgpr_spill", 0) == 0, (d, v)
        assert v["occupancy"] == OCCUPANCY[d], (d, v)
    # the scans take the candidate row through scalar loads, not LDS; the RANSAC's LDS is the two reductions' wave totals
    assert all(mine[d]["lds"] == 0 for d in mine if d.startswith("featnn")) and mine["ransac_count_kernel"]["lds"] == 0
    assert mine["ransac_pairs_kernel"]["lds"] == 16 and mine["ransac_best_kernel"]["lds"] == 32
    assert mine["featnn_scan_kernel<1>"]["vgprs"] <= 64 and mine["featnn_scan_kernel<2>"]["vgprs"] <= 80


# ------------------------------------------------------------------------------------------------------------- the restatement

def fma_fraction(a, b, c):
    """fmaf by exact rational arithmetic: one rounding to fp32, to nearest, ties to even (results in the normal range or 0)."""
    x = Fraction(float(a)) * Fraction(float(b)) + Fraction(float(c))
    if x == 0:
        return np.float32(0.0)
    e = abs(x).numerator.bit_length() - abs(x).denominator.bit_length()
    if abs(x) < Fraction(2) ** e:
        e -= 1
    assert Fraction(2) ** e <= abs(x) < Fraction(2) ** (e + 1) and -126 <= e < 127
    ulp = Fraction(2) ** (e - 23)
    return np.float32(float(round(x / ulp) * ulp))            # round(): half to even; the product is exact in float64


def test_the_exact_fmaf_is_the_rational_one_on_random_triples():
    rs = np.random.RandomState(3)
    n = 12000
    def draw():
        return (rs.uniform(1, 2, n) * 2.0 ** rs.randint(-20, 21, n) * rs.choice([-1, 1], n)).astype(np.float32)
    a, b, c = draw(), draw(), draw()
    c[:3000] = -(a[:3000] * b[:3000])                        # cancellation: the result is the product's own rounding error
    c[3000:5000] = (a[3000:5000] * b[3000:5000]) * np.float32(2.0) ** rs.randint(-3, 4, 2000)
    got = mr.fma32(a, b, c)
    want = np.asarray([fma_fraction(*v) for v in zip(a, b, c)], np.float32)
    assert got.dtype == np.float32 and np.array_equal(got.view(np.int32), want.view(np.int32))
    assert (got[:3000] != 0).mean() > 0.5                    # (the cancellation cases are not trivial)
    # the chain's own values: features in [0, 200], a running sum
    d = (rs.uniform(0, 200, 4000).astype(np.float32) - rs.uniform(0, 200, 4000).astype(np.float32))
    acc = rs.uniform(0, 2e5, 4000).astype(np.float32)
    got = mr.fma32(d, d, acc)
    assert np.array_equal(got, np.asarray([fma_fraction(x, x, y) for x, y in zip(d, acc)], np.float32))


def test_the_exact_fmaf_on_sums_that_fall_on_a_rounding_boundary():
    """c = +-(2^23 + m) 2^7 has an ulp of 128; a b = -+(64 - x^2 2^-40) puts the exact sum just off the midpoint of two fp32
    values, by less than half a float64 ulp (2^-23): the float64 sum IS the midpoint, and rounding it again goes to the even
    neighbour -- the wrong one for every other m."""
    rs = np.random.RandomState(4)
    n = 2000
    m = rs.randint(0, 2 ** 23, n).astype(np.int64)
    x = rs.randint(1, 100, n).astype(np.float64)
    sign = rs.choice([-1.0, 1.0], n)
    c = (sign * ((2 ** 23 + m) * 128.0)).astype(np.float32)
    a = (-sign * 8.0 * (1 + x * 2.0 ** -23)).astype(np.float32)
    b = (8.0 * (1 - x * 2.0 ** -23)).astype(np.float32)
    wide = a.astype(np.float64) * b.astype(np.float64) + c.astype(np.float64)
    assert ((wide.view(np.uint64) & np.uint64(0x1FFFFFFF)) == np.uint64(0x10000000)).all()
    got = mr.fma32(a, b, c)
    want = np.asarray([fma_fraction(*v) for v in zip(a, b, c)], np.float32)
    assert np.array_equal(got, want)
    twice = wide.astype(np.float32)
    assert 0.3 < (twice != want).mean() < 0.7                # rounding twice is wrong on about half of them
    assert np.array_equal(got, c)                            # (the sum lies on c's side of the midpoint)


def test_the_search_is_the_chain_with_the_first_minimum():
    a, b = mr.features(1, 5, 3)
    d = mr.d2_chain(a[0], b[0])
    for i in range(5):
        for j in range(3):
            acc = None
            for ch in range(33):
                dd = np.float32(a[0, ch, i]) - np.float32(b[0, ch, j])
                acc = dd * dd if acc is None else fma_fraction(dd, dd, acc)
            assert d[i, j] == acc
    idx, best = mr.nearest(d)
    assert np.array_equal(idx, d.argmin(1)) and np.array_equal(best, d.min(1))
    rev, _ = mr.nearest_rev(d)
    assert np.array_equal(rev, mr.nearest(mr.d2_chain(b[0], a[0]))[0])
    assert np.array_equal(mr.mutual(idx, rev), [j if rev[j] == i else -1 for i, j in enumerate(idx)])
    tie = np.asarray([[3.0, 1.0, 1.0], [np.nan, np.inf, np.nan], [np.inf, 2.0, np.nan]], np.float32)
    idx, best = mr.nearest(tie)
    assert idx.tolist() == [1, -1, 1] and best[0] == 1 and np.isposinf(best[1]) and best[2] == 2
    assert mr.CHOICE_E == 72 * 2.0 ** -24 and 1 - ((1 - mr.U) / (1 + mr.U)) ** 35 < mr.CHOICE_E


@pytest.mark.parametrize("seed", [0, 1, 12345])
def test_the_draws_are_uniform_and_repeat_as_often_as_they_should(seed):
    T = 65536
    for M in (1000, 5000):
        at = mr.picks(seed, T, M)
        assert at.min() >= 0 and at.max() < M
        counts = np.bincount(at.reshape(-1), minlength=M)
        assert (counts > 0).all()
        expect = 3 * T / M
        chi2 = ((counts - expect) ** 2 / expect).sum() / (M - 1)
        same = ((at[:, 0] == at[:, 1]) | (at[:, 0] == at[:, 2]) | (at[:, 1] == at[:, 2])).mean()
        print(f"draws seed {seed} M {M}: chi2/dof {chi2:.3f}, repeated picks {same:.5f}")
        assert 0.8 <= chi2 <= 1.25, chi2
        assert abs(same - (1 - (1 - 1 / M) * (1 - 2 / M))) <= 0.001
    at = mr.picks(seed, T, 7)
    same = ((at[:, 0] == at[:, 1]) | (at[:, 0] == at[:, 2]) | (at[:, 1] == at[:, 2])).mean()
    assert abs(same - 0.3878) <= 0.01, same
    assert not np.array_equal(mr.picks(seed, 64, 1000), mr.picks(seed + 1, 64, 1000))
    assert mr.mix32(np.uint32(0)) == 0


@pytest.mark.parametrize("M,share,T", mr.RANSAC_SHAPES)
def test_the_restated_ransac_finds_the_planted_pairs(M, share, T):
    c = mr.planted(M, share)
    r = mr.ransac(c["src"], c["tgt"], c["corr"], mr.MAX_DIST, mr.SIMILARITY, T, mr.SEED)
    n_good = int(c["good"].sum())
    assert n_good == round(share * M) and r["pairs"] == M
    assert r["inliers"] == n_good and r["best_trial"] >= 0 and r["status"][r["best_trial"]] == 0
    assert c["good"][r["picks"][r["best_trial"]]].all()
    assert (r["count"][r["status"] != 0] == -1).all() and (r["count"][r["status"] == 0] >= 3).all()
    assert np.abs(r["R"] - c["R"]).max() <= 1e-3 and np.abs(r["t"] - c["t"]).max() <= 1e-3
    # fewer than three pairs: no trial is valid
    few = c["corr"].copy()
    few[2:] = -1
    r = mr.ransac(c["src"], c["tgt"], few, mr.MAX_DIST, mr.SIMILARITY, 65, mr.SEED)
    assert r["pairs"] == 2 and (r["status"] == 1).all() and r["best_trial"] == -1 and r["inliers"] == 0
    assert np.array_equal(r["R"], np.eye(3, dtype=np.float32)) and not r["t"].any()
    none = mr.ransac(c["src"], c["tgt"], np.full(M, -1), mr.MAX_DIST, mr.SIMILARITY, 5, mr.SEED)
    assert none["pairs"] == 0 and (none["status"] == 1).all() and (none["picks"] == -1).all()


def test_the_surface_recipe_is_a_permuted_copy():
    c = mr.surface(600)
    back = c["R"] @ c["src"].astype(np.float64) + c["t"][:, None]
    assert np.abs(back - c["tgt"][:, c["twin"]]).max() <= 4e-7 and sorted(c["twin"]) == list(range(600))


@pytest.mark.parametrize("N,k", [(600, 20), (1500, 30)])
def test_the_surface_recipes_shares_are_the_tables(N, k):
    for oriented in (False, True):
        one, both = mr.surface_shares(N, k, oriented)
        print(f"surface N {N} k {k} oriented {oriented}: one-way {one:.4f}, mutual {both:.4f}")
        assert abs(one - mr.SURFACE_SHARES[(N, k, oriented, False)]) <= 0.001
        assert abs(both - mr.SURFACE_SHARES[(N, k, oriented, True)]) <= 0.001


# ------------------------------------------------------------------------------------------------------------ the Python layer

def test_python_entry_points_refuse_what_they_cannot_run():
    import vcrnet_amd
    from vcrnet_amd import match, native
    for name in ("match_features", "ransac_correspondences", "register_features"):
        assert getattr(vcrnet_amd, name) is getattr(match, name) and name in vcrnet_amd.__all__
    E = native.VcrHipError
    fa, fb = torch.zeros(2, 33, 50), torch.zeros(2, 33, 40)
    with pytest.raises(E, match="no CPU fallback"):
        vcrnet_amd.match_features(fa, fb)
    with pytest.raises(E, match="no CPU fallback"):
        match.feat_nn(fa, fb, mutual=True)
    for bad in (torch.zeros(2, 32, 50), torch.zeros(2, 34, 50), torch.zeros(2, 50, 33), torch.zeros(2, 3, 50)):
        with pytest.raises(E, match="must have 33 channels"):
            vcrnet_amd.match_features(bad, fb)
        with pytest.raises(E, match="must have 33 channels"):
            vcrnet_amd.match_features(fa, bad)
    for bad in (torch.zeros(33, 50), torch.zeros(2, 33, 50, dtype=torch.float64), torch.zeros(2, 33, 50, dtype=torch.int32), "feat", None):
        with pytest.raises(E, match=r"float32 \[B, 33, N\]"):
            vcrnet_amd.match_features(bad, fb)
    with pytest.raises(E, match="1 ... 131072 points"):
        vcrnet_amd.match_features(torch.zeros(2, 33, 0), fb)
    with pytest.raises(E, match="same number of clouds"):
        vcrnet_amd.match_features(fa, torch.zeros(3, 33, 40))

    src, tgt, corr = torch.zeros(2, 3, 50), torch.zeros(2, 3, 40), torch.zeros(2, 50, dtype=torch.int32)
    for fn in (vcrnet_amd.ransac_correspondences, match.ransac):
        with pytest.raises(E, match="no CPU fallback"):                          # (the last refusal: everything else was in order)
            fn(src, tgt, corr, 0.05)
    with pytest.raises(E, match="no CPU fallback"):
        vcrnet_amd.register_features(src, tgt, 0.05)
    with pytest.raises(E, match="no CPU fallback"):
        vcrnet_amd.register_features(src, tgt, 0.05, refine=0.05, mutual=False, similarity=0.0, trials=2 ** 20, seed=2 ** 32 - 1)
    for fn, args in ((vcrnet_amd.ransac_correspondences, (src, tgt, corr)), (vcrnet_amd.register_features, (src, tgt))):
        with pytest.raises(E, match=r"src must be a \[B, 3, N\]"):
            fn(src.transpose(1, 2), *args[1:], 0.05)
        with pytest.raises(E, match=r"tgt must be a \[B, 3, N\]"):
            fn(args[0], torch.zeros(2, 40, 3), *args[2:], 0.05)
        with pytest.raises(E, match="same number of clouds"):
            fn(args[0], tgt[:1], *args[2:], 0.05)
        with pytest.raises(E, match="must be float32"):
            fn(src.double(), *args[1:], 0.05)
        with pytest.raises(E, match="1 ... 131072 points"):
            fn(args[0], torch.zeros(2, 3, 0), *args[2:], 0.05)
        for trials in (0, -1, 2 ** 20 + 1):
            with pytest.raises(E, match=r"trials must be in \[1, 1048576\]"):
                fn(*args, 0.05, trials=trials)
        for md in (-0.1, float("nan"), float("inf")):
            with pytest.raises(E, match="max_dist must be finite"):
                fn(*args, md)
        for sim in (-0.1, 1.1, float("nan")):
            with pytest.raises(E, match="similarity must be 0"):
                fn(*args, 0.05, similarity=sim)
        for seed in (-1, 2 ** 32):
            with pytest.raises(E, match="seed must be in"):
                fn(*args, 0.05, seed=seed)
    for bad in (corr.long(), corr[:, :49], corr[:1], torch.zeros(2, 50), None, "corr"):
        with pytest.raises(E, match=r"corr must be int32 \[B, Ns\]"):
            vcrnet_amd.ransac_correspondences(src, tgt, bad, 0.05)
    for bad in (-1.0, float("nan"), float("inf")):
        with pytest.raises(E, match="refine must be None or a finite"):
            vcrnet_amd.register_features(src, tgt, 0.05, refine=bad)
