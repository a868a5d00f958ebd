"""Fast Global Registration without a GPU: the boundary of include/vcr_hip_fgr.h (prototypes against vcrnet_amd.fgr.SIGNATURES,
the struct against gcc's layout, the exported symbols), every argument error of the call and of the Python functions, the
host-only workspace query, the resource remarks of the new kernels, and the numpy restatement (tests/fgr_restated.py): its exact
fp64 fma against a fractions.Fraction one, its sum order, its ordered cut, and the poses it recovers on the RANSAC's recipe."""
import ctypes
import os
import subprocess
from fractions import Fraction

import numpy as np
import pytest
import torch

import boundary
import fgr_restated as fg
import match_restated as mr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INCLUDE = os.path.join(ROOT, "include")
HEADER = os.path.join(INCLUDE, "vcr_hip_fgr.h")
OTHERS = ("vcr_hip.h", "vcr_hip_score.h", "vcr_hip_refine.h", "vcr_hip_plane.h", "vcr_hip_voxel.h", "vcr_hip_outlier.h",
          "vcr_hip_gicp.h", "vcr_hip_fpfh.h", "vcr_hip_match.h")
EINVAL, EWORKSPACE, EUNSUPPORTED = -1, -2, -3
ENTRY_POINTS = {"vcr_fgr_f32", "vcr_fgr_workspace_bytes"}
KERNELS = {"fgr_pairs_kernel", "fgr_tuple_kernel", "fgr_offsets_kernel", "fgr_scatter_kernel", "fgr_solve_kernel"}


@pytest.fixture(scope="module")
def lib():
    import vcrnet_amd  # noqa: F401
    from vcrnet_amd import build, fgr
    build.build()
    return fgr.lib()


def test_signatures_match_the_header_and_the_library_exports_them(lib):
    from vcrnet_amd import fgr
    boundary.check_signatures(HEADER, fgr, lib, ENTRY_POINTS)


def test_args_match_the_c_layout(tmp_path):
    import vcrnet_amd  # noqa: F401
    from vcrnet_amd import fgr
    boundary.check_layout(HEADER, fgr, tmp_path)


def test_the_other_boundaries_are_where_they_were(lib, monkeypatch):
    """The call lives beside the nine headers, not in them: none mentions it, ABI 27, the same 51 prototypes; the new header is
    taken into the digests through a list of its own; the pair list is one text for both global methods."""
    from vcrnet_amd import build, fgr, fpfh, gicp, match, native, outlier, plane, refine, score, voxel
    for h in OTHERS:
        assert "vcr_fgr" not in open(os.path.join(INCLUDE, h)).read(), h
    assert len(native.PUBLIC) == 51 and lib.vcr_abi_version() == native.ABI_VERSION == 27
    for other in (native, score, refine, plane, voxel, outlier, gicp, fpfh, match):
        assert not set(fgr.SIGNATURES) & set(other.SIGNATURES) and not set(fgr.STRUCTS) & set(other.STRUCTS)
    assert not set(fgr.SIGNATURES) & set(native.PUBLIC)
    assert build.FGR_HEADERS == [HEADER]
    assert HEADER not in (build.PUBLIC_HEADERS + build.LATER_HEADERS + build.OUTLIER_HEADERS + build.GICP_HEADERS
                          + build.FPFH_HEADERS + build.MATCH_HEADERS)
    full = build.sources_sha16()
    monkeypatch.setattr(build, "FGR_HEADERS", [])
    assert build.sources_sha16() != full
    monkeypatch.undo()
    text = open(HEADER).read()
    for name, value in (("VCR_FGR_MAX_ITERATIONS", fgr.MAX_ITERATIONS), ("VCR_FGR_MIN_ENTRIES", fgr.MIN_ENTRIES)):
        assert "#define %s %d" % (name, value) in text, name
    assert (fgr.MAX_TRIALS, fgr.MAX_N, fgr.MIN_ENTRIES, fg.MIN_ENTRIES) == (match.MAX_TRIALS, match.MAX_N, 10, 10)
    csrc = os.path.join(ROOT, "vcr-net_amd", "csrc")
    for f, kernel in (("ransac.hip", "ransac_pairs_kernel"), ("fgr.hip", "fgr_pairs_kernel")):
        text = open(os.path.join(csrc, f)).read()
        assert '#include "corr_pairs.h"' in text and "rs_mix32(uint32_t" not in text and "wg_rank(has" not in text, f
        assert "void %s(RsPairs p) { rs_pairs_body(p); }" % kernel in text, f
    shared = open(os.path.join(csrc, "corr_pairs.h")).read()
    assert shared.count("void rs_pairs_body") == 1 and "wg_rank(has" in shared and "rs_mix32(uint32_t" in shared


def _fg(**kw):
    from vcrnet_amd import fgr
    a = fgr.FgrArgs()
    a.src, a.tgt, a.corr, a.R_out, a.t_out = 0x1000, 0x2000, 0x3000, 0x4000, 0x5000   # (never dereferenced on the host)
    v = dict(B=2, Ns=100, Nt=90, tuple_scale=0.95, tuple_trials=1000, max_tuples=300, seed=7, iterations=64, decrease_mu=1,
             division_factor=1.4, mu_floor=0.025)
    v.update(kw)
    for k, x in v.items():
        setattr(a, k, x)
    return a


def test_argument_errors_return_their_codes_without_a_gpu(lib):
    from vcrnet_amd import fgr

    def codes(a):
        rc = lib.vcr_fgr_f32(ctypes.byref(a), 0x10000, 1 << 40, None)
        assert lib.vcr_fgr_workspace_bytes(ctypes.byref(a), 256) == 0
        return rc
    assert lib.vcr_fgr_f32(None, None, 0, None) == EINVAL and lib.vcr_fgr_workspace_bytes(None, 256) == 0
    for field in ("src", "tgt", "corr", "R_out", "t_out"):
        a = _fg()
        setattr(a, field, None)
        assert codes(a) == EINVAL, field
    nan, inf = float("nan"), float("inf")
    for kw in (dict(B=0), dict(Ns=0), dict(Nt=0), dict(B=-1), dict(tuple_trials=0), dict(tuple_trials=-5), dict(max_tuples=0),
               dict(max_tuples=-1), dict(tuple_scale=-0.1), dict(tuple_scale=1.5), dict(tuple_scale=nan), dict(iterations=-1),
               dict(iterations=1025), dict(division_factor=1.0), dict(division_factor=0.5), dict(division_factor=nan),
               dict(division_factor=inf), dict(mu_floor=0.0), dict(mu_floor=-1.0), dict(mu_floor=nan), dict(mu_floor=inf)):
        assert codes(_fg(**kw)) == EINVAL, kw
    for kw in (dict(tuple_trials=2 ** 20 + 1), dict(Ns=131073), dict(Nt=131073), dict(B=16384, Ns=131072),
               dict(B=512, tuple_trials=2 ** 20)):
        assert codes(_fg(**kw)) == EUNSUPPORTED, kw
    size = ctypes.sizeof(fgr.FgrArgs)
    for bad in (0, fgr.FgrArgs.pairs.offset - 8, size + 8):
        a = _fg()
        a.struct_bytes = bad
        assert codes(a) == EINVAL, bad


def test_the_workspace_query_is_host_only_and_says_what_the_call_holds(lib):
    from vcrnet_amd import fgr
    up = lambda v: (v + 255) & ~255                                               # noqa: E731
    B, Ns, T, K = 2, 100, 1000, 300
    want = up(B * Ns * 32) + 2 * up(B * 4) + up(B * T * 4) + up(B * 4 * 4) + up(B * 3 * K * 4) + up(B * 6 * 3 * K * 8)
    a = _fg()
    a.struct_bytes = fgr.FgrArgs.pairs.offset                 # the mandatory part alone
    assert lib.vcr_fgr_workspace_bytes(ctypes.byref(a), 256) == lib.vcr_fgr_workspace_bytes(ctypes.byref(_fg()), 0) == want
    assert lib.vcr_fgr_workspace_bytes(ctypes.byref(_fg()), 1) == want and lib.vcr_fgr_workspace_bytes(ctypes.byref(_fg()), -1) == 0
    # K above T holds no more than T tuples; no tuple test: the pairs alone, 48 B an entry
    big = up(B * Ns * 32) + 2 * up(B * 4) + up(B * T * 4) + up(B * 4 * 4) + up(B * 3 * T * 4) + up(B * 6 * 3 * T * 8)
    assert lib.vcr_fgr_workspace_bytes(ctypes.byref(_fg(max_tuples=2 ** 31 - 1)), 256) == big
    assert lib.vcr_fgr_workspace_bytes(ctypes.byref(_fg(tuple_scale=0.0)), 256) == up(B * Ns * 32) + 2 * up(B * 4) + up(B * Ns * 48)
    ok = _fg()
    assert lib.vcr_fgr_f32(ctypes.byref(ok), None, want, None) == EINVAL
    assert lib.vcr_fgr_f32(ctypes.byref(ok), 0x10008, want, None) == EINVAL
    assert lib.vcr_fgr_f32(ctypes.byref(ok), 0x10000, want - 1, None) == EWORKSPACE
    for kw in (dict(tuple_scale=1.0), dict(iterations=0), dict(iterations=1024), dict(tuple_trials=2 ** 20, B=1), dict(tuple_trials=1),
               dict(max_tuples=1), dict(decrease_mu=0), dict(division_factor=1.0000001), dict(mu_floor=1e-300)):
        assert lib.vcr_fgr_workspace_bytes(ctypes.byref(_fg(**kw)), 256) > 0, kw


def test_the_new_kernels_use_no_scratch():
    import vcrnet_amd  # noqa: F401
    from vcrnet_amd import build
    build.build()
    res = build.kernel_resources()
    names = list(res)
    dem = subprocess.run(["c++filt"], input="\n".join(names), capture_output=True, text=True, check=True).stdout.splitlines()
    mine = {d.replace("(anonymous namespace)::", "").replace("void ", "").split("(")[0]: res[n]
            for n, d in zip(names, dem) if res[n]["file"] == "fgr.hip"}
    assert set(mine) == KERNELS
    for d, v in mine.items():
        print(d, v)
        assert v.get("scratch", 0) == 0 and v.get("vgpr_spill", 0) == 0, (d, v)
    # the solve's LDS: four wave totals, the waves' 21 sums, the 27 sums, the update and its flag
    assert mine["fgr_solve_kernel"]["lds"] <= 8 * (4 + 4 * 21 + 27 + 12) + 8 and mine["fgr_scatter_kernel"]["lds"] == 0
    assert mine["fgr_pairs_kernel"]["lds"] == mine["fgr_tuple_kernel"]["lds"] == mine["fgr_offsets_kernel"]["lds"] == 16


# ------------------------------------------------------------------------------------------------------------- the restatement

def test_the_exact_fp64_fma_is_the_rational_one():
    rs = np.random.RandomState(5)
    n = 20000
    def draw():
        return rs.uniform(1, 2, n) * 2.0 ** rs.randint(-20, 21, n) * rs.choice([-1, 1], n)
    a, b, c = draw(), draw(), draw()
    c[:5000] = -(a[:5000] * b[:5000])                        # cancellation: the result is the product's own rounding error
    c[5000:8000] = (a[5000:8000] * b[5000:8000]) * 2.0 ** rs.randint(-3, 4, 3000)
    got = fg.fma64(a, b, c)
    want = np.asarray([float(Fraction(x) * Fraction(y) + Fraction(z)) for x, y, z in zip(a, b, c)])
    assert got.dtype == np.float64 and np.array_equal(got.view(np.int64), want.view(np.int64))
    assert (got[:5000] != 0).mean() > 0.5 and (got != a * b + c).mean() > 0.1      # (an fma, not two roundings)
    # sums that fall on a rounding boundary of the two-step form: c = (2^52 + m) 2^7, a b = -(64 - x^2 2^-98)
    m = rs.randint(0, 2 ** 31, 2000).astype(np.float64)
    x = rs.randint(1, 100, 2000).astype(np.float64)
    c = (2.0 ** 52 + m) * 128.0
    a, b = -8.0 * (1 + x * 2.0 ** -52), 8.0 * (1 - x * 2.0 ** -52)
    want = np.asarray([float(Fraction(p) * Fraction(q) + Fraction(r)) for p, q, r in zip(a, b, c)])
    assert np.array_equal(fg.fma64(a, b, c), want) and (a * b + c != want).mean() > 0.3
    assert fg.fma64(2.0, 3.0, 1.0) == 7.0 and fg.fma64(np.ones(3), np.ones(3), 0.0).shape == (3,)


def test_the_sum_order_is_lanes_then_butterfly_then_waves():
    rs = np.random.RandomState(6)
    for n in (0, 1, 10, 255, 256, 257, 1000, 3001):
        x = rs.normal(size=n) * 2.0 ** rs.randint(-30, 30, n)
        lanes = [0.0] * 256
        for i in range(n):
            lanes[i % 256] = lanes[i % 256] + float(x[i])
        waves = []
        for w in range(4):
            v = lanes[64 * w:64 * (w + 1)]
            for o in (32, 16, 8, 4, 2, 1):
                v = [v[l] + v[l ^ o] for l in range(64)]
            assert len(set(v)) == 1                          # every lane ends with the same bits
            waves.append(v[0])
        want = ((waves[0] + waves[1]) + waves[2]) + waves[3]
        got = fg.wg_sum(x)
        assert np.float64(got).view(np.int64) == np.float64(want).view(np.int64), n
    two = fg.wg_sum(np.stack([np.arange(300.0), -np.arange(300.0)], 1))
    assert two.shape == (2,) and two[0] == -two[1] == 299 * 150


def test_the_ordered_cut_is_a_loop_that_breaks_at_k():
    rs = np.random.RandomState(7)
    for n, share in ((0, 0.5), (1, 1.0), (255, 0.1), (256, 0.5), (257, 0.9), (4000, 0.02), (4000, 0.0)):
        ok = rs.uniform(size=n) < share
        for K in (1, 7, 100, 5000):
            want = []
            for t in range(n):
                if ok[t]:
                    want.append(t)
                    if len(want) == K:
                        break
            assert fg.ordered_cut(ok, K).tolist() == want, (n, share, K)
    # ... and on the recipe: the list is the kept trials' picks in (trial, pick) order, repeats kept
    c = mr.planted(40, 0.5, extra=5)
    pl = mr.pair_list(c["corr"], 40)
    at = mr.picks(3, 4000, 40)
    P, Q = c["src"][:, pl].T, c["tgt"][:, c["corr"][pl]].T
    ok = fg.passes(P, Q, at, 0.95)
    same = (at[:, 0] == at[:, 1]) | (at[:, 0] == at[:, 2]) | (at[:, 1] == at[:, 2])
    assert same.any() and not ok[same].any()                 # a repeated pick fails through its zero edge
    for K in (1, 7, 10 ** 6):
        M, ntup, lst = fg.tuples(c["src"], c["tgt"], c["corr"], 0.95, 4000, K, 3)
        kept = np.nonzero(ok)[0][:K]
        assert (M, ntup) == (40, len(kept)) and np.array_equal(lst, pl[at[kept]].reshape(-1))
    assert fg.tuples(c["src"], c["tgt"], c["corr"], 0.95, 10 ** 6, 10 ** 6, 3)[1] == int(fg.passes(P, Q, mr.picks(3, 4000, 40), 0.95).sum())
    M, ntup, lst = fg.tuples(c["src"], c["tgt"], c["corr"], 0.0, 4000, 7, 3)
    assert (M, ntup) == (40, 0) and np.array_equal(lst, pl)


@pytest.mark.parametrize("M,share,T", mr.RANSAC_SHAPES)
def test_the_restatement_recovers_the_planted_pose(M, share, T):
    """From the identity against a 65 degree rotation: within 0.1 degree and 1e-3 with the tuple test (at least 99 % of its kept
    tuples are true pairs), within 2 degrees and 3e-2 on all pairs -- a share of 0.2 to 0.5 true ones -- without it."""
    for seed in range(3):
        c = mr.planted(M, share, seed=seed, extra=5)
        for tuple_scale, rot, shift in ((0.95, 0.1, 1e-3), (0.0, 2.0, 3e-2)):
            o = fg.fgr(c["src"], c["tgt"], c["corr"], tuple_scale=tuple_scale)
            dr = fg.rotation_error_deg(o["pose64"][:9].reshape(3, 3), c["R"])
            dt = float(np.abs(o["pose64"][9:] - c["t"]).max())
            true = float(c["good"][o["list"]].mean())
            print(f"fgr restated M {M} seed {seed} tuple_scale {tuple_scale}: {o['tuples']} tuples, {o['used']} entries "
                  f"({true:.4f} true), rotation {dr:.4f} deg, |dt| {dt:.2e}, mu {o['mu']:.5f}, status {o['status']}")
            assert o["status"] == 0 and o["pairs"] == M and o["used"] == (3 * o["tuples"] if tuple_scale else M)
            assert dr <= rot and dt <= shift, (dr, dt)
            assert true >= 0.99 if tuple_scale else true == c["good"][:M].mean()
            assert np.array_equal(o["R"], o["pose64"][:9].astype(np.float32).reshape(3, 3))
            assert o["mu"] == 1.4 ** -11 or abs(o["mu"] * 1.4 ** 11 - 1) < 1e-12     # eleven divisions: 1.4^-11 < 0.025 <= 1.4^-10


def test_the_restatement_at_its_edges():
    c = mr.planted(40, 0.5, extra=5)
    few = c["corr"].copy()
    few[9:] = -1
    o = fg.fgr(c["src"], c["tgt"], few, tuple_scale=0.0)
    assert (o["pairs"], o["used"], o["status"]) == (9, 9, 1) and np.array_equal(o["pose64"], [1, 0, 0, 0, 1, 0, 0, 0, 1, 0, 0, 0])
    few[9] = c["corr"][9]
    assert fg.fgr(c["src"], c["tgt"], few, tuple_scale=0.0)["status"] == 0
    o = fg.fgr(c["src"], c["tgt"], c["corr"], iterations=0)
    assert np.array_equal(o["pose64"][:9], np.eye(3).reshape(9)) and np.array_equal(o["pose64"][9:], o["norm"][3:6] - o["norm"][:3])
    assert o["mu"] == 1.0 and not o["sums"].any()
    o = fg.fgr(c["src"], c["tgt"], c["corr"], decrease_mu=False, iterations=5)
    assert o["mu"] == 1.0 and o["sums"][15] == o["sums"][18] == o["sums"][20] > 0 and not o["sums"][[3, 9, 14, 16, 17, 19]].any()
    assert sorted(set(range(27)) - set(fg.NZ)) == [3, 9, 14, 16, 17, 19]
    bad = c["src"].copy()
    bad[1, 3] = np.nan
    o = fg.fgr(bad, c["tgt"], c["corr"])
    assert o["status"] == 2 and np.isnan(o["pose64"]).all() and np.isnan(o["R"]).all()
    # both clouds on the x axis: every system is singular, every update the identity
    line = np.zeros((3, 45), np.float32)
    line[0] = np.linspace(0, 1, 45)
    o = fg.fgr(line, line[:, :40], c["corr"], tuple_scale=0.0)
    assert o["status"] == 16 and np.array_equal(o["pose64"][:9], np.eye(3).reshape(9))
    # the solve and the rotation are the library's: A x = -g, Rz Ry Rx
    rs = np.random.RandomState(8)
    Jm = rs.normal(size=(30, 6))
    A, g = Jm.T @ Jm, rs.normal(size=6)
    x, ok = fg.solve6(A[np.triu_indices(6)], g)
    assert ok and np.abs(A @ x + g).max() <= 1e-12
    Ri, ti = fg.euler(np.asarray([0.1, -0.2, 0.3, 1, 2, 3.0]))
    assert np.abs(Ri.T @ Ri - np.eye(3)).max() <= 1e-15 and abs(np.linalg.det(Ri) - 1) <= 1e-15 and ti.tolist() == [1, 2, 3]
    small = fg.euler(np.asarray([1e-6, 0, 0, 0, 0, 0.0]))[0]
    assert small[2, 1] > 0 and small[1, 2] < 0                # a positive x0 turns y towards z


# ------------------------------------------------------------------------------------------------------------ the Python layer

def test_python_entry_points_refuse_what_they_cannot_run():
    import vcrnet_amd
    from vcrnet_amd import fgr, native
    assert vcrnet_amd.fast_global_registration is fgr.fast_global_registration and "fast_global_registration" in vcrnet_amd.__all__
    E = native.VcrHipError
    src, tgt, corr = torch.zeros(2, 3, 50), torch.zeros(2, 3, 40), torch.zeros(2, 50, dtype=torch.int32)
    calls = ((lambda *a, **k: vcrnet_amd.fast_global_registration(*a, **k), (src, tgt, corr)),
             (lambda s, t, **k: vcrnet_amd.register_features(s, t, 0.05, method="fgr", fgr=k), (src, tgt)))
    for fn, args in calls:
        with pytest.raises(E, match="no CPU fallback"):      # (the last refusal: everything else was in order)
            fn(*args)
        with pytest.raises(E, match="no CPU fallback"):
            fn(*args, tuple_scale=0.0, max_tuples=1, iterations=0, division_factor=2.0, mu_floor=1e-3, decrease_mu=False,
               tuple_trials=2 ** 20, seed=2 ** 32 - 1)
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
        for bad in (-0.1, 1.1, float("nan")):
            with pytest.raises(E, match="tuple_scale must be 0"):
                fn(*args, tuple_scale=bad)
        for bad in (0, -1, 2 ** 20 + 1):
            with pytest.raises(E, match=r"tuple_trials must be in \[1, 1048576\]"):
                fn(*args, tuple_trials=bad)
        for bad in (0, -3, 2 ** 31):
            with pytest.raises(E, match="max_tuples must be in"):
                fn(*args, max_tuples=bad)
        for bad in (-1, 1025):
            with pytest.raises(E, match=r"iterations must be in \[0, 1024\]"):
                fn(*args, iterations=bad)
        for bad in (1.0, 0.5, float("nan"), float("inf")):
            with pytest.raises(E, match="division_factor must be finite and > 1"):
                fn(*args, division_factor=bad)
        for bad in (0.0, -1.0, float("nan"), float("inf")):
            with pytest.raises(E, match="mu_floor must be finite and > 0"):
                fn(*args, mu_floor=bad)
        for bad in (-1, 2 ** 32):
            with pytest.raises(E, match="seed must be in"):
                fn(*args, seed=bad)
    with pytest.raises(E, match=r"B \* tuple_trials must stay below 2\^29"):
        vcrnet_amd.fast_global_registration(torch.zeros(512, 3, 5), torch.zeros(512, 3, 5), torch.zeros(512, 5, dtype=torch.int32),
                                            tuple_trials=2 ** 20)
    for bad in (corr.long(), corr[:, :49], corr[:1], torch.zeros(2, 50), None, "corr"):
        with pytest.raises(E, match=r"corr must be int32 \[B, Ns\]"):
            vcrnet_amd.fast_global_registration(src, tgt, bad)
    # register_features: the method, its dict, and what the two methods share
    with pytest.raises(E, match='method must be "ransac" or "fgr"'):
        vcrnet_amd.register_features(src, tgt, 0.05, method="icp")
    with pytest.raises(E, match="fgr must be None or a dict with keys among"):
        vcrnet_amd.register_features(src, tgt, 0.05, method="fgr", fgr=dict(trials=5))
    with pytest.raises(E, match="fgr must be None or a dict"):
        vcrnet_amd.register_features(src, tgt, 0.05, method="fgr", fgr=[1])
    with pytest.raises(E, match='fgr= holds the keywords of method="fgr"'):
        vcrnet_amd.register_features(src, tgt, 0.05, fgr=dict(seed=1))
    for md in (-0.1, float("nan"), float("inf")):
        with pytest.raises(E, match="max_dist must be finite"):
            vcrnet_amd.register_features(src, tgt, md, method="fgr")
    with pytest.raises(E, match="refine must be None or a finite"):
        vcrnet_amd.register_features(src, tgt, 0.05, method="fgr", refine=-1.0)
    with pytest.raises(E, match="no CPU fallback"):
        vcrnet_amd.register_features(src, tgt, 0.05, method="ransac")
    assert set(fgr.DEFAULTS) == {"tuple_scale", "max_tuples", "iterations", "division_factor", "mu_floor", "decrease_mu",
                                 "tuple_trials", "seed"}
