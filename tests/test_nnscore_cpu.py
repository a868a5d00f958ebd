"""Scoring a registration on the full clouds, without a GPU: the boundary of include/vcr_hip_score.h (prototypes against
vcrnet_amd.score.SIGNATURES, the struct against gcc's layout, the exported symbols), the argument errors, the form nn_plan
picks on 256 CUs (DESIGN.md section 4.8's table), and the numpy restatement (tests/nnscore_restated.py) against the definition
written as a plain double loop."""
import ctypes
import os

import numpy as np
import pytest
import torch

import boundary
import nnscore_restated as nr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "vcr_hip_score.h")
EINVAL, EWORKSPACE, EUNSUPPORTED = -1, -2, -3


@pytest.fixture(scope="module")
def lib():
    import vcrnet_amd  # noqa: F401
    from vcrnet_amd import build, score
    build.build()
    return score.lib()


def test_signatures_match_the_header_and_the_library_exports_them(lib):
    from vcrnet_amd import score
    boundary.check_signatures(HEADER, score, lib, {"vcr_nn_score_workspace_bytes", "vcr_nn_score_f32", "vcr_nn_score_form"})


def test_the_main_boundary_is_where_it_was(lib):
    """The feature lives beside include/vcr_hip.h, not in it: the same 51 + 6 prototypes, ABI 27, and no mirror of the new struct
    in native."""
    from vcrnet_amd import native, score
    assert len(native.PUBLIC) == 51 and len(native.INTERNAL) == 6 and lib.vcr_abi_version() == native.ABI_VERSION == 27
    assert not set(score.SIGNATURES) & set(native.SIGNATURES) and not set(score.STRUCTS) & set(native.STRUCTS)
    assert "vcr_nn_score" not in open(os.path.join(ROOT, "include", "vcr_hip.h")).read()
    assert score.NnScoreArgs.__module__ == score.__name__


def test_args_match_the_c_layout(tmp_path):
    import vcrnet_amd  # noqa: F401
    from vcrnet_amd import score
    boundary.check_layout(HEADER, score, tmp_path)
    assert score.NnScoreArgs().struct_bytes == ctypes.sizeof(score.NnScoreArgs)


def _args(B=2, Ns=1000, Nt=1500, max_dist=0.1, variant=0):
    from vcrnet_amd import score
    a = score.NnScoreArgs()
    a.src, a.tgt, a.fitness, a.rmse = 0x1000, 0x2000, 0x3000, 0x4000            # (never dereferenced on the host)
    a.B, a.Ns, a.Nt, a.max_dist, a.variant = B, Ns, Nt, max_dist, variant
    return a


def test_argument_errors_return_their_codes_without_a_gpu(lib):
    from vcrnet_amd import score
    f32 = lambda a, ws=0x10000, n=1 << 40: lib.vcr_nn_score_f32(ctypes.byref(a), ws, n, None)   # noqa: E731
    form = lambda a: lib.vcr_nn_score_form(ctypes.byref(a), 256, None, None)                     # noqa: E731
    size = lambda a: lib.vcr_nn_score_workspace_bytes(ctypes.byref(a), 256)                      # noqa: E731
    assert lib.vcr_nn_score_f32(None, 0x10000, 1 << 40, None) == EINVAL
    assert lib.vcr_nn_score_form(None, 256, None, None) == EINVAL and lib.vcr_nn_score_workspace_bytes(None, 256) == 0
    assert form(_args()) == 0 and size(_args()) > 0
    for field in ("src", "tgt", "fitness", "rmse"):
        a = _args()
        setattr(a, field, None)
        assert f32(a) == EINVAL and form(a) == EINVAL and size(a) == 0, field
    for field in ("R", "t"):                                   # a pose is both or neither
        a = _args()
        setattr(a, field, 0x5000)
        assert f32(a) == EINVAL and form(a) == EINVAL, field
    a = _args()
    a.R, a.t = 0x5000, 0x6000
    assert form(a) == 0
    for kw in (dict(Ns=0), dict(Nt=0), dict(B=0), dict(Ns=-3), dict(Nt=-1), dict(max_dist=-1e-3), dict(max_dist=float("nan")),
               dict(max_dist=float("inf")), dict(max_dist=-float("inf")), dict(variant=3), dict(variant=8), dict(variant=-1),
               dict(variant=score.variant(1, 129)), dict(variant=1 << 16)):
        assert f32(_args(**kw)) == EINVAL and form(_args(**kw)) == EINVAL and size(_args(**kw)) == 0, kw
    assert form(_args(max_dist=0.0)) == 0
    for kw in (dict(Ns=131073), dict(Nt=131073), dict(Ns=131072, Nt=5, B=16384), dict(Ns=5, Nt=131072, B=16384)):
        assert f32(_args(**kw)) == EUNSUPPORTED and form(_args(**kw)) == EUNSUPPORTED and size(_args(**kw)) == 0, kw
    assert form(_args(Ns=131072, Nt=131072, B=16383)) == 0
    assert lib.vcr_nn_score_form(ctypes.byref(_args()), -1, None, None) == EINVAL
    # struct_bytes: unsized, short of rmse, longer than the library knows; the mandatory part alone is served
    for bad in (0, score.NnScoreArgs.variant.offset - 4, ctypes.sizeof(score.NnScoreArgs) + 8):
        a = _args()
        a.struct_bytes = bad
        assert f32(a) == EINVAL and form(a) == EINVAL and size(a) == 0, bad
    a = _args(variant=score.variant(4, 3))
    q, s = ctypes.c_int(0), ctypes.c_int(0)
    assert lib.vcr_nn_score_form(ctypes.byref(a), 256, ctypes.byref(q), ctypes.byref(s)) == 0 and (q.value, s.value) == (4, 3)
    a.struct_bytes = score.NnScoreArgs.variant.offset                             # ... and its variant reads as 0
    assert lib.vcr_nn_score_form(ctypes.byref(a), 256, ctypes.byref(q), ctypes.byref(s)) == 0 and (q.value, s.value) != (4, 3)
    # the workspace: missing, misaligned, short (the size is asked for the device at hand -- without one, 256 CUs)
    a = _args()
    need = lib.vcr_nn_score_workspace_bytes(ctypes.byref(a), 0)
    assert need == size(a) > 0
    assert f32(a, ws=None) == EINVAL and f32(a, ws=0x10004) == EINVAL and f32(a, ws=0x10008) == EINVAL
    assert f32(a, n=need - 1) == EWORKSPACE and f32(a, n=0) == EWORKSPACE


# (B, Ns, Nt) -> (source points per lane, target splits) on 256 CUs: DESIGN.md section 4.8's table
FORMS_256 = {(1, 1, 1): (1, 1), (1, 1024, 131072): (1, 128), (16, 1024, 1024): (1, 4), (1, 131072, 131072): (1, 32),
             (32, 4096, 4096): (1, 16), (16, 16384, 16384): (1, 16), (64, 16384, 16384): (1, 4), (256, 16384, 16384): (1, 1),
             (2, 1024, 1024): (1, 4), (1, 1024, 300): (1, 1), (1, 70001, 131072): (1, 60)}
FILL_256 = 64 * 256                                        # workgroups the plan cuts the work into on 256 CUs, where it can
MIN_SEGMENT = 256                                          # ... into segments no shorter than this


def test_the_plan_picks_the_forms_design_quotes(lib):
    from vcrnet_amd import score
    for (B, Ns, Nt), want in FORMS_256.items():
        q, s, ws = score.nn_score_form(B, Ns, Nt)
        assert (q, s) == want, (B, Ns, Nt, q, s)
        # the workspace holds what S needs: a (d2, index) pair per split and source point, and the per-256-point partials
        assert ws >= s * B * Ns * 8 + B * ((Ns + 255) // 256) * 16, (B, Ns, Nt, ws)
    for B in (1, 2, 3, 16, 100, 1000, 20000):
        for Ns in (1, 255, 256, 257, 1024, 4096, 65536, 131072):
            for Nt in (1, 255, 256, 511, 512, 513, 767, 768, 131072):
                if B * max(Ns, Nt) >= 1 << 31:
                    continue
                q, s, _ = score.nn_score_form(B, Ns, Nt)
                groups = B * ((Ns + 255) // 256)                              # the source's workgroups
                assert q == 1 and 1 <= s <= score.MAX_SPLITS                 # (measured: one point per lane wins; 2 / 4 are forced forms)
                if groups >= FILL_256 or Nt < 2 * MIN_SEGMENT:                # the source alone fills the CUs, or nothing to cut: no split
                    assert s == 1, (B, Ns, Nt)
                if s > 1:                                                    # a split only where it does not; no short segment; no more than needed
                    assert groups * (s - 1) < FILL_256 and (Nt + s - 1) // s >= MIN_SEGMENT, (B, Ns, Nt)
                elif groups < FILL_256:
                    assert Nt < 2 * MIN_SEGMENT, (B, Ns, Nt)
    assert score.nn_score_form(1, 1024, 131072)[1] > 1
    # forcing: each half alone, both, and the workspace follows the splits
    assert score.nn_score_form(16, 1024, 1024, variant=score.variant(4))[:2] == (4, 4)
    assert score.nn_score_form(1, 131072, 131072, variant=score.variant(0, 7))[:2] == (1, 7)
    assert score.nn_score_form(1, 131072, 131072, variant=score.variant(4))[:2] == (4, 128)
    assert score.nn_score_form(1, 5000, 100, variant=score.variant(2, 128))[:2] == (2, 128)
    w1, w8 = score.nn_score_form(4, 5000, 9000, variant=score.variant(1, 1))[2], score.nn_score_form(4, 5000, 9000, variant=score.variant(1, 8))[2]
    assert w8 >= 8 * 4 * 5000 * 8 > 2 * w1
    assert score.nn_score_form(1, 1024, 131072, cu_count=1)[:2] == (1, 16)      # a smaller device is filled sooner
    with pytest.raises(Exception):
        score.nn_score_form(1, 131073, 10)


def test_restatement_against_the_double_loop():
    rs = np.random.RandomState(5)
    p, q = rs.uniform(-1, 1, (3, 7)).astype(np.float32), rs.uniform(-1, 1, (3, 5)).astype(np.float32)
    q[:, 3] = q[:, 1]                                                        # a tie: the lower index wins
    p[:, 2] = q[:, 1]
    idx, d2 = nr.nearest_f32(p, q)
    li, ld = nr.double_loop(p, q)
    assert np.array_equal(idx, li) and np.array_equal(d2.view(np.int32), ld.view(np.int32))
    assert idx[2] == 1 and d2[2] == 0.0
    i64, D, second = nr.nearest_f64(p, q)
    assert np.array_equal(i64, idx) and np.allclose(D, d2, rtol=1e-6) and second[2] == 0.0 and (second >= D).all()
    # non-finite: a NaN / inf target point is never chosen, a NaN source point has no neighbour
    q2 = q.copy()
    q2[0, 0], q2[1, 4] = np.nan, np.inf
    p2 = p.copy()
    p2[2, 6] = np.nan
    idx, d2 = nr.nearest_f32(p2, q2)
    li, ld = nr.double_loop(p2, q2)
    assert np.array_equal(idx, li) and np.array_equal(d2.view(np.int32), ld.view(np.int32))
    assert idx[6] == -1 and np.isinf(d2[6]) and not set(idx[:6]) & {0, 4}
    # the summary: count, the <= at the limit, the fp64 sum's blocks, no inliers
    d = np.asarray([0.25, 0.0625, 1.0, np.inf], np.float32)
    c, s, f, r = nr.summary(np.asarray([0, 1, 2, -1]), d, 0.5)
    assert (c, s) == (2, 0.3125) and f == np.float32(0.5) and r == np.float32(np.sqrt(0.15625))
    assert nr.summary(np.asarray([-1]), np.asarray([np.inf], np.float32), 1e30)[0] == 0      # max_dist^2 overflows: still no inlier
    assert nr.summary(np.asarray([0, 1]), np.asarray([1.0, 2.0], np.float32), 0.5) == (0, 0.0, 0.0, 0.0)
    v = rs.uniform(0, 1, 700)
    parts = nr.block_partials(v)
    assert parts.shape == (3,) and np.allclose(parts, [v[:256].sum(), v[256:512].sum(), v[512:].sum()], rtol=1e-14)
    # the pose: a signed permutation and a lattice shift are exact
    R = np.asarray([[0, -1, 0], [0, 0, 1], [-1, 0, 0]], np.float32)
    t = np.asarray([0.25, -0.5, 1.0], np.float32)
    lat = (rs.randint(0, 5, (3, 9)) * 0.25).astype(np.float32)
    assert np.array_equal(nr.moved(lat, R, t), (R.astype(np.float64) @ lat + t[:, None]).astype(np.float32))
    assert nr.moved(lat) is not None and np.array_equal(nr.moved(lat), lat)


def test_python_entry_points_refuse_what_they_cannot_run():
    import vcrnet_amd
    from vcrnet_amd import native, score
    assert vcrnet_amd.score_registration is score.score_registration and "score_registration" in vcrnet_amd.__all__
    a, b = torch.zeros(2, 3, 300), torch.zeros(2, 3, 410)
    with pytest.raises(native.VcrHipError, match="no CPU fallback"):
        vcrnet_amd.score_registration(a, b, max_dist=0.1)
    with pytest.raises(native.VcrHipError, match="same number of clouds"):
        vcrnet_amd.score_registration(a, torch.zeros(3, 3, 410), max_dist=0.1)
    with pytest.raises(native.VcrHipError, match=r"\[B, 3, N\]"):
        vcrnet_amd.score_registration(a.transpose(1, 2), b, max_dist=0.1)
    with pytest.raises(native.VcrHipError, match=r"\[B, 3, N\]"):
        vcrnet_amd.score_registration(a, torch.zeros(3, 410), max_dist=0.1)
