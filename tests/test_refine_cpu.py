"""Refining a registration on the full clouds, without a GPU: the boundary of include/vcr_hip_refine.h (prototypes against
vcrnet_amd.refine.SIGNATURES, the struct against gcc's layout, the exported symbols), every argument error, the host-only form
and workspace queries, and the numpy restatement (tests/refine_restated.py) on the recipe the GPU tests use: it recovers the
planted pose."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import boundary
import refine_restated as rr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "vcr_hip_refine.h")
EINVAL, EWORKSPACE, EUNSUPPORTED = -1, -2, -3


@pytest.fixture(scope="module")
def lib():
    import vcrnet_amd  # noqa: F401
    from vcrnet_amd import build, refine
    build.build()
    return refine.lib()


def test_signatures_match_the_header_and_the_library_exports_them(lib):
    from vcrnet_amd import refine
    boundary.check_signatures(HEADER, refine, lib, {"vcr_refine_workspace_bytes", "vcr_refine_f32", "vcr_refine_form"})


def test_the_other_boundaries_are_where_they_were(lib):
    """The feature lives beside include/vcr_hip.h and include/vcr_hip_score.h, not in them, and every object's digest takes the
    new header in."""
    from vcrnet_amd import build, native, refine, score
    assert len(native.PUBLIC) == 51 and len(native.INTERNAL) == 6 and lib.vcr_abi_version() == native.ABI_VERSION == 27
    assert len(score.SIGNATURES) == 3 and len(boundary.prototypes(os.path.join(ROOT, "include", "vcr_hip_score.h"))) == 3
    for other in (native, score):
        assert not set(refine.SIGNATURES) & set(other.SIGNATURES) and not set(refine.STRUCTS) & set(other.STRUCTS)
    for header in ("vcr_hip.h", "vcr_hip_score.h"):
        assert "vcr_refine" not in open(os.path.join(ROOT, "include", header)).read()
    assert refine.RefineArgs.__module__ == refine.__name__
    assert [os.path.basename(h) for h in build.PUBLIC_HEADERS] == ["vcr_hip.h", "vcr_hip_score.h", "vcr_hip_refine.h",
                                                                      "vcr_hip_plane.h"]
    assert int(re.search(r"#define\s+VCR_REFINE_MAX_ITERATIONS\s+(\d+)", open(HEADER).read()).group(1)) == refine.MAX_ITERATIONS


def test_args_match_the_c_layout(tmp_path):
    import vcrnet_amd  # noqa: F401
    from vcrnet_amd import refine
    boundary.check_layout(HEADER, refine, tmp_path)
    assert refine.RefineArgs().struct_bytes == ctypes.sizeof(refine.RefineArgs)


def _args(B=2, Ns=1000, Nt=1500, max_dist=0.1, max_iterations=30, rel_fitness=1e-6, rel_rmse=1e-6, variant=0):
    from vcrnet_amd import refine
    a = refine.RefineArgs()
    a.src, a.tgt, a.R_out, a.t_out, a.fitness, a.rmse = 0x1000, 0x2000, 0x3000, 0x4000, 0x5000, 0x6000   # (never dereferenced on the host)
    a.B, a.Ns, a.Nt, a.max_dist, a.max_iterations, a.variant = B, Ns, Nt, max_dist, max_iterations, variant
    a.rel_fitness, a.rel_rmse = rel_fitness, rel_rmse
    return a


def test_argument_errors_return_their_codes_without_a_gpu(lib):
    from vcrnet_amd import refine
    f32 = lambda a, ws=0x10000, n=1 << 40: lib.vcr_refine_f32(ctypes.byref(a), ws, n, None)   # noqa: E731
    form = lambda a: lib.vcr_refine_form(ctypes.byref(a), 256, None, None)                     # noqa: E731
    size = lambda a: lib.vcr_refine_workspace_bytes(ctypes.byref(a), 256)                      # noqa: E731
    assert lib.vcr_refine_f32(None, 0x10000, 1 << 40, None) == EINVAL
    assert lib.vcr_refine_form(None, 256, None, None) == EINVAL and lib.vcr_refine_workspace_bytes(None, 256) == 0
    assert form(_args()) == 0 and size(_args()) > 0
    for field in ("src", "tgt", "R_out", "t_out", "fitness", "rmse"):
        a = _args()
        setattr(a, field, None)
        assert f32(a) == EINVAL and form(a) == EINVAL and size(a) == 0, field
    for field in ("R", "t"):                                   # an initial pose is both or neither
        a = _args()
        setattr(a, field, 0x7000)
        assert f32(a) == EINVAL and form(a) == EINVAL and size(a) == 0, field
    a = _args()
    a.R, a.t = 0x7000, 0x8000
    assert form(a) == 0
    nan, inf = float("nan"), float("inf")
    for kw in (dict(Ns=0), dict(Nt=0), dict(B=0), dict(Ns=-3), dict(Nt=-1), dict(max_dist=-1e-3), dict(max_dist=nan),
               dict(max_dist=inf), dict(max_dist=-inf), dict(max_iterations=-1), dict(rel_fitness=-1e-9), dict(rel_fitness=nan),
               dict(rel_fitness=inf), dict(rel_rmse=-1e-9), dict(rel_rmse=nan), dict(rel_rmse=inf), dict(variant=3), dict(variant=8),
               dict(variant=-1), dict(variant=refine.variant(1, 129)), dict(variant=1 << 16)):
        assert f32(_args(**kw)) == EINVAL and form(_args(**kw)) == EINVAL and size(_args(**kw)) == 0, kw
    for kw in (dict(max_dist=0.0), dict(max_iterations=0), dict(rel_fitness=0.0, rel_rmse=0.0), dict(max_iterations=refine.MAX_ITERATIONS)):
        assert form(_args(**kw)) == 0 and size(_args(**kw)) > 0, kw
    for kw in (dict(Ns=131073), dict(Nt=131073), dict(Ns=131072, Nt=5, B=16384), dict(Ns=5, Nt=131072, B=16384),
               dict(max_iterations=refine.MAX_ITERATIONS + 1)):
        assert f32(_args(**kw)) == EUNSUPPORTED and form(_args(**kw)) == EUNSUPPORTED and size(_args(**kw)) == 0, kw
    assert form(_args(Ns=131072, Nt=131072, B=16383)) == 0
    assert lib.vcr_refine_form(ctypes.byref(_args()), -1, None, None) == EINVAL
    # struct_bytes: unsized, short of rmse, longer than the library knows; the mandatory part alone is served
    for bad in (0, refine.RefineArgs.R_ba.offset - 4, ctypes.sizeof(refine.RefineArgs) + 8):
        a = _args()
        a.struct_bytes = bad
        assert f32(a) == EINVAL and form(a) == EINVAL and size(a) == 0, bad
    a = _args(variant=refine.variant(4, 3))
    q, s = ctypes.c_int(0), ctypes.c_int(0)
    assert lib.vcr_refine_form(ctypes.byref(a), 256, ctypes.byref(q), ctypes.byref(s)) == 0 and (q.value, s.value) == (4, 3)
    a.struct_bytes = refine.RefineArgs.R_ba.offset                                # ... and its variant reads as 0
    assert lib.vcr_refine_form(ctypes.byref(a), 256, ctypes.byref(q), ctypes.byref(s)) == 0 and (q.value, s.value) != (4, 3)
    # the workspace: missing, misaligned, short (the size is asked for the device at hand -- without one, 256 CUs)
    a = _args()
    need = lib.vcr_refine_workspace_bytes(ctypes.byref(a), 0)
    assert need == size(a) > 0
    assert f32(a, ws=None) == EINVAL and f32(a, ws=0x10004) == EINVAL and f32(a, ws=0x10008) == EINVAL
    assert f32(a, n=need - 1) == EWORKSPACE and f32(a, n=0) == EWORKSPACE


def test_the_form_is_the_scores_and_the_workspace_holds_the_rounds_state(lib):
    """One plan: the search runs in the form vcr_nn_score_f32 would pick for the same shape, forced halves included; the
    workspace adds seventeen fp64 partials per 256 source points and the per-cloud state (an fp64 pose and four words) to the
    score's candidates, and does not grow with max_iterations."""
    from vcrnet_amd import refine, score
    for B, Ns, Nt in ((1, 1, 1), (16, 1024, 1024), (1, 131072, 131072), (3, 1137, 1500), (1, 70001, 131072), (256, 16384, 16384)):
        for v in (0, refine.variant(4), refine.variant(0, 7), refine.variant(2, 128)):
            q, s, ws = refine.refine_form(B, Ns, Nt, variant=v)
            assert (q, s) == score.nn_score_form(B, Ns, Nt, variant=v)[:2], (B, Ns, Nt, v)
            assert ws >= s * B * Ns * 8 + B * ((Ns + 255) // 256) * 17 * 8 + B * (12 * 8 + 4 * 4), (B, Ns, Nt, v, ws)
            assert ws == refine.refine_form(B, Ns, Nt, variant=v, max_iterations=0)[2]
    assert refine.refine_form(1, 1024, 131072, cu_count=1)[:2] == score.nn_score_form(1, 1024, 131072, cu_count=1)[:2] == (1, 16)
    with pytest.raises(Exception):
        refine.refine_form(1, 131073, 10)


@pytest.mark.parametrize("kind,Nb,Ns,seed", [("cube", 700, 300, 1), ("torus", 700, 300, 2), ("cube", 1500, 1100, 3),
                                             ("torus", 1500, 1100, 1), ("cube", 2600, 2100, 2), ("torus", 2600, 2100, 3)])
def test_the_restatement_recovers_the_planted_pose(kind, Nb, Ns, seed):
    """The recipe of the GPU tests, on the CPU, at its three shapes: the loop converges inside max_iterations = 30 updates, every clean source point ends on its
    twin, the far points stay out, and the pose is the planted one as closely as fp32 clouds allow.  One step from the final
    neighbours is a proper rotation and optimal for its covariance (the checks the GPU step is held to)."""
    p = rr.pair(seed, Nb, Ns, kind)
    assert np.abs(p["R0"] - p["R"]).max() > 0.01 and 0.039 < np.linalg.norm(p["t0"] - p["t"]) < 0.041
    start = rr.evaluate(p["src"], p["tgt"], p["R0"], p["t0"], rr.MAX_DIST)
    assert not np.array_equal(start["nn_idx"][:Ns], p["twin"])                # the start is no solution
    o = rr.icp(p["src"], p["tgt"], p["R0"], p["t0"], rr.MAX_DIST)
    assert o["converged"] == 1 and 3 <= o["iterations"] < 30           # (30 = max_iterations: the loop stopped on its own)
    assert o["inliers"] == Ns and np.array_equal(o["nn_idx"][:Ns], p["twin"])
    assert (o["nn_d2"][Ns:] > 1.0).all() and o["fitness"] == np.float32(Ns) / np.float32(Ns + rr.FAR)
    assert np.abs(o["R"] - p["R"]).max() <= 1e-6 and np.abs(o["t"] - p["t"]).max() <= 1e-6
    assert o["rmse"] <= 1e-6
    up = rr.step(p["src"], p["tgt"], p["R0"], p["t0"], start["nn_idx"], start["nn_d2"], rr.MAX_DIST)
    assert 3 <= up["n"] < Ns + rr.FAR
    assert np.abs(up["R"] @ up["R"].T - np.eye(3)).max() <= 1e-12 and abs(np.linalg.det(up["R"]) - 1) <= 1e-12
    assert (up["opt"] - np.trace(up["R"] @ up["H"])) / up["s1"] <= 1e-12
    # the sums' order changes nothing beyond fp64 rounding, and H is the centred covariance
    limit = np.float32(rr.MAX_DIST) * np.float32(rr.MAX_DIST)
    inl = (start["nn_idx"] >= 0) & (start["nn_d2"] <= limit)
    pm = rr.nr.moved(p["src"], p["R0"], p["t0"]).astype(np.float64)[:, inl]
    q = p["tgt"].astype(np.float64)[:, start["nn_idx"][inl]]
    H = (pm - pm.mean(1, keepdims=True)) @ (q - q.mean(1, keepdims=True)).T
    assert np.abs(up["H"] - H).max() <= 1e-12 * up["n"]


def test_the_restatement_stops_as_the_header_says():
    p = rr.pair(5, 700, 300)
    # no update asked for: the evaluation of the start
    o = rr.icp(p["src"], p["tgt"], p["R0"], p["t0"], rr.MAX_DIST, max_iterations=0)
    e = rr.evaluate(p["src"], p["tgt"], p["R0"], p["t0"], rr.MAX_DIST)
    assert o["iterations"] == 0 and o["converged"] == 0 and o["inliers"] == e["inliers"] and np.array_equal(o["R"], p["R0"])
    # thresholds of zero never converge (the test is strict)
    o = rr.icp(p["src"], p["tgt"], p["R0"], p["t0"], rr.MAX_DIST, max_iterations=4, rel_fitness=0.0, rel_rmse=0.0)
    assert o["iterations"] == 4 and o["converged"] == 0
    # fewer than three inliers: the pose stays
    two = np.ascontiguousarray(p["src"][:, [0, 1, 300, 301]])            # two clean points and two far ones against the clean two
    tg = np.ascontiguousarray(two[:, :2])
    o = rr.icp(two, tg, None, None, rr.MAX_DIST)
    assert o["inliers"] == 2 and o["iterations"] == 0 and o["converged"] == 0 and np.array_equal(o["R"], np.eye(3, dtype=np.float32))


def test_python_entry_points_refuse_what_they_cannot_run():
    import vcrnet_amd
    from vcrnet_amd import native, refine
    assert vcrnet_amd.refine_registration is refine.refine_registration and "refine_registration" in vcrnet_amd.__all__
    a, b = torch.zeros(2, 3, 300), torch.zeros(2, 3, 410)
    with pytest.raises(native.VcrHipError, match="no CPU fallback"):
        vcrnet_amd.refine_registration(a, b, max_dist=0.1)
    with pytest.raises(native.VcrHipError, match="same number of clouds"):
        vcrnet_amd.refine_registration(a, torch.zeros(3, 3, 410), max_dist=0.1)
    with pytest.raises(native.VcrHipError, match=r"\[B, 3, N\]"):
        vcrnet_amd.refine_registration(a.transpose(1, 2), b, max_dist=0.1)
    with pytest.raises(native.VcrHipError, match=r"\[B, 3, N\]"):
        vcrnet_amd.refine_registration(a, torch.zeros(3, 410), max_dist=0.1)
