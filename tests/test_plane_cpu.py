"""Normals and the point-to-plane refinement, without a GPU: the boundary of include/vcr_hip_plane.h (prototypes against
vcrnet_amd.plane.SIGNATURES, the structs against gcc's layout), every argument error, the host-only form and workspace queries,
the resource remarks of the new kernels, and the numpy restatement (tests/plane_restated.py) on the recipes the GPU tests use."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import boundary
import plane_restated as pr
import refine_restated as rr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "vcr_hip_plane.h")
EINVAL, EWORKSPACE, EUNSUPPORTED = -1, -2, -3
NORMALS_SHAPES = ((1, 5, 4), (2, 64, 20), (3, 257, 20), (2, 1000, 40), (1, 300, 62))     # (B, N, k) of tests/test_hip_normals.py


@pytest.fixture(scope="module")
def lib():
    import vcrnet_amd  # noqa: F401
    from vcrnet_amd import build, plane
    build.build()
    return plane.lib()


def test_signatures_match_the_header_and_the_library_exports_them(lib):
    from vcrnet_amd import plane
    boundary.check_signatures(HEADER, plane, lib, {"vcr_normals_f32", "vcr_refine_plane_workspace_bytes", "vcr_refine_plane_f32",
                                                   "vcr_refine_plane_form"})


def test_the_other_boundaries_are_where_they_were(lib, monkeypatch):
    from vcrnet_amd import build, native, plane, refine, score
    assert lib.vcr_abi_version() == native.ABI_VERSION == 27 and len(refine.SIGNATURES) == 3 and len(score.SIGNATURES) == 3
    for other in (native, score, refine):
        assert not set(plane.SIGNATURES) & set(other.SIGNATURES) and not set(plane.STRUCTS) & set(other.STRUCTS)
    for header in ("vcr_hip.h", "vcr_hip_score.h", "vcr_hip_refine.h"):
        text = open(os.path.join(ROOT, "include", header)).read()
        assert "vcr_normals" not in text and "vcr_refine_plane" not in text
    assert os.path.basename(build.PUBLIC_HEADERS[-1]) == "vcr_hip_plane.h"
    full = build.sources_sha16()                              # the digests take the new header in
    monkeypatch.setattr(build, "PUBLIC_HEADERS", build.PUBLIC_HEADERS[:-1])
    assert build.sources_sha16() != full
    monkeypatch.undo()
    assert int(re.search(r"#define\s+VCR_NORMALS_MAX_K\s+(\d+)", open(HEADER).read()).group(1)) == plane.MAX_K == 62
    assert [f[0] for f in plane.RefinePlaneArgs._fields_] == [f[0] for f in refine.RefineArgs._fields_] + ["tgt_normals"]
    for name, _ in refine.RefineArgs._fields_:
        assert getattr(plane.RefinePlaneArgs, name).offset == getattr(refine.RefineArgs, name).offset, name


def test_args_match_the_c_layout(tmp_path):
    import vcrnet_amd  # noqa: F401
    from vcrnet_amd import plane
    boundary.check_layout(HEADER, plane, tmp_path)


def _nargs(B=2, N=100, k=20):
    from vcrnet_amd import plane
    a = plane.NormalsArgs()
    a.xyz4, a.idx, a.normals = 0x1000, 0x2000, 0x3000          # (never dereferenced: every call below is refused on the host)
    a.B, a.N, a.k = B, N, k
    return a


def test_normals_argument_errors_return_their_codes_without_a_gpu(lib):
    from vcrnet_amd import plane
    f32 = lambda a: lib.vcr_normals_f32(ctypes.byref(a), None)          # noqa: E731
    assert lib.vcr_normals_f32(None, None) == EINVAL
    for field in ("xyz4", "idx", "normals"):
        a = _nargs()
        setattr(a, field, None)
        assert f32(a) == EINVAL, field
    a = _nargs()
    a.xyz4 = 0x1008                                            # rows are read 16 B at a time
    assert f32(a) == EINVAL
    for kw in (dict(k=0), dict(k=-1), dict(B=0), dict(N=0), dict(B=-2), dict(N=-5)):
        assert f32(_nargs(**kw)) == EINVAL, kw
    for kw in (dict(k=63), dict(N=131073), dict(B=16384, N=131072)):
        assert f32(_nargs(**kw)) == EUNSUPPORTED, kw
    for bad in (0, plane.NormalsArgs.curvature.offset - 4, ctypes.sizeof(plane.NormalsArgs) + 8):
        a = _nargs()
        a.struct_bytes = bad
        assert f32(a) == EINVAL, bad


def _args(B=2, Ns=1000, Nt=1500, max_dist=0.1, max_iterations=30, rel_fitness=1e-6, rel_rmse=1e-6, variant=0):
    from vcrnet_amd import plane
    a = plane.RefinePlaneArgs()
    a.src, a.tgt, a.R_out, a.t_out, a.fitness, a.rmse, a.tgt_normals = 0x1000, 0x2000, 0x3000, 0x4000, 0x5000, 0x6000, 0x7000
    a.B, a.Ns, a.Nt, a.max_dist, a.max_iterations, a.variant = B, Ns, Nt, max_dist, max_iterations, variant
    a.rel_fitness, a.rel_rmse = rel_fitness, rel_rmse
    return a


def test_refine_plane_argument_errors_return_their_codes_without_a_gpu(lib):
    from vcrnet_amd import plane, refine
    f32 = lambda a, ws=0x10000, n=1 << 40: lib.vcr_refine_plane_f32(ctypes.byref(a), ws, n, None)   # noqa: E731
    form = lambda a: lib.vcr_refine_plane_form(ctypes.byref(a), 256, None, None)                     # noqa: E731
    size = lambda a: lib.vcr_refine_plane_workspace_bytes(ctypes.byref(a), 256)                      # noqa: E731
    assert lib.vcr_refine_plane_f32(None, 0x10000, 1 << 40, None) == EINVAL
    assert lib.vcr_refine_plane_form(None, 256, None, None) == EINVAL and lib.vcr_refine_plane_workspace_bytes(None, 256) == 0
    assert form(_args()) == 0 and size(_args()) > 0
    for field in ("src", "tgt", "R_out", "t_out", "fitness", "rmse", "tgt_normals"):
        a = _args()
        setattr(a, field, None)
        assert f32(a) == EINVAL and form(a) == EINVAL and size(a) == 0, field
    for field in ("R", "t"):                                   # an initial pose is both or neither
        a = _args()
        setattr(a, field, 0x8000)
        assert f32(a) == EINVAL and form(a) == EINVAL and size(a) == 0, field
    nan, inf = float("nan"), float("inf")
    for kw in (dict(Ns=0), dict(Nt=0), dict(B=0), dict(Ns=-3), dict(Nt=-1), dict(B=-1), dict(max_dist=-1e-3), dict(max_dist=nan),
               dict(max_dist=inf), dict(max_iterations=-1), dict(rel_fitness=-1e-9), dict(rel_fitness=nan), dict(rel_rmse=inf),
               dict(variant=3), dict(variant=-1), dict(variant=refine.variant(1, 129))):
        assert f32(_args(**kw)) == EINVAL and form(_args(**kw)) == EINVAL and size(_args(**kw)) == 0, kw
    for kw in (dict(max_dist=0.0), dict(max_iterations=0), dict(rel_fitness=0.0, rel_rmse=0.0), dict(max_iterations=refine.MAX_ITERATIONS)):
        assert form(_args(**kw)) == 0 and size(_args(**kw)) > 0, kw
    for kw in (dict(Ns=131073), dict(Nt=131073), dict(Ns=131072, Nt=5, B=16384), dict(max_iterations=refine.MAX_ITERATIONS + 1)):
        assert f32(_args(**kw)) == EUNSUPPORTED and form(_args(**kw)) == EUNSUPPORTED and size(_args(**kw)) == 0, kw
    assert lib.vcr_refine_plane_form(ctypes.byref(_args()), -1, None, None) == EINVAL
    # struct_bytes: unsized, short of the mandatory part (tgt_normals, the last field), longer than the library knows
    for bad in (0, plane.RefinePlaneArgs.tgt_normals.offset, ctypes.sizeof(plane.RefinePlaneArgs) + 8):
        a = _args()
        a.struct_bytes = bad
        assert f32(a) == EINVAL and form(a) == EINVAL and size(a) == 0, bad
    # the workspace: missing, misaligned, short
    a = _args()
    need = lib.vcr_refine_plane_workspace_bytes(ctypes.byref(a), 0)
    assert need == size(a) > 0
    assert f32(a, ws=None) == EINVAL and f32(a, ws=0x10004) == EINVAL and f32(a, ws=0x10008) == EINVAL
    assert f32(a, n=need - 1) == EWORKSPACE and f32(a, n=0) == EWORKSPACE


def test_the_form_is_the_point_to_point_refinements(lib):
    """One plan: the search runs in vcr_refine_form's form for the same shape, forced halves included; the workspace holds
    twenty-nine fp64 partials per 256 source points where that one holds seventeen."""
    from vcrnet_amd import plane, refine
    for B, Ns, Nt in ((1, 1, 1), (16, 1024, 1024), (1, 131072, 131072), (3, 1137, 1500), (1, 70001, 131072)):
        for v in (0, refine.variant(4), refine.variant(0, 7), refine.variant(2, 128)):
            q, s, ws = plane.refine_plane_form(B, Ns, Nt, variant=v)
            q0, s0, ws0 = refine.refine_form(B, Ns, Nt, variant=v)
            assert (q, s) == (q0, s0), (B, Ns, Nt, v)
            assert ws0 <= ws <= ws0 + B * ((Ns + 255) // 256) * 12 * 8 + 256, (B, Ns, Nt, v, ws, ws0)
            assert ws >= s * B * Ns * 8 + B * ((Ns + 255) // 256) * 29 * 8 + B * (12 * 8 + 4 * 4)
            assert ws == plane.refine_plane_form(B, Ns, Nt, variant=v, max_iterations=0)[2]
    with pytest.raises(Exception):
        plane.refine_plane_form(1, 131073, 10)


def test_the_new_kernels_use_no_scratch(lib):
    from vcrnet_amd import build
    res = build.kernel_resources()
    new = {k: v for k, v in res.items() if v["file"] in ("normals.hip", "refine_plane.hip")}
    names = sorted(k for k in new)
    for want in ("normals_kernel", "plane_merge_kernel", "plane_cloud_kernel"):
        assert any(want in n for n in names), (want, names)
    for k, v in new.items():
        assert v.get("scratch", 0) == 0 and v.get("vgpr_spill", 0) == 0, (k, v)
    hot = [v for k, v in new.items() if "normals_kernel" in k or "plane_merge_kernel" in k]
    assert all(v["vgprs"] + v.get("agprs", 0) <= 64 and v["occupancy"] == 8 for v in hot), hot     # eight waves per SIMD


# ------------------------------------------------------------------------------------------------------------- the restatement

@pytest.mark.parametrize("B,N,k", NORMALS_SHAPES)
def test_the_normals_recipe_keeps_its_eigenvalues_apart(B, N, k):
    """The GPU test leaves a point out of the comparison of normals where lambda1 - lambda0 < 2^-10 lambda2: on the jittered
    torus at most 1 % of a case, checked here with float64 neighbours."""
    for b in range(B):
        x = pr.jittered_torus(100 * N + b, N)
        C = pr.covariances(x, pr.knn_f64(x, k))
        lam = np.linalg.eigvalsh(C)
        assert (lam[:, 1] - lam[:, 0] < 2.0 ** -10 * lam[:, 2]).mean() <= 0.01
        i = N // 2
        assert np.array_equal(pr.covariance(x, i, pr.knn_f64(x, k)[i]), C[i])
        n, lam_i, cv = pr.normal(C[i])
        assert abs(np.linalg.norm(n.astype(np.float64)) - 1) <= 2.0 ** -22 and n[np.argmax(np.abs(n))] > 0
        nd = n.astype(np.float64)                           # (the Rayleigh quotient: see tests/test_hip_normals.py)
        assert nd @ C[i] @ nd / (nd @ nd) - lam_i[0] <= 2.0 ** -40 * lam_i[2]
        assert 0 <= cv <= 1 / 3 + 1e-6


def test_the_restated_normal_follows_the_surface_and_the_sign_rules():
    p = rr.pair(2, 2600, 300, "torus")
    true = pr.pair_normals(2, 2600, p)
    C = pr.covariances(p["tgt"], pr.knn_f64(p["tgt"], 12))
    n = np.stack([pr.normal(c)[0] for c in C], axis=1)
    cos = np.abs((n.astype(np.float64) * true).sum(0))
    assert np.median(cos) > 0.98 and (cos > 0.9).mean() > 0.9   # (12 neighbours on a tube of radius 0.12: a few degrees)
    # towards a viewpoint, away from it, at a right angle to it (the other rule decides)
    x = np.asarray([1, 2, 3], np.float32)
    assert np.array_equal(pr.orient([0, 0, -1], x, [1, 2, 9]), np.asarray([0, 0, 1], np.float32))
    assert np.array_equal(pr.orient([0, 0, -1], x, [1, 2, -9]), np.asarray([0, 0, -1], np.float32))
    assert np.array_equal(pr.orient([0, -1, 0], x, [1, 2, 9]), np.asarray([0, 1, 0], np.float32))
    assert np.array_equal(pr.orient([-0.5, 0.5, 0]), np.asarray([0.5, -0.5, 0], np.float32))     # the lowest index among equals
    # degenerate sets
    assert pr.normal(np.zeros((3, 3)))[0].tolist() == [0, 0, 1] and pr.normal(np.zeros((3, 3)))[2] == 0
    bad = pr.normal(np.full((3, 3), np.nan))
    assert bad[0].tolist() == [0, 0, 1] and np.isnan(bad[2])


@pytest.mark.parametrize("Nb,Ns,seed", [(700, 300, 2), (1500, 1100, 1)])
def test_the_restatement_recovers_the_planted_pose(Nb, Ns, seed):
    """The recipe of the GPU tests with the torus's true normals: the loop stops on its own inside 30 updates, every clean
    source point ends on its twin, the pose is the planted one as closely as fp32 clouds allow; one step's system is well
    conditioned (the bound the GPU step is held to scales with cond(A)) and its update a proper rotation."""
    p = rr.pair(seed, Nb, Ns, "torus")
    nrm = pr.pair_normals(seed, Nb, p)
    assert np.abs(np.linalg.norm(nrm.astype(np.float64), axis=0) - 1).max() <= 1e-6
    o = pr.plane_icp(p["src"], p["tgt"], nrm, p["R0"], p["t0"], rr.MAX_DIST)
    assert o["converged"] == 1 and 2 <= o["iterations"] < 30
    assert o["inliers"] == Ns and np.array_equal(o["nn_idx"][:Ns], p["twin"])
    assert np.abs(o["R"] - p["R"]).max() <= 1e-6 and np.abs(o["t"] - p["t"]).max() <= 1e-6 and o["rmse"] <= 1e-6
    start = rr.evaluate(p["src"], p["tgt"], p["R0"], p["t0"], rr.MAX_DIST)
    up = pr.plane_step(p["src"], p["tgt"], nrm, p["R0"], p["t0"], start["nn_idx"], start["nn_d2"], rr.MAX_DIST)
    assert 6 <= up["n"] < Ns + rr.FAR and up["cond"] < 1e6
    assert np.abs(up["R"] @ up["R"].T - np.eye(3)).max() <= 1e-12 and abs(np.linalg.det(up["R"]) - 1) <= 1e-12
    assert np.abs(up["A"] @ up["x"] + up["g"]).max() <= 1e-9 * np.abs(up["g"]).max()


def test_the_restatement_stops_as_the_header_says():
    p = rr.pair(5, 700, 300, "torus")
    nrm = pr.pair_normals(5, 700, p)
    o = pr.plane_icp(p["src"], p["tgt"], nrm, p["R0"], p["t0"], rr.MAX_DIST, max_iterations=0)
    e = rr.evaluate(p["src"], p["tgt"], p["R0"], p["t0"], rr.MAX_DIST)
    assert o["iterations"] == 0 and o["converged"] == 0 and o["inliers"] == e["inliers"] and np.array_equal(o["R"], p["R0"])
    o = pr.plane_icp(p["src"], p["tgt"], nrm, p["R0"], p["t0"], rr.MAX_DIST, max_iterations=4, rel_fitness=0.0, rel_rmse=0.0)
    assert o["iterations"] == 4 and o["converged"] == 0
    # fewer than six inliers: the pose stays
    five = np.ascontiguousarray(p["tgt"][:, :5])
    o = pr.plane_icp(five, five, nrm[:, :5], None, None, rr.MAX_DIST)
    assert o["inliers"] == 5 and o["iterations"] == 0 and o["converged"] == 0 and np.array_equal(o["R"], np.eye(3, dtype=np.float32))
    # a planar target with equal normals: three of the six unknowns are free -- singular
    rs = np.random.RandomState(3)
    flat = np.concatenate([rs.uniform(0, 1, (2, 400)), np.full((1, 400), 0.25)]).astype(np.float32)
    up_n = np.tile(np.asarray([[0], [0], [1]], np.float32), (1, 400))
    src = np.ascontiguousarray(flat[:, :200] + np.asarray([[0.001], [0.002], [0.003]], np.float32))
    ev = rr.evaluate(src, flat, None, None, rr.MAX_DIST)
    assert ev["inliers"] == 200
    n, A, g = pr.plane_sums(src, flat[:, ev["nn_idx"]], up_n[:, ev["nn_idx"]], np.ones(200, bool))
    assert n == 200 and pr.singular(A)
    assert pr.plane_step(src, flat, up_n, np.eye(3, dtype=np.float32), np.zeros(3, np.float32), ev["nn_idx"], ev["nn_d2"], rr.MAX_DIST) is None
    o = pr.plane_icp(src, flat, up_n, None, None, rr.MAX_DIST)
    assert o["iterations"] == 0 and o["converged"] == 0 and np.array_equal(o["R"], np.eye(3, dtype=np.float32)) and not o["t"].any()


def test_python_entry_points_refuse_what_they_cannot_run():
    import vcrnet_amd
    from vcrnet_amd import native, plane
    assert vcrnet_amd.estimate_normals is plane.estimate_normals and "estimate_normals" in vcrnet_amd.__all__
    a, b = torch.zeros(2, 3, 300), torch.zeros(2, 3, 410)
    with pytest.raises(native.VcrHipError, match="no CPU fallback"):
        vcrnet_amd.estimate_normals(a)
    with pytest.raises(native.VcrHipError, match=r"\[B, 3, N\]"):
        vcrnet_amd.estimate_normals(a.transpose(1, 2))
    with pytest.raises(native.VcrHipError, match="method must be one of"):
        vcrnet_amd.refine_registration(a, b, max_dist=0.1, method="plane")
    with pytest.raises(native.VcrHipError, match="point_to_plane' only"):
        vcrnet_amd.refine_registration(a, b, max_dist=0.1, tgt_normals=b)
    with pytest.raises(native.VcrHipError, match="no CPU fallback"):
        vcrnet_amd.refine_registration(a, b, max_dist=0.1, method="point_to_plane")
    with pytest.raises(native.VcrHipError, match=r"tgt_normals must be \[B, 3, Nt\]"):
        vcrnet_amd.refine_registration(a, b, max_dist=0.1, method="point_to_plane", tgt_normals=a)
