"""The plane-to-plane refinement, without a GPU: the boundary of include/vcr_hip_gicp.h (prototypes against
vcrnet_amd.gicp.SIGNATURES, the struct against gcc's layout, the exported symbols), every argument error, the host-only form and
workspace queries, the resource remarks of the two new kernels, the two numpy restatements (tests/gicp_restated.py) against each
other, and the conditioning of every recipe the GPU tests use."""
import ctypes
import os
import subprocess

import numpy as np
import pytest
import torch

import boundary
import gicp_restated as gr
import nnscore_restated as nr
import refine_restated as rr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INCLUDE = os.path.join(ROOT, "include")
HEADER = os.path.join(INCLUDE, "vcr_hip_gicp.h")
EINVAL, EWORKSPACE, EUNSUPPORTED = -1, -2, -3
ENTRY_POINTS = {"vcr_refine_gicp_workspace_bytes", "vcr_refine_gicp_f32", "vcr_refine_gicp_form"}
# (seed, Nb, Ns, undisturbed) of every rr.batch recipe tests/test_hip_gicp.py runs
GPU_RECIPES = [(20 + Ns, Nb, Ns, ()) for Nb, Ns in rr.SHAPES[:2]] + [(10 + Ns, Nb, Ns, ()) for Nb, Ns in rr.SHAPES[:2]] + \
              [(41, rr.SHAPES[1][0], rr.SHAPES[1][1], (1,)), (77, 700, 256 - rr.FAR, ())]


@pytest.fixture(scope="module")
def lib():
    import vcrnet_amd  # noqa: F401
    from vcrnet_amd import build, gicp
    build.build()
    return gicp.lib()


def test_signatures_match_the_header_and_the_library_exports_them(lib):
    from vcrnet_amd import gicp
    boundary.check_signatures(HEADER, gicp, lib, ENTRY_POINTS)


def test_args_match_the_c_layout(tmp_path):
    import vcrnet_amd  # noqa: F401
    from vcrnet_amd import gicp
    boundary.check_layout(HEADER, gicp, tmp_path)


def test_the_other_boundaries_are_where_they_were(lib, monkeypatch):
    """The fit lives beside the six headers, not in them: none mentions it, ABI 27, the same 51 prototypes; the new header is
    taken into the digests through a list of its own; vcr_refine_args' fields lead the struct at their offsets."""
    from vcrnet_amd import build, gicp, native, plane, refine
    for h in ("vcr_hip.h", "vcr_hip_score.h", "vcr_hip_refine.h", "vcr_hip_plane.h", "vcr_hip_voxel.h", "vcr_hip_outlier.h"):
        assert "vcr_refine_gicp" not in open(os.path.join(INCLUDE, h)).read(), h
    assert len(native.PUBLIC) == 51 and lib.vcr_abi_version() == native.ABI_VERSION == 27
    for other in (native, refine, plane):
        assert not set(gicp.SIGNATURES) & set(other.SIGNATURES) and not set(gicp.STRUCTS) & set(other.STRUCTS)
    full = build.sources_sha16()
    assert build.GICP_HEADERS == [HEADER] and HEADER not in build.PUBLIC_HEADERS + build.LATER_HEADERS + build.OUTLIER_HEADERS
    monkeypatch.setattr(build, "GICP_HEADERS", [])
    assert build.sources_sha16() != full
    monkeypatch.undo()
    names = [f[0] for f in gicp.RefineGicpArgs._fields_]
    assert names == [f[0] for f in refine.RefineArgs._fields_] + ["tgt_normals", "src_normals", "epsilon"]
    for name, _ in refine.RefineArgs._fields_:
        assert getattr(gicp.RefineGicpArgs, name).offset == getattr(refine.RefineArgs, name).offset, name
    assert gicp.RefineGicpArgs.tgt_normals.offset == plane.RefinePlaneArgs.tgt_normals.offset == ctypes.sizeof(refine.RefineArgs)
    assert refine.METHODS == ("point_to_point", "point_to_plane", "generalized")


def _args(B=2, Ns=1000, Nt=1500, max_dist=0.1, max_iterations=30, rel_fitness=1e-6, rel_rmse=1e-6, variant=0, epsilon=1e-3):
    from vcrnet_amd import gicp
    a = gicp.RefineGicpArgs()
    a.src, a.tgt, a.R_out, a.t_out, a.fitness, a.rmse, a.tgt_normals, a.src_normals = (0x1000, 0x2000, 0x3000, 0x4000, 0x5000, 0x6000,
                                                                                        0x7000, 0x9000)   # (never dereferenced)
    a.B, a.Ns, a.Nt, a.max_dist, a.max_iterations, a.variant = B, Ns, Nt, max_dist, max_iterations, variant
    a.rel_fitness, a.rel_rmse, a.epsilon = rel_fitness, rel_rmse, epsilon
    return a


def test_argument_errors_return_their_codes_without_a_gpu(lib):
    from vcrnet_amd import gicp, refine
    f32 = lambda a, ws=0x10000, n=1 << 40: lib.vcr_refine_gicp_f32(ctypes.byref(a), ws, n, None)   # noqa: E731
    form = lambda a: lib.vcr_refine_gicp_form(ctypes.byref(a), 256, None, None)                     # noqa: E731
    size = lambda a: lib.vcr_refine_gicp_workspace_bytes(ctypes.byref(a), 256)                      # noqa: E731
    refused = lambda a, code: f32(a) == code and form(a) == code and size(a) == 0                   # noqa: E731
    assert lib.vcr_refine_gicp_f32(None, 0x10000, 1 << 40, None) == EINVAL
    assert lib.vcr_refine_gicp_form(None, 256, None, None) == EINVAL and lib.vcr_refine_gicp_workspace_bytes(None, 256) == 0
    assert form(_args()) == 0 and size(_args()) > 0
    for field in ("src", "tgt", "R_out", "t_out", "fitness", "rmse", "tgt_normals", "src_normals"):
        a = _args()
        setattr(a, field, None)
        assert refused(a, EINVAL), field
    nan, inf = float("nan"), float("inf")
    for eps in (0.0, -0.0, -1e-3, 1.0000001, 2.0, nan, inf, -inf):
        assert refused(_args(epsilon=eps), EINVAL), eps
    for eps in (1.0, 1e-3, 1e-6, 1e-45):
        assert form(_args(epsilon=eps)) == 0 and size(_args(epsilon=eps)) == size(_args()), eps
    # the inherited refusals
    for field in ("R", "t"):                                   # an initial pose is both or neither
        a = _args()
        setattr(a, field, 0x8000)
        assert refused(a, EINVAL), field
    for kw in (dict(Ns=0), dict(Nt=0), dict(B=0), dict(Ns=-3), dict(Nt=-1), dict(B=-1), dict(max_dist=-1e-3), dict(max_dist=nan),
               dict(max_dist=inf), dict(max_iterations=-1), dict(rel_fitness=-1e-9), dict(rel_fitness=nan), dict(rel_rmse=inf),
               dict(variant=3), dict(variant=-1), dict(variant=refine.variant(1, 129))):
        assert refused(_args(**kw), EINVAL), kw
    for kw in (dict(max_dist=0.0), dict(max_iterations=0), dict(rel_fitness=0.0, rel_rmse=0.0), dict(max_iterations=refine.MAX_ITERATIONS)):
        assert form(_args(**kw)) == 0 and size(_args(**kw)) > 0, kw
    for kw in (dict(Ns=131073), dict(Nt=131073), dict(Ns=131072, Nt=5, B=16384), dict(max_iterations=refine.MAX_ITERATIONS + 1)):
        assert refused(_args(**kw), EUNSUPPORTED), kw
    assert lib.vcr_refine_gicp_form(ctypes.byref(_args()), -1, None, None) == EINVAL
    # struct_bytes: unsized, short of the mandatory part (epsilon, the last field), longer than the library knows
    for bad in (0, gicp.RefineGicpArgs.src_normals.offset, gicp.RefineGicpArgs.epsilon.offset, ctypes.sizeof(gicp.RefineGicpArgs) + 8):
        a = _args()
        a.struct_bytes = bad
        assert refused(a, EINVAL), bad
    # the workspace: missing, misaligned, short
    a = _args()
    need = lib.vcr_refine_gicp_workspace_bytes(ctypes.byref(a), 0)
    assert need == size(a) > 0
    assert f32(a, ws=None) == EINVAL and f32(a, ws=0x10004) == EINVAL and f32(a, ws=0x10008) == EINVAL
    assert f32(a, n=need - 1) == EWORKSPACE and f32(a, n=0) == EWORKSPACE


def test_the_form_and_the_workspace_are_the_plane_fits(lib):
    """One plan: the search runs in vcr_refine_form's form for the same shape, forced halves included, and the workspace holds
    twenty-nine fp64 partials per 256 source points, as the point-to-plane fit's."""
    from vcrnet_amd import gicp, plane, refine
    for B, Ns, Nt in ((1, 1, 1), (1, 5, 7), (16, 1024, 1024), (1, 131072, 131072), (3, 1137, 1500), (1, 70001, 131072)):
        for v in (0, refine.variant(4), refine.variant(0, 7), refine.variant(2, 128)):
            for cu in (256, 1, 304):
                q, s, ws = gicp.refine_gicp_form(B, Ns, Nt, cu_count=cu, variant=v)
                assert (q, s) == refine.refine_form(B, Ns, Nt, cu_count=cu, variant=v)[:2], (B, Ns, Nt, v, cu)
                assert (q, s, ws) == plane.refine_plane_form(B, Ns, Nt, cu_count=cu, variant=v), (B, Ns, Nt, v, cu)
            assert ws == gicp.refine_gicp_form(B, Ns, Nt, cu_count=304, variant=v, max_iterations=0)[2]
    with pytest.raises(Exception):
        gicp.refine_gicp_form(1, 131073, 10)


def test_the_new_kernels_use_no_scratch_and_the_merge_keeps_eight_waves(lib):
    """hipcc's remarks for the two kernels of refine_gicp.hip, pinned: the merge at 54 VGPRs (W, p and d live across twenty-seven
    butterflies) and eight waves per SIMD; the per-cloud kernel is plane_cloud_kernel's text with another MIN_INLIERS, and its
    90 VGPRs and five waves (one workgroup per cloud: its occupancy carries nothing)."""
    from vcrnet_amd import build
    res = build.kernel_resources()
    names = list(res)
    dem = subprocess.run(["c++filt"], input="\n".join(names), capture_output=True, text=True, check=True).stdout.splitlines()
    mine = {d.replace("(anonymous namespace)::", "").split("(")[0]: res[n] for n, d in zip(names, dem) if res[n]["file"] == "refine_gicp.hip"}
    assert set(mine) == {"gicp_merge_kernel", "gicp_cloud_kernel"}
    for k, v in mine.items():
        assert v.get("scratch", 0) == 0 and v.get("vgpr_spill", 0) == 0 and v.get("sgpr_spill", 0) == 0, (k, v)
    merge, cloud = mine["gicp_merge_kernel"], mine["gicp_cloud_kernel"]
    assert (merge["vgprs"], merge.get("agprs", 0), merge["occupancy"]) == (54, 0, 8), merge
    assert (cloud["vgprs"], cloud.get("agprs", 0), cloud["occupancy"]) == (90, 0, 5), cloud
    plane_cloud = [v for n, v in res.items() if "plane_cloud_kernel" in n][0]
    assert (cloud["vgprs"], cloud["occupancy"], cloud["lds"]) == (plane_cloud["vgprs"], plane_cloud["occupancy"], plane_cloud["lds"])


# ------------------------------------------------------------------------------------------------------------ the restatements

def _first_rounds():
    """(name, src, tgt, nrm_s, nrm_t, R0, t0, evaluation of the start) of every cloud of every recipe the GPU tests run, and
    the tiny case."""
    out = []
    for seed, Nb, Ns, und in GPU_RECIPES:
        c = gr.batch(seed, Nb, Ns, und)
        for b in range(3):
            out.append(((seed, Nb, Ns, b), c["src"][b], c["tgt"][b], c["nrm_s"][b], c["nrm_t"][b], c["R0"][b], c["t0"][b]))
    c = gr.tiny()
    out.append(("tiny", c["src"][0], c["tgt"][0], c["nrm_s"][0], c["nrm_t"][0], c["R0"][0], c["t0"][0]))
    return [o + (rr.evaluate(o[1], o[2], o[5], o[6], rr.MAX_DIST),) for o in out]


@pytest.fixture(scope="module")
def first_rounds():
    return _first_rounds()


def test_every_gpu_recipe_is_well_conditioned_at_its_first_round(first_rounds):
    """The bound the GPU step is held to scales with cond(A): every recipe keeps it at or below 1e6, with at least three
    inliers, unit normals to fp32's precision, and an update that is a proper rotation solving the system."""
    for name, src, tgt, ns, nt, R0, t0, ev in first_rounds:
        assert np.abs(np.linalg.norm(ns.astype(np.float64), axis=0) - 1).max() <= 1e-6, name
        assert np.abs(np.linalg.norm(nt.astype(np.float64), axis=0) - 1).max() <= 1e-6, name
        up = gr.gicp_step(src, tgt, ns, nt, R0, t0, ev["nn_idx"], ev["nn_d2"], rr.MAX_DIST)
        assert up is not None and up["n"] == ev["inliers"] >= 3, name
        assert up["cond"] <= 1e6, (name, up["cond"])
        assert np.abs(up["R"] @ up["R"].T - np.eye(3)).max() <= 1e-12 and abs(np.linalg.det(up["R"]) - 1) <= 1e-12
        assert np.abs(up["A"] @ up["x"] + up["g"]).max() <= 1e-9 * np.abs(up["g"]).max(), name
        assert np.array_equal(up["A"], up["A"].T)


def test_the_two_restatements_agree(first_rounds):
    """x of restatement 1 (the header's cofactors and sums) against x of restatement 2 (explicit covariances, numpy's inverse,
    a least-squares solve of the stacked rows) to 1e-9 (1 + |x|) on every recipe.  Both read the inputs as the definition
    idealises them (gicp_restated.idealised: unit normals and a rotation to float64's precision): the two forms of a covariance,
    I - (1 - eps) n n^T and Rot diag(eps,1,1) Rot^T, are one matrix only for |n| = 1, and fp32 normals miss that by 2^-23
    where M is 2 eps -- four digits, which says nothing about either formula."""
    for name, src, tgt, ns, nt, R0, t0, ev in first_rounds:
        inl = (ev["nn_idx"] >= 0) & (ev["nn_d2"] <= np.float32(rr.MAX_DIST) * np.float32(rr.MAX_DIST))
        at = np.maximum(ev["nn_idx"], 0)
        p, q = nr.moved(src, R0, t0), tgt[:, at]
        m, s, R = gr.idealised(nt[:, at], ns, R0)
        n, A, g = gr.gicp_sums(p, q, m, s, R, inl)
        x1 = np.linalg.solve(A, -g)
        x2 = gr.independent_x(p, q, m, s, R, inl)
        assert np.abs(x1 - x2).max() <= 1e-9 * (1 + np.abs(x1).max()), (name, x1, x2)
        # and on the fp32 inputs themselves the header's x stays within the four digits said above
        x0 = gr.gicp_step(src, tgt, ns, nt, R0, t0, ev["nn_idx"], ev["nn_d2"], rr.MAX_DIST)["x"]
        assert np.abs(x0 - x1).max() <= 1e-3 * (1 + np.abs(x1).max()), (name, x0, x1)


def test_the_sums_reduce_to_the_plane_fits_and_mask_what_is_no_inlier():
    """With W = m m^T the header's expressions are section 4.10's J J^T and J r; a lane that is no inlier adds exact zeros,
    within Ns or beyond it -- so the sums of a recipe and of the same recipe with more FAR points (and any normals) BEHIND it
    are bit-equal: the lanes the new points take added zeros before, and further workgroups add zero partials at the end."""
    import plane_restated as pr
    c = gr.batch(10 + 300, 700, 300)
    src, tgt, ns, nt, R0, t0 = (c[k][0] for k in ("src", "tgt", "nrm_s", "nrm_t", "R0", "t0"))
    ev = rr.evaluate(src, tgt, R0, t0, rr.MAX_DIST)
    inl = (ev["nn_idx"] >= 0) & (ev["nn_d2"] <= np.float32(rr.MAX_DIST) * np.float32(rr.MAX_DIST))
    at = np.maximum(ev["nn_idx"], 0)
    p, q, m = nr.moved(src, R0, t0), tgt[:, at], nt[:, at]
    n, A, g = gr.gicp_sums(p, q, m, ns, R0, inl)
    assert 3 <= n < src.shape[1] and inl[:300].sum() == n and not inl[300:].any()
    # the plane fit: a_r . (m m^T a_c) = J_r J_c
    _, Ap, gp = pr.plane_sums(p, q, m, inl)
    z = lambda a: np.where(inl, a, 0).astype(np.float64)     # noqa: E731
    pz, mz, dz = z(p), z(m), z(p) - z(q)
    W = mz[:, None, :] * mz[None, :, :]
    Aw = np.asarray([[gr._dot(r, pz, gr._u(col, pz, W)).sum() for col in range(6)] for r in range(6)])
    e = np.stack([(W[i, 0] * dz[0] + W[i, 1] * dz[1]) + W[i, 2] * dz[2] for i in range(3)])
    gw = np.asarray([gr._dot(r, pz, e).sum() for r in range(6)])
    assert np.abs(Aw - Ap).max() <= 1e-12 * np.abs(Ap).max() and np.abs(gw - gp).max() <= 1e-12 * np.abs(gp).max()
    # the mask: 200 more FAR points (the last workgroup stays partial); 431 (it fills, and a whole one follows)
    rs = np.random.RandomState(5)
    for extra in (200, 512 - 337 + 256):
        far = rs.uniform(2.0, 3.0, (3, extra)).astype(np.float32)
        junk = rs.normal(size=(3, extra)).astype(np.float32)
        src2, ns2 = np.concatenate([src, far], axis=1), np.concatenate([ns, junk], axis=1)
        ev2 = rr.evaluate(src2, tgt, R0, t0, rr.MAX_DIST)
        inl2 = np.concatenate([inl, np.zeros(extra, bool)])
        assert ev2["inliers"] == n
        at2 = np.maximum(ev2["nn_idx"], 0)
        n2, A2, g2 = gr.gicp_sums(nr.moved(src2, R0, t0), tgt[:, at2], nt[:, at2], ns2, R0, inl2)
        assert n2 == n
        assert np.array_equal(A2, A) and np.array_equal(g2, g), extra


def test_the_restatement_recovers_the_planted_pose_and_stops_as_the_header_says():
    import plane_restated as pr
    c = gr.batch(10 + 300, 700, 300)
    src, tgt, ns, nt, R0, t0 = (c[k][0] for k in ("src", "tgt", "nrm_s", "nrm_t", "R0", "t0"))
    o = gr.gicp_icp(src, tgt, ns, nt, R0, t0, rr.MAX_DIST)
    assert o["converged"] == 1 and 2 <= o["iterations"] < 30 and o["inliers"] == 300
    assert np.array_equal(o["nn_idx"][:300], c["twin"][0])
    e = pr.pose_error(o["R"], o["t"], c["R"][0], c["t"][0])
    assert e[0] <= 1e-5 and e[1] <= 1e-5, e
    # the signs of the normals do not enter: not by one bit
    rs = np.random.RandomState(9)
    fs, ft = rs.choice([-1.0, 1.0], ns.shape[1]).astype(np.float32), rs.choice([-1.0, 1.0], nt.shape[1]).astype(np.float32)
    ev = rr.evaluate(src, tgt, R0, t0, rr.MAX_DIST)
    a = gr.gicp_step(src, tgt, ns, nt, R0, t0, ev["nn_idx"], ev["nn_d2"], rr.MAX_DIST)
    b = gr.gicp_step(src, tgt, ns * fs, nt * ft, R0, t0, ev["nn_idx"], ev["nn_d2"], rr.MAX_DIST)
    assert np.array_equal(a["A"], b["A"]) and np.array_equal(a["g"], b["g"])
    # evaluation only; fewer than three inliers; three collinear ones; a NaN normal of an inlier
    o = gr.gicp_icp(src, tgt, ns, nt, R0, t0, rr.MAX_DIST, max_iterations=0)
    assert o["iterations"] == 0 and o["converged"] == 0 and np.array_equal(o["R"], R0)
    two = np.ascontiguousarray(tgt[:, :2])
    o = gr.gicp_icp(two, two, nt[:, :2], nt[:, :2], None, None, rr.MAX_DIST)
    assert o["inliers"] == 2 and o["iterations"] == 0 and o["converged"] == 0
    k = gr.collinear()
    ev = rr.evaluate(k["src"][0], k["tgt"][0], None, None, rr.MAX_DIST)
    assert ev["inliers"] == 3 and ev["nn_idx"].tolist() == [0, 1, 2]
    eye, zero = np.eye(3, dtype=np.float32), np.zeros(3, np.float32)
    n, A, g = gr.gicp_sums(k["src"][0], k["tgt"][0], k["nrm_t"][0], k["nrm_s"][0], eye, np.ones(3, bool))
    assert n == 3 and np.isfinite(A).all() and pr.singular(A)
    assert gr.gicp_step(k["src"][0], k["tgt"][0], k["nrm_s"][0], k["nrm_t"][0], eye, zero, ev["nn_idx"], ev["nn_d2"], rr.MAX_DIST) is None
    bad = ns.copy()
    bad[1, 17] = np.nan
    ev = rr.evaluate(src, tgt, R0, t0, rr.MAX_DIST)
    up = gr.gicp_step(src, tgt, bad, nt, R0, t0, ev["nn_idx"], ev["nn_d2"], rr.MAX_DIST)
    assert np.isnan(up["R"]).all() and np.isnan(up["t"]).all()


# ------------------------------------------------------------------------------------------------------------ the Python layer

def test_python_entry_points_refuse_what_they_cannot_run():
    import vcrnet_amd
    from vcrnet_amd import gicp, native
    a, b = torch.zeros(2, 3, 300), torch.zeros(2, 3, 410)
    with pytest.raises(native.VcrHipError, match="method must be one of"):
        vcrnet_amd.refine_registration(a, b, max_dist=0.1, method="gicp")
    for method in ("point_to_point", "point_to_plane"):
        with pytest.raises(native.VcrHipError, match="method='generalized' only"):
            vcrnet_amd.refine_registration(a, b, max_dist=0.1, method=method, src_normals=a)
        with pytest.raises(native.VcrHipError, match="method='generalized' only"):
            vcrnet_amd.refine_registration(a, b, max_dist=0.1, method=method, epsilon=1e-2)
    with pytest.raises(native.VcrHipError, match="point_to_plane' only"):        # (the message of before)
        vcrnet_amd.refine_registration(a, b, max_dist=0.1, tgt_normals=b)
    for eps in (0.0, -1e-3, 1.5, float("nan"), float("inf")):
        with pytest.raises(native.VcrHipError, match="epsilon must be finite, > 0 and <= 1"):
            vcrnet_amd.refine_registration(a, b, max_dist=0.1, method="generalized", epsilon=eps)
    with pytest.raises(native.VcrHipError, match="no CPU fallback"):
        vcrnet_amd.refine_registration(a, b, max_dist=0.1, method="generalized")
    with pytest.raises(native.VcrHipError, match=r"tgt_normals must be \[B, 3, Nt\]"):
        gicp.refine_gicp(a, b, a, a, max_dist=0.1)
    with pytest.raises(native.VcrHipError, match=r"src_normals must be \[B, 3, Ns\]"):
        gicp.refine_gicp(a, b, b, b, max_dist=0.1)
    with pytest.raises(native.VcrHipError, match="no CPU fallback"):
        gicp.refine_gicp(a, b, a, b, max_dist=0.1)
