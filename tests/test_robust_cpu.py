"""The robust point-to-plane refinement and the information matrix, without a GPU: the boundary of
include/robust/vcr_hip_robust.h (prototypes against vcrnet_amd.robust.SIGNATURES, the structs against gcc's layout, the exported
symbols), every argument error, the host-only form and workspace queries, the resource remarks of the new kernels, and the numpy
restatement (tests/robust_restated.py): the weights at their edges, the contaminated recipe on which the GPU's accuracy test
rests, and the matrix against Open3D's sum of G^T G."""
import ctypes
import inspect
import os
import re
import subprocess

import numpy as np
import pytest
import torch

import boundary
import plane_restated as pr
import refine_restated as rr
import robust_restated as ro

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INCLUDE = os.path.join(ROOT, "include")
HEADER = os.path.join(INCLUDE, "robust", "vcr_hip_robust.h")
EINVAL, EWORKSPACE, EUNSUPPORTED = -1, -2, -3
ENTRY_POINTS = {f"vcr_{what}{grid}_{tail}" for what in ("refine_robust", "information") for grid in ("", "_grid")
                for tail in ("workspace_bytes", "f32", "form")}
CASES = [(Nb, Ns, seed) for Nb, Ns in rr.SHAPES[:2] for seed in (5, 6)]


@pytest.fixture(scope="module")
def lib():
    import vcrnet_amd  # noqa: F401
    from vcrnet_amd import build, robust
    build.build()
    return robust.lib()


def test_signatures_match_the_header_and_the_library_exports_them(lib):
    import types
    from vcrnet_amd import gridnn, robust
    assert len(ENTRY_POINTS) == 12
    both = types.SimpleNamespace(SIGNATURES=robust.SIGNATURES, STRUCTS={**robust.STRUCTS, **gridnn.NEW_STRUCTS})
    boundary.check_signatures(HEADER, both, lib, ENTRY_POINTS)


def test_args_match_the_c_layout(tmp_path):
    import vcrnet_amd  # noqa: F401
    from vcrnet_amd import robust
    boundary.check_layout(HEADER, robust, tmp_path)


def test_the_other_boundaries_are_where_they_were(lib):
    """The two fits live beside the other headers, not in them: none mentions them, ABI 27, the same 51 prototypes;
    include/robust/ holds the one header, which enters the digest of refine_robust.o and of no other; the plane fit's fields
    lead the robust struct and vcr_refine_args' the information struct, at their offsets; refine_registration keeps its
    methods and its signature."""
    import vcrnet_amd
    from vcrnet_amd import build, colored, gicp, gridnn, native, plane, refine, robust
    assert os.listdir(os.path.join(INCLUDE, "robust")) == ["vcr_hip_robust.h"]
    for dirpath, _, files in os.walk(INCLUDE):
        for f in files:
            path = os.path.join(dirpath, f)
            if path != HEADER:
                text = open(path).read()
                assert "vcr_refine_robust" not in text and "vcr_information" not in text and "VCR_LOSS" not in text, path
    assert len(native.PUBLIC) == 51 and lib.vcr_abi_version() == native.ABI_VERSION == 27
    for other in (native, refine, plane, gicp, gridnn, colored):
        assert not set(robust.SIGNATURES) & set(other.SIGNATURES) and not set(robust.STRUCTS) & set(other.STRUCTS)
    assert build.ROBUST_HEADERS == [HEADER] and build.OWN_HEADERS["refine_robust.hip"] == [HEADER]
    assert [k for k, v in build.OWN_HEADERS.items() if HEADER in v] == ["refine_robust.hip"]
    flags = " ".join(build.FLAGS)
    hdrs = sorted(os.path.join(build.CSRC, f) for f in os.listdir(build.CSRC) if f.endswith(".h"))
    hdrs += (build.PUBLIC_HEADERS + build.LATER_HEADERS + build.OUTLIER_HEADERS + build.GICP_HEADERS + build.FPFH_HEADERS
             + build.MATCH_HEADERS + build.FGR_HEADERS + build.GRID_HEADERS + build.GRIDNN_HEADERS + build.VOXEL_SORT_HEADERS
             + build.RADIUS_HEADERS + build.ROWS_HEADERS + build.DBSCAN_HEADERS + build.SEGMENT_HEADERS + build.ORIENT_HEADERS
             + build.ISS_HEADERS + build.QUERY_HEADERS)
    assert HEADER not in hdrs
    sha = lambda name: open(os.path.join(build.OBJ, name + ".o.sha")).read()    # noqa: E731 (build() ran in the fixture)
    src = lambda name: os.path.join(build.CSRC, name + ".hip")                  # noqa: E731
    assert sha("refine_robust") == build._digest([src("refine_robust")] + hdrs + [HEADER], flags) != build._digest([src("refine_robust")] + hdrs, flags)
    for name in ("refine_plane", "refine_gicp", "refine", "normals", "nnscore", "gridnn"):
        assert sha(name) == build._digest([src(name)] + hdrs, flags), name
    for name in ("color_gradient", "refine_colored"):
        assert sha(name) == build._digest([src(name)] + hdrs + build.COLORED_HEADERS, flags), name
    names = [f[0] for f in robust.RefineRobustArgs._fields_]
    assert names == [f[0] for f in plane.RefinePlaneArgs._fields_] + ["loss", "k"]
    for name, _ in plane.RefinePlaneArgs._fields_:
        assert getattr(robust.RefineRobustArgs, name).offset == getattr(plane.RefinePlaneArgs, name).offset, name
    assert robust.RefineRobustArgs.loss.offset == ctypes.sizeof(plane.RefinePlaneArgs)
    assert robust.RefineRobustArgs.k.offset == ctypes.sizeof(plane.RefinePlaneArgs) + 4
    assert [f[0] for f in robust.InformationArgs._fields_] == [f[0] for f in refine.RefineArgs._fields_] + ["information"]
    for name, _ in refine.RefineArgs._fields_:
        assert getattr(robust.InformationArgs, name).offset == getattr(refine.RefineArgs, name).offset, name
    assert robust.InformationArgs.information.offset == ctypes.sizeof(refine.RefineArgs)
    text = open(os.path.join(build.CSRC, "refine_robust.hip")).read()
    assert "static_assert(offsetof(vcr_refine_robust_args, variant) == offsetof(vcr_refine_plane_args, variant)" in text
    assert refine.METHODS == ("point_to_point", "point_to_plane", "generalized")
    assert "loss" not in inspect.signature(vcrnet_amd.refine_registration).parameters
    assert {"refine_registration_robust", "information_matrix"} <= set(vcrnet_amd.__all__) and "robust" not in vcrnet_amd.__all__
    assert vcrnet_amd.refine_registration_robust is robust.refine_registration_robust
    assert vcrnet_amd.information_matrix is robust.information_matrix
    text = boundary.stripped(HEADER)
    for i, name in enumerate(("L2", "HUBER", "CAUCHY", "GM", "TUKEY")):
        assert re.search(r"#define VCR_LOSS_%s\s+%d\b" % (name, i), open(HEADER).read()), name
        assert robust.LOSSES[i] == ro.LOSSES[i] == name.lower()
    assert "VCR_LOSS_L1" not in text
    text = open(HEADER).read()
    assert "GEOMETRIC" in text and "never the weighted residual" in text and "L1 is not built" in text


def _args(B=2, Ns=1000, Nt=1500, max_dist=0.1, max_iterations=30, rel_fitness=1e-6, rel_rmse=1e-6, variant=0, loss=4, k=0.02):
    from vcrnet_amd import robust
    a = robust.RefineRobustArgs()
    a.src, a.tgt, a.R_out, a.t_out, a.fitness, a.rmse, a.tgt_normals = 0x1000, 0x2000, 0x3000, 0x4000, 0x5000, 0x6000, 0x7000   # (never dereferenced)
    a.B, a.Ns, a.Nt, a.max_dist, a.max_iterations, a.variant = B, Ns, Nt, max_dist, max_iterations, variant
    a.rel_fitness, a.rel_rmse, a.loss, a.k = rel_fitness, rel_rmse, loss, k
    return a


def _info(B=2, Ns=1000, Nt=1500, max_dist=0.1, max_iterations=0, variant=0, information=0x7000):
    from vcrnet_amd import robust
    a = robust.InformationArgs()
    a.src, a.tgt, a.R_out, a.t_out, a.fitness, a.rmse, a.information = 0x1000, 0x2000, 0x3000, 0x4000, 0x5000, 0x6000, information
    a.B, a.Ns, a.Nt, a.max_dist, a.max_iterations, a.variant = B, Ns, Nt, max_dist, max_iterations, variant
    return a


def _calls(lib, entry):
    from vcrnet_amd import gridnn
    g = gridnn.grid_args()
    fn = lambda tail: getattr(lib, f"vcr_{entry}{tail}")                                                   # noqa: E731
    f32 = lambda a, ws=0x10000, n=1 << 40: fn("_f32")(ctypes.byref(a), ws, n, None)                        # noqa: E731
    form = lambda a: fn("_form")(ctypes.byref(a), 256, None, None)                                         # noqa: E731
    size = lambda a: fn("_workspace_bytes")(ctypes.byref(a), 256)                                          # noqa: E731
    gf32 = lambda a: fn("_grid_f32")(ctypes.byref(a), ctypes.byref(g), 0x10000, 1 << 40, None)             # noqa: E731
    gform = lambda a: fn("_grid_form")(ctypes.byref(a), ctypes.byref(g), 256, None, None, None)            # noqa: E731
    gsize = lambda a: fn("_grid_workspace_bytes")(ctypes.byref(a), ctypes.byref(g), 256)                   # noqa: E731
    refused = lambda a, code: (f32(a) == code and form(a) == code and size(a) == 0                         # noqa: E731
                               and gf32(a) == code and gform(a) == code and gsize(a) == 0)
    return f32, form, size, gf32, gform, gsize, refused


def test_the_robust_fit_refuses_what_it_cannot_run_without_a_gpu(lib):
    from vcrnet_amd import refine, robust
    f32, form, size, gf32, gform, gsize, refused = _calls(lib, "refine_robust")
    assert lib.vcr_refine_robust_f32(None, 0x10000, 1 << 40, None) == EINVAL
    assert lib.vcr_refine_robust_form(None, 256, None, None) == EINVAL and lib.vcr_refine_robust_workspace_bytes(None, 256) == 0
    assert form(_args()) == 0 and size(_args()) > 0 and gform(_args()) == 0 and gsize(_args()) > size(_args())
    assert lib.vcr_refine_robust_grid_f32(ctypes.byref(_args()), None, 0x10000, 1 << 40, None) == EINVAL
    assert lib.vcr_refine_robust_grid_form(ctypes.byref(_args()), None, 256, None, None, None) == EINVAL
    assert lib.vcr_refine_robust_grid_workspace_bytes(ctypes.byref(_args()), None, 256) == 0
    nan, inf = float("nan"), float("inf")
    for loss in (-1, 5, 6, 1 << 20, -(1 << 31)):               # (5 would be an L1: not built)
        assert refused(_args(loss=loss), EINVAL), loss
    for loss in (1, 2, 3, 4):
        for k in (0.0, -0.0, -1e-3, nan, inf, -inf):
            assert refused(_args(loss=loss, k=k), EINVAL), (loss, k)
        for k in (1e-45, 1e-9, 0.02, 1e30, 3.4e38):
            assert form(_args(loss=loss, k=k)) == 0 and size(_args(loss=loss, k=k)) == size(_args()), (loss, k)
    for k in (0.0, -1.0, nan, inf, 0.02):                       # L2 does not read k
        assert form(_args(loss=0, k=k)) == 0 and gform(_args(loss=0, k=k)) == 0 and size(_args(loss=0, k=k)) == size(_args()), k
    for field in ("src", "tgt", "R_out", "t_out", "fitness", "rmse", "tgt_normals"):
        a = _args()
        setattr(a, field, None)
        assert refused(a, EINVAL), field
    for field in ("R", "t"):                                   # an initial pose is both or neither
        a = _args()
        setattr(a, field, 0x8000)
        assert refused(a, EINVAL), field
    for kw in (dict(Ns=0), dict(Nt=0), dict(B=0), dict(Ns=-3), dict(B=-1), dict(max_dist=-1e-3), dict(max_dist=nan), dict(max_dist=inf),
               dict(max_iterations=-1), dict(rel_fitness=-1e-9), dict(rel_fitness=nan), dict(rel_rmse=inf)):
        assert refused(_args(**kw), EINVAL), kw
    for kw in (dict(variant=3), dict(variant=-1), dict(variant=refine.variant(1, 129))):
        a = _args(**kw)
        assert f32(a) == EINVAL and form(a) == EINVAL and size(a) == 0 and gf32(a) == EINVAL, kw
    assert gf32(_args(variant=refine.variant(2))) == EINVAL      # (the scan's forms do not apply to the grid)
    for kw in (dict(max_dist=0.0), dict(max_iterations=0), dict(rel_fitness=0.0, rel_rmse=0.0), dict(max_iterations=refine.MAX_ITERATIONS)):
        assert form(_args(**kw)) == 0 and size(_args(**kw)) > 0, kw
    for kw in (dict(Ns=131073), dict(Nt=131073), dict(max_iterations=refine.MAX_ITERATIONS + 1)):
        assert refused(_args(**kw), EUNSUPPORTED), kw
    assert lib.vcr_refine_robust_form(ctypes.byref(_args()), -1, None, None) == EINVAL
    for bad in (0, robust.RefineRobustArgs.loss.offset, robust.RefineRobustArgs.k.offset, ctypes.sizeof(robust.RefineRobustArgs) + 8):
        a = _args()
        a.struct_bytes = bad
        assert refused(a, EINVAL), bad
    a = _args()
    need = lib.vcr_refine_robust_workspace_bytes(ctypes.byref(a), 0)
    assert need == size(a) > 0
    assert f32(a, ws=None) == EINVAL and f32(a, ws=0x10004) == EINVAL and f32(a, ws=0x10008) == EINVAL
    assert f32(a, n=need - 1) == EWORKSPACE and f32(a, n=0) == EWORKSPACE


def test_the_information_call_refuses_what_it_cannot_run_without_a_gpu(lib):
    from vcrnet_amd import refine, robust
    f32, form, size, gf32, gform, gsize, refused = _calls(lib, "information")
    assert lib.vcr_information_f32(None, 0x10000, 1 << 40, None) == EINVAL
    assert lib.vcr_information_form(None, 256, None, None) == EINVAL and lib.vcr_information_workspace_bytes(None, 256) == 0
    assert form(_info()) == 0 and size(_info()) > 0 and gform(_info()) == 0 and gsize(_info()) > size(_info())
    assert lib.vcr_information_grid_f32(ctypes.byref(_info()), None, 0x10000, 1 << 40, None) == EINVAL
    assert lib.vcr_information_grid_form(ctypes.byref(_info()), None, 256, None, None, None) == EINVAL
    assert lib.vcr_information_grid_workspace_bytes(ctypes.byref(_info()), None, 256) == 0
    for it in (1, 30, -1, refine.MAX_ITERATIONS + 1):           # the call is one round
        assert refused(_info(max_iterations=it), EINVAL), it
    assert refused(_info(information=None), EINVAL)
    for field in ("src", "tgt", "R_out", "t_out", "fitness", "rmse"):
        a = _info()
        setattr(a, field, None)
        assert refused(a, EINVAL), field
    for field in ("R", "t"):
        a = _info()
        setattr(a, field, 0x8000)
        assert refused(a, EINVAL), field
    nan, inf = float("nan"), float("inf")
    for kw in (dict(Ns=0), dict(Nt=0), dict(B=0), dict(B=-1), dict(max_dist=-1e-3), dict(max_dist=nan), dict(max_dist=inf)):
        assert refused(_info(**kw), EINVAL), kw
    for kw in (dict(Ns=131073), dict(Nt=131073)):
        assert refused(_info(**kw), EUNSUPPORTED), kw
    for kw in (dict(variant=3), dict(variant=-1)):
        a = _info(**kw)
        assert f32(a) == EINVAL and form(a) == EINVAL and size(a) == 0 and gf32(a) == EINVAL, kw
    assert gf32(_info(variant=refine.variant(2))) == EINVAL
    for bad in (0, robust.InformationArgs.variant.offset, robust.InformationArgs.information.offset, ctypes.sizeof(robust.InformationArgs) + 8):
        a = _info()
        a.struct_bytes = bad
        assert refused(a, EINVAL), bad
    a = _info()
    need = lib.vcr_information_workspace_bytes(ctypes.byref(a), 0)
    assert need == size(a) > 0
    assert f32(a, ws=None) == EINVAL and f32(a, ws=0x10004) == EINVAL
    assert f32(a, n=need - 1) == EWORKSPACE and f32(a, n=0) == EWORKSPACE


def test_the_forms_and_the_workspaces(lib):
    """The robust fit's are the plane fit's (the same search, V = 29); the information call's search is the point-to-point
    refinement's at max_iterations = 0, with a smaller partial (V = 11 against 16)."""
    from vcrnet_amd import gridnn, plane, refine, robust
    for B, Ns, Nt in ((1, 1, 1), (1, 5, 7), (16, 1024, 1024), (1, 131072, 131072), (3, 1137, 1500)):
        for v in (0, refine.variant(4), refine.variant(0, 7), refine.variant(2, 128)):
            for cu in (256, 1, 304):
                assert robust.refine_robust_form(B, Ns, Nt, cu_count=cu, variant=v) == plane.refine_plane_form(B, Ns, Nt, cu_count=cu, variant=v)
                q, s, size = robust.information_form(B, Ns, Nt, cu_count=cu, variant=v)
                q0, s0, size0 = refine.refine_form(B, Ns, Nt, cu_count=cu, variant=v, max_iterations=0)
                assert (q, s) == (q0, s0) and 0 < size <= size0
        for order in (0, 1, 2):
            assert robust.refine_robust_grid_form(B, Ns, Nt, order=order) == gridnn.refine_grid_form(B, Ns, Nt, order=order, method="point_to_plane")
    with pytest.raises(Exception):
        robust.refine_robust_form(1, 131073, 10)


def test_the_new_kernels_use_no_scratch(lib):
    from vcrnet_amd import build
    res = build.kernel_resources()
    names = list(res)
    dem = subprocess.run(["c++filt"], input="\n".join(names), capture_output=True, text=True, check=True).stdout.splitlines()
    short = lambda d: re.sub(r"^void ", "", d.replace("(anonymous namespace)::", "")).split("(")[0]       # noqa: E731
    mine = {short(d): res[n] for n, d in zip(names, dem) if res[n]["file"] == "refine_robust.hip"}
    assert set(mine) == ({f"robust_merge_kernel<{i}>" for i in range(5)}                     # one instantiation per loss
                         | {"robust_cloud_kernel", "info_merge_kernel", "info_cloud_kernel", "info_matrix_kernel"}), sorted(mine)
    for k, v in mine.items():
        assert v.get("scratch", 0) == 0 and v.get("vgpr_spill", 0) == 0 and v.get("sgpr_spill", 0) == 0, (k, v)
        assert v.get("agprs", 0) == 0, (k, v)
    plane_cloud = [v for n, v in res.items() if "plane_cloud_kernel" in n][0]
    cloud = mine["robust_cloud_kernel"]                           # plane_cloud_kernel's text
    assert (cloud["vgprs"], cloud["occupancy"], cloud["lds"]) == (plane_cloud["vgprs"], plane_cloud["occupancy"], plane_cloud["lds"])
    for i in range(5):
        assert mine[f"robust_merge_kernel<{i}>"]["occupancy"] >= 4, (i, mine[f"robust_merge_kernel<{i}>"])
    assert mine["info_merge_kernel"]["occupancy"] >= 4


# ------------------------------------------------------------------------------------------------------------ the restatement

def test_the_weights_at_their_edges():
    k32 = np.float32(0.02)
    k = np.float64(k32)
    up, down = np.nextafter(k, np.inf), np.nextafter(k, 0.0)
    for loss in ro.LOSSES:
        kk = k32 * k32 if loss == "gm" else k32
        w0 = ro.weight(loss, kk, 0.0)
        assert w0 == (np.float64(kk) / (np.float64(kk) * np.float64(kk)) if loss == "gm" else 1.0), loss          # GM: k / k^2
        r = np.asarray([-3 * k, -k, -0.5 * k, 0.0, 0.5 * k, k, 3 * k])
        w = ro.weight(loss, kk, r)
        assert np.array_equal(w, w[::-1]) and np.isfinite(w).all() and (w >= 0).all(), loss      # even in r
        assert (np.diff(w[3:]) <= 0).all(), loss                                     # and never growing with |r|
    assert np.array_equal(ro.weight("l2", 0.0, np.asarray([0.0, 1e30, -5.0])), np.ones(3))       # L2 does not read k
    # Huber: exactly 1 up to and AT |r| = k, k / |r| beyond
    assert ro.weight("huber", k32, k) == 1.0 and ro.weight("huber", k32, -k) == 1.0 and ro.weight("huber", k32, down) == 1.0
    assert ro.weight("huber", k32, up) == k / up < 1.0 and ro.weight("huber", k32, 4 * k) == 0.25
    assert (ro.weight("huber", 1e30, np.asarray([0.0, 1.0, -1e29])) == 1.0).all()
    # Tukey: exactly 0 AT |r| = k and beyond, (1 - u^2)^2 within
    assert ro.weight("tukey", k32, k) == 0.0 and ro.weight("tukey", k32, -k) == 0.0 and ro.weight("tukey", k32, up) == 0.0
    assert ro.weight("tukey", k32, 1e3) == 0.0 and 0.0 < ro.weight("tukey", k32, down) < 1e-30
    assert ro.weight("tukey", k32, 0.5 * k) == 0.5625
    assert not ro.weight("tukey", 1e-9, np.asarray([1e-8, -1e-3, 0.05])).any()
    # Cauchy and GM never reach zero
    assert ro.weight("cauchy", k32, k) == 0.5 and ro.weight("cauchy", k32, 3 * k) == 1.0 / (1.0 + 9.0)
    assert ro.weight("gm", k32, 0.1) == k / ((k + 0.1 * 0.1) * (k + 0.1 * 0.1)) > 0
    # the scale is the fp32 argument, widened
    assert ro.weight("cauchy", 0.01, 0.01) != 0.5 and ro.weight("cauchy", np.float32(0.01), np.float64(np.float32(0.01))) == 0.5
    # a lane that is no inlier: r = 0, a finite weight for every k > 0, the smallest fp32 included
    for loss in ro.LOSSES[1:]:
        for kk in (1e-45, 1e-30, 3.4e38):
            w = ro.weight(loss, kk, 0.0)
            assert np.isfinite(w) and w * 0.0 == 0.0, (loss, kk)


@pytest.fixture(scope="module")
def fits():
    """Per case of the recipe: the pair, and the restated least-squares, Cauchy and two-stage Tukey fits (20 updates each)."""
    return {(Nb, Ns, seed): ro.fits(seed, Nb, Ns) for Nb, Ns, seed in CASES}


def test_the_contaminated_recipe_is_the_issues(fits):
    for (Nb, Ns, seed), f in fits.items():
        c = f["c"]
        p = rr.pair(seed, Nb, Ns, "torus")
        assert c["src"].shape == (3, Ns + rr.FAR) and c["src"].dtype == np.float32 and np.array_equal(c["tgt"], p["tgt"])
        assert np.array_equal(c["R0"], p["R0"]) and np.array_equal(c["t0"], p["t0"]) and np.array_equal(c["clean"], p["src"])
        assert c["pushed"].sum() == round(0.25 * Ns) and not c["pushed"][Ns:].any()
        d = c["src"].astype(np.float64) - p["src"].astype(np.float64)
        assert not d[:, ~c["pushed"]].any()
        far = np.linalg.norm(d[:, c["pushed"]], axis=0)
        assert far.min() >= 0.03 - 1e-6 and far.max() <= 0.07 + 1e-6 < rr.MAX_DIST
        assert np.abs(d[:, c["pushed"]] / far - np.asarray([[0.6], [0.0], [0.8]])).max() <= 1e-5
        e0 = pr.pose_error(c["R0"], c["t0"], c["R"], c["t"])
        assert abs(e0[0] - np.deg2rad(6.0)) <= 1e-6 and abs(e0[1] - 0.04) <= 1e-6
        nrm = c["nrm"].astype(np.float64)
        assert np.abs(np.linalg.norm(nrm, axis=0) - 1).max() <= 1e-6
        # a clean source point is its twin under the planted pose
        q = (c["R"] @ p["src"][:, :Ns].astype(np.float64) + c["t"][:, None]) - c["tgt"][:, p["twin"]].astype(np.float64)
        assert np.abs(q).max() <= 1e-6


def test_the_robust_fits_beat_least_squares_on_the_restatement(fits):
    """The condition that makes the GPU's accuracy test meaningful: Cauchy (k = 0.01) from the recipe's start ends at most a
    third of the least-squares rotation AND translation errors, Tukey (k = 0.02) from the least-squares result at most a fifth.
    Measured on this restatement: least squares 3.6e-3 ... 1.8e-2 rad and 1.1e-2 ... 1.3e-2; Cauchy a sixth or less, Tukey a
    ninth or less.  (Tukey from the recipe's start instead ends 0.11 and 0.18 rad off on the two 700-point cases.)"""
    for (Nb, Ns, seed), f in fits.items():
        c = f["c"]
        err = lambda o: np.asarray(pr.pose_error(o["R"], o["t"], c["R"], c["t"]))    # noqa: E731
        ls, cauchy, tukey = err(f["ls"]), err(f["cauchy"]), err(f["tukey"])
        print(f"robust restated Nb {Nb} Ns {Ns} seed {seed}: least squares rot {ls[0]:.3e} t {ls[1]:.3e}  cauchy rot {cauchy[0]:.3e} "
              f"t {cauchy[1]:.3e}  tukey rot {tukey[0]:.3e} t {tukey[1]:.3e}")
        assert f["ls"]["iterations"] == f["cauchy"]["iterations"] == f["tukey"]["iterations"] == 20
        assert (cauchy <= ls / 3).all(), (Nb, Ns, seed, ls, cauchy)
        assert (tukey <= ls / 5).all(), (Nb, Ns, seed, ls, tukey)


def test_l2_and_a_wide_huber_are_the_plane_fit_and_the_stops(fits):
    c = fits[700, 300, 5]["c"]
    a = (c["src"], c["tgt"], c["nrm"])
    ev = rr.evaluate(c["src"], c["tgt"], c["R0"], c["t0"], rr.MAX_DIST)
    plain = pr.plane_step(*a, c["R0"], c["t0"], ev["nn_idx"], ev["nn_d2"], rr.MAX_DIST)
    for loss, k in (("l2", 0.0), ("huber", 1e30)):
        up = ro.robust_step(*a, c["R0"], c["t0"], ev["nn_idx"], ev["nn_d2"], rr.MAX_DIST, loss, k)
        assert up["n"] == plain["n"] and np.array_equal(up["A"], plain["A"]) and np.array_equal(up["g"], plain["g"]), loss
    for loss, k in (("huber", 0.01), ("cauchy", 0.01), ("gm", 4e-4), ("tukey", 0.02)):
        up = ro.robust_step(*a, c["R0"], c["t0"], ev["nn_idx"], ev["nn_d2"], rr.MAX_DIST, loss, k)
        assert up["n"] == plain["n"] and not np.array_equal(up["A"], plain["A"]) and np.array_equal(up["A"], up["A"].T), loss
        assert up["cond"] < 1e6, (loss, up["cond"])
    # every weight zero: A = 0, singular, the loop takes no update
    n, A, g = ro.robust_sums(np.zeros((3, 4), np.float32), np.ones((3, 4), np.float32), np.ones((3, 4), np.float32), np.ones(4, bool), "tukey", 1e-9)
    assert n == 4 and not A.any() and not g.any() and pr.singular(A)
    o = ro.robust_icp(*a, c["R0"], c["t0"], rr.MAX_DIST, "tukey", 1e-9)
    assert o["iterations"] == 0 and o["converged"] == 0 and o["inliers"] >= 6 and np.array_equal(o["R"], c["R0"])
    # fewer than six inliers; NaN normals
    few = ro.robust_icp(*a, c["R0"], c["t0"], 1e-4, "cauchy", 0.01)
    assert few["inliers"] < 6 and few["iterations"] == 0 and np.array_equal(few["t"], c["t0"])
    up = ro.robust_step(c["src"], c["tgt"], np.full_like(c["nrm"], np.nan), c["R0"], c["t0"], ev["nn_idx"], ev["nn_d2"], rr.MAX_DIST, "tukey", 0.02)
    assert np.isnan(up["R"]).all() and np.isnan(up["t"]).all()


def test_the_information_matrix_is_open3ds_sum_of_gtg(fits):
    """The nine ordered sums laid out as the header says against the plain float64 sum of G^T G over Open3D's three rows a
    pair: 1e-12 relative.  Symmetric, positive semi-definite, the inliers' count on the last three diagonal entries."""
    for (Nb, Ns, seed), f in fits.items():
        c = f["c"]
        ev = rr.evaluate(c["src"], c["tgt"], c["R0"], c["t0"], rr.MAX_DIST)
        I = ro.information(c["tgt"], ev["nn_idx"], ev["nn_d2"], rr.MAX_DIST)
        G = ro.information_gtg(c["tgt"], ev["nn_idx"], ev["nn_d2"], rr.MAX_DIST)
        assert I.shape == (6, 6) and I.dtype == np.float64
        assert np.abs(I - G).max() <= 1e-12 * np.abs(G).max(), (Nb, Ns, seed)
        assert np.array_equal(I, I.T) and I[3, 3] == I[4, 4] == I[5, 5] == ev["inliers"] and 6 <= ev["inliers"] < Ns + rr.FAR
        assert np.linalg.eigvalsh(I).min() > 0
        assert len(set(ev["nn_idx"][ev["nn_d2"] <= np.float32(rr.MAX_DIST) ** 2].tolist())) < ev["inliers"]   # (a target point counted twice)
    c = fits[700, 300, 5]["c"]
    ev = rr.evaluate(c["src"], c["tgt"], c["R0"], c["t0"], 0.0)
    assert ev["inliers"] == 0 and not ro.information(c["tgt"], ev["nn_idx"], ev["nn_d2"], 0.0).any()
    assert not ro.information(c["tgt"], np.full(5, -1), np.full(5, np.inf, np.float32), 0.1).any()


# ------------------------------------------------------------------------------------------------------------ the Python layer

def test_python_entry_points_refuse_what_they_cannot_run():
    import vcrnet_amd
    from vcrnet_amd import native, robust
    a, b = torch.zeros(2, 3, 300), torch.zeros(2, 3, 410)
    with pytest.raises(native.VcrHipError, match="no CPU fallback"):
        vcrnet_amd.refine_registration_robust(a, b, max_dist=0.1, k=0.02)
    with pytest.raises(native.VcrHipError, match="k has no default"):
        vcrnet_amd.refine_registration_robust(a, b, max_dist=0.1)
    for k in (0.0, -1.0, float("nan"), float("inf"), "wide"):
        with pytest.raises(native.VcrHipError, match="k must be finite and > 0"):
            vcrnet_amd.refine_registration_robust(a, b, max_dist=0.1, k=k)
    for loss in ("l1", "Tukey", 4, None):
        with pytest.raises(native.VcrHipError, match="loss must be one of"):
            vcrnet_amd.refine_registration_robust(a, b, max_dist=0.1, loss=loss, k=0.02)
    with pytest.raises(native.VcrHipError, match='search must be "scan" or "grid"'):
        vcrnet_amd.refine_registration_robust(a, b, max_dist=0.1, k=0.02, search="knn")
    with pytest.raises(native.VcrHipError, match="cell must be None"):
        vcrnet_amd.refine_registration_robust(a, b, max_dist=0.1, k=0.02, search="grid", cell=-1.0)
    with pytest.raises(native.VcrHipError, match=r"\[B, 3, N\] point cloud"):
        vcrnet_amd.refine_registration_robust(a[0], b, max_dist=0.1, k=0.02)
    with pytest.raises(native.VcrHipError, match="no CPU fallback"):
        vcrnet_amd.information_matrix(a, b, max_dist=0.1)
    with pytest.raises(native.VcrHipError, match='search must be "scan" or "grid"'):
        vcrnet_amd.information_matrix(a, b, max_dist=0.1, search="knn")
    with pytest.raises(native.VcrHipError, match="method must be one of"):
        vcrnet_amd.refine_registration(a, b, max_dist=0.1, method="robust")
    assert robust.LOSSES == ("l2", "huber", "cauchy", "gm", "tukey")
    sig = inspect.signature(vcrnet_amd.refine_registration_robust)
    assert list(sig.parameters) == ["src", "tgt", "R", "t", "max_dist", "loss", "k", "max_iterations", "rel_fitness", "rel_rmse",
                                    "want_nn", "tgt_normals", "normal_k", "centre", "search", "cell"]
    d = {k: v.default for k, v in sig.parameters.items() if v.default is not inspect.Parameter.empty}
    assert d == dict(R=None, t=None, max_dist=0.0, loss="tukey", k=None, max_iterations=30, rel_fitness=1e-6, rel_rmse=1e-6,
                     want_nn=False, tgt_normals=None, normal_k=20, centre=False, search="scan", cell=None)
    sig = inspect.signature(vcrnet_amd.information_matrix)
    assert list(sig.parameters) == ["src", "tgt", "R", "t", "max_dist", "search", "cell", "want_score"]
    d = {k: v.default for k, v in sig.parameters.items() if v.default is not inspect.Parameter.empty}
    assert d == dict(R=None, t=None, max_dist=0.0, search="scan", cell=None, want_score=False)
    doc = vcrnet_amd.refine_registration_robust.__doc__
    assert "Where it is weak" in doc and "lose the pose" in doc and "no honest default" in doc
