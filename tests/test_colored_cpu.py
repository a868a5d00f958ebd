"""The colored refinement, without a GPU: the boundary of include/colored/vcr_hip_colored.h (prototypes against
vcrnet_amd.colored.SIGNATURES, the structs against gcc's layout, the exported symbols), every argument error, the host-only form
and workspace queries, the resource remarks of the three new kernels, and the numpy restatement (tests/colored_restated.py):
against an independent solution, against the analytic colour gradient, and through the whole loop on the textured patch."""
import ctypes
import os
import subprocess
import types

import numpy as np
import pytest
import torch

import boundary
import colored_restated as cr
import nnscore_restated as nr
import plane_restated as pr
import refine_restated as rr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INCLUDE = os.path.join(ROOT, "include")
HEADER = os.path.join(INCLUDE, "colored", "vcr_hip_colored.h")
EINVAL, EWORKSPACE, EUNSUPPORTED = -1, -2, -3
ENTRY_POINTS = {"vcr_color_gradient_f32", "vcr_refine_colored_workspace_bytes", "vcr_refine_colored_f32", "vcr_refine_colored_form",
                "vcr_refine_colored_grid_workspace_bytes", "vcr_refine_colored_grid_f32", "vcr_refine_colored_grid_form"}
SEEDS = (1, 2, 3)


@pytest.fixture(scope="module")
def lib():
    import vcrnet_amd  # noqa: F401
    from vcrnet_amd import build, colored
    build.build()
    return colored.lib()


def test_signatures_match_the_header_and_the_library_exports_them(lib):
    from vcrnet_amd import colored, gridnn
    both = types.SimpleNamespace(SIGNATURES=colored.SIGNATURES, STRUCTS={**colored.STRUCTS, **gridnn.NEW_STRUCTS})
    boundary.check_signatures(HEADER, both, lib, ENTRY_POINTS)


def test_args_match_the_c_layout(tmp_path):
    import vcrnet_amd  # noqa: F401
    from vcrnet_amd import colored
    boundary.check_layout(HEADER, colored, tmp_path)


def test_the_other_boundaries_are_where_they_were(lib):
    """The fit lives beside the other headers, not in them: none mentions it, ABI 27, the same 51 prototypes; include/colored/
    holds the one header, which enters the digests of its own two objects and of no other; vcr_refine_args' fields lead the
    struct at their offsets; refine_registration keeps its three methods."""
    import vcrnet_amd
    from vcrnet_amd import build, colored, gicp, gridnn, native, plane, refine
    assert os.listdir(os.path.join(INCLUDE, "colored")) == ["vcr_hip_colored.h"]
    for dirpath, _, files in os.walk(INCLUDE):
        for f in files:
            path = os.path.join(dirpath, f)
            if path != HEADER:
                text = open(path).read()
                assert "vcr_refine_colored" not in text and "vcr_color_gradient" not in text, path
    assert len(native.PUBLIC) == 51 and lib.vcr_abi_version() == native.ABI_VERSION == 27
    for other in (native, refine, plane, gicp, gridnn):
        assert not set(colored.SIGNATURES) & set(other.SIGNATURES) and not set(colored.STRUCTS) & set(other.STRUCTS)
    assert build.COLORED_HEADERS == [HEADER]
    flags = " ".join(build.FLAGS)
    hdrs = sorted(os.path.join(build.CSRC, f) for f in os.listdir(build.CSRC) if f.endswith(".h"))
    hdrs += (build.PUBLIC_HEADERS + build.LATER_HEADERS + build.OUTLIER_HEADERS + build.GICP_HEADERS + build.FPFH_HEADERS
             + build.MATCH_HEADERS + build.FGR_HEADERS + build.GRID_HEADERS + build.GRIDNN_HEADERS + build.VOXEL_SORT_HEADERS
             + build.RADIUS_HEADERS + build.ROWS_HEADERS + build.DBSCAN_HEADERS + build.SEGMENT_HEADERS + build.ORIENT_HEADERS
             + build.ISS_HEADERS + build.QUERY_HEADERS)
    assert HEADER not in hdrs
    sha = lambda name: open(os.path.join(build.OBJ, name + ".o.sha")).read()    # noqa: E731 (build() ran in the fixture)
    src = lambda name: os.path.join(build.CSRC, name + ".hip")                  # noqa: E731
    for name in ("color_gradient", "refine_colored"):
        assert sha(name) == build._digest([src(name)] + hdrs + [HEADER], flags) != build._digest([src(name)] + hdrs, flags)
    for name in ("refine_plane", "refine_gicp", "normals"):
        assert sha(name) == build._digest([src(name)] + hdrs, flags), name
    names = [f[0] for f in colored.RefineColoredArgs._fields_]
    assert names == [f[0] for f in refine.RefineArgs._fields_] + ["tgt_normals", "tgt_gradient", "tgt_intensity", "src_intensity",
                                                                  "lambda_geometric"]
    for name, _ in refine.RefineArgs._fields_:
        assert getattr(colored.RefineColoredArgs, name).offset == getattr(refine.RefineArgs, name).offset, name
    assert colored.RefineColoredArgs.tgt_normals.offset == plane.RefinePlaneArgs.tgt_normals.offset == ctypes.sizeof(refine.RefineArgs)
    assert refine.METHODS == ("point_to_point", "point_to_plane", "generalized")
    assert {"compute_color_gradient", "refine_registration_colored"} <= set(vcrnet_amd.__all__)
    assert vcrnet_amd.refine_registration_colored is colored.refine_registration_colored
    assert vcrnet_amd.compute_color_gradient is colored.compute_color_gradient
    text = open(HEADER).read()
    assert "GEOMETRIC" in text and "joint residual" in text      # the header names the difference to Open3D's inlier_rmse


def _args(B=2, Ns=1000, Nt=1500, max_dist=0.1, max_iterations=30, rel_fitness=1e-6, rel_rmse=1e-6, variant=0, lam=0.968):
    from vcrnet_amd import colored
    a = colored.RefineColoredArgs()
    a.src, a.tgt, a.R_out, a.t_out, a.fitness, a.rmse = 0x1000, 0x2000, 0x3000, 0x4000, 0x5000, 0x6000       # (never dereferenced)
    a.tgt_normals, a.tgt_gradient, a.tgt_intensity, a.src_intensity = 0x7000, 0x9000, 0xa000, 0xb000
    a.B, a.Ns, a.Nt, a.max_dist, a.max_iterations, a.variant = B, Ns, Nt, max_dist, max_iterations, variant
    a.rel_fitness, a.rel_rmse, a.lambda_geometric = rel_fitness, rel_rmse, lam
    return a


def test_argument_errors_return_their_codes_without_a_gpu(lib):
    from vcrnet_amd import colored, gridnn, refine
    g = gridnn.grid_args()
    f32 = lambda a, ws=0x10000, n=1 << 40: lib.vcr_refine_colored_f32(ctypes.byref(a), ws, n, None)   # noqa: E731
    form = lambda a: lib.vcr_refine_colored_form(ctypes.byref(a), 256, None, None)                     # noqa: E731
    size = lambda a: lib.vcr_refine_colored_workspace_bytes(ctypes.byref(a), 256)                      # noqa: E731
    gf32 = lambda a: lib.vcr_refine_colored_grid_f32(ctypes.byref(a), ctypes.byref(g), 0x10000, 1 << 40, None)        # noqa: E731
    gform = lambda a: lib.vcr_refine_colored_grid_form(ctypes.byref(a), ctypes.byref(g), 256, None, None, None)       # noqa: E731
    gsize = lambda a: lib.vcr_refine_colored_grid_workspace_bytes(ctypes.byref(a), ctypes.byref(g), 256)              # noqa: E731
    refused = lambda a, code: (f32(a) == code and form(a) == code and size(a) == 0                                    # noqa: E731
                               and gf32(a) == code and gform(a) == code and gsize(a) == 0)
    assert lib.vcr_refine_colored_f32(None, 0x10000, 1 << 40, None) == EINVAL
    assert lib.vcr_refine_colored_form(None, 256, None, None) == EINVAL and lib.vcr_refine_colored_workspace_bytes(None, 256) == 0
    assert form(_args()) == 0 and size(_args()) > 0 and gform(_args()) == 0 and gsize(_args()) > size(_args())
    assert lib.vcr_refine_colored_grid_f32(ctypes.byref(_args()), None, 0x10000, 1 << 40, None) == EINVAL
    assert lib.vcr_refine_colored_grid_form(ctypes.byref(_args()), None, 256, None, None, None) == EINVAL
    assert lib.vcr_refine_colored_grid_workspace_bytes(ctypes.byref(_args()), None, 256) == 0
    for field in ("src", "tgt", "R_out", "t_out", "fitness", "rmse", "tgt_normals", "tgt_gradient", "tgt_intensity", "src_intensity"):
        a = _args()
        setattr(a, field, None)
        assert refused(a, EINVAL), field
    nan, inf = float("nan"), float("inf")
    for lam in (-1e-3, 1.0000001, 2.0, nan, inf, -inf):
        assert refused(_args(lam=lam), EINVAL), lam
    for lam in (0.0, -0.0, 1.0, 0.968, 1e-45):
        assert form(_args(lam=lam)) == 0 and size(_args(lam=lam)) == size(_args()), lam
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
    assert lib.vcr_refine_colored_form(ctypes.byref(_args()), -1, None, None) == EINVAL
    for bad in (0, colored.RefineColoredArgs.src_intensity.offset, colored.RefineColoredArgs.lambda_geometric.offset,
                ctypes.sizeof(colored.RefineColoredArgs) + 8):
        a = _args()
        a.struct_bytes = bad
        assert refused(a, EINVAL), bad
    a = _args()
    need = lib.vcr_refine_colored_workspace_bytes(ctypes.byref(a), 0)
    assert need == size(a) > 0
    assert f32(a, ws=None) == EINVAL and f32(a, ws=0x10004) == EINVAL and f32(a, ws=0x10008) == EINVAL
    assert f32(a, n=need - 1) == EWORKSPACE and f32(a, n=0) == EWORKSPACE


def _gradient_args(**kw):
    from vcrnet_amd import colored
    a = colored.ColorGradientArgs(xyz4=0x1000, idx=0x2000, B=2, N=300, k=20, normals=0x3000, intensity=0x4000, radius=0.0,
                                  gradient=0x5000)
    for k, v in kw.items():
        setattr(a, k, v)
    return a


def test_the_gradient_refuses_what_it_cannot_run(lib):
    from vcrnet_amd import colored
    call = lambda a: lib.vcr_color_gradient_f32(ctypes.byref(a), None)   # noqa: E731
    assert lib.vcr_color_gradient_f32(None, None) == EINVAL
    for field in ("xyz4", "idx", "normals", "intensity", "gradient"):
        assert call(_gradient_args(**{field: None})) == EINVAL, field
    for kw in (dict(B=0), dict(N=0), dict(k=0), dict(B=-1), dict(xyz4=0x1008), dict(radius=-1e-3), dict(radius=float("nan")),
               dict(radius=float("inf")), dict(struct_bytes=0), dict(struct_bytes=colored.ColorGradientArgs.gradient.offset),
               dict(struct_bytes=ctypes.sizeof(colored.ColorGradientArgs) + 8)):
        assert call(_gradient_args(**kw)) == EINVAL, kw
    for kw in (dict(k=63), dict(N=131073), dict(B=1 << 14, N=131072)):
        assert call(_gradient_args(**kw)) == EUNSUPPORTED, kw


def test_the_form_and_the_workspace_are_the_plane_fits(lib):
    from vcrnet_amd import colored, gridnn, plane, refine
    for B, Ns, Nt in ((1, 1, 1), (1, 5, 7), (16, 1024, 1024), (1, 131072, 131072), (3, 1137, 1500)):
        for v in (0, refine.variant(4), refine.variant(0, 7), refine.variant(2, 128)):
            for cu in (256, 1, 304):
                assert colored.refine_colored_form(B, Ns, Nt, cu_count=cu, variant=v) == plane.refine_plane_form(B, Ns, Nt, cu_count=cu, variant=v)
        for order in (0, 1, 2):
            assert colored.refine_colored_grid_form(B, Ns, Nt, order=order) == gridnn.refine_grid_form(B, Ns, Nt, order=order, method="point_to_plane")
    with pytest.raises(Exception):
        colored.refine_colored_form(1, 131073, 10)


def test_the_new_kernels_use_no_scratch(lib):
    from vcrnet_amd import build
    res = build.kernel_resources()
    names = list(res)
    dem = subprocess.run(["c++filt"], input="\n".join(names), capture_output=True, text=True, check=True).stdout.splitlines()
    mine = {d.replace("(anonymous namespace)::", "").split("(")[0]: res[n] for n, d in zip(names, dem)
            if res[n]["file"] in ("color_gradient.hip", "refine_colored.hip")}
    assert set(mine) == {"color_gradient_kernel", "colored_merge_kernel", "colored_cloud_kernel"}
    for k, v in mine.items():
        assert v.get("scratch", 0) == 0 and v.get("vgpr_spill", 0) == 0 and v.get("sgpr_spill", 0) == 0, (k, v)
        assert v.get("agprs", 0) == 0, (k, v)
    assert mine["color_gradient_kernel"]["lds"] == 0
    plane_cloud = [v for n, v in res.items() if "plane_cloud_kernel" in n][0]
    cloud = mine["colored_cloud_kernel"]                          # plane_cloud_kernel's text
    assert (cloud["vgprs"], cloud["occupancy"], cloud["lds"]) == (plane_cloud["vgprs"], plane_cloud["occupancy"], plane_cloud["lds"])
    assert mine["colored_merge_kernel"]["occupancy"] >= 4, mine["colored_merge_kernel"]


# ------------------------------------------------------------------------------------------------------------ the restatement

@pytest.fixture(scope="module")
def pairs():
    """Every cloud the loop tests run, with the restated gradient over the restatement's own neighbours."""
    out = {}
    for kind in cr.KINDS:
        for Nt, Ns in cr.SHAPES:
            for seed in SEEDS:
                p = cr.pair(kind, seed, Nt, Ns)
                idx = cr.neighbours(p["tgt"])
                g, x, cond, m = cr.gradient(p["tgt"], p["nrm_t"], p["I_t"], idx, want_cond=True)
                out[kind, Nt, Ns, seed] = dict(p, idx=idx, grad=g, grad64=x, cond=cond, m=m)
    return out


def test_the_recipe_is_the_issues(pairs):
    for (kind, Nt, Ns, seed), p in pairs.items():
        assert p["src"].shape == (3, Ns) and p["tgt"].shape == (3, Nt)
        e0 = pr.pose_error(p["R0"], p["t0"], p["R"], p["t"])
        assert abs(e0[0] - 3.49e-2) <= 1e-4 and abs(e0[1] - 3.61e-2) <= 1e-4, e0
        assert np.abs(np.linalg.norm(p["nrm_t"].astype(np.float64), axis=0) - 1).max() <= 1e-6
        back = p["R"].T @ (p["tgt"].astype(np.float64) - p["t"][:, None])
        assert np.abs(back[2] - cr.height(kind, back[0], back[1])).max() <= 1e-6
        moved = p["R"] @ p["src"].astype(np.float64) + p["t"][:, None]
        d = np.linalg.norm(moved[:, :, None] - p["tgt"].astype(np.float64)[:, None, :], axis=0).min(axis=1)
        assert d.min() > 0                                         # no source point is a target point


def test_the_gradient_recovers_the_analytic_one_in_the_tangent_plane(pairs):
    """On the flat patch, away from the rim (where a neighbourhood is one-sided), to the discretisation's error: the slope over
    twenty neighbours of a texture whose period is a dozen spacings.  Measured with this restatement, rms over the inner points
    of |g - grad I| (|grad I| is 1.4 in the mean): 0.243 - 0.250 at 700 points, 0.156 - 0.165 at 1500; held to twice that.
    Orthogonal to the normal to 1e-12 everywhere, on both patches; a second summation order (the rows reversed) moves no value
    by more than 2^-22 |x| + 64 cond(M) 2^-53, the bound the device is held to."""
    twice = {700: 0.50, 1500: 0.33}
    for (kind, Nt, Ns, seed), p in pairs.items():
        x, n = p["grad64"], p["nrm_t"].astype(np.float64)
        assert (p["m"] == cr.K).all() and np.isfinite(p["cond"]).all()
        assert np.abs((x * n).sum(0)).max() <= 1e-12, (kind, Nt, seed)
        inner = (np.abs(p["uv_t"] - 0.5) <= 0.4).all(0)
        err = np.linalg.norm(x - p["grad_t"], axis=0)
        rms = np.sqrt((err[inner] ** 2).mean())
        assert rms <= twice[Nt], (kind, Nt, seed, rms)
        assert rms <= 0.2 * np.linalg.norm(p["grad_t"], axis=0).mean() + 0.1
        _, x2, _, _ = cr.gradient(p["tgt"], p["nrm_t"], p["I_t"], p["idx"][:, ::-1], want_cond=True)
        bound = 2.0 ** -22 * np.abs(x).max(0) + 64 * p["cond"] * 2.0 ** -53
        assert (np.abs(x - x2).max(0) <= bound).all()
        assert p["cond"].max() <= 1e6


def test_the_gradient_skips_what_the_header_says():
    p = cr.pair("bowl", 1, 300, 10)
    x, nrm, I = p["tgt"], p["nrm_t"], p["I_t"]
    idx = cr.neighbours(x, 8)
    base = cr.gradient(x, nrm, I, idx)
    # entries outside [0, N), the point itself and nothing else: the same sums
    own = np.arange(300)[:, None]
    padded = np.concatenate([np.full((300, 1), -1), idx[:, :4], own, np.full((300, 1), 300), idx[:, 4:], np.full((300, 1), 1 << 30)], axis=1)
    assert np.array_equal(cr.gradient(x, nrm, I, padded), base)
    # a repeated entry counts twice
    twice = np.concatenate([idx, idx[:, :1]], axis=1)
    assert not np.array_equal(cr.gradient(x, nrm, I, twice), base) and (cr.gradient_system(x, nrm, I, twice)[2] == 9).all()
    # m < 3: an exact zero; the radius drops the far part of a row
    assert not cr.gradient(x, nrm, I, idx[:, :2]).any() and cr.gradient(x, nrm, I, idx[:, :3]).any()
    d = np.linalg.norm(x[:, idx[:, 4]].astype(np.float64) - x.astype(np.float64), axis=0)
    r = float(np.median(d))
    m = cr.gradient_system(x, nrm, I, idx, r)[2]
    assert m.min() < 3 <= m.max() < 8 or (m.min() < 8 and m.max() == 8)
    g = cr.gradient(x, nrm, I, idx, r)
    assert not g[:, m < 3].any() and g[:, m >= 3].any()
    # a NaN intensity stays in the rows that hold it: those are zero, the others keep their bits
    bad = I.copy()
    bad[17] = np.nan
    g = cr.gradient(x, nrm, bad, idx)
    holds = (idx == 17).any(1) | (np.arange(300) == 17)
    assert not g[:, holds].any() and np.array_equal(g[:, ~holds], base[:, ~holds]) and holds.sum() > 1
    # collinear neighbours: singular
    line = np.stack([np.linspace(0, 1, 9), np.zeros(9), np.zeros(9)]).astype(np.float32)
    up = np.tile(np.asarray([[0], [0], [1]], np.float32), (1, 9))
    assert not cr.gradient(line, up, np.linspace(0, 1, 9).astype(np.float32), cr.neighbours(line, 4)).any()


def _first_round(p):
    ev = rr.evaluate(p["src"], p["tgt"], p["R0"], p["t0"], cr.MAX_DIST)
    return cr._lanes(p, p["R0"], p["t0"], ev["nn_idx"], ev["nn_d2"], cr.MAX_DIST), ev


def test_the_normal_equations_against_an_independent_solution(pairs):
    """x of the header's sums against numpy.linalg.lstsq on the stacked residual rows, whose Jacobian is taken by central
    differences of the residuals AS DEFINED (the photometric one read at the foot of the moved point on the neighbour's tangent
    plane): the same x, and J_G, J_I are the derivatives of r_G, r_I."""
    for key, p in pairs.items():
        if key[3] != 1:
            continue
        lanes, ev = _first_round(p)
        n, A, g = cr.colored_sums(*lanes)
        assert n == ev["inliers"] >= 6 and not pr.singular(A) and np.array_equal(A, A.T)
        x1 = np.linalg.solve(A, -g)
        x2 = cr.independent_x(*lanes)
        assert np.abs(x1 - x2).max() <= 1e-7 * (1 + np.abs(x1).max()), (key, x1, x2)
        inl = lanes[6]
        at = np.flatnonzero(inl)
        a = [np.asarray(v, np.float64)[..., at] for v in lanes[:6]]
        JG, rG, JI, rI = cr.colored_terms(*lanes)
        r0 = cr.residuals(np.zeros(6), *a)
        assert np.abs(r0[0] - rG[at]).max() <= 1e-12 and np.abs(r0[1] - rI[at]).max() <= 1e-12
        for k in range(6):
            e = np.zeros(6)
            e[k] = 1e-6
            plus, minus = cr.residuals(e, *a), cr.residuals(-e, *a)
            assert np.abs((plus[0] - minus[0]) / 2e-6 - JG[k][at]).max() <= 1e-8, (key, k)
            assert np.abs((plus[1] - minus[1]) / 2e-6 - JI[k][at]).max() <= 1e-7, (key, k)
        cond = np.linalg.cond(A)
        assert cond <= 1e6, (key, cond)


def test_cond_of_the_first_round_under_the_planted_pose(pairs):
    """cond(A) is a property of the frame: about 6e2 - 3e3 at the start AND under the planted pose of every recipe (the patch
    lies within 0.9 of the origin in both frames); the one-update bound of the GPU tests takes cond(A) <= 1e6."""
    for key, p in pairs.items():
        R32, t32 = p["R"].astype(np.float32), p["t"].astype(np.float32)
        ev = rr.evaluate(p["src"], p["tgt"], R32, t32, cr.MAX_DIST)
        up = cr.colored_step(p, R32, t32, ev["nn_idx"], ev["nn_d2"], cr.MAX_DIST)
        assert up is not None and 1e2 <= up["cond"] <= 1e4, (key, up["cond"])


def test_at_lambda_one_the_sums_are_the_plane_fits_and_lanes_without_a_partner_add_zeros(pairs):
    p = pairs["bowl", 700, 300, 1]
    lanes, ev = _first_round(p)
    n, A, g = cr.colored_sums(*lanes, lam=1.0)
    n_p, A_p, g_p = pr.plane_sums(lanes[0], lanes[1], lanes[2], lanes[6])
    assert n == n_p and np.array_equal(A, A_p) and np.array_equal(g, g_p)
    n_c, A_c, g_c = cr.colored_sums(*lanes)
    assert not np.array_equal(A_c, A_p)
    # far source points behind the cloud, with any colour: the same bits
    rs = np.random.RandomState(5)
    for extra in (200, 212 + 256):
        far = rs.uniform(2.0, 3.0, (3, extra)).astype(np.float32)
        q = dict(p, src=np.concatenate([p["src"], far], axis=1), I_s=np.concatenate([p["I_s"], rs.normal(size=extra).astype(np.float32)]))
        ev2 = rr.evaluate(q["src"], q["tgt"], q["R0"], q["t0"], cr.MAX_DIST)
        assert ev2["inliers"] == n
        n2, A2, g2 = cr.colored_sums(*cr._lanes(q, q["R0"], q["t0"], ev2["nn_idx"], ev2["nn_d2"], cr.MAX_DIST))
        assert n2 == n and np.array_equal(A2, A_c) and np.array_equal(g2, g_c), extra


def test_the_restated_loop_takes_the_slide_back_where_point_to_plane_cannot(pairs):
    """From 3.49e-2 rad and 3.61e-2: the colored loop converges in 2 to 6 updates to within 1.1e-3 rad and 9.1e-4 -- a
    thirtieth of the start -- on both patches (at 1500 / 900 points 3.4e-4 and 2.7e-4).  Point to plane takes no update on the
    flat patch (its system is singular) and ends 4e-3 to 1.7e-2 off in translation on the bowl."""
    for (kind, Nt, Ns, seed), p in pairs.items():
        o = cr.colored_icp(p, p["R0"], p["t0"])
        e = pr.pose_error(o["R"], o["t"], p["R"], p["t"])
        e0 = pr.pose_error(p["R0"], p["t0"], p["R"], p["t"])
        assert o["converged"] == 1 and 2 <= o["iterations"] <= 6, (kind, Nt, seed, o["iterations"])
        assert e[0] <= e0[0] / 30 and e[1] <= e0[1] / 30, (kind, Nt, seed, e)
        if Nt == 1500:
            assert e[0] <= 4e-4 and e[1] <= 3e-4, (kind, seed, e)
        pl = pr.plane_icp(p["src"], p["tgt"], p["nrm_t"], p["R0"], p["t0"], cr.MAX_DIST)
        ep = pr.pose_error(pl["R"], pl["t"], p["R"], p["t"])
        if kind == "flat":
            assert pl["iterations"] == 0 and ep == e0
        else:
            assert pl["iterations"] >= 2 and ep[1] >= 4e-3 and ep[1] >= 5 * e[1], (Nt, seed, ep, e)


def test_the_stops_of_the_restatement(pairs):
    p = pairs["flat", 700, 300, 1]
    ev = rr.evaluate(p["src"], p["tgt"], p["R0"], p["t0"], cr.MAX_DIST)
    # one colour on a plane: singular
    flat = dict(p, I_t=np.full_like(p["I_t"], 0.5), I_s=np.full_like(p["I_s"], 0.5), grad=np.zeros_like(p["grad"]))
    assert cr.colored_step(flat, p["R0"], p["t0"], ev["nn_idx"], ev["nn_d2"], cr.MAX_DIST) is None
    # fewer than six inliers
    few = cr.colored_icp(p, p["R0"], p["t0"], max_dist=1e-4)
    assert few["inliers"] < 6 and few["iterations"] == 0 and np.array_equal(few["R"], p["R0"])
    # a NaN colour of an inlier: a NaN step
    bad = dict(p, I_s=p["I_s"].copy())
    bad["I_s"][int(np.flatnonzero(ev["nn_d2"] <= np.float32(cr.MAX_DIST) ** 2)[3])] = np.nan
    up = cr.colored_step(bad, p["R0"], p["t0"], ev["nn_idx"], ev["nn_d2"], cr.MAX_DIST)
    assert np.isnan(up["R"]).all() and np.isnan(up["t"]).all()
    # the tiny case: every point an inlier, a well-conditioned system
    for Ns in (6, 5):
        c = cr.tiny(Ns=Ns)
        one = cr.cloud(c, 0)
        assert one["src"].shape == (3, Ns) and one["tgt"].shape == (3, 7)
        ev = rr.evaluate(one["src"], one["tgt"], c["R0"][0], c["t0"][0], cr.MAX_DIST)
        up = cr.colored_step(one, c["R0"][0], c["t0"][0], ev["nn_idx"], ev["nn_d2"], cr.MAX_DIST)
        assert ev["inliers"] == Ns and ev["nn_idx"].tolist() == list(range(Ns))
        if Ns == 5:
            assert up is None                                     # five pairs: one short of six
        else:
            assert up["n"] == 6 and up["cond"] <= 1e6, up["cond"]


# ------------------------------------------------------------------------------------------------------------ the Python layer

def test_python_entry_points_refuse_what_they_cannot_run():
    import vcrnet_amd
    from vcrnet_amd import colored, native
    a, b = torch.zeros(2, 3, 300), torch.zeros(2, 3, 410)
    ca, cb = torch.zeros(2, 3, 300), torch.zeros(2, 410)
    with pytest.raises(native.VcrHipError, match="no CPU fallback"):
        vcrnet_amd.refine_registration_colored(a, b, ca, cb, max_dist=0.1)
    for lam in (-0.1, 1.5, float("nan"), float("inf")):
        with pytest.raises(native.VcrHipError, match=r"lambda_geometric must be finite and in \[0, 1\]"):
            vcrnet_amd.refine_registration_colored(a, b, ca, cb, max_dist=0.1, lambda_geometric=lam)
    with pytest.raises(native.VcrHipError, match='search must be "scan" or "grid"'):
        vcrnet_amd.refine_registration_colored(a, b, ca, cb, max_dist=0.1, search="knn")
    with pytest.raises(native.VcrHipError, match="cell must be None"):
        vcrnet_amd.refine_registration_colored(a, b, ca, cb, max_dist=0.1, search="grid", cell=-1.0)
    with pytest.raises(native.VcrHipError, match=r"\[B, 3, N\] point cloud"):
        vcrnet_amd.refine_registration_colored(a[0], b, ca, cb, max_dist=0.1)
    with pytest.raises(native.VcrHipError, match="no CPU fallback"):
        vcrnet_amd.compute_color_gradient(a, a, ca)
    with pytest.raises(native.VcrHipError, match='search must be "knn" or "grid"'):
        vcrnet_amd.compute_color_gradient(a, a, ca, search="scan")
    with pytest.raises(native.VcrHipError, match="radius must be None or finite and > 0"):
        vcrnet_amd.compute_color_gradient(a, a, ca, radius=0.0)
    with pytest.raises(native.VcrHipError, match="method must be one of"):
        vcrnet_amd.refine_registration(a, b, max_dist=0.1, method="colored")
    assert colored.LAMBDA_GEOMETRIC == 0.968
    import inspect
    sig = inspect.signature(vcrnet_amd.refine_registration_colored)
    assert list(sig.parameters) == ["src", "tgt", "src_colors", "tgt_colors", "R", "t", "max_dist", "max_iterations", "rel_fitness",
                                    "rel_rmse", "lambda_geometric", "tgt_normals", "normal_k", "gradient_k", "gradient_radius",
                                    "tgt_gradient", "want_nn", "centre", "search", "cell"]
    d = {k: v.default for k, v in sig.parameters.items() if v.default is not inspect.Parameter.empty}
    assert d == dict(R=None, t=None, max_dist=0.0, max_iterations=30, rel_fitness=1e-6, rel_rmse=1e-6, lambda_geometric=0.968,
                     tgt_normals=None, normal_k=20, gradient_k=20, gradient_radius=None, tgt_gradient=None, want_nn=False,
                     centre=False, search="scan", cell=None)
    sig = inspect.signature(vcrnet_amd.compute_color_gradient)
    assert list(sig.parameters) == ["xyz", "normals", "colors", "k", "radius", "search", "idx"]
