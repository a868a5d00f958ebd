"""Pose-graph optimisation without a GPU: the boundary of include/posegraph/vcr_hip_posegraph.h (prototypes against
vcrnet_amd.posegraph.SIGNATURES, the struct against gcc's layout, the exported symbols), every argument error on the host, the
form and workspace queries, the resource remarks of the kernel, and the numpy restatement (tests/posegraph_restated.py) against
itself and against ground truth: the Jacobians against finite differences, vec6 as the inverse of pl_euler, the closed-form line
process, and the ring recipe on which the GPU tests rest."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest
import torch

import boundary
import posegraph_restated as pgr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INCLUDE = os.path.join(ROOT, "include")
HEADER = os.path.join(INCLUDE, "posegraph", "vcr_hip_posegraph.h")
EINVAL, EWORKSPACE, EUNSUPPORTED = -1, -2, -3
ENTRY_POINTS = {"vcr_posegraph_optimize_workspace_bytes", "vcr_posegraph_optimize_f64", "vcr_posegraph_optimize_form",
                "vcr_posegraph_check_edges"}
EPS = 2.0 ** -53


def _emit(line, first=[True]):
    print(line)
    out = os.environ.get("VCR_LEDGER_DIR", "")
    if os.path.isdir(out):
        with open(os.path.join(out, "posegraph_ledger_cpu.txt"), "w" if first[0] else "a") as f:
            f.write(line + "\n")
        first[0] = False


@pytest.fixture(scope="module")
def lib():
    import vcrnet_amd  # noqa: F401
    from vcrnet_amd import build, posegraph
    build.build()
    return posegraph.lib()


def test_signatures_match_the_header_and_the_library_exports_them(lib):
    from vcrnet_amd import posegraph
    boundary.check_signatures(HEADER, posegraph, lib, ENTRY_POINTS)


def test_args_match_the_c_layout(tmp_path):
    import vcrnet_amd  # noqa: F401
    from vcrnet_amd import posegraph
    boundary.check_layout(HEADER, posegraph, tmp_path)


def test_the_other_boundaries_are_where_they_were(lib):
    """The optimiser lives beside the other headers, not in them: none mentions it, ABI 27, the same 51 prototypes;
    include/posegraph/ holds the one header, which enters the digest of posegraph.o and of no other."""
    import vcrnet_amd
    from vcrnet_amd import build, native, posegraph, refine, robust
    assert os.listdir(os.path.join(INCLUDE, "posegraph")) == ["vcr_hip_posegraph.h"]
    for dirpath, _, files in os.walk(INCLUDE):
        for f in files:
            path = os.path.join(dirpath, f)
            if path != HEADER:
                text = open(path).read()
                assert "vcr_posegraph" not in text and "VCR_POSEGRAPH" not in text, path
    assert len(native.PUBLIC) == 51 and lib.vcr_abi_version() == native.ABI_VERSION == 27
    for other in (native, refine, robust):
        assert not set(posegraph.SIGNATURES) & set(other.SIGNATURES) and not set(posegraph.STRUCTS) & set(other.STRUCTS)
    assert build.POSEGRAPH_HEADERS == [HEADER] and build.OWN_HEADERS["posegraph.hip"] == [HEADER]
    assert [k for k, v in build.OWN_HEADERS.items() if HEADER in v] == ["posegraph.hip"]
    flags = " ".join(build.FLAGS)
    hdrs = sorted(os.path.join(build.CSRC, f) for f in os.listdir(build.CSRC) if f.endswith(".h"))
    hdrs += (build.PUBLIC_HEADERS + build.LATER_HEADERS + build.OUTLIER_HEADERS + build.GICP_HEADERS + build.FPFH_HEADERS
             + build.MATCH_HEADERS + build.FGR_HEADERS + build.GRID_HEADERS + build.GRIDNN_HEADERS + build.VOXEL_SORT_HEADERS
             + build.RADIUS_HEADERS + build.ROWS_HEADERS + build.DBSCAN_HEADERS + build.SEGMENT_HEADERS + build.ORIENT_HEADERS
             + build.ISS_HEADERS + build.QUERY_HEADERS)
    assert HEADER not in hdrs
    sha = lambda name: open(os.path.join(build.OBJ, name + ".o.sha")).read()    # noqa: E731 (build() ran in the fixture)
    src = lambda name: os.path.join(build.CSRC, name + ".hip")                  # noqa: E731
    assert sha("posegraph") == build._digest([src("posegraph")] + hdrs + [HEADER], flags) != build._digest([src("posegraph")] + hdrs, flags)
    for name in ("fgr", "refine_plane", "refine", "nnscore", "forward"):
        assert sha(name) == build._digest([src(name)] + hdrs, flags), name
    assert sha("refine_robust") == build._digest([src("refine_robust")] + hdrs + build.ROBUST_HEADERS, flags)
    text = open(src("posegraph")).read()
    assert '#include "refine_solve6.h"' in text and "atomic" not in text.replace("no atomic", "")
    assert {"optimize_pose_graph", "pose_graph_from_clouds", "register_multiway"} <= set(vcrnet_amd.__all__)
    assert "posegraph" not in vcrnet_amd.__all__
    for name in ("optimize_pose_graph", "pose_graph_from_clouds", "register_multiway"):
        assert getattr(vcrnet_amd, name) is getattr(posegraph, name)
    assert posegraph.CRITERIA == pgr.CRITERIA
    text = open(HEADER).read()
    assert "upper_scale_factor is taken and NOT used" in text and "ASCENDING EDGE INDEX" in text
    for name, value in (("MAX_NODES", 128), ("MAX_EDGES", 65536), ("MAX_TRIALS", 4096), ("FORM_LDS", 1), ("FORM_GLOBAL", 2)):
        assert re.search(r"#define VCR_POSEGRAPH_%s\s+%d\b" % (name, value), text) and getattr(posegraph, name) == value, name


def _calls(lib):
    f64 = lambda a, ws=0x10000, n=1 << 40: lib.vcr_posegraph_optimize_f64(ctypes.byref(a), ws, n, None)      # noqa: E731
    form = lambda a: lib.vcr_posegraph_optimize_form(ctypes.byref(a), 256, None, None)                        # noqa: E731
    size = lambda a: lib.vcr_posegraph_optimize_workspace_bytes(ctypes.byref(a), 256)                         # noqa: E731
    refused = lambda a, code: f64(a) == code and form(a) == code and size(a) == 0                             # noqa: E731
    return f64, form, size, refused


def test_the_entry_points_refuse_what_they_cannot_run_without_a_gpu(lib):
    from vcrnet_amd import posegraph
    A = lambda **kw: posegraph.form_args(kw.pop("G", 2), kw.pop("K", 8), kw.pop("E", 14), **kw)               # noqa: E731
    f64, form, size, refused = _calls(lib)
    assert lib.vcr_posegraph_optimize_f64(None, 0x10000, 1 << 40, None) == EINVAL
    assert lib.vcr_posegraph_optimize_form(None, 256, None, None) == EINVAL and lib.vcr_posegraph_optimize_workspace_bytes(None, 256) == 0
    assert form(A()) == 0 and size(A()) > 0
    nan, inf = float("nan"), float("inf")
    for field in ("R", "t", "src", "dst", "R_edge", "t_edge", "information", "uncertain", "R_out", "t_out", "weight", "kept", "residual",
                  "iterations", "converged"):
        a = A()
        setattr(a, field, None)
        assert refused(a, EINVAL), field
    a = A(E=0)                                                # without edge slots the edge arrays may be missing
    for field in ("src", "dst", "R_edge", "t_edge", "information", "uncertain", "weight", "kept"):
        setattr(a, field, None)
    assert form(a) == 0 and size(a) > 0
    for kw in (dict(G=0), dict(G=-1), dict(K=0), dict(K=-2), dict(E=-1), dict(anchor=-1), dict(anchor=8), dict(max_correspondence_distance=-1e-3),
               dict(max_correspondence_distance=nan), dict(max_correspondence_distance=inf), dict(edge_prune_threshold=-0.1),
               dict(edge_prune_threshold=nan), dict(max_iteration=-1), dict(max_iteration_lm=-1), dict(max_iteration=4097, max_iteration_lm=0),
               dict(max_iteration=0, max_iteration_lm=4097), dict(max_iteration=65, max_iteration_lm=64), dict(max_iteration=205, max_iteration_lm=20),
               dict(min_relative_increment=-1e-9), dict(min_relative_increment=nan), dict(min_relative_residual_increment=nan),
               dict(min_right_term=-1.0), dict(min_residual=nan), dict(lower_scale_factor=0.0), dict(lower_scale_factor=nan),
               dict(lower_scale_factor=inf), dict(upper_scale_factor=-1.0), dict(upper_scale_factor=inf), dict(variant=-1), dict(variant=3)):
        assert refused(A(**kw), EINVAL), kw
    for kw in (dict(max_iteration=64, max_iteration_lm=64), dict(max_iteration=4096, max_iteration_lm=1), dict(max_iteration=0),
               dict(max_correspondence_distance=0.0), dict(edge_prune_threshold=0.0), dict(min_residual=inf), dict(anchor=7), dict(prune=0),
               dict(K=1, E=0), dict(K=128, E=65536, G=1), dict(variant=1), dict(variant=2)):
        assert form(A(**kw)) == 0 and size(A(**kw)) > 0, kw
    for kw in (dict(K=129), dict(E=65537), dict(G=1 << 15, E=65536), dict(G=1 << 16, E=32768)):
        assert refused(A(**kw), EUNSUPPORTED), kw
    assert lib.vcr_posegraph_optimize_form(ctypes.byref(A()), -1, None, None) == EINVAL
    for bad in (0, posegraph.PosegraphArgs.converged.offset, ctypes.sizeof(posegraph.PosegraphArgs) + 8):
        a = A()
        a.struct_bytes = bad
        assert refused(a, EINVAL), bad
    a = A()
    a.struct_bytes = posegraph.PosegraphArgs.trials.offset   # a caller built before the optional outputs
    assert form(a) == 0 and size(a) == size(A())
    a = A()
    need = lib.vcr_posegraph_optimize_workspace_bytes(ctypes.byref(a), 0)
    assert need == size(a) > 0
    assert f64(a, ws=None) == EINVAL and f64(a, ws=0x10004) == EINVAL and f64(a, ws=0x10008) == EINVAL
    assert f64(a, n=need - 1) == EWORKSPACE and f64(a, n=0) == EWORKSPACE


def test_edges_are_checked_on_the_host(lib):
    from vcrnet_amd import posegraph
    from vcrnet_amd.native import VcrHipError
    ip = ctypes.POINTER(ctypes.c_int)
    def check(src, dst, G, K, E):
        s, d = (ctypes.c_int * len(src))(*src), (ctypes.c_int * len(dst))(*dst)
        return lib.vcr_posegraph_check_edges(ctypes.cast(s, ip), ctypes.cast(d, ip), G, K, E)
    assert check([0, 1, -1, 2], [1, 2, 99, 0], 1, 3, 4) == 0                  # a blank's dst is not looked at
    assert check([0, 1, -1, 2], [1, 2, 99, 0], 2, 3, 2) == 0
    for src, dst in (([0, 3], [1, 0]), ([0, 1], [1, 3]), ([0, 1], [1, 1]), ([0, 1], [1, -1]), ([0, 1 << 30], [1, 0])):
        assert check(src, dst, 1, 3, 2) == EINVAL, (src, dst)
    assert lib.vcr_posegraph_check_edges(None, None, 1, 3, 2) == EINVAL and lib.vcr_posegraph_check_edges(None, None, 1, 3, 0) == 0
    assert check([0], [1], 0, 3, 1) == EINVAL and check([0], [1], 1, 0, 1) == EINVAL and check([0], [1], 1, 3, -1) == EINVAL
    s, d = posegraph.check_edges([0, -1, 2], [1, 5, 0], 3)
    assert s.dtype == d.dtype == torch.int32 and s.tolist() == [0, -1, 2]
    for src, dst in (([0, 3], [1, 0]), ([0, 1], [1, 1]), ([[0, 1]], [[1, 7]]), ([0, 1], [1]), (np.zeros((1, 2, 2), int), np.zeros((1, 2, 2), int))):
        with pytest.raises(VcrHipError):
            posegraph.check_edges(src, dst, 3)


def test_the_python_calls_refuse_bad_arguments_on_the_host():
    import vcrnet_amd
    from vcrnet_amd import posegraph
    from vcrnet_amd.native import VcrHipError
    R, t = torch.eye(3, dtype=torch.float64).repeat(4, 1, 1), torch.zeros(4, 3, dtype=torch.float64)
    e = (torch.tensor([0, 1]), torch.tensor([1, 2]), torch.eye(3).repeat(2, 1, 1), torch.zeros(2, 3), torch.eye(6).repeat(2, 1, 1), torch.zeros(2))
    ok = dict(max_correspondence_distance=0.05)
    for kw, what in ((dict(), "no default"), (dict(max_correspondence_distance=-1.0), "finite and >= 0"),
                     (dict(max_correspondence_distance=float("nan")), "finite and >= 0"), (dict(ok, edge_prune_threshold=float("inf")), "finite"),
                     (dict(ok, anchor=4), "anchor"), (dict(ok, anchor=-1), "anchor"), (dict(ok, criteria=dict(max_iters=3)), "criteria"),
                     (dict(ok, criteria=[1]), "criteria"), (dict(ok, criteria=dict(max_iteration=2.5)), "max_iteration"),
                     (dict(ok, criteria=dict(max_iteration=300, max_iteration_lm=20)), "4096"), (dict(ok, criteria=dict(max_iteration=-1)), "max_iteration"),
                     (dict(ok, criteria=dict(min_residual=-1.0)), "min_residual"), (dict(ok, criteria=dict(min_right_term=float("nan"))), "min_right_term"),
                     (dict(ok, criteria=dict(lower_scale_factor=0.0)), "lower_scale_factor"), (dict(ok), "no CPU fallback")):
        with pytest.raises(VcrHipError, match=what):
            vcrnet_amd.optimize_pose_graph(R, t, *e, **kw)
    with pytest.raises(VcrHipError, match="variant"):
        posegraph.optimize(R, t, *e, variant=3, **ok)
    with pytest.raises(VcrHipError, match="R must be"):
        vcrnet_amd.optimize_pose_graph(torch.zeros(4, 3), t, *e, **ok)
    with pytest.raises(VcrHipError, match="at most 128"):
        vcrnet_amd.optimize_pose_graph(torch.zeros(129, 3, 3), torch.zeros(129, 3), *e, **ok)
    clouds = torch.zeros(4, 3, 50)
    for args, kw, what in (((clouds, None, 0.05), {}, "no default"), ((clouds, 0.1, -1.0), {}, "finite"), ((torch.zeros(4, 50, 3), 0.1, 0.05), {}, "point cloud"),
                           ((clouds[:1], 0.1, 0.05), {}, "2 ... 128"), ((clouds, 0.1, 0.05), dict(pairs=[(0, 1), (1, 2)]), "odometry pair"),
                           ((clouds, 0.1, 0.05), dict(pairs=[(0, 1), (2, 1), (2, 3)]), "distinct"), ((clouds, 0.1, 0.05), dict(pairs=[(0, 1), (1, 2), (2, 3), (0, 4)]), "distinct"),
                           ((clouds, 0.1, 0.05), dict(pairs=[(0, 1), (1, 2), (2, 3), (0, 3)]), "cuda")):
        with pytest.raises(VcrHipError, match=what):
            vcrnet_amd.pose_graph_from_clouds(*args, **kw)
    with pytest.raises(VcrHipError, match="cuda"):
        vcrnet_amd.register_multiway(clouds, 0.1, 0.05)
    assert posegraph.all_pairs(4) == [(0, 1), (0, 2), (0, 3), (1, 2), (1, 3), (2, 3)]
    assert posegraph.check_criteria(None) == posegraph.CRITERIA and posegraph.check_criteria(dict(max_iteration=6))["max_iteration"] == 6


def test_the_form_follows_the_lds_a_graph_needs(lib):
    """The factor is K (K + 1) / 2 blocks of 288 bytes; with the poses, b, d and the lists it must fit the 160 KiB of a CU's LDS,
    allocated in 1280-byte granules, next to the kernel's static 4 KiB: the last K of the LDS form, the first of the global
    form, and the ends of the domain."""
    from vcrnet_amd import posegraph
    small = lambda K: (12 * 2 + 6 * 2 + 1) * K * 8 + ((K + 2) & ~1) * 4                                      # noqa: E731
    full = lambda K: small(K) + K * (K + 1) // 2 * 288                                                       # noqa: E731
    fits = lambda K: -(-(full(K) + 4096) // 1280) * 1280 <= 160 * 1024                                       # noqa: E731
    last = max(K for K in range(1, 129) if fits(K))
    assert fits(1) and not fits(128) and all(fits(K) for K in range(1, last + 1))
    for K in (1, 8, last, last + 1, 128):
        form, lds, ws = posegraph.posegraph_form(K, G=3, E=10)
        assert form == (posegraph.FORM_LDS if K <= last else posegraph.FORM_GLOBAL), K
        assert lds == (full(K) if K <= last else small(K)), K
        packed = -(-(3 * K * (K + 1) // 2 * 288) // 256) * 256
        assert ws >= packed * (1 if K <= last else 2) + 3 * 10 * (29 * 8 + 12) and ws % 256 == 0, K
        assert posegraph.posegraph_form(K, G=3, E=10, variant=posegraph.FORM_GLOBAL) == (posegraph.FORM_GLOBAL, small(K), ws if K > last else ws + packed)
        if K <= last:
            assert posegraph.posegraph_form(K, G=3, E=10, variant=posegraph.FORM_LDS) == (form, lds, ws)
        else:
            with pytest.raises(Exception):
                posegraph.posegraph_form(K, variant=posegraph.FORM_LDS)
    res = __import__("vcrnet_amd").build.kernel_resources()
    static = [v["lds"] for n, v in res.items() if v["file"] == "posegraph.hip" and "posegraph_kernel" in n]
    assert len(static) == 2 and max(static) <= 4096          # what the plan sets aside for the static __shared__


def test_the_kernel_uses_no_scratch(lib):
    from vcrnet_amd import build
    res = build.kernel_resources()
    names = list(res)
    dem = subprocess.run(["c++filt"], input="\n".join(names), capture_output=True, text=True, check=True).stdout.splitlines()
    short = lambda d: re.sub(r"^void ", "", d.replace("(anonymous namespace)::", "")).split("(")[0]       # noqa: E731
    mine = {short(d): res[n] for n, d in zip(names, dem) if res[n]["file"] == "posegraph.hip" and "copy_words" not in n}
    assert set(mine) == {"posegraph_kernel<1>", "posegraph_kernel<2>"}, sorted(mine)   # one instantiation per form
    for k, v in mine.items():
        assert v.get("scratch", 0) == 0 and v.get("vgpr_spill", 0) == 0 and v.get("agprs", 0) == 0, (k, v)
        assert v["vgprs"] <= 256, (k, v)                     # (a 256-lane workgroup: 512 registers a lane are there)


# ------------------------------------------------------------------------------------------------------ the restatement

def _consistent_ring():
    """The ring's nodes and edge list with every X exact: r_e = 0 at the planted poses."""
    rc = pgr.ring()
    g, R, t = rc["graph"], rc["R_true"], rc["t_true"]
    Re, te = [], []
    for i, j in zip(g.src, g.dst):
        Rj, tj = pgr.inverse(R[j], t[j])
        Rx, tx = pgr.compose(Rj, tj, R[i], t[i])
        Re.append(Rx); te.append(tx)
    return pgr.Graph(g.src, g.dst, Re, te, g.info, g.unc, g.K), R, t


def test_the_jacobians_match_central_differences_on_a_consistent_graph():
    """Step and bound from fp64 rounding: r is computed from entries of size S = 1 + max |t| with an absolute error of a few
    eps S, so a central difference of step h carries about 32 eps S / h of rounding and h^2 S of truncation (the third
    derivatives of vec6 about 0 are of order S).  h = 2^-16 balances the two near 1e-9."""
    g, R, t = _consistent_ring()
    assert np.abs(pgr.residuals(R, t, g.s, g.d, g.Re, g.te)).max() < 64 * EPS * 3
    J = pgr.jacobians(R, t, g.s, g.d, g.Re, g.te)
    h = 2.0 ** -16
    S = 1 + np.abs(t).max()
    bound = h * h * S + 32 * EPS * S / h
    worst = 0.0
    for e in range(g.E):
        for node, sign in ((g.s[e], 1.0), (g.d[e], -1.0)):
            for k in range(6):
                x = np.zeros(6)
                x[k] = h
                Rp, tp, Rm, tm = R.copy(), t.copy(), R.copy(), t.copy()
                Rp[node], tp[node] = pgr.step(x, R[node], t[node])
                Rm[node], tm[node] = pgr.step(-x, R[node], t[node])
                fd = (pgr.residuals(Rp, tp, g.s, g.d, g.Re, g.te)[e] - pgr.residuals(Rm, tm, g.s, g.d, g.Re, g.te)[e]) / (2 * h)
                worst = max(worst, np.abs(fd - sign * J[e, :, k]).max())
    _emit(f"restatement: max |J - central difference| {worst:.3e} (bound {bound:.3e}, h = 2^-16)")
    assert worst <= bound


def test_vec6_inverts_pl_euler():
    rs = np.random.RandomState(0)
    for _ in range(200):
        x = np.concatenate([rs.uniform(-np.pi, np.pi, 1), rs.uniform(-np.pi / 2, np.pi / 2, 1) * 0.999, rs.uniform(-np.pi, np.pi, 1), rs.normal(size=3)])
        back = pgr.vec6(*pgr.euler(x))
        assert np.abs(back - x).max() <= 64 * EPS / np.cos(x[1]) ** 2 + 64 * EPS * np.pi, (x, back)
    for x1 in (np.pi / 2, -np.pi / 2):                       # sy <= 1e-6: x2 is reported 0 and x0 takes the turn about z with it
        x = np.array([0.3, x1, 0.0, 1.0, -2.0, 0.5])
        R, t = pgr.euler(x)
        assert np.sqrt(R[0, 0] ** 2 + R[1, 0] ** 2) <= 1e-6
        back = pgr.vec6(R, t)
        assert back[2] == 0.0 and abs(back[0] - 0.3) < 1e-12 and abs(back[1] - x1) < 1e-12 and np.array_equal(back[3:], x[3:])
        R2, _ = pgr.euler(back)
        assert np.abs(R2 - R).max() < 1e-12
    assert np.array_equal(pgr.vec6(np.eye(3), np.zeros(3)), np.zeros(6))
    R, t = pgr.euler(np.zeros(6))
    assert np.array_equal(R, np.eye(3)) and not t.any()        # the anchor's update is exact


def test_the_line_process_weight_zeroes_the_objectives_derivative():
    """d/dl (l q + mu (sqrt(l) - 1)^2) = q + mu (1 - 1 / sqrt(l)), zero at sqrt(l) = mu / (mu + q)."""
    rs = np.random.RandomState(1)
    for mu, q in zip(10.0 ** rs.uniform(-3, 3, 100), 10.0 ** rs.uniform(-6, 4, 100)):
        s = float(pgr.line_process(np.array([q]), np.array([True]), mu)[0])
        assert 0 < s <= 1 and abs(q + mu * (1 - 1 / s)) <= 8 * EPS * (q + mu)
        f = lambda l: l * q + mu * (np.sqrt(l) - 1) ** 2                                                # noqa: E731
        assert f(s * s) <= f(s * s * 1.01) and f(s * s) <= f(s * s * 0.99)
    assert pgr.line_process(np.array([3.0]), np.array([False]), 0.5)[0] == 1.0
    assert pgr.line_process(np.array([0.0]), np.array([True]), 0.5)[0] == 1.0


def test_the_ring_recipe():
    rc = pgr.ring()
    g = rc["graph"]
    assert g.K == 8 and g.E == 14 and g.unc.sum() == 7 and g.valid.all() and (g.info[:, 5, 5] == 60).all()
    trace = []
    o = pgr.optimize(g, rc["R0"], rc["t0"], pgr.MCD, trace=trace)
    first = pgr.optimize(g, rc["R0"], rc["t0"], pgr.MCD, prune=False)
    w = rc["wrong_edge"]
    assert first["weight"][w] < 0.25 and o["kept"][w] == 0
    true = np.nonzero(g.unc)[0][np.nonzero(g.unc)[0] != w]
    assert o["kept"][true].all() and (first["weight"][true] > 0.25).all() and o["kept"][~g.unc].all()
    assert o["converged"] == 1 and o["residual"][1] <= o["residual"][0]
    e_opt = pgr.pose_error(o["R"], o["t"], rc["R_true"], rc["t_true"])
    e_odo = pgr.pose_error(rc["R0"], rc["t0"], rc["R_true"], rc["t_true"])
    assert e_opt[0] < e_odo[0] and e_opt[1] < e_odo[1]
    assert o["R"][0].tobytes() == rc["R0"][0].tobytes() and o["t"][0].tobytes() == rc["t0"][0].tobytes()     # the anchor, to the bit
    _emit(f"restatement, ring (seed 3): pose error (rad, length) optimised {e_opt[0]:.6e} {e_opt[1]:.6e}, chained odometry {e_odo[0]:.6e} {e_odo[1]:.6e}; "
          f"l of the wrong edge {first['weight'][w]:.3e}, least l of a true closure {first['weight'][true].min():.3f}; residual {o['residual'][0]:.6e} -> "
          f"{o['residual'][1]:.6e}; iterations {o['iterations'].tolist()}, trials {o['trials'].tolist()}")
    # the system: symmetric, the anchor's rows the identity's, a duplicate edge adds to the same blocks
    tri = pgr.triangle()
    gt = tri["graph"]
    lin = pgr.linearise(gt, tri["R0"], tri["t0"], gt.valid, pgr.mu_of(gt, gt.valid, pgr.MCD))
    assert np.array_equal(lin["H"], lin["H"].T) and np.array_equal(lin["H"][:6, :6], np.eye(6)) and not lin["H"][:6, 6:].any() and not lin["b"][:6].any()
    d, ok = pgr.solve(lin["H"], 1e-5 * lin["H"].diagonal().max(), lin["b"])
    A = lin["H"] + 1e-5 * lin["H"].diagonal().max() * np.eye(18)
    assert ok and np.abs(A @ d - lin["b"]).max() <= 64 * EPS * np.linalg.cond(A) * np.abs(lin["b"]).max() and not d[:6].any()
    assert not pgr.solve(np.zeros((6, 6)), 0.0, np.ones(6))[1] and not pgr.solve(np.full((6, 6), np.nan), 1.0, np.ones(6))[1]
    # a blank anywhere changes nothing
    src, dst = np.insert(g.src, 5, -1), np.insert(g.dst, 5, 3)
    gb = pgr.Graph(src, dst, np.insert(g.Re, 5, np.nan, 0), np.insert(g.te, 5, np.nan, 0), np.insert(g.info, 5, np.nan, 0), np.insert(g.unc, 5, 1), 8)
    ob = pgr.optimize(gb, rc["R0"], rc["t0"], pgr.MCD)
    assert ob["R"].tobytes() == o["R"].tobytes() and ob["residual"].tobytes() == o["residual"].tobytes() and np.isnan(ob["weight"][5]) and ob["kept"][5] == 0
