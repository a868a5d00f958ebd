"""The grid siblings of the scoring and refining calls without a GPU: the boundary of include/vcr_hip_gridnn.h (prototypes against
vcrnet_amd.gridnn.SIGNATURES, vcr_grid_nn_args against gcc's layout, the exported symbols, the other headers' structs where they
were), every argument error of the calls and of the Python functions, the host-only form and workspace queries against the
header's formula, the resource remarks of grid_nn_kernel, and the numpy restatement (tests/gridnn_restated.py): the walk -- the
query clamped into the target's grid, rings, the ring bound, the outside bound, the three stops -- against the brute-force
definition, row for row and bit for bit, with no bound undercut."""
import ctypes
import os
import subprocess
import types

import numpy as np
import pytest
import torch

import boundary
import grid_restated as gr
import gridnn_restated as gn

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INCLUDE = os.path.join(ROOT, "include")
HEADER = os.path.join(INCLUDE, "vcr_hip_gridnn.h")
OTHERS = ("vcr_hip.h", "vcr_hip_score.h", "vcr_hip_refine.h", "vcr_hip_plane.h", "vcr_hip_voxel.h", "vcr_hip_outlier.h",
          "vcr_hip_gicp.h", "vcr_hip_fpfh.h", "vcr_hip_match.h", "vcr_hip_fgr.h", "vcr_hip_grid.h")
EINVAL, EWORKSPACE, EUNSUPPORTED = -1, -2, -3
FAMILIES = ("vcr_nn_score_grid", "vcr_refine_grid", "vcr_refine_plane_grid", "vcr_refine_gicp_grid")
ENTRY_POINTS = {f + s for f in FAMILIES for s in ("_f32", "_workspace_bytes", "_form")}
VALUES = {"vcr_refine_grid": 17, "vcr_refine_plane_grid": 29, "vcr_refine_gicp_grid": 29}


@pytest.fixture(scope="module")
def lib():
    import vcrnet_amd  # noqa: F401
    from vcrnet_amd import build, gridnn
    build.build()
    return gridnn.lib()


# ---------------------------------------------------------------------------------------------------------------- the boundary

def test_signatures_match_the_header_and_the_library_exports_them(lib):
    from vcrnet_amd import gridnn
    boundary.check_signatures(HEADER, gridnn, lib, ENTRY_POINTS)
    assert len(ENTRY_POINTS) == 12


def test_args_match_the_c_layout(tmp_path):
    import vcrnet_amd  # noqa: F401
    from vcrnet_amd import gridnn
    assert set(gridnn.NEW_STRUCTS) == {"vcr_grid_nn_args"}
    boundary.check_layout(HEADER, types.SimpleNamespace(STRUCTS=gridnn.NEW_STRUCTS), tmp_path)
    assert ctypes.sizeof(gridnn.GridNnArgs) == 12


def test_the_other_boundaries_are_where_they_were(lib, tmp_path, monkeypatch):
    """The calls live beside the eleven headers, not in them: none mentions them, ABI 27, the same 51 prototypes, every struct of
    the four scan siblings laid out as its own header lays it out; the new header is taken into the digests through a list of
    its own."""
    from vcrnet_amd import build, fgr, fpfh, gicp, grid, gridnn, match, native, outlier, plane, refine, score, voxel
    for h in OTHERS:
        text = open(os.path.join(INCLUDE, h)).read()
        assert "gridnn" not in text and "vcr_grid_nn" not in text and "_grid_f32" not in text, h
    assert len(native.PUBLIC) == 51 and lib.vcr_abi_version() == native.ABI_VERSION == 27
    for other in (native, score, refine, plane, voxel, outlier, gicp, fpfh, match, fgr, grid):
        assert not set(gridnn.SIGNATURES) & set(other.SIGNATURES) and not set(gridnn.NEW_STRUCTS) & set(other.STRUCTS)
    assert not set(gridnn.SIGNATURES) & set(native.PUBLIC)
    for header, module in (("vcr_hip_score.h", score), ("vcr_hip_refine.h", refine), ("vcr_hip_plane.h", plane), ("vcr_hip_gicp.h", gicp)):
        boundary.check_layout(os.path.join(INCLUDE, header), module, tmp_path)
        for name, ct in module.STRUCTS.items():
            assert gridnn.STRUCTS.get(name, ct) is ct                # (the siblings' own mirrors, not copies)
    assert build.GRIDNN_HEADERS == [HEADER] and build.GRID_HEADERS == [os.path.join(INCLUDE, "vcr_hip_grid.h")]
    full = build.sources_sha16()
    monkeypatch.setattr(build, "GRIDNN_HEADERS", [])
    assert build.sources_sha16() != full


def _score(**kw):
    from vcrnet_amd import score
    a = score.NnScoreArgs()
    a.src, a.tgt, a.fitness, a.rmse = 0x1000, 0x2000, 0x3000, 0x4000          # (never dereferenced on the host)
    v = dict(B=2, Ns=1000, Nt=700, max_dist=0.1, variant=0)
    v.update(kw)
    for k, x in v.items():
        setattr(a, k, x)
    return a


def _refine(family, **kw):
    from vcrnet_amd import gicp, plane, refine
    Args = {"vcr_refine_grid": refine.RefineArgs, "vcr_refine_plane_grid": plane.RefinePlaneArgs,
            "vcr_refine_gicp_grid": gicp.RefineGicpArgs}[family]
    a = Args()
    a.src, a.tgt, a.R_out, a.t_out, a.fitness, a.rmse = 0x1000, 0x2000, 0x3000, 0x4000, 0x5000, 0x6000
    v = dict(B=2, Ns=1000, Nt=700, max_dist=0.1, max_iterations=30, rel_fitness=1e-6, rel_rmse=1e-6, variant=0)
    if family != "vcr_refine_grid":
        v["tgt_normals"] = 0x7000
    if family == "vcr_refine_gicp_grid":
        v.update(src_normals=0x8000, epsilon=1e-3)
    v.update(kw)
    for k, x in v.items():
        setattr(a, k, x)
    return a


def _args(family, **kw):
    return _score(**kw) if family == "vcr_nn_score_grid" else _refine(family, **kw)


def _g(cell=0.0, order=0):
    from vcrnet_amd import gridnn
    return gridnn.GridNnArgs(cell, order)


def _codes(lib, family, a, g):
    """The three entry points agree on a refusal: its code, its code, 0 bytes."""
    ga = None if g is None else ctypes.byref(g)
    aa = None if a is None else ctypes.byref(a)
    rc = getattr(lib, family + "_f32")(aa, ga, 0x10000, 1 << 40, None)
    assert getattr(lib, family + "_workspace_bytes")(aa, ga, 256) == 0
    assert getattr(lib, family + "_form")(aa, ga, 256, None, None, None) == rc
    return rc


@pytest.mark.parametrize("family", FAMILIES)
def test_argument_errors_return_their_codes_without_a_gpu(lib, family):
    from vcrnet_amd import gridnn
    nan, inf = float("nan"), float("inf")
    assert _codes(lib, family, None, _g()) == EINVAL and _codes(lib, family, _args(family), None) == EINVAL
    # the scan's forms do not apply
    for variant in (1, 2, 4, 0x100, 0x8001, -1):
        assert _codes(lib, family, _args(family, variant=variant), _g()) == EINVAL, variant
    # the grid's own arguments
    for kw in (dict(cell=-1.0), dict(cell=-1e-30), dict(cell=nan), dict(cell=inf), dict(cell=-inf), dict(order=3), dict(order=-1),
               dict(order=0x100)):
        assert _codes(lib, family, _args(family), _g(**kw)) == EINVAL, kw
    size = ctypes.sizeof(gridnn.GridNnArgs)
    for bad in (0, 4, size - 4, size + 4):
        g = _g()
        g.struct_bytes = bad
        assert _codes(lib, family, _args(family), g) == EINVAL, bad
    # the sibling's refusals, passed through with the sibling's codes
    for field in ("src", "tgt", "fitness", "rmse"):
        a = _args(family)
        setattr(a, field, None)
        assert _codes(lib, family, a, _g()) == EINVAL, field
    for kw in (dict(B=0), dict(Ns=0), dict(Nt=0), dict(max_dist=-1.0), dict(max_dist=nan), dict(max_dist=inf)):
        assert _codes(lib, family, _args(family, **kw), _g()) == EINVAL, kw
    for kw in (dict(Ns=131073), dict(Nt=131073), dict(B=16384, Ns=131072)):
        assert _codes(lib, family, _args(family, **kw), _g()) == EUNSUPPORTED, kw
    a = _args(family)
    a.struct_bytes = 0
    assert _codes(lib, family, a, _g()) == EINVAL
    if family != "vcr_nn_score_grid":
        for kw in (dict(max_iterations=-1), dict(rel_fitness=-1.0), dict(rel_rmse=nan), dict(R_out=None), dict(t_out=None)):
            assert _codes(lib, family, _args(family, **kw), _g()) == EINVAL, kw
        assert _codes(lib, family, _args(family, max_iterations=4097), _g()) == EUNSUPPORTED
    if family in ("vcr_refine_plane_grid", "vcr_refine_gicp_grid"):
        assert _codes(lib, family, _args(family, tgt_normals=None), _g()) == EINVAL
    if family == "vcr_refine_gicp_grid":
        for kw in (dict(src_normals=None), dict(epsilon=0.0), dict(epsilon=2.0), dict(epsilon=nan)):
            assert _codes(lib, family, _args(family, **kw), _g()) == EINVAL, kw
    assert getattr(lib, family + "_form")(ctypes.byref(_args(family)), ctypes.byref(_g()), -1, None, None, None) == EINVAL
    assert getattr(lib, family + "_workspace_bytes")(ctypes.byref(_args(family)), ctypes.byref(_g()), -1) == 0
    # a good call's workspace is checked before anything is launched
    need = getattr(lib, family + "_workspace_bytes")(ctypes.byref(_args(family)), ctypes.byref(_g()), 0)
    assert need > 0
    f32 = getattr(lib, family + "_f32")
    assert f32(ctypes.byref(_args(family)), ctypes.byref(_g()), None, need, None) == EINVAL
    assert f32(ctypes.byref(_args(family)), ctypes.byref(_g()), 0x10008, need, None) == EINVAL
    assert f32(ctypes.byref(_args(family)), ctypes.byref(_g()), 0x10000, need - 1, None) == EWORKSPACE


def _formula(family, B, Ns, Nt, order):
    """The header's workspace formula."""
    up = lambda v: (v + 255) & ~255                                               # noqa: E731
    G = lambda N: 2 * N + 64                                                      # noqa: E731
    cloud = lambda N: up(64 * B) + up(4 * B * N) + up(4 * B * (G(N) + 2)) + up(16 * B * N)   # noqa: E731
    nb = (Ns + 255) // 256
    grid = cloud(Nt) + (cloud(Ns) if order == 1 else 0)
    if family == "vcr_nn_score_grid":
        return 2 * up(4 * B * Ns) + up(16 * B * nb) + grid
    return 2 * up(4 * B * Ns) + up(8 * VALUES[family] * B * nb) + up(96 * B) + up(8 * B) + 2 * up(4 * B) + grid


@pytest.mark.parametrize("family", FAMILIES)
def test_the_form_and_workspace_queries_are_host_only_and_follow_the_header(lib, family):
    """The workspace is the header's formula of (B, Ns, Nt, order) alone -- no CU count, no cell enters it --; the form reports
    the target's budget, the order taken and 256 queries a workgroup; order 0 is the plan's: index order for the one evaluation,
    the source's order for a refinement that enqueues at least eight searches."""
    from vcrnet_amd import grid, gridnn
    wsb, form = getattr(lib, family + "_workspace_bytes"), getattr(lib, family + "_form")
    for B, Ns, Nt in ((1, 1, 1), (3, 300, 1), (3, 1, 300), (2, 255, 257), (16, 1024, 1024), (1, 131072, 70001), (1, 70001, 131072)):
        for order in (1, 2):
            for cell in (0.0, 0.25):
                a, g = _args(family, B=B, Ns=Ns, Nt=Nt), _g(cell, order)
                got = wsb(ctypes.byref(a), ctypes.byref(g), 256)
                assert got == _formula(family, B, Ns, Nt, order), (B, Ns, Nt, order)
                assert got == wsb(ctypes.byref(a), ctypes.byref(g), 0) == wsb(ctypes.byref(a), ctypes.byref(g), 1)
                c, o, q = ctypes.c_int(0), ctypes.c_int(0), ctypes.c_int(0)
                assert form(ctypes.byref(a), ctypes.byref(g), 256, ctypes.byref(c), ctypes.byref(o), ctypes.byref(q)) == 0
                assert (c.value, o.value, q.value) == (grid.cells(Nt), order, 256)
        a = _args(family, B=B, Ns=Ns, Nt=Nt)
        plan = 2 if family == "vcr_nn_score_grid" else 1
        assert gridnn.form(family, a, _g(0.0, 0)) == (grid.cells(Nt), plan, 256, _formula(family, B, Ns, Nt, plan))
    if family != "vcr_nn_score_grid":
        for its, want in ((0, 2), (6, 2), (7, 1), (30, 1), (4096, 1)):
            assert gridnn.form(family, _args(family, max_iterations=its), _g())[1] == want, its
            assert gridnn.form(family, _args(family, max_iterations=its), _g(0.0, 2))[1] == 2
    assert gridnn.nn_score_grid_form(2, 1000, 700) == gridnn.form("vcr_nn_score_grid", _score(), _g())
    for method, fam in (("point_to_point", "vcr_refine_grid"), ("point_to_plane", "vcr_refine_plane_grid"), ("generalized", "vcr_refine_gicp_grid")):
        assert gridnn.refine_grid_form(2, 1000, 700, method=method) == gridnn.form(fam, _refine(fam), _g())
    assert (gridnn.SEARCHES, gridnn.ORDERS, gridnn.QUERIES) == (("scan", "grid"), (0, 1, 2), 256)


def test_the_new_kernels_use_no_scratch_and_the_search_keeps_eight_waves():
    """hipcc's remarks for gridnn.hip: no scratch, no spill; grid_nn_kernel within 64 VGPRs (eight waves a SIMD), no LDS -- the
    best key lives in a register pair.  The five build kernels are grid.hip's text (grid_build.h) and keep its resources."""
    import vcrnet_amd  # noqa: F401
    from vcrnet_amd import build
    build.build()
    res = build.kernel_resources()
    names = list(res)
    dem = subprocess.run(["c++filt"], input="\n".join(names), capture_output=True, text=True, check=True).stdout.splitlines()
    short = {d.replace("(anonymous namespace)::", "").replace("void ", "").split("(")[0]: res[n] for n, d in zip(names, dem)}
    mine = {k: v for k, v in short.items() if v["file"] == "gridnn.hip"}
    assert set(mine) == {"grid_nn_kernel", "grid_perm_kernel"}
    for d, v in mine.items():
        print(d, v)
        assert v.get("scratch", 0) == 0 and v.get("vgpr_spill", 0) == 0 and v.get("sgpr_spill", 0) == 0, (d, v)
    s = mine["grid_nn_kernel"]
    assert s["occupancy"] == 8 and s["vgprs"] <= 64 and s["agprs"] == 0 and s["lds"] == 0
    text = open(os.path.join(ROOT, "vcr-net_amd", "csrc", "gridnn.hip")).read()
    kernel = text[text.index("void grid_nn_kernel"):text.index("}  // namespace")]
    assert "atomic" not in kernel and "__syncthreads" not in kernel and "__shared__" not in kernel
    assert "gd_walk(" in kernel                              # ... nor has the walk it runs
    walk = open(os.path.join(ROOT, "vcr-net_amd", "csrc", "grid_walk.h")).read()
    assert "atomic" not in walk and "__syncthreads" not in walk and "__shared__" not in walk
    for k in ("grid_bounds_kernel", "grid_clear_kernel", "grid_count_kernel", "grid_scan_kernel", "grid_scatter_kernel"):
        assert short[k]["file"] == "grid.hip" and short[k].get("scratch", 0) == 0


# ------------------------------------------------------------------------------------------------------------- the restatement

def test_the_definition_on_clouds_worked_by_hand():
    q = np.asarray([[0, 1, 1, 5, 1], [0, 0, 0, 0, 0], [0, 0, 0, 0, np.nan]], np.float32)     # 1 and 2 are copies; 4 is not finite
    p = np.asarray([[1, 0.25, 4, np.nan, 1e30, 9], [0, 0, 0, 0, 0, 0], [0, 0, 0, 0, 0, 0]], np.float32)
    idx, bits = gn.scan(p, q)
    assert idx.tolist() == [1, 0, 3, -1, -1, 3] and bits.view(np.float32).tolist()[:3] == [0, 0.0625, 1]
    assert np.isinf(bits.view(np.float32)[3:5]).all() and bits.view(np.float32)[5] == 16
    idx, bits = gn.definition(p, q, 1.0)                      # the cap is inclusive; 16 > 1: (-1, +inf)
    assert idx.tolist() == [1, 0, 3, -1, -1, -1] and np.isinf(bits.view(np.float32)[3:]).all()
    idx, bits = gn.definition(p, q, 0.0)
    assert idx.tolist() == [1, -1, -1, -1, -1, -1] and bits[0] == 0
    idx, bits = gn.definition(p, q, 1e30)                     # cap2 = +inf: the scan form's rows
    assert np.array_equal(idx, gn.scan(p, q)[0]) and np.array_equal(bits, gn.scan(p, q)[1])
    for cell in (0.0, 0.5, 100.0):
        for md in (0.0, 0.25, 1.0, 4.0, 1e30):
            got = gn.walk(p, q, md, cell)
            want = gn.definition(p, q, md)
            assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]) and got[2]["violations"] == 0


CASES = [(name, 300) for name in gn.RECIPES] + [(name, 2000) for name in gn.LARGE]


@pytest.mark.parametrize("name,N", CASES)
def test_the_walk_returns_the_definition_bit_for_bit(name, N):
    """Every recipe at the origin and moved by 1 024; the source as it is and shifted a whole extent beyond the box along one,
    two and three axes; max_dist in {0, half the edge, 4 edges, 1e30}; the automatic grid and the forced edges from "every point
    its own cell" to "one cell" (at N = 2 000 the automatic edge, a fine one and one cell): the walk's rows are the
    definition's, and no ring bound and no outside bound it took was undercut by a point it had not seen."""
    checks = outside = by_cap = by_best = skipped = 0
    for offset in (0.0, 1024.0):
        q = gr.RECIPES[name](N, seed=N)
        q = gr.moved(q, offset) if offset else q
        p0 = gn.source_of(q, seed=N)
        cells = [0.0] + gr.forced_cells(q)
        if N > 300:
            cells = [cells[0], cells[2], cells[-1]]
        grids = set()
        for shift in gn.SHIFTS:
            p = gn.shifted(p0, q, shift)
            D = gn.d2_matrix(p, q)
            for max_dist in gn.caps(q):
                want = gn.definition(p, q, max_dist, D)
                assert want[0].min() >= -1 and want[0].max() < N
                for cell in cells:
                    idx, bits, st = gn.walk(p, q, max_dist, cell, D=D)
                    assert np.array_equal(idx, want[0]) and np.array_equal(bits, want[1]), (name, offset, shift, max_dist, cell, st)
                    assert st["violations"] == 0 and st["outside_violations"] == 0, (name, offset, shift, max_dist, cell, st)
                    assert st["n"][0] * st["n"][1] * st["n"][2] <= gr.cells_budget(N), st
                    checks += st["checks"]; outside += st["outside"]; skipped += st["skipped"]
                    by_cap += st["stopped_by_cap"]; by_best += st["stopped_by_best"]
                    grids.add(st["n"])
            if not shift:
                zero = gn.definition(p, q, 0.0, D)
                assert (zero[0] >= 0).sum() >= 1 or name == "nonfinite"          # (the untouched copies: d2 = 0 is an inlier at cap 0)
        assert (1, 1, 1) in grids and (len(grids) >= 3 or name == "equal"), grids
    print(name, N, "ring bounds", checks, "outside bounds", outside, "walks skipped", skipped, "stopped by the cap", by_cap,
          "stopped by the best", by_best)
    assert skipped > 0 and checks > 0                          # (the far points and the shifted sources walk nothing under a small cap)
    if name in ("lattice", "flat", "tiny", "clustered", "copies"):
        assert by_cap > 0 and by_best > 0                      # (both strict stops are exercised, not only the exhaustion)


# ------------------------------------------------------------------------------------------------------------ the Python layer

def test_python_entry_points_refuse_an_unknown_search():
    import vcrnet_amd
    from vcrnet_amd import gicp, native, plane, refine, score
    E = native.VcrHipError
    x = torch.zeros(2, 3, 50)
    R, t = torch.eye(3).repeat(2, 1, 1), torch.zeros(2, 3)
    calls = (("score_registration", "search", lambda **kw: vcrnet_amd.score_registration(x, x, R, t, 0.1, **kw)),
             ("score_registration", "search", lambda **kw: vcrnet_amd.score_registration(x, x, None, None, 0.1, symmetric=True, **kw)),
             ("score_registration", "search", lambda **kw: score.nn_score(x, x, R, t, 0.1, **kw)),
             ("refine_registration", "search", lambda **kw: vcrnet_amd.refine_registration(x, x, R, t, 0.1, **kw)),
             ("refine_registration", "search", lambda **kw: vcrnet_amd.refine_registration(x, x, R, t, 0.1, method="point_to_plane", **kw)),
             ("refine_registration", "search", lambda **kw: vcrnet_amd.refine_registration(x, x, R, t, 0.1, method="generalized", **kw)),
             ("refine_registration", "search", lambda **kw: vcrnet_amd.refine_registration(x, x, R, t, 0.1, centre=True, **kw)),
             ("refine_registration", "search", lambda **kw: refine.refine(x, x, R, t, 0.1, **kw)),
             ("refine_registration", "search", lambda **kw: plane.refine_plane(x, x, x, R, t, 0.1, **kw)),
             ("refine_registration", "search", lambda **kw: gicp.refine_gicp(x, x, x, x, R, t, 0.1, **kw)),
             ("register_sampled", "nn_search", lambda **kw: vcrnet_amd.register_sampled(None, x, x, 16, **{("nn_" + k if k == "search" else k): v for k, v in kw.items()})),
             ("register_features", "nn_search", lambda **kw: vcrnet_amd.register_features(x, x, 0.05, **{("nn_" + k if k == "search" else k): v for k, v in kw.items()})),
             ("register_features", "nn_search", lambda **kw: vcrnet_amd.register_features(x, x, 0.05, method="fgr", centre=True, **{("nn_" + k if k == "search" else k): v for k, v in kw.items()})))
    for api, word, fn in calls:
        for bad in ("knn", "brute", "", None, 1, "GRID"):
            with pytest.raises(E, match=f'{api}: {word} must be "scan" or "grid"'):
                fn(search=bad)
        for good in ("scan", "grid"):
            with pytest.raises(E, match="no CPU fallback"):
                fn(search=good)
        with pytest.raises(E, match="no CPU fallback"):
            fn()
    for api, word, fn in calls[:10]:
        for bad in (0.0, -1.0, float("nan"), float("inf"), "wide"):
            with pytest.raises(E, match="cell must be None"):
                fn(search="grid", cell=bad)
        with pytest.raises(E, match="no CPU fallback"):
            fn(search="grid", cell=0.25)
    # register_features' search= keeps meaning the feature stages' kNN and nothing more
    with pytest.raises(E, match='register_features: search must be "knn" or "grid"'):
        vcrnet_amd.register_features(x, x, 0.05, search="scan")
    import inspect
    for fn, name in ((vcrnet_amd.score_registration, "search"), (vcrnet_amd.refine_registration, "search"), (score.nn_score, "search"),
                     (refine.refine, "search"), (plane.refine_plane, "search"), (gicp.refine_gicp, "search"),
                     (vcrnet_amd.register_sampled, "nn_search"), (vcrnet_amd.register_features, "nn_search")):
        assert inspect.signature(fn).parameters[name].default == "scan", fn            # every default is the path as it was
