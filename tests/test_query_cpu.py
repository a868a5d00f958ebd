"""The searches from any query positions without a GPU: the numpy restatement (tests/query_restated.py) -- the walk on the points'
grid with the query's cell clamped, against the brute-force definition, row for row and bit for bit, for queries inside, on and
far outside the box --, the boundary of include/query/vcr_hip_query.h (prototypes against vcrnet_amd.query.SIGNATURES, the structs
against gcc's layout), every argument error of the calls and of the Python functions, the host-only form and workspace queries,
and the resource remarks of query.hip."""
import ctypes
import inspect
import os
import subprocess

import numpy as np
import pytest
import torch

import boundary
import grid_restated as gr
import outlier_restated as orr
import query_restated as qr
import radius_restated as rr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INCLUDE = os.path.join(ROOT, "include")
HEADER = os.path.join(INCLUDE, "query", "vcr_hip_query.h")
EINVAL, EWORKSPACE, EUNSUPPORTED = -1, -2, -3
ENTRY_POINTS = {"vcr_query_knn_f32", "vcr_query_knn_workspace_bytes", "vcr_query_knn_form",
                "vcr_query_radius_f32", "vcr_query_radius_workspace_bytes", "vcr_query_radius_form"}
KERNELS = {"query_knn_kernel", "query_count_kernel", "rows_offsets_kernel", "query_fill_kernel", "rows_order_kernel",
           "rows_pad_kernel"}
N, M, K = 300, 200, 20


@pytest.fixture(scope="module")
def lib():
    import vcrnet_amd  # noqa: F401
    from vcrnet_amd import build, query
    build.build()
    return query.lib()


# ------------------------------------------------------------------------------------------------------------- the restatement

def test_the_definition_on_clouds_worked_by_hand():
    x = np.asarray([[0, 1, 1, 5, 1], [0, 0, 0, 0, 0], [0, 0, 0, 0, np.nan]], np.float32)   # 1 and 2 are copies; 4 is not finite
    q = np.asarray([[1, -1, np.inf, 3], [0, 0, 0, 0], [0, 0, 0, 0]], np.float32)           # ON the copies; outside; not finite
    idx, bits = qr.knn(x, q, 5)
    assert idx.tolist() == [[1, 2, 0, 3, -1], [0, 1, 2, 3, -1], [-1] * 5, [1, 2, 3, 0, -1]]  # no index excluded; ties by index
    assert bits.view(np.float32)[0].tolist() == [0, 0, 1, 16, np.inf] and (bits[2] == qr.INF_BITS).all()
    got = qr.radius_rows(x, q, 2.0)
    assert got["count"].tolist() == [3, 3, 0, 3] and got["row_start"].tolist() == [0, 3, 6, 6, 9] and got["total"] == 9
    assert got["idx"].tolist() == [1, 2, 0, 0, 1, 2, 1, 2, 3]            # a point ON the sphere (d2 == r2 == 4) is in the row
    assert got["bits"].view(np.float32).tolist() == [0, 0, 1, 1, 4, 4, 4, 4, 4]
    assert qr.radius_rows(x, q, 1.999)["count"].tolist() == [3, 1, 0, 0]
    big = np.asarray([[3e38, 0], [0, 0], [0, 0]], np.float32)           # a d2 that overflows is no candidate
    assert qr.knn(big, np.asarray([[-1e19], [0], [0]], np.float32), 2)[0].tolist() == [[1, -1]]
    none = np.full((3, 4), np.nan, np.float32)                          # a cloud without a finite point
    assert (qr.knn(none, q, 3)[0] == -1).all() and qr.radius_rows(none, q, 2.0)["total"] == 0
    for res, st in (qr.walk(none, q, k=3), qr.walk(none, q, radius=2.0)):
        assert st["checks"] == 0                             # nothing is walked there


def _radii(x):
    return [orr.radius_for(N, 2), orr.radius_for(N, 12), orr.radius_for(N, 70), rr.spanning_radius(x)]


@pytest.mark.parametrize("queries", sorted(qr.QUERIES))
@pytest.mark.parametrize("name", sorted(gr.RECIPES))
def test_the_walk_returns_the_definition_bit_for_bit(name, queries):
    """Every points recipe x every query recipe at N = 300, M = 200; the automatic edge and every forced one from "every point
    its own cell" to "one cell"; both stop rules (the row's k-th d2 strictly below the ring bound; max(ring bound, outside bound)
    strictly above r2): the walk's rows are the brute force's, and no bound taken -- ring or outside -- was undercut by a
    candidate not yet seen.  This is the proof that section 4.19's bound holds for a query clamped into the grid from outside."""
    x = gr.RECIPES[name](N, seed=N)
    q = qr.QUERIES[queries](x, M, seed=1)
    assert q.shape == (3, M) and q.dtype == np.float32
    D = qr.d2_matrix(x, q)
    want = qr.knn(x, q, K, D)
    checks = early = skipped = 0
    grids = set()
    for cell in [0.0] + gr.forced_cells(x):
        (idx, bits), st = qr.walk(x, q, k=K, cell=cell, D=D)
        assert np.array_equal(idx, want[0]) and np.array_equal(bits, want[1]), (name, queries, cell, st)
        assert st["violations"] == 0 and st["n"][0] * st["n"][1] * st["n"][2] <= gr.cells_budget(N), st
        checks += st["checks"]
        early += st["stopped_early"]
        grids.add(st["n"])
    assert (1, 1, 1) in grids
    for radius in _radii(x):
        rows = qr.radius_rows(x, q, radius, D)
        for cell in [0.0] + gr.forced_cells(x):
            got, st = qr.walk(x, q, radius=radius, cell=cell, D=D)
            assert rr.same(got, rows), (name, queries, radius, cell, st)
            assert st["violations"] == 0 and st["outside_violations"] == 0, st
            checks += st["checks"]
            early += st["stopped_early"]
            skipped += st["skipped"]
    ok = gr.finite(q)
    assert (want[0][~ok] == -1).all() and not np.isin(want[0], np.flatnonzero(~gr.finite(x))).any()
    if queries == "same" and name not in ("nonfinite", "nonfinite_late"):
        assert (want[1][:, 0] == 0).all()                     # the point itself heads its row at d2 = 0: nothing is excluded
    if queries == "far":
        half = (M + 1) // 2                                   # 1e6 away: full rows; 3e19 away: every d2 overflows
        assert (want[0][half:] == -1).all() and (want[0][:half][ok[:half]] >= 0).all() and ok[:half].sum() > half // 2
    if queries == "far" or (queries == "outside" and name != "tiny"):         # (every radius spans the tiny cloud's x3 box)
        assert skipped > 0                                    # (queries whose outside bound exceeds r2 walked nothing)
    print(name, queries, "stops taken", checks, "before the grid's end", early, "walked nothing", skipped)
    if name in ("random", "lattice", "flat", "clustered") and queries in ("same", "jitter", "faces"):
        assert early > M                                      # (the stop rules are exercised, not only the exhaustion)


# ---------------------------------------------------------------------------------------------------------------- the boundary

def test_signatures_match_the_header_and_the_library_exports_them(lib):
    from vcrnet_amd import query
    boundary.check_signatures(HEADER, query, lib, ENTRY_POINTS)


def test_args_match_the_c_layout(tmp_path):
    import vcrnet_amd  # noqa: F401
    from vcrnet_amd import query
    assert set(query.STRUCTS) == {"vcr_query_knn_args", "vcr_query_radius_args"}
    boundary.check_layout(HEADER, query, tmp_path)
    assert query.QueryKnnArgs.d2.offset == query.QueryKnnArgs.idx.offset + 8            # the mandatory part ends behind idx
    assert query.QueryRadiusArgs.idx.offset == query.QueryRadiusArgs.total.offset + 8   # ... behind total


def test_the_other_boundaries_are_where_they_were(lib, monkeypatch):
    """The calls live beside the other headers, not in them: the header is alone in a directory of its own, no other header
    mentions its calls, ABI 27, the same 51 prototypes; it enters both digests through a list of its own; the header's numbers
    are the module's."""
    from vcrnet_amd import build, grid, gridnn, iss, native, orient, outlier, query, radius, rows
    assert os.listdir(os.path.join(INCLUDE, "query")) == ["vcr_hip_query.h"]
    for d in sorted(os.listdir(INCLUDE)):
        for f in ([d] if d.endswith(".h") else os.listdir(os.path.join(INCLUDE, d))):
            h = os.path.join(INCLUDE, f) if d.endswith(".h") else os.path.join(INCLUDE, d, f)
            if h != HEADER:
                text = open(h).read()
                assert "vcr_query" not in text and "VCR_QUERY" not in text, h
    assert len(native.PUBLIC) == 51 and lib.vcr_abi_version() == native.ABI_VERSION == 27
    for other in (native, grid, gridnn, outlier, radius, rows, orient, iss):
        assert not set(query.SIGNATURES) & set(other.SIGNATURES) and not set(query.STRUCTS) & set(other.STRUCTS), other
    assert build.QUERY_HEADERS == [HEADER]
    assert HEADER not in (build.PUBLIC_HEADERS + build.LATER_HEADERS + build.OUTLIER_HEADERS + build.GICP_HEADERS
                          + build.FPFH_HEADERS + build.MATCH_HEADERS + build.FGR_HEADERS + build.GRID_HEADERS
                          + build.GRIDNN_HEADERS + build.VOXEL_SORT_HEADERS + build.RADIUS_HEADERS + build.ROWS_HEADERS
                          + build.DBSCAN_HEADERS + build.SEGMENT_HEADERS + build.ORIENT_HEADERS + build.ISS_HEADERS)
    full = build.sources_sha16()                               # the profiles' digest ...
    obj = open(os.path.join(build.OBJ, "query.o.sha")).read()  # ... and the objects' (build() ran in the fixture)
    monkeypatch.setattr(build, "QUERY_HEADERS", [])
    assert build.sources_sha16() != full
    hdrs = sorted(os.path.join(build.CSRC, f) for f in os.listdir(build.CSRC) if f.endswith(".h"))
    hdrs += (build.PUBLIC_HEADERS + build.LATER_HEADERS + build.OUTLIER_HEADERS + build.GICP_HEADERS + build.FPFH_HEADERS
             + build.MATCH_HEADERS + build.FGR_HEADERS + build.GRID_HEADERS + build.GRIDNN_HEADERS + build.VOXEL_SORT_HEADERS
             + build.RADIUS_HEADERS + build.ROWS_HEADERS + build.DBSCAN_HEADERS + build.SEGMENT_HEADERS + build.ORIENT_HEADERS
             + build.ISS_HEADERS)
    src = os.path.join(build.CSRC, "query.hip")
    assert build._digest([src] + hdrs, " ".join(build.FLAGS)) != obj == build._digest([src] + hdrs + [HEADER], " ".join(build.FLAGS))
    monkeypatch.undo()
    text = open(HEADER).read()
    for name, value in (("VCR_QUERY_MAX_N", query.MAX_N), ("VCR_QUERY_MAX_K", query.MAX_K), ("VCR_QUERY_CHUNK", query.CHUNK)):
        assert "#define %s %d" % (name, value) in text, name
    assert '#include "../vcr_hip.h"' in text and '#include "../vcr_hip_grid.h"' in text
    assert query.ORDERS == {"cell": 1, "index": 2} and (query.MAX_N, query.MAX_K) == (grid.MAX_N, grid.MAX_K)


def _knn(**kw):
    from vcrnet_amd import query
    a = query.QueryKnnArgs()
    a.xyz, a.queries, a.idx, a.d2 = 0x1000, 0x2000, 0x3000, 0x4000      # (never dereferenced)
    v = dict(B=2, N=1000, M=700, k=20, cell=0.0, variant=0)
    v.update(kw)
    for k, x in v.items():
        setattr(a, k, x)
    return a


def _rd(**kw):
    from vcrnet_amd import query
    a = query.QueryRadiusArgs()
    a.xyz, a.queries, a.count, a.row_start, a.total, a.idx, a.d2 = 0x1000, 0x2000, 0x3000, 0x4000, 0x5000, 0x6000, 0x7000
    v = dict(B=2, N=1000, M=700, radius=0.1, cell=0.0, capacity=20000, variant=0)
    v.update(kw)
    for k, x in v.items():
        setattr(a, k, x)
    return a


def _codes(lib, entry, a):
    """The three entry points agree on a refusal; nothing is dereferenced and no device is touched."""
    rc = getattr(lib, entry + "_f32")(ctypes.byref(a), 0x10000, 1 << 40, None)
    assert getattr(lib, entry + "_workspace_bytes")(ctypes.byref(a), 256) == 0
    assert getattr(lib, entry + "_form")(ctypes.byref(a), 256, None, None) == rc
    return rc


def test_the_knn_search_returns_its_argument_errors_without_a_gpu(lib):
    from vcrnet_amd import query
    entry = "vcr_query_knn"
    assert lib.vcr_query_knn_f32(None, None, 0, None) == EINVAL and lib.vcr_query_knn_workspace_bytes(None, 256) == 0
    assert lib.vcr_query_knn_form(None, 256, None, None) == EINVAL
    for field in ("xyz", "queries", "idx"):
        a = _knn()
        setattr(a, field, None)
        assert _codes(lib, entry, a) == EINVAL, field
    nan, inf = float("nan"), float("inf")
    for kw in (dict(B=0), dict(B=-1), dict(cell=-1.0), dict(cell=-1e-30), dict(cell=nan), dict(cell=inf), dict(cell=-inf),
               dict(variant=3), dict(variant=-1), dict(variant=0x11), dict(variant=1 << 30)):
        assert _codes(lib, entry, _knn(**kw)) == EINVAL, kw
    for kw in (dict(N=0), dict(N=-5), dict(N=131073), dict(M=0), dict(M=-1), dict(M=131073), dict(B=16384, N=131072),
               dict(B=16384, M=131072), dict(k=0), dict(k=-1), dict(k=63)):
        assert _codes(lib, entry, _knn(**kw)) == EUNSUPPORTED, kw
    size = ctypes.sizeof(query.QueryKnnArgs)
    for bad in (0, query.QueryKnnArgs.d2.offset - 8, size + 8):
        a = _knn()
        a.struct_bytes = bad
        assert _codes(lib, entry, a) == EINVAL, bad
    assert lib.vcr_query_knn_form(ctypes.byref(_knn()), -1, None, None) == EINVAL
    assert lib.vcr_query_knn_workspace_bytes(ctypes.byref(_knn()), -1) == 0
    # what passes: no d2, k above N, one point, one query, every variant, any finite edge, the mandatory part alone
    for kw in (dict(d2=None), dict(N=5, k=62), dict(N=1), dict(M=1), dict(N=131072, M=131072, B=1), dict(variant=1),
               dict(variant=2), dict(cell=1e-30), dict(cell=3e38), dict(k=1), dict(k=62)):
        assert lib.vcr_query_knn_workspace_bytes(ctypes.byref(_knn(**kw)), 256) > 0, kw
    a = _knn()
    a.struct_bytes = query.QueryKnnArgs.d2.offset
    need = lib.vcr_query_knn_workspace_bytes(ctypes.byref(a), 256)
    assert need > 0
    ok = _knn()
    assert lib.vcr_query_knn_f32(ctypes.byref(ok), None, need, None) == EINVAL
    assert lib.vcr_query_knn_f32(ctypes.byref(ok), 0x10008, need, None) == EINVAL
    assert lib.vcr_query_knn_f32(ctypes.byref(ok), 0x10000, need - 1, None) == EWORKSPACE


def test_the_radius_search_returns_its_argument_errors_without_a_gpu(lib):
    from vcrnet_amd import query
    entry = "vcr_query_radius"
    assert lib.vcr_query_radius_f32(None, None, 0, None) == EINVAL and lib.vcr_query_radius_workspace_bytes(None, 256) == 0
    assert lib.vcr_query_radius_form(None, 256, None, None) == EINVAL
    for field in ("xyz", "queries", "count", "row_start", "total"):
        a = _rd()
        setattr(a, field, None)
        assert _codes(lib, entry, a) == EINVAL, field
    nan, inf = float("nan"), float("inf")
    for kw in (dict(B=0), dict(B=-1), dict(radius=0.0), dict(radius=-1.0), dict(radius=nan), dict(radius=inf), dict(radius=-inf),
               dict(radius=1.9e19), dict(radius=3e38),                       # finite, the square is not
               dict(cell=-1.0), dict(cell=-1e-30), dict(cell=nan), dict(cell=inf), dict(cell=-inf),
               dict(capacity=-1), dict(idx=None), dict(idx=None, d2=None, capacity=1), dict(idx=None, capacity=0),
               dict(variant=3), dict(variant=0x11), dict(variant=0x20), dict(variant=-1), dict(variant=1 << 30)):
        assert _codes(lib, entry, _rd(**kw)) == EINVAL, kw
    for kw in (dict(N=0), dict(N=-5), dict(N=131073), dict(M=0), dict(M=131073), dict(B=16384, N=131072), dict(B=16384, M=131072),
               dict(B=3, capacity=1 << 30), dict(B=2, capacity=1 << 30)):
        assert _codes(lib, entry, _rd(**kw)) == EUNSUPPORTED, kw
    size = ctypes.sizeof(query.QueryRadiusArgs)
    for bad in (0, query.QueryRadiusArgs.idx.offset - 8, size + 8):
        a = _rd()
        a.struct_bytes = bad
        assert _codes(lib, entry, a) == EINVAL, bad
    assert lib.vcr_query_radius_form(ctypes.byref(_rd()), -1, None, None) == EINVAL
    assert lib.vcr_query_radius_workspace_bytes(ctypes.byref(_rd()), -1) == 0
    for kw in (dict(radius=1.8e19), dict(radius=1e-30), dict(idx=None, d2=None, capacity=0), dict(d2=None), dict(capacity=0),
               dict(variant=1), dict(variant=2), dict(cell=1e-30), dict(cell=3e38), dict(N=1), dict(M=1),
               dict(B=1, capacity=(1 << 31) - 1)):
        assert lib.vcr_query_radius_workspace_bytes(ctypes.byref(_rd(**kw)), 256) > 0, kw
    ok = _rd()
    need = lib.vcr_query_radius_workspace_bytes(ctypes.byref(ok), 256)
    assert lib.vcr_query_radius_f32(ctypes.byref(ok), None, need, None) == EINVAL
    assert lib.vcr_query_radius_f32(ctypes.byref(ok), 0x10008, need, None) == EINVAL
    assert lib.vcr_query_radius_f32(ctypes.byref(ok), 0x10000, need - 1, None) == EWORKSPACE


def test_the_forms_and_workspaces_are_host_only_and_follow_the_header(lib):
    from vcrnet_amd import grid, query
    up = lambda v: (v + 255) & ~255                                               # noqa: E731

    def want(B, N, M, capacity=0):
        G = grid.cells(N)
        return (up(64 * B) + up(4 * B * N) + up(4 * B * (G + 2)) + up(16 * B * N)
                + up(4 * B * M) + up(4 * B * (G + 2)) + up(16 * B * M) + up(8 * B * capacity))
    for B in (1, 2, 3, 16):
        for N, M, capacity in ((1, 1, 0), (21, 1000, 20), (1000, 21, 12000), (1000, 1000, 0), (16384, 4096, 200000),
                               (131072, 16384, 1572864), (16384, 131072, 1572864)):
            a = _knn(B=B, N=N, M=M)
            got = lib.vcr_query_knn_workspace_bytes(ctypes.byref(a), 256)
            assert got == want(B, N, M) == lib.vcr_query_knn_workspace_bytes(ctypes.byref(a), 0), (B, N, M)
            for k, cell, v in ((1, 0.0, 1), (62, 0.5, 2), (7, 1e-3, 0)):          # ... nor on k, the cell, the order
                assert lib.vcr_query_knn_workspace_bytes(ctypes.byref(_knn(B=B, N=N, M=M, k=k, cell=cell, variant=v)), 1) == got
            assert query.knn_form(B, N, M, 20) == (grid.cells(N), 1, got)
            assert query.knn_form(B, N, M, 20, variant=2) == (grid.cells(N), 2, got)
            a = _rd(B=B, N=N, M=M, capacity=capacity)
            got = lib.vcr_query_radius_workspace_bytes(ctypes.byref(a), 256)
            assert got == want(B, N, M, capacity) == lib.vcr_query_radius_workspace_bytes(ctypes.byref(a), 0), (B, N, M, capacity)
            for r, cell, v in ((0.1, 0.0, 0), (7.0, 0.5, 1), (1e-3, 0.0, 2)):
                assert lib.vcr_query_radius_workspace_bytes(
                    ctypes.byref(_rd(B=B, N=N, M=M, capacity=capacity, radius=r, cell=cell, variant=v)), 1) == got
            assert query.radius_form(B, N, M, capacity) == (grid.cells(N), 1, got)
            assert query.radius_form(B, N, M, capacity, variant=2)[1] == 2
    count_only = _rd(idx=None, d2=None, capacity=0)
    assert lib.vcr_query_radius_workspace_bytes(ctypes.byref(count_only), 256) == want(2, 1000, 700, 0)
    assert query.radius_form(2, 1000, 700, 0, with_idx=False)[2] == want(2, 1000, 700, 0)
    a = _rd()
    a.struct_bytes = query.QueryRadiusArgs.idx.offset          # the mandatory part alone: a count-only call, so capacity 0
    a.capacity = 0
    assert lib.vcr_query_radius_workspace_bytes(ctypes.byref(a), 256) == want(2, 1000, 700, 0)


def test_the_kernels_of_query_hip_use_no_scratch_and_keep_eight_waves():
    """hipcc's remarks for query.hip.  Its kernel set is the three query_* kernels and the row tail (csr_rows.h's text, which
    radius.hip compiles too): the build kernels are grid.hip's text (grid_build.h), and the remarks list a kernel under the first
    file that compiles it.  No scratch, no VGPR or SGPR spill; the kNN kernel's rows are dynamic LDS (k x 256 keys), the
    ordering stages VCR_QUERY_CHUNK keys."""
    import vcrnet_amd  # noqa: F401
    from vcrnet_amd import build, query
    build.build()
    res = build.kernel_resources()
    names = list(res)
    dem = subprocess.run(["c++filt"], input="\n".join(names), capture_output=True, text=True, check=True).stdout.splitlines()
    by_name = {d.replace("(anonymous namespace)::", "").replace("void ", "").split("(")[0]: res[n] for n, d in zip(names, dem)}
    mine = {d: v for d, v in by_name.items() if v["file"] == "query.hip"}
    assert set(mine) == KERNELS
    for d, v in mine.items():
        print(d, v)
        assert v.get("scratch", 0) == 0 and v.get("vgpr_spill", 0) == 0 and v.get("sgpr_spill", 0) == 0, (d, v)
        assert v["occupancy"] == 8 and v["vgprs"] <= 64 and v["agprs"] == 0, (d, v)
    assert {d: v["lds"] for d, v in mine.items()} == {
        "query_knn_kernel": 0, "query_count_kernel": 0, "rows_offsets_kernel": 32, "query_fill_kernel": 0,
        "rows_order_kernel": query.CHUNK * 8, "rows_pad_kernel": 0}
    # what query.hip shares keeps its owner
    assert by_name["grid_scatter_kernel"]["file"] == by_name["grid_count_kernel"]["file"] == "grid.hip"
    assert by_name["radius_order_lane_kernel"]["file"] == "radius.hip" and by_name["grid_search_kernel"]["file"] == "grid.hip"


# ------------------------------------------------------------------------------------------------------------ the Python layer

def test_the_paths_without_queries_are_untouched():
    """queries is a TRAILING keyword that defaults to None on both public searches; every earlier parameter keeps its place and
    its default."""
    import vcrnet_amd
    from vcrnet_amd import grid, radius
    sig = inspect.signature(grid.search_knn)
    assert list(sig.parameters) == ["xyz", "k", "want_d2", "cell", "queries"]
    assert [p.default for p in sig.parameters.values()] == [inspect.Parameter.empty, inspect.Parameter.empty, False, None, None]
    sig = inspect.signature(radius.search_radius)
    assert list(sig.parameters) == ["xyz", "radius", "max_nn", "want_d2", "cell", "capacity", "queries"]
    assert [p.default for p in sig.parameters.values()][2:] == [None, False, None, None, None]
    assert vcrnet_amd.search_knn is grid.search_knn and vcrnet_amd.search_radius is radius.search_radius
    x = torch.zeros(2, 3, 50)
    E = vcrnet_amd.native.VcrHipError
    with pytest.raises(E, match="k \\+ 1 = 51 neighbours need at least as many points"):       # the self search's rule stays
        vcrnet_amd.search_knn(x, 50)
    with pytest.raises(E, match="max_nn \\+ 1 = 51 neighbours need at least as many points"):
        vcrnet_amd.search_radius(x, 0.5, max_nn=50)


def test_python_entry_points_refuse_what_they_cannot_run():
    import vcrnet_amd
    from vcrnet_amd import native, query
    assert vcrnet_amd.compute_point_cloud_distance is query.compute_point_cloud_distance
    assert "compute_point_cloud_distance" in vcrnet_amd.__all__ and "query" not in vcrnet_amd.__all__
    E = native.VcrHipError
    x, q = torch.zeros(2, 3, 50), torch.zeros(2, 3, 70)
    # everything in order but the device: the last refusal.  k above N and max_nn above N are served (short rows are padded)
    for call in (lambda: vcrnet_amd.search_knn(x, 20, queries=q), lambda: vcrnet_amd.search_knn(x, 62, want_d2=True, cell=0.3, queries=q),
                 lambda: vcrnet_amd.search_radius(x, 0.5, queries=q),
                 lambda: vcrnet_amd.search_radius(x, 0.5, want_d2=True, cell=0.25, capacity=400, queries=q),
                 lambda: vcrnet_amd.search_radius(x, 0.5, max_nn=62, queries=q),
                 lambda: vcrnet_amd.compute_point_cloud_distance(q, x), lambda: vcrnet_amd.compute_point_cloud_distance(q, x, want_index=True),
                 lambda: query.grid_knn(x, q, 20), lambda: query.grid_radius(x, q, 0.5, 100)):
        with pytest.raises(E, match="no CPU fallback"):
            call()
    for bad in (q.transpose(1, 2), torch.zeros(3, 70), "q", 7):
        with pytest.raises(E, match=r"search_knn: queries must be a \[B, 3, N\]"):
            vcrnet_amd.search_knn(x, 5, queries=bad)
        with pytest.raises(E, match=r"search_radius: queries must be a \[B, 3, N\]"):
            vcrnet_amd.search_radius(x, 0.5, queries=bad)
    for fn in (lambda qq: vcrnet_amd.search_knn(x, 5, queries=qq), lambda qq: vcrnet_amd.search_radius(x, 0.5, queries=qq)):
        with pytest.raises(E, match="must hold the same number of clouds, got 2 and 3"):
            fn(torch.zeros(3, 3, 70))
        with pytest.raises(E, match="queries must have 1 ... 131072 points"):
            fn(torch.zeros(2, 3, 0))
        with pytest.raises(E, match="queries must have 1 ... 131072 points"):
            fn(torch.zeros(2, 3, 131073))
    for bad in (0, -1, 63, 2.0, "3", True):
        with pytest.raises(E, match=r"k must be an integer in \[1, 62\]"):
            vcrnet_amd.search_knn(x, bad, queries=q)
        with pytest.raises(E, match=r"max_nn must be None or an integer in \[1, 62\]"):
            vcrnet_amd.search_radius(x, 0.5, max_nn=bad, queries=q)
    for bad in (0.0, -1.0, float("nan"), float("inf")):
        with pytest.raises(E, match="cell must be None"):
            vcrnet_amd.search_knn(x, 5, cell=bad, queries=q)
        with pytest.raises(E, match="cell must be None"):
            vcrnet_amd.search_radius(x, 0.5, cell=bad, queries=q)
    for bad in (0.0, -1.0, float("nan"), float("inf"), 1.9e19, "r", None):
        with pytest.raises(E, match="radius must be finite and > 0 with a finite square"):
            vcrnet_amd.search_radius(x, bad, queries=q)
    for bad in (-1, 2.5, "7", True):
        with pytest.raises(E, match="capacity must be None or an integer >= 0"):
            vcrnet_amd.search_radius(x, 0.5, capacity=bad, queries=q)
    with pytest.raises(E, match="beyond 2\\^31"):
        vcrnet_amd.search_radius(x, 0.5, capacity=1 << 30, queries=q)
    with pytest.raises(E, match="cell must be None"):
        query.grid_knn(x, q, 5, cell=-1.0)
    with pytest.raises(E, match="finite square"):
        query.grid_radius(x, q, 1.9e19, 10)
    with pytest.raises(E, match=r"compute_point_cloud_distance: src must be a \[B, 3, N\]"):
        vcrnet_amd.compute_point_cloud_distance(None, x)
    with pytest.raises(E, match=r"compute_point_cloud_distance: tgt must be a \[B, 3, N\]"):
        vcrnet_amd.compute_point_cloud_distance(q, torch.zeros(3, 50))
    with pytest.raises(E, match="tgt and src must hold the same number of clouds"):
        vcrnet_amd.compute_point_cloud_distance(torch.zeros(1, 3, 70), x)
