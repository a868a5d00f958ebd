"""The radius search without a GPU: the numpy restatement (tests/radius_restated.py) -- the walk with its strict stop against the
brute-force definition, row for row and bit for bit, ties ON the sphere, the filter's count --, the boundary of
include/vcr_hip_radius.h (prototypes against vcrnet_amd.radius.SIGNATURES, the struct against gcc's layout), every argument error
of the calls and of the Python functions, the host-only form and workspace queries, and the resource remarks of radius.hip."""
import ctypes
import os
import subprocess
import types

import numpy as np
import pytest
import torch

import boundary
import grid_restated as gr
import outlier_restated as orr
import radius_restated as rr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INCLUDE = os.path.join(ROOT, "include")
HEADER = os.path.join(INCLUDE, "vcr_hip_radius.h")
OTHERS = ("vcr_hip.h", "vcr_hip_score.h", "vcr_hip_refine.h", "vcr_hip_plane.h", "vcr_hip_voxel.h", "vcr_hip_outlier.h",
          "vcr_hip_gicp.h", "vcr_hip_fpfh.h", "vcr_hip_match.h", "vcr_hip_fgr.h", "vcr_hip_grid.h", "vcr_hip_gridnn.h",
          "vcr_hip_voxel_sort.h")
EINVAL, EWORKSPACE, EUNSUPPORTED = -1, -2, -3
ENTRY_POINTS = {"vcr_grid_radius_f32", "vcr_grid_radius_workspace_bytes", "vcr_grid_radius_form",
                "vcr_outlier_radius_grid_f32", "vcr_outlier_radius_grid_workspace_bytes", "vcr_outlier_radius_grid_form"}
KERNELS = {"radius_count_kernel", "radius_fill_kernel", "radius_order_lane_kernel"}
ROW_KERNELS = {"rows_offsets_kernel", "rows_order_kernel", "rows_pad_kernel"}      # csr_rows.h's, shared with query.hip
INSIDE = (2, 12, 70)


@pytest.fixture(scope="module")
def lib():
    import vcrnet_amd  # noqa: F401
    from vcrnet_amd import build, radius
    build.build()
    return radius.lib()


# ------------------------------------------------------------------------------------------------------------- the restatement

def test_the_definition_on_a_cloud_worked_by_hand():
    x = np.asarray([[0, 1, 1, 5, 1], [0, 0, 0, 0, 0], [0, 0, 0, 0, np.nan]], np.float32)   # 1 and 2 are copies; 4 is not finite
    got = rr.radius_rows(x, 1.0)
    assert got["count"].tolist() == [2, 2, 2, 0, 0] and got["row_start"].tolist() == [0, 2, 4, 6, 6, 6] and got["total"] == 6
    assert got["idx"].tolist() == [1, 2, 2, 0, 1, 0]                    # (d2, j): the copy at 0 first, then the point ON the sphere
    assert got["bits"].view(np.float32).tolist() == [1, 1, 0, 1, 0, 1]
    assert rr.counts_c(x, 1.0).tolist() == [3, 3, 3, 1, 0]
    assert rr.radius_rows(x, 0.999)["count"].tolist() == [0, 1, 1, 0, 0]
    wide = rr.radius_rows(x, 4.0)
    assert wide["count"].tolist() == [2, 3, 3, 2, 0] and wide["idx"][-2:].tolist() == [1, 2]
    assert rr.cut(wide, 2)["count"].tolist() == [2, 2, 2, 2, 0] and rr.cut(wide, 2)["idx"].tolist() == [1, 2, 2, 0, 1, 0, 1, 2]
    idx, bits = rr.padded(got, 8)
    assert idx.tolist() == [1, 2, 2, 0, 1, 0, -1, -1] and (bits[6:] == rr.INF_BITS).all()
    idx, bits = rr.padded(got, 5)                             # does not fit: nothing of it
    assert (idx == -1).all() and (bits == rr.INF_BITS).all()
    big = np.asarray([[3e38, -3e38, 0], [0, 0, 0], [0, 0, 0]], np.float32)                  # a d2 that overflows is no hit
    assert rr.radius_rows(big, 1e19)["count"].tolist() == [0, 0, 0]


def _radii(x, N):
    return [orr.radius_for(N, inside) for inside in INSIDE] + [rr.spanning_radius(x)]


@pytest.mark.parametrize("name", sorted(gr.RECIPES))
def test_the_walk_returns_the_definition_bit_for_bit(name):
    """Every recipe at N = 300, at the origin and moved by (1024, -512, 256); the edge of the radius (cell = 0) and every forced
    edge from "every point its own cell" to "one cell"; radii that put about 2, 12 and 70 points of a uniform cube inside, and
    one above the cloud's extent: the walk's rows are the brute force's, and at no stop did an unseen hit exist."""
    N = 300
    checks = early = 0
    for far in (False, True):
        x = gr.RECIPES[name](N, seed=N)
        x = gr.moved(x, rr.FAR) if far else x
        d2 = rr.d2_all(x)
        ok = gr.finite(x)
        for radius in _radii(x, N):
            want = rr.radius_rows(x, radius, d2=d2)
            assert (want["count"][~ok] == 0).all() and not np.isin(want["idx"], np.flatnonzero(~ok)).any()
            grids = set()
            for cell in [0.0] + gr.forced_cells(x):
                got, st = rr.walk_radius(x, radius, cell, d2=d2)
                assert rr.same(got, want), (name, far, radius, cell, st)
                assert st["violations"] == 0 and st["n"][0] * st["n"][1] * st["n"][2] <= gr.cells_budget(N), st
                checks += st["checks"]
                early += st["stopped_early"]
                grids.add(st["n"])
            assert (1, 1, 1) in grids
        span = rr.radius_rows(x, rr.spanning_radius(x), d2=d2)
        assert (span["count"][ok] == ok.sum() - 1).all()        # every finite point in every finite point's row
    print(name, "stops taken", checks, "walks that stopped before the grid's end", early)
    if name in ("random", "lattice", "flat", "clustered"):  # (tiny: every radius here spans that cloud)
        assert early > N                                       # (the stop rule is exercised, not only the exhaustion)


def test_ties_on_the_sphere_are_hits():
    """The 2^-6 lattice at radius 2^-6 -- the six face neighbours lie ON the sphere, d2 == r2 exactly -- and at
    float32(sqrt(2)) 2^-6, where r2 rounds to one side of the edge neighbours' 2 * 2^-12: whichever, the definition decides."""
    x = orr.lattice(14, 150)[0]
    d2 = rr.d2_all(x)
    for k, radius in enumerate((float(2.0 ** -6), float(np.float32(np.sqrt(2.0)) * np.float32(2.0 ** -6)))):
        r2 = rr.r2_of(radius)
        want = rr.radius_rows(x, radius, d2=d2)
        on = (d2 == r2) & ~np.eye(x.shape[1], dtype=bool)
        if k == 0:
            assert on.any() and r2 == np.float32(2.0 ** -12)
            assert want["total"] == int(on.sum()) > 0            # face neighbours alone, all of them ON the sphere
        else:
            edge = (d2 == np.float32(2.0 ** -11)) & ~np.eye(x.shape[1], dtype=bool)
            assert edge.any() and want["total"] == int(((d2 <= r2) & ~np.eye(x.shape[1], dtype=bool)).sum())
            print("sqrt(2) 2^-6: r2 - 2^-11 =", float(r2) - 2.0 ** -11, "edge neighbours are hits:", bool(r2 >= np.float32(2.0 ** -11)))
        for cell in [0.0] + gr.forced_cells(x) + [float(2.0 ** -6), float(2.0 ** -5)]:
            got, st = rr.walk_radius(x, radius, cell, d2=d2)
            assert rr.same(got, want) and st["violations"] == 0, (radius, cell, st)


@pytest.mark.parametrize("name", [n for n in orr.RADIUS_RECIPES if n not in orr.LARGE])
def test_the_count_is_the_filters(name):
    """c_i = n_i + 1 for a finite point, 0 otherwise, is vcr_outlier_radius_f32's count on every radius case of the filter's
    tests up to N = 2 049."""
    xyz, radius, _ = orr.RADIUS_RECIPES[name]()
    assert xyz.shape[2] <= 2049 and np.isfinite(rr.r2_of(radius))
    for cloud in xyz:
        assert np.array_equal(rr.counts_c(cloud, radius), orr.radius_counts(cloud, radius)), name


# ---------------------------------------------------------------------------------------------------------------- the boundary

def test_signatures_match_the_header_and_the_library_exports_them(lib):
    from vcrnet_amd import radius
    boundary.check_signatures(HEADER, radius, lib, ENTRY_POINTS)


def test_args_match_the_c_layout(tmp_path):
    import vcrnet_amd  # noqa: F401
    from vcrnet_amd import gridnn, outlier, radius
    assert set(radius.NEW_STRUCTS) == {"vcr_grid_radius_args"}
    boundary.check_layout(HEADER, types.SimpleNamespace(STRUCTS=radius.NEW_STRUCTS), tmp_path)
    assert radius.STRUCTS["vcr_outlier_radius_args"] is outlier.RadiusArgs and radius.STRUCTS["vcr_grid_nn_args"] is gridnn.GridNnArgs
    assert radius.GridRadiusArgs.idx.offset == radius.GridRadiusArgs.total.offset + 8     # the mandatory part ends behind total


def test_the_other_boundaries_are_where_they_were(lib, monkeypatch):
    """The calls live beside the thirteen headers, not in them: none mentions them, ABI 27, the same 51 prototypes; the new header
    is taken into the digests through a list of its own; the header's numbers are the module's."""
    from vcrnet_amd import build, grid, gridnn, native, outlier, radius
    assert len(OTHERS) == 13 and set(OTHERS) | {"vcr_hip_radius.h"} == {f for f in os.listdir(INCLUDE) if f.endswith(".h")}
    for h in OTHERS:
        text = open(os.path.join(INCLUDE, h)).read()
        assert "vcr_grid_radius" not in text and "vcr_outlier_radius_grid" not in text and "VCR_RADIUS" not in text, h
    assert len(native.PUBLIC) == 51 and lib.vcr_abi_version() == native.ABI_VERSION == 27
    for other in (native, grid, gridnn, outlier):
        assert not set(radius.SIGNATURES) & set(other.SIGNATURES) and not set(radius.NEW_STRUCTS) & set(other.STRUCTS)
    assert build.RADIUS_HEADERS == [HEADER]
    assert HEADER not in (build.PUBLIC_HEADERS + build.LATER_HEADERS + build.OUTLIER_HEADERS + build.GICP_HEADERS
                          + build.FPFH_HEADERS + build.MATCH_HEADERS + build.FGR_HEADERS + build.GRID_HEADERS
                          + build.GRIDNN_HEADERS + build.VOXEL_SORT_HEADERS)
    full = build.sources_sha16()
    monkeypatch.setattr(build, "RADIUS_HEADERS", [])
    assert build.sources_sha16() != full
    monkeypatch.undo()
    text = open(HEADER).read()
    for name, value in (("VCR_RADIUS_MAX_N", radius.MAX_N), ("VCR_RADIUS_CHUNK", radius.CHUNK)):
        assert "#define %s %d" % (name, value) in text, name
    assert radius.variant() == 0 and radius.variant(2, 1) == 0x12 and radius.variant(1, 2) == 0x21
    assert radius.ORDER_FORMS == {"wave": 1, "lane": 2} and radius.MAX_NN == 62


def _rd(**kw):
    from vcrnet_amd import radius
    a = radius.GridRadiusArgs()
    a.xyz, a.count, a.row_start, a.total, a.idx, a.d2 = 0x1000, 0x2000, 0x3000, 0x4000, 0x5000, 0x6000   # (never dereferenced)
    v = dict(B=2, N=1000, radius=0.1, cell=0.0, capacity=20000, variant=0)
    v.update(kw)
    for k, x in v.items():
        setattr(a, k, x)
    return a


def test_the_search_returns_its_argument_errors_without_a_gpu(lib):
    from vcrnet_amd import radius

    def codes(a):
        rc = lib.vcr_grid_radius_f32(ctypes.byref(a), 0x10000, 1 << 40, None)
        assert lib.vcr_grid_radius_workspace_bytes(ctypes.byref(a), 256) == 0
        assert lib.vcr_grid_radius_form(ctypes.byref(a), 256, None, None, None) == rc
        return rc
    assert lib.vcr_grid_radius_f32(None, None, 0, None) == EINVAL and lib.vcr_grid_radius_workspace_bytes(None, 256) == 0
    assert lib.vcr_grid_radius_form(None, 256, None, None, None) == EINVAL
    for field in ("xyz", "count", "row_start", "total"):
        a = _rd()
        setattr(a, field, None)
        assert codes(a) == EINVAL, field
    nan, inf = float("nan"), float("inf")
    for kw in (dict(B=0), dict(B=-1), dict(radius=0.0), dict(radius=-1.0), dict(radius=nan), dict(radius=inf), dict(radius=-inf),
               dict(radius=1.9e19), dict(radius=3e38),                       # finite, the square is not
               dict(cell=-1.0), dict(cell=-1e-30), dict(cell=nan), dict(cell=inf), dict(cell=-inf),
               dict(capacity=-1), dict(idx=None), dict(idx=None, d2=None, capacity=1), dict(idx=None, capacity=0),
               dict(variant=3), dict(variant=0x30), dict(variant=0x33), dict(variant=0x100), dict(variant=-1), dict(variant=1 << 30)):
        assert codes(_rd(**kw)) == EINVAL, kw
    for kw in (dict(N=0), dict(N=-5), dict(N=131073), dict(B=16384, N=131072), dict(B=3, capacity=1 << 30),
               dict(B=2, capacity=1 << 30)):
        assert codes(_rd(**kw)) == EUNSUPPORTED, kw
    size = ctypes.sizeof(radius.GridRadiusArgs)
    for bad in (0, radius.GridRadiusArgs.idx.offset - 8, size + 8):
        a = _rd()
        a.struct_bytes = bad
        assert codes(a) == EINVAL, bad
    assert lib.vcr_grid_radius_form(ctypes.byref(_rd()), -1, None, None, None) == EINVAL
    # what passes: a radius whose square is the largest finite one's neighbour, the count-only call, every variant
    for kw in (dict(radius=1.8e19), dict(radius=1e-30), dict(idx=None, d2=None, capacity=0), dict(d2=None), dict(capacity=0),
               dict(variant=0x11), dict(variant=0x22), dict(variant=0x20), dict(variant=2), dict(cell=1e-30), dict(cell=3e38),
               dict(N=1), dict(B=1, capacity=(1 << 31) - 1)):
        assert lib.vcr_grid_radius_workspace_bytes(ctypes.byref(_rd(**kw)), 256) > 0, kw


def test_the_searchs_form_and_workspace_are_host_only_and_follow_the_header(lib):
    from vcrnet_amd import grid, radius
    up = lambda v: (v + 255) & ~255                                               # noqa: E731

    def want(B, N, capacity):
        return up(64 * B) + up(4 * B * N) + up(4 * B * (grid.cells(N) + 2)) + up(16 * B * N) + up(8 * B * capacity)
    for B in (1, 2, 3, 16):
        for N, capacity in ((1, 0), (21, 20), (1000, 12000), (1000, 0), (16384, 200000), (131072, 1572864)):
            a = _rd(B=B, N=N, capacity=capacity)
            got = lib.vcr_grid_radius_workspace_bytes(ctypes.byref(a), 256)
            assert got == want(B, N, capacity) == lib.vcr_grid_radius_workspace_bytes(ctypes.byref(a), 0), (B, N, capacity)
            assert got == lib.vcr_grid_radius_workspace_bytes(ctypes.byref(a), 1)   # (the form does not depend on the device)
            for r, cell, v in ((0.1, 0.0, 0), (7.0, 0.5, 0x12), (1e-3, 0.0, 0x21)):  # ... nor on the radius, the cell, the variant
                assert lib.vcr_grid_radius_workspace_bytes(ctypes.byref(_rd(B=B, N=N, capacity=capacity, radius=r, cell=cell, variant=v)), 256) == got
            cells, queries, form, ws = radius.radius_form(B, N, capacity)
            assert (cells, queries, ws, form) == (grid.cells(N), 256, got, 1)
    count_only = _rd(idx=None, d2=None, capacity=0)
    assert lib.vcr_grid_radius_workspace_bytes(ctypes.byref(count_only), 256) == want(2, 1000, 0)
    assert radius.radius_form(2, 1000, 0, with_idx=False)[2] == 0              # nothing to order
    a = _rd()
    a.struct_bytes = radius.GridRadiusArgs.idx.offset          # the mandatory part alone: a count-only call, so capacity 0
    a.capacity = 0
    assert lib.vcr_grid_radius_workspace_bytes(ctypes.byref(a), 256) == want(2, 1000, 0)
    assert lib.vcr_grid_radius_workspace_bytes(ctypes.byref(_rd()), -1) == 0
    # the plan's form is a wave per row whatever the shape (the lane form lost every measurement); variant forces either
    assert radius.radius_form(1, 1000, 1000 * 12)[2] == 1 and radius.radius_form(1, 1000, 1000 * 500)[2] == 1
    assert radius.radius_form(1, 1000, 1000 * 12, variant=radius.variant(0, 1))[2] == 1
    assert radius.radius_form(1, 1000, 1000 * 500, variant=radius.variant(2, 2))[2] == 2
    ok = _rd()
    need = want(2, 1000, 20000)
    assert lib.vcr_grid_radius_f32(ctypes.byref(ok), None, need, None) == EINVAL
    assert lib.vcr_grid_radius_f32(ctypes.byref(ok), 0x10008, need, None) == EINVAL
    assert lib.vcr_grid_radius_f32(ctypes.byref(ok), 0x10000, need - 1, None) == EWORKSPACE


def _ol(**kw):
    from vcrnet_amd import outlier
    a = outlier.RadiusArgs()
    a.xyz, a.points, a.count, a.index, a.neighbours = 0x1000, 0x2000, 0x3000, 0x4000, 0x5000   # (never dereferenced)
    v = dict(B=2, N=1000, radius=0.1, nb_points=4, variant=0)
    v.update(kw)
    for k, x in v.items():
        setattr(a, k, x)
    return a


def test_the_filters_sibling_returns_its_argument_errors_and_its_workspace_without_a_gpu(lib):
    from vcrnet_amd import grid, gridnn, outlier, radius
    g = gridnn.grid_args

    def codes(a, gg):
        pa, pg = (ctypes.byref(a) if a is not None else None), (ctypes.byref(gg) if gg is not None else None)
        rc = lib.vcr_outlier_radius_grid_f32(pa, pg, 0x10000, 1 << 40, None)
        assert lib.vcr_outlier_radius_grid_workspace_bytes(pa, pg, 256) == 0
        assert lib.vcr_outlier_radius_grid_form(pa, pg, 256, None, None, None) == rc
        return rc
    nan, inf = float("nan"), float("inf")
    assert codes(None, g()) == EINVAL and codes(_ol(), None) == EINVAL
    for field in ("xyz", "points", "count"):
        a = _ol()
        setattr(a, field, None)
        assert codes(a, g()) == EINVAL, field
    for kw in (dict(B=0), dict(nb_points=-1), dict(radius=0.0), dict(radius=-1.0), dict(radius=nan), dict(radius=inf),
               dict(radius=1.9e19), dict(variant=1), dict(variant=outlier.variant(2))):
        assert codes(_ol(**kw), g()) == EINVAL, kw
    for gg in (g(-1.0), g(nan), g(inf), g(0.0, 3), g(0.0, -1)):
        assert codes(_ol(), gg) == EINVAL, (gg.cell, gg.order)
    for kw in (dict(N=0), dict(N=131073), dict(B=16384, N=131072)):
        assert codes(_ol(**kw), g()) == EUNSUPPORTED, kw
    bad = g()
    bad.struct_bytes = 8
    assert codes(_ol(), bad) == EINVAL
    up = lambda v: (v + 255) & ~255                                               # noqa: E731
    for B, N in ((1, 1), (2, 1000), (16, 16384), (1, 131072)):
        want = (up(64 * B) + up(4 * B * N) + up(4 * B * (grid.cells(N) + 2)) + up(16 * B * N) + up(4 * B * N)
                + up(4 * B * ((N + 255) // 256)))
        for order, taken in ((0, 1), (1, 1), (2, 2)):
            for cell in (0.0, 0.37):
                assert radius.filter_grid_form(B, N, order, cell) == (grid.cells(N), taken, 256, want), (B, N, order, cell)
    a, gg = _ol(), g()
    need = radius.filter_grid_form(2, 1000)[3]
    assert lib.vcr_outlier_radius_grid_f32(ctypes.byref(a), ctypes.byref(gg), None, need, None) == EINVAL
    assert lib.vcr_outlier_radius_grid_f32(ctypes.byref(a), ctypes.byref(gg), 0x10000, need - 1, None) == EWORKSPACE
    assert lib.vcr_outlier_radius_grid_form(ctypes.byref(a), ctypes.byref(gg), -1, None, None, None) == EINVAL
    # the scan accepts a radius whose square overflows; the grid sibling does not (the header says so)
    assert lib.vcr_outlier_radius_workspace_bytes(ctypes.byref(_ol(radius=1.9e19)), 256) > 0


def test_the_kernels_of_radius_hip_use_no_scratch_and_keep_eight_waves():
    """hipcc's remarks for the six kernels radius.hip runs behind the grid.  Its own set is the three radius_* kernels: the row
    tail is csr_rows.h's text, shared with query.hip, the five build kernels are grid.hip's (grid_build.h), the filter's tail
    outlier.hip's (outlier_tail.h), and the remarks list a kernel under the first file that compiles it.  No scratch, no VGPR or
    SGPR spill.  As recorded from the build (waves a SIMD, static LDS bytes a workgroup; none takes dynamic LDS):
      radius_count_kernel       8 waves,    0 B   (50 VGPRs)
      rows_offsets_kernel       8 waves,   32 B   (the four waves' 64-bit totals)
      radius_fill_kernel        8 waves,    0 B   (39 VGPRs)
      rows_order_kernel         8 waves, 1024 B   (VCR_RADIUS_CHUNK = 128 keys of 8 bytes; a workgroup is ONE wave)
      radius_order_lane_kernel  8 waves,    0 B
      rows_pad_kernel           8 waves,    0 B"""
    import vcrnet_amd  # noqa: F401
    from vcrnet_amd import build, radius
    build.build()
    res = build.kernel_resources()
    names = list(res)
    dem = subprocess.run(["c++filt"], input="\n".join(names), capture_output=True, text=True, check=True).stdout.splitlines()
    by_name = {d.replace("(anonymous namespace)::", "").replace("void ", "").split("(")[0]: res[n] for n, d in zip(names, dem)}
    mine = {d: v for d, v in by_name.items() if v["file"] == "radius.hip"}
    assert set(mine) == KERNELS
    assert all(by_name[d]["file"] == "query.hip" for d in ROW_KERNELS)
    mine.update({d: by_name[d] for d in ROW_KERNELS})
    for d, v in mine.items():
        print(d, v)
        assert v.get("scratch", 0) == 0 and v.get("vgpr_spill", 0) == 0 and v.get("sgpr_spill", 0) == 0, (d, v)
        assert v["occupancy"] == 8 and v["vgprs"] <= 64 and v["agprs"] == 0, (d, v)
    assert {d: v["lds"] for d, v in mine.items()} == {
        "radius_count_kernel": 0, "rows_offsets_kernel": 32, "radius_fill_kernel": 0, "rows_order_kernel": radius.CHUNK * 8,
        "radius_order_lane_kernel": 0, "rows_pad_kernel": 0}
    # what radius.hip shares keeps its owner and its resources
    assert by_name["grid_scatter_kernel"]["file"] == "grid.hip" and by_name["outlier_write_kernel"]["file"] == "outlier.hip"
    assert by_name["outlier_mark_kernel"]["file"] == by_name["outlier_offsets_kernel"]["file"] == "outlier.hip"


# ------------------------------------------------------------------------------------------------------------ the Python layer

def test_python_entry_points_refuse_what_they_cannot_run():
    import vcrnet_amd
    from vcrnet_amd import native, outlier, radius
    assert vcrnet_amd.search_radius is radius.search_radius and "search_radius" in vcrnet_amd.__all__
    assert vcrnet_amd.remove_radius_outlier is outlier.remove_radius_outlier
    E = native.VcrHipError
    x = torch.zeros(2, 3, 50)
    for kw in (dict(), dict(want_d2=True, cell=0.25, capacity=400), dict(max_nn=20), dict(max_nn=49, capacity=0)):
        with pytest.raises(E, match="no CPU fallback"):      # (the last refusal: everything else was in order)
            vcrnet_amd.search_radius(x, 0.5, **kw)
    for bad in (x.transpose(1, 2), torch.zeros(3, 50), None, "xyz"):
        with pytest.raises(E, match=r"xyz must be a \[B, 3, N\]"):
            vcrnet_amd.search_radius(bad, 0.5)
    for bad in (0.0, -1.0, float("nan"), float("inf"), 1.9e19, "r", None):
        with pytest.raises(E, match="radius must be finite and > 0 with a finite square"):
            vcrnet_amd.search_radius(x, bad)
    for bad in (0, -1, 63, 2.0, "3", True):
        with pytest.raises(E, match=r"max_nn must be None or an integer in \[1, 62\]"):
            vcrnet_amd.search_radius(x, 0.5, max_nn=bad)
    with pytest.raises(E, match="max_nn \\+ 1 = 51 neighbours need at least as many points"):
        vcrnet_amd.search_radius(x, 0.5, max_nn=50)
    for bad in (-1, 2.5, "7", True):
        with pytest.raises(E, match="capacity must be None or an integer >= 0"):
            vcrnet_amd.search_radius(x, 0.5, capacity=bad)
    with pytest.raises(E, match="beyond 2\\^31"):
        vcrnet_amd.search_radius(x, 0.5, capacity=1 << 30)
    with pytest.raises(E, match="1 ... 131072 points"):
        vcrnet_amd.search_radius(torch.zeros(1, 3, 131073), 0.5)
    for bad in (0.0, -1.0, float("nan"), float("inf")):
        with pytest.raises(E, match="cell must be None"):
            vcrnet_amd.search_radius(x, 0.5, cell=bad)
    with pytest.raises(E, match="no CPU fallback"):
        radius.grid_radius(x, 0.5, 100)
    with pytest.raises(E, match="cell must be None"):
        radius.grid_radius(x, 0.5, 100, cell=-1.0)
    with pytest.raises(E, match="no CPU fallback"):
        radius.radius_filter_grid(x, 0.5, 3)
    with pytest.raises(E, match="finite square"):
        radius.radius_filter_grid(x, 1.9e19, 3)
    # search= of the radius filter: anything but the two names raises before anything else is looked at
    for bad in ("knn", "", None, 1, "GRID"):
        with pytest.raises(E, match='remove_radius_outlier: search must be "scan" or "grid"'):
            vcrnet_amd.remove_radius_outlier(x, 4, 0.1, search=bad)
    for kw in (dict(), dict(search="scan"), dict(search="grid")):
        with pytest.raises(E, match="no CPU fallback"):
            vcrnet_amd.remove_radius_outlier(x, 4, 0.1, **kw)
    with pytest.raises(E, match="nb_points must be an integer >= 0"):
        vcrnet_amd.remove_radius_outlier(x, -1, 0.1, search="grid")
    for spec in (("radius", 4, 0.1), ("radius", 4, 0.1, "grid"), ["radius", 4, 0.1, "grid"], ("statistical", 10, 2.0)):
        with pytest.raises(E, match="no CPU fallback"):
            outlier.filter_by(spec, x)
    for spec in (("radius", 4, 0.1, "scan"), ("radius", 4, 0.1, "knn"), ("radius", 4, 0.1, "grid", 1), ("statistical", 10, 2.0, "grid"),
                 ("radius", 4), ()):
        with pytest.raises(E, match="outlier must be"):
            outlier.filter_by(spec, x)
    assert radius.SEARCHES == ("scan", "grid")
