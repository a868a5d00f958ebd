"""The grid kNN without a GPU: the boundary of include/vcr_hip_grid.h (prototypes against vcrnet_amd.grid.SIGNATURES, the struct
against gcc's layout, the exported symbols), every argument error of the call and of the Python functions, the host-only form and
workspace queries, the resource remarks of the new kernels, and the numpy restatement (tests/grid_restated.py): its exact fp32 fma
against a fractions.Fraction one, and the walk -- faces, cells by comparison, rings, the fp32 bound, the strict stop -- against the
brute-force definition, row for row and bit for bit."""
import ctypes
import os
import re
import subprocess
from fractions import Fraction

import numpy as np
import pytest
import torch

import boundary
import grid_restated as gr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INCLUDE = os.path.join(ROOT, "include")
HEADER = os.path.join(INCLUDE, "vcr_hip_grid.h")
OTHERS = ("vcr_hip.h", "vcr_hip_score.h", "vcr_hip_refine.h", "vcr_hip_plane.h", "vcr_hip_voxel.h", "vcr_hip_outlier.h",
          "vcr_hip_gicp.h", "vcr_hip_fpfh.h", "vcr_hip_match.h", "vcr_hip_fgr.h")
EINVAL, EWORKSPACE, EUNSUPPORTED = -1, -2, -3
ENTRY_POINTS = {"vcr_grid_knn_f32", "vcr_grid_knn_workspace_bytes", "vcr_grid_knn_form"}
KERNELS = {"grid_bounds_kernel", "grid_clear_kernel", "grid_count_kernel", "grid_scan_kernel", "grid_scatter_kernel",
           "grid_search_kernel"}


@pytest.fixture(scope="module")
def lib():
    import vcrnet_amd  # noqa: F401
    from vcrnet_amd import build, grid
    build.build()
    return grid.lib()


# ---------------------------------------------------------------------------------------------------------------- the boundary

def test_signatures_match_the_header_and_the_library_exports_them(lib):
    from vcrnet_amd import grid
    boundary.check_signatures(HEADER, grid, lib, ENTRY_POINTS)


def test_args_match_the_c_layout(tmp_path):
    import vcrnet_amd  # noqa: F401
    from vcrnet_amd import grid
    boundary.check_layout(HEADER, grid, tmp_path)


def test_the_other_boundaries_are_where_they_were(lib, monkeypatch):
    """The call lives beside the ten headers, not in them: none mentions it, ABI 27, the same 51 prototypes; the new header is
    taken into the digests through a list of its own; the header's numbers are the module's."""
    from vcrnet_amd import build, fgr, fpfh, gicp, grid, match, native, outlier, plane, refine, score, voxel
    assert len(OTHERS) == 10
    for h in OTHERS:
        assert "vcr_grid" not in open(os.path.join(INCLUDE, h)).read(), h
    assert len(native.PUBLIC) == 51 and lib.vcr_abi_version() == native.ABI_VERSION == 27
    for other in (native, score, refine, plane, voxel, outlier, gicp, fpfh, match, fgr):
        assert not set(grid.SIGNATURES) & set(other.SIGNATURES) and not set(grid.STRUCTS) & set(other.STRUCTS)
    assert not set(grid.SIGNATURES) & set(native.PUBLIC)
    assert build.GRID_HEADERS == [HEADER]
    assert HEADER not in (build.PUBLIC_HEADERS + build.LATER_HEADERS + build.OUTLIER_HEADERS + build.GICP_HEADERS
                          + build.FPFH_HEADERS + build.MATCH_HEADERS + build.FGR_HEADERS)
    full = build.sources_sha16()
    monkeypatch.setattr(build, "GRID_HEADERS", [])
    assert build.sources_sha16() != full
    monkeypatch.undo()
    text = open(HEADER).read()
    for name, value in (("VCR_GRID_MAX_K", grid.MAX_K), ("VCR_GRID_MAX_N", grid.MAX_N), ("VCR_GRID_QUERIES", grid.QUERIES)):
        assert "#define %s %d" % (name, value) in text, name
    assert "#define VCR_GRID_CELLS(N) (2 * (N) + 64)" in text
    assert grid.cells(1000) == gr.cells_budget(1000) == 2064 and (grid.MAX_K, gr.MAX_K) == (62, 62)


def _gd(**kw):
    from vcrnet_amd import grid
    a = grid.GridKnnArgs()
    a.xyz, a.idx, a.d2 = 0x1000, 0x2000, 0x3000             # (never dereferenced on the host)
    v = dict(B=2, N=1000, k=20, cell=0.0, variant=0)
    v.update(kw)
    for k, x in v.items():
        setattr(a, k, x)
    return a


def test_argument_errors_return_their_codes_without_a_gpu(lib):
    from vcrnet_amd import grid

    def codes(a):
        rc = lib.vcr_grid_knn_f32(ctypes.byref(a), 0x10000, 1 << 40, None)
        assert lib.vcr_grid_knn_workspace_bytes(ctypes.byref(a), 256) == 0
        assert lib.vcr_grid_knn_form(ctypes.byref(a), 256, None, None) == rc
        return rc
    assert lib.vcr_grid_knn_f32(None, None, 0, None) == EINVAL and lib.vcr_grid_knn_workspace_bytes(None, 256) == 0
    assert lib.vcr_grid_knn_form(None, 256, None, None) == EINVAL
    for field in ("xyz", "idx"):
        a = _gd()
        setattr(a, field, None)
        assert codes(a) == EINVAL, field
    nan, inf = float("nan"), float("inf")
    for kw in (dict(B=0), dict(B=-1), dict(cell=-1.0), dict(cell=-1e-30), dict(cell=nan), dict(cell=inf), dict(cell=-inf),
               dict(variant=3), dict(variant=15), dict(variant=0x100), dict(variant=-1), dict(variant=1 << 4)):
        assert codes(_gd(**kw)) == EINVAL, kw
    for kw in (dict(N=0), dict(N=-5), dict(N=131073), dict(B=16384, N=131072), dict(k=0), dict(k=-1), dict(k=63)):
        assert codes(_gd(**kw)) == EUNSUPPORTED, kw
    size = ctypes.sizeof(grid.GridKnnArgs)
    for bad in (0, grid.GridKnnArgs.d2.offset - 8, size + 8):
        a = _gd()
        a.struct_bytes = bad
        assert codes(a) == EINVAL, bad
    assert lib.vcr_grid_knn_form(ctypes.byref(_gd()), -1, None, None) == EINVAL


def test_the_form_and_workspace_queries_are_host_only_and_say_what_the_call_holds(lib):
    from vcrnet_amd import grid
    up = lambda v: (v + 255) & ~255                                               # noqa: E731

    def want(B, N):
        return up(64 * B) + up(4 * B * N) + up(4 * B * (grid.cells(N) + 2)) + up(16 * B * N)
    last = 0
    for B in (1, 2, 3, 16, 100):
        for N, k in ((1, 1), (21, 20), (1000, 20), (1000, 62), (16384, 30), (131072, 1)):
            a = _gd(B=B, N=N, k=k)
            got = lib.vcr_grid_knn_workspace_bytes(ctypes.byref(a), 256)
            assert got == want(B, N) == lib.vcr_grid_knn_workspace_bytes(ctypes.byref(a), 0), (B, N, k)
            assert got == lib.vcr_grid_knn_workspace_bytes(ctypes.byref(a), 1)   # (the form does not depend on the device)
            assert grid.grid_form(B, N, k) == (grid.cells(N), 256, got)
        now = lib.vcr_grid_knn_workspace_bytes(ctypes.byref(_gd(B=B)), 256)
        assert now > last                                                         # monotone in B
        last = now
    a = _gd()
    a.struct_bytes = grid.GridKnnArgs.d2.offset                # the mandatory part alone
    assert lib.vcr_grid_knn_workspace_bytes(ctypes.byref(a), 256) == want(2, 1000)
    assert lib.vcr_grid_knn_workspace_bytes(ctypes.byref(_gd()), -1) == 0
    cells, queries = ctypes.c_int(0), ctypes.c_int(0)
    assert lib.vcr_grid_knn_form(ctypes.byref(_gd(variant=2)), 256, ctypes.byref(cells), ctypes.byref(queries)) == 0
    assert (cells.value, queries.value) == (2064, 256)
    ok = _gd()
    need = want(2, 1000)
    assert lib.vcr_grid_knn_f32(ctypes.byref(ok), None, need, None) == EINVAL
    assert lib.vcr_grid_knn_f32(ctypes.byref(ok), 0x10008, need, None) == EINVAL
    assert lib.vcr_grid_knn_f32(ctypes.byref(ok), 0x10000, need - 1, None) == EWORKSPACE
    for kw in (dict(cell=1e-30), dict(cell=3e38), dict(variant=1), dict(variant=2), dict(k=62), dict(N=1),
               dict(N=5, k=20)):
        assert lib.vcr_grid_knn_workspace_bytes(ctypes.byref(_gd(**kw)), 256) > 0, kw


def test_the_new_kernels_use_no_scratch_and_the_search_keeps_its_occupancy():
    """No scratch anywhere.  The search kernel's registers leave room for 8 waves a SIMD (the compiler's remark), so what bounds
    its residency is the rows' LDS alone: k * 256 * 8 bytes of dynamic LDS a workgroup (none static) -- 4 workgroups a CU at
    k = 20, 2 at k = 30, 1 at k = 62 of the CU's 160 KiB."""
    import vcrnet_amd  # noqa: F401
    from vcrnet_amd import build
    build.build()
    res = build.kernel_resources()
    names = list(res)
    dem = subprocess.run(["c++filt"], input="\n".join(names), capture_output=True, text=True, check=True).stdout.splitlines()
    mine = {d.replace("(anonymous namespace)::", "").replace("void ", "").split("(")[0]: res[n]
            for n, d in zip(names, dem) if res[n]["file"] == "grid.hip"}
    assert set(mine) == KERNELS
    for d, v in mine.items():
        print(d, v)
        assert v.get("scratch", 0) == 0 and v.get("vgpr_spill", 0) == 0 and v.get("sgpr_spill", 0) == 0, (d, v)
    s = mine["grid_search_kernel"]
    assert s["occupancy"] == 8 and s["vgprs"] <= 64 and s["agprs"] == 0 and s["sgprs"] <= 80 and s["lds"] == 0
    lds = 160 * 1024
    assert [lds // (k * 256 * 8) for k in (20, 30, 62)] == [4, 2, 1]
    assert mine["grid_scan_kernel"]["lds"] == 16 and mine["grid_bounds_kernel"]["lds"] == 96
    assert mine["grid_count_kernel"]["lds"] == mine["grid_scatter_kernel"]["lds"] == mine["grid_clear_kernel"]["lds"] == 0


def test_the_ring_walk_is_written_once():
    """Every search on the grid walks grid_walk.h's rings: among the kernel sources and their headers the enumeration -- rmax, the
    shell test -- and the faces of the ring bound stand in that header alone, and the four searches include it."""
    csrc = os.path.join(ROOT, "vcr-net_amd", "csrc")
    text = {f: open(os.path.join(csrc, f)).read() for f in sorted(os.listdir(csrc)) if f.endswith((".hip", ".h"))}
    assert [f for f, t in text.items() if re.search(r"\b(rmax|shell)\b", t)] == ["grid_walk.h"]
    assert [f for f, t in text.items() if "gd_face(" in t] == ["grid_build.h", "grid_walk.h"]      # (the faces decide the cells too)
    for f in ("grid.hip", "gridnn.hip", "radius.hip", "query.hip"):
        assert '#include "grid_walk.h"' in text[f], f


# ------------------------------------------------------------------------------------------------------------- the restatement

def _round32(v):
    """A Fraction rounded once to fp32, ties to even, by exact comparison with the candidates around it."""
    c = np.float32(float(v))
    cands = [np.nextafter(c, np.float32(-np.inf)), c, np.nextafter(c, np.float32(np.inf))]
    best = min(cands, key=lambda x: (abs(Fraction(float(x)) - v), int(np.float32(x).view(np.uint32)) & 1))
    return np.float32(best)


def test_the_exact_fp32_fma_is_the_rational_one():
    rs = np.random.RandomState(5)
    n = 6000

    def draw():
        return (rs.uniform(1, 2, n) * 2.0 ** rs.randint(-20, 21, n) * rs.choice([-1, 1], n)).astype(np.float32)
    a, b, c = draw(), draw(), draw()
    c[:1500] = -(a[:1500] * b[:1500])                        # cancellation: the result is the product's own rounding error
    c[1500:2500] = (a[1500:2500] * b[1500:2500]) * np.float32(2.0) ** rs.randint(-3, 4, 1000).astype(np.float32)
    # sums that sit on an fp32 tie of the two-step (fp64, then fp32) form: c = 2^24 + 2 m + 1 ulps apart, a b tiny
    m = rs.randint(0, 2 ** 22, 1000)
    c[2500:3500] = (2.0 ** 24 + 2.0 * m).astype(np.float32)
    a[2500:3500] = np.float32(1.0) + rs.randint(1, 100, 1000).astype(np.float32) * np.float32(2.0 ** -23)
    b[2500:3500] = np.float32(1.0) * rs.choice([-1, 1], 1000).astype(np.float32)
    got = gr.fmaf32(a, b, c)
    want = np.asarray([_round32(Fraction(float(x)) * Fraction(float(y)) + Fraction(float(z))) for x, y, z in zip(a, b, c)])
    assert got.dtype == np.float32 and np.array_equal(got.view(np.int32), want.view(np.int32))
    assert (got[:1500] != 0).mean() > 0.5 and (got != a * b + c).mean() > 0.1      # (an fma, not two roundings)
    # the double rounding the odd-neighbour step is there for: 1 + 2^-24 + 2^-60 lies ABOVE the tie
    tie = gr.fmaf32(np.float32(2.0 ** -30), np.float32(2.0 ** -30), np.float32(1.0))
    assert tie == np.float32(1.0)
    a1, b1, c1 = np.float32(2.0 ** -12 + 2.0 ** -35), np.float32(2.0 ** -12), np.float32(1.0)
    exact = Fraction(float(a1)) * Fraction(float(b1)) + 1               # 1 + 2^-24 + 2^-47: above the tie 1 + 2^-24
    assert gr.fmaf32(a1, b1, c1) == _round32(exact) == np.nextafter(np.float32(1), np.float32(2))
    assert np.float32(np.float64(a1) * np.float64(b1) + 1.0) == _round32(exact)    # (fp64 still sees 2^-47)
    a2 = np.float32(2.0 ** -12 + 2.0 ** -34)
    b2 = np.float32(2.0 ** -12 + 2.0 ** -34)                 # a2 b2 = 2^-24 + 2^-45 + 2^-68: 2^-68 is below fp64's ulp at 1
    exact = Fraction(float(a2)) * Fraction(float(b2)) + 1
    assert gr.fmaf32(a2, b2, c1) == _round32(exact)
    assert gr.fmaf32(2.0, 3.0, 1.0) == 7.0 and gr.fmaf32(np.ones(3), np.ones(3), 0.0).shape == (3,)


def test_the_definition_on_a_cloud_worked_by_hand():
    x = np.asarray([[0, 1, 1, 5, 1], [0, 0, 0, 0, 0], [0, 0, 0, 0, np.nan]], np.float32)   # 1 and 2 are copies; 4 is not finite
    idx, bits = gr.knn(x, 3)
    d2 = bits.view(np.float32)
    assert idx.tolist() == [[1, 2, 3], [2, 0, 3], [1, 0, 3], [1, 2, 0], [4, 4, 4]]
    assert d2[0].tolist() == [1, 1, 25] and d2[1].tolist() == [0, 1, 16] and d2[3].tolist() == [16, 16, 25]
    assert np.isinf(d2[4]).all()
    idx, bits = gr.knn(x, 5)                                  # k + 1 > N: the own index and +inf behind the candidates
    assert idx[0].tolist() == [1, 2, 3, 0, 0] and np.isinf(bits.view(np.float32)[0, 3:]).all()
    big = np.asarray([[3e38, -3e38, 3e38, 0], [0, 0, 0, 0], [0, 0, 0, 0]], np.float32)   # a d2 that overflows: no candidate
    idx, bits = gr.knn(big, 2)
    assert idx.tolist() == [[2, 0], [1, 1], [0, 2], [3, 3]] and bits[0].tolist() == [0, gr.INF_BITS]


CASES = [(name, N, k) for name in gr.RECIPES for N, k in ((300, 20), (97, 7))] + [("random", 5, 20), ("lattice", 9, 62),
                                                                                   ("random", 1, 1), ("copies", 64, 62)]


@pytest.mark.parametrize("name,N,k", CASES)
def test_the_walk_returns_the_definition_bit_for_bit(name, N, k):
    """Every recipe at the origin and moved by 1024, the automatic grid and every forced edge from "every point its own cell"
    to "one cell": the walk's rows are the brute force's, and no bound it took was undercut by a point it had not seen."""
    checks = early = 0
    for offset in (0.0, 1024.0):
        x = gr.RECIPES[name](N, seed=N + k)
        x = gr.moved(x, offset) if offset else x
        want_idx, want_bits = gr.knn(x, k)
        assert want_idx.min() >= 0 and want_idx.max() < N
        grids = set()
        for cell in [0.0] + gr.forced_cells(x):
            idx, bits, st = gr.walk(x, k, cell)
            assert np.array_equal(idx, want_idx) and np.array_equal(bits, want_bits), (name, offset, cell, st)
            assert st["violations"] == 0 and st["n"][0] * st["n"][1] * st["n"][2] <= gr.cells_budget(N), st
            checks += st["checks"]
            early += st["stopped_early"]
            grids.add(st["n"])
        assert (1, 1, 1) in grids and (len(grids) >= 3 or name == "equal" or N == 1), grids
    print(name, N, k, "bounds taken", checks, "walks that stopped before the grid's end", early)
    if name in ("random", "lattice", "flat", "tiny", "clustered") and N >= 97:
        assert early > N                                     # (the prune rule is exercised, not only the exhaustion)


def test_the_grid_of_the_edge_cases():
    f32 = np.float32
    lo, h, n = gr.make_grid(gr.flat(300))
    assert n[2] == 1 and n[0] > 1 and n[1] > 1                # one cell across the flat axis
    assert gr.make_grid(gr.collinear(300))[2][1:] == [1, 1]
    assert gr.make_grid(gr.equal(300))[2] == [1, 1, 1]
    assert gr.make_grid(np.full((3, 4), np.nan, f32))[2] == [1, 1, 1]
    lo, h, n = gr.make_grid(gr.random_cloud(300), cell=1e-6)   # far too fine: widened until it fits, never an error
    assert h > 1e-6 and n[0] * n[1] * n[2] <= gr.cells_budget(300) < (n[0] + 1) * (n[1] + 1) * (n[2] + 1) * 2
    lo, h, n = gr.make_grid(np.asarray([[-3e38, 3e38], [0, 1], [0, 0]], f32))     # an extent that overflows
    assert np.isfinite(h) and n[0] * n[1] * n[2] <= gr.cells_budget(2)
    # cells by comparison: a point ON a face belongs to the cell above it; the last cell is open above
    face = gr.faces(f32(0), f32(1), 4)
    assert face.tolist() == [0, 1, 2, 3, 4]
    assert gr.cells_of(np.asarray([0, 0.5, 1, 2.9999, 3, 4, 7], f32), face, 4).tolist() == [0, 0, 1, 2, 3, 3, 3]
    far = gr.faces(f32(1024), f32(1e-5), 50)                  # an edge below the offset's ulp: faces repeat, still monotone
    assert (np.diff(far) >= 0).all() and len(set(far.tolist())) < 51


# ------------------------------------------------------------------------------------------------------------ the Python layer

def test_python_entry_points_refuse_what_they_cannot_run():
    import vcrnet_amd
    from vcrnet_amd import grid, native
    assert vcrnet_amd.search_knn is grid.search_knn and "search_knn" in vcrnet_amd.__all__
    E = native.VcrHipError
    x = torch.zeros(2, 3, 50)
    with pytest.raises(E, match="no CPU fallback"):          # (the last refusal: everything else was in order)
        vcrnet_amd.search_knn(x, 20)
    with pytest.raises(E, match="no CPU fallback"):
        vcrnet_amd.search_knn(x, 49, want_d2=True, cell=0.25)
    for bad in (x.transpose(1, 2), torch.zeros(3, 50), None, "xyz"):
        with pytest.raises(E, match=r"xyz must be a \[B, 3, N\]"):
            vcrnet_amd.search_knn(bad, 5)
    for bad in (0, -1, 63, 2.0, "3", None, True):
        with pytest.raises(E, match=r"k must be an integer in \[1, 62\]"):
            vcrnet_amd.search_knn(x, bad)
    with pytest.raises(E, match="k \\+ 1 = 51 neighbours need at least as many points"):
        vcrnet_amd.search_knn(x, 50)
    with pytest.raises(E, match="1 ... 131072 points"):
        vcrnet_amd.search_knn(torch.zeros(1, 3, 131073), 5)
    for bad in (0.0, -1.0, float("nan"), float("inf")):
        with pytest.raises(E, match="cell must be None"):
            vcrnet_amd.search_knn(x, 5, cell=bad)
    with pytest.raises(E, match="no CPU fallback"):
        grid.grid_knn(x, 5)
    with pytest.raises(E, match="cell must be None"):
        grid.grid_knn(x, 5, cell=-1.0)
    # search= of the consumers: anything but the two names raises before anything else is looked at; the names pass it on
    calls = (("estimate_normals", lambda **kw: vcrnet_amd.estimate_normals(x, 10, **kw)),
             ("compute_fpfh_feature", lambda **kw: vcrnet_amd.compute_fpfh_feature(x, None, 10, **kw)),
             ("remove_statistical_outlier", lambda **kw: vcrnet_amd.remove_statistical_outlier(x, 10, 2.0, **kw)),
             ("register_features", lambda **kw: vcrnet_amd.register_features(x, x, 0.05, **kw)),
             ("register_features", lambda **kw: vcrnet_amd.register_features(x, x, 0.05, method="fgr", **kw)),
             ("register_features", lambda **kw: vcrnet_amd.register_features(x, x, 0.05, centre=True, **kw)))
    for api, fn in calls:
        for bad in ("brute", "", None, 1, "GRID"):
            with pytest.raises(E, match=api + ': search must be "knn" or "grid"'):
                fn(search=bad)
        for good in ("knn", "grid"):
            with pytest.raises(E, match="no CPU fallback"):
                fn(search=good)
        with pytest.raises(E, match="no CPU fallback"):
            fn()
    assert grid.SEARCHES == ("knn", "grid")
    assert grid.variant() == 0 and grid.variant(2) == 2
