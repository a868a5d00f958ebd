"""DBSCAN over ragged rows without a GPU: the numpy restatement (tests/dbscan_restated.py) -- its sequential definition against
its vectorised form, both against scikit-learn's DBSCAN on the definition's distances, a cloud worked by hand, caller-built rows
-- the recipe of the GPU test (what it must contain), the boundary of include/cluster/vcr_hip_dbscan.h (prototypes against
vcrnet_amd.dbscan.SIGNATURES, the structs against gcc's layout), every argument error of the calls and of the Python functions,
the host-only form query, and the resource remarks of dbscan.hip."""
import ctypes
import functools
import os
import subprocess

import numpy as np
import pytest
import torch

import boundary
import dbscan_restated as dr
import fpfh_restated as fr
import grid_restated as gr
import outlier_restated as orr
import radius_restated as rr
import rows_restated as wr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INCLUDE = os.path.join(ROOT, "include")
HEADER = os.path.join(INCLUDE, "cluster", "vcr_hip_dbscan.h")
EINVAL, EUNSUPPORTED = -1, -3
ENTRY_POINTS = {"vcr_rows_dbscan_workspace_bytes", "vcr_rows_dbscan_f32", "vcr_rows_dbscan_form",
                "vcr_cluster_largest_workspace_bytes", "vcr_cluster_largest_f32"}
KERNELS = {"dbscan_check_kernel", "dbscan_served_kernel", "dbscan_core_kernel<1>", "dbscan_core_kernel<2>", "dbscan_hook_kernel<1>", "dbscan_hook_kernel<2>",
           "dbscan_flatten_kernel", "dbscan_offsets_kernel", "dbscan_rank_kernel", "dbscan_label_kernel<1>", "dbscan_label_kernel<2>",
           "largest_pick_kernel", "largest_member_kernel"}
RECIPES = ("random", "copies", "nonfinite", "flat", "lattice")
MIN_POINTS = (1, 4, 6)                                      # what every recipe runs at


@pytest.fixture(scope="module")
def lib():
    import vcrnet_amd  # noqa: F401
    from vcrnet_amd import build, dbscan
    build.build()
    return dbscan.lib()


def recipe_radius(name, N):
    return 1.5 if name == "lattice" else orr.radius_for(N, 12)        # tests/test_rows_cpu.py's radii (the lattice's spacing is 1)


@functools.lru_cache(maxsize=None)
def cases():
    """Every (name, cloud [3,N], radius, d2) of the GPU test's small recipes: computed once, read-only."""
    out = []
    for N in (60,):
        for name in RECIPES:
            x = gr.RECIPES[name](N, seed=N)
            out.append(("%s-%d" % (name, N), x, recipe_radius(name, N), rr.d2_all(x)))
    B, N = wr.RAGGED
    X = fr.cloud(B, N)
    for b in range(B):
        d2 = rr.d2_all(X[b])
        for radius in wr.RAGGED_RADII:
            out.append(("torus-%d-%g" % (b, radius), X[b], radius, d2))
    for _, x, _, d2 in out:
        x.setflags(write=False)
        d2.setflags(write=False)
    return tuple(out)


def padded(want, N):
    sizes = np.zeros(N, np.int32)
    sizes[:len(want["sizes"])] = want["sizes"]
    return {"labels": np.asarray(want["labels"], np.int32), "core": np.asarray(want["core"], np.int32),
            "n_clusters": want["n_clusters"], "sizes": sizes}


# ------------------------------------------------------------------------------------------------------------- the restatement

def test_the_two_restatements_agree_on_every_recipe_and_the_recipe_holds_what_the_gpu_test_needs():
    """The sequential definition labels EVERY point of every recipe (the cap on excluded points is 0) and the vectorised form
    returns the same.  Together the recipes hold a cloud with three clusters or more, a contested border point, a noise point,
    rows of 0, 1, 63, 64, 65 and more than 255 entries, and the spanning radius gives exactly one cluster of N."""
    lens, most, n_contested, n_noise, points = set(), 0, 0, 0, 0
    for name, x, radius, d2 in cases():
        N = x.shape[1]
        for mp in MIN_POINTS:
            a, rows = dr.of_cloud(x, radius, mp, dr.sequential, d2)
            b, _ = dr.of_cloud(x, radius, mp, dr.vectorised, d2)
            assert dr.same(a, b), (name, mp)
            assert a["labels"].shape == (N,) and a["labels"].min() >= -1 and a["labels"].max() == a["n_clusters"] - 1
            assert a["sizes"].sum() == (a["labels"] >= 0).sum() and (a["sizes"][:a["n_clusters"]] > 0).all()
            assert (a["labels"][a["core"] == 1] >= 0).all() and (a["labels"][~gr.finite(x)] == -1).all()
            points += N
            lens |= set(rows["count"].tolist())
            most = max(most, a["n_clusters"])
            n_contested += len(dr.contested(rows["idx"], rows["row_start"], N, a))
            n_noise += int(((a["labels"] == -1) & gr.finite(x)).sum())
            if name.startswith("torus") and radius == wr.RAGGED_RADII[-1]:
                assert a["n_clusters"] == 1 and a["sizes"][0] == N and (rows["count"] == N - 1).all(), (name, mp)
    print("points labelled", points, "most clusters", most, "contested", n_contested, "noise", n_noise)
    assert most >= 3 and n_contested >= 1 and n_noise >= 1
    assert {0, 1, 63, 64, 65} <= lens and max(lens - {wr.RAGGED[1] - 1}) > 255, sorted(lens)


def test_both_restatements_equal_scikit_learn_on_the_finite_recipes():
    """sklearn.cluster.DBSCAN(metric="precomputed") on the definition's fp32 d2 with eps = r2: its labels number the clusters
    in the order its sequential loop meets them, which is the lowest core index's; its core_sample_indices_ are the core set."""
    cluster = pytest.importorskip("sklearn.cluster")
    seen = 0
    for name, x, radius, d2 in cases() + (("hand", dr.hand_cloud()[:, :11], dr.HAND_EPS, None),):
        if not gr.finite(x).all():
            continue
        d2 = rr.d2_all(x) if d2 is None else d2
        N = x.shape[1]
        for mp in MIN_POINTS:
            sk = cluster.DBSCAN(eps=float(rr.r2_of(radius)), min_samples=mp, metric="precomputed").fit(d2.astype(np.float64))
            core = np.zeros(N, np.int32)
            core[sk.core_sample_indices_] = 1
            for form in (dr.sequential, dr.vectorised):
                got, _ = dr.of_cloud(x, radius, mp, form, d2)
                assert np.array_equal(got["labels"], sk.labels_) and np.array_equal(got["core"], core), (name, mp, form.__name__)
            seen += 1
    assert seen >= 30


def test_a_cloud_worked_by_hand():
    """dbscan_restated.hand_cloud: a cluster whose lowest member is a border point and whose lowest core index comes behind the
    other cluster's; a border point two clusters reach; noise; copies; a non-finite point; min_points = 1 and min_points > N."""
    x = dr.hand_cloud()
    N = x.shape[1]
    rows = rr.radius_rows(x, dr.HAND_EPS)
    assert rows["idx"][rows["row_start"][7]:rows["row_start"][8]].tolist() == [5, 6]      # cluster 1's core point comes first
    assert rows["count"][11] == 0 and 11 not in rows["idx"]
    assert 3 in rows["idx"][rows["row_start"][2]:rows["row_start"][3]]                    # the copy at d2 = 0 is a neighbour
    for mp, want in dr.HAND_WANT.items():
        for form in (dr.sequential, dr.vectorised):
            got = form(rows["idx"], rows["row_start"], N, mp, gr.finite(x))
            assert dr.same(got, padded(want, N)), (mp, form.__name__, got)
    got = dr.sequential(rows["idx"], rows["row_start"], N, dr.HAND_MIN_POINTS, gr.finite(x))
    assert dr.contested(rows["idx"], rows["row_start"], N, got).tolist() == [7]
    # without the copy's d2 = 0 entry point 2 would fall short of min_points
    assert got["core"][2] == 1 and rows["count"][2] + 1 == dr.HAND_MIN_POINTS
    points, count, index = dr.largest(x, got)
    assert count == 5 and index[:5].tolist() == [2, 3, 4, 6, 7] and np.isnan(points[:, 5:]).all()     # a tie: the lower label
    assert dr.largest(x, dr.sequential(rows["idx"], rows["row_start"], N, 13, gr.finite(x)))[1] == 0   # no cluster


def test_caller_built_rows_on_the_restatement():
    """Rows need not be symmetric: the closure is the definition.  -1, an index past N and the row's own index are ignored --
    they neither count nor link; an empty row."""
    N = 7
    # 0 names 1 (1 does not name 0), 2 names 1: with min_points = 1 all three are one component through one-sided entries;
    # 3's row holds only ignored entries; 4 is empty; 5 names 6 twice (counted twice), 6 names nobody
    rows = [[1], [], [1], [-1, 3, 99, N], [], [6, 6], []]
    idx = np.asarray([e for r in rows for e in r] + [0, 0], np.int32)                # (two slots behind total: never read)
    row_start = np.cumsum([0] + [len(r) for r in rows]).astype(np.int64)
    for form in (dr.sequential, dr.vectorised):
        got = form(idx, row_start, N, 1)
        assert got["labels"].tolist() == [0, 0, 0, 1, 2, 3, 3] and got["n_clusters"] == 4, form.__name__
        # min_points = 2: 0, 2 and 5 are core (one entry that counts, or two); 1 and 6 are not and their rows are empty, so
        # nothing of their own reaches a core point: noise.  3's four entries count for nothing
        got = form(idx, row_start, N, 2)
        assert got["core"].tolist() == [1, 0, 1, 0, 0, 1, 0] and got["labels"].tolist() == [0, -1, 1, -1, -1, 2, -1], form.__name__
        got = form(idx, row_start, N, 3)
        assert got["core"].tolist() == [0, 0, 0, 0, 0, 1, 0] and got["n_clusters"] == 1, form.__name__
    # a border point's label comes from ITS OWN row: 1 names the core point 0, 2 (not core) is named by it and names nobody
    rows = [[1, 2, 3], [0], [], [0, 4, 5], [3, 5, 6], [3, 4], [4]]
    idx = np.asarray([e for r in rows for e in r], np.int32)
    row_start = np.cumsum([0] + [len(r) for r in rows]).astype(np.int64)
    for form in (dr.sequential, dr.vectorised):
        got = form(idx, row_start, N, 4)
        assert got["core"].tolist() == [1, 0, 0, 1, 1, 0, 0] and got["labels"].tolist() == [0, 0, -1, 0, 0, 0, 0], form.__name__
    assert dr.served(row_start, int(row_start[-1]), len(idx)) and not dr.served(row_start, int(row_start[-1]), len(idx) - 1)
    bad = row_start.copy()
    bad[3] = bad[4] + 1
    assert not dr.served(bad, int(bad[-1]), 100) and not dr.served(row_start + 1, int(row_start[-1]) + 1, 100)


def test_the_path_recipes():
    """The union-find's worst case as the definition sees it: one cluster, and eight numbered by their lowest index."""
    for cuts in ((), dr.SHORT_PATH_CUTS):
        x, perm = dr.path(256, cuts)
        want = dr.path_want(256, perm, cuts)
        for form in (dr.sequential, dr.vectorised):
            got, _ = dr.of_cloud(x, 1.0, 2, form)
            assert np.array_equal(got["labels"], want) and got["n_clusters"] == len(cuts) + 1 and got["core"].all()
    x, perm = dr.path(4096, dr.PATH_CUTS)
    want = dr.path_want(4096, perm, dr.PATH_CUTS)
    assert want.max() == 7 and sorted(set(np.diff(np.sort(x[0])).tolist())) == [1.0, 3.0]


# ---------------------------------------------------------------------------------------------------------------- the boundary

def test_signatures_match_the_header_and_the_library_exports_them(lib):
    from vcrnet_amd import dbscan
    boundary.check_signatures(HEADER, dbscan, lib, ENTRY_POINTS)


def test_args_match_the_c_layout(tmp_path):
    import vcrnet_amd  # noqa: F401
    from vcrnet_amd import dbscan
    assert set(dbscan.STRUCTS) == {"vcr_rows_dbscan_args", "vcr_cluster_largest_args"}
    boundary.check_layout(HEADER, dbscan, tmp_path)
    A, G = dbscan.RowsDbscanArgs, dbscan.ClusterLargestArgs
    assert A.core.offset == A.n_clusters.offset + 8 and G.index.offset == G.count.offset + 8     # where the mandatory parts end


def test_the_header_lives_in_a_directory_of_its_own_and_enters_the_digests(lib, monkeypatch):
    """include/*.h and include/ext/ are what they were, none of those headers mentions the new calls, ABI 27 and the same 51
    prototypes; the header enters the digests through a list of its own; its numbers are the module's."""
    from vcrnet_amd import build, dbscan, native, outlier, radius, rows
    others = sorted(f for f in os.listdir(INCLUDE) if f.endswith(".h"))
    assert len(others) == 14 and os.listdir(os.path.join(INCLUDE, "ext")) == ["vcr_hip_rows.h"]
    assert os.listdir(os.path.join(INCLUDE, "cluster")) == ["vcr_hip_dbscan.h"]
    for h in [os.path.join(INCLUDE, f) for f in others] + build.ROWS_HEADERS:
        text = open(h).read()
        assert "dbscan" not in text.lower() and "vcr_cluster_" not in text, h
    assert '#include "../vcr_hip.h"' in open(HEADER).read()
    assert len(native.PUBLIC) == 51 and lib.vcr_abi_version() == native.ABI_VERSION == 27
    for other in (native, outlier, radius, rows):
        assert not set(dbscan.SIGNATURES) & set(other.SIGNATURES) and not set(dbscan.STRUCTS) & set(other.STRUCTS)
    assert build.DBSCAN_HEADERS == [HEADER]
    assert HEADER not in (build.PUBLIC_HEADERS + build.LATER_HEADERS + build.OUTLIER_HEADERS + build.GICP_HEADERS
                          + build.FPFH_HEADERS + build.MATCH_HEADERS + build.FGR_HEADERS + build.GRID_HEADERS
                          + build.GRIDNN_HEADERS + build.VOXEL_SORT_HEADERS + build.RADIUS_HEADERS + build.ROWS_HEADERS)
    full = build.sources_sha16()
    monkeypatch.setattr(build, "DBSCAN_HEADERS", [])
    assert build.sources_sha16() != full
    monkeypatch.undo()
    text = open(HEADER).read()
    for name, value in (("VCR_DBSCAN_MAX_N", dbscan.MAX_N), ("VCR_DBSCAN_LANE", dbscan.FORMS["lane"]),
                        ("VCR_DBSCAN_WAVE", dbscan.FORMS["wave"]), ("VCR_DBSCAN_WAVE_HOOK", dbscan.WAVE_HOOK),
                        ("VCR_DBSCAN_WAVE_LABEL", dbscan.WAVE_LABEL)):
        assert "#define %s %d" % (name, value) in text, name
    assert "#define VCR_DBSCAN_NOISE (%d)" % dbscan.NOISE in text and "#define VCR_DBSCAN_NOT_SERVED (%d)" % dbscan.NOT_SERVED in text


def _args(kind="dbscan", **kw):
    from vcrnet_amd import dbscan
    a = {"dbscan": dbscan.RowsDbscanArgs, "largest": dbscan.ClusterLargestArgs}[kind]()
    for k, f in enumerate(n for n, t in a._fields_ if t is ctypes.c_void_p):       # (never dereferenced)
        setattr(a, f, 0x1000 * (k + 1))
    v = dict(B=2, N=1000, capacity=20000, min_points=4) if kind == "dbscan" else dict(B=2, N=1000)
    v.update(kw)
    for k, x in v.items():
        setattr(a, k, x)
    return a


WS = 0x100000                                               # a 256-aligned address that is never dereferenced


def test_the_dbscan_call_returns_its_argument_errors_without_a_gpu(lib):
    need = lambda a: lib.vcr_rows_dbscan_workspace_bytes(ctypes.byref(a), 0)       # noqa: E731
    f32 = lambda a, ws=WS, n=None: lib.vcr_rows_dbscan_f32(ctypes.byref(a), ws, need(_args()) if n is None else n, None)  # noqa: E731
    assert lib.vcr_rows_dbscan_f32(None, WS, 1 << 30, None) == EINVAL and lib.vcr_rows_dbscan_workspace_bytes(None, 0) == 0
    for field in ("row_start", "total", "labels", "n_clusters", "idx"):
        assert f32(_args(**{field: None})) == EINVAL and need(_args(**{field: None})) == 0, field
    assert need(_args(idx=None, capacity=0)) > 0 and need(_args(xyz=None, core=None, sizes=None)) == need(_args()) > 0
    for kw in (dict(B=0), dict(B=-1), dict(capacity=-1), dict(min_points=0), dict(min_points=-3), dict(variant=3), dict(variant=-1),
               dict(variant=0x10)):
        assert f32(_args(**kw)) == EINVAL and need(_args(**kw)) == 0, kw
    for kw in (dict(N=0), dict(N=-5), dict(N=131073), dict(B=16384, N=131072), dict(B=2, capacity=1 << 30),
               dict(B=3, capacity=1 << 30)):
        assert f32(_args(**kw), n=1 << 40) == EUNSUPPORTED and need(_args(**kw)) == 0, kw
    size = ctypes.sizeof(type(_args()))
    for wrong in (0, size - 24, size + 8):                  # unsized, short of the mandatory part, longer than known
        a = _args()
        a.struct_bytes = wrong
        assert f32(a) == EINVAL and need(a) == 0, wrong
    a = _args()
    a.struct_bytes = size - 16                              # a caller that knows neither core nor sizes is served
    assert need(a) == need(_args())
    # the workspace: missing, not 256-aligned, short
    good = need(_args())
    assert good % 256 == 0 and good >= 3 * 2 * 1000 * 4
    assert f32(_args(), ws=None) == EINVAL and f32(_args(), ws=WS + 128) == EINVAL and f32(_args(), ws=WS + 16) == EINVAL
    assert f32(_args(), n=good - 1) == EINVAL and f32(_args(), n=0) == EINVAL
    assert lib.vcr_rows_dbscan_workspace_bytes(ctypes.byref(_args()), -1) == 0
    assert need(_args(B=1, N=131072, capacity=1 << 24)) >= 3 * 131072 * 4


def test_the_largest_call_returns_its_argument_errors_without_a_gpu(lib):
    need = lambda a: lib.vcr_cluster_largest_workspace_bytes(ctypes.byref(a), 0)   # noqa: E731
    good = need(_args("largest"))
    f32 = lambda a, ws=WS, n=good: lib.vcr_cluster_largest_f32(ctypes.byref(a), ws, n, None)       # noqa: E731
    assert good > 0 and good % 256 == 0 and lib.vcr_cluster_largest_f32(None, WS, good, None) == EINVAL
    for field in ("xyz", "labels", "sizes", "points", "count"):
        assert f32(_args("largest", **{field: None})) == EINVAL and need(_args("largest", **{field: None})) == 0, field
    assert need(_args("largest", index=None)) == good
    for kw in (dict(B=0), dict(B=-1)):
        assert f32(_args("largest", **kw)) == EINVAL, kw
    for kw in (dict(N=0), dict(N=131073), dict(B=16384, N=131072)):
        assert f32(_args("largest", **kw), n=1 << 40) == EUNSUPPORTED and need(_args("largest", **kw)) == 0, kw
    size = ctypes.sizeof(type(_args("largest")))
    for wrong in (0, size - 16, size + 8):
        a = _args("largest")
        a.struct_bytes = wrong
        assert f32(a) == EINVAL, wrong
    assert f32(_args("largest"), ws=None) == EINVAL and f32(_args("largest"), ws=WS + 64) == EINVAL
    assert f32(_args("largest"), n=good - 1) == EINVAL


def test_the_form_is_host_only_and_follows_the_header(lib):
    """est = capacity / N: the wave form from VCR_DBSCAN_WAVE_HOOK / VCR_DBSCAN_WAVE_LABEL on, per pass; variant forces either;
    the device's size and min_points do not enter."""
    from vcrnet_amd import dbscan
    H, L = dbscan.WAVE_HOOK, dbscan.WAVE_LABEL
    lane, wave = dbscan.FORMS["lane"], dbscan.FORMS["wave"]
    for B, N in ((1, 1), (2, 1000), (16, 16384), (1, 131072)):
        for est in sorted({0, 1, H - 1, H, H + 1, L - 1, L, L + 1, 330, 4096}):
            if B * (N * est + N) >= 1 << 31:
                continue
            for cap in (N * est, N * est + N - 1):
                want = (wave if est >= H else lane, wave if est >= L else lane)
                for kw in (dict(), dict(cu_count=0), dict(cu_count=1), dict(min_points=50)):
                    assert dbscan.form(B, N, cap, **kw)[:2] == want, (B, N, cap, kw)
                assert dbscan.form(B, N, cap, variant=lane)[:2] == (lane, lane)
                assert dbscan.form(B, N, cap, variant=wave)[:2] == (wave, wave)
                assert dbscan.form(B, N, cap)[2] == dbscan.form(B, N, 0)[2] > 0       # the workspace is B's and N's alone
    form = lib.vcr_rows_dbscan_form
    assert form(ctypes.byref(_args()), 256, None, None) == 0
    assert form(None, 256, None, None) == EINVAL and form(ctypes.byref(_args()), -1, None, None) == EINVAL
    for kw in (dict(B=0), dict(capacity=-1), dict(min_points=0), dict(variant=3)):
        assert form(ctypes.byref(_args(**kw)), 256, None, None) == EINVAL, kw
    for kw in (dict(N=0), dict(N=131073), dict(B=16384, N=131072), dict(capacity=1 << 30)):
        assert form(ctypes.byref(_args(**kw)), 256, None, None) == EUNSUPPORTED, kw
    with pytest.raises(Exception):
        dbscan.form(1, 131073, 10)


def test_the_kernels_of_dbscan_hip_use_no_scratch_and_keep_eight_waves():
    """hipcc's remarks for dbscan.hip: its kernel set is the thirteen below (the three row passes in two forms each), none with
    scratch or a spill, none with AGPRs; the tail vcr_cluster_largest_f32 launches stays outlier.hip's.  As recorded from the
    build (waves a SIMD, VGPRs, static LDS bytes a workgroup; none takes dynamic LDS):
      dbscan_check_kernel      8 waves,  8 VGPRs, 256 B   (the workgroup's "or")
      dbscan_served_kernel     8 waves, 14 VGPRs, 256 B   (likewise)
      dbscan_core_kernel<1>    8 waves, 20 VGPRs,   0 B
      dbscan_core_kernel<2>    8 waves, 23 VGPRs,   0 B
      dbscan_hook_kernel<1>    8 waves, 28 VGPRs,   0 B   (four entries and their nodes in flight)
      dbscan_hook_kernel<2>    8 waves, 36 VGPRs,   0 B
      dbscan_flatten_kernel    8 waves, 14 VGPRs,  16 B   (the four waves' root counts)
      dbscan_offsets_kernel    8 waves, 24 VGPRs,  16 B
      dbscan_rank_kernel       8 waves, 13 VGPRs,  16 B
      dbscan_label_kernel<1>   8 waves, 20 VGPRs,   0 B
      dbscan_label_kernel<2>   8 waves, 22 VGPRs,   0 B
      largest_pick_kernel      8 waves,  8 VGPRs,  32 B
      largest_member_kernel    8 waves, 13 VGPRs,   0 B"""
    import vcrnet_amd  # noqa: F401
    from vcrnet_amd import build
    build.build()
    res = build.kernel_resources()
    names = list(res)
    dem = subprocess.run(["c++filt"], input="\n".join(names), capture_output=True, text=True, check=True).stdout.splitlines()
    by_name = {d.replace("(anonymous namespace)::", "").replace("void ", "").split("(")[0]: res[n] for n, d in zip(names, dem)}
    mine = {d: v for d, v in by_name.items() if v["file"] == "dbscan.hip"}
    assert set(mine) == KERNELS
    for d, v in mine.items():
        print(d, v)
        assert v.get("scratch", 0) == 0 and v.get("vgpr_spill", 0) == 0 and v.get("sgpr_spill", 0) == 0 and v["agprs"] == 0, (d, v)
        assert v["occupancy"] == 8 and v["vgprs"] <= 40, (d, v)
    assert {d: v["lds"] for d, v in mine.items() if v["lds"]} == {
        "dbscan_check_kernel": 256, "dbscan_served_kernel": 256, "dbscan_flatten_kernel": 16, "dbscan_offsets_kernel": 16, "dbscan_rank_kernel": 16,
        "largest_pick_kernel": 32}
    for k in ("outlier_mark_kernel", "outlier_offsets_kernel", "outlier_write_kernel"):
        assert by_name[k]["file"] == "outlier.hip", k


# ------------------------------------------------------------------------------------------------------------ the Python layer

def test_python_entry_points_refuse_what_they_cannot_run():
    import vcrnet_amd
    from vcrnet_amd import dbscan, native
    assert vcrnet_amd.cluster_dbscan is dbscan.cluster_dbscan and vcrnet_amd.largest_cluster is dbscan.largest_cluster
    assert {"cluster_dbscan", "largest_cluster"} <= set(vcrnet_amd.__all__) and "dbscan" not in vcrnet_amd.__all__
    E = native.VcrHipError
    x = torch.zeros(2, 3, 50)
    for bad in (x.transpose(1, 2), torch.zeros(3, 50), None, "xyz"):
        with pytest.raises(E, match=r"xyz must be a \[B, 3, N\]"):
            vcrnet_amd.cluster_dbscan(bad, 0.5, 4)
    with pytest.raises(E, match="cluster_dbscan: a cloud must have 1 ... 131072 points"):
        vcrnet_amd.cluster_dbscan(torch.zeros(1, 3, 131073), 0.5, 4)
    for bad in (0.0, -1.0, float("nan"), float("inf"), 1.9e19, "r", None):
        with pytest.raises(E, match="cluster_dbscan: radius must be finite and > 0 with a finite square"):
            vcrnet_amd.cluster_dbscan(x, bad, 4)
    for bad in (0, -1, 2.0, "3", True, None):
        with pytest.raises(E, match="cluster_dbscan: min_points must be an integer >= 1"):
            vcrnet_amd.cluster_dbscan(x, 0.5, bad)
    for bad in (-1, 2.5, "7", True):
        with pytest.raises(E, match="cluster_dbscan: capacity must be None or an integer >= 0"):
            vcrnet_amd.cluster_dbscan(x, 0.5, 4, capacity=bad)
    with pytest.raises(E, match="beyond 2\\^31"):
        vcrnet_amd.cluster_dbscan(x, 0.5, 4, capacity=1 << 30)
    for bad in (0.0, -1.0, float("nan"), float("inf")):
        with pytest.raises(E, match="cluster_dbscan: cell must be None"):
            vcrnet_amd.cluster_dbscan(x, 0.5, 4, cell=bad)
    for kw in (dict(), dict(capacity=400), dict(cell=0.25, want_core=True, want_sizes=True), dict(capacity=0)):
        with pytest.raises(E, match="no CPU fallback"):      # (the last refusal: everything else was in order)
            vcrnet_amd.cluster_dbscan(x, 0.5, 1, **kw)
    # the raw call: shapes and types first, then the device
    idx, rs, tot = torch.zeros(2, 100, dtype=torch.int32), torch.zeros(2, 51, dtype=torch.int64), torch.zeros(2, dtype=torch.int64)
    with pytest.raises(E, match=r"idx must be int32 \[B, capacity\]"):
        dbscan.cluster_rows(idx.long(), rs, tot, 50, 4)
    with pytest.raises(E, match=r"row_start must be int64 \[B, N \+ 1\]"):
        dbscan.cluster_rows(idx, rs, tot, 49, 4)
    with pytest.raises(E, match=r"total must be int64 \[B\]"):
        dbscan.cluster_rows(idx, rs, tot.int(), 50, 4)
    with pytest.raises(E, match=r"xyz must be None or float32 \[B, 3, N\]"):
        dbscan.cluster_rows(idx, rs, tot, 50, 4, xyz=torch.zeros(2, 3, 49))
    for bad in (0, 131073, 50.0, True):
        with pytest.raises(E, match=r"N must be an integer in \[1, 131072\]"):
            dbscan.cluster_rows(idx, rs, tot, bad, 4)
    with pytest.raises(E, match="min_points must be an integer >= 1"):
        dbscan.cluster_rows(idx, rs, tot, 50, 0)
    with pytest.raises(E, match="variant must be 0"):
        dbscan.cluster_rows(idx, rs, tot, 50, 4, variant="block")
    with pytest.raises(E, match="below 2\\^31"):
        dbscan.cluster_rows(torch.zeros(1 << 20, 0, dtype=torch.int32), rs, tot, 4096, 4)
    for call in (lambda: dbscan.cluster_rows(idx, rs, tot, 50, 4), lambda: dbscan.cluster_rows(idx, rs, tot, 50, 1, xyz=x, variant="wave"),
                 lambda: dbscan.cluster_rows(idx, rs, tot, 50, 4, want_core=True, want_sizes=True, variant="lane")):
        with pytest.raises(E, match="no CPU fallback"):
            call()
    lab = torch.zeros(2, 50, dtype=torch.int32)
    with pytest.raises(E, match=r"xyz must be a \[B, 3, N\]"):
        vcrnet_amd.largest_cluster(lab, lab, lab)
    with pytest.raises(E, match=r"labels must be int32 \[B, N\]"):
        vcrnet_amd.largest_cluster(x, lab.long(), lab)
    with pytest.raises(E, match=r"sizes must be int32 \[B, N\]"):
        vcrnet_amd.largest_cluster(x, lab, lab[:, :49])
    with pytest.raises(E, match="no CPU fallback"):
        vcrnet_amd.largest_cluster(x, lab, lab)
