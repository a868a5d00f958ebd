"""Normals and FPFH over ragged rows without a GPU: the numpy restatement (tests/rows_restated.py) against plane_restated and
fpfh_restated on the same lists, the recipe of the GPU test (the row lengths it must hit, no pair on an atan2 bin edge), the
boundary of include/ext/vcr_hip_rows.h (prototypes against vcrnet_amd.rows.SIGNATURES, the structs against gcc's layout), every
argument error of the calls and of the Python functions, the host-only form query, and the resource remarks of rows.hip."""
import ctypes
import os
import subprocess

import numpy as np
import pytest
import torch

import boundary
import fpfh_restated as fr
import grid_restated as gr
import outlier_restated as orr
import plane_restated as pr
import radius_restated as rr
import rows_restated as wr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INCLUDE = os.path.join(ROOT, "include")
HEADER = os.path.join(INCLUDE, "ext", "vcr_hip_rows.h")
EINVAL, EUNSUPPORTED = -1, -3
ENTRY_POINTS = {"vcr_rows_normals_f32", "vcr_rows_spfh_f32", "vcr_rows_fpfh_f32", "vcr_rows_form"}
KERNELS = {"rows_normals_kernel", "rows_spfh_lane_kernel", "rows_spfh_wave_kernel", "rows_fpfh_lane_kernel", "rows_fpfh_wave_kernel",
           "rows_void_kernel"}
MAX_NN = (0, 1, 2, 5)


@pytest.fixture(scope="module")
def lib():
    import vcrnet_amd  # noqa: F401
    from vcrnet_amd import build, rows
    build.build()
    return rows.lib()


# ------------------------------------------------------------------------------------------------------------- the restatement

def _against_the_fixed_width_restatements(x, idx, row_start, nrm):
    """For max_nn = 0, 1, 2, 5: the restated rows' C, normals (by eigh) and both FPFH passes against plane_restated /
    fpfh_restated run on each row alone."""
    N = x.shape[1]
    for m in MAX_NN:
        j, used, L = wr.padded(idx, row_start, m)
        assert (L == (np.minimum(np.diff(row_start), m) if m else np.diff(row_start))).all() and (used.sum(1) == L).all()
        n, cv, C, _ = wr.normals(x, idx, row_start, m, solve=pr.normal)
        p = wr.pairs(x, nrm, idx, row_start, m)
        sp = wr.pack(p)
        for i in range(N):
            row = np.asarray(idx)[row_start[i]:row_start[i] + L[i]]
            if L[i] >= 2:
                Ci = pr.covariance(x, i, row)
                assert np.array_equal(C[i], Ci, equal_nan=True), (m, i)
                want = pr.normal(Ci, x[:, i])
                assert np.array_equal(n[:, i], want[0]) and np.array_equal(cv[i], want[2], equal_nan=True), (m, i)
            else:
                assert n[:, i].tolist() == [0, 0, 1] and cv[i] == 0, (m, i)
            # the first pass: the row alone as a fixed-width list of point i (the other points' rows: their own index)
            one = np.broadcast_to(np.arange(N)[:, None], (N, max(int(L[i]), 1))).copy()
            one[i, :L[i]] = row
            q = fr.pairs(x, nrm, one)
            cnt = q["counted"][i, :L[i]]
            assert np.array_equal(p["counted"][i, :L[i]], cnt) and not p["counted"][i, L[i]:].any(), (m, i)
            assert np.array_equal(p["bins"][i, :L[i]][cnt], q["bins"][i, :L[i]][cnt]), (m, i)
            assert sp[i, 0, 11] == sp[i, 1, 11] == sp[i, 2, 11] == cnt.sum() and (sp[i, :, :11].sum(1) == cnt.sum()).all()
        assert sp.min() >= 0
        yield m, L, sp


def test_the_definitions_on_a_cloud_worked_by_hand():
    """Five points on the x axis and one off it; rows built by hand: an empty row, a row of one, rows holding a copy of the
    query (d2 = 0), -1 and an index past N (both read as the query: counted at distance 0), and unused slots behind a cut."""
    x = np.asarray([[0, 1, 1, 2, 4, 1], [0, 0, 0, 0, 0, 1], [0, 0, 0, 0, 0, 0.5]], np.float32)     # 1 and 2 are copies
    nrm = np.tile(np.asarray([[0], [0], [1]], np.float32), (1, 6))
    rows = [[1, 2, 5, 3], [2, 0, 5], [], [1], [-1, 3, 99, 0], [0, 1, 2, 3, 4, 5]]
    idx = np.asarray([e for r in rows for e in r] + [7, 7], np.int32)              # (two slots behind total: never read)
    row_start = np.cumsum([0] + [len(r) for r in rows]).astype(np.int64)
    seen = {m: (L, sp) for m, L, sp in _against_the_fixed_width_restatements(x, idx, row_start, nrm)}
    assert seen[0][0].tolist() == [4, 3, 0, 1, 4, 6] and seen[2][0].tolist() == [2, 2, 0, 1, 2, 2]
    sp = seen[0][1]
    # every normal is (0,0,1).  Row 4 is [-1, 3, 99, 0]: two entries read as 4 itself (distance 0: bins 5, 5, 5) and two lie on
    # the axis (f = (0, 0, 0) as well); row 1 is [2, 0, 5]: a copy, a point on the axis, and point 5 with f2 = 0.5 / sqrt(1.25)
    assert sp[2].sum() == 0 and sp[4, :, 5].tolist() == [4, 4, 4] and sp[4, :, 11].tolist() == [4, 4, 4]
    assert sp[1, 2, 5] == 2 and sp[1, 2, 7] == 1 and sp[1, :, 11].tolist() == [3, 3, 3]
    # padding with -1 instead of masking WOULD count: the restatement must not do it
    bad = fr.pairs(x, nrm, np.asarray([r[:1] + [-1] * 5 for r in [[1], [2], [0], [1], [3], [0]]]))
    assert bad["counted"].all()
    f = wr.fpfh(x, idx, row_start, sp)
    assert f.shape == (33, 6) and np.isfinite(f).all()
    assert np.array_equal(f[:, 2], np.zeros(33, np.float32))                       # an empty row with no pairs of its own
    for g in range(3):                                                             # neighbours with pairs: each group sums to 200
        assert abs(float(f[11 * g:11 * g + 11, 0].sum()) - 200.0) < 1e-3


@pytest.mark.parametrize("name", ["random", "copies", "nonfinite", "flat", "lattice"])
def test_the_restatement_on_radius_rows_of_the_small_recipes(name):
    N = 60
    x = gr.RECIPES[name](N, seed=N)
    got = rr.radius_rows(x, 1.5 if name == "lattice" else orr.radius_for(N, 12))      # (the lattice's spacing is 1)
    rs = np.random.RandomState(3)
    nrm = rs.normal(size=(3, N)).astype(np.float32)
    nrm /= np.linalg.norm(nrm, axis=0)
    lens = set()
    for m, L, sp in _against_the_fixed_width_restatements(x, got["idx"], got["row_start"], nrm):
        lens |= set(L.tolist())
        f = wr.fpfh(x, got["idx"], got["row_start"], sp, m)
        assert f.shape == (33, N)
    print(name, "row lengths", sorted(lens))
    assert max(lens) >= 5, lens                              # (max_nn = 5 cuts something)


@pytest.mark.parametrize("B,N,k", [(1, 5, 4), (2, 64, 20), (1, 300, 62)])
def test_a_fixed_width_list_written_as_rows_gives_the_fixed_width_values(B, N, k):
    """fpfh_restated.spfh / fpfh bit for bit (the counts widened), plane_restated's C bit for bit, and the Jacobi restated from
    the device's code against numpy's eigh: the same eigenvalue ratio to 1e-9 and the same axis where the two smallest
    eigenvalues are apart (2^-10 lambda2, the normals tests' own rule)."""
    x = fr.cloud(B, N)
    for b in range(B):
        idx = fr.neighbours(x[b], k)
        flat, row_start = wr.dense_csr(idx)
        nrm = fr.normals(x[b], idx)
        sp = fr.spfh(x[b], nrm, idx)
        assert np.array_equal(wr.spfh(x[b], nrm, flat, row_start), wr.widen(sp))
        assert np.array_equal(wr.fpfh(x[b], flat, row_start, wr.widen(sp)), fr.fpfh(x[b], idx, sp))
        n, cv, C, L = wr.normals(x[b], flat, row_start)
        assert (L == k).all() and np.array_equal(C, pr.covariances(x[b], idx))
        lam = np.linalg.eigvalsh(C)
        apart = lam[:, 1] - lam[:, 0] >= 2.0 ** -10 * lam[:, 2]
        assert apart.mean() >= 0.95
        dots = np.abs((n * nrm).sum(0))
        assert (dots[apart] >= 1 - 1e-6).all(), float(dots[apart].min())
        want_cv = np.asarray([pr.normal(c)[2] for c in C])
        assert np.allclose(cv, want_cv, rtol=1e-5, atol=1e-9)
        big = np.abs(n).argmax(0)
        assert (n[big, np.arange(N)] > 0).all()              # the sign rule without a viewpoint
        # cutting a fixed-width list: max_nn = 5 is the list's first five columns
        if k > 5:
            assert np.array_equal(wr.normals(x[b], flat, row_start, 5)[2], pr.covariances(x[b], idx[:, :5]))
            sp5 = fr.spfh(x[b], nrm, idx[:, :5])
            assert np.array_equal(wr.spfh(x[b], nrm, flat, row_start, 5), wr.widen(sp5))
            assert np.array_equal(wr.fpfh(x[b], flat, row_start, wr.widen(sp5), 5), fr.fpfh(x[b], idx[:, :5], sp5))


def test_the_ragged_recipe_has_the_rows_the_gpu_test_needs_and_no_pair_on_a_bin_edge():
    """tests/test_hip_rows.py compares the device with the restatement on fpfh_restated.cloud(2, 300) at rows_restated's radii:
    rows of 0, 1, 2, 63, 64, 65 and 129 entries and of more than 255 occur, the last radius puts the whole cloud into every
    row, and no counted pair lies within 2^-30 of an atan2 bin edge (the cap on excluded pairs is 0)."""
    B, N = wr.RAGGED
    x = fr.cloud(B, N)
    lens, excluded = set(), 0
    for b in range(B):
        d2 = rr.d2_all(x[b])
        for radius in wr.RAGGED_RADII:
            got = rr.radius_rows(x[b], radius, d2=d2)
            lens |= set(got["count"].tolist())
            if radius == wr.RAGGED_RADII[-1]:
                assert (got["count"] == N - 1).all()
            nrm = wr.normals(x[b], got["idx"], got["row_start"])[0]
            p = wr.pairs(x[b], nrm, got["idx"], got["row_start"])
            excluded += int(fr.excluded(p).sum())
    assert set(wr.WANTED_LENGTHS) <= lens and max(lens - {N - 1}) > 255, sorted(lens)
    assert excluded == 0
    e = wr.exact_cloud()
    assert e.shape == (2, 3, 300) and (np.abs(e) < 4).all() and np.array_equal(e * 64, np.round(e * 64))


# ---------------------------------------------------------------------------------------------------------------- the boundary

def test_signatures_match_the_header_and_the_library_exports_them(lib):
    from vcrnet_amd import rows
    boundary.check_signatures(HEADER, rows, lib, ENTRY_POINTS)


def test_args_match_the_c_layout(tmp_path):
    import vcrnet_amd  # noqa: F401
    from vcrnet_amd import rows
    assert set(rows.STRUCTS) == {"vcr_rows_normals_args", "vcr_rows_spfh_args", "vcr_rows_fpfh_args"}
    boundary.check_layout(HEADER, rows, tmp_path)
    assert rows.RowsNormalsArgs.curvature.offset == rows.RowsNormalsArgs.normals.offset + 8   # the mandatory part ends behind normals


def test_the_header_lives_beside_the_others_and_enters_the_digests(lib, monkeypatch):
    """include/*.h is what it was (new public headers go to include/ext/), none of those fourteen mentions the new calls, ABI 27
    and the same 51 prototypes; the header enters the digests through a list of its own; its numbers are the module's."""
    from vcrnet_amd import build, fpfh, native, plane, radius, rows
    others = sorted(f for f in os.listdir(INCLUDE) if f.endswith(".h"))
    assert len(others) == 14 and os.listdir(os.path.join(INCLUDE, "ext")) == ["vcr_hip_rows.h"]
    for h in others:
        text = open(os.path.join(INCLUDE, h)).read()
        assert "vcr_rows_" not in text and "VCR_ROWS" not in text, h             # (vcr_hip.h has vcr_rows4_f32, the layout call)
    assert '#include "../vcr_hip_plane.h"' in open(HEADER).read()
    assert len(native.PUBLIC) == 51 and lib.vcr_abi_version() == native.ABI_VERSION == 27
    for other in (native, plane, fpfh, radius):
        assert not set(rows.SIGNATURES) & set(other.SIGNATURES) and not set(rows.STRUCTS) & set(other.STRUCTS)
    assert build.ROWS_HEADERS == [HEADER]
    assert HEADER not in (build.PUBLIC_HEADERS + build.LATER_HEADERS + build.OUTLIER_HEADERS + build.GICP_HEADERS
                          + build.FPFH_HEADERS + build.MATCH_HEADERS + build.FGR_HEADERS + build.GRID_HEADERS
                          + build.GRIDNN_HEADERS + build.VOXEL_SORT_HEADERS + build.RADIUS_HEADERS)
    full = build.sources_sha16()
    monkeypatch.setattr(build, "ROWS_HEADERS", [])
    assert build.sources_sha16() != full
    monkeypatch.undo()
    text = open(HEADER).read()
    for name, value in (("VCR_ROWS_MAX_N", rows.MAX_N), ("VCR_ROWS_SPFH_WORDS", rows.SPFH_WORDS), ("VCR_ROWS_LANE", rows.FORMS["lane"]),
                        ("VCR_ROWS_WAVE", rows.FORMS["wave"]), ("VCR_ROWS_WAVE_SPFH", rows.WAVE_SPFH),
                        ("VCR_ROWS_WAVE_FPFH", rows.WAVE_FPFH)):
        assert "#define %s %d" % (name, value) in text, name


def _args(kind, **kw):
    from vcrnet_amd import rows
    a = {"normals": rows.RowsNormalsArgs, "spfh": rows.RowsSpfhArgs, "fpfh": rows.RowsFpfhArgs}[kind]()
    for k, f in enumerate(n for n, t in a._fields_ if t is ctypes.c_void_p):       # (never dereferenced)
        setattr(a, f, 0x1000 * (k + 1))
    v = dict(B=2, N=1000, capacity=20000, max_nn=0)
    v.update(kw)
    for k, x in v.items():
        setattr(a, k, x)
    return a


@pytest.mark.parametrize("kind", ["normals", "spfh", "fpfh"])
def test_the_calls_return_their_argument_errors_without_a_gpu(lib, kind):
    f32 = lambda a: getattr(lib, "vcr_rows_%s_f32" % kind)(ctypes.byref(a), None)  # noqa: E731
    assert getattr(lib, "vcr_rows_%s_f32" % kind)(None, None) == EINVAL
    optional = {"viewpoint", "curvature"}
    pointers = [n for n, t in _args(kind)._fields_ if t is ctypes.c_void_p and n not in optional]
    for field in pointers:
        assert f32(_args(kind, **{field: None})) == EINVAL, field
    aligned = {"normals": ("xyz4",), "spfh": ("xyz4", "spfh"), "fpfh": ("xyz4", "spfh")}[kind]
    for field in aligned:
        assert f32(_args(kind, **{field: 0x1008})) == EINVAL, field
    bad = [dict(B=0), dict(B=-1), dict(capacity=-1), dict(max_nn=-1), dict(idx=None, capacity=1)]
    if kind != "normals":
        bad += [dict(variant=3), dict(variant=-1), dict(variant=0x10)]
    for kw in bad:
        assert f32(_args(kind, **kw)) == EINVAL, kw
    for kw in (dict(N=0), dict(N=-5), dict(N=131073), dict(B=16384, N=131072), dict(B=2, capacity=1 << 30), dict(B=3, capacity=1 << 30)):
        assert f32(_args(kind, **kw)) == EUNSUPPORTED, kw
    size = ctypes.sizeof(type(_args(kind)))
    for wrong in (0, size - 16, size + 8):                  # unsized, short of the mandatory part, longer than known
        a = _args(kind)
        a.struct_bytes = wrong
        assert f32(a) == EINVAL, wrong
    assert _args(kind).struct_bytes == size


def test_the_form_is_host_only_and_follows_the_header(lib):
    """est = capacity / N, cut at max_nn: the wave form from VCR_ROWS_WAVE_SPFH / VCR_ROWS_WAVE_FPFH on, per pass; variant
    forces either; the device's size does not enter."""
    from vcrnet_amd import rows
    S, F = rows.WAVE_SPFH, rows.WAVE_FPFH
    lane, wave = rows.FORMS["lane"], rows.FORMS["wave"]
    for B, N in ((1, 1), (2, 1000), (16, 16384), (1, 131072)):
        for est in (0, 1, S - 1, S, S + 1, 330, 4096, F - 1, F, F + 7):       # (capacity / N may exceed N: slots are the caller's)
            if B * (N * est + N) >= 1 << 31:
                continue
            for cap in (N * est, N * est + N - 1):
                want = (wave if est >= S else lane, wave if est >= F else lane)
                assert rows.form(B, N, cap) == want == rows.form(B, N, cap, cu_count=0) == rows.form(B, N, cap, cu_count=1), (B, N, cap)
                assert rows.form(B, N, cap, max_nn=est + 5) == want
                for m in (1, S - 1, S, F):
                    e = min(est, m)
                    assert rows.form(B, N, cap, max_nn=m) == (wave if e >= S else lane, wave if e >= F else lane), (B, N, cap, m)
                assert rows.form(B, N, cap, variant=lane) == (lane, lane) and rows.form(B, N, cap, variant=wave) == (wave, wave)
    assert rows.form(1, 1000, 0) == (lane, lane)
    form = lib.vcr_rows_form
    assert form(2, 1000, 20000, 0, 256, 0, None, None) == 0
    for a in ((0, 1000, 0, 0, 256, 0), (2, 1000, -1, 0, 256, 0), (2, 1000, 0, -1, 256, 0), (2, 1000, 0, 0, -1, 0), (2, 1000, 0, 0, 256, 3)):
        assert form(*a, None, None) == EINVAL, a
    for a in ((2, 0, 0, 0, 256, 0), (2, 131073, 0, 0, 256, 0), (16384, 131072, 0, 0, 256, 0), (2, 1000, 1 << 30, 0, 256, 0)):
        assert form(*a, None, None) == EUNSUPPORTED, a
    with pytest.raises(Exception):
        rows.form(1, 131073, 10)


def test_the_kernels_of_rows_hip_use_no_scratch_and_keep_their_occupancy():
    """hipcc's remarks for rows.hip: its kernel set is the six rows_* kernels, none with scratch or a spill.  As recorded from the
    build (waves a SIMD, static LDS bytes a workgroup; none takes dynamic LDS):
      rows_normals_kernel     8 waves,      0 B   (64 VGPRs: normals_kernel's 61 and the row's bounds)
      rows_spfh_lane_kernel   4 waves, 33 792 B   (110 VGPRs; 33 counters a lane in LDS: four workgroups fill 135 of a CU's 160 KB)
      rows_spfh_wave_kernel   4 waves,    576 B   (116 VGPRs; four waves' 33 counters and c_i)
      rows_fpfh_lane_kernel   5 waves,      0 B   (92 VGPRs: eleven fp64 sums and two 48-byte groups)
      rows_fpfh_wave_kernel   6 waves,      0 B   (76 VGPRs)
      rows_void_kernel        8 waves,    256 B   (the workgroup's "or")
    normals.hip and fpfh.hip keep their kernels: what rows.hip shares with normals.hip is a header, compiled into both."""
    import vcrnet_amd  # noqa: F401
    from vcrnet_amd import build
    build.build()
    res = build.kernel_resources()
    names = list(res)
    dem = subprocess.run(["c++filt"], input="\n".join(names), capture_output=True, text=True, check=True).stdout.splitlines()
    by_name = {d.replace("(anonymous namespace)::", "").replace("void ", "").split("(")[0]: res[n] for n, d in zip(names, dem)}
    mine = {d: v for d, v in by_name.items() if v["file"] == "rows.hip"}
    assert set(mine) == KERNELS
    for d, v in mine.items():
        print(d, v)
        assert v.get("scratch", 0) == 0 and v.get("vgpr_spill", 0) == 0 and v.get("sgpr_spill", 0) == 0 and v["agprs"] == 0, (d, v)
    assert {d: v["occupancy"] for d, v in mine.items()} == {
        "rows_normals_kernel": 8, "rows_spfh_lane_kernel": 4, "rows_spfh_wave_kernel": 4, "rows_fpfh_lane_kernel": 5,
        "rows_fpfh_wave_kernel": 6, "rows_void_kernel": 8}
    assert {d: v["lds"] for d, v in mine.items()} == {
        "rows_normals_kernel": 0, "rows_spfh_lane_kernel": 33 * 256 * 4, "rows_spfh_wave_kernel": 4 * 36 * 4, "rows_fpfh_lane_kernel": 0,
        "rows_fpfh_wave_kernel": 0, "rows_void_kernel": 256}
    assert by_name["normals_kernel"]["file"] == "normals.hip"
    assert by_name["spfh_kernel"]["file"] == by_name["fpfh_kernel"]["file"] == "fpfh.hip"
    assert by_name["normals_kernel"]["vgprs"] <= 64 and by_name["normals_kernel"]["occupancy"] == 8
    assert {d for d, v in by_name.items() if v["file"] == "normals.hip"} == {"normals_kernel"}
    assert {d for d, v in by_name.items() if v["file"] == "fpfh.hip"} == {"spfh_kernel", "fpfh_kernel"}


# ------------------------------------------------------------------------------------------------------------ the Python layer

def test_python_entry_points_refuse_what_they_cannot_run():
    import vcrnet_amd
    from vcrnet_amd import grid, native, rows
    assert vcrnet_amd.rows is rows and "rows" not in vcrnet_amd.__all__ and grid.SEARCHES == ("knn", "grid")
    with pytest.raises(native.VcrHipError, match='search must be "knn" or "grid"'):
        grid.check_search("x", "radius")                    # (the callers handle "radius" before they ask)
    E = native.VcrHipError
    x, y = torch.zeros(2, 3, 50), torch.zeros(2, 3, 60)
    calls = ((lambda **kw: vcrnet_amd.estimate_normals(x, **kw)), (lambda **kw: vcrnet_amd.compute_fpfh_feature(x, **kw)),
             (lambda **kw: vcrnet_amd.register_features(x, y, 0.1, **kw)))
    for call in calls:
        with pytest.raises(E, match='search="radius" needs a radius'):
            call(search="radius")
        for search in ("knn", "grid"):
            for kw in (dict(max_nn=30), dict(capacity=100), dict(max_nn=30, capacity=100)):
                with pytest.raises(E, match='max_nn and capacity belong to search="radius"'):
                    call(search=search, **kw)
        for bad in (0, -1, 2.0, "3", True):
            with pytest.raises(E, match="max_nn must be None or an integer >= 1"):
                call(search="radius", radius=0.5, max_nn=bad)
        for kw in (dict(), dict(max_nn=1), dict(max_nn=100), dict(max_nn=1000, capacity=500), dict(capacity=0)):
            with pytest.raises(E, match="no CPU fallback"):  # (the last refusal: everything else was in order)
                call(search="radius", radius=0.5, **kw)
        for bad in ("Radius", "", None, 1):
            with pytest.raises(E, match='search must be "knn" or "grid"'):
                call(search=bad)
    with pytest.raises(E, match='radius belongs to search="radius"'):
        vcrnet_amd.estimate_normals(x, radius=0.5)
    for kw in (dict(), dict(search="grid"), dict(k=30, radius=0.5, search="grid")):       # the defaults are where they were
        with pytest.raises(E, match="no CPU fallback"):
            vcrnet_amd.compute_fpfh_feature(x, **kw)
    with pytest.raises(E, match="no CPU fallback"):
        vcrnet_amd.estimate_normals(x)
    # the raw wrappers: shapes and types first, then the device
    x4 = torch.zeros(2, 50, 4)
    idx, rs, tot = torch.zeros(2, 100, dtype=torch.int32), torch.zeros(2, 51, dtype=torch.int64), torch.zeros(2, dtype=torch.int64)
    nrm, sp = torch.zeros(2, 3, 50), torch.zeros(2, 50, 3, 12, dtype=torch.int32)
    with pytest.raises(E, match=r"idx must be int32 \[B, capacity\]"):
        rows.normals(x4, idx.long(), rs, tot)
    with pytest.raises(E, match=r"row_start must be int64 \[B, N \+ 1\]"):
        rows.normals(x4, idx, rs[:, :50], tot)
    with pytest.raises(E, match=r"total must be int64 \[B\]"):
        rows.spfh(x4, nrm, idx, rs, tot.int())
    with pytest.raises(E, match=r"spfh must be int32 \[B, N, 3, 12\]"):
        rows.fpfh(x4, idx, rs, tot, sp.view(2, 50, 36))
    with pytest.raises(E, match="max_nn must be None or an integer >= 1"):
        rows.normals(x4, idx, rs, tot, max_nn=0)
    with pytest.raises(E, match="variant must be 0"):
        rows.spfh(x4, nrm, idx, rs, tot, variant="block")
    for call in (lambda: rows.normals(x4, idx, rs, tot), lambda: rows.spfh(x4, nrm, idx, rs, tot, variant="wave"),
                 lambda: rows.fpfh(x4, idx, rs, tot, sp, max_nn=7, variant="lane")):
        with pytest.raises(E, match="no CPU fallback"):
            call()
