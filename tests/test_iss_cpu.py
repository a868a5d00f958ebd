"""ISS keypoints without a GPU (include/keypoint/vcr_hip_iss.h): the restatement (tests/iss_restated.py)
against a cloud worked by hand, its 64-chain sums against a plain loop, the definition against Open3D's float64 arithmetic, the
prefix rule against a second search, the header against the ctypes binding and the library's exports, the argument errors of the
C entry points and of the Python layer, and the resource remarks of iss.hip."""
import ctypes
import os
import subprocess

import numpy as np
import pytest
import torch

import boundary
import iss_restated as ir
import radius_restated as rr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INCLUDE = os.path.join(ROOT, "include")
HEADER = os.path.join(INCLUDE, "keypoint", "vcr_hip_iss.h")
ENTRY_POINTS = ("vcr_rows_iss_saliency_f32", "vcr_rows_iss_nms_f32", "vcr_rows_iss_form", "vcr_iss_select_workspace_bytes",
                "vcr_iss_select_f32")
KERNELS = {"iss_saliency_kernel", "iss_nms_lane_kernel", "iss_nms_wave_kernel", "iss_void_kernel"}
EINVAL, EUNSUPPORTED = -1, -3
F32 = np.float32


@pytest.fixture(scope="module")
def lib():
    import vcrnet_amd  # noqa: F401
    from vcrnet_amd import iss
    return iss.lib()


# --------------------------------------------------------------------------------------------------------------- the definition

def test_the_cloud_worked_by_hand():
    """Two stars (iss_restated.hand_cloud): the centres' eigenvalues are 2/7 (0.5/7), 8/7, 32/7 with nothing to rotate; the arms
    have m = 2.  Over the whole non-max rows the sharper star's centre beats the other; with the prefix cut below d2 = 100 the
    centres do not see each other and both stay."""
    x, rows, nms_rows, d2 = ir.hand_cloud()
    sal, eig = ir.saliency(x, *rows)
    assert sal[0] == 2.0 / 7.0 and sal[7] == 0.5 / 7.0 and not sal[1:7].any() and not sal[8:].any()
    assert eig[0].tolist() == [2.0 / 7.0, 8.0 / 7.0, 32.0 / 7.0] and eig[7].tolist() == [0.5 / 7.0, 8.0 / 7.0, 32.0 / 7.0]
    assert not eig[1:7].any() and not eig[8:].any()         # m = 2 < min_neighbors
    whole = ir.definition(x, rows, nms_rows=nms_rows)
    assert whole["keypoint"].tolist() == [1] + [0] * 13 and whole["count"] == 1 and whole["index"][:2].tolist() == [0, -1]
    assert whole["points"][:, 0].tolist() == [0, 0, 0] and np.isnan(whole["points"][:, 1:]).all()
    cut = ir.definition(x, rows, nms_rows=nms_rows, d2=d2, r2_nm=99.0)
    assert cut["keypoint"].tolist() == [1] + [0] * 6 + [1] + [0] * 6 and cut["index"][:3].tolist() == [0, 7, -1]
    assert ir.used_lengths(nms_rows[1], d2, 99.0).tolist() == [6] + [1] * 6 + [6] + [1] * 6
    assert ir.used_lengths(nms_rows[1], d2, 0.25)[7] == 2 and ir.used_lengths(nms_rows[1], d2, 0.2)[7] == 0
    # seven used entries and the point: min_neighbors = 8 keeps, 9 drops; the saliency asks it of m = 7
    assert ir.nms(sal, *nms_rows, min_neighbors=8)[0] == 1 and ir.nms(sal, *nms_rows, min_neighbors=9)[0] == 0
    assert ir.saliency(x, *rows, min_neighbors=7)[0][0] == 2.0 / 7.0 and ir.saliency(x, *rows, min_neighbors=8)[0][0] == 0.0
    # min_neighbors = 2: an arm's C is diag(4, 0, 0) (or its like): l0 = l1 = 0, the ratio l0 / l1 is NaN and fails
    sal2, eig2 = ir.saliency(x, *rows, min_neighbors=2)
    assert eig2[1].tolist() == [0.0, 0.0, 4.0] and sal2[1] == 0.0 and eig2[5].tolist() == [0.0, 0.0, 0.25]
    # the ratio tests: 0.25 and 0.25 at the first centre
    assert ir.saliency(x, *rows, gamma_21=0.25)[0][0] == 0.0 and ir.saliency(x, *rows, gamma_32=0.25)[0][0] == 0.0
    assert ir.saliency(x, *rows, gamma_21=0.26, gamma_32=0.26)[0][0] == 2.0 / 7.0


@pytest.mark.parametrize("L", ir.LENGTHS)
def test_the_sixty_four_chains_against_a_plain_loop(L):
    """Values whose sum depends on the order (nine magnitudes apart), at every row length around the chain count."""
    rs = np.random.RandomState(L)
    vals = rs.normal(size=L) * 10.0 ** rs.randint(-4, 5, L)
    terms = np.zeros((2, max(L, 1) + 3, 1))
    terms[0, :L, 0] = vals
    terms[1, :, 0] = 7.0                                    # (a second row, all of it unused)
    used = np.zeros(terms.shape[:2], bool)
    used[0, :L] = True
    got = ir.chain_sums(terms, used)
    want = ir.chain_loop(vals)
    assert got[0, 0].view(np.uint64) == np.float64(want).view(np.uint64) and got[1, 0] == 0.0 and not np.signbit(got[1, 0])
    if L == 0:
        assert want == 0.0 and not np.signbit(want)


@pytest.mark.parametrize("gammas", ir.GAMMAS)
@pytest.mark.parametrize("name", list(ir.CLOUDS))
def test_the_definition_against_the_float64_reading(name, gammas):
    """Open3D's defaults for the radii.  The keypoint sets are equal except at points where a comparison of the float64 reading
    lies within 2^-16 relative (a ratio against its gamma, or s_i against an s_j of its non-max row where that comparison
    decides the point -- a subset of all such comparisons, so the exception is the narrower one); at most 1 % of a cloud's
    points are such.  Measured, as keypoints / differing / near: torus 38 / 0 / 2 and 46 / 0 / 0 (gamma 0.6), bumpy600 27 / 1 / 4
    and 42 / 1 / 4, bumpy1500 56 / 2 / 8 and 98 / 3 / 10, cube 2 / 0 / 0 and 16 / 0 / 0."""
    x = ir.CLOUDS[name]()
    N = x.shape[1]
    sr, nr = ir.default_radii(x)
    f = ir.float64_reading(x, sr, nr, *gammas)
    d = ir.of_cloud(x, sr, nr, gamma_21=gammas[0], gamma_32=gammas[1])
    differ = (d["keypoint"] > 0) != f["keypoint"]
    print(name, gammas, "keypoints", int(f["keypoint"].sum()), "differing", int(differ.sum()), "near", int(f["near"].sum()),
          "salient", int((f["saliency"] > 0).sum()), "entries a row", float(np.diff(f["rows"]["row_start"]).mean()))
    assert f["near"].sum() <= 0.01 * N
    assert not (differ & ~f["near"]).any(), np.flatnonzero(differ & ~f["near"])
    assert f["keypoint"].sum() >= 2
    both = f["saliency"] > 0
    assert both.sum() >= 40 and (gammas[0] > 0.9 or (~both).sum() >= N // 2)      # at 0.6 the ratio tests reject most points
    rel = np.abs(d["saliency"] - f["saliency"])[both & (d["saliency"] > 0)] / f["saliency"][both & (d["saliency"] > 0)]
    assert rel.max() <= 1e-5


def test_the_prefix_is_the_row_of_a_second_search():
    """One search at the larger radius and the d2 prefix against two searches: the used lengths are the smaller search's counts,
    the entries its entries, the keypoints the same."""
    for name in ("torus", "cube"):
        x = ir.CLOUDS[name]()
        sr, nr = ir.default_radii(x)
        big, small = rr.radius_rows(x, sr), rr.radius_rows(x, nr)
        u = ir.used_lengths(big["row_start"], big["bits"].view(F32), rr.r2_of(nr))
        assert np.array_equal(u, small["count"])
        for i in range(x.shape[1]):
            assert np.array_equal(big["idx"][big["row_start"][i]:big["row_start"][i] + u[i]],
                                  small["idx"][small["row_start"][i]:small["row_start"][i + 1]])
        one = ir.of_cloud(x, sr, nr)
        two = ir.definition(x, (big["idx"], big["row_start"]), nms_rows=(small["idx"], small["row_start"]))
        assert np.array_equal(one["keypoint"], two["keypoint"]) and one["count"] == two["count"] >= 2
        # the larger non-max radius takes the second search
        wide = ir.of_cloud(x, nr, sr)
        assert wide["count"] <= ir.of_cloud(x, nr, nr)["count"]


def test_copies_of_a_point_are_both_kept():
    """Two points alike have the same row up to each other, the same differences and the same sums: equal saliency, and the
    strict comparison keeps both."""
    x = ir.bumpy(300, seed=5)
    sr, nr = ir.default_radii(x)
    first = ir.of_cloud(x, sr, nr)
    k = int(first["index"][0])
    x = np.concatenate([x, x[:, k:k + 1]], axis=1)
    got = ir.of_cloud(x, sr, nr)
    assert got["saliency"][k] == got["saliency"][300] > 0 and got["keypoint"][k] == got["keypoint"][300] == 1


def test_a_cloud_that_is_not_served_and_a_nan_saliency():
    x, rows, nms_rows, _ = ir.hand_cloud()
    bad = rows[1].copy()
    bad[3] = bad[2] - 1
    got = ir.definition(x, (rows[0], bad), nms_rows=nms_rows)
    assert np.isnan(got["saliency"]).all() and np.isnan(got["eigen"]).all() and (got["keypoint"] == -2).all() and got["count"] == 0
    got = ir.definition(x, rows, nms_rows=(nms_rows[0], nms_rows[1], 99))
    assert got["saliency"][0] == 2.0 / 7.0 and (got["keypoint"] == -2).all() and got["count"] == 0
    got = ir.definition(x, rows, capacity=len(rows[0]) - 1)
    assert np.isnan(got["saliency"]).all() and (got["keypoint"] == -2).all()
    sal = ir.saliency(x, *rows)[0]
    sal[9] = np.nan
    assert (ir.nms(sal, *nms_rows) == -2).all()


def test_the_model_resolution_and_the_default_radii():
    x = np.asarray([[0, 1, 3, 7], [0, 0, 0, 0], [0, 0, 0, 0]], F32)
    assert ir.model_resolution(x) == (1 + 1 + 2 + 4) / 4
    assert ir.default_radii(x) == (float(F32(6 * 2.0)), float(F32(4 * 2.0)))
    x[:, 3] = np.nan                                        # a point that is not finite is nobody's neighbour and not counted
    assert ir.model_resolution(x) == (1 + 1 + 2) / 3


# ---------------------------------------------------------------------------------------------------------------- the boundary

def test_signatures_match_the_header_and_the_library_exports_them(lib):
    from vcrnet_amd import iss
    boundary.check_signatures(HEADER, iss, lib, ENTRY_POINTS)


def test_args_match_the_c_layout(tmp_path):
    import vcrnet_amd  # noqa: F401
    from vcrnet_amd import iss
    assert set(iss.STRUCTS) == {"vcr_rows_iss_saliency_args", "vcr_rows_iss_nms_args", "vcr_iss_select_args"}
    boundary.check_layout(HEADER, iss, tmp_path)
    A = iss.RowsIssSaliencyArgs
    assert A.eigen.offset == A.saliency.offset + 8          # where the mandatory part ends
    S = iss.IssSelectArgs
    assert S.index.offset == S.count.offset + 8


def test_the_header_lives_in_a_directory_of_its_own_and_enters_the_digests(lib, monkeypatch):
    from vcrnet_amd import build, dbscan, iss, native, orient, rows, segment
    assert os.listdir(os.path.join(INCLUDE, "keypoint")) == ["vcr_hip_iss.h"]
    for d in sorted(os.listdir(INCLUDE)):
        for f in ([d] if d.endswith(".h") else os.listdir(os.path.join(INCLUDE, d))):
            h = os.path.join(INCLUDE, f) if d.endswith(".h") else os.path.join(INCLUDE, d, f)
            if h != HEADER:
                assert "_iss_" not in open(h).read(), h
    assert '#include "../vcr_hip.h"' in open(HEADER).read()
    assert lib.vcr_abi_version() == native.ABI_VERSION == 27
    for other in (native, rows, dbscan, segment, orient):
        assert not set(iss.SIGNATURES) & set(other.SIGNATURES) and not set(iss.STRUCTS) & set(other.STRUCTS)
    assert build.ISS_HEADERS == [HEADER]
    assert HEADER not in (build.PUBLIC_HEADERS + build.LATER_HEADERS + build.OUTLIER_HEADERS + build.GICP_HEADERS
                          + build.FPFH_HEADERS + build.MATCH_HEADERS + build.FGR_HEADERS + build.GRID_HEADERS
                          + build.GRIDNN_HEADERS + build.VOXEL_SORT_HEADERS + build.RADIUS_HEADERS + build.ROWS_HEADERS
                          + build.DBSCAN_HEADERS + build.SEGMENT_HEADERS + build.ORIENT_HEADERS)
    full = build.sources_sha16()
    monkeypatch.setattr(build, "ISS_HEADERS", [])
    assert build.sources_sha16() != full
    monkeypatch.undo()
    text = open(HEADER).read()
    for name, value in (("VCR_ISS_MAX_N", iss.MAX_N), ("VCR_ISS_LANE", iss.FORMS["lane"]), ("VCR_ISS_WAVE", iss.FORMS["wave"]),
                        ("VCR_ISS_WAVE_NMS", iss.WAVE_NMS), ("VCR_ISS_NOT_SERVED", "(%d)" % iss.NOT_SERVED)):
        assert "#define %s %s" % (name, value) in text, name
    assert iss.NOT_SERVED == ir.NOT_SERVED


def test_the_form_query_is_the_row_length_rule(lib):
    from vcrnet_amd import iss
    form = lambda *a: lib.vcr_rows_iss_form(*a, None)       # noqa: E731
    N = 1000
    for est in (0, 1, 23, 64, 200, iss.WAVE_NMS - 1, iss.WAVE_NMS, iss.WAVE_NMS + 1):
        for cap in (est * N, est * N + N - 1):              # est = capacity / N, rounded down
            if 2 * cap >= 1 << 31:
                continue
            assert iss.form(2, N, cap) == (2 if est >= iss.WAVE_NMS else 1), cap
            assert iss.form(2, N, cap, variant=1) == 1 and iss.form(2, N, cap, variant=2) == 2
    assert iss.form(1, 1, iss.WAVE_NMS) == 2 and iss.form(1, 1, iss.WAVE_NMS - 1) == 1
    assert iss.form(1, 131072, 131072 * 8191) == (2 if 8191 >= iss.WAVE_NMS else 1)
    for a in ((0, N, N, 0, 0), (-1, N, N, 0, 0), (1, N, -1, 0, 0), (1, N, N, -1, 0), (1, N, N, 0, 3), (1, N, N, 0, -1)):
        assert form(*a) == EINVAL, a
    for a in ((1, 0, 0, 0, 0), (1, -3, 0, 0, 0), (1, 131073, 0, 0, 0), (16384, 131072, 0, 0, 0), (2, N, 1 << 30, 0, 0)):
        assert form(*a) == EUNSUPPORTED, a
    assert form(1, 131072, 0, 7, 0) == 0


def _args(kind, **kw):
    from vcrnet_amd import iss
    a = {"saliency": iss.RowsIssSaliencyArgs, "nms": iss.RowsIssNmsArgs, "select": iss.IssSelectArgs}[kind]()
    for k, f in enumerate(n for n, t in a._fields_ if t is ctypes.c_void_p):       # (never dereferenced)
        setattr(a, f, 0x1000 * (k + 1))
    v = dict(B=2, N=1000)
    if kind != "select":
        v.update(capacity=30000, min_neighbors=5)
    if kind == "saliency":
        v.update(gamma_21=0.975, gamma_32=0.975)
    if kind == "nms":
        v.update(r2_nm=0.25)
    v.update(kw)
    for k, x in v.items():
        setattr(a, k, x)
    return a


WS = 0x100000                                               # a 256-aligned address that is never dereferenced


def test_the_calls_return_their_argument_errors_without_a_gpu(lib):
    sal = lambda **kw: lib.vcr_rows_iss_saliency_f32(ctypes.byref(_args("saliency", **kw)), None)      # noqa: E731
    nms = lambda **kw: lib.vcr_rows_iss_nms_f32(ctypes.byref(_args("nms", **kw)), None)                 # noqa: E731
    assert lib.vcr_rows_iss_saliency_f32(None, None) == EINVAL and lib.vcr_rows_iss_nms_f32(None, None) == EINVAL
    for field in ("xyz4", "idx", "row_start", "total", "saliency"):
        assert sal(**{field: None}) == EINVAL, field
    for field in ("idx", "row_start", "total", "saliency", "keypoint"):
        assert nms(**{field: None}) == EINVAL, field
    assert sal(xyz4=0x1008) == EINVAL
    for fn in (sal, nms):
        for kw in (dict(B=0), dict(capacity=-1), dict(min_neighbors=0), dict(min_neighbors=-2)):
            assert fn(**kw) == EINVAL, kw
        for kw in (dict(N=0), dict(N=131073), dict(B=16384, N=131072), dict(B=4, capacity=1 << 29)):
            assert fn(**kw) == EUNSUPPORTED, kw
    for g in (0.0, -0.5, float("nan"), float("inf")):
        assert sal(gamma_21=g) == EINVAL and sal(gamma_32=g) == EINVAL, g
    for kw in (dict(variant=3), dict(variant=-1), dict(r2_nm=-1.0), dict(r2_nm=float("nan"))):
        assert nms(**kw) == EINVAL, kw
    for kind, fn in (("saliency", lib.vcr_rows_iss_saliency_f32), ("nms", lib.vcr_rows_iss_nms_f32)):
        size = ctypes.sizeof(type(_args(kind)))
        for wrong in (0, size - 16, size + 8):
            a = _args(kind)
            a.struct_bytes = wrong
            assert fn(ctypes.byref(a), None) == EINVAL, (kind, wrong)
    # the selection
    need = lambda a: lib.vcr_iss_select_workspace_bytes(ctypes.byref(a), 0)       # noqa: E731
    f32 = lambda a, ws=WS, n=None: lib.vcr_iss_select_f32(ctypes.byref(a), ws, need(_args("select")) if n is None else n, None)  # noqa: E731
    assert lib.vcr_iss_select_f32(None, WS, 1 << 30, None) == EINVAL and lib.vcr_iss_select_workspace_bytes(None, 0) == 0
    for field in ("xyz", "keypoint", "points", "count"):
        assert f32(_args("select", **{field: None})) == EINVAL and need(_args("select", **{field: None})) == 0, field
    assert need(_args("select", index=None)) == need(_args("select")) > 0
    assert f32(_args("select", B=0)) == EINVAL and need(_args("select", B=0)) == 0
    for kw in (dict(N=0), dict(N=131073), dict(B=16384, N=131072)):
        assert f32(_args("select", **kw), n=1 << 40) == EUNSUPPORTED and need(_args("select", **kw)) == 0, kw
    good = need(_args("select"))
    assert good % 256 == 0 and good >= 4 * 2 * 4
    assert f32(_args("select"), ws=None) == EINVAL and f32(_args("select"), ws=WS + 128) == EINVAL
    assert f32(_args("select"), n=good - 1) == EINVAL and lib.vcr_iss_select_workspace_bytes(ctypes.byref(_args("select")), -1) == 0
    a = _args("select")
    a.struct_bytes = ctypes.sizeof(type(a)) - 8             # a caller that does not know `index` is served
    assert need(a) == good


def test_the_kernels_of_iss_hip_use_no_scratch():
    """hipcc's remarks for iss.hip: its kernel set is the four below, none with scratch, a spill or AGPRs, all at eight waves a
    SIMD; the saliency pass, nine fp64 sums and the Jacobi in registers, stays within 64 VGPRs."""
    import vcrnet_amd  # noqa: F401
    from vcrnet_amd import build
    build.build()
    res = build.kernel_resources()
    names = list(res)
    dem = subprocess.run(["c++filt"], input="\n".join(names), capture_output=True, text=True, check=True).stdout.splitlines()
    by_name = {d.replace("(anonymous namespace)::", "").replace("void ", "").split("(")[0]: res[n] for n, d in zip(names, dem)}
    mine = {d: v for d, v in by_name.items() if v["file"] == "iss.hip"}
    assert set(mine) == KERNELS
    for d, v in mine.items():
        print(d, v)
        assert v.get("scratch", 0) == 0 and v.get("vgpr_spill", 0) == 0 and v.get("sgpr_spill", 0) == 0 and v["agprs"] == 0, (d, v)
        assert v["occupancy"] == 8 and v["vgprs"] <= 64, (d, v)
    assert mine["iss_void_kernel"]["lds"] > 0 and not mine["iss_saliency_kernel"]["lds"]


# ------------------------------------------------------------------------------------------------------------ the Python layer

def test_python_entry_points_refuse_what_they_cannot_run():
    import vcrnet_amd
    from vcrnet_amd import iss, native
    fn = vcrnet_amd.compute_iss_keypoints
    assert fn is iss.compute_iss_keypoints and vcrnet_amd.model_resolution is iss.model_resolution
    assert {"compute_iss_keypoints", "model_resolution"} <= set(vcrnet_amd.__all__) and "iss" not in vcrnet_amd.__all__
    E = native.VcrHipError
    x = torch.zeros(2, 3, 50)
    for bad in (x.transpose(1, 2), torch.zeros(3, 50), None, "xyz"):
        with pytest.raises(E, match=r"compute_iss_keypoints: xyz must be a \[B, 3, N\]"):
            fn(bad)
        with pytest.raises(E, match=r"model_resolution: xyz must be a \[B, 3, N\]"):
            vcrnet_amd.model_resolution(bad)
    with pytest.raises(E, match="a cloud must have 1 ... 131072 points"):
        fn(torch.zeros(1, 3, 131073))
    for name in ("salient_radius", "non_max_radius"):
        for bad in (0.0, -1.0, float("nan"), float("inf"), "r", 1e30):
            with pytest.raises(E, match=f"compute_iss_keypoints: {name} must be finite and > 0"):
                fn(x, **{name: bad})
    for name in ("gamma_21", "gamma_32"):
        for bad in (0.0, -0.1, float("nan"), float("inf"), "g", None, True):
            with pytest.raises(E, match=f"compute_iss_keypoints: {name} must be finite and > 0"):
                fn(x, 0.1, 0.1, **{name: bad})
    for bad in (0, -1, 2.0, "5", True, None):
        with pytest.raises(E, match="compute_iss_keypoints: min_neighbors must be an integer >= 1"):
            fn(x, 0.1, 0.1, min_neighbors=bad)
    with pytest.raises(E, match="model_resolution, which needs at least 2 points"):
        fn(torch.zeros(1, 3, 1), 0.1)
    with pytest.raises(E, match="model_resolution: a nearest other point needs at least 2 points"):
        vcrnet_amd.model_resolution(torch.zeros(1, 3, 1))
    for kw in (dict(), dict(salient_radius=0.2), dict(salient_radius=0.2, non_max_radius=0.1), dict(salient_radius=0.1, non_max_radius=0.2),
               dict(salient_radius=0.2, non_max_radius=0.1, capacity=100, cell=0.3, want_flag=True, want_saliency=True)):
        with pytest.raises(E, match="no CPU fallback"):      # (the last refusal: everything else was in order)
            fn(x, **kw)
    with pytest.raises(E, match="no CPU fallback"):
        vcrnet_amd.model_resolution(x)
    # the raw calls
    N, cap = 50, 64
    xyz4, idx = torch.zeros(2, N, 4), torch.zeros(2, cap, dtype=torch.int32)
    rs, tot = torch.zeros(2, N + 1, dtype=torch.int64), torch.zeros(2, dtype=torch.int64)
    sal, d2 = torch.zeros(2, N, dtype=torch.float64), torch.zeros(2, cap)
    for bad in (xyz4[:, :, :3], xyz4.double(), None):
        with pytest.raises(E, match=r"iss.saliency_rows: xyz4 must be float32 \[B, N, 4\]"):
            iss.saliency_rows(bad, idx, rs, tot)
    for bad in (idx.long(), idx[:1], idx[0], None):
        with pytest.raises(E, match=r"iss.saliency_rows: idx must be int32 \[B, capacity\]"):
            iss.saliency_rows(xyz4, bad, rs, tot)
        with pytest.raises(E, match=r"iss.nms_rows: idx must be int32 \[B, capacity\]"):
            iss.nms_rows(bad, rs, tot, sal)
    for bad in (rs[:, :N], rs.int(), None):
        with pytest.raises(E, match=r"row_start must be int64 \[B, N \+ 1\]"):
            iss.saliency_rows(xyz4, idx, bad, tot)
    for bad in (tot[:1], tot.int(), None):
        with pytest.raises(E, match=r"total must be int64 \[B\]"):
            iss.nms_rows(idx, rs, bad, sal)
    for bad in (sal.float(), sal[0], None):
        with pytest.raises(E, match=r"iss.nms_rows: saliency must be float64 \[B, N\]"):
            iss.nms_rows(idx, rs, tot, bad)
    with pytest.raises(E, match="give both d2 and r2_nm"):
        iss.nms_rows(idx, rs, tot, sal, d2=d2)
    with pytest.raises(E, match="give both d2 and r2_nm"):
        iss.nms_rows(idx, rs, tot, sal, r2_nm=1.0)
    for bad in (d2[:, :cap - 1], d2.double()):
        with pytest.raises(E, match=r"d2 must be None or float32 \[B, capacity\]"):
            iss.nms_rows(idx, rs, tot, sal, d2=bad, r2_nm=1.0)
    for bad in (-1.0, float("nan"), "r"):
        with pytest.raises(E, match="r2_nm must be >= 0"):
            iss.nms_rows(idx, rs, tot, sal, d2=d2, r2_nm=bad)
    for bad in ("block", 3, True):
        with pytest.raises(E, match="iss.nms_rows: variant must be 0"):
            iss.nms_rows(idx, rs, tot, sal, variant=bad)
    with pytest.raises(E, match="gamma_21 must be finite"):
        iss.saliency_rows(xyz4, idx, rs, tot, gamma_21=0.0)
    with pytest.raises(E, match="min_neighbors must be an integer >= 1"):
        iss.nms_rows(idx, rs, tot, sal, min_neighbors=0)
    for bad in (torch.zeros(2, N), torch.zeros(2, N + 1, dtype=torch.int32), None):
        with pytest.raises(E, match=r"iss.select: keypoint must be int32 \[B, N\]"):
            iss.select(x, bad)
    with pytest.raises(E, match="no CPU fallback"):
        iss.select(x, torch.zeros(2, N, dtype=torch.int32))
    for call in (lambda: iss.saliency_rows(xyz4, idx, rs, tot, want_eigen=True), lambda: iss.nms_rows(idx, rs, tot, sal, variant="wave"),
                 lambda: iss.nms_rows(idx, rs, tot, sal, d2=d2, r2_nm=1.0)):
        with pytest.raises(E, match="no CPU fallback|device tensors only"):
            call()


def test_register_features_takes_keypoints_and_refuses_other_values():
    import inspect
    import vcrnet_amd
    from vcrnet_amd import match, native
    params = inspect.signature(match.register_features).parameters
    assert params["keypoints"].default is None and params["iss"].default is None
    names = list(params)
    assert names.index("keypoints") + 1 == names.index("iss") and names[-2:] == ["orient", "orient_k"]
    E = native.VcrHipError
    x = torch.zeros(1, 3, 64)
    for bad in ("ISS", "harris", True, 1, ""):
        for kw in (dict(), dict(method="fgr"), dict(centre=True)):
            with pytest.raises(E, match='register_features: keypoints must be None or "iss"'):
                vcrnet_amd.register_features(x, x, 0.1, keypoints=bad, **kw)
    for bad in (5, "x", dict(radius=1.0), dict(want_flag=True)):
        with pytest.raises(E, match="register_features: iss must be None or a dict with keys among"):
            vcrnet_amd.register_features(x, x, 0.1, keypoints="iss", iss=bad)
    with pytest.raises(E, match='iss= holds the keywords of keypoints="iss"'):
        vcrnet_amd.register_features(x, x, 0.1, iss=dict(min_neighbors=3))
    for kw in (dict(), dict(method="fgr")):
        with pytest.raises(E, match="register_features: gamma_21 must be finite"):
            vcrnet_amd.register_features(x, x, 0.1, k=10, keypoints="iss", iss=dict(gamma_21=-1.0), **kw)
        with pytest.raises(E, match="no CPU fallback"):
            vcrnet_amd.register_features(x, x, 0.1, k=10, keypoints="iss", iss=dict(salient_radius=0.2), **kw)
