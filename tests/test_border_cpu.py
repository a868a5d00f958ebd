"""Boundary points without a GPU (include/border/vcr_hip_border.h): the restatement
(tests/border_restated.py) against surfaces whose rim is known by construction, the header against the ctypes binding and the
library's exports, the place of the header among the others and in the digests, the argument errors of the C entry points and of
the Python layer, and the resource remarks of border.hip."""
import ctypes
import inspect
import math
import os
import subprocess

import numpy as np
import pytest
import torch

import border_restated as br
import boundary
import iss_restated as ir
import radius_restated as rr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INCLUDE = os.path.join(ROOT, "include")
HEADER = os.path.join(INCLUDE, "border", "vcr_hip_border.h")
ENTRY_POINTS = ("vcr_border_angles_f32", "vcr_border_gap_f32", "vcr_border_form", "vcr_border_near_f32")
KERNELS = {"border_angles_kernel", "border_gap_lane_kernel", "border_gap_wave_kernel", "border_near_kernel", "border_void_kernel"}
BANNED = ("_iss_", "vcr_query", "VCR_QUERY", "orient_tangent", "vcr_posegraph", "VCR_POSEGRAPH", "vcr_refine_colored",
          "vcr_color_gradient", "vcr_refine_robust", "vcr_information", "VCR_LOSS")
EINVAL, EUNSUPPORTED = -1, -3
F32 = np.float32


@pytest.fixture(scope="module")
def lib():
    import vcrnet_amd  # noqa: F401
    from vcrnet_amd import border, build
    build.build()
    return border.lib()


# --------------------------------------------------------------------------------------------------------------- the definition

def test_two_pi_and_the_threshold_in_degrees():
    import vcrnet_amd  # noqa: F401
    from vcrnet_amd import border
    assert np.float64(br.TWO_PI).view(np.uint64) == 0x401921FB54442D18 == np.float64(border.TWO_PI).view(np.uint64)
    assert br.TWO_PI == 2.0 * math.pi
    for deg in (0.0, 45.0, 90.0, 117.3, 180.0):
        assert br.radians(deg) == border.radians(deg) == deg * (math.pi / 180.0)


def test_a_frame_worked_by_hand():
    """n = (0, 0, 2): nh = (0, 0, 1), the smallest |nh_a| is at axis 0 (the lowest among equals), u = nh x e_x = (0, 1, 0), v = nh x u
    = (-1, 0, 0).  Four neighbours on the axes: atan2(pv, pu) = atan2(-dx, dy)."""
    u, v = br.frame([0, 0, 0], [0, 0, 2])
    assert u == [0.0, 1.0, 0.0] and v == [-1.0, 0.0, 0.0]
    u, v = br.frame([0, 0, 0], [3, 0, 0])                    # axis 1: e_y; u = (0, 0, 1) up to the sign of a zero, v = (0, -1, 0)
    assert [abs(c) for c in u] == [0.0, 0.0, 1.0] and [abs(c) for c in v] == [0.0, 1.0, 0.0] and v[1] == -1.0
    for bad_n in ([0, 0, 0], [np.nan, 0, 1], [np.inf, 0, 0], [1e-30, 0, 0]):      # (1e-30 as fp32, squared in fp64: > 0, a frame)
        got = br.frame([0, 0, 0], np.asarray(bad_n, F32))
        assert (got is None) == (bad_n[0] != 1e-30), bad_n
    assert br.frame([np.nan, 0, 0], [0, 0, 1]) is None and br.frame([0, np.inf, 0], [0, 0, 1]) is None
    x = np.asarray([[0, 1, 0, -1, 0], [0, 0, 1, 0, -1], [0, 0, 0, 0, 0]], F32)
    nrm = np.zeros((3, 5), F32)
    nrm[2] = 2
    idx, row_start = ir.flat([[1, 2, 3, 4], [0], [0], [0], [0]])
    ang, fr, skipped = br.angles(x, nrm, idx, row_start)
    assert fr.tolist() == [1] * 5 and not skipped.any()
    assert ang[:4].tolist() == [math.atan2(-1.0, 0.0), math.atan2(-0.0, 1.0), math.atan2(1.0, -0.0), math.atan2(0.0, -1.0)]
    gap, flag = br.gaps(ang, row_start, 3, math.pi / 2, fr)
    assert gap[0] == math.pi / 2 and flag[0] == 0             # four quarters: the gap IS the threshold, and the comparison is strict
    assert br.gaps(ang, row_start, 3, br.radians(89.0), fr)[1][0] == 1
    assert gap[1:].tolist() == [0.0] * 4 and not flag[1:].any()              # m = 2 < 3
    g2, f2 = br.gaps(ang, row_start, 2, math.pi / 2, fr)
    assert (g2[1:] == br.TWO_PI).all() and f2[1:].all()     # a single angle: all the way round


def test_a_single_angle_gives_two_pi():
    """(TWO_PI - a) + a is TWO_PI for every a >= 0 and for the negative angles whose sum with TWO_PI stays below 8; beyond it is
    within one unit in the last place (the header says so)."""
    rs = np.random.RandomState(0)
    for a in np.concatenate([rs.uniform(0, math.pi, 2000), rs.uniform(-(8 - br.TWO_PI), 0, 2000), [0.0, math.pi, 1e-300, 2.0 ** -51]]):
        assert br.gap_of([a], 2, 1) == br.TWO_PI, a
    for a in rs.uniform(-math.pi, -(8 - br.TWO_PI), 2000):
        assert abs(br.gap_of([a], 2, 1) - br.TWO_PI) <= 2.0 ** -50, a
    assert br.gap_of([np.nan, 0.25, np.nan], 4, 3) == br.TWO_PI and br.gap_of([0.25, 0.25], 3, 3) == br.TWO_PI      # copies: one angle
    assert br.gap_of([0.25], 2, 3) == 0.0 and br.gap_of([np.nan, np.nan], 3, 3) == 0.0 and br.gap_of([], 1, 1) == 0.0


def test_the_gap_is_free_of_any_order_and_counts_copies_once():
    rs = np.random.RandomState(1)
    for L in (2, 3, 17, 64, 65, 300):
        a = rs.uniform(-math.pi, math.pi, L)
        a[rs.uniform(size=L) < 0.2] = np.nan
        a[-1] = a[0]
        want = br.gap_of(a, L + 1)
        for _ in range(3):
            assert br.gap_of(rs.permutation(a), L + 1) == want
        # the definition read literally: every counted angle's successor
        c = a[~np.isnan(a)]
        if len(c):
            diffs = [min(c[c > x]) - x for x in c if (c > x).any()]
            assert want == max(diffs + [(br.TWO_PI - c.max()) + c.min()])


def test_copies_and_nan_points_are_skipped_and_a_nan_point_has_no_frame():
    x, nrm, _ = br.lattice(6)
    N = x.shape[1]
    x = np.concatenate([x, x[:, 14:15]], axis=1)             # a copy of point 14 ...
    nrm = np.concatenate([nrm, nrm[:, 14:15]], axis=1)
    x[:, 20] = np.nan                                       # ... and a NaN point
    rows = [[j for j in range(N + 1) if j != i] for i in range(N + 1)]
    rows[3] = rows[3] + [-1, N + 9]                         # entries that read as the point itself
    idx, row_start = ir.flat(rows)
    ang, fr, skipped = br.angles(x, nrm, idx, row_start)
    assert fr[20] == 0 and fr.sum() == N and skipped[row_start[20]:row_start[21]].all()
    for i in range(N + 1):
        if i == 20:
            continue
        sk = skipped[row_start[i]:row_start[i + 1]]
        want = [j == 20 or (i in (14, N) and j in (14, N)) or not 0 <= j <= N for j in rows[i]]
        assert sk.tolist() == want, i
    gap, flag = br.gaps(ang, row_start, 3, br.radians(90.0), fr)
    assert np.isnan(gap[20]) and flag[20] == 0 and not np.isnan(np.delete(gap, 20)).any()
    assert gap[14] == gap[N] and flag[14] == flag[N]        # a point and its copy: the same differences, the same angles


def test_the_prefix_is_the_row_of_a_second_search():
    x, nrm = br.sphere(300)
    big, small = rr.radius_rows(x, 0.6), rr.radius_rows(x, 0.35)
    d2, r2 = big["bits"].view(F32), rr.r2_of(0.35)
    one = br.definition(x, nrm, (big["idx"], big["row_start"]), d2=d2, r2=r2)
    two = br.definition(x, nrm, (small["idx"], small["row_start"]))
    assert np.array_equal(one["gap"].view(np.uint64), two["gap"].view(np.uint64)) and np.array_equal(one["flag"], two["flag"])
    flag = (np.arange(300) % 37 == 0).astype(np.int32)
    assert np.array_equal(br.near(flag, big["idx"], big["row_start"], d2, r2), br.near(flag, small["idx"], small["row_start"]))
    assert br.near(flag, small["idx"], small["row_start"]).sum() > flag.sum()
    flag[5] = -2
    assert (br.near(flag, small["idx"], small["row_start"]) == -2).all()


# ------------------------------------------------------------------------------------------- surfaces whose rim is known

def test_the_lattice_flags_exactly_its_outer_ring():
    x, nrm, ring = br.lattice()
    got = br.of_cloud(x, nrm, 1.6)
    assert np.array_equal(got["flag"] > 0, ring) and got["count"] == ring.sum() == 60
    assert np.array_equal(got["index"][:60], np.flatnonzero(ring)) and (got["index"][60:] == -1).all()
    inner = got["gap"][~ring]
    assert inner.max() < br.radians(63.0) and got["gap"][ring].min() > br.radians(150.0)
    corners = [0, 15, 240, 255]
    assert (got["gap"][corners] > br.radians(240.0)).all()
    res = br.hybrid_rows(x, 1.6)
    assert set(res["count"][~ring].tolist()) == {8} and set(res["count"][ring].tolist()) == {3, 5}


def test_the_closed_sphere_flags_nothing():
    x, nrm = br.sphere()
    res = br.hybrid_rows(x, br.SPHERE_RADIUS)
    assert res["count"].min() >= 10 and res["count"].max() <= 30            # (the cap of 30 cuts no row)
    got = br.of_cloud(x, nrm, br.SPHERE_RADIUS)
    assert not got["flag"].any() and got["count"] == 0 and got["gap"].max() < br.radians(90.0) and got["gap"].min() > 0


def test_the_capped_sphere_flags_the_points_at_the_cut():
    """By construction: a point no removed point was within one radius of keeps its row's points, hence the closed sphere's gap,
    bit for bit -- it is not flagged.  A point within 0.4 radii of the cut has lost the part of its disc beyond a chord that
    subtends 2 acos 0.4 = 133 degrees at it -- it is flagged.  Between the two the lattice decides (a point that lost one far
    neighbour of fifteen has no gap of 90 degrees): the flagged set is held between them, not to either."""
    x, nrm, keep = br.capped()
    closed = br.of_cloud(*br.sphere(), br.SPHERE_RADIUS)
    got = br.of_cloud(x, nrm, br.SPHERE_RADIUS)
    touched = br.touched()
    assert np.array_equal(got["gap"][~touched].view(np.uint64), closed["gap"][keep][~touched].view(np.uint64))
    flagged = got["flag"] > 0
    assert not (flagged & ~touched).any()
    # the distance along the sphere to the cut's circle of latitude
    t = np.arcsin(np.float64(br.CUT)) - np.arcsin(np.clip(x[2].astype(np.float64), -1, 1))
    assert (t >= 0).all() and flagged[t <= 0.4 * br.SPHERE_RADIUS].all()
    assert 20 <= flagged.sum() < touched.sum() and (t <= 0.4 * br.SPHERE_RADIUS).sum() >= 20
    print("capped sphere: points", x.shape[1], "flagged", int(flagged.sum()), "touched", int(touched.sum()),
          "within 0.4 r", int((t <= 0.4 * br.SPHERE_RADIUS).sum()))


@pytest.mark.parametrize("name", list(br.RECIPES))
def test_no_gap_of_a_recipe_lies_at_the_threshold(name):
    """The condition under which the GPU tests compare every flag: a device angle differs from numpy's by 1e-12 at the most, a gap
    by twice that, so a gap farther than 1e-9 from the threshold falls on the same side."""
    make, radius = br.RECIPES[name]
    x, nrm = make()
    for max_nn in (30, None):
        got = br.of_cloud(x, nrm, radius, max_nn)
        gap = got["gap"][~np.isnan(got["gap"])]              # (a point without a frame has no gap to compare)
        assert np.abs(gap - br.radians(90.0)).min() > br.MARGIN, (name, max_nn)
    for seed in (12, 13):                                   # the batch of the GPU test
        lx, ln, _ = br.lattice(seed=seed)
        assert np.abs(br.of_cloud(lx, ln, 1.6)["gap"] - br.radians(90.0)).min() > br.MARGIN, seed


# ---------------------------------------------------------------------------------------------------------------- the boundary

def test_signatures_match_the_header_and_the_library_exports_them(lib):
    from vcrnet_amd import border
    boundary.check_signatures(HEADER, border, lib, ENTRY_POINTS)


def test_args_match_the_c_layout(tmp_path):
    import vcrnet_amd  # noqa: F401
    from vcrnet_amd import border
    assert set(border.STRUCTS) == {"vcr_border_angles_args", "vcr_border_gap_args", "vcr_border_near_args"}
    boundary.check_layout(HEADER, border, tmp_path)
    A = border.BorderAnglesArgs
    assert A.frame.offset == A.angle.offset + 8             # where the mandatory part ends


def test_the_other_boundaries_are_where_they_were(lib):
    """The header is alone in a directory of its own and includes its base by relative path; it carries no other family's call
    name; ABI 27, the same 51 prototypes; it enters the digest of border.o ALONE and not the profiles' digest; the header's
    numbers are the module's."""
    import vcrnet_amd
    from vcrnet_amd import border, build, iss, native, rows
    assert os.listdir(os.path.join(INCLUDE, "border")) == ["vcr_hip_border.h"]
    text = open(HEADER).read()
    for word in BANNED:
        assert word not in text, word
    for dirpath, _, files in os.walk(INCLUDE):
        for f in files:
            path = os.path.join(dirpath, f)
            if path != HEADER:
                other = open(path).read()
                assert "vcr_border" not in other and "VCR_BORDER" not in other, path
    assert '#include "../vcr_hip.h"' in text and text.count("#include") == 1
    assert len(native.PUBLIC) == 51 and lib.vcr_abi_version() == native.ABI_VERSION == 27
    for other in (native, rows, iss):
        assert not set(border.SIGNATURES) & set(other.SIGNATURES) and not set(border.STRUCTS) & set(other.STRUCTS)
    assert all(n.startswith("vcr_border_") for n in border.SIGNATURES)
    assert build.BORDER_HEADERS == [HEADER] and build.OWN_HEADERS["border.hip"] == [HEADER]
    assert [k for k, v in build.OWN_HEADERS.items() if HEADER in v] == ["border.hip"]
    flags = " ".join(build.FLAGS)
    hdrs = sorted(os.path.join(build.CSRC, f) for f in os.listdir(build.CSRC) if f.endswith(".h"))
    hdrs += (build.PUBLIC_HEADERS + build.LATER_HEADERS + build.OUTLIER_HEADERS + build.GICP_HEADERS + build.FPFH_HEADERS
             + build.MATCH_HEADERS + build.FGR_HEADERS + build.GRID_HEADERS + build.GRIDNN_HEADERS + build.VOXEL_SORT_HEADERS
             + build.RADIUS_HEADERS + build.ROWS_HEADERS + build.DBSCAN_HEADERS + build.SEGMENT_HEADERS + build.ORIENT_HEADERS
             + build.ISS_HEADERS + build.QUERY_HEADERS)
    assert HEADER not in hdrs
    sha = lambda name: open(os.path.join(build.OBJ, name + ".o.sha")).read()    # noqa: E731 (build() ran in the fixture)
    src = lambda name: os.path.join(build.CSRC, name + ".hip")                  # noqa: E731
    assert sha("border") == build._digest([src("border")] + hdrs + [HEADER], flags) != build._digest([src("border")] + hdrs, flags)
    for name in ("iss", "rows", "radius", "forward"):
        assert sha(name) == build._digest([src(name)] + hdrs, flags), name
    assert sha("posegraph") == build._digest([src("posegraph")] + hdrs + build.POSEGRAPH_HEADERS, flags)
    source = open(src("border")).read()
    assert "atomic" not in source.replace("No atomics", "") and "hipMalloc" not in source and "Synchronize" not in source
    assert "compute_boundary_points" in vcrnet_amd.__all__ and "border" not in vcrnet_amd.__all__
    assert vcrnet_amd.compute_boundary_points is border.compute_boundary_points
    for name, value in (("VCR_BORDER_MAX_N", border.MAX_N), ("VCR_BORDER_LANE", border.FORMS["lane"]),
                        ("VCR_BORDER_WAVE", border.FORMS["wave"]), ("VCR_BORDER_CHUNK", border.CHUNK),
                        ("VCR_BORDER_WAVE_GAP", border.WAVE_GAP), ("VCR_BORDER_NOT_SERVED", "(%d)" % border.NOT_SERVED)):
        assert "#define %s %s" % (name, value) in text, name
    assert border.NOT_SERVED == br.NOT_SERVED == iss.NOT_SERVED and border.CHUNK == br.CHUNK and border.MAX_N == iss.MAX_N
    assert "0x401921FB54442D18" in text


def test_the_form_query_is_the_row_length_rule(lib):
    from vcrnet_amd import border
    form = lambda *a: lib.vcr_border_form(*a, None)         # noqa: E731
    N = 1000
    for est in (0, 1, border.WAVE_GAP - 1, border.WAVE_GAP, border.WAVE_GAP + 1, 64, 200):
        for cap in (est * N, est * N + N - 1):              # est = capacity / N, rounded down
            assert border.form(2, N, cap) == (2 if est >= border.WAVE_GAP else 1), cap
            assert border.form(2, N, cap, variant=1) == 1 and border.form(2, N, cap, variant=2) == 2
    assert border.form(1, 1, border.WAVE_GAP) == 2 and border.form(1, 1, border.WAVE_GAP - 1) == 1
    for a in ((0, N, N, 0, 0), (-1, N, N, 0, 0), (1, N, -1, 0, 0), (1, N, N, -1, 0), (1, N, N, 0, 3), (1, N, N, 0, -1)):
        assert form(*a) == EINVAL, a
    for a in ((1, 0, 0, 0, 0), (1, -3, 0, 0, 0), (1, 131073, 0, 0, 0), (16384, 131072, 0, 0, 0), (2, N, 1 << 30, 0, 0)):
        assert form(*a) == EUNSUPPORTED, a
    assert form(1, 131072, 0, 7, 0) == 0


def _args(kind, **kw):
    from vcrnet_amd import border
    a = {"angles": border.BorderAnglesArgs, "gap": border.BorderGapArgs, "near": border.BorderNearArgs}[kind]()
    for k, f in enumerate(n for n, t in a._fields_ if t is ctypes.c_void_p):       # (never dereferenced)
        setattr(a, f, 0x1000 * (k + 1))
    v = dict(B=2, N=1000, capacity=30000)
    if kind == "gap":
        v.update(min_neighbors=3, angle_threshold=1.5, r2=0.25)
    else:
        v.update(r2=0.25)
    v.update(kw)
    for k, x in v.items():
        setattr(a, k, x)
    return a


def test_the_calls_return_their_argument_errors_without_a_gpu(lib):
    ang = lambda **kw: lib.vcr_border_angles_f32(ctypes.byref(_args("angles", **kw)), None)       # noqa: E731
    gap = lambda **kw: lib.vcr_border_gap_f32(ctypes.byref(_args("gap", **kw)), None)             # noqa: E731
    near = lambda **kw: lib.vcr_border_near_f32(ctypes.byref(_args("near", **kw)), None)          # noqa: E731
    for fn in (lib.vcr_border_angles_f32, lib.vcr_border_gap_f32, lib.vcr_border_near_f32):
        assert fn(None, None) == EINVAL
    for field in ("xyz4", "normals", "idx", "row_start", "total", "angle"):
        assert ang(**{field: None}) == EINVAL, field
    for field in ("angle", "row_start", "total", "gap", "flag"):
        assert gap(**{field: None}) == EINVAL, field
    for field in ("flag", "idx", "row_start", "total", "near"):
        assert near(**{field: None}) == EINVAL, field
    assert ang(xyz4=0x1008) == EINVAL
    for fn in (ang, gap, near):
        for kw in (dict(B=0), dict(capacity=-1), dict(r2=-1.0), dict(r2=float("nan"))):
            assert fn(**kw) == EINVAL, kw
        for kw in (dict(N=0), dict(N=131073), dict(B=16384, N=131072), dict(B=4, capacity=1 << 29)):
            assert fn(**kw) == EUNSUPPORTED, kw
    for kw in (dict(min_neighbors=0), dict(min_neighbors=-2), dict(angle_threshold=float("nan")), dict(variant=3), dict(variant=-1)):
        assert gap(**kw) == EINVAL, kw
    for kind, fn in (("angles", lib.vcr_border_angles_f32), ("gap", lib.vcr_border_gap_f32), ("near", lib.vcr_border_near_f32)):
        size = ctypes.sizeof(type(_args(kind)))
        for wrong in (0, size - 32, size + 8):
            a = _args(kind)
            a.struct_bytes = wrong
            assert fn(ctypes.byref(a), None) == EINVAL, (kind, wrong)


def test_the_kernels_of_border_hip_use_no_scratch():
    """hipcc's remarks for border.hip: its kernel set is the five below, none with scratch, a spill or AGPRs; the fp64 atan2 of
    the angles pass stays within 96 VGPRs, every other kernel runs at eight waves a SIMD; LDS in the wave form (a chunk of
    doubles) and in the check's vote alone."""
    import vcrnet_amd  # noqa: F401
    from vcrnet_amd import border, build
    build.build()
    res = build.kernel_resources()
    names = list(res)
    dem = subprocess.run(["c++filt"], input="\n".join(names), capture_output=True, text=True, check=True).stdout.splitlines()
    by_name = {d.replace("(anonymous namespace)::", "").replace("void ", "").split("(")[0]: res[n] for n, d in zip(names, dem)}
    mine = {d: v for d, v in by_name.items() if v["file"] == "border.hip"}
    assert set(mine) == KERNELS
    for d, v in mine.items():
        print(d, v)
        assert v.get("scratch", 0) == 0 and v.get("vgpr_spill", 0) == 0 and v.get("sgpr_spill", 0) == 0 and v["agprs"] == 0, (d, v)
        assert v["vgprs"] <= 96 and (v["occupancy"] == 8 or d == "border_angles_kernel"), (d, v)
    assert mine["border_gap_wave_kernel"]["lds"] == 8 * border.CHUNK and mine["border_void_kernel"]["lds"] > 0
    assert not mine["border_angles_kernel"]["lds"] and not mine["border_gap_lane_kernel"]["lds"] and not mine["border_near_kernel"]["lds"]


# ------------------------------------------------------------------------------------------------------------ the Python layer

def test_python_entry_points_refuse_what_they_cannot_run():
    import vcrnet_amd
    from vcrnet_amd import border, native
    fn = vcrnet_amd.compute_boundary_points
    E = native.VcrHipError
    params = inspect.signature(fn).parameters
    assert list(params) == ["xyz", "normals", "radius", "max_nn", "angle_threshold", "min_neighbors", "capacity", "cell",
                            "want_flag", "want_gap"]
    assert (params["max_nn"].default, params["angle_threshold"].default, params["min_neighbors"].default) == (30, 90.0, 3)
    x = torch.zeros(2, 3, 50)
    for bad in (x.transpose(1, 2), torch.zeros(3, 50), None, "xyz"):
        with pytest.raises(E, match=r"compute_boundary_points: xyz must be a \[B, 3, N\]"):
            fn(bad, radius=0.1)
    with pytest.raises(E, match="a cloud must have 1 ... 131072 points"):
        fn(torch.zeros(1, 3, 131073), radius=0.1)
    with pytest.raises(E, match="compute_boundary_points: radius has no default"):
        fn(x)
    for bad in (0.0, -1.0, float("nan"), float("inf"), "r", 1e30):
        with pytest.raises(E, match="compute_boundary_points: radius must be finite and > 0"):
            fn(x, radius=bad)
    for bad in (torch.zeros(2, 3, 49), torch.zeros(1, 3, 50), torch.zeros(2, 50, 3), "n"):
        with pytest.raises(E, match=r"compute_boundary_points: normals must be None or a \[B, 3, N\]"):
            fn(x, bad, 0.1)
    for bad in (0, -1, 63, 2.0, "5", True):
        with pytest.raises(E, match=r"compute_boundary_points: max_nn must be None or an integer in \[1, 62\]"):
            fn(x, radius=0.1, max_nn=bad)
    for bad in (-1.0, float("nan"), float("inf"), "a", None, True):
        with pytest.raises(E, match="compute_boundary_points: angle_threshold must be finite and >= 0"):
            fn(x, radius=0.1, angle_threshold=bad)
    for bad in (0, -1, 2.0, "5", True, None):
        with pytest.raises(E, match="compute_boundary_points: min_neighbors must be an integer >= 1"):
            fn(x, radius=0.1, min_neighbors=bad)
    with pytest.raises(E, match="compute_boundary_points: capacity must be None or an integer >= 0"):
        fn(x, radius=0.1, capacity=-1)
    for kw in (dict(), dict(max_nn=None), dict(normals=torch.zeros(2, 3, 50)), dict(capacity=100, cell=0.3, want_flag=True, want_gap=True)):
        with pytest.raises(E, match="no CPU fallback"):      # (the last refusal: everything else was in order)
            fn(x, radius=0.1, **kw)
    # the raw calls
    N, cap = 50, 64
    xyz4, nrm, idx = torch.zeros(2, N, 4), torch.zeros(2, 3, N), torch.zeros(2, cap, dtype=torch.int32)
    rs, tot = torch.zeros(2, N + 1, dtype=torch.int64), torch.zeros(2, dtype=torch.int64)
    ang, d2, flag = torch.zeros(2, cap, dtype=torch.float64), torch.zeros(2, cap), torch.zeros(2, N, dtype=torch.int32)
    for bad in (xyz4[:, :, :3], xyz4.double(), None):
        with pytest.raises(E, match=r"border.angles_rows: xyz4 must be float32 \[B, N, 4\]"):
            border.angles_rows(bad, nrm, idx, rs, tot)
    for bad in (nrm.double(), nrm[:, :, :N - 1], nrm.transpose(1, 2), None):
        with pytest.raises(E, match=r"border.angles_rows: normals must be float32 \[B, 3, N\]"):
            border.angles_rows(xyz4, bad, idx, rs, tot)
    for bad in (idx.long(), idx[:1], idx[0], None):
        with pytest.raises(E, match=r"border.angles_rows: idx must be int32 \[B, capacity\]"):
            border.angles_rows(xyz4, nrm, bad, rs, tot)
        with pytest.raises(E, match=r"border.near_rows: idx must be int32 \[B, capacity\]"):
            border.near_rows(flag, bad, rs, tot)
    for bad in (rs[:, :N], rs.int(), None):
        with pytest.raises(E, match=r"row_start must be int64 \[B, N \+ 1\]"):
            border.angles_rows(xyz4, nrm, idx, bad, tot)
    for bad in (rs.int(), rs[:1], rs[:, :1], None):
        with pytest.raises(E, match=r"border.gap_rows: row_start must be int64 \[B, N \+ 1\]"):
            border.gap_rows(ang, bad, tot)
    for bad in (tot[:1], tot.int(), None):
        with pytest.raises(E, match=r"total must be int64 \[B\]"):
            border.gap_rows(ang, rs, bad)
        with pytest.raises(E, match=r"total must be int64 \[B\]"):
            border.near_rows(flag, idx, rs, bad)
    for bad in (ang.float(), ang[0], None):
        with pytest.raises(E, match=r"border.gap_rows: angle must be float64 \[B, capacity\]"):
            border.gap_rows(bad, rs, tot)
    for bad in (flag.long(), flag[0], None):
        with pytest.raises(E, match=r"border.near_rows: flag must be int32 \[B, N\]"):
            border.near_rows(bad, idx, rs, tot)
    for bad in (flag.long(), flag[:, :N - 1]):
        with pytest.raises(E, match=r"border.gap_rows: frame must be None or int32 \[B, N\]"):
            border.gap_rows(ang, rs, tot, frame=bad)
    for call in (lambda **kw: border.angles_rows(xyz4, nrm, idx, rs, tot, **kw), lambda **kw: border.gap_rows(ang, rs, tot, **kw),
                 lambda **kw: border.near_rows(flag, idx, rs, tot, **kw)):
        with pytest.raises(E, match="give both d2 and r2"):
            call(d2=d2)
        with pytest.raises(E, match="give both d2 and r2"):
            call(r2=1.0)
        for bad in (d2[:, :cap - 1], d2.double()):
            with pytest.raises(E, match=r"d2 must be None or float32 \[B, capacity\]"):
                call(d2=bad, r2=1.0)
        for bad in (-1.0, float("nan"), "r"):
            with pytest.raises(E, match="r2 must be >= 0"):
                call(d2=d2, r2=bad)
    for bad in ("block", 3, True):
        with pytest.raises(E, match="border.gap_rows: variant must be 0"):
            border.gap_rows(ang, rs, tot, variant=bad)
    with pytest.raises(E, match="min_neighbors must be an integer >= 1"):
        border.gap_rows(ang, rs, tot, min_neighbors=0)
    with pytest.raises(E, match="angle_threshold must be finite and >= 0"):
        border.gap_rows(ang, rs, tot, angle_threshold=float("nan"))
    for call in (lambda: border.angles_rows(xyz4, nrm, idx, rs, tot, want_frame=True), lambda: border.gap_rows(ang, rs, tot, variant="wave"),
                 lambda: border.near_rows(flag, idx, rs, tot, d2=d2, r2=1.0)):
        with pytest.raises(E, match="no CPU fallback|device tensors only"):
            call()


def test_the_keypoint_call_takes_the_border_rule_and_refuses_other_values():
    import vcrnet_amd
    from vcrnet_amd import iss, match, native
    params = inspect.signature(iss.compute_iss_keypoints).parameters
    assert list(params)[-4:] == ["border_radius", "normal_radius", "border_angle", "normals"]
    assert [params[k].default for k in list(params)[-4:]] == [None, None, 90.0, None]
    assert {"border_radius", "normal_radius", "border_angle", "normals"} <= set(match.ISS_KEYWORDS)
    E = native.VcrHipError
    fn = vcrnet_amd.compute_iss_keypoints
    x = torch.zeros(2, 3, 50)
    for name in ("border_radius", "normal_radius"):
        for bad in (0.0, -1.0, float("nan"), float("inf"), "r", 1e30):
            with pytest.raises(E, match=f"compute_iss_keypoints: {name} must be finite and > 0"):
                fn(x, 0.2, 0.1, **{"border_radius": 0.1, name: bad})
    for bad in (-1.0, float("nan"), "a", None):
        with pytest.raises(E, match="compute_iss_keypoints: border_angle must be finite and >= 0"):
            fn(x, 0.2, 0.1, border_radius=0.1, border_angle=bad)
    with pytest.raises(E, match="normal_radius belongs to border_radius"):
        fn(x, 0.2, 0.1, normal_radius=0.1)
    with pytest.raises(E, match="normals belong to border_radius"):
        fn(x, 0.2, 0.1, normals=torch.zeros(2, 3, 50))
    with pytest.raises(E, match=r"compute_iss_keypoints: normals must be None or a \[B, 3, N\]"):
        fn(x, 0.2, 0.1, border_radius=0.1, normals=torch.zeros(2, 3, 49))
    for kw in (dict(border_radius=0.1), dict(border_radius=0.3, normal_radius=0.2), dict(border_radius=0.1, normals=torch.zeros(2, 3, 50))):
        with pytest.raises(E, match="no CPU fallback"):
            fn(x, 0.2, 0.1, **kw)
    for kw in (dict(), dict(method="fgr")):
        with pytest.raises(E, match="register_features: border_radius must be finite and > 0"):
            vcrnet_amd.register_features(x[:1], x[:1], 0.1, k=10, keypoints="iss", iss=dict(border_radius=-1.0), **kw)
        with pytest.raises(E, match="register_features: border_angle must be finite and >= 0"):
            vcrnet_amd.register_features(x[:1], x[:1], 0.1, k=10, keypoints="iss", iss=dict(border_radius=0.1, border_angle=-3), **kw)
        with pytest.raises(E, match="no CPU fallback"):
            vcrnet_amd.register_features(x[:1], x[:1], 0.1, k=10, keypoints="iss",
                                         iss=dict(salient_radius=0.2, non_max_radius=0.1, border_radius=0.1), **kw)
