"""segment_plane without a GPU: the numpy restatement (tests/segment_restated.py) -- its trial-by-trial loops against its
vectorised form, a planted plane it must recover on its own -- the boundary of include/segment/vcr_hip_segment.h (prototypes
against vcrnet_amd.segment.SIGNATURES, the structs against gcc's layout, the header's place and numbers), every argument error of
the calls and of the Python functions, the host-only form query, and the resource remarks of segment.hip."""
import ctypes
import os
import subprocess

import numpy as np
import pytest
import torch

import boundary
import segment_restated as sr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INCLUDE = os.path.join(ROOT, "include")
HEADER = os.path.join(INCLUDE, "segment", "vcr_hip_segment.h")
EINVAL, EUNSUPPORTED = -1, -3
ENTRY_POINTS = {"vcr_plane_ransac_workspace_bytes", "vcr_plane_ransac_f32", "vcr_plane_ransac_form",
                "vcr_plane_split_workspace_bytes", "vcr_plane_split_f32"}
KERNELS = {"plane_mark_kernel", "plane_offsets_kernel", "plane_gather_kernel", "plane_trial_kernel", "plane_count_trial_kernel",
           "plane_count_point_kernel", "plane_best_kernel", "plane_flags_kernel", "plane_refit_kernel", "plane_invert_kernel"}
COUNT_KERNELS = ("plane_count_trial_kernel", "plane_count_point_kernel")


@pytest.fixture(scope="module")
def lib():
    import vcrnet_amd  # noqa: F401
    from vcrnet_amd import build, segment
    build.build()
    return segment.lib()


# ------------------------------------------------------------------------------------------------------------- the restatement

def edge_clouds():
    """(name, x [3,N], mask or None): the edges the GPU test runs, small enough for the loops."""
    rs = np.random.RandomState(5)
    out = [("N%d" % N, sr.cloud(N), None) for N in (1, 2, 3, 63, 65, 257)]
    x = sr.cloud(130)
    x[rs.randint(0, 3, 20), rs.permutation(130)[:20]] = np.asarray([np.nan, np.inf, -np.inf, np.nan] * 5, np.float32)
    out.append(("nonfinite", x, None))
    out.append(("mask", sr.cloud(200), (rs.uniform(size=200) < 0.6).astype(np.int32)))
    line = np.arange(50, dtype=np.float32) / 64
    out.append(("collinear", np.stack([line, 2 * line, -line]), None))
    out.append(("copies", np.repeat(sr.cloud(6), 12, axis=1), None))
    out.append(("two-candidates", sr.cloud(40), (np.arange(40) % 23 == 4).astype(np.int32)))
    return out


def test_the_two_restated_forms_agree():
    seen = set()
    for name, x, mask in edge_clouds():
        for T, thr in ((70, 0.02), (9, 0.0)):
            a = sr.segment_plane(x, thr, T, 3, mask, trials=sr.trials_loops)
            b = sr.segment_plane(x, thr, T, 3, mask, trials=sr.trials_vector)
            for k in ("M", "status", "picks", "plane", "count", "best_trial", "best_count", "inlier"):
                assert np.array_equal(a[k], b[k]), (name, T, k)
            for k in ("fit", "point"):                    # bits: NaN rows included
                assert np.array_equal(a[k].view(np.int32), b[k].view(np.int32)), (name, T, k)
            assert np.array_equal(a["sums"].view(np.int64), b["sums"].view(np.int64))
            seen |= set(a["status"].tolist())
            if name in ("N1", "N2", "collinear", "two-candidates"):
                assert a["best_trial"] == -1 and np.isnan(a["fit"]).all() and not a["inlier"].any(), name
            if name == "copies":
                assert 2 in a["status"]                     # bitwise copies among the picks: collinear
            if a["best_trial"] >= 0:
                assert a["inlier"].sum() == a["best_count"] == a["count"][a["best_trial"]]
                assert abs(np.linalg.norm(a["fit"][:3].astype(np.float64)) - 1) <= 2.0 ** -22
    assert seen == {0, 1, 2}


def test_the_restatement_alone_recovers_a_planted_plane():
    """60 % of 2 000 points within PLANTED_NOISE thr of a plane, the rest uniform in the box, T = 256: every planted point is an
    inlier of the winner, every other inlier lies within EXTRA_WITHIN thr of the planted plane, and the refitted normal is the
    planted one within segment_restated.angle_bound (all three reasoned there).  Three recipe seeds, none chosen."""
    P = sr.PLANTED
    for seed in (0, 1, 2):
        c = sr.planted(P["N"], P["share"], P["thr"], seed)
        o = sr.segment_plane(c["x"], P["thr"], P["T"], P["seed"])
        inl = o["inlier"] > 0
        dist = np.abs(c["normal"] @ c["x"].astype(np.float64) + c["d"])
        ang = sr.angle(o["fit"][:3], c["normal"])
        print("seed", seed, "best", o["best_trial"], "count", o["best_count"], "extra", int((inl & ~c["on"]).sum()),
              "farthest inlier / thr", dist[inl].max() / P["thr"], "angle", ang)
        assert o["best_trial"] >= 0 and (inl | ~c["on"]).all()
        assert dist[inl].max() <= sr.EXTRA_WITHIN * P["thr"]
        assert ang <= sr.angle_bound(P["thr"])
        q = o["point"].astype(np.float64)
        assert abs(o["fit"][:3].astype(np.float64) @ q + o["fit"][3]) <= 2.0 ** -22       # the point is on the plane


def test_the_refit_sums_follow_the_stated_order():
    """Against an independent statement of the same order in plain loops, on a size that is no multiple of the block."""
    x = sr.cloud(700)
    inl = (np.arange(700) % 3 != 0).astype(np.int32)
    o = x[:, 5]
    got = sr.refit_sums(x, inl, o)
    r = (x - o[:, None]).astype(np.float32).astype(np.float64)
    terms = np.stack([r[0], r[1], r[2], r[0] * r[0], r[0] * r[1], r[0] * r[2], r[1] * r[1], r[1] * r[2], r[2] * r[2]])
    terms = np.concatenate([np.where(inl[None] > 0, terms, 0.0), np.zeros((9, 68))], 1)
    tot = np.zeros(9)
    for blk in range(3):
        waves = []
        for w in range(4):
            v = [terms[:, blk * 256 + w * 64 + l].copy() for l in range(64)]
            for off in (32, 16, 8, 4, 2, 1):
                v = [v[l] + v[l ^ off] for l in range(64)]
            waves.append(v[0])
        tot = tot + (((waves[0] + waves[1]) + waves[2]) + waves[3])
    assert np.array_equal(got.view(np.int64), tot.view(np.int64))


# ---------------------------------------------------------------------------------------------------------------- the boundary

def test_signatures_match_the_header_and_the_library_exports_them(lib):
    from vcrnet_amd import segment
    boundary.check_signatures(HEADER, segment, lib, ENTRY_POINTS)


def test_args_match_the_c_layout(tmp_path):
    import vcrnet_amd  # noqa: F401
    from vcrnet_amd import segment
    assert set(segment.STRUCTS) == {"vcr_plane_ransac_args", "vcr_plane_split_args"}
    boundary.check_layout(HEADER, segment, tmp_path)
    A, S = segment.PlaneRansacArgs, segment.PlaneSplitArgs
    assert A.point.offset == A.count.offset + 8 and S.plane_index.offset == S.rest_count.offset + 8    # the mandatory parts' ends


def test_the_header_lives_in_a_directory_of_its_own_and_enters_the_digests(lib, monkeypatch):
    from vcrnet_amd import build, dbscan, native, outlier, radius, rows, segment
    others = sorted(f for f in os.listdir(INCLUDE) if f.endswith(".h"))
    assert len(others) == 14 and os.listdir(os.path.join(INCLUDE, "ext")) == ["vcr_hip_rows.h"]
    assert os.listdir(os.path.join(INCLUDE, "cluster")) == ["vcr_hip_dbscan.h"]
    assert os.listdir(os.path.join(INCLUDE, "segment")) == ["vcr_hip_segment.h"]
    for h in [os.path.join(INCLUDE, f) for f in others] + build.ROWS_HEADERS + build.DBSCAN_HEADERS:
        assert "vcr_plane_ransac" not in open(h).read() and "vcr_plane_split" not in open(h).read(), h
    assert '#include "../vcr_hip.h"' in open(HEADER).read()
    assert len(native.PUBLIC) == 51 and lib.vcr_abi_version() == native.ABI_VERSION == 27
    for other in (native, outlier, radius, rows, dbscan):
        assert not set(segment.SIGNATURES) & set(other.SIGNATURES) and not set(segment.STRUCTS) & set(other.STRUCTS)
    assert build.SEGMENT_HEADERS == [HEADER]
    assert HEADER not in (build.PUBLIC_HEADERS + build.LATER_HEADERS + build.OUTLIER_HEADERS + build.GICP_HEADERS
                          + build.FPFH_HEADERS + build.MATCH_HEADERS + build.FGR_HEADERS + build.GRID_HEADERS
                          + build.GRIDNN_HEADERS + build.VOXEL_SORT_HEADERS + build.RADIUS_HEADERS + build.ROWS_HEADERS
                          + build.DBSCAN_HEADERS)
    full = build.sources_sha16()
    monkeypatch.setattr(build, "SEGMENT_HEADERS", [])
    assert build.sources_sha16() != full
    monkeypatch.undo()
    text = open(HEADER).read()
    for name, value in (("VCR_PLANE_MAX_N", segment.MAX_N), ("VCR_PLANE_MAX_TRIALS", segment.MAX_TRIALS),
                        ("VCR_PLANE_TRIAL", segment.FORMS["trial"]), ("VCR_PLANE_POINT", segment.FORMS["point"]),
                        ("VCR_PLANE_MAX_SPLITS", segment.MAX_SPLITS), ("VCR_PLANE_POINT_PER_LANE", segment.POINT_PER_LANE),
                        ("VCR_PLANE_POINT_MIN_N", segment.POINT_MIN_N), ("VCR_PLANE_POINT_MIN_T", segment.POINT_MIN_T),
                        ("VCR_PLANE_FILL", segment.FILL),
                        ("VCR_PLANE_TRIAL_MIN_RANGE", segment.TRIAL_MIN_RANGE)):
        assert "#define %s %d " % (name, value) in text or "#define %s %d\n" % (name, value) in text, name


def _args(kind="ransac", **kw):
    from vcrnet_amd import segment
    a = {"ransac": segment.PlaneRansacArgs, "split": segment.PlaneSplitArgs}[kind]()
    for k, f in enumerate(n for n, t in a._fields_ if t is ctypes.c_void_p):       # (never dereferenced; 16-B aligned)
        setattr(a, f, 0x1000 * (k + 1))
    v = dict(B=2, N=1000, distance_threshold=0.05, ransac_n=3, trials=500, seed=1) if kind == "ransac" else dict(B=2, N=1000)
    v.update(kw)
    for k, x in v.items():
        setattr(a, k, x)
    return a


WS = 0x100000                                               # a 256-aligned address that is never dereferenced


def test_the_ransac_call_returns_its_argument_errors_without_a_gpu(lib):
    need = lambda a: lib.vcr_plane_ransac_workspace_bytes(ctypes.byref(a), 0)      # noqa: E731
    f32 = lambda a, ws=WS, n=None: lib.vcr_plane_ransac_f32(ctypes.byref(a), ws, need(_args()) if n is None else n, None)  # noqa: E731
    form = lambda a, cus=256: lib.vcr_plane_ransac_form(ctypes.byref(a), cus, None, None)     # noqa: E731
    assert lib.vcr_plane_ransac_f32(None, WS, 1 << 30, None) == EINVAL and lib.vcr_plane_ransac_workspace_bytes(None, 0) == 0
    for field in ("xyz", "plane", "inlier", "count"):
        assert f32(_args(**{field: None})) == EINVAL and need(_args(**{field: None})) == 0, field
    optional = ("mask", "point", "best_trial", "candidates", "trial_picks", "refit_sums")
    assert need(_args(**{f: None for f in optional})) == need(_args()) > 0
    # the per-trial arrays a caller does not give live in the workspace
    assert need(_args(trial_status=None, trial_plane=None, trial_count=None)) >= need(_args()) + 2 * 500 * 40
    nan, inf = float("nan"), float("inf")
    for kw in (dict(B=0), dict(B=-1), dict(distance_threshold=-0.5), dict(distance_threshold=nan), dict(distance_threshold=inf),
               dict(trials=0), dict(trials=-4), dict(variant=3), dict(variant=-1), dict(variant=0x100), dict(variant=4),
               dict(variant=1 | 513 << 8), dict(trial_plane=0x1008)):
        assert f32(_args(**kw)) == EINVAL and need(_args(**kw)) == 0, kw
        if "trial_plane" not in kw:
            assert form(_args(**kw)) == EINVAL, kw
    for kw in (dict(ransac_n=4), dict(ransac_n=2), dict(N=0), dict(N=-5), dict(N=131073), dict(trials=(1 << 20) + 1),
               dict(B=16384, N=131072), dict(B=1 << 10, trials=1 << 19)):
        assert f32(_args(**kw), n=1 << 40) == EUNSUPPORTED and need(_args(**kw)) == 0 and form(_args(**kw)) == EUNSUPPORTED, kw
    assert need(_args(distance_threshold=0.0)) > 0 and need(_args(B=1, N=131072, trials=1 << 20)) > 0
    assert need(_args(variant=2 | 512 << 8)) == need(_args(variant=1)) == need(_args())       # the workspace is no form's
    size = ctypes.sizeof(type(_args()))
    for wrong in (0, size - 72, size + 8):                  # unsized, short of the mandatory part, longer than known
        a = _args()
        a.struct_bytes = wrong
        assert f32(a) == EINVAL and need(a) == 0 and form(a) == EINVAL, wrong
    a = _args()
    a.struct_bytes = size - 64                              # a caller that knows none of the optional outputs is served
    assert need(a) > need(_args())
    good = need(_args())
    assert good % 256 == 0 and good >= 2 * 1000 * 16
    assert f32(_args(), ws=None) == EINVAL and f32(_args(), ws=WS + 128) == EINVAL and f32(_args(), ws=WS + 16) == EINVAL
    assert f32(_args(), n=good - 1) == EINVAL and f32(_args(), n=0) == EINVAL
    assert lib.vcr_plane_ransac_workspace_bytes(ctypes.byref(_args()), -1) == 0 and form(_args(), -1) == EINVAL
    assert form(_args()) == 0 and lib.vcr_plane_ransac_form(None, 256, None, None) == EINVAL


def test_the_split_call_returns_its_argument_errors_without_a_gpu(lib):
    need = lambda a: lib.vcr_plane_split_workspace_bytes(ctypes.byref(a), 0)       # noqa: E731
    good = need(_args("split"))
    f32 = lambda a, ws=WS, n=good: lib.vcr_plane_split_f32(ctypes.byref(a), ws, n, None)      # noqa: E731
    assert good > 0 and good % 256 == 0 and lib.vcr_plane_split_f32(None, WS, good, None) == EINVAL
    for field in ("xyz", "inlier", "plane_points", "plane_count", "rest_points", "rest_count"):
        assert f32(_args("split", **{field: None})) == EINVAL and need(_args("split", **{field: None})) == 0, field
    assert need(_args("split", plane_index=None, rest_index=None)) == good
    for kw in (dict(B=0), dict(B=-1)):
        assert f32(_args("split", **kw)) == EINVAL and need(_args("split", **kw)) == 0, kw
    for kw in (dict(N=0), dict(N=131073), dict(B=16384, N=131072)):
        assert f32(_args("split", **kw), n=1 << 40) == EUNSUPPORTED and need(_args("split", **kw)) == 0, kw
    size = ctypes.sizeof(type(_args("split")))
    for wrong in (0, size - 24, size + 8):
        a = _args("split")
        a.struct_bytes = wrong
        assert f32(a) == EINVAL, wrong
    a = _args("split")
    a.struct_bytes = size - 16
    assert need(a) == good
    assert f32(_args("split"), ws=None) == EINVAL and f32(_args("split"), ws=WS + 64) == EINVAL
    assert f32(_args("split"), n=good - 1) == EINVAL
    assert lib.vcr_plane_split_workspace_bytes(ctypes.byref(_args("split")), -1) == 0


def test_the_form_is_host_only_and_follows_the_header():
    """POINT with ceil(N / 1024) splits from VCR_PLANE_POINT_MIN_N points a cloud or VCR_PLANE_POINT_MIN_T trials on; below
    both TRIAL, split until the launch has VCR_PLANE_FILL workgroups a CU, no range under VCR_PLANE_TRIAL_MIN_RANGE points;
    variant forces form and splits."""
    from vcrnet_amd import segment
    trial, point = segment.FORMS["trial"], segment.FORMS["point"]

    def want(B, N, T, cus):
        if N >= segment.POINT_MIN_N or T >= segment.POINT_MIN_T:
            return point, -(-N // (256 * segment.POINT_PER_LANE))
        wgs = B * -(-T // 256)
        return trial, min(max(N // segment.TRIAL_MIN_RANGE, 1), -(-segment.FILL * (cus or 256) // wgs), segment.MAX_SPLITS)
    for B, N, T in ((1, 131072, 100), (1, 131072, 1000), (1, 131072, 10000), (16, 16384, 1000), (16, 1024, 100), (16, 1024, 1000),
                    (16, 1024, 10000), (1, 1, 1), (3, 300, 64), (2, 8191, 257), (2, 8192, 257), (1, 5000, 1 << 20), (2, 500, 4095),
                    (2, 500, 4096)):
        for cus in (0, 1, 64, 256, 304):
            assert segment.form(B, N, T, cu_count=cus)[:2] == want(B, N, T, cus), (B, N, T, cus)
        for f in ("trial", "point"):
            assert segment.form(B, N, T, variant=(f, 7))[:2] == (segment.FORMS[f], 7)
            assert segment.form(B, N, T, variant=f)[0] == segment.FORMS[f]
        assert segment.form(B, N, T)[2] == segment.form(B, N, T, variant=("trial", 3))[2] > 0
    # the two shapes the plan is there for: one large cloud fills the chip at any T, sixteen small ones are not cut to shreds
    for T in (100, 1000):
        f, s, _ = segment.form(1, 131072, T)
        assert f == point and s * -(-T // 64) >= 256
    for T in (100, 1000):
        f, s, _ = segment.form(16, 1024, T)
        assert f == trial and 1024 // s >= segment.TRIAL_MIN_RANGE and 16 * -(-T // 256) * s <= 4 * 256 * 4
    with pytest.raises(Exception):
        segment.form(1, 131073, 10)
    with pytest.raises(segment.VcrHipError, match="variant must be 0"):
        segment.form(1, 100, 10, variant=("wave", 1))


def test_the_count_kernels_of_segment_hip_use_no_scratch():
    """hipcc's remarks for segment.hip: its kernel set is the ten below, none with scratch, a spill or AGPRs, all at eight waves
    a SIMD; the tail vcr_plane_split_f32 launches stays outlier.hip's."""
    import vcrnet_amd  # noqa: F401
    from vcrnet_amd import build
    build.build()
    res = build.kernel_resources()
    names = list(res)
    dem = subprocess.run(["c++filt"], input="\n".join(names), capture_output=True, text=True, check=True).stdout.splitlines()
    by_name = {d.replace("(anonymous namespace)::", "").replace("void ", "").split("(")[0]: res[n] for n, d in zip(names, dem)}
    mine = {d: v for d, v in by_name.items() if v["file"] == "segment.hip"}
    assert set(mine) == KERNELS
    for d, v in mine.items():
        print(d, v)
        assert v.get("scratch", 0) == 0 and v.get("vgpr_spill", 0) == 0 and v.get("sgpr_spill", 0) == 0 and v["agprs"] == 0, (d, v)
        assert v["occupancy"] == 8, (d, v)
    for k in COUNT_KERNELS:
        assert mine[k]["vgprs"] <= 40 and mine[k]["lds"] == 0, (k, mine[k])
    for k in ("outlier_mark_kernel", "outlier_offsets_kernel", "outlier_write_kernel"):
        assert by_name[k]["file"] == "outlier.hip", k


# ------------------------------------------------------------------------------------------------------------ the Python layer

def test_python_entry_points_refuse_what_they_cannot_run():
    import vcrnet_amd
    from vcrnet_amd import native, segment
    for name in ("segment_plane", "split_by_plane", "segment_planes"):
        assert getattr(vcrnet_amd, name) is getattr(segment, name) and name in vcrnet_amd.__all__
    assert "segment" not in vcrnet_amd.__all__
    E = native.VcrHipError
    x = torch.zeros(2, 3, 50)
    for bad in (x.transpose(1, 2), torch.zeros(3, 50), None, "xyz"):
        with pytest.raises(E, match=r"xyz must be a \[B, 3, N\]"):
            vcrnet_amd.segment_plane(bad, 0.5)
    with pytest.raises(E, match="segment_plane: a cloud must have 1 ... 131072 points"):
        vcrnet_amd.segment_plane(torch.zeros(1, 3, 131073), 0.5)
    for bad in (-1.0, float("nan"), float("inf"), 1e39, "r", None, True):
        with pytest.raises(E, match="segment_plane: distance_threshold must be finite and >= 0"):
            vcrnet_amd.segment_plane(x, bad)
    for bad in (2, 4, 0, True):
        with pytest.raises(E, match="segment_plane: ransac_n must be 3"):
            vcrnet_amd.segment_plane(x, 0.5, ransac_n=bad)
    for bad in (0, -1, 2.0, "3", True, (1 << 20) + 1):
        with pytest.raises(E, match="segment_plane: num_iterations must be an integer in"):
            vcrnet_amd.segment_plane(x, 0.5, num_iterations=bad)
    with pytest.raises(E, match="below 2\\^29"):
        vcrnet_amd.segment_plane(torch.zeros(1 << 10, 3, 1), 0.5, num_iterations=1 << 19)
    for bad in (-1, 1 << 32, 1.5, True):
        with pytest.raises(E, match="segment_plane: seed must be an integer in"):
            vcrnet_amd.segment_plane(x, 0.5, seed=bad)
    for bad in (torch.zeros(2, 50), torch.zeros(2, 49, dtype=torch.int32), "m"):
        with pytest.raises(E, match=r"mask must be int32 \[B, N\]"):
            vcrnet_amd.segment_plane(x, 0.5, mask=bad)
    with pytest.raises(E, match="variant must be 0"):
        segment.plane_ransac(x, 0.5, variant=("trial", 513))
    m = torch.ones(2, 50, dtype=torch.int32)
    for call in (lambda: vcrnet_amd.segment_plane(x, 0.0), lambda: vcrnet_amd.segment_plane(x, 0.5, 3, 10, 7, m),
                 lambda: segment.plane_ransac(x, 0.5, want_trials=True, variant=("point", 3)),
                 lambda: vcrnet_amd.split_by_plane(x, m), lambda: vcrnet_amd.segment_planes(x, 0.5, 3, 10)):
        with pytest.raises(E, match="no CPU fallback"):      # (the last refusal: everything else was in order)
            call()
    with pytest.raises(E, match=r"inlier must be int32 \[B, N\]"):
        vcrnet_amd.split_by_plane(x, m.long())
    with pytest.raises(E, match=r"xyz must be a \[B, 3, N\]"):
        vcrnet_amd.split_by_plane(m, m)
    for kw in (dict(max_planes=0), dict(max_planes=2.0), dict(min_inliers=-1), dict(min_inliers=True)):
        args = dict(max_planes=2, min_inliers=5)
        args.update(kw)
        with pytest.raises(E, match="segment_planes: (max_planes|min_inliers) must be an integer"):
            vcrnet_amd.segment_planes(x, 0.5, **args)
    with pytest.raises(E, match="segment_planes: seed"):
        vcrnet_amd.segment_planes(x, 0.5, 2, 5, seed=-1)
