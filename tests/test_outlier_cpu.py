"""The outlier filters, without a GPU: the boundary of include/vcr_hip_outlier.h (prototypes against
vcrnet_amd.outlier.SIGNATURES, the structs against gcc's layout, the exported symbols), the argument errors, the form and the
workspaces the plans answer, the new kernels' resource remarks, the two numpy restatements of each definition
(tests/outlier_restated.py) against each other, and the recipes' distance from their thresholds."""
import ctypes
import inspect
import os
import subprocess

import numpy as np
import pytest
import torch

import boundary
import outlier_restated as orr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INCLUDE = os.path.join(ROOT, "include")
HEADER = os.path.join(INCLUDE, "vcr_hip_outlier.h")
EINVAL, EWORKSPACE, EUNSUPPORTED = -1, -2, -3
ENTRY_POINTS = {"vcr_outlier_stat_workspace_bytes", "vcr_outlier_stat_f32", "vcr_outlier_radius_workspace_bytes",
                "vcr_outlier_radius_f32", "vcr_outlier_radius_form"}
KERNELS = {"outlier_dist_kernel", "outlier_mu_kernel", "outlier_dev_kernel", "outlier_sigma_kernel", "outlier_mark_kernel",
           "outlier_offsets_kernel", "outlier_write_kernel", "outlier_count_kernel", "outlier_merge_kernel"}


@pytest.fixture(scope="module")
def lib():
    import vcrnet_amd  # noqa: F401
    from vcrnet_amd import build, outlier
    build.build()
    return outlier.lib()


def test_signatures_match_the_header_and_the_library_exports_them(lib):
    from vcrnet_amd import outlier
    boundary.check_signatures(HEADER, outlier, lib, ENTRY_POINTS)


def test_args_match_the_c_layout(tmp_path):
    import vcrnet_amd  # noqa: F401
    from vcrnet_amd import outlier
    boundary.check_layout(HEADER, outlier, tmp_path)


def test_the_other_boundaries_are_where_they_were(lib, monkeypatch):
    """The feature lives beside the five headers, not in them: none mentions it, ABI 27, the same 51 prototypes; the new header
    is taken into the digests."""
    from vcrnet_amd import build, native, outlier
    for h in ("vcr_hip.h", "vcr_hip_score.h", "vcr_hip_refine.h", "vcr_hip_plane.h", "vcr_hip_voxel.h"):
        assert "vcr_outlier" not in open(os.path.join(INCLUDE, h)).read(), h
    assert len(native.PUBLIC) == 51 and lib.vcr_abi_version() == native.ABI_VERSION == 27
    assert not set(outlier.SIGNATURES) & set(native.SIGNATURES) and not set(outlier.STRUCTS) & set(native.STRUCTS)
    full = build.sources_sha16()
    assert HEADER in build.OUTLIER_HEADERS
    monkeypatch.setattr(build, "OUTLIER_HEADERS", [])
    assert build.sources_sha16() != full


def _stat(B=2, N=1000, k=8, ratio=1.0):
    from vcrnet_amd import outlier
    a = outlier.StatArgs()
    a.xyz4, a.idx, a.points, a.count = 0x1000, 0x2000, 0x3000, 0x4000   # (never dereferenced on the host)
    a.B, a.N, a.k, a.std_ratio = B, N, k, ratio
    return a


def _radius(B=2, N=1000, radius=0.1, nb=4, variant=0):
    from vcrnet_amd import outlier
    a = outlier.RadiusArgs()
    a.xyz, a.points, a.count = 0x1000, 0x2000, 0x3000
    a.B, a.N, a.radius, a.nb_points, a.variant = B, N, radius, nb, variant
    return a


def test_statistical_argument_errors_return_their_codes_without_a_gpu(lib):
    from vcrnet_amd import outlier
    f32 = lambda a, ws=0x10000, n=1 << 40: lib.vcr_outlier_stat_f32(ctypes.byref(a), ws, n, None)       # noqa: E731
    size = lambda a: lib.vcr_outlier_stat_workspace_bytes(ctypes.byref(a), 256)                          # noqa: E731
    assert lib.vcr_outlier_stat_f32(None, 0x10000, 1 << 40, None) == EINVAL
    assert lib.vcr_outlier_stat_workspace_bytes(None, 256) == 0
    assert size(_stat()) > 0 and lib.vcr_outlier_stat_workspace_bytes(ctypes.byref(_stat()), -1) == 0
    for field in ("xyz4", "idx", "points", "count"):
        a = _stat()
        setattr(a, field, None)
        assert f32(a) == EINVAL and size(a) == 0, field
    a = _stat()
    a.xyz4 = 0x1008                                         # rows are read 16 bytes at a time
    assert f32(a) == EINVAL and size(a) == 0
    a = _stat()
    a.index, a.mean_dist, a.valid, a.stats = 0x5000, 0x6000, 0x7000, 0x8000       # the optional outputs change nothing here
    assert size(a) == size(_stat())
    for kw in (dict(B=0), dict(B=-2), dict(k=0), dict(k=-1), dict(ratio=-0.5), dict(ratio=float("nan")),
               dict(ratio=float("inf")), dict(ratio=-float("inf"))):
        assert f32(_stat(**kw)) == EINVAL and size(_stat(**kw)) == 0, kw
    assert size(_stat(ratio=0.0)) > 0 and size(_stat(k=62)) > 0 and size(_stat(k=1, N=1)) > 0
    for kw in (dict(k=63), dict(N=0), dict(N=-4), dict(N=131073), dict(N=131072, B=16384)):
        assert f32(_stat(**kw)) == EUNSUPPORTED and size(_stat(**kw)) == 0, kw
    assert size(_stat(N=131072, B=16383)) > 0
    for bad in (0, outlier.StatArgs.index.offset - 4, ctypes.sizeof(outlier.StatArgs) + 8):
        a = _stat()
        a.struct_bytes = bad
        assert f32(a) == EINVAL and size(a) == 0, bad
    a = _stat()
    a.struct_bytes = outlier.StatArgs.index.offset          # the mandatory part alone is served
    assert size(a) == size(_stat())
    need = size(_stat())
    a = _stat()
    assert f32(a, ws=None) == EINVAL and f32(a, ws=0x10004) == EINVAL and f32(a, ws=0x10008) == EINVAL
    assert f32(a, n=need - 1) == EWORKSPACE and f32(a, n=0) == EWORKSPACE


def test_radius_argument_errors_return_their_codes_without_a_gpu(lib):
    from vcrnet_amd import outlier
    f32 = lambda a, ws=0x10000, n=1 << 40: lib.vcr_outlier_radius_f32(ctypes.byref(a), ws, n, None)     # noqa: E731
    form = lambda a: lib.vcr_outlier_radius_form(ctypes.byref(a), 256, None, None)                      # noqa: E731
    size = lambda a: lib.vcr_outlier_radius_workspace_bytes(ctypes.byref(a), 256)                       # noqa: E731
    assert lib.vcr_outlier_radius_f32(None, 0x10000, 1 << 40, None) == EINVAL
    assert lib.vcr_outlier_radius_form(None, 256, None, None) == EINVAL and lib.vcr_outlier_radius_workspace_bytes(None, 256) == 0
    assert form(_radius()) == 0 and size(_radius()) > 0
    for field in ("xyz", "points", "count"):
        a = _radius()
        setattr(a, field, None)
        assert f32(a) == EINVAL and form(a) == EINVAL and size(a) == 0, field
    a = _radius()
    a.index, a.neighbours = 0x4000, 0x5000                  # the optional outputs change nothing here
    assert form(a) == 0 and size(a) == size(_radius())
    for kw in (dict(B=0), dict(B=-2), dict(radius=0.0), dict(radius=-0.5), dict(radius=float("nan")), dict(radius=float("inf")),
               dict(radius=-float("inf")), dict(nb=-1), dict(variant=2), dict(variant=4), dict(variant=-1),
               dict(variant=outlier.variant(129)), dict(variant=1 << 16), dict(variant=1 << 4)):
        assert f32(_radius(**kw)) == EINVAL and form(_radius(**kw)) == EINVAL and size(_radius(**kw)) == 0, kw
    assert form(_radius(radius=1e-45)) == 0 and form(_radius(nb=0)) == 0 and form(_radius(nb=2 ** 31 - 1)) == 0
    assert form(_radius(variant=1)) == 0 and form(_radius(variant=1 | outlier.variant(128))) == 0
    for kw in (dict(N=0), dict(N=-4), dict(N=131073), dict(N=131072, B=16384)):
        assert f32(_radius(**kw)) == EUNSUPPORTED and form(_radius(**kw)) == EUNSUPPORTED and size(_radius(**kw)) == 0, kw
    assert form(_radius(N=131072, B=16383)) == 0
    assert lib.vcr_outlier_radius_form(ctypes.byref(_radius()), -1, None, None) == EINVAL
    for bad in (0, outlier.RadiusArgs.index.offset - 4, ctypes.sizeof(outlier.RadiusArgs) + 8):
        a = _radius()
        a.struct_bytes = bad
        assert f32(a) == EINVAL and form(a) == EINVAL and size(a) == 0, bad
    a = _radius(variant=outlier.variant(2))
    q, s = ctypes.c_int(0), ctypes.c_int(0)
    assert lib.vcr_outlier_radius_form(ctypes.byref(a), 256, ctypes.byref(q), ctypes.byref(s)) == 0 and (q.value, s.value) == (1, 2)
    a.struct_bytes = outlier.RadiusArgs.index.offset        # the mandatory part alone: its variant reads as 0
    assert lib.vcr_outlier_radius_form(ctypes.byref(a), 256, ctypes.byref(q), ctypes.byref(s)) == 0 and (q.value, s.value) == (1, 3)
    a = _radius()
    need = lib.vcr_outlier_radius_workspace_bytes(ctypes.byref(a), 0)
    assert need == size(a) > 0
    assert f32(a, ws=None) == EINVAL and f32(a, ws=0x10004) == EINVAL and f32(a, ws=0x10008) == EINVAL
    assert f32(a, n=need - 1) == EWORKSPACE and f32(a, n=0) == EWORKSPACE


def up(v):
    return (v + 255) // 256 * 256


def test_the_form_is_the_score_plans_and_the_workspaces_the_headers(lib):
    from vcrnet_amd import outlier, score
    shapes = [(1, 1), (1, 5), (1, 257), (16, 1024), (16, 16384), (1, 70001), (1, 131072), (64, 16384), (256, 16384), (3, 700)]
    for B, N in shapes:
        nblk = (N + 255) // 256
        for cu in (256, 1, 304):
            for force in (0, 1, 2, 3, 8, 9, 128):
                q, s, ws = outlier.radius_form(B, N, cu_count=cu, variant=outlier.variant(force))
                assert (q, s) == (1, score.nn_score_form(B, N, N, cu_count=cu, variant=score.variant(0, force))[1]), (B, N, cu, force)
                assert force == 0 or s == force
                assert ws == up(4 * s * B * N) + up(4 * B * N) + up(4 * B * nblk), (B, N, cu, force)
        for k in (1, 20, 62):                               # the statistical filter's: no k, no device in it
            assert lib.vcr_outlier_stat_workspace_bytes(ctypes.byref(_stat(B, N, k)), 0) == \
                up(4 * B * N) + up(40 * B) + 2 * up(8 * B * nblk) + 2 * up(4 * B * nblk), (B, N, k)
    assert outlier.radius_form(1, 131072)[1] == 32 and outlier.radius_form(256, 16384)[1] == 1
    assert outlier.radius_form(1, 2049, variant=1)[:2] == outlier.radius_form(1, 2049)[:2]    # "one point per lane" is the form
    for B, N in ((1, 0), (1, 131073), (16384, 131072)):
        with pytest.raises(Exception):
            outlier.radius_form(B, N)


def test_the_new_kernels_use_no_scratch_and_keep_eight_waves():
    import vcrnet_amd  # noqa: F401
    from vcrnet_amd import build
    build.build()
    res = build.kernel_resources()
    names = list(res)
    dem = subprocess.run(["c++filt"], input="\n".join(names), capture_output=True, text=True, check=True).stdout.splitlines()
    mine = {d.replace("(anonymous namespace)::", ""): res[n] for n, d in zip(names, dem) if res[n]["file"] == "outlier.hip"}
    assert {d.split("(")[0] for d in mine} == KERNELS
    for d, v in mine.items():
        assert v.get("scratch", 0) == 0 and v.get("vgpr_spill", 0) == 0 and v.get("sgpr_spill", 0) == 0, (d, v)
        assert v["occupancy"] >= 8 and v["vgprs"] <= 64, (d, v)                  # 256 lanes: eight workgroups a CU
    count = [v for d, v in mine.items() if d.startswith("outlier_count_kernel")][0]
    assert count["lds"] == 3 * 4 * 1024, count                                   # nn_scan_kernel's three planes of 1024 points
    assert max(v["lds"] for d, v in mine.items() if not d.startswith("outlier_count_kernel")) <= 3 * 1024


# ---------------------------------------------------------------- the restatements

SMALL = 300                                                # the largest cloud the plain double loops walk whole


@pytest.fixture(scope="module")
def radius_cases():
    """name -> (xyz, radius, nb_points, the vectorised result; None for the LARGE ones), computed once."""
    out = {}
    for name, make in orr.RADIUS_RECIPES.items():
        xyz, r, nb = make()
        out[name] = (xyz, r, nb, None if name in orr.LARGE else orr.batch(orr.radius_fast, xyz, r, nb))
    return out


@pytest.fixture(scope="module")
def stat_cases():
    """name -> (xyz, the reference neighbours, k, std_ratio, the vectorised result), computed once."""
    out = {}
    for name, make in orr.STAT_RECIPES.items():
        xyz, k, ratio = make()
        idx = np.stack([orr.neighbours(c, k) for c in xyz])
        out[name] = (xyz, idx, k, ratio, orr.batch(orr.stat, xyz, idx, ratio))
    return out


def _same(a, b, keys):
    return all(np.array_equal(orr.bits(a[k]), orr.bits(b[k])) for k in keys)


def test_the_two_radius_restatements_agree_bit_for_bit(radius_cases):
    for name, (xyz, r, nb, fast) in radius_cases.items():
        N = xyz.shape[2]
        if N <= SMALL:
            assert _same(orr.batch(orr.radius_loop, xyz, r, nb), fast, ("neighbours", "points", "count", "index")), name
            continue
        rows = orr.rows_of(name, N, 14 if name in orr.LARGE else 24)             # a larger cloud: some rows of it
        for b, cloud in enumerate(xyz):
            want = orr.radius_counts_loop(cloud, r, rows)
            got = orr.radius_counts(cloud, r, rows) if fast is None else fast["neighbours"][b][rows]
            assert np.array_equal(want, got), (name, b)


def test_the_two_statistical_restatements_agree_bit_for_bit(stat_cases):
    for name, (xyz, idx, k, ratio, fast) in stat_cases.items():
        N = xyz.shape[2]
        if N * k <= 1100 * 20:
            assert _same(orr.batch(orr.stat_loop, xyz, idx, ratio), fast,
                         ("mean_dist", "valid", "stats", "var", "keep", "points", "count", "index")), name
            continue
        rows = orr.rows_of(name, N, 64)
        assert np.array_equal(orr.bits(orr.mean_dist_loop(xyz[0], idx[0], rows)), orr.bits(fast["mean_dist"][0][rows])), name
        slow = orr.decide(fast["mean_dist"][0], ratio, orr._ordered_loop)
        assert [orr.bits(slow[q]) for q in ("mu", "var", "sigma", "thr")] == \
            [orr.bits(v) for v in (fast["stats"][0, 0], fast["var"][0], fast["stats"][0, 1], fast["stats"][0, 2])], name


def test_the_outputs_have_the_shape_the_header_gives_them(radius_cases, stat_cases):
    for name, case in list(radius_cases.items()) + list(stat_cases.items()):
        xyz, r = case[0], case[-1]
        if r is None:
            continue
        for b, cloud in enumerate(xyz):
            M, index, points = int(r["count"][b]), r["index"][b], r["points"][b]
            assert (np.diff(index[:M]) > 0).all() and (index[M:] == -1).all(), name
            assert np.array_equal(orr.bits(points[:, :M]), orr.bits(cloud[:, index[:M]])), name
            assert (orr.bits(points[:, M:]) == orr.NAN_BITS).all() and np.isfinite(points[:, :M]).all(), name


def test_the_recipes_meet_the_edges_they_are_named_for(radius_cases, stat_cases):
    r = radius_cases
    assert r["n1_nb0"][3]["count"][0] == 1 and r["n1_nb1"][3]["count"][0] == 0 and r["n1_nb0"][3]["neighbours"][0, 0] == 1
    assert r["all_kept"][3]["count"][0] == 600 and r["none_kept"][3]["count"][0] == 0
    assert (r["none_kept"][3]["neighbours"] == 600).all()
    for cases, name, seed in ((r, "blob_far", 12), (stat_cases, "blob_far", 31)):
        far = orr.blob_far(seed, 2000)[1]
        res = cases[name][-1]
        assert len(far) == 100 and np.array_equal(res["index"][0, :1900], np.setdiff1d(np.arange(2000), far)), name
    assert (r["copies"][3]["neighbours"] == 2).all() and r["copies"][3]["count"][0] == 900
    xyz, rad, nb, res = r["lattice"]
    steps = np.abs(xyz[0][:, :, None] - xyz[0][:, None, :]).sum(axis=0) * 64.0   # lattice steps between two points, exact
    assert np.array_equal(res["neighbours"][0], (steps <= 1.0).sum(axis=1))      # itself and the neighbours ON the sphere
    assert (res["neighbours"][0] > 1).mean() > 0.9 and 0 < res["count"][0] < 150
    for cases, cut in ((r, 3), (stat_cases, 4)):
        xyz, res = cases["non_finite"][0], cases["non_finite"][-1]
        N = xyz.shape[2]
        kept = res["index"][0, :res["count"][0]]
        assert 0 not in kept and N // 2 not in kept
    nf, far = r["non_finite"][3], r["far_instead"][3]
    assert (nf["neighbours"][0, [0, 450]] == 0).all() and (far["neighbours"][0, [0, 450]] == 1).all()
    rest = np.setdiff1d(np.arange(900), [0, 450])
    assert np.array_equal(nf["neighbours"][0, rest], far["neighbours"][0, rest])
    assert _same(nf, far, ("count", "index")) and np.array_equal(orr.bits(nf["points"]), orr.bits(far["points"]))
    s = stat_cases
    assert s["non_finite"][4]["valid"][0] == 898 and not np.isfinite(s["non_finite"][4]["mean_dist"][0, [0, 450]]).any()
    assert s["all_kept"][4]["count"][0] == 600
    res = s["copies"][4]
    zero = res["mean_dist"][0] == 0.0
    assert zero.sum() == 600 and res["keep"][0][zero].all() and res["stats"][0, 2] > 0.0      # a mean distance of 0 is kept
    res = s["n2_k1"][4]
    assert res["count"][0] == 2 and res["stats"][0, 1] == 0.0 and res["stats"][0, 0] == res["stats"][0, 2] == res["mean_dist"][0, 0]
    assert list(s["three_clouds"][4]["valid"]) == [700, 700, 698]


def test_no_statistical_recipe_has_a_point_near_its_threshold(stat_cases):
    """The runs from coordinates alone compare the kept SET: the device's neighbours and its fp64 square root may move a mean
    distance by an fp32 ulp (2^-23 relative), so no valid point may lie within 2^-20 thr of thr."""
    for name, (xyz, idx, k, ratio, res) in stat_cases.items():
        for b in range(xyz.shape[0]):
            band = orr.stat_band(res["mean_dist"][b], res["stats"][b, 2])
            if name in orr.EQUAL:
                assert band == 0.0 and len(set(orr.bits(res["mean_dist"][b]).tolist())) == 1, name
            else:
                assert band > orr.BAND, (name, b, band)


def test_no_radius_recipe_has_a_pair_near_its_sphere(radius_cases):
    """Where the fp64 distance of a pair lies further than 2^-20 r^2 from r^2, the fp32 chain (three roundings, 2^-22 relative
    at most) decides as the exact distance does.  The lattice is excepted by construction (its pairs ON the sphere are exact);
    of the two large clouds the rows the GPU test compares are held to it (all pairs of 131 072 points cannot be: a shell that
    thin still holds a few of 8.6e9 pairs)."""
    for name, (xyz, r, nb, _) in radius_cases.items():
        if name in orr.LATTICE:
            continue
        rows = orr.rows_of(name, xyz.shape[2]) if name in orr.LARGE else None
        for b, cloud in enumerate(xyz):
            assert orr.radius_band(cloud, r, rows) > orr.BAND, (name, b)


# ---------------------------------------------------------------- the Python layer

def test_python_entry_points_refuse_what_they_cannot_run():
    import vcrnet_amd
    from vcrnet_amd import module, native, outlier
    assert vcrnet_amd.remove_statistical_outlier is outlier.remove_statistical_outlier
    assert vcrnet_amd.remove_radius_outlier is outlier.remove_radius_outlier
    assert {"remove_statistical_outlier", "remove_radius_outlier"} <= set(vcrnet_amd.__all__)
    a = torch.zeros(2, 3, 300)
    for call in (lambda x: vcrnet_amd.remove_statistical_outlier(x), lambda x: vcrnet_amd.remove_radius_outlier(x, 4, 0.1)):
        with pytest.raises(native.VcrHipError, match="no CPU fallback"):
            call(a)
        with pytest.raises(native.VcrHipError, match=r"xyz must be a \[B, 3, N\]"):
            call(a.transpose(1, 2))
        with pytest.raises(native.VcrHipError, match=r"\[B, 3, N\]"):
            call(torch.zeros(3, 300))
    with pytest.raises(native.VcrHipError, match="no CPU fallback"):
        outlier.stat_filter(torch.zeros(2, 300, 4), torch.zeros(2, 300, 8, dtype=torch.int32), 1.0)
    with pytest.raises(native.VcrHipError, match="xyz4 must be float32"):
        outlier.stat_filter(torch.zeros(2, 300, 3), torch.zeros(2, 300, 8, dtype=torch.int32), 1.0)
    with pytest.raises(native.VcrHipError, match="idx must be int32"):
        outlier.stat_filter(torch.zeros(2, 300, 4), torch.zeros(2, 300, 8, dtype=torch.int64), 1.0)
    params = list(inspect.signature(module.register_sampled).parameters)
    assert params[-1] == "outlier" and inspect.signature(module.register_sampled).parameters["outlier"].default is None
    with pytest.raises(native.VcrHipError, match="outlier must be"):
        outlier.filter_by(("median", 3, 1.0), a)
