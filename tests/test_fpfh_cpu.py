"""The FPFH features, without a GPU: the boundary of include/vcr_hip_fpfh.h (prototypes against vcrnet_amd.fpfh.SIGNATURES, the
structs against gcc's layout, the exported symbols), every argument error of both calls, the resource remarks of the two kernels,
the numpy restatement (tests/fpfh_restated.py) on the recipes the GPU tests use -- its invariants, an exact plane, and the cap
on the pairs whose f0 bin the last bit of an arc tangent could move -- and the refusals of the public function."""
import ctypes
import os
import subprocess

import numpy as np
import pytest
import torch

import boundary
import fpfh_restated as fr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INCLUDE = os.path.join(ROOT, "include")
HEADER = os.path.join(INCLUDE, "vcr_hip_fpfh.h")
OTHERS = ("vcr_hip.h", "vcr_hip_score.h", "vcr_hip_refine.h", "vcr_hip_plane.h", "vcr_hip_voxel.h", "vcr_hip_outlier.h",
          "vcr_hip_gicp.h")
EINVAL, EUNSUPPORTED = -1, -3
ENTRY_POINTS = {"vcr_spfh_f32", "vcr_fpfh_f32"}
KERNELS = {"spfh_kernel", "fpfh_kernel"}
EXCLUDED_CAP = 0.001                                        # of a case's counted pairs


@pytest.fixture(scope="module")
def lib():
    import vcrnet_amd  # noqa: F401
    from vcrnet_amd import build, fpfh
    build.build()
    return fpfh.lib()


def test_signatures_match_the_header_and_the_library_exports_them(lib):
    from vcrnet_amd import fpfh
    boundary.check_signatures(HEADER, fpfh, lib, ENTRY_POINTS)


def test_args_match_the_c_layout(tmp_path):
    import vcrnet_amd  # noqa: F401
    from vcrnet_amd import fpfh
    boundary.check_layout(HEADER, fpfh, tmp_path)


def test_the_other_boundaries_are_where_they_were(lib, monkeypatch):
    """The feature lives beside the seven headers, not in them: none mentions it, ABI 27, the same 51 prototypes; the new
    header is taken into the digests through a list of its own."""
    from vcrnet_amd import build, fpfh, gicp, native, outlier, plane, refine, score, voxel
    for h in OTHERS:
        text = open(os.path.join(INCLUDE, h)).read()
        assert "vcr_spfh" not in text and "vcr_fpfh" not in text, h
    assert len(native.PUBLIC) == 51 and lib.vcr_abi_version() == native.ABI_VERSION == 27
    for other in (native, score, refine, plane, voxel, outlier, gicp):
        assert not set(fpfh.SIGNATURES) & set(other.SIGNATURES) and not set(fpfh.STRUCTS) & set(other.STRUCTS)
    assert build.FPFH_HEADERS == [HEADER]
    assert HEADER not in build.PUBLIC_HEADERS + build.LATER_HEADERS + build.OUTLIER_HEADERS + build.GICP_HEADERS
    full = build.sources_sha16()
    monkeypatch.setattr(build, "FPFH_HEADERS", [])
    assert build.sources_sha16() != full
    monkeypatch.undo()
    text = open(HEADER).read()
    for name, value in (("VCR_FPFH_MAX_K", fpfh.MAX_K), ("VCR_FPFH_BINS", fpfh.BINS), ("VCR_SPFH_ROW_BYTES", fpfh.ROW_BYTES)):
        assert "#define %s %d " % (name, value) in text, name
    assert (fpfh.MAX_K, fpfh.BINS, fpfh.ROW_BYTES) == (plane.MAX_K, fr.BINS, fr.ROW) == (62, 11, 48)


def _spfh(B=2, N=100, k=20, radius=0.0):
    from vcrnet_amd import fpfh
    a = fpfh.SpfhArgs()
    a.xyz4, a.normals, a.idx, a.spfh = 0x1000, 0x2000, 0x3000, 0x4000           # (never dereferenced: every call is refused)
    a.B, a.N, a.k, a.radius = B, N, k, radius
    return a


def _fpfh(B=2, N=100, k=20, radius=0.0):
    from vcrnet_amd import fpfh
    a = fpfh.FpfhArgs()
    a.xyz4, a.idx, a.spfh, a.fpfh = 0x1000, 0x3000, 0x4000, 0x5000
    a.B, a.N, a.k, a.radius = B, N, k, radius
    return a


@pytest.mark.parametrize("entry,make,pointers", [("vcr_spfh_f32", _spfh, ("xyz4", "normals", "idx", "spfh")),
                                                 ("vcr_fpfh_f32", _fpfh, ("xyz4", "idx", "spfh", "fpfh"))])
def test_argument_errors_return_their_codes_without_a_gpu(lib, entry, make, pointers):
    fn = getattr(lib, entry)
    f32 = lambda a: fn(ctypes.byref(a), None)                                   # noqa: E731
    assert fn(None, None) == EINVAL
    for field in pointers:
        a = make()
        setattr(a, field, None)
        assert f32(a) == EINVAL, field
    for field in ("xyz4", "spfh"):                          # rows and histogram groups are read and written 16 B at a time
        a = make()
        setattr(a, field, getattr(a, field) + 8)
        assert f32(a) == EINVAL, field
    nan, inf = float("nan"), float("inf")
    for kw in (dict(k=0), dict(k=-1), dict(B=0), dict(N=0), dict(B=-2), dict(N=-5), dict(radius=-0.5), dict(radius=nan),
               dict(radius=inf), dict(radius=-inf)):
        assert f32(make(**kw)) == EINVAL, kw
    for kw in (dict(k=63), dict(N=131073), dict(B=16384, N=131072)):
        assert f32(make(**kw)) == EUNSUPPORTED, kw
    size = ctypes.sizeof(type(make()))
    for bad in (0, size - 8, size + 8):                     # unsized, short of the last (mandatory) pointer, longer than known
        a = make()
        a.struct_bytes = bad
        assert f32(a) == EINVAL, bad
    assert make().struct_bytes == size and getattr(type(make()), pointers[-1]).offset == size - 8


def test_the_new_kernels_use_no_scratch_and_keep_their_occupancy():
    import vcrnet_amd  # noqa: F401
    from vcrnet_amd import build
    build.build()
    res = build.kernel_resources()
    names = list(res)
    dem = subprocess.run(["c++filt"], input="\n".join(names), capture_output=True, text=True, check=True).stdout.splitlines()
    mine = {d.replace("(anonymous namespace)::", "").split("(")[0]: res[n] for n, d in zip(names, dem) if res[n]["file"] == "fpfh.hip"}
    assert set(mine) == KERNELS
    for d, v in mine.items():
        assert v.get("scratch", 0) == 0 and v.get("vgpr_spill", 0) == 0 and v.get("sgpr_spill", 0) == 0 and v["lds"] == 0, (d, v)
    # waves per SIMD, as DESIGN section 4.14 records them: the pair feature's fp64 chain and atan2 take 120 registers, the
    # second pass's eleven accumulators stay inside 64
    assert mine["spfh_kernel"]["occupancy"] == 4 and mine["spfh_kernel"]["vgprs"] + mine["spfh_kernel"].get("agprs", 0) <= 128
    assert mine["fpfh_kernel"]["occupancy"] == 8 and mine["fpfh_kernel"]["vgprs"] + mine["fpfh_kernel"].get("agprs", 0) <= 64


# ------------------------------------------------------------------------------------------------------------- the restatement

@pytest.fixture(scope="module")
def cases():
    """(B, N, k) -> per cloud (x, idx, normals, pairs, spfh bytes, fpfh), computed once."""
    out = {}
    for B, N, k in fr.SHAPES:
        x = fr.cloud(B, N)
        per = []
        for b in range(B):
            idx = fr.neighbours(x[b], k)
            nrm = fr.normals(x[b], idx)
            p = fr.pairs(x[b], nrm, idx)
            sp = fr.pack(p)
            per.append((x[b], idx, nrm, p, sp, fr.fpfh(x[b], idx, sp)))
        out[(B, N, k)] = per
    return out


def test_the_restated_histograms_keep_their_sums(cases):
    """Each group of every SPFH row sums to c_i = k, no count exceeds k, and every FPFH row sums to 600 within 1e-9 in front of
    its conversion to fp32: per group 100 from the neighbours and 100 of its own."""
    for (B, N, k), per in cases.items():
        for x, idx, nrm, p, sp, feat in per:
            assert idx.shape == (N, k) and not (idx == np.arange(N)[:, None]).any()
            counts, c = fr.group_bins(sp)
            assert (c == k).all() and p["counted"].all()
            assert (counts.reshape(N, 3, 11).sum(2) == k).all()
            assert counts.max() <= k
            assert feat.shape == (33, N) and feat.dtype == np.float32 and np.isfinite(feat).all() and feat.min() >= 0
            wide = fr.fpfh(x, idx, sp, rounded=False)
            assert np.array_equal(wide.astype(np.float32), feat)
            assert np.abs(wide.sum(0) - 600).max() <= 1e-9, (B, N, k)


def test_an_exact_plane_has_one_bin_a_group():
    x, nrm = fr.plane_cloud()
    idx = fr.neighbours(x, 10)
    p = fr.pairs(x, nrm, idx)
    assert p["counted"].all() and (p["bins"] == 5).all() and np.abs(p["coord"] - 5.5).max() <= 2.0 ** -50 and not fr.excluded(p).any()
    sp = fr.pack(p)
    counts, c = fr.group_bins(sp)
    want = np.zeros(33, np.int64)
    want[[5, 16, 27]] = 10
    assert (counts == want).all() and (c == 10).all()
    feat = fr.fpfh(x, idx, sp)
    assert np.array_equal(feat, np.tile(np.where(want > 0, np.float32(200), np.float32(0))[:, None], (1, 200)))


def test_at_most_a_thousandth_of_a_recipes_pairs_is_excluded(cases):
    """The one step numpy and the device need not reproduce bit for bit is atan2: a pair is excluded iff its f0 coordinate lies
    within 2^-30 of an integer -- an fp64 atan2 is good to a few ulp, about 1e-15 on that coordinate.  Ties |a1| == |a2| and f1 /
    f2 coordinates near an integer are plain IEEE arithmetic and exclude nothing."""
    for (B, N, k), per in cases.items():
        n = e = ties = 0
        for x, idx, nrm, p, sp, feat in per:
            n += int(p["counted"].sum())
            e += int(fr.excluded(p).sum())
            ties += int(p["tie"].sum())
        print(f"fpfh recipe B {B} N {N} k {k}: {e} of {n} pairs excluded, {ties} with |a1| == |a2|")
        assert n == B * N * k and e <= EXCLUDED_CAP * n, (B, N, k, e, n)


def test_a_radius_drops_the_same_pairs_in_both_passes():
    B, N, k = fr.SHAPES[1]
    x = fr.cloud(B, N)[0]
    idx = fr.neighbours(x, k)
    nrm = fr.normals(x, idx)
    d = np.sqrt(fr.geometry(x, idx)[2])
    radius = fr.radius_between(d, 5)
    inside = fr.geometry(x, idx)[2] <= fr.r2_of(radius)
    assert 0 < inside.sum() < inside.size
    p = fr.pairs(x, nrm, idx, radius)
    assert np.array_equal(p["counted"], inside)
    sp = fr.pack(p)
    assert np.array_equal(fr.group_bins(sp)[1], inside.sum(1))
    # the second pass skips them too: moving a dropped neighbour's histogram changes nothing
    feat = fr.fpfh(x, idx, sp, radius)
    masked = np.where(inside, idx, -1)                       # (an entry outside [0, N) reads as the row itself: d2 = 0, skipped)
    assert np.array_equal(feat, fr.fpfh(x, masked, sp, radius))
    huge = fr.pairs(x, nrm, idx, 10.0)
    assert huge["counted"].all() and np.array_equal(fr.pack(huge), fr.spfh(x, nrm, idx))


def test_non_finite_rows_are_not_counted():
    x = fr.cloud(1, 64)[0]
    idx = fr.neighbours(x, 8)
    nrm = fr.normals(x, idx)
    bad_x, bad_n = x.copy(), nrm.copy()
    bad_x[1, 7] = np.nan
    bad_x[2, 30] = np.inf
    bad_n[0, 50] = np.nan
    p = fr.pairs(bad_x, bad_n, idx)
    hit = np.isin(idx, [7, 30, 50])
    hit[[7, 30, 50]] = True
    assert np.array_equal(p["counted"], ~hit)
    sp = fr.pack(p)
    feat = fr.fpfh(bad_x, idx, sp)
    assert (fr.group_bins(sp)[1][[7, 30, 50]] == 0).all()
    # a point without a finite position has no distance to weigh by; one without a normal still gathers its neighbours'
    assert np.isfinite(feat).all() and (feat[:, [7, 30]] == 0).all() and feat[:, 50].any()


# ------------------------------------------------------------------------------------------------------------ the Python layer

def test_python_entry_points_refuse_what_they_cannot_run():
    import vcrnet_amd
    from vcrnet_amd import fpfh, native
    assert vcrnet_amd.compute_fpfh_feature is fpfh.compute_fpfh_feature and "compute_fpfh_feature" in vcrnet_amd.__all__
    assert "Centre such a cloud first" in fpfh.compute_fpfh_feature.__doc__
    a = torch.zeros(2, 3, 300)
    with pytest.raises(native.VcrHipError, match="no CPU fallback"):
        vcrnet_amd.compute_fpfh_feature(a)
    with pytest.raises(native.VcrHipError, match="no CPU fallback"):
        vcrnet_amd.compute_fpfh_feature(a, normals=a, k=20, radius=0.1)
    with pytest.raises(native.VcrHipError, match=r"xyz must be a \[B, 3, N\]"):
        vcrnet_amd.compute_fpfh_feature(a.transpose(1, 2))
    with pytest.raises(native.VcrHipError, match=r"\[B, 3, N\]"):
        vcrnet_amd.compute_fpfh_feature(torch.zeros(3, 300))
    for k in (0, -1, 63):
        with pytest.raises(native.VcrHipError, match=r"k must be in \[1, 62\]"):
            vcrnet_amd.compute_fpfh_feature(a, k=k)
    with pytest.raises(native.VcrHipError, match=r"k \+ 1 = 31 neighbours"):
        vcrnet_amd.compute_fpfh_feature(a[:, :, :30])
    for bad in (torch.zeros(2, 3, 299), torch.zeros(2, 300, 3), torch.zeros(1, 3, 300), "normals"):
        with pytest.raises(native.VcrHipError, match=r"normals must be \[B, 3, N\]"):
            vcrnet_amd.compute_fpfh_feature(a, normals=bad)
    for bad in (0.0, -0.1, float("nan"), float("inf")):
        with pytest.raises(native.VcrHipError, match="radius must be positive and finite"):
            vcrnet_amd.compute_fpfh_feature(a, radius=bad)
    rows, idx = torch.zeros(2, 300, 4), torch.zeros(2, 300, 8, dtype=torch.int32)
    with pytest.raises(native.VcrHipError, match="xyz4 must be float32"):
        fpfh.spfh(torch.zeros(2, 300, 3), a, idx)
    with pytest.raises(native.VcrHipError, match="idx must be int32"):
        fpfh.spfh(rows, a, idx.long())
    with pytest.raises(native.VcrHipError, match="normals must be float32"):
        fpfh.spfh(rows, a[:, :, :299], idx)
    with pytest.raises(native.VcrHipError, match="spfh must be uint8"):
        fpfh.fpfh(rows, idx, torch.zeros(2, 300, 33, dtype=torch.uint8))
    with pytest.raises(native.VcrHipError, match="no CPU fallback"):
        fpfh.spfh(rows, a, idx)
    with pytest.raises(native.VcrHipError, match="no CPU fallback"):
        fpfh.fpfh(rows, idx, torch.zeros(2, 300, 48, dtype=torch.uint8))
