"""Moving least squares without a GPU (include/smooth/vcr_hip_mls.h): the restatement
(tests/mls_restated.py) against facts that are not its own, the smoothing condition on the noisy sphere, the header against the
ctypes binding and the library's exports, the place of the header among the others and in the digests, the argument errors of the C
entry points and of the Python layer, and the resource remarks of mls.hip."""
import ctypes
import functools
import inspect
import os
import subprocess

import numpy as np
import pytest
import torch

import boundary
import border_restated as br
import iss_restated as ir
import mls_restated as ml

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INCLUDE = os.path.join(ROOT, "include")
HEADER = os.path.join(INCLUDE, "smooth", "vcr_hip_mls.h")
ENTRY_POINTS = ("vcr_mls_weights_f32", "vcr_mls_fit_f32")
KERNELS = {"mls_weights_kernel", "mls_fit_kernel<true>", "mls_fit_kernel<false>", "mls_void_kernel"}
BANNED = ("_iss_", "vcr_query", "VCR_QUERY", "orient_tangent", "vcr_posegraph", "VCR_POSEGRAPH", "vcr_refine_colored",
          "vcr_color_gradient", "vcr_refine_robust", "vcr_information", "VCR_LOSS", "vcr_border", "VCR_BORDER", "vcr_rows")
EINVAL, EUNSUPPORTED = -1, -3
F32, F64 = np.float32, np.float64


@pytest.fixture(scope="module")
def lib():
    import vcrnet_amd  # noqa: F401
    from vcrnet_amd import build, mls
    build.build()
    return mls.lib()


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view({4: np.uint32, 8: np.uint64}[a.dtype.itemsize])


# --------------------------------------------------------------------------------------------------------------- the definition

def test_the_frame_is_the_boundary_pass_s_with_u_normalised():
    rs = np.random.RandomState(0)
    for n in [[0, 0, 2], [3, 0, 0], [0, -1, 0], [1, 1, 1], [1e-30, 0, 0]] + rs.normal(size=(50, 3)).tolist():
        n = np.asarray(n, F32)
        h, u, uh, v = ml.frame([0, 0, 0], n)
        bu, bv = br.frame([0, 0, 0], n)
        assert u.tolist() == bu                                                 # bit for bit the other family's u ...
        raw_v = [h[1] * u[2] - h[2] * u[1], h[2] * u[0] - h[0] * u[2], h[0] * u[1] - h[1] * u[0]]
        assert raw_v == bv                                                      # ... and its v from the same nh and u
        for a in (h, uh, v):
            assert abs(float(a @ a) - 1.0) < 1e-15
        assert abs(float(h @ uh)) < 1e-15 and abs(float(h @ v)) < 1e-15 and abs(float(uh @ v)) < 1e-15
        assert np.linalg.det(np.stack([uh, v, h])) > 0.999
    h, u, uh, v = ml.frame([0, 0, 0], [0, 0, 2])
    assert h.tolist() == [0, 0, 1] and uh.tolist() == [0, 1, 0] and v.tolist() == [-1, 0, 0]
    for bad_n in ([0, 0, 0], [np.nan, 0, 1], [np.inf, 0, 0]):
        assert ml.frame([0, 0, 0], bad_n) is None
    assert ml.frame([np.nan, 0, 0], [0, 0, 1]) is None and ml.frame([0, np.inf, 0], [0, 0, 1]) is None


def header_chains(values):
    """One row's one sum, written from the header's words alone: 64 chains, then six steps."""
    v = [0.0] * 64
    for p in range(64):
        e = p
        while e < len(values):
            v[p] = v[p] + float(values[e])
            e += 64
    for s in (32, 16, 8, 4, 2, 1):
        v = [v[p] + v[p ^ s] for p in range(64)]
    assert len({F64(a).view(np.uint64).item() for a in v}) == 1                 # every chain ends with the same bits
    return v[0]


@pytest.mark.parametrize("L", [65, 129])
def test_the_sums_are_added_in_the_64_chains(L):
    rs = np.random.RandomState(L)
    terms = rs.normal(size=(L, ml.SUMS)) * np.exp(rs.uniform(-8, 8, (L, 1)))
    got = ml.chains(terms)
    assert got.tolist() == [header_chains(terms[:, t]) for t in range(ml.SUMS)] == [ir.chain_loop(terms[:, t]) for t in range(ml.SUMS)]
    assert (got != terms.sum(0)).any()                                          # not numpy's pairwise order
    assert np.allclose(got, terms.sum(0), rtol=1e-9, atol=1e-9 * np.abs(terms).max())
    # ... and through the restatement's sums of a real row: A_00 is the sum of the weights and the point's own, added last
    x = rs.uniform(-1, 1, (3, L + 1)).astype(F32)
    w = rs.uniform(0.1, 1.0, L)
    h, _, uh, v = ml.frame(x[:, 0], [0.1, 0.2, 1.0])
    S = ml.sums(x, 0, np.arange(1, L + 1), w, np.asarray([0.01, 0.02, 0.1]), 0.75, uh, v, h)
    assert S[0] == header_chains(w) + 0.75
    assert S[ml.at(0, 0)] == S[0] and ml.at(5, 5) == 20 and ml.at(1, 1) == 6 and ml.at(0, 5) == 5


def test_the_solve_is_numpy_s_on_well_conditioned_rows():
    rs = np.random.RandomState(3)
    worst = 0.0
    for trial in range(40):
        L = int(rs.randint(12, 80))
        uu, vv, f, w = rs.uniform(-1, 1, L), rs.uniform(-1, 1, L), rs.normal(size=L), rs.uniform(0.2, 1.0, L)
        S = ml.chains(ml.terms_of(w, uu, vv, f))
        c, failed = ml.cholesky_solve(S)
        A = np.zeros((6, 6))
        for a in range(6):
            for b in range(a, 6):
                A[a, b] = A[b, a] = S[ml.at(a, b)]
        assert not failed and np.linalg.cond(A) < 1e4
        want = np.linalg.solve(A, S[21:])
        worst = max(worst, float(np.abs(c - want).max() / np.abs(want).max()))
        P = np.stack([np.ones(L), vv, vv * vv, uu, uu * vv, uu * uu], axis=1)   # PCL's term order
        assert np.allclose(A, (P * w[:, None]).T @ P) and np.allclose(S[21:], (P * w[:, None]).T @ f)
    print("largest relative difference to numpy.linalg.solve", worst)
    assert worst <= 1e-12


def small_cloud(points, normal=(0, 0, 1)):
    x = np.asarray(points, F32).T.copy()
    nrm = np.tile(np.asarray(normal, F32)[:, None], (1, x.shape[1]))
    N = x.shape[1]
    idx, row_start = ir.flat([[j for j in range(N) if j != i] for i in range(N)])
    return x, nrm, idx, row_start


def test_five_points_give_the_plane_and_six_the_quadratic():
    pts = [[0, 0, 0], [1, 0, 0.1], [0, 1, -0.1], [-1, 0.3, 0.05], [0.2, -1, 0.02], [0.7, 0.8, -0.03], [-0.6, -0.7, 0.07]]
    for count, want in ((5, 1), (6, 2), (7, 2)):
        x, nrm, idx, row_start = small_cloud(pts[:count])
        got = ml.definition(x, nrm, (idx, row_start), 4.0)
        assert (got["fit"] == want).all(), count
        assert ((got["coeffs"] == 0).all(1) == (want == 1)).all()
        assert (ml.definition(x, nrm, (idx, row_start), 4.0, order=1)["fit"] == 1).all()
        assert (ml.definition(x, nrm, (idx, row_start), 4.0, min_neighbors=count + 1)["fit"] == 0).all()
    # six points ON a quadratic over the plane z = 0 come back on it: the fit interpolates
    surf = lambda p: 0.05 + 0.1 * p[0] - 0.2 * p[1] + 0.3 * p[0] * p[0] - 0.1 * p[0] * p[1] + 0.2 * p[1] * p[1]   # noqa: E731
    x, nrm, idx, row_start = small_cloud([[p[0], p[1], surf(p)] for p in pts[:6]])
    got = ml.definition(x, nrm, (idx, row_start), 4.0)
    assert (got["fit"] == 2).all() and np.abs(got["points"] - x).max() < 1e-5


def test_a_collinear_row_and_a_row_of_equal_points_fail_their_pivot():
    x, nrm, idx, row_start = ml.hand_cloud()
    got = ml.definition(x, nrm, (idx, row_start), 0.5)
    assert got["fit"][ml.COLLINEAR] == 1 and got["fit"][ml.EQUAL] == 1
    assert (got["coeffs"][[ml.COLLINEAR, ml.EQUAL]] == 0).all()
    assert got["fit"][ml.NAN_OWNER] == 0 and got["fit"][ml.ZERO_NORMAL] == 0 and got["frame"][ml.NAN_OWNER] == 0
    assert np.isnan(got["normals"][:, ml.ZERO_NORMAL]).all() and np.isnan(got["w_self"][ml.ZERO_NORMAL])
    assert np.array_equal(bits(got["points"][:, ml.ZERO_NORMAL]), bits(x[:, ml.ZERO_NORMAL]))
    n = np.diff(row_start)
    ok = np.ones(ml.HAND_N, bool)
    ok[[ml.NAN_POINT, ml.NAN_OWNER, ml.ZERO_NORMAL, ml.COLLINEAR, ml.EQUAL]] = False
    assert set(got["fit"][ok & (n + 1 < 3)]) == {0} and set(got["fit"][ok & (n + 1 >= 3) & (n + 1 < 6)]) == {1}
    assert (got["fit"][ok & (n >= 63)] == 2).all()
    assert set(n.tolist()) >= set(ml.LENGTHS)
    w = got["weight"]
    assert (w[~np.isnan(w)] == 0).sum() > 10 and np.isfinite(got["coeffs"]).all()          # the skipped entries: weight +0.0


def test_the_lattice_in_a_plane_comes_back_with_its_bits():
    x, nrm = ml.plane_lattice()
    got = ml.of_cloud(x, nrm, 4.0)
    assert (got["fit"] == 2).all() and np.array_equal(bits(got["points"]), bits(x))
    assert (got["coeffs"] == 0).all() and np.array_equal(got["normals"], nrm)
    assert np.diff(ml.hybrid_rows(x, 4.0)["row_start"]).min() >= 10


@functools.lru_cache(maxsize=None)
def sphere_case(seed):
    x = ml.noisy_sphere(seed)
    rows = ml.hybrid_rows(x, ml.SPHERE_RADIUS)
    nrm = ml.sphere_normals(x, rows=rows)
    return x, nrm, rows


@pytest.mark.parametrize("seed", ml.SEEDS)
def test_the_quadratic_smooths_the_noisy_sphere_and_the_plane_flattens_it(seed):
    """1 200 points on the unit sphere, radial noise of sigma 0.01, radius 0.3.  Measured with this restatement (seeds 0, 1, 2):
    rms radial error in 0.01005 / 0.01012 / 0.00983; order 2 out 0.00419 / 0.00398 / 0.00408 (0.39 - 0.42 of the input's);
    order 1 out 0.02145 / 0.02064 / 0.02123 (2.0 - 2.2 times the input's); the normals' mean angle to the radial direction
    1.68 / 1.68 / 1.77 degrees in and 1.17 / 1.15 / 1.22 out; rows of 12 to 44 entries."""
    x, nrm, rows = sphere_case(seed)
    two = ml.of_cloud(x, nrm, ml.SPHERE_RADIUS, rows=rows)
    one = ml.of_cloud(x, nrm, ml.SPHERE_RADIUS, order=1, rows=rows)
    rms_in, rms_two, ang_in, ang_two = ml.smoothing(x, nrm, two)
    rms_one = ml.radial_rms(one["points"])
    print("seed", seed, "rms in", rms_in, "order 2", rms_two, "order 1", rms_one, "angle in", ang_in, "order 2", ang_two,
          "row lengths", int(np.diff(rows["row_start"]).min()), int(np.diff(rows["row_start"]).max()))
    assert (two["fit"] == 2).all() and (one["fit"] == 1).all()
    assert rms_two <= 0.5 * rms_in
    assert rms_one >= rms_in
    assert ang_two < ang_in


# ---------------------------------------------------------------------------------------------------------------- the boundary

def test_signatures_match_the_header_and_the_library_exports_them(lib):
    from vcrnet_amd import mls
    boundary.check_signatures(HEADER, mls, lib, ENTRY_POINTS)


def test_args_match_the_c_layout(tmp_path):
    import vcrnet_amd  # noqa: F401
    from vcrnet_amd import mls
    assert set(mls.STRUCTS) == {"vcr_mls_weights_args", "vcr_mls_fit_args"}
    boundary.check_layout(HEADER, mls, tmp_path)
    A = mls.MlsFitArgs
    assert A.normals_out.offset == A.fit.offset + 8           # where the mandatory part ends
    for S in mls.STRUCTS.values():
        assert S._fields_[0][0] == "struct_bytes"


def test_the_other_boundaries_are_where_they_were(lib):
    """The header is alone in a directory of its own and includes its base by relative path; it carries no other family's call
    name and no other header carries its; ABI 27, the same 51 prototypes; it enters the digest of mls.o ALONE and not the
    profiles' digest; the header's numbers are the module's."""
    import vcrnet_amd
    from vcrnet_amd import border, build, iss, mls, native, rows
    assert os.listdir(os.path.join(INCLUDE, "smooth")) == ["vcr_hip_mls.h"]
    text = open(HEADER).read()
    for word in BANNED:
        assert word not in text, word
    for dirpath, _, files in os.walk(INCLUDE):
        for f in files:
            path = os.path.join(dirpath, f)
            if path != HEADER:
                other = open(path).read()
                assert "vcr_mls" not in other and "VCR_MLS" not in other, path
    assert '#include "../vcr_hip.h"' in text and text.count("#include") == 1
    assert len(native.PUBLIC) == 51 and lib.vcr_abi_version() == native.ABI_VERSION == 27
    for other in (native, rows, iss, border):
        assert not set(mls.SIGNATURES) & set(other.SIGNATURES) and not set(mls.STRUCTS) & set(other.STRUCTS)
    assert all(n.startswith("vcr_mls_") for n in mls.SIGNATURES)
    assert build.MLS_HEADERS == [HEADER] and build.OWN_HEADERS["mls.hip"] == [HEADER]
    assert [k for k, v in build.OWN_HEADERS.items() if HEADER in v] == ["mls.hip"]
    flags = " ".join(build.FLAGS)
    hdrs = sorted(os.path.join(build.CSRC, f) for f in os.listdir(build.CSRC) if f.endswith(".h"))
    hdrs += (build.PUBLIC_HEADERS + build.LATER_HEADERS + build.OUTLIER_HEADERS + build.GICP_HEADERS + build.FPFH_HEADERS
             + build.MATCH_HEADERS + build.FGR_HEADERS + build.GRID_HEADERS + build.GRIDNN_HEADERS + build.VOXEL_SORT_HEADERS
             + build.RADIUS_HEADERS + build.ROWS_HEADERS + build.DBSCAN_HEADERS + build.SEGMENT_HEADERS + build.ORIENT_HEADERS
             + build.ISS_HEADERS + build.QUERY_HEADERS)
    assert HEADER not in hdrs
    sha = lambda name: open(os.path.join(build.OBJ, name + ".o.sha")).read()    # noqa: E731 (build() ran in the fixture)
    src = lambda name: os.path.join(build.CSRC, name + ".hip")                  # noqa: E731
    assert sha("mls") == build._digest([src("mls")] + hdrs + [HEADER], flags) != build._digest([src("mls")] + hdrs, flags)
    for name in ("iss", "rows", "radius", "forward"):
        assert sha(name) == build._digest([src(name)] + hdrs, flags), name
    assert sha("border") == build._digest([src("border")] + hdrs + build.BORDER_HEADERS, flags)
    source = open(src("mls")).read()
    assert "atomic" not in source.replace("No atomics", "") and "hipMalloc" not in source and "Synchronize" not in source
    assert "smooth_mls" in vcrnet_amd.__all__ and "mls" not in vcrnet_amd.__all__
    assert vcrnet_amd.smooth_mls is mls.smooth_mls
    for name, value in (("VCR_MLS_MAX_N", mls.MAX_N), ("VCR_MLS_PLAIN", mls.FORMS["plain"]),
                        ("VCR_MLS_TRANSPOSE", mls.FORMS["transpose"]), ("VCR_MLS_TERMS", mls.TERMS),
                        ("VCR_MLS_NOT_SERVED", "(%d)" % mls.NOT_SERVED)):
        assert "#define %s %s" % (name, value) in text, name
    assert mls.NOT_SERVED == ml.NOT_SERVED == iss.NOT_SERVED == border.NOT_SERVED and mls.MAX_N == iss.MAX_N
    assert mls.TERMS == ml.TERMS and "2^-40" in text and ml.TINY == 2.0 ** -40
    h = hashlib_of_profiles(build)
    assert h == build.sources_sha16()


def hashlib_of_profiles(build):
    """sources_sha16 recomputed from the lists it is defined over: the new header is in none of them."""
    import hashlib
    h = hashlib.sha256()
    files = sorted(os.path.join(build.CSRC, f) for f in os.listdir(build.CSRC) if f.endswith((".hip", ".h")))
    files += (build.PUBLIC_HEADERS + build.LATER_HEADERS + build.OUTLIER_HEADERS + build.GICP_HEADERS + build.FPFH_HEADERS
              + build.MATCH_HEADERS + build.FGR_HEADERS + build.GRID_HEADERS + build.GRIDNN_HEADERS + build.VOXEL_SORT_HEADERS
              + build.RADIUS_HEADERS + build.ROWS_HEADERS + build.DBSCAN_HEADERS + build.SEGMENT_HEADERS + build.ORIENT_HEADERS
              + build.ISS_HEADERS + build.QUERY_HEADERS + build.SUPPORT_HEADERS)
    assert HEADER not in files
    for f in files:
        h.update(os.path.basename(f).encode())
        h.update(open(f, "rb").read())
    return h.hexdigest()[:16]


def _args(kind, **kw):
    from vcrnet_amd import mls
    a = {"weights": mls.MlsWeightsArgs, "fit": mls.MlsFitArgs}[kind]()
    for k, f in enumerate(n for n, t in a._fields_ if t is ctypes.c_void_p):       # (never dereferenced)
        setattr(a, f, 0x1000 * (k + 1))
    v = dict(B=2, N=1000, capacity=30000)
    v.update(dict(sqr_gauss_param=0.09) if kind == "weights" else dict(order=2, min_neighbors=3, variant=0))
    v.update(kw)
    for k, x in v.items():
        setattr(a, k, x)
    return a


def test_the_calls_return_their_argument_errors_without_a_gpu(lib):
    wts = lambda **kw: lib.vcr_mls_weights_f32(ctypes.byref(_args("weights", **kw)), None)       # noqa: E731
    fit = lambda **kw: lib.vcr_mls_fit_f32(ctypes.byref(_args("fit", **kw)), None)               # noqa: E731
    for fn in (lib.vcr_mls_weights_f32, lib.vcr_mls_fit_f32):
        assert fn(None, None) == EINVAL
    for field in ("xyz4", "normals", "idx", "row_start", "total", "weight", "origin", "w_self", "frame"):
        assert wts(**{field: None}) == EINVAL, field
        assert fit(**{field: None}) == EINVAL, field
    for field in ("points", "fit"):
        assert fit(**{field: None}) == EINVAL, field
    for fn in (wts, fit):
        assert fn(xyz4=0x1008) == EINVAL
        for kw in (dict(B=0), dict(capacity=-1)):
            assert fn(**kw) == EINVAL, kw
        for kw in (dict(N=0), dict(N=131073), dict(B=16384, N=131072), dict(B=4, capacity=1 << 29)):
            assert fn(**kw) == EUNSUPPORTED, kw
    for bad in (0.0, -1.0, float("nan"), float("inf")):
        assert wts(sqr_gauss_param=bad) == EINVAL, bad
    for kw in (dict(order=0), dict(order=3), dict(min_neighbors=0), dict(min_neighbors=-2), dict(variant=3), dict(variant=-1)):
        assert fit(**kw) == EINVAL, kw
    for kind, fn in (("weights", lib.vcr_mls_weights_f32), ("fit", lib.vcr_mls_fit_f32)):
        size = ctypes.sizeof(type(_args(kind)))
        for wrong in (0, size - 32, size + 8):
            a = _args(kind)
            a.struct_bytes = wrong
            assert fn(ctypes.byref(a), None) == EINVAL, (kind, wrong)


def test_the_kernels_of_mls_hip_use_no_scratch():
    """hipcc's remarks for mls.hip: its kernel set is the four below, none with scratch, a spill, AGPRs or (but for the check's
    vote) LDS; the weights run at eight waves a SIMD, the fit -- 27 fp64 sums and a 6 x 6 factor a lane -- within 160 VGPRs, at
    three waves a SIMD or more."""
    import vcrnet_amd  # noqa: F401
    from vcrnet_amd import build
    build.build()
    res = build.kernel_resources()
    names = list(res)
    dem = subprocess.run(["c++filt"], input="\n".join(names), capture_output=True, text=True, check=True).stdout.splitlines()
    by_name = {d.replace("(anonymous namespace)::", "").replace("void ", "").split("(")[0]: res[n] for n, d in zip(names, dem)}
    mine = {d: v for d, v in by_name.items() if v["file"] == "mls.hip"}
    assert set(mine) == KERNELS
    for d, v in mine.items():
        print(d, v)
        assert v.get("scratch", 0) == 0 and v.get("vgpr_spill", 0) == 0 and v.get("sgpr_spill", 0) == 0 and v["agprs"] == 0, (d, v)
        assert v["vgprs"] <= 160 and v["occupancy"] >= 3, (d, v)
        assert (v["lds"] > 0) == (d == "mls_void_kernel"), (d, v)
    assert mine["mls_weights_kernel"]["occupancy"] == 8 and mine["mls_fit_kernel<true>"]["vgprs"] <= 128


# ------------------------------------------------------------------------------------------------------------ the Python layer

def test_python_entry_points_refuse_what_they_cannot_run():
    import vcrnet_amd
    from vcrnet_amd import mls, native
    fn = vcrnet_amd.smooth_mls
    E = native.VcrHipError
    params = inspect.signature(fn).parameters
    assert list(params) == ["xyz", "radius", "normals", "order", "max_nn", "sqr_gauss_param", "min_neighbors", "capacity", "cell",
                            "want_normals", "want_coeffs"]
    assert [params[k].default for k in list(params)[1:]] == [None, None, 2, None, None, 3, None, None, False, False]
    x = torch.zeros(2, 3, 50)
    for bad in (x.transpose(1, 2), torch.zeros(3, 50), None, "xyz"):
        with pytest.raises(E, match=r"smooth_mls: xyz must be a \[B, 3, N\]"):
            fn(bad, 0.1)
    with pytest.raises(E, match="a cloud must have 1 ... 131072 points"):
        fn(torch.zeros(1, 3, 131073), 0.1)
    with pytest.raises(E, match="smooth_mls: radius has no default"):
        fn(x)
    for bad in (0.0, -1.0, float("nan"), float("inf"), "r", 1e30):
        with pytest.raises(E, match="smooth_mls: radius must be finite and > 0"):
            fn(x, bad)
    for bad in (torch.zeros(2, 3, 49), torch.zeros(1, 3, 50), torch.zeros(2, 50, 3), "n"):
        with pytest.raises(E, match=r"smooth_mls: normals must be None or a \[B, 3, N\]"):
            fn(x, 0.1, bad)
    for bad in (0, 3, -1, 2.0, "2", True, None):
        with pytest.raises(E, match="smooth_mls: order must be 1"):
            fn(x, 0.1, order=bad)
    for bad in (0, -1, 63, 2.0, "5", True):
        with pytest.raises(E, match=r"smooth_mls: max_nn must be None or an integer in \[1, 62\]"):
            fn(x, 0.1, max_nn=bad)
    for bad in (0.0, -1.0, float("nan"), float("inf"), "a", True):
        with pytest.raises(E, match="smooth_mls: sqr_gauss_param must be None or finite and > 0"):
            fn(x, 0.1, sqr_gauss_param=bad)
    for bad in (0, -1, 2.0, "5", True, None):
        with pytest.raises(E, match="smooth_mls: min_neighbors must be an integer >= 1"):
            fn(x, 0.1, min_neighbors=bad)
    with pytest.raises(E, match="smooth_mls: capacity must be None or an integer >= 0"):
        fn(x, 0.1, capacity=-1)
    for kw in (dict(), dict(max_nn=30), dict(normals=torch.zeros(2, 3, 50)), dict(order=1, sqr_gauss_param=0.02),
               dict(capacity=100, cell=0.3, want_normals=True, want_coeffs=True)):
        with pytest.raises(E, match="no CPU fallback"):      # (the last refusal: everything else was in order)
            fn(x, 0.1, **kw)
    assert mls.check_arguments("f", 0.3) == 0.3 * 0.3 and mls.check_arguments("f", 0.3, sqr_gauss_param=2) == 2.0
    # the raw calls
    N, cap = 50, 64
    xyz4, nrm, idx = torch.zeros(2, N, 4), torch.zeros(2, 3, N), torch.zeros(2, cap, dtype=torch.int32)
    rs, tot = torch.zeros(2, N + 1, dtype=torch.int64), torch.zeros(2, dtype=torch.int64)
    w, o = torch.zeros(2, cap, dtype=torch.float64), torch.zeros(2, N, 3, dtype=torch.float64)
    ws, fr = torch.zeros(2, N, dtype=torch.float64), torch.zeros(2, N, dtype=torch.int32)
    stage_a = lambda a=xyz4, b=nrm, c=idx, d=rs, e=tot, h2=0.1: mls.weights_rows(a, b, c, d, e, h2)           # noqa: E731
    stage_b = lambda a=xyz4, b=nrm, c=idx, d=rs, e=tot, **kw: mls.fit_rows(a, b, c, d, e, *[kw.pop(k, t) for k, t in  # noqa: E731
                                                                             (("weight", w), ("origin", o), ("w_self", ws),
                                                                              ("frame", fr))], **kw)
    for name, call in (("mls.weights_rows", stage_a), ("mls.fit_rows", stage_b)):
        for bad in (xyz4[:, :, :3], xyz4.double(), None):
            with pytest.raises(E, match=name + r": xyz4 must be float32 \[B, N, 4\]"):
                call(a=bad)
        for bad in (nrm.double(), nrm[:, :, :N - 1], nrm.transpose(1, 2), None):
            with pytest.raises(E, match=name + r": normals must be float32 \[B, 3, N\]"):
                call(b=bad)
        for bad in (idx.long(), idx[:1], idx[0], None):
            with pytest.raises(E, match=name + r": idx must be int32 \[B, capacity\]"):
                call(c=bad)
        for bad in (rs[:, :N], rs.int(), None):
            with pytest.raises(E, match=name + r": row_start must be int64 \[B, N \+ 1\]"):
                call(d=bad)
        for bad in (tot[:1], tot.int(), None):
            with pytest.raises(E, match=name + r": total must be int64 \[B\]"):
                call(e=bad)
    for bad in (0.0, -2.0, float("nan"), None, "h"):
        with pytest.raises(E, match="mls.weights_rows: sqr_gauss_param must be None or finite and > 0"):
            stage_a(h2=bad)
    for name, good in (("weight", w), ("origin", o), ("w_self", ws), ("frame", fr)):
        for bad in (good[:1], good.float() if good.dtype != torch.int32 else good.long(), None):
            with pytest.raises(E, match=f"mls.fit_rows: {name} must be"):
                stage_b(**{name: bad})
    for bad in ("lane", 3, True):
        with pytest.raises(E, match="mls.fit_rows: variant must be 0"):
            stage_b(variant=bad)
    with pytest.raises(E, match="mls.fit_rows: order must be 1"):
        stage_b(order=3)
    with pytest.raises(E, match="mls.fit_rows: min_neighbors must be an integer >= 1"):
        stage_b(min_neighbors=0)
    for call in (stage_a, lambda: stage_b(variant="transpose"), lambda: stage_b(order=1, want_normals=False, want_coeffs=False)):
        with pytest.raises(E, match="no CPU fallback|device tensors only"):
            call()
