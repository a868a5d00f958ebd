"""include/cpd/vcr_hip_cpd.h without a GPU: the boundary -- the header as C and as C++, the prototypes,
the struct's layout, the error codes, the host-only form and workspace queries, the build's lists, the kernels' resources --, the
numpy restatement (tests/cpd_restated.py) against an independent dense fp64 CPD and on the recovery recipe, and what the two
Python calls refuse."""
import ctypes
import math
import os
import subprocess

import numpy as np
import pytest
import torch

import boundary
import cpd_restated as cr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INCLUDE = os.path.join(ROOT, "include")
HEADER = os.path.join(INCLUDE, "cpd", "vcr_hip_cpd.h")
EINVAL, EWORKSPACE, EUNSUPPORTED = -1, -2, -3
ENTRY_POINTS = {"vcr_cpd_expectation_workspace_bytes", "vcr_cpd_expectation_f32", "vcr_cpd_expectation_form",
                "vcr_cpd_workspace_bytes", "vcr_cpd_f32", "vcr_cpd_form"}
KERNELS = {"cpd_init_kernel", "cpd_move_kernel", "cpd_col_kernel", "cpd_row_kernel", "cpd_np_kernel", "cpd_stage_kernel",
           "cpd_step_kernel", "cpd_finish_kernel"} | {"cpd_pass_kernel<%s, %s, %d>" % (p2, sc, ppl) for p2 in ("false", "true")
                                                      for sc in ("false", "true") for ppl in (1, 2, 4)}
F32 = np.float32
# The exact copy's floor.  sigma2_new is a difference of sums of size Np r^2 whose inputs carry fp32 products (p * x): below about
# 2^-24 r^2 / 3 it is rounding noise -- with the torus' mean squared radius r^2 = 1.3 that is 2.6e-8, and the restated trace
# wanders between 0.8e-8 and 2.2e-8 there, above the default floor (1e-8 of a start of 0.63), which it therefore never meets.
# 2^-25 = 2.98e-8 sits on that noise: the recipe was fixed, not the bound (the issue's prototype kept p in fp64).
COPY_FLOOR = 2.0 ** -25


@pytest.fixture(scope="module")
def lib():
    import vcrnet_amd  # noqa: F401
    from vcrnet_amd import build, cpd
    build.build()
    return cpd.lib()


# ----------------------------------------------------------------------------------------------------------------- the boundary

@pytest.mark.parametrize("language,compiler", [("c", "gcc"), ("c++", "g++")])
def test_the_header_compiles_as_c_and_as_cpp(language, compiler, tmp_path):
    src = tmp_path / ("use." + ("c" if language == "c" else "cpp"))
    src.write_text('#include "cpd/vcr_hip_cpd.h"\n'
                   "int main(void) { vcr_cpd_args a; a.struct_bytes = sizeof a; return a.struct_bytes == VCR_CPD_SEGMENT; }\n")
    r = subprocess.run([compiler, "-x", language, "-Wall", "-Werror", "-pedantic", "-fsyntax-only", "-I", INCLUDE, str(src)],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr


def test_signatures_match_the_header_and_the_library_exports_them(lib):
    from vcrnet_amd import cpd
    boundary.check_signatures(HEADER, cpd, lib, ENTRY_POINTS)


def test_args_match_the_c_layout(tmp_path):
    import vcrnet_amd  # noqa: F401
    from vcrnet_amd import cpd
    boundary.check_layout(HEADER, cpd, tmp_path)
    text = open(HEADER).read()
    for name, v in (("TILE", cpd.TILE), ("SEGMENT", cpd.SEGMENT), ("STATE_BYTES", cpd.STATE_BYTES), ("FORMS", cpd.FORMS)):
        assert "#define VCR_CPD_%s %d" % (name, v) in text
    for code, name in enumerate(("CONVERGED", "MAX_ITERATIONS", "COLLAPSED", "NO_MASS", "NOT_FINITE")):
        assert "#define VCR_CPD_%s %d" % (name, code) in text
    assert cpd.STATUS == cr.STATUS and len(cpd.STATUS) == 5 and (cr.TILE, cr.SEGMENT) == (cpd.TILE, cpd.SEGMENT)
    assert len(cpd.VARIANTS) == 21 and cpd.VARIANTS[0] == 0


def test_the_call_lives_beside_the_other_headers_not_in_them(lib):
    """No other public header mentions it, the ABI version is where it was, and the header enters the digest of cpd.o alone."""
    from vcrnet_amd import build, cpd, native, ndt
    for d, _, files in os.walk(INCLUDE):
        for f in files:
            if os.path.join(d, f) != HEADER:
                assert "vcr_cpd" not in open(os.path.join(d, f)).read(), f
    assert lib.vcr_abi_version() == native.ABI_VERSION == 27
    for other in (native, ndt):
        assert not set(cpd.SIGNATURES) & set(other.SIGNATURES) and not set(cpd.STRUCTS) & set(other.STRUCTS)
    assert not set(cpd.SIGNATURES) & set(native.PUBLIC)
    assert build.CPD_HEADERS == [HEADER] and build.OWN_HEADERS["cpd.hip"] is build.CPD_HEADERS
    assert [k for k, v in build.OWN_HEADERS.items() if HEADER in v] == ["cpd.hip"]
    import vcrnet_amd
    for name in ("coherent_point_drift", "cpd_expectation"):
        assert name in vcrnet_amd.__all__ and getattr(vcrnet_amd, name) is getattr(cpd, name)


def _args(loop, **kw):
    from vcrnet_amd import cpd
    a = cpd.CpdArgs()
    v = dict(src=0x1000, tgt=0x2000, B=2, M=1000, N=900, sigma2=0.5, scale=1.0, w=0.1, Pt1=0x3000, P1=0x4000, PX=0x5000, Np=0x6000)
    if loop:
        v.update(max_iterations=50, tolerance=1e-4, R_out=0x7000, t_out=0x8000)                # (never dereferenced)
    v.update(kw)
    for k, x in v.items():
        setattr(a, k, x)
    return a


def _codes(lib, a, loop):
    entry = "vcr_cpd" if loop else "vcr_cpd_expectation"
    rc = getattr(lib, entry + "_f32")(ctypes.byref(a), 0x10000, 1 << 40, None)
    assert getattr(lib, entry + "_workspace_bytes")(ctypes.byref(a), 256) == 0
    assert getattr(lib, entry + "_form")(ctypes.byref(a), 256, None, None, None) == rc
    return rc


def test_argument_errors_return_their_codes_without_a_gpu(lib):
    from vcrnet_amd import cpd
    nan, inf = float("nan"), float("inf")
    assert lib.vcr_cpd_f32(None, None, 0, None) == EINVAL and lib.vcr_cpd_expectation_f32(None, None, 0, None) == EINVAL
    assert lib.vcr_cpd_workspace_bytes(None, 256) == 0
    for loop in (False, True):
        for field in ("src", "tgt", "Pt1", "P1", "PX") + (("R_out", "t_out") if loop else ("Np",)):
            assert _codes(lib, _args(loop, **{field: None}), loop) == EINVAL, field
        for kw in (dict(B=0), dict(M=0), dict(N=0), dict(B=-1), dict(R=0x100), dict(t=0x100), dict(w=-0.1), dict(w=1.0), dict(w=nan),
                   dict(sigma2=-1.0), dict(sigma2=nan), dict(sigma2=inf), dict(variant=-1), dict(variant=7), dict(variant=24),
                   dict(variant=15)):
            assert _codes(lib, _args(loop, **kw), loop) == EINVAL, kw
        for kw in (dict(M=131073), dict(N=131073), dict(B=16384, M=131072), dict(B=16384, N=131072)):
            assert _codes(lib, _args(loop, **kw), loop) == EUNSUPPORTED, kw
        for bad in (0, cpd.CpdArgs.max_iterations.offset - 8, ctypes.sizeof(cpd.CpdArgs) + 8):
            a = _args(loop)
            a.struct_bytes = bad
            assert _codes(lib, a, loop) == EINVAL, bad
        for v in cpd.VARIANTS:
            assert getattr(lib, "vcr_cpd_workspace_bytes" if loop else "vcr_cpd_expectation_workspace_bytes")(ctypes.byref(_args(loop, variant=v)), 256) > 0
        # a per-cloud sigma2 on the device stands in for the host's
        assert getattr(lib, "vcr_cpd_workspace_bytes" if loop else "vcr_cpd_expectation_workspace_bytes")(
            ctypes.byref(_args(loop, sigma2=0.0, sigma2_dev=0x9000)), 256) > 0
    assert _codes(lib, _args(False, sigma2=0.0), False) == EINVAL                               # only the loop computes a start
    assert lib.vcr_cpd_workspace_bytes(ctypes.byref(_args(True, sigma2=0.0)), 256) > 0
    for kw in (dict(scale=0.0), dict(scale=-1.0), dict(scale=nan), dict(scale=inf)):
        assert _codes(lib, _args(False, **kw), False) == EINVAL, kw
    assert lib.vcr_cpd_expectation_workspace_bytes(ctypes.byref(_args(False, scale=0.0, scale_dev=0x9000)), 256) > 0
    for kw in (dict(max_iterations=-1), dict(tolerance=-1.0), dict(tolerance=nan), dict(sigma2_floor=-1.0), dict(sigma2_floor=nan),
               dict(sigma2_floor=inf)):
        assert _codes(lib, _args(True, **kw), True) == EINVAL, kw
    assert _codes(lib, _args(True, max_iterations=(1 << 20) + 1), True) == EUNSUPPORTED
    # the expectation call ignores what follows e_stage: its mandatory part alone is served
    a = _args(False)
    a.struct_bytes = cpd.CpdArgs.max_iterations.offset
    assert lib.vcr_cpd_expectation_workspace_bytes(ctypes.byref(a), 256) > 0
    assert cpd.CpdArgs.max_iterations.offset == cpd.CpdArgs.e_stage.offset + 8


def test_the_forms_and_the_workspaces_are_host_only_queries(lib):
    from vcrnet_amd import cpd
    up = lambda v: (v + 255) & ~255                                               # noqa: E731
    for B, M, N in ((1, 1, 1), (2, 1000, 900), (3, 4097, 300), (3, 300, 8200), (16, 1024, 1024), (1, 131072, 131072)):
        sm, sn = -(-M // 4096), -(-N // 4096)
        want = up(cpd.STATE_BYTES * B) + up(16 * B * M) + up(16 * B * N) + up(8 * B * sm * N) + up(32 * B * sn * M)
        for loop in (False, True):
            for v in cpd.VARIANTS:
                for cu in (1, 104, 256):
                    form, s1, s2, ws = cpd.cpd_form(B, M, N, loop=loop, cu_count=cu, variant=v)
                    assert ws == want and 1 <= form <= cpd.FORMS and 1 <= s1 <= sm and 1 <= s2 <= sn
                    if v & 7:
                        assert form == v & 7
                    if v >> 3 == 1:
                        assert (s1, s2) == (1, 1)
                    if v >> 3 == 2:
                        assert (s1, s2) == (sm, sn)
    # the deal fills the chip: one big cloud is split, sixteen small ones are not
    assert cpd.cpd_form(16, 1024, 1024)[1:3] == (1, 1)
    form, s1, s2, _ = cpd.cpd_form(1, 131072, 131072)
    ppl = (1, 2, 4)[(form - 1) % 3]
    assert s1 * -(-131072 // (256 * ppl)) >= 256 and s2 == s1
    a = _args(True)
    ws = lib.vcr_cpd_workspace_bytes(ctypes.byref(a), 256)
    assert ws > 0 and lib.vcr_cpd_workspace_bytes(ctypes.byref(a), -1) == 0
    assert lib.vcr_cpd_f32(ctypes.byref(a), None, ws, None) == EINVAL
    assert lib.vcr_cpd_f32(ctypes.byref(a), 0x10008, ws, None) == EINVAL
    assert lib.vcr_cpd_f32(ctypes.byref(a), 0x10000, ws - 1, None) == EWORKSPACE
    assert lib.vcr_cpd_expectation_f32(ctypes.byref(_args(False)), 0x10000, ws - 1, None) == EWORKSPACE


def test_the_new_kernels_use_no_scratch():
    import vcrnet_amd  # noqa: F401
    from vcrnet_amd import build
    build.build()
    res = build.kernel_resources()
    names = list(res)
    dem = subprocess.run(["c++filt"], input="\n".join(names), capture_output=True, text=True, check=True).stdout.splitlines()
    mine = {d.replace("(anonymous namespace)::", "").replace("void ", "").split("(")[0]: res[n]
            for n, d in zip(names, dem) if res[n]["file"] == "cpd.hip"}
    mine.pop("vcr_copy_words_kernel", None)                                       # (common.h's, compiled into every object)
    assert set(mine) == KERNELS
    for d, v in mine.items():
        print(d, v)
        assert v.get("scratch", 0) == 0 and v.get("vgpr_spill", 0) == 0, (d, v)
        if d.startswith("cpd_pass_kernel"):                                       # the LDS forms hold one tile of 16-B records
            assert v["lds"] == (4096 if ", false, " in d else 0) and v["occupancy"] >= 4, (d, v)


# ------------------------------------------------------------------------------------------------------------- the restatement

dense_cpd_round = cr.dense_cpd_round


# What the fp32 weights may cost a round against fp64.  A weight e = exp2(d2 k) carries the roundings of d (3), of d2 (5 more) and of
# the product with k, each 2^-24 of a value that d2 k then multiplies into e's relative error: |d2 k| ln 2 * 9 * 2^-24, with
# |d2 k| <= 60 for any pair that matters (e >= 2^-60 of the largest), plus e's own and p's roundings: some 400 * 2^-24 = 2.4e-5
# relative per weight, not all of one sign.  sigma2_new and the pose are ratios of sums of them; sigma2_new also cancels
# (xPx - 2 trAR + yPy is sigma2 / r^2 of its terms, r^2 about 1.3): over a round from the SAME state
#   |sigma2' - sigma2'_64| <= 2.4e-5 * (1 + r^2 / sigma2') * sigma2',   |pose' - pose'_64| <= 2.4e-5 * 10
ROUND_REL = 2.4e-5


def test_the_restated_round_is_the_dense_fp64_round_within_the_fp32_weights():
    src, tgt, Rg, tg = cr.recipe(0.8, 0.3, 0)
    Y, X = src.astype(np.float64), tgt.astype(np.float64)
    R, t, s = np.eye(3), np.zeros(3), 1.0
    s2 = cr.sigma2_start(src, tgt)
    assert abs(s2 - ((X[:, None, :] - Y[:, :, None]) ** 2).sum() / (3 * 500 * 700)) <= 1e-12 * s2
    worst = [0.0, 0.0]
    for it in range(30):
        E = cr.expectation(src, tgt, s2, R, t, s, 0.1)
        m = cr.mstep(src, tgt, E["Pt1"], E["P1"], E["PX"], with_scaling=(it % 2 == 1))
        Rd, td, sd, s2d = dense_cpd_round(Y, X, R.astype(F32).astype(np.float64), t.astype(F32).astype(np.float64), s, s2, 0.1, it % 2 == 1)
        ds = abs(m["sigma2"] - s2d) / ((1 + 1.3 / s2d) * s2d)
        dp = max(np.abs(m["R"] - Rd).max(), np.abs(m["t"] - td).max(), abs(m["s"] - sd))
        worst = [max(worst[0], ds), max(worst[1], dp)]
        assert ds <= ROUND_REL and dp <= 10 * ROUND_REL, (it, ds, dp)
        R, t, s, s2 = m["R"].astype(F32).astype(np.float64), m["t"].astype(F32).astype(np.float64), m["s"], m["sigma2"]
    print("fp32 weights against fp64 over 30 rounds: sigma2 %.3g of its allowance's unit, pose %.3g" % tuple(worst))
    assert s2 < 0.01                                                              # (the rounds went somewhere)


def test_both_solve_three_points_by_hand():
    """Three points turned by 90 degrees about z and shifted, at a sigma2 far under their spacing: the assignment is the
    identity, so one round returns the pose exactly (to rounding) and a variance of rounding size."""
    Y = np.array([[0.0, 1.0, 0.0], [0.0, 0.0, 2.0], [0.0, 0.0, 0.0]])
    Rz = np.array([[0.0, -1.0, 0.0], [1.0, 0.0, 0.0], [0.0, 0.0, 1.0]])
    tz = np.array([0.5, -0.25, 1.0])
    X = Rz @ Y + tz[:, None]
    start = cr.pose(0.1, 0.0, 3)[0]
    R0 = (start @ Rz).astype(F32).astype(np.float64)
    E = cr.expectation(Y.astype(F32), X.astype(F32), 0.01, R0, tz.astype(F32), 1.0, 0.0)
    assert np.allclose(E["P1"], 1.0, atol=1e-6) and np.allclose(E["Pt1"], 1.0, atol=1e-6) and abs(E["Np"] - 3.0) < 1e-6
    assert np.allclose(E["PX"] / E["P1"], X, atol=1e-6)                           # the virtual correspondences are the partners
    m = cr.mstep(Y.astype(F32), X.astype(F32), E["Pt1"], E["P1"], E["PX"])
    Rd, td, sd, s2d = dense_cpd_round(Y, X, R0, tz, 1.0, 0.01, 0.0)
    for R, t, s2 in ((m["R"], m["t"], m["sigma2"]), (Rd, td, s2d)):
        assert np.abs(R - Rz).max() < 1e-6 and np.abs(t - tz).max() < 1e-6 and abs(s2) < 1e-6


def test_the_sum_hierarchy_is_tiles_segments_total():
    rs = np.random.RandomState(3)
    terms = (rs.standard_normal((8200, 2)) * 10.0 ** rs.randint(-6, 6, size=(8200, 2))).astype(F32)
    got = cr.hier_sum(terms)
    for col in range(2):
        total = 0.0
        for s0 in range(0, 8200, 4096):
            seg = 0.0
            for t0 in range(s0, min(s0 + 4096, 8200), 256):
                acc = F32(0)
                for v in terms[t0:min(t0 + 256, 8200), col]:
                    acc = F32(acc + v)
                seg = seg + float(acc)
            total = total + seg
        assert got[col] == total
    vals = rs.standard_normal((2, 3, 300))
    b = cr.block_sum(vals)
    import ndt_restated as nd
    ref = nd.reduce_points(np.concatenate([vals.reshape(6, 300), np.zeros((23, 300))]))
    assert cr.same_bits(b.reshape(6), ref[:6])


# ---------------------------------------------------------------------------------------------------------------- the recipe

def angle_error(R, Rg):
    """The angle of R Rg^T by atan2 of its skew part: acos((tr - 1) / 2) cannot resolve under 3e-4 rad on an fp32 rotation."""
    D = np.asarray(R, np.float64) @ Rg.T
    v = 0.5 * np.array([D[2, 1] - D[1, 2], D[0, 2] - D[2, 0], D[1, 0] - D[0, 1]])
    return math.atan2(float(np.linalg.norm(v)), (np.trace(D) - 1.0) / 2.0)


@pytest.mark.parametrize("seed", cr.SEEDS)
@pytest.mark.parametrize("angle", cr.ANGLES)
def test_the_restated_loop_meets_the_recipes_conditions(angle, seed):
    src, tgt, Rg, tg = cr.recipe(angle, cr.SHIFT, seed)
    o = cr.cpd(src, tgt, w=0.1, tolerance=1e-4, max_iterations=150)
    ea, es = cr.pose_error(o["R"], o["t"], Rg, tg)
    print("restated recipe %g rad seed %d: status %s iterations %d angle %.4e shift %.4e sigma2 %.4e"
          % (angle, seed, cr.STATUS[o["status"]], o["iterations"], ea, es, o["sigma2"]))
    assert o["status"] == 0 and ea <= 7e-2 and es <= 2e-2
    tr = o["trace"][:o["iterations"] + 1]                                         # sigma2 falls; at the end it may rest within the tolerance
    assert np.isnan(o["trace"][o["iterations"] + 1:]).all() and (np.diff(tr) <= 1e-4 * tr[:-1]).all() and tr[-1] == o["sigma2"]
    closing = cr.expectation(src, tgt, o["sigma2"], o["R"], o["t"], o["scale"], 0.1)
    for k in ("Pt1", "P1", "PX"):
        assert cr.same_bits(closing[k], o[k]), k
    assert closing["Np"] == o["Np"]


@pytest.mark.parametrize("seed", (0, 1))
def test_the_restated_loop_collapses_on_an_exact_copy(seed):
    src, tgt, Rg, tg = cr.exact_copy(seed)
    o = cr.cpd(src, tgt, w=0.1, tolerance=1e-4, max_iterations=150, sigma2_floor=COPY_FLOOR)
    ea, es = angle_error(o["R"], Rg), cr.pose_error(o["R"], o["t"], Rg, tg)[1]
    print("restated exact copy seed %d: status %s iterations %d angle %.3e shift %.3e" % (seed, cr.STATUS[o["status"]], o["iterations"], ea, es))
    assert o["status"] == 2 and o["sigma2"] == COPY_FLOOR and ea <= 1e-5 and es <= 1e-5


def test_the_restated_loop_finds_a_scale():
    src, tgt, Rg, tg = cr.shrunk()
    o = cr.cpd(src, tgt, w=0.1, tolerance=1e-4, max_iterations=150, with_scaling=True)
    print("restated scale: status %s iterations %d scale %.5f" % (cr.STATUS[o["status"]], o["iterations"], o["scale"]))
    assert o["status"] == 0 and abs(o["scale"] - 1.3) <= 0.03


# ------------------------------------------------------------------------------------------------------------------ the refusals

def test_the_python_calls_refuse_before_any_launch():
    import vcrnet_amd
    from vcrnet_amd.native import VcrHipError
    tgt, src = torch.zeros(2, 3, 50), torch.zeros(2, 3, 40)
    R, t = torch.eye(3).repeat(2, 1, 1), torch.zeros(2, 3)
    nan, inf = float("nan"), float("inf")
    common = ((dict(src=torch.zeros(2, 40, 3)), "point cloud"), (dict(tgt=None), "point cloud"), (dict(src=src.double()), "float32"),
              (dict(tgt=tgt.double()), "float32"), (dict(src=torch.zeros(2, 3, 0)), "1 ..."), (dict(tgt=torch.zeros(3, 3, 50)), "same number"),
              (dict(R=R), "both R and t"), (dict(t=t), "both R and t"), (dict(R=R[:1], t=t), r"\[B, 3, 3\]"), (dict(R=R.double(), t=t), r"\[B, 3, 3\]"),
              (dict(w=-0.1), "w must"), (dict(w=1.0), "w must"), (dict(w=nan), "w must"), (dict(w=None), "w must"),
              (dict(sigma2=0.0), "sigma2"), (dict(sigma2=-1.0), "sigma2"), (dict(sigma2=nan), "sigma2"), (dict(sigma2=inf), "sigma2"),
              (dict(sigma2=torch.ones(2)), "float64 tensor"), (dict(sigma2=torch.ones(3, dtype=torch.float64)), "float64 tensor"),
              (dict(variant=7), "variant"), (dict(variant=-1), "variant"), (dict(variant=1.0), "variant"),
              (dict(), "HIP path only"), (dict(R=R, t=t), "HIP path only"))
    for kw, word in common + ((dict(scale=0.0), "scale"), (dict(scale=nan), "scale"), (dict(scale=torch.ones(2)), "float64 tensor")):
        a = dict(src=src, tgt=tgt, sigma2=0.5)
        a.update(kw)
        with pytest.raises(VcrHipError, match=word):
            vcrnet_amd.cpd_expectation(**a)
    with pytest.raises(TypeError):
        vcrnet_amd.cpd_expectation(src, tgt)                                      # sigma2 has no default
    for kw, word in common + ((dict(max_iterations=-1), "max_iterations"), (dict(max_iterations=2.5), "max_iterations"),
                              (dict(max_iterations=None), "max_iterations"), (dict(tolerance=-1.0), "tolerance"), (dict(tolerance=nan), "tolerance"),
                              (dict(sigma2_floor=0.0), "sigma2_floor"), (dict(sigma2_floor=-1.0), "sigma2_floor"), (dict(sigma2_floor=nan), "sigma2_floor")):
        a = dict(src=src, tgt=tgt)
        a.update(kw)
        with pytest.raises(VcrHipError, match=word):
            vcrnet_amd.coherent_point_drift(**a)
