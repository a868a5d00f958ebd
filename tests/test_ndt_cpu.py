"""include/ndt/vcr_hip_ndt.h without a GPU: the boundary -- the header as C and as C++, the prototypes,
the structs' layouts, the error codes, the host-only form and workspace queries, the build's lists, the kernels' resources --,
the numpy restatement (tests/ndt_restated.py) against an independent map, against differences of its own score and on the
recovery recipe, and what the three Python calls refuse."""
import ctypes
import math
import os
import subprocess

import numpy as np
import pytest
import torch

import boundary
import ndt_restated as nd

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INCLUDE = os.path.join(ROOT, "include")
HEADER = os.path.join(INCLUDE, "ndt", "vcr_hip_ndt.h")
LEDGER = os.path.join(ROOT, "profiles", "ndt_ledger.txt")
EINVAL, EWORKSPACE, EUNSUPPORTED = -1, -2, -3
ENTRY_POINTS = {"vcr_ndt_table_slots", "vcr_ndt_map_workspace_bytes", "vcr_ndt_map_f32", "vcr_ndt_map_form",
                "vcr_ndt_derivatives_workspace_bytes", "vcr_ndt_derivatives_f32", "vcr_ndt_derivatives_form",
                "vcr_ndt_workspace_bytes", "vcr_ndt_f32", "vcr_ndt_form"}
KERNELS = {"ndt_origin_kernel", "ndt_clear_kernel", "ndt_stats_kernel", "ndt_pose_kernel", "ndt_round_kernel", "ndt_sums_kernel",
           "ndt_step_kernel", "ndt_finish_kernel"}
F32 = np.float32


@pytest.fixture(scope="module")
def lib():
    import vcrnet_amd  # noqa: F401
    from vcrnet_amd import build, ndt
    build.build()
    return ndt.lib()


# ----------------------------------------------------------------------------------------------------------------- the boundary

@pytest.mark.parametrize("language,compiler", [("c", "gcc"), ("c++", "g++")])
def test_the_header_compiles_as_c_and_as_cpp(language, compiler, tmp_path):
    src = tmp_path / ("use." + ("c" if language == "c" else "cpp"))
    src.write_text('#include "ndt/vcr_hip_ndt.h"\n'
                   "int main(void) { vcr_ndt_map_args m; vcr_ndt_args a; m.struct_bytes = sizeof m; a.struct_bytes = sizeof a;\n"
                   "  return m.struct_bytes == a.struct_bytes; }\n")
    r = subprocess.run([compiler, "-x", language, "-Wall", "-Werror", "-pedantic", "-fsyntax-only", "-I", INCLUDE, str(src)],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr


def test_signatures_match_the_header_and_the_library_exports_them(lib):
    from vcrnet_amd import ndt
    boundary.check_signatures(HEADER, ndt, lib, ENTRY_POINTS)


def test_args_match_the_c_layout(tmp_path):
    import vcrnet_amd  # noqa: F401
    from vcrnet_amd import ndt
    boundary.check_layout(HEADER, ndt, tmp_path)
    text = open(HEADER).read()
    assert "#define VCR_NDT_VALUES %d" % ndt.VALUES in text and "#define VCR_NDT_STATE_BYTES %d" % ndt.STATE_BYTES in text
    for code, name in enumerate(("CONVERGED", "MAX_ITERATIONS", "MAX_TRIALS", "NO_HITS", "NOT_FINITE")):
        assert "#define VCR_NDT_%s %d" % (name, code) in text
    assert ndt.STATUS == nd.STATUS and len(ndt.STATUS) == 5 and nd.VALUES == ndt.VALUES


def test_the_call_lives_beside_the_other_headers_not_in_them(lib):
    """No other public header mentions it, the ABI version is where it was, and the header enters the digest of ndt.o alone;
    refine.METHODS does not know it: it is a function of its own."""
    from vcrnet_amd import build, native, ndt, refine, voxel_sort
    for d, _, files in os.walk(INCLUDE):
        for f in files:
            if os.path.join(d, f) != HEADER:
                assert "vcr_ndt" not in open(os.path.join(d, f)).read(), f
    assert lib.vcr_abi_version() == native.ABI_VERSION == 27
    for other in (native, voxel_sort):
        assert not set(ndt.SIGNATURES) & set(other.SIGNATURES) and not set(ndt.STRUCTS) & set(other.STRUCTS)
    assert not set(ndt.SIGNATURES) & set(native.PUBLIC)
    assert build.NDT_HEADERS == [HEADER] and build.OWN_HEADERS["ndt.hip"] is build.NDT_HEADERS
    assert [k for k, v in build.OWN_HEADERS.items() if HEADER in v] == ["ndt.hip"]
    assert not any("ndt" in m for m in refine.METHODS)
    import vcrnet_amd
    for name in ("ndt_map", "ndt_derivatives", "refine_registration_ndt"):
        assert name in vcrnet_amd.__all__ and getattr(vcrnet_amd, name) is getattr(ndt, name)


def _map(**kw):
    from vcrnet_amd import ndt
    a = ndt.NdtMapArgs()
    v = dict(tgt=0x1000, B=2, Nt=900, resolution=0.3, min_points=6, min_eig_ratio=0.01, mean=0x2000, inv_cov=0x3000, valid=0x4000,
             count=0x5000, voxel_points=0x6000, origin=0x7000, table_keys=0x8000, table_vals=0x9000)   # (never dereferenced)
    v.update(kw)
    for k, x in v.items():
        setattr(a, k, x)
    return a


def _args(loop, **kw):
    from vcrnet_amd import ndt
    a = ndt.NdtArgs()
    v = dict(src=0x1000, Ns=1000, neighbors=7, d1=-3.0, d2=0.5, score=0x2000, hits=0x3000, g=0x4000, H=0x5000)
    if loop:
        v.update(max_iterations=30, max_trials=120, rot_epsilon=1e-6, trans_epsilon=1e-6, R_out=0x6000, t_out=0x7000)
    v.update(kw)
    for k, x in v.items():
        setattr(a, k, x)
    return a


def test_argument_errors_return_their_codes_without_a_gpu(lib):
    from vcrnet_amd import ndt

    def map_codes(m):
        rc = lib.vcr_ndt_map_f32(ctypes.byref(m), 0x10000, 1 << 40, None)
        assert lib.vcr_ndt_map_workspace_bytes(ctypes.byref(m), 256) == 0
        assert lib.vcr_ndt_map_form(ctypes.byref(m), 256, None, None) == rc
        return rc

    def codes(m, a, loop):
        entry = "vcr_ndt" if loop else "vcr_ndt_derivatives"
        rc = getattr(lib, entry + "_f32")(ctypes.byref(m), ctypes.byref(a), 0x10000, 1 << 40, None)
        assert getattr(lib, entry + "_workspace_bytes")(ctypes.byref(m), ctypes.byref(a), 256) == 0
        assert getattr(lib, entry + "_form")(ctypes.byref(m), ctypes.byref(a), 256, None, None, None) == rc
        return rc
    assert lib.vcr_ndt_map_f32(None, None, 0, None) == EINVAL and lib.vcr_ndt_map_workspace_bytes(None, 256) == 0
    assert lib.vcr_ndt_f32(None, None, None, 0, None) == EINVAL and lib.vcr_ndt_derivatives_f32(ctypes.byref(_map()), None, None, 0, None) == EINVAL
    nan, inf = float("nan"), float("inf")
    for field in ("tgt", "mean", "inv_cov", "valid", "count", "voxel_points", "origin", "table_keys", "table_vals"):
        assert map_codes(_map(**{field: None})) == EINVAL, field
    for kw in (dict(B=0), dict(Nt=0), dict(B=-1), dict(resolution=0.0), dict(resolution=-1.0), dict(resolution=nan), dict(resolution=inf),
               dict(min_points=2), dict(min_points=0), dict(min_eig_ratio=0.0), dict(min_eig_ratio=1.5), dict(min_eig_ratio=nan)):
        assert map_codes(_map(**kw)) == EINVAL, kw
    for kw in (dict(Nt=131073), dict(B=16384, Nt=131072)):
        assert map_codes(_map(**kw)) == EUNSUPPORTED, kw
    for bad in (0, ctypes.sizeof(ndt.NdtMapArgs) - 8, ctypes.sizeof(ndt.NdtMapArgs) + 8):      # every field is mandatory
        m = _map()
        m.struct_bytes = bad
        assert map_codes(m) == EINVAL, bad
    for loop in (False, True):
        for field in ("src",) + (("R_out", "t_out") if loop else ("score", "hits", "g", "H")):
            assert codes(_map(), _args(loop, **{field: None}), loop) == EINVAL, field
        for kw in (dict(Ns=0), dict(neighbors=0), dict(neighbors=6), dict(neighbors=27), dict(d1=nan), dict(d2=nan), dict(d2=inf),
                   dict(d2=0.0), dict(d2=-1.0), dict(R=0x100), dict(t=0x100), dict(variant=2), dict(variant=-1)):
            assert codes(_map(), _args(loop, **kw), loop) == EINVAL, kw
        assert codes(_map(), _args(loop, Ns=131073), loop) == EUNSUPPORTED
        assert codes(_map(B=16384), _args(loop, Ns=131072), loop) == EUNSUPPORTED
        assert codes(_map(mean=None), _args(loop), loop) == EINVAL            # the map's fields are read ...
        m = _map(tgt=None, voxel_points=None, min_points=0, min_eig_ratio=0.0)  # ... but not what only the build needs
        a = _args(loop)
        assert getattr(lib, "vcr_ndt_workspace_bytes" if loop else "vcr_ndt_derivatives_workspace_bytes")(ctypes.byref(m), ctypes.byref(a), 256) > 0
        for bad in (0, ndt.NdtArgs.max_iterations.offset - 8, ctypes.sizeof(ndt.NdtArgs) + 8):
            a = _args(loop)
            a.struct_bytes = bad
            assert codes(_map(), a, loop) == EINVAL, bad
    for kw in (dict(max_iterations=-1), dict(max_trials=-1), dict(rot_epsilon=-1.0), dict(rot_epsilon=nan), dict(trans_epsilon=-1.0),
               dict(trans_epsilon=nan)):
        assert codes(_map(), _args(True, **kw), True) == EINVAL, kw
    # the derivative call ignores what follows H: its mandatory part alone is served
    a = _args(False)
    a.struct_bytes = ndt.NdtArgs.max_iterations.offset
    assert lib.vcr_ndt_derivatives_workspace_bytes(ctypes.byref(_map()), ctypes.byref(a), 256) > 0
    assert ndt.NdtArgs.max_iterations.offset == ndt.NdtArgs.H.offset + 8


def test_the_forms_and_the_workspaces_are_host_only_queries(lib):
    from vcrnet_amd import ndt, voxel_sort
    up = lambda v: (v + 255) & ~255                                               # noqa: E731
    for Nt, slots in ((1, 4), (2, 8), (3, 8), (7, 16), (8, 32), (1000, 2048), (1023, 2048), (1024, 4096), (131072, 1 << 19)):
        assert ndt.table_slots(Nt) == slots == 1 << math.ceil(math.log2(2 * Nt + 2)), Nt
    assert ndt.table_slots(0) == 0 and ndt.table_slots(131073) == 0
    for B, Nt, cu in ((1, 1, 256), (2, 900, 256), (3, 5000, 104), (1, 131072, 1), (16, 16384, 256)):
        lanes, slots, ws = ndt.map_form(B, Nt, cu_count=cu)
        assert (lanes, slots) == (1, ndt.table_slots(Nt))
        assert ws == up(12 * B * Nt) + 2 * up(4 * B * Nt) + voxel_sort.voxel_sort_form(B, Nt, cu_count=cu)[3]
    for B, Ns, Nt in ((1, 1, 5), (2, 1000, 900), (3, 257, 5000), (1, 131072, 131072), (16, 16384, 1024)):
        nblk = -(-Ns // 256)
        want = up(ndt.STATE_BYTES * B) + up(8 * ndt.VALUES * B * nblk)
        assert ndt.ndt_form(B, Ns, Nt, loop=False) == (1, nblk, 3, want)
        assert ndt.ndt_form(B, Ns, Nt, loop=False, variant=1, neighbors=1, cu_count=1) == (1, nblk, 3, want)
        assert ndt.ndt_form(B, Ns, Nt, max_iterations=30) == (1, nblk, 2 * 121 + 2, want)
        assert ndt.ndt_form(B, Ns, Nt, max_iterations=5, max_trials=7) == (1, nblk, 2 * 8 + 2, want)
        assert ndt.ndt_form(B, Ns, Nt, max_iterations=0) == (1, nblk, 4, want)
    m, a = _map(), _args(True)
    ws = lib.vcr_ndt_workspace_bytes(ctypes.byref(m), ctypes.byref(a), 256)
    assert ws > 0 and lib.vcr_ndt_workspace_bytes(ctypes.byref(m), ctypes.byref(a), -1) == 0
    assert lib.vcr_ndt_f32(ctypes.byref(m), ctypes.byref(a), None, ws, None) == EINVAL
    assert lib.vcr_ndt_f32(ctypes.byref(m), ctypes.byref(a), 0x10008, ws, None) == EINVAL
    assert lib.vcr_ndt_f32(ctypes.byref(m), ctypes.byref(a), 0x10000, ws - 1, None) == EWORKSPACE
    assert lib.vcr_ndt_derivatives_f32(ctypes.byref(m), ctypes.byref(_args(False)), 0x10000, ws - 1, None) == EWORKSPACE
    mws = lib.vcr_ndt_map_workspace_bytes(ctypes.byref(m), 256)
    assert lib.vcr_ndt_map_f32(ctypes.byref(m), 0x10000, mws - 1, None) == EWORKSPACE
    assert lib.vcr_ndt_map_f32(ctypes.byref(m), 0x10008, mws, None) == EINVAL


def test_the_new_kernels_use_no_scratch():
    import vcrnet_amd  # noqa: F401
    from vcrnet_amd import build
    build.build()
    res = build.kernel_resources()
    names = list(res)
    dem = subprocess.run(["c++filt"], input="\n".join(names), capture_output=True, text=True, check=True).stdout.splitlines()
    mine = {d.replace("(anonymous namespace)::", "").replace("void ", "").split("(")[0]: res[n]
            for n, d in zip(names, dem) if res[n]["file"] == "ndt.hip"}
    assert set(mine) == KERNELS
    for d, v in mine.items():
        print(d, v)
        assert v.get("scratch", 0) == 0 and v.get("vgpr_spill", 0) == 0, (d, v)
    # the round: 29 fp64 accumulators and a voxel's terms in registers, four waves' partials in LDS
    assert mine["ndt_round_kernel"]["lds"] == 4 * 29 * 8 and mine["ndt_round_kernel"]["occupancy"] >= 2


# ------------------------------------------------------------------------------------------------------------- the restatement

def cloud(seed, n, lo=-1.0, hi=1.0):
    return np.random.RandomState(seed).uniform(lo, hi, size=(3, n)).astype(F32)


MAP_RTOL = 1e-12    # 2^-52 times the condition 1 / min_eig_ratio = 100 of the floored inverse times some forty operations


def test_the_restated_map_is_the_two_pass_mean_covariance_and_floored_inverse():
    """Against a plain computation: members by a dict, np.mean, np.cov, eigh, the floor, the inverse.  The Jacobi and eigh differ in
    rounding only: the largest relative difference of an inverse covariance here was 5.5e-15 of its largest entry."""
    worst = 0.0
    for seed, n, h in ((1, 700, 0.5), (2, 3000, 0.4), (3, 500, 10.0)):
        x = cloud(seed, n)
        m = nd.ndt_map(x, h)
        x64 = x.astype(np.float64)
        cells = {}
        for i in range(n):
            cells.setdefault(tuple(np.floor((x64[:, i] - m["origin"]) / m["h"]).astype(int)), []).append(i)
        assert int(m["count"]) == len(cells) and set(m["lookup"]) == set(cells)
        assert not np.isfinite(m["mean"][:, len(cells):]).any() and not m["valid"][len(cells):].any()
        for cell, mem in cells.items():
            v = m["lookup"][cell]
            assert m["voxel_points"][v] == len(mem)
            assert np.allclose(m["mean"][:, v], x64[:, mem].mean(axis=1), rtol=0, atol=1e-15)
            if len(mem) < 6:
                assert not m["valid"][v] and np.isnan(m["inv_cov"][:, v]).all()
                continue
            l, V = np.linalg.eigh(np.cov(x64[:, mem]))
            A = (V / np.maximum(l, 0.01 * l.max())) @ V.T
            got = nd.full(m["inv_cov"][:, v])
            assert m["valid"][v]
            worst = max(worst, np.abs(got - A).max() / np.abs(A).max())
    print("largest relative difference of an inverse covariance: %.3g" % worst)
    assert worst < MAP_RTOL


def test_the_restated_map_refuses_what_the_header_calls_invalid():
    rs = np.random.RandomState(4)
    x = np.concatenate([np.repeat(rs.uniform(0, 0.1, (3, 1)), 8, axis=1),             # eight copies of a point: C is all zero
                        np.stack([rs.uniform(1.0, 1.2, 9), rs.uniform(1.0, 1.2, 9), np.full(9, 1.1)]),      # a planar voxel
                        rs.uniform(2.0, 2.2, (3, 5)), rs.uniform(3.0, 3.2, (3, 6))], axis=1).astype(F32)   # five and six points
    m = nd.ndt_map(x, 0.5)
    assert int(m["count"]) == 4 and list(m["voxel_points"][:4]) == [8, 9, 5, 6] and list(m["valid"][:4]) == [0, 1, 0, 1]
    l = np.linalg.eigvalsh(nd.full(m["inv_cov"][:, 1]))
    assert abs(l.max() / l.min() - 100.0) < 1e-6                                      # the floor acted: 1 / 0.01
    assert int(nd.ndt_map(np.full((3, 10), np.nan, F32), 0.5)["count"]) == 0
    assert int(nd.ndt_map(np.array([[0.0, 3000.0]] * 3, F32), 2.0 ** -10)["count"]) == -1          # too fine
    assert list(nd.ndt_map(x, 0.5, min_points=5)["valid"][:4]) == [0, 1, 1, 1]


def scene(seed=5, nt=900, ns=300, h=0.4):
    tgt = nd.torus(seed, nt, noise=0.01)
    src = nd.torus(seed + 1, ns, noise=0.01)
    m = nd.ndt_map(tgt, h)
    R, t = nd.pose(0.03, 0.02, seed)
    return src, m, R, t


def moved_by(x, P):
    Ri, ti = nd.euler(x)
    return Ri @ P + ti[:, None]


def test_the_restated_gradient_is_the_central_difference_of_the_restated_score():
    src, m, R, t = scene()
    _, d2 = nd.constants(0.55, m["h"])
    P = R @ src.astype(np.float64) + t[:, None]
    base = nd.derivatives_at(P, m, d2)
    assert base["hits"] > 200
    eps = 1e-6
    for a in range(6):
        x = np.zeros(6)
        x[a] = eps
        fd = (nd.derivatives_at(moved_by(x, P), m, d2, voxel=base["voxel"])["f"] - nd.derivatives_at(moved_by(-x, P), m, d2, voxel=base["voxel"])["f"]) / (2 * eps)
        # the difference's own error: f's rounding (2^-52 |f| hits) over eps, and eps^2 times a third derivative of H's size
        bound = 1e-6 * np.abs(base["g"]).max() + 1e-5
        print(a, base["g"][a], fd)
        assert abs(fd - base["g"][a]) < bound, (a, fd, base["g"][a])


def test_the_restated_hessian_is_the_second_difference_with_the_voxels_frozen():
    """f jumps where a point changes its cell, so the differences keep every point in the voxels of the base pose.  euler(x) is
    Rz Ry Rx, so two coordinates set together ARE the chart's mixed point.  The S_ab term (the chart's second derivative) is
    judged here: the header's formula passes unchanged.  The bound: the step 1e-5 leaves the four scores' rounding,
    4 hits 2^-52 / (4 step^2) < 1e-2 absolute, and a truncation of step^2 times f's fourth derivative, which is the second's size
    times (d2 / the smallest eigenvalue)^2 < 1e5 here: 1e-5 of the largest entry covers both."""
    src, m, R, t = scene()
    _, d2 = nd.constants(0.55, m["h"])
    P = R @ src.astype(np.float64) + t[:, None]
    base = nd.derivatives_at(P, m, d2)
    H = nd.full(base["H"])
    step = 1e-5
    f = lambda u: nd.derivatives_at(moved_by(u, P), m, d2, voxel=base["voxel"])["f"]      # noqa: E731
    worst = 0.0
    for a in range(6):
        u = np.zeros(6)
        u[a] = step
        for b in range(a, 6):
            w = np.zeros(6)
            w[b] = step
            if a == b:
                fd = (f(u) - 2 * base["f"] + f(-u)) / (step * step)
            else:
                fd = (f(u + w) - f(u - w) - f(-u + w) + f(-u - w)) / (4 * step * step)
            worst = max(worst, abs(fd - H[a, b]) / np.abs(H).max())
            assert abs(fd - H[a, b]) < 1e-5 * np.abs(H).max() + 1e-2, (a, b, fd, H[a, b])
    print("largest |difference - H| / max|H|: %.3g" % worst)


def test_one_neighbour_and_seven_agree_inside_one_voxel():
    """A target in one voxel: the six face neighbours are empty, so DIRECT1 and DIRECT7 read the same voxel and add the same bits."""
    tgt = cloud(6, 200, 0.1, 0.9)
    src = cloud(7, 120, 0.2, 0.8)
    m = nd.ndt_map(tgt, 5.0)
    assert int(m["count"]) == 1 and m["valid"][0]
    one, seven = nd.derivatives(src, m, neighbors=1), nd.derivatives(src, m, neighbors=7)
    assert one["hits"] == seven["hits"] == 120
    assert nd.same_bits(one["values"], seven["values"])
    assert (seven["voxel"][:, 1:] == -1).all() and (seven["voxel"][:, 0] == 0).all()


def test_the_sum_order_is_the_refinements():
    """reduce_points against the order spelled out for one workgroup and a tail: lanes l and l ^ o, waves, partials."""
    rs = np.random.RandomState(8)
    vals = rs.standard_normal((nd.VALUES, 300)) * 10.0 ** rs.randint(-8, 8, size=(nd.VALUES, 300))
    got = nd.reduce_points(vals)
    pad = np.zeros((nd.VALUES, 512))
    pad[:, :300] = vals
    for e in (0, 7, 28):
        parts = []
        for blk in range(2):
            waves = []
            for w in range(4):
                v = list(pad[e, blk * 256 + w * 64: blk * 256 + (w + 1) * 64])
                for o in (32, 16, 8, 4, 2, 1):
                    v = [v[l] + v[l ^ o] for l in range(64)]
                waves.append(v[0])
            parts.append(((waves[0] + waves[1]) + waves[2]) + waves[3])
        assert got[e] == (0.0 + parts[0]) + parts[1]


def ledger_figures():
    """{case: (angle, shift)} of the restated loop on the recovery recipe, as profiles/ndt_ledger.txt records them."""
    out = {}
    for ln in open(LEDGER):
        if ln.startswith("restated recovery"):
            w = ln.split()
            out[int(w[2])] = (float(w[w.index("angle") + 1]), float(w[w.index("shift") + 1]))
    return out


def test_the_restated_loop_recovers_the_pose_and_the_ledger_records_it():
    """700 target and 500 source torus points at h = 0.3 from (0.05 rad, 0.03) and (0.2 rad, 0.1): the restated loop ends closer
    than it started, its accepted scores fall strictly, and its errors are the figures the ledger records -- the GPU loop's
    allowance is 1.5 times them (tests/test_hip_ndt.py)."""
    figures = ledger_figures()
    for i, (angle, shift) in enumerate(nd.RECOVERY):
        src, tgt, R0, t0, Rg, tg = nd.recovery_case(i)
        m = nd.ndt_map(tgt, nd.RECOVERY_H)
        o = nd.ndt(src, m, R0, t0)
        ea, es = nd.pose_error(o["R"], o["t"], Rg, tg)
        print("restated recovery %d from angle %g shift %g: iterations %d trials %d status %s angle %.6e shift %.6e"
              % (i, angle, shift, o["iterations"], o["trials"], nd.STATUS[o["status"]], ea, es))
        assert ea < angle / 2 and es < shift / 2
        acc = o["trace"][np.isfinite(o["trace"])]
        assert len(acc) == o["iterations"] + 1 and (np.diff(acc) < 0).all()
        closing = nd.derivatives(src, m, o["R"], o["t"])
        assert nd.same_bits(closing["values"], np.concatenate([[o["score"], float(o["hits"])], o["g"], o["H"]]))
        assert abs(figures[i][0] - ea) <= 1e-6 * max(ea, 1e-12) + 1e-12 and abs(figures[i][1] - es) <= 1e-6 * max(es, 1e-12) + 1e-12


# ------------------------------------------------------------------------------------------------------------------ the refusals

def test_the_python_calls_refuse_before_any_launch():
    import vcrnet_amd
    from vcrnet_amd.native import VcrHipError
    tgt, src = torch.zeros(2, 3, 50), torch.zeros(2, 3, 40)
    R, t = torch.eye(3).repeat(2, 1, 1), torch.zeros(2, 3)
    nan = float("nan")
    for kw, word in ((dict(tgt=torch.zeros(2, 50, 3)), "point cloud"), (dict(tgt=tgt.double()), "float32"), (dict(tgt=None), "point cloud"),
                     (dict(tgt=torch.zeros(2, 3, 0)), "1 ..."), (dict(resolution=None), "no default"), (dict(resolution=0.0), "resolution"),
                     (dict(resolution=nan), "resolution"), (dict(resolution=-1.0), "resolution"), (dict(min_points=2), "min_points"),
                     (dict(min_points=6.0), "min_points"), (dict(min_eig_ratio=0.0), "min_eig_ratio"), (dict(min_eig_ratio=2.0), "min_eig_ratio"),
                     (dict(), "HIP path only")):
        a = dict(tgt=tgt, resolution=0.5)
        a.update(kw)
        with pytest.raises(VcrHipError, match=word):
            vcrnet_amd.ndt_map(**a)
    for kw, word in ((dict(src=torch.zeros(2, 40, 3)), "point cloud"), (dict(src=src.double()), "float32"), (dict(src=torch.zeros(3, 3, 40)), "same number"),
                     (dict(src=torch.zeros(2, 3, 0)), "1 ..."), (dict(R=R), "both R and t"), (dict(t=t), "both R and t"),
                     (dict(R=R[:1], t=t), r"\[B, 3, 3\]"), (dict(R=R.double(), t=t), r"\[B, 3, 3\]"), (dict(neighbors=6), "neighbors"),
                     (dict(neighbors=27), "neighbors"), (dict(outlier_ratio=0.0), "outlier_ratio"), (dict(outlier_ratio=1.0), "outlier_ratio"),
                     (dict(outlier_ratio=nan), "outlier_ratio"), (dict(resolution=None), "no default"), (dict(resolution=-1.0), "resolution"),
                     (dict(map_or_tgt=torch.zeros(2, 50, 3)), "point cloud"), (dict(variant=2), "variant"), (dict(), "HIP path only"),
                     (dict(R=R, t=t), "HIP path only")):
        a = dict(src=src, map_or_tgt=tgt, resolution=0.5)
        a.update(kw)
        with pytest.raises(VcrHipError, match=word):
            vcrnet_amd.ndt_derivatives(**a)
    for kw, word in ((dict(resolution=None), "no default"), (dict(resolution=0.0), "resolution"), (dict(src=src[:1]), "same number"),
                     (dict(tgt=tgt.double()), "float32"), (dict(neighbors=2), "neighbors"), (dict(max_iterations=-1), "max_iterations"),
                     (dict(max_iterations=2.5), "max_iterations"), (dict(max_iterations=None), "max_iterations"), (dict(max_trials=-1), "max_trials"),
                     (dict(rot_epsilon=-1.0), "epsilon"), (dict(trans_epsilon=nan), "epsilon"), (dict(map=tgt), "NdtMap"),
                     (dict(min_points=1), "min_points"), (dict(outlier_ratio=1.5), "outlier_ratio"), (dict(R=R), "both R and t"),
                     (dict(variant=7), "variant"), (dict(), "HIP path only"), (dict(R=R, t=t), "HIP path only")):
        a = dict(src=src, tgt=tgt, resolution=0.5)
        a.update(kw)
        with pytest.raises(VcrHipError, match=word):
            vcrnet_amd.refine_registration_ndt(**a)


def test_a_map_on_the_host_is_refused_and_its_resolution_is_the_maps():
    import vcrnet_amd
    from vcrnet_amd import ndt
    from vcrnet_amd.native import VcrHipError
    B, Nt = 2, 50
    T = ndt.table_slots(Nt)
    m = ndt.NdtMap(0.5, 6, 0.01, mean=torch.zeros(B, 3, Nt, dtype=torch.float64), inv_cov=torch.zeros(B, 6, Nt, dtype=torch.float64),
                   valid=torch.zeros(B, Nt, dtype=torch.int32), count=torch.zeros(B, dtype=torch.int32),
                   voxel_points=torch.zeros(B, Nt, dtype=torch.int32), origin=torch.zeros(B, 3, dtype=torch.float64),
                   table_keys=torch.zeros(B, T, dtype=torch.int64), table_vals=torch.zeros(B, T, dtype=torch.int32))
    assert (m.B, m.Nt) == (B, Nt)
    src = torch.zeros(B, 3, 40)
    with pytest.raises(VcrHipError, match="HIP path only"):
        vcrnet_amd.ndt_derivatives(src, m)
    with pytest.raises(VcrHipError, match="HIP path only"):
        vcrnet_amd.refine_registration_ndt(src, None, map=m)
    with pytest.raises(VcrHipError, match="not the map's"):
        vcrnet_amd.refine_registration_ndt(src, None, map=m, resolution=0.25)
    with pytest.raises(VcrHipError, match="same number"):
        vcrnet_amd.ndt_derivatives(src[:1], m)
    d1, d2 = ndt.constants(0.55, 0.3)
    assert (d1, d2) == nd.constants(0.55, 0.3) and d2 > 0 and math.isfinite(d1)
