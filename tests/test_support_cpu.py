"""Normals and FPFH at centres over a support cloud without a GPU: the numpy restatement (tests/support_restated.py) against
rows_restated where the centres are the cloud's own points, on a cloud worked by hand, and the conditions the GPU test's recipe
must meet; the boundary of include/support/vcr_hip_support.h (prototypes against vcrnet_amd.support.SIGNATURES, the structs
against gcc's layout, the header rules of the other families), every argument error of the four calls and of the Python
functions, the host-only form and plan queries, and the resource remarks of support.hip."""
import ctypes
import inspect
import os
import subprocess

import numpy as np
import pytest
import torch

import boundary
import fpfh_restated as fr
import query_restated as qr
import radius_restated as rr
import rows_restated as wr
import support_restated as sr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INCLUDE = os.path.join(ROOT, "include")
HEADER = os.path.join(INCLUDE, "support", "vcr_hip_support.h")
EINVAL, EWORKSPACE, EUNSUPPORTED = -1, -2, -3
ENTRY_POINTS = {"vcr_support_normals_f32", "vcr_support_spfh_f32", "vcr_support_needed_f32", "vcr_support_needed_workspace_bytes",
                "vcr_support_fpfh_f32", "vcr_support_form"}
KERNELS = {"support_normals_kernel", "support_spfh_lane_kernel", "support_spfh_wave_kernel", "support_zero_kernel",
           "support_mark_kernel", "support_slot_kernel", "support_fpfh_kernel"}
# the other families' call names: no header may carry them outside its own family, comments included
REFUSED = ("vcr_query", "VCR_QUERY", "_iss_", "vcr_spfh", "vcr_fpfh", "vcr_rows_", "VCR_ROWS", "vcr_normals", "vcr_refine_plane",
           "vcr_feat_nn", "vcr_ransac", "vcr_grid_radius", "VCR_RADIUS", "gridnn", "vcr_grid_nn", "_grid_f32", "dbscan", "vcr_cluster_",
           "vcr_plane_ransac", "vcr_plane_split", "orient_tangent")
I32 = np.int32


@pytest.fixture(scope="module")
def lib():
    import vcrnet_amd  # noqa: F401
    from vcrnet_amd import build, support
    build.build()
    return support.lib()


def bits(a):
    return np.ascontiguousarray(a).view(I32)


# ------------------------------------------------------------------------------------------------------------- the restatement

@pytest.mark.parametrize("radius", wr.RAGGED_RADII[:2])
def test_centres_that_are_the_points_return_rows_restated(radius):
    """Centres = the points, self = arange, rows = the self rows with i inserted at the head: normals, curvature, spfh and fpfh
    are rows_restated's, bit for bit, for max_nn in (0, 1, 2, 5)."""
    x = fr.cloud(*wr.RAGGED)[0]
    N = x.shape[1]
    got = rr.radius_rows(x, radius)
    idx, rs = got["idx"], got["row_start"]
    idx2, rs2 = sr.with_self_at_head(idx, rs)
    me = np.arange(N)
    for max_nn in (0, 1, 2, 5):
        n0, c0, _, _ = wr.normals(x, idx, rs, max_nn)
        n1, c1 = sr.normals(x, x, idx2, rs2, me, max_nn)
        assert np.array_equal(bits(n0), bits(n1)) and np.array_equal(bits(c0), bits(c1)), (radius, max_nn)
        sp0 = wr.spfh(x, n0, idx, rs, max_nn)
        sp1 = sr.spfh(x, n0, x, n0, idx2, rs2, me, max_nn)
        assert np.array_equal(sp0, sp1), (radius, max_nn)
        f0 = wr.fpfh(x, idx, rs, sp0, max_nn)
        f1 = sr.fpfh(x, x, idx2, rs2, sp0, sp1, me, None, max_nn)
        assert np.array_equal(bits(f0), bits(f1)), (radius, max_nn)
        whole, nq, mine = sr.feature(x, None, x, (idx2, rs2), (idx, rs), me, None, max_nn)
        assert np.array_equal(bits(whole), bits(f0)) and np.array_equal(bits(nq), bits(n0)) and np.array_equal(mine, sp0)
        need = sr.needed(x, x, idx2, rs2, me, max_nn)
        lens = wr.lengths(rs, max_nn)
        want = np.zeros(N, bool)
        for i in range(N):
            want[idx[rs[i]:rs[i] + lens[i]]] = True
        assert need["count"] == want.sum() and np.array_equal(need["index"][:need["count"]], np.flatnonzero(want))


def hand():
    """Seven support points (5 is a copy of 0; 6 lies in a NaN centre's row alone) and seven centres."""
    x = np.asarray([[0, 0, 0], [1, 0, 0], [0, 1, 0], [0, 0, 1], [1, 1, 0], [0, 0, 0], [5, 5, 5]], np.float32).T.copy()
    nrm = np.tile(np.asarray([[0], [0], [1]], np.float32), (1, 7))
    nan = np.nan
    c = np.asarray([[0, 0, 0],            # 0: IS point 0; its row holds itself, -1, 99 and the copy 5
                    [0, 0, 0],            # 1: a copy of point 0 WITHOUT a self index
                    [9, 9, 9],            # 2: an empty row
                    [1, 1, 1],            # 3: a row of one
                    [0, 1, 0],            # 4: IS point 2; its self entry stands behind the second neighbour entry
                    [nan, 0, 0],          # 5: not finite
                    [0.5, 0.5, 0]], np.float32).T.copy()   # 6: four points of the plane z = 0
    rows = [[0, 1, 2, 3, -1, 99, 5], [0, 1], [], [4], [1, 3, 2, 4], [1, 6], [0, 1, 2, 4]]
    idx = np.asarray([e for r in rows for e in r], np.int64)
    rs = np.concatenate([[0], np.cumsum([len(r) for r in rows])]).astype(np.int64)
    me = np.asarray([0, -1, -1, -1, 2, -1, -1], np.int32)
    return x, nrm, c, idx, rs, me


def test_a_cloud_worked_by_hand():
    x, nrm, c, idx, rs, me = hand()
    N = 7
    u = sr.used(idx, rs, N, me, 0)
    assert [e.tolist() for e, _ in u] == [[0, 1, 2, 3, 5], [0, 1], [], [4], [1, 3, 2, 4], [1, 6], [0, 1, 2, 4]]   # -1 and 99: nothing
    assert [o.tolist() for _, o in u] == [[True, False, False, False, False], [False, False], [], [False],
                                          [False, False, True, False], [False, False], [False] * 4]
    u2 = sr.used(idx, rs, N, me, 2)
    assert [e.tolist() for e, _ in u2] == [[0, 1, 2], [0, 1], [], [4], [1, 3], [1, 6], [0, 1]]   # 4: the self entry behind the cut
    assert [e.tolist() for e, _ in sr.used(idx, rs, N, None, 2)] == [[0, 1], [0, 1], [], [4], [1, 3], [1, 6], [0, 1]]
    # normals: m < 3 is (0, 0, 1), curvature 0; four points of z = 0 give exactly that as well; the NaN centre NaN
    n, cv = sr.normals(x, c, idx, rs, me, 0)
    for i in (1, 2, 3, 6):
        assert n[:, i].tolist() == [0, 0, 1] and cv[i] == 0, i
    assert np.isnan(n[:, 5]).all() and np.isnan(cv[5])
    assert np.isfinite(n[:, [0, 4]]).all() and np.allclose(np.linalg.norm(n[:, [0, 4]].astype(np.float64), axis=0), 1, atol=1e-6)
    n2, cv2 = sr.normals(x, c, idx, rs, me, 2)
    assert n2[:, 4].tolist() == [0, 0, 1] and cv2[4] == 0            # (two used entries: the self entry was not reached)
    # ... and centre 0's used entries (0, 1, 2) with its self entry are three points: the plane z = 0 again
    assert n2[:, 0].tolist() == [0, 0, 1] and cv2[0] == 0
    # the first pass: the copy is counted where it is not the self entry -- bins 5, 5, 5
    sp = sr.spfh(x, nrm, c, nrm[:, :7], idx, rs, me, 0)
    assert sp[:, :, 11].tolist() == [[4] * 3, [2] * 3, [0] * 3, [1] * 3, [3] * 3, [0] * 3, [4] * 3]
    only_copy = sr.spfh(x, nrm, c, nrm[:, :7], np.asarray([0, 5]), np.asarray([0, 2] + [2] * 6), me, 0)[0]
    assert only_copy[:, 11].tolist() == [1, 1, 1] and only_copy[:, 5].tolist() == [1, 1, 1] and only_copy[:, :11].sum() == 3
    assert sr.spfh(x, nrm, c, nrm[:, :7], np.asarray([0, 5]), np.asarray([0, 2] + [2] * 6), None, 0)[0][:, 11].tolist() == [2, 2, 2]
    assert not sp[5].any() and not sp[2].any()
    assert sr.spfh(x, nrm, c, nrm[:, :7], idx, rs, me, 2)[:, 0, 11].tolist() == [2, 2, 0, 1, 2, 0, 2]
    # needed: 6 is in the NaN centre's row alone; under the cut 5 is not reached either
    need = sr.needed(x, c, idx, rs, me, 0)
    assert need["count"] == 6 and need["index"].tolist() == [0, 1, 2, 3, 4, 5, -1] and need["slot"].tolist() == [0, 1, 2, 3, 4, 5, -1]
    assert np.array_equal(need["points"][:, :6], x[:, :6]) and np.isnan(need["points"][:, 6]).all()
    need2 = sr.needed(x, c, idx, rs, me, 2)
    assert need2["count"] == 5 and need2["slot"].tolist() == [0, 1, 2, 3, 4, -1, -1] and need2["index"].tolist() == [0, 1, 2, 3, 4, -1, -1]
    # the second pass on made-up histograms (point j: c = 2, one count in bin g of group g and one in bin 3 + j)
    h = np.zeros((N, 3, 12), np.int64)
    for g in range(3):
        h[:, g, g], h[:, g, 11] = 1, 2
        h[np.arange(N), g, 3 + np.arange(N)] = 1
    f = sr.fpfh(x, c, idx, rs, h, sp, me, None, 0)
    assert np.isnan(f[:, 5]).all() and not f[:, 2].any()             # the NaN centre; an empty row with c_i = 0
    for i in (0, 1, 3, 4, 6):                                        # neighbours and an own term: each group sums to 200
        assert np.allclose(f[:, i].reshape(3, 11).sum(1), 200, atol=1e-4), i
    # the copy of the centre is skipped at d2 == 0: centre 1's row (0, 1) is point 1 alone
    alone = sr.fpfh(x, c, np.asarray([1]), np.asarray([0, 0, 1, 1, 1, 1, 1, 1]), h, sp, None, None, 0)
    assert np.array_equal(bits(f[:, 1]), bits(alone[:, 1]))
    # a slot of -1 is a neighbour skipped: the same as a histogram row with c == 0
    slot = np.arange(N)
    slot[3] = -1
    h0 = h.copy()
    h0[3] = 0
    a, b = sr.fpfh(x, c, idx, rs, h, sp, me, slot, 0), sr.fpfh(x, c, idx, rs, h0, sp, me, None, 0)
    assert np.array_equal(bits(a), bits(b)) and not np.array_equal(bits(a[:, 0]), bits(f[:, 0]))
    assert np.array_equal(bits(a[:, 6]), bits(f[:, 6]))                # (point 3 is not in centre 6's row)
    short = sr.fpfh(x, c, idx, rs, h[:3], sp, me, None, 0)             # R = 3: the slots 3 .. 6 are outside [0, R)
    h3 = h.copy()
    h3[3:] = 0
    assert np.array_equal(bits(short), bits(sr.fpfh(x, c, idx, rs, h3, sp, me, None, 0)))


def test_the_recipe_meets_its_conditions():
    """Conditions, not measurements: every radius yields the row lengths it is there for, on both sides of the form threshold; no
    counted pair of any case the GPU test compares with the restatement lies within 2^-30 of an atan2 bin edge (the cap is 0);
    the jittered centres are not all on points."""
    from vcrnet_amd import support
    B, N = wr.RAGGED
    x = fr.cloud(B, N)
    excluded, est = 0, {}
    for b in range(B):
        self_rows = {r: rr.radius_rows(x[b], r) for r in sr.RADII}
        self_nrm = {r: wr.normals(x[b], s["idx"], s["row_start"])[0] for r, s in self_rows.items()}
        for name in sr.CENTRES:
            for M in (1, 333):
                c = sr.centres(x[b], name, M, seed=b)
                D = qr.d2_matrix(x[b], c)
                if name == "jitter" and M == 333:
                    assert (D.min(1) > 0).any()                     # a centre whose nearest point is not at distance 0
                for r in sr.RADII:
                    got = qr.radius_rows(x[b], c, r, D)
                    nrm = self_nrm[r]
                    cn = sr.normals(x[b], c, got["idx"], got["row_start"])[0]
                    excluded += int(fr.excluded(sr.pairs(x[b], nrm, c, np.nan_to_num(cn), got["idx"], got["row_start"])).sum())
                    if M == 333:
                        n = got["count"]
                        est[(name, r)] = int(got["total"]) // M
                        if name != "outside":
                            assert (n == 0).any() if r == 0.1 else n.max() > (255 if r == 0.53 else 128), (name, r)
                        if name == "jitter" and r == 0.335:
                            assert n.min() < support.WAVE_SPFH < 63 < 64 < 65 <= n.max()
    assert excluded == 0
    assert est[("jitter", 0.1)] < support.WAVE_SPFH <= est[("jitter", 0.335)] and est[("outside", 0.53)] < support.WAVE_SPFH
    assert est[("jitter", 0.53)] > 128
    at = sr.subset(N)
    assert len(at) == 37 and (at == -1).sum() == 1 and len(set(at.tolist())) == 36


# ---------------------------------------------------------------------------------------------------------------- the boundary

def test_signatures_match_the_header_and_the_library_exports_them(lib):
    from vcrnet_amd import support
    boundary.check_signatures(HEADER, support, lib, ENTRY_POINTS)


def test_args_match_the_c_layout(tmp_path):
    import vcrnet_amd  # noqa: F401
    from vcrnet_amd import support
    assert set(support.STRUCTS) == {"vcr_support_normals_args", "vcr_support_spfh_args", "vcr_support_needed_args",
                                    "vcr_support_fpfh_args"}
    boundary.check_layout(HEADER, support, tmp_path)
    assert support.SupportNormalsArgs.curvature.offset == support.SupportNormalsArgs.normals.offset + 8   # the mandatory part's end


def _headers():
    for d in sorted(os.listdir(INCLUDE)):
        if d.endswith(".h"):
            yield os.path.join(INCLUDE, d)
        else:
            for f in sorted(os.listdir(os.path.join(INCLUDE, d))):
                yield os.path.join(INCLUDE, d, f)


def test_the_other_boundaries_are_where_they_were(lib, monkeypatch):
    """The header is alone in a directory of its own and includes its base by relative path; it carries no other family's call
    name and no other header carries its prefix; ABI 27, the same 51 prototypes; it enters the profiles' digest behind the query
    header and the digest of support.o ALONE; the header's numbers are the module's."""
    from vcrnet_amd import build, fpfh, grid, iss, native, plane, query, radius, rows, support
    assert os.listdir(os.path.join(INCLUDE, "support")) == ["vcr_hip_support.h"]
    text = open(HEADER).read()
    for word in REFUSED:
        assert word not in text, word
    for h in _headers():
        if h != HEADER:
            other = open(h).read()
            assert "vcr_support" not in other and "VCR_SUPPORT" not in other, h
    assert '#include "../vcr_hip_plane.h"' in text and text.count("#include") == 1
    assert len(native.PUBLIC) == 51 and lib.vcr_abi_version() == native.ABI_VERSION == 27
    for other in (native, plane, fpfh, grid, radius, rows, iss, query):
        assert not set(support.SIGNATURES) & set(other.SIGNATURES) and not set(support.STRUCTS) & set(other.STRUCTS), other
    assert all(n.startswith("vcr_support_") for n in support.SIGNATURES)
    assert build.SUPPORT_HEADERS == [HEADER]
    earlier = (build.PUBLIC_HEADERS + build.LATER_HEADERS + build.OUTLIER_HEADERS + build.GICP_HEADERS + build.FPFH_HEADERS
               + build.MATCH_HEADERS + build.FGR_HEADERS + build.GRID_HEADERS + build.GRIDNN_HEADERS + build.VOXEL_SORT_HEADERS
               + build.RADIUS_HEADERS + build.ROWS_HEADERS + build.DBSCAN_HEADERS + build.SEGMENT_HEADERS + build.ORIENT_HEADERS
               + build.ISS_HEADERS + build.QUERY_HEADERS)
    assert HEADER not in earlier
    full = build.sources_sha16()
    flags = " ".join(build.FLAGS)
    hdrs = sorted(os.path.join(build.CSRC, f) for f in os.listdir(build.CSRC) if f.endswith(".h")) + earlier
    sha = lambda name: open(os.path.join(build.OBJ, name + ".o.sha")).read()    # noqa: E731 (build() ran in the fixture)
    src = lambda name: os.path.join(build.CSRC, name + ".hip")                  # noqa: E731
    assert sha("support") == build._digest([src("support")] + hdrs + [HEADER], flags) != build._digest([src("support")] + hdrs, flags)
    for name in ("rows", "query", "radius", "fpfh"):                            # every other object: the lists up to the query header
        assert sha(name) == build._digest([src(name)] + hdrs, flags), name
    monkeypatch.setattr(build, "SUPPORT_HEADERS", [])
    assert build.sources_sha16() != full
    monkeypatch.undo()
    # ... behind the query header: the digest is that of the earlier files, then this one
    import hashlib
    h = hashlib.sha256()
    files = sorted(os.path.join(build.CSRC, f) for f in os.listdir(build.CSRC) if f.endswith((".hip", ".h"))) + earlier + [HEADER]
    for f in files:
        h.update(os.path.basename(f).encode())
        h.update(open(f, "rb").read())
    assert h.hexdigest()[:16] == full
    for name, value in (("VCR_SUPPORT_MAX_N", support.MAX_N), ("VCR_SUPPORT_SPFH_WORDS", support.SPFH_WORDS),
                        ("VCR_SUPPORT_LANE", support.FORMS["lane"]), ("VCR_SUPPORT_WAVE", support.FORMS["wave"]),
                        ("VCR_SUPPORT_WAVE_SPFH", support.WAVE_SPFH), ("VCR_SUPPORT_WAVE_CENTRES", support.WAVE_CENTRES),
                        ("VCR_SUPPORT_COVERAGE_PCT", support.COVERAGE_PCT)):
        assert "#define %s %d" % (name, value) in text, name
    assert (support.MAX_N, support.SPFH_WORDS, support.FORMS) == (rows.MAX_N, rows.SPFH_WORDS, rows.FORMS)
    # what rows.hip and support.hip share is a csrc header, compiled into both; the grid's words stay in the grid's headers
    for f in ("rows.hip", "support.hip"):
        assert '#include "rows_pair.h"' in open(os.path.join(build.CSRC, f)).read()
    shared = open(os.path.join(build.CSRC, "rows_pair.h")).read()
    for fn in ("rw_row(", "rw_pair(", "rw_bin("):
        assert shared.count("__device__ __forceinline__") >= 5 and fn in shared
        for f in ("rows.hip", "support.hip"):
            assert "__forceinline__ bool " + fn not in open(os.path.join(build.CSRC, f)).read()


KINDS = {"normals": "SupportNormalsArgs", "spfh": "SupportSpfhArgs", "needed": "SupportNeededArgs", "fpfh": "SupportFpfhArgs"}
OPTIONAL = {"self", "viewpoint", "curvature", "slot"}
ALIGNED = {"normals": ("xyz4", "c4"), "spfh": ("xyz4", "c4", "spfh"), "needed": ("xyz4", "c4"),
           "fpfh": ("xyz4", "c4", "support_spfh", "centre_spfh")}


def _args(kind, **kw):
    from vcrnet_amd import support
    a = getattr(support, KINDS[kind])()
    for k, f in enumerate(n for n, t in a._fields_ if t is ctypes.c_void_p):       # (never dereferenced)
        setattr(a, f, 0x1000 * (k + 1))
    v = dict(B=2, N=1000, M=700, capacity=20000, max_nn=0)
    if kind == "fpfh":
        v["R"] = 1000
    v.update(kw)
    for k, x in v.items():
        setattr(a, k, x)
    return a


@pytest.mark.parametrize("kind", sorted(KINDS))
def test_the_calls_return_their_argument_errors_without_a_gpu(lib, kind):
    """Nothing is dereferenced and no device is touched: every refusal returns before any device call."""
    if kind == "needed":
        def f32(a):
            rc = lib.vcr_support_needed_f32(ctypes.byref(a), 0x10000, 1 << 40, None)
            assert lib.vcr_support_needed_workspace_bytes(ctypes.byref(a), 256) == 0
            return rc
        assert lib.vcr_support_needed_f32(None, 0x10000, 1 << 40, None) == EINVAL
        assert lib.vcr_support_needed_workspace_bytes(None, 256) == 0
    else:
        f32 = lambda a: getattr(lib, "vcr_support_%s_f32" % kind)(ctypes.byref(a), None)  # noqa: E731
        assert getattr(lib, "vcr_support_%s_f32" % kind)(None, None) == EINVAL
    pointers = [n for n, t in _args(kind)._fields_ if t is ctypes.c_void_p and n not in OPTIONAL]
    for field in pointers:
        assert f32(_args(kind, **{field: None})) == EINVAL, field
    for field in ALIGNED[kind]:
        assert f32(_args(kind, **{field: 0x1008})) == EINVAL, field
    bad = [dict(B=0), dict(B=-1), dict(capacity=-1), dict(max_nn=-1), dict(idx=None, capacity=1)]
    if kind == "spfh":
        bad += [dict(variant=3), dict(variant=-1), dict(variant=0x10)]
    for kw in bad:
        assert f32(_args(kind, **kw)) == EINVAL, kw
    big = [dict(N=0), dict(N=-5), dict(N=131073), dict(M=0), dict(M=-1), dict(M=131073), dict(B=16384, N=131072, M=1),
           dict(B=16384, M=131072, N=1), dict(B=2, capacity=1 << 30), dict(B=3, capacity=1 << 30)]
    if kind == "fpfh":
        big += [dict(R=0), dict(R=-1), dict(R=131073), dict(B=16384, N=1, M=1, R=131072)]
    for kw in big:
        assert f32(_args(kind, **kw)) == EUNSUPPORTED, kw
    size = ctypes.sizeof(type(_args(kind)))
    for wrong in (0, size - 16, size + 8):                  # unsized, short of the mandatory part, longer than known
        a = _args(kind)
        a.struct_bytes = wrong
        assert f32(a) == EINVAL, wrong
    assert _args(kind).struct_bytes == size
    if kind == "needed":                                     # what passes, and the workspace's own refusals
        up = lambda v: (v + 255) & ~255                      # noqa: E731
        for kw in (dict(), dict(self=None), dict(idx=None, capacity=0), dict(N=1, M=1), dict(B=1, N=131072, M=131072), dict(max_nn=7)):
            a = _args(kind, **kw)
            want = up(4 * a.B * a.N) + up(4 * a.B * ((a.N + 255) // 256))
            assert lib.vcr_support_needed_workspace_bytes(ctypes.byref(a), 256) == want == lib.vcr_support_needed_workspace_bytes(
                ctypes.byref(a), 0), kw
        ok = _args(kind)
        need = lib.vcr_support_needed_workspace_bytes(ctypes.byref(ok), 256)
        assert lib.vcr_support_needed_workspace_bytes(ctypes.byref(ok), -1) == 0
        assert lib.vcr_support_needed_f32(ctypes.byref(ok), None, need, None) == EINVAL
        assert lib.vcr_support_needed_f32(ctypes.byref(ok), 0x10008, need, None) == EINVAL
        assert lib.vcr_support_needed_f32(ctypes.byref(ok), 0x10000, need - 1, None) == EWORKSPACE


def test_the_form_and_the_plan_are_host_only_and_follow_the_header(lib):
    """The wave form where B * M <= VCR_SUPPORT_WAVE_CENTRES, otherwise from est = capacity / M, cut at max_nn, from
    VCR_SUPPORT_WAVE_SPFH on; variant forces either; the device's size and N do not enter.  The plan: "all" where the normals are
    estimated, else by min(N, est M) / N against VCR_SUPPORT_COVERAGE_PCT; without a capacity "all"."""
    from vcrnet_amd import native, support
    S = support.WAVE_SPFH
    lane, wave = support.FORMS["lane"], support.FORMS["wave"]
    W = support.WAVE_CENTRES
    assert W == 32768
    for B, M in ((1, 1), (2, 1000), (1, W), (2, W // 2), (1, W + 1), (3, W // 2), (16, 16384), (1, 131072)):
        few = B * M <= W
        for est in (0, 1, S - 1, S, S + 1, 330, 4096):
            if B * (M * est + M) >= 1 << 31:
                continue
            for cap in (M * est, M * est + M - 1):
                want = wave if few or est >= S else lane
                for N in (1, 5000, 131072):
                    assert support.form(B, N, M, cap) == want == support.form(B, N, M, cap, cu_count=0), (B, N, M, cap)
                assert support.form(B, 1000, M, cap, max_nn=est + 5) == want
                for m in (1, S - 1, S):
                    assert support.form(B, 1000, M, cap, max_nn=m) == (wave if few or min(est, m) >= S else lane), (B, M, cap, m)
                assert support.form(B, 1000, M, cap, variant=lane) == lane and support.form(B, 1000, M, cap, variant=wave) == wave
    form = lib.vcr_support_form
    assert form(2, 1000, 700, 20000, 0, 256, 0, None) == 0
    for a in ((0, 1000, 700, 0, 0, 256, 0), (2, 1000, 700, -1, 0, 256, 0), (2, 1000, 700, 0, -1, 256, 0), (2, 1000, 700, 0, 0, -1, 0),
              (2, 1000, 700, 0, 0, 256, 3)):
        assert form(*a, None) == EINVAL, a
    for a in ((2, 0, 700, 0, 0, 256, 0), (2, 1000, 0, 0, 0, 256, 0), (2, 131073, 700, 0, 0, 256, 0), (2, 1000, 131073, 0, 0, 256, 0),
              (16384, 131072, 1, 0, 0, 256, 0), (2, 1000, 700, 1 << 30, 0, 256, 0)):
        assert form(*a, None) == EUNSUPPORTED, a
    with pytest.raises(native.VcrHipError):
        support.form(1, 10, 131073, 10)
    P = support.COVERAGE_PCT
    assert support.PLANS == ("all", "needed") and P == 0
    for N, M in ((1000, 10), (131072, 1310), (16384, 16384), (300, 333)):
        assert support.plan(N, M, capacity=10 * M, normals_given=False) == "all"
        assert support.plan(N, M, normals_given=False) == "all"
        assert support.plan(N, M) == "all"
        for est in (0, 1, 12, 30, 100):
            want = "needed" if min(N, est * M) * 100 <= P * N else "all"
            assert support.plan(N, M, capacity=est * M) == support.plan(N, M, capacity=(est * M, 5)) == want, (N, M, est)
            assert support.plan(N, M, capacity=100 * M, max_nn=est or None) == ("needed" if min(N, (est or 100) * M) * 100 <= P * N else "all")
        for forced in support.PLANS:
            assert support.plan(N, M, capacity=est * M, support=forced) == forced
    with pytest.raises(native.VcrHipError, match='support="needed" needs the support\'s normals'):
        support.plan(1000, 10, normals_given=False, support="needed")
    for bad in ("All", "", 1, True):
        with pytest.raises(native.VcrHipError, match='support must be None, "all" or "needed"'):
            support.plan(1000, 10, support=bad)


def test_the_kernels_of_support_hip_use_no_scratch_and_keep_their_occupancy():
    """hipcc's remarks for support.hip: its kernel set is the seven support_* kernels, none with scratch or a spill.  As built
    (waves a SIMD, static LDS bytes a workgroup; none takes dynamic LDS):
      support_normals_kernel     8 waves,      0 B   (60 VGPRs: rows_normals_kernel's shape)
      support_spfh_lane_kernel   4 waves, 33 792 B   (112 VGPRs; 33 counters a lane in LDS, as rows_spfh_lane_kernel)
      support_spfh_wave_kernel   4 waves,    576 B   (120 VGPRs; four waves' 33 counters and c_i)
      support_fpfh_kernel        4 waves,      0 B   (108 VGPRs: rows_fpfh_lane_kernel's 92, the slot and the own row's pointer)
      support_zero / mark / slot 8 waves             (the slot kernel's 16 B: the ballot rank's wave counts)
    What support.hip shares keeps its owner: the void kernel is rows.hip's, the compaction outlier.hip's; rows.hip's six kernels
    are what they were (tests/test_rows_cpu.py)."""
    import vcrnet_amd  # noqa: F401
    from vcrnet_amd import build
    build.build()
    res = build.kernel_resources()
    names = list(res)
    dem = subprocess.run(["c++filt"], input="\n".join(names), capture_output=True, text=True, check=True).stdout.splitlines()
    by_name = {d.replace("(anonymous namespace)::", "").replace("void ", "").split("(")[0]: res[n] for n, d in zip(names, dem)}
    mine = {d: v for d, v in by_name.items() if v["file"] == "support.hip"}
    assert set(mine) == KERNELS
    for d, v in mine.items():
        print(d, v)
        assert v.get("scratch", 0) == 0 and v.get("vgpr_spill", 0) == 0 and v.get("sgpr_spill", 0) == 0 and v["agprs"] == 0, (d, v)
    assert {d: v["occupancy"] for d, v in mine.items()} == {
        "support_normals_kernel": 8, "support_spfh_lane_kernel": 4, "support_spfh_wave_kernel": 4, "support_zero_kernel": 8,
        "support_mark_kernel": 8, "support_slot_kernel": 8, "support_fpfh_kernel": 4}
    assert {d: v["lds"] for d, v in mine.items()} == {
        "support_normals_kernel": 0, "support_spfh_lane_kernel": 33 * 256 * 4, "support_spfh_wave_kernel": 4 * 36 * 4,
        "support_zero_kernel": 0, "support_mark_kernel": 0, "support_slot_kernel": 16, "support_fpfh_kernel": 0}
    assert by_name["rows_void_kernel"]["file"] == "rows.hip" and by_name["outlier_mark_kernel"]["file"] == "outlier.hip"
    assert by_name["outlier_write_kernel"]["file"] == by_name["outlier_offsets_kernel"]["file"] == "outlier.hip"


# ------------------------------------------------------------------------------------------------------------ the Python layer

def test_the_paths_without_the_new_arguments_are_untouched():
    """The new keywords trail compute_fpfh_feature's and estimate_normals' and default to None; register_features' describe
    defaults to "all" and stands behind iss (existing tests pin capacity, orient and orient_k as the last three)."""
    import vcrnet_amd
    from vcrnet_amd import fpfh, match, plane
    p = inspect.signature(fpfh.compute_fpfh_feature).parameters
    assert list(p)[-4:] == ["queries", "query_index", "query_normals", "support"] and list(p)[-5] == "capacity"
    assert all(p[n].default is None for n in list(p)[-4:])
    p = inspect.signature(plane.estimate_normals).parameters
    assert list(p)[-2:] == ["capacity", "queries"] and p["queries"].default is None
    p = inspect.signature(match.register_features).parameters
    assert p["describe"].default == "all" and list(p).index("describe") == list(p).index("iss") + 1
    assert vcrnet_amd.compute_fpfh_feature is fpfh.compute_fpfh_feature and "support" not in vcrnet_amd.__all__


def test_python_entry_points_refuse_what_they_cannot_run():
    import vcrnet_amd
    from vcrnet_amd import native, support
    E = native.VcrHipError
    x, q = torch.zeros(2, 3, 50), torch.zeros(2, 3, 70)
    qi = torch.zeros(2, 70, dtype=torch.int32)
    nrm = torch.zeros(2, 3, 50)
    fp = vcrnet_amd.compute_fpfh_feature
    for kw in (dict(queries=q), dict(query_index=qi), dict(queries=q, query_normals=torch.zeros(2, 3, 70)), dict(queries=q, support="all")):
        for search in ("knn", "grid"):
            with pytest.raises(E, match='queries, query_index, query_normals and support belong to search="radius"'):
                fp(x, search=search, **kw)
        with pytest.raises(E, match='search="radius" needs a radius'):
            fp(x, search="radius", **kw)
    for kw in (dict(query_normals=torch.zeros(2, 3, 70)), dict(support="all")):
        with pytest.raises(E, match="belong to queries= or query_index=; neither is given"):
            fp(x, search="radius", radius=0.5, **kw)
    R = dict(search="radius", radius=0.5)
    for kw in (dict(want_normals=True), dict(want_idx=True)):
        with pytest.raises(E, match="want_normals and want_idx are not served with queries"):
            fp(x, queries=q, **R, **kw)
    for bad in (0, -1, 2.0, "3", True):
        with pytest.raises(E, match="max_nn must be None or an integer >= 1"):
            fp(x, queries=q, max_nn=bad, **R)
    for bad in (q.transpose(1, 2), torch.zeros(3, 70), "q", 7):
        with pytest.raises(E, match=r"compute_fpfh_feature: queries must be a \[B, 3, N\]"):
            fp(x, queries=bad, **R)
        with pytest.raises(E, match=r"estimate_normals: queries must be a \[B, 3, N\]"):
            vcrnet_amd.estimate_normals(x, queries=bad, **R)
    with pytest.raises(E, match="must hold the same number of clouds, got 2 and 3"):
        fp(x, queries=torch.zeros(3, 3, 70), **R)
    for bad in (qi.long(), qi[:, :69], torch.zeros(3, 70, dtype=torch.int32), "i"):
        with pytest.raises(E, match=r"query_index must be int32 \[B, M\] with B = 2, M = 70"):
            fp(x, queries=q, query_index=bad, **R)
    with pytest.raises(E, match=r"query_index must be int32 \[B, M\] with B = 2$"):
        fp(x, query_index=qi.long(), **R)
    for bad in (torch.zeros(2, 3, 0), torch.zeros(2, 3, 131073)):
        with pytest.raises(E, match="queries must have 1 ... 131072 points"):
            fp(x, queries=bad, **R)
    for bad in (-1, 2.5, "7", True, (1, 2, 3), (1, -1), [5, 5]):
        with pytest.raises(E, match="capacity must be None, an integer >= 0 or a pair"):
            fp(x, queries=q, capacity=bad, **R)
    for bad in ("All", 1, True):
        with pytest.raises(E, match='support must be None, "all" or "needed"'):
            fp(x, queries=q, support=bad, **R)
    with pytest.raises(E, match='support="needed" needs the support\'s normals'):
        fp(x, queries=q, support="needed", **R)
    with pytest.raises(E, match=r"normals must be \[B, 3, N\] like xyz"):
        fp(x, torch.zeros(2, 3, 49), queries=q, **R)
    with pytest.raises(E, match=r"query_normals must be \[B, 3, M\] with B, M = 2, 70"):
        fp(x, queries=q, query_normals=torch.zeros(2, 3, 50), **R)
    # everything in order but the device: the last refusal
    for kw in (dict(queries=q), dict(query_index=qi), dict(queries=q, query_index=qi, support="all"), dict(queries=q, capacity=(100, 200)),
               dict(queries=q, max_nn=5, capacity=0), dict(queries=q, query_normals=torch.zeros(2, 3, 70))):
        with pytest.raises(E, match="no CPU fallback"):
            fp(x, **R, **kw)
        with pytest.raises(E, match="no CPU fallback"):
            fp(x, nrm, support="needed", **R, **kw) if "support" not in kw else fp(x, nrm, **R, **kw)
    en = vcrnet_amd.estimate_normals
    for search in ("knn", "grid"):
        with pytest.raises(E, match='estimate_normals: queries belongs to search="radius"'):
            en(x, search=search, queries=q)
    with pytest.raises(E, match='search="radius" needs a radius'):
        en(x, search="radius", queries=q)
    with pytest.raises(E, match="want_idx is not served with queries"):
        en(x, queries=q, want_idx=True, **R)
    with pytest.raises(E, match="capacity must be None or an integer >= 0"):
        en(x, queries=q, capacity=(1, 2), **R)
    for kw in (dict(), dict(max_nn=3), dict(capacity=100, want_curvature=True)):
        with pytest.raises(E, match="no CPU fallback"):
            en(x, queries=q, **R, **kw)
    # register_features(describe=)
    y = torch.zeros(2, 3, 60)
    rf = vcrnet_amd.register_features
    for bad in ("ALL", "iss", None, 1, True):
        with pytest.raises(E, match='register_features: describe must be "all" or "keypoints"'):
            rf(x, y, 0.1, describe=bad)
    for kw in (dict(), dict(keypoints="iss"), dict(search="radius", radius=0.5), dict(keypoints="iss", search="grid"),
               dict(keypoints="iss", method="fgr"), dict(keypoints="iss", centre=True)):
        with pytest.raises(E, match='describe="keypoints" needs keypoints="iss" and search="radius"'):
            rf(x, y, 0.1, describe="keypoints", **kw)
    for kw in (dict(), dict(method="fgr"), dict(centre=True)):
        with pytest.raises(E, match="no CPU fallback"):
            rf(x, y, 0.1, describe="keypoints", keypoints="iss", iss=dict(salient_radius=0.2, non_max_radius=0.1), **R, **kw)
        with pytest.raises(E, match="no CPU fallback"):
            rf(x, y, 0.1, describe="all", keypoints="iss", iss=dict(salient_radius=0.2, non_max_radius=0.1), **R, **kw)
    # the raw wrappers: shapes and types first, then the device
    x4, c4 = torch.zeros(2, 50, 4), torch.zeros(2, 70, 4)
    idx, rs, tot = torch.zeros(2, 100, dtype=torch.int32), torch.zeros(2, 71, dtype=torch.int64), torch.zeros(2, dtype=torch.int64)
    cn, sp, cs = torch.zeros(2, 3, 70), torch.zeros(2, 50, 3, 12, dtype=torch.int32), torch.zeros(2, 70, 3, 12, dtype=torch.int32)
    with pytest.raises(E, match=r"c4 must be float32 \[B, M, 4\]"):
        support.normals(x4, c4[:1], idx, rs, tot)
    with pytest.raises(E, match=r"idx must be int32 \[B, capacity\]"):
        support.normals(x4, c4, idx.long(), rs, tot)
    with pytest.raises(E, match=r"row_start must be int64 \[B, M \+ 1\]"):
        support.needed(x4, c4, idx, rs[:, :51], tot)
    with pytest.raises(E, match=r"total must be int64 \[B\]"):
        support.spfh(x4, nrm, c4, cn, idx, rs, tot.int())
    with pytest.raises(E, match=r"self_index must be None or int32 \[B, M\]"):
        support.normals(x4, c4, idx, rs, tot, self_index=qi.long())
    with pytest.raises(E, match=r"centre_normals must be float32 \[B, 3, M\]"):
        support.spfh(x4, nrm, c4, nrm, idx, rs, tot)
    with pytest.raises(E, match=r"support_spfh must be int32 \[B, R, 3, 12\]"):
        support.fpfh(x4, c4, idx, rs, tot, sp.view(2, 50, 36), cs)
    with pytest.raises(E, match=r"centre_spfh must be int32 \[B, M, 3, 12\]"):
        support.fpfh(x4, c4, idx, rs, tot, sp, sp)
    with pytest.raises(E, match=r"slot must be None or int32 \[B, N\]"):
        support.fpfh(x4, c4, idx, rs, tot, sp, cs, slot=qi)
    with pytest.raises(E, match="without a slot support_spfh must hold a row a support point"):
        support.fpfh(x4, c4, idx, rs, tot, sp[:, :40], cs)
    with pytest.raises(E, match="max_nn must be None or an integer >= 1"):
        support.normals(x4, c4, idx, rs, tot, max_nn=0)
    with pytest.raises(E, match="variant must be 0"):
        support.spfh(x4, nrm, c4, cn, idx, rs, tot, variant="block")
    for call in (lambda: support.normals(x4, c4, idx, rs, tot), lambda: support.spfh(x4, nrm, c4, cn, idx, rs, tot, variant="wave"),
                 lambda: support.needed(x4, c4, idx, rs, tot, self_index=qi),
                 lambda: support.fpfh(x4, c4, idx, rs, tot, sp, cs, max_nn=7)):
        with pytest.raises(E, match="no CPU fallback|device tensors only"):
            call()
