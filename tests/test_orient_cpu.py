"""Consistent normal orientation without a GPU: the two numpy restatements (tests/orient_restated.py) -- the definition by
Kruskal's algorithm on the sorted keys against the device's rounds --, the forest's weight against scipy's minimum spanning
tree, the bound that lets a weight, two indices and their order share one 64-bit key, the three checks of the definition on
the project's test surface and on tori and spheres, the boundary of include/orient/vcr_hip_orient.h (prototypes against
vcrnet_amd.orient.SIGNATURES, the struct against gcc's layout), every argument error of the call and of the Python functions,
and the resource remarks of orient.hip."""
import ctypes
import functools
import os
import subprocess

import numpy as np
import pytest
import torch

import boundary
import fpfh_restated as fr
import match_restated as mr
import orient_restated as ot

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INCLUDE = os.path.join(ROOT, "include")
HEADER = os.path.join(INCLUDE, "orient", "vcr_hip_orient.h")
EINVAL, EUNSUPPORTED = -1, -3
ENTRY_POINTS = {"vcr_orient_tangent_workspace_bytes", "vcr_orient_tangent_f32"}
KERNELS = {"orient_init_kernel", "orient_pick_kernel", "orient_hook_kernel", "orient_flatten_kernel", "orient_top_kernel",
           "orient_out_kernel"}
SURFACES = ((600, 20), (1500, 30))                          # match_restated.SURFACE_SHARES' (N, k)
GRAPH_K = (8, 12, None)                                     # the graph's neighbours: 8, 12 or all k of the normals'
ROUND_SHAPES = ((256, 8), (256, 12), (2048, 8), (2048, 12))


@pytest.fixture(scope="module")
def lib():
    import vcrnet_amd  # noqa: F401
    from vcrnet_amd import build, orient
    build.build()
    return orient.lib()


@functools.lru_cache(maxsize=None)
def surface_case(N, k):
    """The surface recipe with the CPU chain's neighbours and estimated normals, per side: read-only."""
    c = mr.surface(N)
    sides = []
    for x, up in zip((c["src"], c["tgt"]), mr.surface_up(c)):
        nrm, idx = ot.estimated(x, k)
        for a in (x, nrm, idx):
            a.setflags(write=False)
        sides.append((x, nrm, idx, up))
    return c, tuple(sides)


@functools.lru_cache(maxsize=None)
def round_case(kind, N, k):
    x, outward = {"torus": ot.torus, "sphere": ot.sphere}[kind](N)
    nrm, idx = ot.estimated(x, k)
    for a in (x, nrm, idx, outward):
        a.setflags(write=False)
    return x, nrm, idx, outward


def all_cases():
    """(name, xyz, nrm, idx) of every recipe the restatements are compared on."""
    for name, (x, nrm, idx) in ot.small_recipes().items():
        yield name, x, nrm, idx
    for kind in ("torus", "sphere"):
        for N, k in ROUND_SHAPES:
            yield ("%s-%d-%d" % (kind, N, k),) + round_case(kind, N, k)[:3]
    for N, k in SURFACES:
        for s, (x, nrm, idx, _) in enumerate(surface_case(N, k)[1]):
            yield "surface-%d-%d-%d" % (N, k, s), x, nrm, idx[:, :12]
    for scrambled in (False, True):
        yield ("path-4096-%d" % scrambled,) + ot.path(4096, scrambled)
    yield ("rows-2000-7",) + ot.random_rows(2000, 7)


# ------------------------------------------------------------------------------------------------------------ the restatements

def test_the_two_restatements_agree_on_every_recipe():
    """Equal flip, ref, trees, oriented bits and the forest's very edges; together the recipes hold one tree and several, a
    round count of 0, 1 and 5 or more, a reversing edge, and a flip by the reference's rule alone."""
    trees, rounds_seen, seen = set(), set(), 0
    for name, x, nrm, idx in all_cases():
        a = ot.definition(x, nrm, idx)
        b, rounds = ot.boruvka(x, nrm, idx, want_rounds=True)
        assert ot.same(a, b), name
        N = x.shape[1]
        assert len(a["tree"]) == N - a["n_trees"] and a["flip"].shape == (N,) and set(np.unique(a["flip"])) <= {0, 1}, name
        assert (a["ref"][a["ref"]] == a["ref"]).all() and len(np.unique(a["ref"])) == a["n_trees"], name
        flipped = a["oriented"].view(np.uint32) ^ np.ascontiguousarray(nrm).view(np.uint32)
        assert (flipped == (a["flip"].astype(np.uint32) << np.uint32(31))[None, :]).all(), name
        with np.errstate(invalid="ignore"):
            assert not (a["oriented"][2, np.unique(a["ref"])] < 0).any(), name         # every top point looks up
        trees.add(a["n_trees"])
        rounds_seen.add(rounds)
        seen += 1
    print("recipes", seen, "trees", sorted(trees), "rounds", sorted(rounds_seen))
    assert {1, 2, 5} <= trees and {0, 1} <= rounds_seen and max(rounds_seen) >= 5
    # the in-order path hooks every vertex under its predecessor in ONE round; the scrambled one needs several
    assert ot.boruvka(*ot.path(4096), want_rounds=True)[1] == 1 and ot.boruvka(*ot.path(4096, True), want_rounds=True)[1] > 3


def test_cases_worked_by_hand():
    r = ot.small_recipes()
    one = ot.definition(*r["one"])                          # a single point looking down: flipped by the reference's rule
    assert one["flip"].tolist() == [1] and one["ref"].tolist() == [0] and one["n_trees"] == 1 and one["oriented"][2, 0] == 1
    two = ot.definition(*r["two"])                          # n . n = -1: the edge reverses; equal z, so 0 is the reference
    assert two["flip"].tolist() == [1, 0] and two["ref"].tolist() == [0, 0] and (two["oriented"][2] == 1).all()
    far = ot.definition(*r["far-end"])
    assert far["n_trees"] == 1 and far["ref"].tolist() == [0] * 4 and far["flip"].tolist() == [0, 0, 1, 0]
    tri = ot.definition(*r["one-sided-triangle"])           # the forest is {0,2} and {1,2}: the heaviest edge is left out
    e = ot.edges(r["one-sided-triangle"][1], r["one-sided-triangle"][2])
    assert tri["n_trees"] == 1 and sorted(tri["tree"].tolist()) == sorted(e["key"][[1, 2]].tolist()) and e["lo"].tolist() == [0, 0, 1]
    assert e["w"][0] > e["w"][2] > e["w"][1]
    assert ot.definition(*r["equal-top"])["ref"].tolist() == [2] * 7
    assert ot.definition(*r["signed-zero-top"])["ref"].tolist() == [0] * 7
    nz = ot.definition(*r["nonfinite-z-tree"])
    assert nz["n_trees"] == 2 and nz["ref"].tolist() == [0, 0, 0, 3, 3]
    nf = ot.definition(*r["nonfinite"])
    assert not np.isin(nf["ref"], [3, 50, 90, 91]).any()    # a z that is not finite ranks below every finite one
    e = ot.edges(r["nonfinite"][1], r["nonfinite"][2])
    bad = ~np.isfinite(e["d"])
    assert bad.any() and (e["w"][bad] == 1).all() and not e["rev"][bad].any()
    for n_blobs in (2, 5):
        got = ot.definition(*r["blobs-%d" % n_blobs])
        assert got["n_trees"] == n_blobs
    # all normals equal: every d is 1 exactly, every weight 0, nothing reverses; the last point of the path is on top and looks
    # down, so everything is flipped
    for name in ("path-64", "path-257-scrambled"):
        x, nrm, idx = r[name]
        got = ot.definition(x, nrm, idx)
        assert got["weight"] == 0 and got["flip"].all() and (got["ref"] == int(np.argmax(x[2]))).all() and got["n_trees"] == 1


def test_the_forest_weighs_what_scipys_minimum_spanning_tree_weighs():
    """scipy reads a stored 0 as no edge, so it is given w + 1: every spanning forest of a graph has the same number of
    edges, N - trees, and the shift moves them all alike."""
    sparse = pytest.importorskip("scipy.sparse")
    csgraph = pytest.importorskip("scipy.sparse.csgraph")
    seen = 0
    for name, x, nrm, idx in all_cases():
        N = x.shape[1]
        e = ot.edges(nrm, idx)
        got = ot.definition(x, nrm, idx)
        g = sparse.coo_matrix((e["w"].astype(np.float64) + 1.0, (e["lo"], e["hi"])), shape=(N, N)).tocsr()
        n_comp, _ = csgraph.connected_components(g, directed=False)
        assert n_comp == got["n_trees"], name
        t = csgraph.minimum_spanning_tree(g)
        assert t.nnz == N - got["n_trees"], name
        # fp32 weights in [0, 1] summed in float64: each sum is exact to N ulps of N
        assert abs((t.sum() - t.nnz) - got["weight"]) <= 1e-12 * N * max(1.0, N), name
        seen += 1
    assert seen >= 30


def test_the_keys_bits_fit_and_order_as_the_triple():
    """Every w the rule can produce lies in [0, 1], whose bits are below 2^30 and ascend with the value; an index is below 2^17:
    the key is (w, lo, hi) in one unsigned 64-bit compare."""
    d = np.asarray([0.0, -0.0, 1.0, -1.0, 0.5, 1 - 2.0 ** -24, 1 + 2.0 ** -23, -(1 + 2.0 ** -23), 2.0 ** -149, 2.0 ** -126, 3.4e38, -3.4e38,
                    np.inf, -np.inf, np.nan, 1e-30, 0.99999994, 7.0], np.float32)
    rs = np.random.RandomState(0)
    with np.errstate(all="ignore"):
        sample = np.concatenate([d, rs.uniform(-1.5, 1.5, 200000).astype(np.float32), rs.normal(size=50000).astype(np.float32) ** 5,
                                 rs.randint(0, 1 << 32, 200000, dtype=np.uint64).astype(np.uint32).view(np.float32)])
    w, rev = ot.weight(sample)
    assert w.dtype == np.float32 and (w >= 0).all() and (w <= 1).all() and not np.signbit(w).any()
    bits = w.view(np.uint32)
    assert int(bits.max()) == 0x3F800000 < 1 << 30 and int(bits.min()) == 0
    assert (w[~np.isfinite(sample)] == 1).all() and not rev[~np.isfinite(sample)].any() and not rev[sample == 0].any()
    assert (rev == (np.isfinite(sample) & (sample < 0))).all()
    order = np.argsort(w, kind="stable")
    assert (np.diff(bits[order].astype(np.int64)) >= 0).all()                       # the bits ascend with the value
    assert ot.MAX_N - 1 < 1 << 17
    top = ot.pack(np.float32(1), ot.MAX_N - 2, ot.MAX_N - 1)
    assert int(top.reshape(-1)[0]) < (1 << 64) - 1 == int(ot.NONE)                                  # "no key" is above every key
    # the key's order is the triple's
    n = 4000
    ws = rs.choice(np.asarray([0, 2.0 ** -24, 0.25, 0.5, 1], np.float32), n)
    lo = rs.randint(0, ot.MAX_N - 1, n)
    hi = lo + 1 + rs.randint(0, ot.MAX_N, n) % (ot.MAX_N - 1 - lo)
    keys = ot.pack(ws, lo, hi)
    by_key, by_triple = np.argsort(keys, kind="stable"), np.lexsort((hi, lo, ws))
    assert (keys[by_key] == keys[by_triple]).all()
    # the same bits from either end
    nrm = rs.normal(size=(3, 500)).astype(np.float32)
    i, j = rs.randint(0, 500, 3000), rs.randint(0, 500, 3000)
    assert np.array_equal(ot.dot(nrm, i, j).view(np.uint32), ot.dot(nrm, j, i).view(np.uint32))


# --------------------------------------------------------------------------------------------------------- what it is good for

@pytest.mark.parametrize("N,k", SURFACES)
def test_the_surfaces_normals_agree_with_the_sensors_up_to_one_sign(N, k):
    """On both clouds of match_restated.surface, with graphs of 8, 12 and k neighbours: one tree, and every normal equal to
    match_restated.orient's up to ONE global sign -- a share of exactly 1.0."""
    for x, nrm, idx, up in surface_case(N, k)[1]:
        for gk in GRAPH_K:
            got = ot.definition(x, nrm, idx[:, :gk])
            assert got["n_trees"] == 1 and ot.agreement(got["oriented"], mr.orient(nrm, up)) == 1.0, (N, k, gk)


@pytest.mark.parametrize("N,k", ROUND_SHAPES)
def test_tori_and_spheres_come_out_outward(N, k):
    for kind in ("torus", "sphere"):
        x, nrm, idx, outward = round_case(kind, N, k)
        got = ot.definition(x, nrm, idx)
        assert got["n_trees"] == 1 and ot.outward_share(got["oriented"], outward) == 1.0, (kind, N, k)


@pytest.mark.parametrize("N,k", SURFACES)
def test_the_surfaces_matches_with_tangent_orientation_reach_the_oriented_share(N, k):
    """surface_shares' chain with the normals oriented by the definition (a graph of 12 neighbours): under the better of the
    source's two global signs the one-way share reaches the table's oriented figure; under the other it collapses, which is
    why register_features tries both.  As computed: 0.9967 against 0.11 at (600, 20), 1.0000 against 0.11 at (1500, 30)."""
    c, sides = surface_case(N, k)
    nrms = [ot.definition(x, nrm, idx[:, :12])["oriented"] for x, nrm, idx, _ in sides]
    feat = lambda s, n: fr.fpfh(sides[s][0], sides[s][2], fr.spfh(sides[s][0], n, sides[s][2])).astype(np.float64)   # noqa: E731
    b = feat(1, nrms[1])
    shares = []
    for sign in (1, -1):
        a = feat(0, (nrms[0] * np.float32(sign)).astype(np.float32))
        d = ((a[:, :, None] - b[:, None, :]) ** 2).sum(0)
        shares.append(float((d.argmin(1) == c["twin"]).mean()))
    print("one-way shares under the two source signs", N, k, shares)
    assert max(shares) >= mr.SURFACE_SHARES[(N, k, True, False)] - mr.SHARE_SLACK
    assert min(shares) < 0.5


# ---------------------------------------------------------------------------------------------------------------- the boundary

def test_signatures_match_the_header_and_the_library_exports_them(lib):
    from vcrnet_amd import orient
    boundary.check_signatures(HEADER, orient, lib, ENTRY_POINTS)


def test_args_match_the_c_layout(tmp_path):
    import vcrnet_amd  # noqa: F401
    from vcrnet_amd import orient
    assert set(orient.STRUCTS) == {"vcr_orient_tangent_args"}
    boundary.check_layout(HEADER, orient, tmp_path)
    A = orient.OrientTangentArgs
    assert A.flip.offset == A.oriented.offset + 8           # where the mandatory part ends


def test_the_header_lives_in_a_directory_of_its_own_and_enters_the_digests(lib, monkeypatch):
    from vcrnet_amd import build, dbscan, native, orient, segment
    assert os.listdir(os.path.join(INCLUDE, "orient")) == ["vcr_hip_orient.h"]
    for d in sorted(os.listdir(INCLUDE)):
        for f in ([d] if d.endswith(".h") else os.listdir(os.path.join(INCLUDE, d))):
            h = os.path.join(INCLUDE, f) if d.endswith(".h") else os.path.join(INCLUDE, d, f)
            if h != HEADER:
                assert "orient_tangent" not in open(h).read(), h
    assert '#include "../vcr_hip.h"' in open(HEADER).read()
    assert lib.vcr_abi_version() == native.ABI_VERSION == 27
    for other in (native, dbscan, segment):
        assert not set(orient.SIGNATURES) & set(other.SIGNATURES) and not set(orient.STRUCTS) & set(other.STRUCTS)
    assert build.ORIENT_HEADERS == [HEADER]
    assert HEADER not in (build.PUBLIC_HEADERS + build.LATER_HEADERS + build.OUTLIER_HEADERS + build.GICP_HEADERS
                          + build.FPFH_HEADERS + build.MATCH_HEADERS + build.FGR_HEADERS + build.GRID_HEADERS
                          + build.GRIDNN_HEADERS + build.VOXEL_SORT_HEADERS + build.RADIUS_HEADERS + build.ROWS_HEADERS
                          + build.DBSCAN_HEADERS + build.SEGMENT_HEADERS)
    full = build.sources_sha16()
    monkeypatch.setattr(build, "ORIENT_HEADERS", [])
    assert build.sources_sha16() != full
    monkeypatch.undo()
    text = open(HEADER).read()
    for name, value in (("VCR_ORIENT_MAX_N", orient.MAX_N), ("VCR_ORIENT_ROUNDS", orient.FORMS["rounds"]),
                        ("VCR_ORIENT_ONE_LAUNCH", orient.FORMS["one_launch"])):
        assert "#define %s %d" % (name, value) in text, name
    assert orient.MAX_N == ot.MAX_N


def _args(**kw):
    from vcrnet_amd import orient
    a = orient.OrientTangentArgs()
    for k, f in enumerate(n for n, t in a._fields_ if t is ctypes.c_void_p):       # (never dereferenced)
        setattr(a, f, 0x1000 * (k + 1))
    v = dict(B=2, N=1000, k=12)
    v.update(kw)
    for k, x in v.items():
        setattr(a, k, x)
    return a


WS = 0x100000                                               # a 256-aligned address that is never dereferenced


def test_the_call_returns_its_argument_errors_without_a_gpu(lib):
    need = lambda a: lib.vcr_orient_tangent_workspace_bytes(ctypes.byref(a), 0)    # noqa: E731
    f32 = lambda a, ws=WS, n=None: lib.vcr_orient_tangent_f32(ctypes.byref(a), ws, need(_args()) if n is None else n, None)  # noqa: E731
    assert lib.vcr_orient_tangent_f32(None, WS, 1 << 30, None) == EINVAL and lib.vcr_orient_tangent_workspace_bytes(None, 0) == 0
    for field in ("xyz", "normals", "idx", "oriented"):
        assert f32(_args(**{field: None})) == EINVAL and need(_args(**{field: None})) == 0, field
    assert need(_args(flip=None, ref=None, n_trees=None)) == need(_args()) > 0
    for kw in (dict(B=0), dict(B=-1), dict(k=0), dict(k=-2), dict(variant=3), dict(variant=-1), dict(variant=0x10)):
        assert f32(_args(**kw)) == EINVAL and need(_args(**kw)) == 0, kw
    for kw in (dict(N=0), dict(N=-5), dict(N=131073), dict(B=16384, N=131072), dict(B=16, N=131072, k=1024), dict(variant=2)):
        assert f32(_args(**kw), n=1 << 40) == EUNSUPPORTED and need(_args(**kw)) == 0, kw
    assert need(_args(variant=1)) == need(_args())
    size = ctypes.sizeof(type(_args()))
    for wrong in (0, size - 32, size + 8):                  # unsized, short of the mandatory part, longer than known
        a = _args()
        a.struct_bytes = wrong
        assert f32(a) == EINVAL and need(a) == 0, wrong
    a = _args()
    a.struct_bytes = size - 24                              # a caller that knows none of the optional outputs is served
    assert need(a) == need(_args())
    good = need(_args())
    assert good % 256 == 0 and good >= 24 * 2 * 1000        # two words and two 64-bit slots a point
    assert f32(_args(), ws=None) == EINVAL and f32(_args(), ws=WS + 128) == EINVAL and f32(_args(), ws=WS + 16) == EINVAL
    assert f32(_args(), n=good - 1) == EINVAL and f32(_args(), n=0) == EINVAL
    assert lib.vcr_orient_tangent_workspace_bytes(ctypes.byref(_args()), -1) == 0
    assert need(_args(B=1, N=131072, k=62)) >= 24 * 131072 and need(_args(B=1, N=1, k=1)) > 0


def test_the_kernels_of_orient_hip_use_no_scratch():
    """hipcc's remarks for orient.hip: its kernel set is the six below, none with scratch or a spill, none with AGPRs, all at
    eight waves a SIMD; only the output pass holds LDS (the workgroup's count of roots)."""
    import vcrnet_amd  # noqa: F401
    from vcrnet_amd import build
    build.build()
    res = build.kernel_resources()
    names = list(res)
    dem = subprocess.run(["c++filt"], input="\n".join(names), capture_output=True, text=True, check=True).stdout.splitlines()
    by_name = {d.replace("(anonymous namespace)::", "").replace("void ", "").split("(")[0]: res[n] for n, d in zip(names, dem)}
    mine = {d: v for d, v in by_name.items() if v["file"] == "orient.hip"}
    assert set(mine) == KERNELS
    for d, v in mine.items():
        print(d, v)
        assert v.get("scratch", 0) == 0 and v.get("vgpr_spill", 0) == 0 and v.get("sgpr_spill", 0) == 0 and v["agprs"] == 0, (d, v)
        assert v["occupancy"] == 8 and v["vgprs"] <= 40, (d, v)


# ------------------------------------------------------------------------------------------------------------ the Python layer

def test_python_entry_points_refuse_what_they_cannot_run():
    import vcrnet_amd
    from vcrnet_amd import native, orient
    fn = vcrnet_amd.orient_normals_consistent_tangent_plane
    assert fn is orient.orient_normals_consistent_tangent_plane
    assert "orient_normals_consistent_tangent_plane" in vcrnet_amd.__all__ and "orient" not in vcrnet_amd.__all__
    E = native.VcrHipError
    x, n = torch.zeros(2, 3, 50), torch.zeros(2, 3, 50)
    idx = torch.zeros(2, 50, 4, dtype=torch.int32)
    for bad in (x.transpose(1, 2), torch.zeros(3, 50), None, "xyz"):
        with pytest.raises(E, match=r"xyz must be a \[B, 3, N\]"):
            fn(bad, n)
    for bad in (n[:, :, :49], n.double(), n[:1], None, "n"):
        with pytest.raises(E, match=r"normals must be float32 \[B, 3, N\]"):
            fn(x, bad)
    with pytest.raises(E, match="a cloud must have 1 ... 131072 points"):
        fn(torch.zeros(1, 3, 131073), torch.zeros(1, 3, 131073))
    for bad in (idx.long(), idx[:, :49], idx[:, :, :0], idx[0], "idx"):
        with pytest.raises(E, match=r"idx must be None or int32 \[B, N, k\]"):
            fn(x, n, idx=bad)
    for bad in (0, -1, 2.0, "3", True, None):
        with pytest.raises(E, match="orient_normals_consistent_tangent_plane: k must be an integer >= 1"):
            fn(x, n, k=bad)
    for kw in (dict(), dict(k=5), dict(idx=idx), dict(idx=idx, want_flip=True, want_ref=True, want_trees=True)):
        with pytest.raises(E, match="no CPU fallback"):      # (the last refusal: everything else was in order)
            fn(x, n, **kw)
    with pytest.raises(E, match="variant must be 0"):
        orient.orient_tangent(x, n, idx, variant="block")
    with pytest.raises(E, match=r"idx must be int32 \[B, N, k\]"):
        orient.orient_tangent(x, n, None)
    with pytest.raises(E, match="no CPU fallback"):
        orient.orient_tangent(x, n, idx, variant="rounds")


def test_register_features_takes_orient_at_the_end_and_refuses_other_values():
    import inspect
    import vcrnet_amd
    from vcrnet_amd import match, native
    params = inspect.signature(match.register_features).parameters
    assert list(params)[-2:] == ["orient", "orient_k"] and params["orient"].default is None and params["orient_k"].default == 12
    assert list(params)[-3] == "capacity"                   # appended: nothing in front of them moved
    E = native.VcrHipError
    x = torch.zeros(1, 3, 64)
    for bad in ("viewpoint", "Tangent", True, 1, ""):
        for kw in (dict(), dict(method="fgr"), dict(centre=True)):
            with pytest.raises(E, match='register_features: orient must be None or "tangent"'):
                vcrnet_amd.register_features(x, x, 0.1, orient=bad, **kw)
    for bad in (0, -3, 2.5, "12", True, None):
        with pytest.raises(E, match="register_features: orient_k must be an integer >= 1"):
            vcrnet_amd.register_features(x, x, 0.1, orient="tangent", orient_k=bad)
    for kw in (dict(), dict(method="fgr"), dict(src_normals=x, tgt_normals=x)):
        with pytest.raises(E, match="no CPU fallback"):
            vcrnet_amd.register_features(x, x, 0.1, k=10, orient="tangent", **kw)
