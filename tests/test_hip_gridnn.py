"""The grid siblings of vcr_nn_score_f32 and of the three refinements on the GPU (include/vcr_hip_gridnn.h, DESIGN.md section
4.20): the nearest neighbour searched on the target's uniform grid and capped at max_dist.

The yardstick is the SCAN form on the same device, unchanged by this search: every output of the grid form must equal it bit
for bit -- inliers, sum_d2, fitness, rmse, every pose, iterations, converged -- and nn_idx / nn_d2 after the scan form's
non-inlier rows are overwritten with (-1, +inf), the one difference of the definition.  Every equality is on bits; there are no
tolerances.  Every output buffer, and the workspace, is prefilled with a garbage byte and carries a guard band."""
import functools

import numpy as np
import pytest
import torch

import grid_restated as gr
import gridnn_restated as gn
import refine_restated as rr

pytestmark = pytest.mark.gpu

SENTINEL_BYTE = 0x5A
GUARD = 64
EVAL = ("nn_idx", "nn_d2", "inliers", "sum_d2", "fitness", "rmse")
POSE = ("R", "t", "R_ba", "t_ba", "iterations", "converged")
F32 = np.float32
INF_BITS = gr.INF_BITS


def mods():
    import vcrnet_amd  # noqa: F401
    from vcrnet_amd import gicp, plane, refine, score
    return score, refine, plane, gicp


def dev(x):
    return None if x is None else torch.tensor(np.ascontiguousarray(x)).cuda()         # (a copy: the shared cases are read-only)


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view({4: np.int32, 8: np.int64}[a.dtype.itemsize])


def guarded(o, keys, prefill=SENTINEL_BYTE):
    """All of every output must have been overwritten, none of the band behind it -> dict of numpy."""
    torch.cuda.synchronize()
    for k in keys:
        raw, n = o["_raw"][k], o[k].numel()
        band = raw[n:].view(torch.uint8).cpu().numpy()
        assert band.size == GUARD * raw.element_size() and (band == prefill).all(), (k, "guard band written")
        body = raw[:n].view(torch.uint8).cpu().numpy().reshape(n, -1)
        assert not (body == prefill).all(axis=1).any(), (k, "element left unwritten")
    return {k: o[k].cpu().numpy() for k in keys}


def nn_score(src, tgt, R=None, t=None, max_dist=0.1, **kw):
    """numpy [B,3,N] in, dict of numpy out; guarded and prefilled (the grid form's workspace too)."""
    score = mods()[0]
    return guarded(score.nn_score(dev(src), dev(tgt), dev(R), dev(t), max_dist, guard=GUARD, prefill=SENTINEL_BYTE, **kw), EVAL)


def masked(o, max_dist):
    """A scan form's dict with its non-inlier nn rows overwritten with (-1, +inf): the grid form's definition."""
    with np.errstate(over="ignore"):
        cap2 = F32(max_dist) * F32(max_dist)
    far = ~((o["nn_idx"] >= 0) & (o["nn_d2"] <= cap2))
    out = dict(o)
    out["nn_idx"] = np.where(far, np.int32(-1), o["nn_idx"]).astype(np.int32)
    out["nn_d2"] = np.where(far, F32(np.inf), o["nn_d2"]).astype(F32)
    return out


def assert_same_bits(a, b, what, keys=EVAL):
    for k in keys:
        assert a[k].dtype == b[k].dtype and np.array_equal(bits(a[k]), bits(b[k])), (what, k, np.argwhere(bits(a[k]) != bits(b[k]))[:5])


def assert_grid_is_scan(src, tgt, R, t, max_dist, what, forms=((None, 0),)):
    """The grid form under every (cell, order) of `forms` against the masked scan form -> the scan form's dict."""
    want = nn_score(src, tgt, R, t, max_dist)
    Nt = tgt.shape[2]
    for cell, order in forms:
        got = nn_score(src, tgt, R, t, max_dist, search="grid", cell=cell, order=order)
        assert (got["nn_idx"] >= -1).all() and (got["nn_idx"] < Nt).all()
        assert_same_bits(got, masked(want, max_dist), (what, cell, order))
    return want


def pose(seed, B, degrees=3.0, shift=0.01):
    rs = np.random.RandomState(seed)
    R = np.stack([rr.rotation(rs.normal(size=3), degrees) for _ in range(B)]).astype(F32)
    t = (shift * rs.normal(size=(B, 3))).astype(F32)
    return R, t


# ---------------------------------------------------------------------------------------------------------------------- sizes

@pytest.mark.parametrize("Ns,Nt", [(1, 1), (1, 300), (300, 1), (255, 257), (257, 255), (1000, 64)])
def test_sizes_against_the_scan_form(Ns, Nt):
    """One point on either side; a workgroup's edge on either side; more than one workgroup against fewer points than a wave.
    B = 3, under a pose, both orders and the plan's."""
    rs = np.random.RandomState(Ns * 1000 + Nt)
    tgt = rs.uniform(0, 1, (3, 3, Nt)).astype(F32)
    src = np.concatenate([tgt[:, :, rs.randint(0, Nt, Ns - Ns // 3)], rs.uniform(0, 1, (3, 3, Ns // 3)).astype(F32)], 2)
    R, t = pose(Ns + Nt, 3, 1.0, 0.004)
    for max_dist in (0.03, 0.3):
        want = assert_grid_is_scan(src, tgt, R, t, max_dist, (Ns, Nt, max_dist), ((None, 0), (None, 1), (None, 2)))
        if Ns >= 255:
            assert 0 < want["inliers"].min()
            assert max_dist > 0.1 or want["inliers"].max() < Ns             # (the cap cuts: both kinds of row are there)
    assert_grid_is_scan(src, tgt, None, None, 0.0, (Ns, Nt, "identity"), ((None, 1), (None, 2)))


# ------------------------------------------------------------------------------------------------------------ recipes and caps

@functools.lru_cache(maxsize=None)
def recipe(name, N):
    """(src [8,3,n], tgt [8,3,N]): the CPU test's target at the origin and moved by 1 024, against its source as it is and
    shifted a whole extent beyond the box along one, two and three axes -- eight clouds of one batch.  Read-only."""
    srcs, tgts = [], []
    for offset in (0.0, 1024.0):
        q = gr.RECIPES[name](N, seed=N)
        q = gr.moved(q, offset) if offset else q
        p0 = gn.source_of(q, seed=N)
        for sh in gn.SHIFTS:
            srcs.append(gn.shifted(p0, q, sh))
            tgts.append(q)
    src, tgt = np.stack(srcs), np.stack(tgts)
    src.setflags(write=False), tgt.setflags(write=False)
    return src, tgt


@pytest.mark.parametrize("name,N", [(name, 300) for name in gn.RECIPES] + [(name, 2000) for name in gn.LARGE])
def test_recipes_and_caps(name, N):
    """The CPU test's recipes, sources and caps on the device: max_dist in {0, half the edge, 4 edges, 1e30}."""
    src, tgt = recipe(name, N)
    for max_dist in gn.caps(tgt[0]):
        want = assert_grid_is_scan(src, tgt, None, None, max_dist, (name, N, max_dist))
        if max_dist == 1e30:                                 # cap2 = +inf: nothing is masked, the scan form's arrays as they are
            got = nn_score(src, tgt, None, None, max_dist, search="grid")
            assert_same_bits(got, want, (name, N, "1e30 unmasked"))
    # the CPU restatement's definition, for the first cloud: the yardstick itself is the header's
    idx, d2 = gn.definition(src[0], tgt[0], gn.caps(tgt[0])[2])
    got = nn_score(src[:1], tgt[:1], None, None, gn.caps(tgt[0])[2], search="grid")
    assert np.array_equal(got["nn_idx"][0], idx) and np.array_equal(bits(got["nn_d2"][0]), d2)
    # max_dist = 0 on a copy of the target: every finite point is its own (or an earlier copy's) partner at d2 = 0
    got = nn_score(tgt, tgt, None, None, 0.0, search="grid")
    finite = np.isfinite(tgt).all(1)
    assert np.array_equal(got["inliers"], finite.sum(1).astype(np.int32))
    assert (got["fitness"] == finite.sum(1).astype(F32) / F32(N)).all() and (got["rmse"] == 0).all()
    if finite.all():
        assert (got["fitness"] == 1).all()
    assert (got["nn_idx"][finite] <= np.broadcast_to(np.arange(N), finite.shape)[finite]).all() and (got["nn_idx"][~finite] == -1).all()


# ---------------------------------------------------------------------------------------------------------- grid independence

@pytest.mark.parametrize("name", ["random", "lattice", "copies", "nonfinite", "outlier"])
def test_every_grid_and_both_orders_return_the_same_bits(name):
    """Every forced cell from "every point its own cell" to "one cell", both orders; the second cloud's source lies wholly
    outside the target's box and its points are inliers under a cap larger than the shift."""
    N = 300
    q = gr.RECIPES[name](N, seed=3)
    p = gn.source_of(q, seed=3)
    e, _ = gn.extent(q)
    src, tgt = np.stack([p, gn.shifted(p, q, (0, 1, 2))]), np.stack([q, q])
    forms = [(cell, order) for cell in [None] + gr.forced_cells(q) for order in (1, 2)]
    h = float(gr.make_grid(q)[1])
    for max_dist in (2.0 * h, 2.5 * float(np.sqrt((e.astype(np.float64) ** 2).sum()))):
        want = assert_grid_is_scan(src, tgt, None, None, max_dist, (name, max_dist), forms)
    finite = np.isfinite(src[1]).all(0)
    assert (want["nn_idx"][1][finite] >= 0).sum() > N // 2 and want["inliers"][1] > N // 2      # (outside the box, and inliers)


# ------------------------------------------------------------------------------------------------------------ non-finite input

def test_non_finite_input():
    rs = np.random.RandomState(11)
    N = 700
    tgt = rs.uniform(0, 1, (2, 3, N)).astype(F32)
    src = (tgt[:, :, rs.permutation(N)[:500]] + F32(0.001)).astype(F32)
    R, t = pose(5, 2, 0.5, 0.002)
    clean = assert_grid_is_scan(src, tgt, R, t, 0.05, "clean", ((None, 1), (None, 2)))
    assert clean["inliers"].min() > 400
    # a NaN pose: every moved point is NaN -- nobody has a neighbour
    Rn = R.copy()
    Rn[1, 1, 1] = np.nan
    got = nn_score(src, tgt, Rn, t, 0.05, search="grid")
    assert_same_bits(got, masked(nn_score(src, tgt, Rn, t, 0.05), 0.05), "nan pose")
    assert (got["nn_idx"][1] == -1).all() and (bits(got["nn_d2"][1]) == INF_BITS).all()
    assert got["fitness"][1] == 0 and got["rmse"][1] == 0 and got["inliers"][1] == 0
    assert_same_bits({k: v[:1] for k, v in got.items()}, {k: v[:1] for k, v in masked(clean, 0.05).items()}, "the other cloud")
    # a NaN source point: its own row only
    sn = src.copy()
    sn[0, 2, 17] = np.nan
    sn[1, 0, 499] = np.inf
    got = nn_score(sn, tgt, R, t, 0.05, search="grid")
    assert_same_bits(got, masked(nn_score(sn, tgt, R, t, 0.05), 0.05), "nan source point")
    assert got["nn_idx"][0, 17] == -1 and got["nn_idx"][1, 499] == -1
    keep = np.ones((2, 500), bool)
    keep[0, 17] = keep[1, 499] = False
    want = masked(clean, 0.05)
    assert np.array_equal(got["nn_idx"][keep], want["nn_idx"][keep]) and np.array_equal(bits(got["nn_d2"][keep]), bits(want["nn_d2"][keep]))
    # a NaN / inf target point is never chosen, the partners of the others stay
    tn = tgt.copy()
    lost = clean["nn_idx"][0, :3]
    tn[0, 0, lost[0]], tn[0, 1, lost[1]], tn[0, 2, lost[2]] = np.nan, np.inf, -np.inf
    got = assert_grid_is_scan(src, tn, R, t, 0.05, "nan target point", ((None, 1), (None, 2), (0.5, 2)))
    assert not np.isin(got["nn_idx"][0], lost).any()
    # a source point at 1e30 (and one at -3e38): far outside, no overflow in the query's cell, no walk; under every cap
    sf = src.copy()
    sf[0, :, 5] = 1e30
    sf[1, 1, 6] = -3e38
    for max_dist in (0.05, 1e30):
        got = nn_score(sf, tgt, None, None, max_dist, search="grid")
        assert_same_bits(got, masked(nn_score(sf, tgt, None, None, max_dist), max_dist), ("1e30", max_dist))
        assert got["nn_idx"][0, 5] == -1 and got["nn_idx"][1, 6] == -1
    # a target without a finite point
    got = nn_score(src, np.full_like(tgt, np.nan), R, t, 0.05, search="grid")
    assert (got["nn_idx"] == -1).all() and (got["fitness"] == 0).all()


# ------------------------------------------------------------------------------------------------------- batch and translation

def test_a_batch_is_its_clouds_alone_and_a_call_repeats_itself():
    src, tgt = recipe("clustered", 300)
    h = gn.caps(tgt[0])[2]
    whole = nn_score(src, tgt, None, None, h, search="grid")
    again = nn_score(src, tgt, None, None, h, search="grid")
    assert_same_bits(whole, again, "a second call")
    for b in (0, 3, 7):
        alone = nn_score(src[b:b + 1], tgt[b:b + 1], None, None, h, search="grid")
        assert_same_bits(alone, {k: v[b:b + 1] for k, v in whole.items()}, ("alone", b))


def test_a_translation_that_is_exact_in_fp32_returns_the_same_bits():
    """Coordinates on a 2^-10 lattice in [0, 1), a signed permutation as the rotation: moving both clouds by (1024, -512, 256)
    -- and the pose's t with them -- is exact in every step, so every d2 keeps its bits."""
    rs = np.random.RandomState(2)
    tgt = (rs.randint(0, 1024, (2, 3, 900)) / 1024.0).astype(F32)
    src = (rs.randint(0, 1024, (2, 3, 700)) / 1024.0).astype(F32)
    src[:, :, :300] = tgt[:, :, 100:400]
    T = np.asarray([1024.0, -512.0, 256.0], F32)
    for R1 in (None, np.asarray([[0, -1, 0], [0, 0, 1], [-1, 0, 0]], F32)):
        R = t = R2 = t2 = None
        if R1 is not None:
            R = np.stack([R1, R1.T])
            t = (rs.randint(-64, 64, (2, 3)) / 1024.0).astype(F32)
            src = src.copy()
            src[:, :, :300] = np.einsum("bji,bjn->bin", R, tgt[:, :, 100:400] - t[:, :, None])      # R^T (q - t): exact
            R2, t2 = R, (t + T[None] - np.einsum("bij,j->bi", R, T)).astype(F32)
        for max_dist in (0.0, 0.02, 0.2):
            here = assert_grid_is_scan(src, tgt, R, t, max_dist, ("origin", max_dist), ((None, 1), (None, 2)))
            there = nn_score(src + T[None, :, None], tgt + T[None, :, None], R2, t2, max_dist, search="grid")
            assert_same_bits(there, masked(here, max_dist), ("moved", max_dist))
        assert here["inliers"].min() >= 300


# ---------------------------------------------------------------------------------------------------------------------- large

@pytest.mark.parametrize("Ns,Nt", [(131072, 70001), (70001, 131072)])
@pytest.mark.parametrize("kind", ["random", "sphere"])
def test_large_clouds_against_the_scan_form(kind, Ns, Nt):
    tgt = gr.RECIPES[kind](Nt, seed=1) if kind == "random" else gr.sphere(Nt, seed=1)
    src = gr.RECIPES[kind](Ns, seed=2) if kind == "random" else gr.sphere(Ns, seed=2)
    R, t = pose(9, 1, 2.0, 0.01)
    max_dist = 0.02 if kind == "random" else 0.005           # about the spacing: inliers and points without a partner
    want = assert_grid_is_scan(src[None], tgt[None], R, t, max_dist, (kind, Ns, Nt), ((None, 1), (None, 2)))
    assert 0 < want["inliers"][0] < Ns


# ----------------------------------------------------------------------------------------------------------------- refinement

METHODS = ("point_to_point", "point_to_plane", "generalized")


@functools.lru_cache(maxsize=None)
def refine_case(Nb, Ns):
    c = rr.batch(7, Nb, Ns)
    for v in c.values():
        v.setflags(write=False)
    return c


def normals_of(x):
    plane = mods()[2]
    return plane.estimate_normals(dev(x), 20)


def run_refine(method, src, tgt, R, t, max_dist=rr.MAX_DIST, nrm=None, **kw):
    """numpy in, dict of numpy out: refine.refine / plane.refine_plane / gicp.refine_gicp, guarded and prefilled."""
    _, refine, plane, gicp = mods()
    a = (dev(src), dev(tgt))
    kw = dict(kw, guard=GUARD, prefill=SENTINEL_BYTE)
    if method == "point_to_point":
        o = refine.refine(*a, dev(R), dev(t), max_dist, **kw)
    elif method == "point_to_plane":
        o = plane.refine_plane(*a, nrm[1], dev(R), dev(t), max_dist, **kw)
    else:
        o = gicp.refine_gicp(*a, nrm[0], nrm[1], dev(R), dev(t), max_dist, **kw)
    return guarded(o, EVAL + POSE)


@pytest.mark.parametrize("Nb,Ns", rr.SHAPES)
@pytest.mark.parametrize("method", METHODS)
def test_refinement_on_the_grid_is_the_scan_forms(method, Nb, Ns):
    """Every pose, evaluation, count and flag bit-equal; nn after masking; the closing invariant against the grid score; both
    orders and a forced cell; max_iterations = 0 is the score."""
    score = mods()[0]
    c = refine_case(Nb, Ns)
    nrm = (normals_of(c["src"]), normals_of(c["tgt"]))
    want = run_refine(method, c["src"], c["tgt"], c["R0"], c["t0"], nrm=nrm)
    assert want["iterations"].min() >= 1 and want["inliers"].min() >= Ns // 2
    for cell, order in ((None, 0), (None, 2), (0.07, 1)):
        got = run_refine(method, c["src"], c["tgt"], c["R0"], c["t0"], nrm=nrm, search="grid", cell=cell, order=order)
        assert_same_bits(got, masked(want, rr.MAX_DIST), (method, cell, order), EVAL + POSE)
        s = score.nn_score(dev(c["src"]), dev(c["tgt"]), dev(got["R"]), dev(got["t"]), rr.MAX_DIST, search="grid")
        assert_same_bits(got, {k: s[k].cpu().numpy() for k in EVAL}, ("closing invariant", method))
    zero = run_refine(method, c["src"], c["tgt"], c["R0"], c["t0"], nrm=nrm, search="grid", max_iterations=0)
    s = nn_score(c["src"], c["tgt"], c["R0"], c["t0"], rr.MAX_DIST, search="grid")
    assert_same_bits(zero, s, ("max_iterations = 0", method))
    assert (zero["iterations"] == 0).all() and np.array_equal(bits(zero["R"]), bits(c["R0"])) and np.array_equal(bits(zero["t"]), bits(c["t0"]))
    assert_same_bits(zero, masked(run_refine(method, c["src"], c["tgt"], c["R0"], c["t0"], nrm=nrm, max_iterations=0), rr.MAX_DIST),
                     ("max_iterations = 0 against the scan", method), EVAL + POSE)


@pytest.mark.parametrize("method", METHODS)
def test_a_refined_cloud_does_not_depend_on_its_batch(method):
    """rel_* = 0: no cloud converges, so clouds 0 and 2 run their 30 rounds; cloud 1 starts ten units away, has no inlier and
    stops at round 0 -- its workgroups return at once in every later search."""
    Nb, Ns = rr.SHAPES[0]
    c = refine_case(Nb, Ns)
    t0 = c["t0"].copy()
    t0[1] += 10
    nrm = (normals_of(c["src"]), normals_of(c["tgt"]))
    kw = dict(rel_fitness=0.0, rel_rmse=0.0, search="grid")
    whole = run_refine(method, c["src"], c["tgt"], c["R0"], t0, nrm=nrm, **kw)
    assert whole["iterations"].tolist() == [30, 0, 30] and whole["inliers"][1] == 0 and (whole["nn_idx"][1] == -1).all()
    scan = run_refine(method, c["src"], c["tgt"], c["R0"], t0, nrm=nrm, rel_fitness=0.0, rel_rmse=0.0)
    assert_same_bits(whole, masked(scan, rr.MAX_DIST), (method, "scan"), EVAL + POSE)
    for b in range(3):
        alone = run_refine(method, c["src"][b:b + 1], c["tgt"][b:b + 1], c["R0"][b:b + 1], t0[b:b + 1],
                           nrm=(nrm[0][b:b + 1], nrm[1][b:b + 1]), **kw)
        assert_same_bits(alone, {k: v[b:b + 1] for k, v in whole.items()}, (method, "alone", b), EVAL + POSE)


# ----------------------------------------------------------------------------------------------------------------- pass-through

def same_tensors(a, b, what):
    assert sorted(a) == sorted(b), what
    for k in a:
        x, y = a[k], b[k]
        assert x.dtype == y.dtype and x.shape == y.shape, (what, k)
        assert torch.equal(x.view(torch.int32) if x.dtype == torch.float32 else x, y.view(torch.int32) if y.dtype == torch.float32 else y), (what, k)


@pytest.fixture
def entries(monkeypatch):
    """The entry points extension.call_with_workspace is asked for, in order."""
    from vcrnet_amd import extension
    seen, real = [], extension.call_with_workspace

    def spy(L, entry, *a, **kw):
        seen.append(entry)
        return real(L, entry, *a, **kw)
    monkeypatch.setattr(extension, "call_with_workspace", spy)
    return seen


def searches(entries):
    """Of the entry points seen, those that score or refine."""
    return [e for e in entries if e.startswith(("vcr_nn_score", "vcr_refine"))]


def test_the_public_calls_pass_the_search_through(entries):
    import vcrnet_amd
    Nb, Ns = rr.SHAPES[0]
    c = refine_case(Nb, Ns)
    src, tgt, R, t = dev(c["src"]), dev(c["tgt"]), dev(c["R0"]), dev(c["t0"])
    for kw in (dict(), dict(symmetric=True), dict(want_nn=True, cell=0.2)):
        del entries[:]
        a = vcrnet_amd.score_registration(src, tgt, R, t, rr.MAX_DIST, search="grid", **kw)
        assert searches(entries) == ["vcr_nn_score_grid"] * (2 if kw.get("symmetric") else 1), entries
        b = vcrnet_amd.score_registration(src, tgt, R, t, rr.MAX_DIST, **{k: v for k, v in kw.items() if k != "cell"})
        if "nn_idx" in b:
            far = ~((b["nn_idx"] >= 0) & (b["nn_d2"] <= float(F32(rr.MAX_DIST) * F32(rr.MAX_DIST))))
            b["nn_idx"], b["nn_d2"] = b["nn_idx"].masked_fill(far, -1), b["nn_d2"].masked_fill(far, float("inf"))
        same_tensors(a, b, ("score_registration", kw))
    for method, entry in zip(METHODS, ("vcr_refine_grid", "vcr_refine_plane_grid", "vcr_refine_gicp_grid")):
        for kw in (dict(), dict(centre=True)):
            del entries[:]
            a = vcrnet_amd.refine_registration(src, tgt, R, t, rr.MAX_DIST, method=method, search="grid", **kw)
            assert searches(entries) == [entry] + (["vcr_nn_score_grid"] if kw else []), entries  # (centre's closing evaluation)
            b = vcrnet_amd.refine_registration(src, tgt, R, t, rr.MAX_DIST, method=method, **kw)
            same_tensors(a, b, (method, kw))
            assert a["iterations"].min() >= 1


def test_register_sampled_and_register_features_pass_nn_search_through(entries):
    import vcrnet_amd
    import match_restated as mr
    from test_hip_forward import build_net
    from test_hip_fps import _pair
    net, _ = build_net()
    src, tgt = _pair(3000, 4100)
    s, t = dev(src), dev(tgt)
    with torch.no_grad():
        want = vcrnet_amd.register_sampled(net, s, t, 1024, score=0.1, refine=0.1)
        del entries[:]
        got = vcrnet_amd.register_sampled(net, s, t, 1024, score=0.1, refine=0.1, nn_search="grid")
    assert searches(entries) == ["vcr_nn_score_grid", "vcr_refine_grid"], entries
    for a, b in zip(want[:8], got[:8]):
        assert torch.equal(a.view(torch.int32) if a.dtype == torch.float32 else a, b.view(torch.int32) if b.dtype == torch.float32 else b)
    same_tensors(got[8], want[8], "register_sampled: score")
    same_tensors(got[9], want[9], "register_sampled: refine")
    c = mr.surface(600)
    src, tgt = dev(c["src"][None]), dev(c["tgt"][None])
    for kw in (dict(), dict(method="fgr"), dict(centre=True)):
        kw = dict(kw, k=20, trials=4096, seed=mr.SEED, refine=mr.MAX_DIST, refine_method="point_to_plane")
        if kw.get("method") == "fgr":
            del kw["trials"], kw["seed"]
        want = vcrnet_amd.register_features(src, tgt, mr.MAX_DIST, **kw)
        del entries[:]
        got = vcrnet_amd.register_features(src, tgt, mr.MAX_DIST, nn_search="grid", **kw)
        scans = searches(entries)
        assert "vcr_nn_score_grid" in scans and "vcr_refine_plane_grid" in scans and all(e.endswith("_grid") for e in scans), entries
        refined_want, refined_got = want.pop("refined"), got.pop("refined")
        same_tensors(got, want, ("register_features", kw))
        same_tensors(refined_got, refined_want, ("register_features: refined", kw))
