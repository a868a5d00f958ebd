"""vcr_support_normals_f32, vcr_support_spfh_f32, vcr_support_needed_f32 and vcr_support_fpfh_f32 on the GPU: normals and FPFH at
centres over a support cloud (include/support/vcr_hip_support.h), and the public calls on top of them --
``compute_fpfh_feature(queries= / query_index=)``, ``estimate_normals(queries=)``, ``register_features(describe="keypoints")``.

Everything is compared bit for bit, on int32 views: with the self form (``search="radius"``) where the centres are the cloud's own
points or a subset of them, with the numpy restatement (tests/support_restated.py) at positions that are not points, the two
plans with each other.  The one step whose last bit is the math library's is the first pass's atan2; tests/test_support_cpu.py
shows the recipe has no pair within 2^-30 of a bin edge (the cap is 0).  ``chain`` is the public call written out on the raw
bindings: every call in it runs with its outputs prefilled with the byte 0x5A and 64 elements of guard behind them, in the launch
form asked for, and is held to the public call's result."""
import functools

import numpy as np
import pytest
import torch

import fpfh_restated as fr
import rows_restated as wr
import support_restated as sr

pytestmark = pytest.mark.gpu

BYTE = 0x5A
GUARD = 64
FORMS = ("lane", "wave")
I32 = np.int32
B, N = wr.RAGGED


def mods():
    import vcrnet_amd
    from vcrnet_amd import rows, support
    return vcrnet_amd, support, rows


def dev(x):
    return torch.from_numpy(np.array(x, order="C")).cuda()              # (a copy: the shared cases are read-only)


def rows4(xyz):
    from vcrnet_amd import native
    return native.to_rows4(xyz)


def checked(out, raw, name):
    """The output as it is; all of it must have been overwritten, none of the band behind it."""
    torch.cuda.synchronize()
    buf, n = raw[name], out.numel()
    size = buf.element_size()
    band = buf[n:].view(torch.uint8).cpu().numpy()
    assert band.size == GUARD * size and (band == BYTE).all(), (name, "guard band written")
    body = buf[:n].view(torch.uint8).cpu().numpy().reshape(n, size)
    assert not (body == BYTE).all(axis=1).any(), (name, "element left unwritten")
    return out


def bits(a):
    a = np.ascontiguousarray(a.cpu().numpy() if torch.is_tensor(a) else a)
    return a.view(I32) if a.dtype.itemsize == 4 else a.view(np.uint8)       # (bool flags, 64-bit rows: their bytes)


def same(a, b, what):
    x, y = bits(a), bits(b)
    assert x.shape == y.shape and np.array_equal(x, y), (what, int((x != y).sum()) if x.shape == y.shape else (x.shape, y.shape))


def needed_of(x4, c4, csr, qi, max_nn):
    _, support, _ = mods()
    o = support.needed(x4, c4, *csr, self_index=qi, max_nn=max_nn, guard=GUARD, prefill=BYTE)
    return {k: checked(o[k], o["_raw"], k) for k in ("points", "count", "index", "slot")}


def chain(xyz, nrm, queries, qi, radius, max_nn=None, plan="all", variant=0, qn=None, capacity=(None, None)):
    """compute_fpfh_feature(xyz, nrm, queries=, query_index=qi, support=plan) on the raw bindings, guarded -> dict of tensors."""
    vcr, support, rows = mods()
    xyz = xyz.contiguous()
    x4, c4 = rows4(xyz), rows4(queries)
    kw = dict(guard=GUARD, prefill=BYTE)
    q_csr = vcr.search_radius(xyz, radius, queries=queries, capacity=capacity[0])
    o = {}
    if plan == "all":
        s_csr = vcr.search_radius(xyz, radius, capacity=capacity[1])
        if nrm is None:
            nrm = rows.normals(x4, *s_csr, max_nn=max_nn, want_curvature=False)[0]
        sup, slot = rows.spfh(x4, nrm, *s_csr, max_nn=max_nn, variant=variant), None
    else:
        need = needed_of(x4, c4, q_csr, qi, max_nn)
        n_csr = vcr.search_radius(xyz, radius, queries=need["points"], capacity=capacity[1])
        at = need["index"].clamp(min=0).long()
        n_nrm = torch.gather(nrm, 2, at[:, None, :].expand(-1, 3, -1)).contiguous()
        sup, raw = support.spfh(x4, nrm, rows4(need["points"]), n_nrm, *n_csr, self_index=need["index"], max_nn=max_nn,
                                variant=variant, **kw)
        sup, slot = checked(sup, raw, "spfh"), need["slot"]
        o["needed"] = need
    est, cur, raw = support.normals(x4, c4, *q_csr, max_nn=max_nn, **kw)
    o["estimated"], o["curvature"] = checked(est, raw, "normals"), checked(cur, raw, "curvature")
    if qn is None:
        qn = est
        if qi is not None:
            ok = (qi >= 0) & (qi < xyz.shape[2])
            at = torch.where(ok, qi, torch.zeros_like(qi)).long()
            qn = torch.where(ok[:, None, :], torch.gather(nrm, 2, at[:, None, :].expand(-1, 3, -1)), est)
    mine, raw = support.spfh(x4, nrm, c4, qn.contiguous(), *q_csr, self_index=qi, max_nn=max_nn, variant=variant, **kw)
    o["spfh"] = checked(mine, raw, "spfh")
    f, raw = support.fpfh(x4, c4, *q_csr, sup, o["spfh"], self_index=qi, slot=slot, max_nn=max_nn, **kw)
    o["fpfh"], o["normals"], o["q_csr"], o["support_spfh"] = checked(f, raw, "fpfh"), qn, q_csr, sup
    return o


@functools.lru_cache(maxsize=None)
def cloud():
    """(x [B,3,N] numpy, the device's normals of radius 0.335 as given normals): computed once, shared, read-only."""
    vcr, _, _ = mods()
    x = fr.cloud(B, N)
    x.setflags(write=False)
    nrm = vcr.estimate_normals(dev(x), search="radius", radius=0.335).cpu().numpy()
    nrm.setflags(write=False)
    return x, nrm


@functools.lru_cache(maxsize=None)
def whole(radius, max_nn, given):
    """compute_fpfh_feature(search="radius") of the whole cloud, and its normals: the self form every parity test compares with."""
    vcr, _, _ = mods()
    x, nrm = cloud()
    f, n = vcr.compute_fpfh_feature(dev(x), dev(nrm) if given else None, search="radius", radius=radius, max_nn=max_nn,
                                    want_normals=True)
    return f.cpu().numpy(), n.cpu().numpy()


# ------------------------------------------------------------------------------------------------------------- 1. self parity

@pytest.mark.parametrize("max_nn", [None, 5, 30])
@pytest.mark.parametrize("radius", sr.RADII)
def test_the_points_as_their_own_queries_return_the_self_form(radius, max_nn):
    vcr, support, _ = mods()
    x, nrm = cloud()
    xyz, me = dev(x), torch.arange(N, dtype=torch.int32, device="cuda").repeat(B, 1)
    for given in (True, False):
        want = whole(radius, max_nn, given)[0]
        for plan in ("all", "needed") if given else ("all",):
            got = vcr.compute_fpfh_feature(xyz, dev(nrm) if given else None, search="radius", radius=radius, max_nn=max_nn,
                                           queries=xyz, query_index=me, support=plan)
            same(got, want, (radius, max_nn, given, plan))
            for form in FORMS:
                same(chain(xyz, dev(nrm) if given else None, xyz, me, radius, max_nn, plan, form)["fpfh"], want,
                     (radius, max_nn, given, plan, form))
        same(vcr.compute_fpfh_feature(xyz, dev(nrm) if given else None, search="radius", radius=radius, max_nn=max_nn, query_index=me),
             want, (radius, max_nn, given, "no positions, the plan's choice"))
    if max_nn is None:
        n0, c0 = vcr.estimate_normals(xyz, search="radius", radius=radius, want_curvature=True)
        n1, c1 = vcr.estimate_normals(xyz, search="radius", radius=radius, want_curvature=True, queries=xyz)
        same(n1, n0, radius)
        same(c1, c0, radius)
        view = dev(np.asarray([[0.5, 0.5, 3.0], [-2.0, 0.5, 0.5]], np.float32))
        same(vcr.estimate_normals(xyz, search="radius", radius=radius, viewpoint=view, queries=xyz),
             vcr.estimate_normals(xyz, search="radius", radius=radius, viewpoint=view), (radius, "viewpoint"))


# ----------------------------------------------------------------------------------------------------------------- 2. subsets

@pytest.mark.parametrize("radius", sr.RADII)
def test_a_subset_of_indices_returns_the_whole_clouds_columns(radius):
    vcr, _, _ = mods()
    x, nrm = cloud()
    xyz = dev(x)
    at = np.stack([sr.subset(N, seed=11 + b) for b in range(B)])
    qi = dev(at)
    for max_nn in (None, 5):
        for given in (True, False):
            want = whole(radius, max_nn, given)[0]
            want = np.stack([np.where(at[b][None, :] >= 0, want[b][:, np.maximum(at[b], 0)], np.nan) for b in range(B)]).astype(np.float32)
            for plan in ("all", "needed") if given else ("all",):
                got = vcr.compute_fpfh_feature(xyz, dev(nrm) if given else None, search="radius", radius=radius, max_nn=max_nn,
                                               query_index=qi, support=plan).cpu().numpy()
                assert np.isnan(got[:, :, 9]).all() and got.shape == (B, 33, 37)
                ok = ~np.isnan(want)
                assert np.array_equal(np.isnan(got), ~ok) and np.array_equal(bits(got)[ok], bits(want)[ok]), (radius, max_nn, given, plan)
                for form in FORMS:
                    o = chain(xyz, dev(nrm) if given else None, vcr.support.gather_positions(xyz, qi), qi, radius, max_nn, plan, form)
                    same(o["fpfh"], got, (radius, max_nn, given, plan, form))


# ----------------------------------------------------------------------------------------------------- 3. arbitrary positions

@functools.lru_cache(maxsize=None)
def support_side(radius, b):
    """rows_restated's histograms of cloud b's own points on the device's self rows: shared by every case of (radius, b)."""
    vcr, _, _ = mods()
    x, nrm = cloud()
    s_csr = [t[0].cpu().numpy() for t in vcr.search_radius(dev(x[b][None]), radius)]
    return wr.spfh(x[b], nrm[b], s_csr[0], s_csr[1])


@functools.lru_cache(maxsize=None)
def restated(name, M, radius, b):
    """One cloud's centres and the restatement's answer on the DEVICE's rows (the searches have their own tests): shared."""
    vcr, _, _ = mods()
    x, nrm = cloud()
    c = sr.centres(x[b], name, M, seed=b)
    qi = None
    if name == "jitter" and M > 1:                           # a centre ON a point without an index, and one with it
        c[:, 1], c[:, 2] = x[b][:, 17], x[b][:, 40]
        qi = np.full(M, -1, np.int32)
        qi[2] = 40
    xyz, q = dev(x[b][None]), dev(c[None])
    q_csr = [t[0].cpu().numpy() for t in vcr.search_radius(xyz, radius, queries=q)]
    f, qn, mine = sr.feature(x[b], nrm[b], c, q_csr[:2], None, qi, support_spfh=support_side(radius, b))
    n, cv = sr.normals(x[b], c, q_csr[0], q_csr[1], qi)
    need = sr.needed(x[b], c, q_csr[0], q_csr[1], qi)
    return c, qi, {"fpfh": f, "normals": qn, "spfh": mine.astype(I32), "estimated": n, "curvature": cv, "needed": need}


@pytest.mark.parametrize("M", [1, 333])
@pytest.mark.parametrize("radius", sr.RADII)
@pytest.mark.parametrize("name", sr.CENTRES)
def test_positions_that_are_not_points_return_the_restatement(name, radius, M):
    vcr, support, _ = mods()
    x, nrm = cloud()
    for b in range(B):
        c, qi, want = restated(name, M, radius, b)
        xyz, q, n = dev(x[b][None]), dev(c[None]), dev(nrm[b][None])
        di = None if qi is None else dev(qi[None])
        for plan in ("all", "needed"):
            for form in FORMS + (0,):
                o = chain(xyz, n, q, di, radius, None, plan, form)
                for k in ("fpfh", "normals", "spfh", "estimated", "curvature"):
                    same(o[k][0], want[k], (name, radius, M, b, plan, form, k))
                if plan == "needed":
                    for k in ("points", "index", "slot"):
                        same(o["needed"][k][0], want["needed"][k], (name, radius, M, b, k))
                    assert int(o["needed"]["count"][0]) == want["needed"]["count"]
            same(vcr.compute_fpfh_feature(xyz, n, search="radius", radius=radius, queries=q, query_index=di, support=plan)[0],
                 want["fpfh"], (name, radius, M, b, plan, "public"))
        ne, cu = vcr.estimate_normals(xyz, search="radius", radius=radius, queries=q, want_curvature=True)
        if qi is None:                                       # (estimate_normals takes no index: every entry is a neighbour)
            same(ne[0], want["estimated"], (name, radius, M, b))
            same(cu[0], want["curvature"], (name, radius, M, b))
        if name == "nonfinite":
            assert np.isnan(o["fpfh"][0].cpu().numpy()[:, 0]).all() and not o["spfh"][0, 0].any()
    cap = int(o["q_csr"][0].shape[1])                         # few centres: the plan's form (variant 0 above) was the wave's
    many = 128 * M > support.WAVE_CENTRES                     # (a batch of 128 such clouds: the row length decides)
    assert support.form(1, N, M, cap) == 2 and support.form(128, N, M, cap) == (1 if many and cap // M < support.WAVE_SPFH else 2)


def test_the_plans_form_is_lane_for_many_short_rows_and_wave_otherwise():
    """Many centres with short rows take the lane form, by the plan and on the device: a batch of 128 copies (B * M above
    VCR_SUPPORT_WAVE_CENTRES) returns the single cloud's bits under variant 0, "lane" and "wave"."""
    vcr, support, _ = mods()
    x, nrm = cloud()
    q = sr.centres(x[0], "jitter", 333)
    Bm = 128
    assert Bm * 333 > support.WAVE_CENTRES
    xyz, n, qq = dev(x[0][None]).repeat(Bm, 1, 1), dev(nrm[0][None]).repeat(Bm, 1, 1), dev(q[None]).repeat(Bm, 1, 1)
    for radius, want in ((0.1, 1), (0.335, 2)):
        one = chain(xyz[:1], n[:1], qq[:1], None, radius, None, "all", 0)
        cap = one["q_csr"][0].shape[1]
        assert support.form(Bm, N, 333, cap) == want and support.form(1, N, 333, cap) == 2
        for form in (0,) + FORMS:
            o = chain(xyz, n, qq, None, radius, None, "all", form)
            for b in (0, 77, Bm - 1):
                same(o["spfh"][b], one["spfh"][0], (radius, form, b))
                same(o["fpfh"][b], one["fpfh"][0], (radius, form, b))


# ------------------------------------------------------------------------------------------------------------------ 4. needed

def test_needed_against_numpy_and_every_point_needed():
    vcr, support, rows = mods()
    x, nrm = cloud()
    xyz, n = dev(x), dev(nrm)
    x4 = rows4(xyz)
    me = torch.arange(N, dtype=torch.int32, device="cuda").repeat(B, 1)
    for radius, max_nn in ((0.1, None), (0.335, None), (0.335, 3)):
        q_csr = vcr.search_radius(xyz, radius, queries=xyz)
        need = needed_of(x4, x4, q_csr, me, max_nn)
        for b in range(B):
            want = sr.needed(x[b], x[b], q_csr[0][b].cpu().numpy(), q_csr[1][b].cpu().numpy(), np.arange(N), max_nn or 0)
            for k in ("points", "index", "slot"):
                same(need[k][b], want[k], (radius, max_nn, b, k))
            assert int(need["count"][b]) == want["count"]
        every = radius == 0.335 and max_nn is None           # every point is somebody's neighbour: slot is the identity
        if every:
            assert (need["count"] == N).all() and (need["slot"] == me).all() and (need["index"] == me).all()
        else:
            assert (need["count"] < N).any()                 # (short or cut rows: some point is in nobody's)
        # call 2 on the needed points' own rows is rows.spfh on the self rows, at the needed points
        s_csr = vcr.search_radius(xyz, radius)
        n_csr = vcr.search_radius(xyz, radius, queries=need["points"])
        at = need["index"].clamp(min=0).long()
        n_nrm = torch.gather(n, 2, at[:, None, :].expand(-1, 3, -1)).contiguous()
        for form in FORMS:
            sp, raw = support.spfh(x4, n, rows4(need["points"]), n_nrm, *n_csr, self_index=need["index"], max_nn=max_nn,
                                   variant=form, guard=GUARD, prefill=BYTE)
            sp, whole_sp = checked(sp, raw, "spfh"), rows.spfh(x4, n, *s_csr, max_nn=max_nn, variant=form)
            if every:
                same(sp, whole_sp, (radius, max_nn, form))
            for b in range(B):
                c = int(need["count"][b])
                same(sp[b, :c], whole_sp[b, need["index"][b, :c].long()], (radius, max_nn, form, b))
                assert not sp[b, c:].any()                   # (the padding: NaN centres, zero words)


# -------------------------------------------------------------------------------------------------------------- 5. not served

def test_a_cloud_whose_rows_do_not_fit_comes_back_nan_and_leaves_the_other_alone():
    vcr, _, _ = mods()
    x, nrm = cloud()
    radius = 0.335
    c = np.stack([sr.centres(x[b], "outside", 37, seed=b) for b in range(B)])   # cloud 0: mostly empty rows, few points needed
    c[1] = x[1][:, :37]                                      # cloud 1's centres: points, so that its rows are the longer ones
    xyz, n, q = dev(x), dev(nrm), dev(c)
    alone = vcr.compute_fpfh_feature(xyz[:1], n[:1], search="radius", radius=radius, queries=q[:1], support="needed")
    q_tot = vcr.search_radius(xyz, radius, queries=q)[2].cpu().numpy()
    assert q_tot[0] < q_tot[1]
    need = vcr.support.needed(rows4(xyz), rows4(q), *vcr.search_radius(xyz, radius, queries=q))
    n_tot = vcr.search_radius(xyz, radius, queries=need["points"])[2].cpu().numpy()
    s_tot = vcr.search_radius(xyz, radius)[2].cpu().numpy()
    assert n_tot[0] < n_tot[1] and s_tot[0] < s_tot[1]
    fits = int(q_tot[1])
    cases = (("needed", (int(q_tot[0]), int(n_tot[1]))),     # cloud 1's QUERY rows exceed the first capacity
             ("needed", (fits, int(n_tot[0]))),              # only its NEEDED rows exceed the second
             ("all", (int(q_tot[0]), int(s_tot[1]))), ("all", (fits, int(s_tot[0]))))
    for plan, cap in cases:
        got = vcr.compute_fpfh_feature(xyz, n, search="radius", radius=radius, queries=q, support=plan, capacity=cap)
        torch.cuda.synchronize()
        assert torch.isnan(got[1]).all(), (plan, cap)
        same(got[0], alone[0], (plan, cap))
        for form in FORMS:
            o = chain(xyz, n, q, None, radius, None, plan, form, capacity=cap)
            same(o["fpfh"][0], alone[0], (plan, cap, form))
            if cap[0] < fits:                                # the raw calls void the cloud themselves where the centres' rows did not fit
                assert torch.isnan(o["fpfh"][1]).all() and torch.isnan(o["estimated"][1]).all() and not o["spfh"][1].any()
                if plan == "needed":
                    assert int(o["needed"]["count"][1]) == 0 and (o["needed"]["slot"][1] == -1).all()
    one = vcr.compute_fpfh_feature(xyz, n, search="radius", radius=radius, queries=q, capacity=int(max(q_tot[1], n_tot[1], s_tot[1])))
    same(one[0], alone[0], "an int for both searches")
    assert not torch.isnan(one[1]).any()
    ne = vcr.estimate_normals(xyz, search="radius", radius=radius, queries=q, capacity=int(q_tot[0]))
    assert torch.isnan(ne[1]).all() and not torch.isnan(ne[0]).any()


# ------------------------------------------------------------------------------------------------------------------- 6. batch

def test_a_cloud_alone_equals_the_same_cloud_in_a_batch_of_three():
    vcr, _, _ = mods()
    x, nrm = cloud()
    radius = 0.335
    c = [sr.centres(x[0], "jitter", 333), sr.centres(x[1], "outside", 333, seed=1), sr.centres(x[0], "nonfinite", 333, seed=2)]
    xs, ns = np.stack([x[0], x[1], x[0]]), np.stack([nrm[0], nrm[1], nrm[0]])
    xyz, n, q = dev(xs), dev(ns), dev(np.stack(c))
    for plan in ("all", "needed"):
        for max_nn in (None, 30):
            got = {form: chain(xyz, n, q, None, radius, max_nn, plan, form) for form in FORMS + (0,)}
            for k in ("fpfh", "spfh", "estimated", "curvature"):
                same(got["lane"][k], got["wave"][k], (plan, max_nn, k, "forms"))
                same(got["lane"][k], got[0][k], (plan, max_nn, k, "the plan's form"))
            same(vcr.compute_fpfh_feature(xyz, n, search="radius", radius=radius, max_nn=max_nn, queries=q, support=plan),
                 got[0]["fpfh"], (plan, max_nn, "public"))
            for b in range(3):
                one = chain(xyz[b:b + 1], n[b:b + 1], q[b:b + 1], None, radius, max_nn, plan, 0)
                for k in ("fpfh", "spfh", "estimated", "curvature"):
                    same(one[k][0], got[0][k][b], (plan, max_nn, b, k))
    same(vcr.compute_fpfh_feature(xyz, n, search="radius", radius=radius, queries=q, support="all"),
         vcr.compute_fpfh_feature(xyz, n, search="radius", radius=radius, queries=q, support="needed"), "the two plans")


# ------------------------------------------------------------------------------------------------------- 7. register_features

@functools.lru_cache(maxsize=None)
def pair():
    """match_restated's surface recipe (600 points over the unit square and a moved, permuted copy), the ISS options of
    tests/test_hip_iss.py (default radii) and a feature radius of about twenty neighbours."""
    import match_restated as mr
    c = mr.surface(600)
    return c["src"][None], c["tgt"][None], dict(gamma_21=0.8, gamma_32=0.8, min_neighbors=4)


FEAT = dict(search="radius", radius=0.12, max_nn=30)


def _equal_results(a, b, what):
    assert set(a) == set(b), what
    for k in a:
        same(a[k], b[k], (what, k))


@pytest.mark.parametrize("method", ["ransac", "fgr"])
def test_describing_the_keypoints_alone_registers_as_describing_all(method):
    vcr, _, _ = mods()
    src, tgt, iss = pair()
    s, t = dev(src), dev(tgt)
    kw = dict(keypoints="iss", iss=iss, method=method, mutual=False, **FEAT)
    if method == "ransac":
        kw.update(trials=2048, seed=7)
    a = vcr.register_features(s, t, 0.05, describe="all", **kw)
    b = vcr.register_features(s, t, 0.05, describe="keypoints", **kw)
    _equal_results(a, b, method)
    count = vcr.compute_iss_keypoints(s, **iss)[1]
    assert 2 <= int(count[0]) < 600 and int((b["corr"] >= 0).sum()) <= int(count[0])
    a = vcr.register_features(s, t, 0.05, describe="all", orient="tangent", **kw)
    b = vcr.register_features(s, t, 0.05, describe="keypoints", orient="tangent", **kw)
    _equal_results(a, b, (method, "tangent"))                # both runs take the keypoints' features


def test_mutual_matches_among_the_keypoints_are_the_public_pieces_composed():
    vcr, _, _ = mods()
    src, tgt, iss = pair()
    s, t = dev(src), dev(tgt)
    feat = FEAT
    res = vcr.register_features(s, t, 0.05, describe="keypoints", keypoints="iss", iss=iss, mutual=True, trials=500, **feat)
    _, count, index = vcr.compute_iss_keypoints(s, **iss)
    f_src = vcr.compute_fpfh_feature(s, query_index=index, **feat)
    f_tgt = vcr.compute_fpfh_feature(t, **feat)
    m = vcr.match_features(f_src, f_tgt, mutual=True).cpu().numpy()
    index, count = index.cpu().numpy(), count.cpu().numpy()
    want = np.full(src.shape[::2], -1, np.int32)
    for b in range(1):
        assert (m[b, count[b]:] == -1).all()                 # a NaN feature never wins
        want[b, index[b, :count[b]]] = m[b, :count[b]]
    same(res["corr"], want, "corr")
    whole_corr = vcr.register_features(s, t, 0.05, describe="all", keypoints="iss", iss=iss, mutual=True, trials=500, **feat)["corr"]
    assert ((whole_corr.cpu().numpy() >= 0) <= (want >= 0)).all()    # "all" asks more of a pair: it keeps no pair this one drops
