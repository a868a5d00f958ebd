"""vcr_rows_normals_f32, vcr_rows_spfh_f32 and vcr_rows_fpfh_f32 on the GPU: normals and FPFH over ragged CSR rows
(include/ext/vcr_hip_rows.h).

Everything is compared bit for bit, on int32 views: with the fixed-width kernels on a fixed-width list written as rows, with the
numpy restatement (tests/rows_restated.py) on real rows from ``search_radius``, rows cut by max_nn with rows cut by torch ops, the
hybrid neighbourhood with the existing hybrid path.  The one step whose last bit is the math library's is the first pass's atan2:
a pair within 2^-30 of a bin edge would be excluded, and tests/test_rows_cpu.py shows the recipe has none (the cap is 0).  Every
call runs with its outputs prefilled with the byte 0x5A and 64 elements of guard behind them, and every test that has two launch
forms runs in both."""
import functools

import numpy as np
import pytest
import torch

import fpfh_restated as fr
import grid_restated as gr
import radius_restated as rr
import refine_restated as fr_pair
import rows_restated as wr

pytestmark = pytest.mark.gpu

BYTE = 0x5A
GUARD = 64
FORMS = ("lane", "wave")
I32 = np.int32


def mods():
    import vcrnet_amd
    from vcrnet_amd import rows
    return vcrnet_amd, rows


def dev(x):
    return torch.from_numpy(np.array(x, order="C")).cuda()              # (a copy: the shared cases are read-only)


def checked(out, raw, name):
    """The output as numpy; all of it must have been overwritten, none of the band behind it."""
    torch.cuda.synchronize()
    buf, n = raw[name], out.numel()
    size = buf.element_size()
    band = buf[n:].view(torch.uint8).cpu().numpy()
    assert band.size == GUARD * size and (band == BYTE).all(), (name, "guard band written")
    body = buf[:n].view(torch.uint8).cpu().numpy().reshape(n, size)
    assert not (body == BYTE).all(axis=1).any(), (name, "element left unwritten")
    return out.cpu().numpy()


def run(x4, csr, normals=None, max_nn=None, variant=0, viewpoint=None):
    """The three calls on xyz4 and the rows -> dict of numpy: normals, curvature (the rows' own), spfh (from `normals` where
    given, else from the rows' normals) and fpfh."""
    _, rows = mods()
    n, c, raw = rows.normals(x4, *csr, max_nn=max_nn, viewpoint=viewpoint, guard=GUARD, prefill=BYTE)
    out = {"normals": checked(n, raw, "normals"), "curvature": checked(c, raw, "curvature")}
    use = n if normals is None else normals
    sp, raw = rows.spfh(x4, use, *csr, max_nn=max_nn, variant=variant, guard=GUARD, prefill=BYTE)
    out["spfh"] = checked(sp, raw, "spfh")
    f, raw = rows.fpfh(x4, *csr, sp, max_nn=max_nn, variant=variant, guard=GUARD, prefill=BYTE)
    out["fpfh"] = checked(f, raw, "fpfh")
    return out


def same(a, b, what, keys=("normals", "curvature", "spfh", "fpfh")):
    for k in keys:
        x, y = np.ascontiguousarray(a[k]).view(I32), np.ascontiguousarray(b[k]).view(I32)
        assert np.array_equal(x, y), (what, k, int((x != y).sum()))


def rows4(xyz):
    from vcrnet_amd import native
    return native.to_rows4(xyz)


def dense_csr(idx):
    """idx [B,N,k] (device) -> the same lists as rows: row_start = i k."""
    B, N, k = idx.shape
    row_start = (torch.arange(N + 1, device=idx.device, dtype=torch.int64) * k).repeat(B, 1)
    return idx.reshape(B, N * k).contiguous(), row_start, torch.full((B,), N * k, dtype=torch.int64, device=idx.device)


def restated(x, idx, row_start, nrm=None, max_nn=0, viewpoint=None):
    """One cloud by tests/rows_restated.py -> the dict `run` returns for it (spfh from nrm where given)."""
    n, cv, _, _ = wr.normals(x, idx, row_start, max_nn, viewpoint)
    sp = wr.spfh(x, n if nrm is None else nrm, idx, row_start, max_nn)
    return {"normals": n, "curvature": cv, "spfh": sp.astype(I32), "fpfh": wr.fpfh(x, idx, row_start, sp, max_nn)}


def void(o, b, what):
    """Cloud b was not served: NaN normals, curvature and fpfh, zero spfh words."""
    assert np.isnan(o["normals"][b]).all() and np.isnan(o["curvature"][b]).all() and np.isnan(o["fpfh"][b]).all(), what
    assert not o["spfh"][b].any(), what


# ------------------------------------------------------------------------------------------ parity with the fixed-width kernels

@pytest.mark.parametrize("k", [2, 20, 62])
def test_a_fixed_width_list_as_rows_returns_the_fixed_width_kernels_bits(k):
    vcrnet_amd, rows = mods()
    from vcrnet_amd import fpfh, plane
    B, N = 2, 300
    xyz = dev(fr.cloud(B, N))
    x4 = rows4(xyz)
    idx = vcrnet_amd.search_knn(xyz, k)
    csr = dense_csr(idx)
    view = dev(np.asarray([[0.5, 0.5, 3.0], [-2.0, 0.5, 0.5]], np.float32))
    for vp in (None, view):
        n0, c0 = plane.normals(x4, idx, vp)
        n1, c1, raw = rows.normals(x4, *csr, viewpoint=vp, guard=GUARD, prefill=BYTE)
        same({"normals": n0.cpu().numpy(), "curvature": c0.cpu().numpy()},
             {"normals": checked(n1, raw, "normals"), "curvature": checked(c1, raw, "curvature")}, (k, vp is None),
             ("normals", "curvature"))
    nrm = plane.normals(x4, idx)[0]
    sp0 = fpfh.spfh(x4, nrm, idx)
    f0 = fpfh.fpfh(x4, idx, sp0)
    wide = sp0.cpu().numpy().reshape(B, N, 3, 16)
    assert not wide[..., 12:].any()
    for form in FORMS:
        o = run(x4, csr, variant=form)
        assert np.array_equal(o["spfh"], wide[..., :12].astype(I32)), (k, form)
        same(o, {"fpfh": f0.cpu().numpy()}, (k, form), ("fpfh",))
        assert o["spfh"][..., 11].max() == k


# -------------------------------------------------------------------------------------- the restatement on real ragged rows

@functools.lru_cache(maxsize=None)
def ragged(radius):
    """(x [B,3,N], the definition's rows per cloud, the restated results per cloud) at one radius: computed once, shared."""
    B, N = wr.RAGGED
    x = fr.cloud(B, N)
    res = [rr.radius_rows(x[b], radius) for b in range(B)]
    want = [restated(x[b], res[b]["idx"], res[b]["row_start"]) for b in range(B)]
    x.setflags(write=False)
    return x, res, want


def test_the_recipe_has_the_row_lengths_it_is_there_for():
    lens = set()
    for radius in wr.RAGGED_RADII:
        lens |= {int(c) for r in ragged(radius)[1] for c in r["count"]}
    assert set(wr.WANTED_LENGTHS) <= lens and max(lens - {wr.RAGGED[1] - 1}) > 255 and wr.RAGGED[1] - 1 in lens, sorted(lens)
    assert (ragged(wr.RAGGED_RADII[-1])[1][0]["count"] == wr.RAGGED[1] - 1).all()


@pytest.mark.parametrize("radius", wr.RAGGED_RADII)
def test_search_radius_rows_against_the_restatement(radius):
    """The device's own rows (they are the definition's: asserted), then the three calls in both forms against the restatement:
    normals, curvature and the second pass bit for bit, the counts equal (no excluded pair on this recipe)."""
    vcrnet_amd, _ = mods()
    x, res, want = ragged(radius)
    xyz = dev(x)
    csr = vcrnet_amd.search_radius(xyz, radius)
    cap = csr[0].shape[1]
    assert cap == max(r["total"] for r in res)
    for b, r in enumerate(res):
        assert np.array_equal(csr[0][b].cpu().numpy(), rr.padded(r, cap)[0]) and np.array_equal(csr[1][b].cpu().numpy(), r["row_start"])
    x4 = rows4(xyz)
    for form in FORMS:
        o = run(x4, csr, variant=form)
        for b in range(len(res)):
            same({k: v[b] for k, v in o.items()}, want[b], (radius, form, b))


# ------------------------------------------------------------------------------------------------------------ cutting the rows

def cut_rows(csr, m):
    """Every row's first min(n_i, m) entries as rows of their own, by torch ops."""
    idx, row_start, _ = csr
    B, N = row_start.shape[0], row_start.shape[1] - 1
    L = torch.clamp(row_start[:, 1:] - row_start[:, :-1], max=m)
    new_start = torch.zeros_like(row_start)
    torch.cumsum(L, dim=1, out=new_start[:, 1:])
    total = new_start[:, N].clone()
    cap = int(total.max())
    out = torch.full((B, cap), -1, dtype=torch.int32, device=idx.device)
    for b in range(B):
        p = torch.arange(int(total[b]), device=idx.device)
        i = torch.searchsorted(new_start[b], p, right=True) - 1
        out[b, :int(total[b])] = idx[b, row_start[b, i] + (p - new_start[b, i])]
    return out, new_start, total


@pytest.mark.parametrize("form", FORMS)
def test_max_nn_is_the_call_on_cut_rows(form):
    vcrnet_amd, _ = mods()
    radius = wr.RAGGED_RADII[1]                              # rows of up to 133 entries
    x, res, _ = ragged(radius)
    xyz = dev(x)
    x4 = rows4(xyz)
    csr = vcrnet_amd.search_radius(xyz, radius)
    longest = max(int(r["count"].max()) for r in res)
    assert longest > 100
    for m in (1, 2, 30, 100):
        cut = cut_rows(csr, m)
        assert int(cut[2].max()) < csr[0].shape[1]
        same(run(x4, csr, max_nn=m, variant=form), run(x4, cut, variant=form), (form, m))
    whole = run(x4, csr, variant=form)
    for m in (longest, longest + 1, 1 << 20):
        same(run(x4, csr, max_nn=m, variant=form), whole, (form, m))


def test_the_hybrid_neighbourhood_is_the_existing_hybrid_path():
    """Coordinates on the 2^-6 lattice inside (-4, 4): every d2 is exact in fp32 and fp64, so the fixed-width path's fp64 sphere
    test and the search's fp32 one agree, and with GIVEN normals the two features are the same bits."""
    vcrnet_amd, _ = mods()
    x = wr.exact_cloud()
    radius, m = 2.25, 30
    counts = np.concatenate([rr.radius_rows(c, radius)["count"] for c in x])
    assert (counts < m).any() and (counts > m).any() and (counts > 0).all()
    rs = np.random.RandomState(11)
    nrm = rs.normal(size=x.shape).astype(np.float32)
    nrm /= np.linalg.norm(nrm, axis=1, keepdims=True)
    xyz, nrm = dev(x), dev(nrm)
    old = vcrnet_amd.compute_fpfh_feature(xyz, nrm, k=m, radius=radius, search="grid")
    new = vcrnet_amd.compute_fpfh_feature(xyz, nrm, search="radius", radius=radius, max_nn=m)
    assert torch.equal(old.view(torch.int32), new.view(torch.int32))


# ----------------------------------------------------------------------------------------------------------------------- edges

@pytest.mark.parametrize("form", FORMS)
def test_one_point_two_points_and_rows_built_by_hand(form):
    vcrnet_amd, _ = mods()
    for N in (1, 2):
        x = fr.cloud(2, 300)[:, :, :N].copy()
        xyz = dev(x)
        csr = vcrnet_amd.search_radius(xyz, 10.0)
        assert csr[0].shape[1] == N * (N - 1)
        o = run(rows4(xyz), csr, variant=form)
        for b in range(2):
            res = rr.radius_rows(x[b], 10.0)
            same({k: v[b] for k, v in o.items()}, restated(x[b], res["idx"], res["row_start"]), (form, N, b))
        assert (o["normals"] == np.asarray([0, 0, 1], np.float32)[None, :, None]).all() and not o["curvature"].any()
    # copies of the query (d2 = 0), -1 and an index past N (both read as the query), an empty row, slots behind total
    x = np.asarray([[0, 1, 1, 2, 4, 1], [0, 0, 0, 0, 0, 1], [0, 0, 0, 0, 0, 0.5]], np.float32)
    lists = [[1, 2, 5, 3], [2, 0, 5], [], [1], [-1, 3, 99, 0], [0, 1, 2, 3, 4, 5]]
    idx = np.asarray([e for r in lists for e in r] + [7, -5], I32)
    row_start = np.cumsum([0] + [len(r) for r in lists]).astype(np.int64)
    nrm = np.tile(np.asarray([[0], [0], [1]], np.float32), (1, 6))
    csr = (dev(idx[None]), dev(row_start[None]), dev(np.asarray([row_start[-1]], np.int64)))
    for m in (None, 2):
        o = run(rows4(dev(x[None])), csr, normals=dev(nrm[None]), max_nn=m, variant=form)
        same({k: v[0] for k, v in o.items()}, restated(x, idx, row_start, nrm, m or 0), (form, m))
    assert o["normals"][0, :, 2].tolist() == [0, 0, 1]


@pytest.mark.parametrize("form", FORMS)
def test_a_point_that_is_not_finite_has_an_empty_row_and_is_in_nobodys(form):
    vcrnet_amd, _ = mods()
    N = 300
    x = gr.RECIPES["nonfinite"](N, seed=N)
    radius = 0.5
    res = rr.radius_rows(x, radius)
    bad = np.flatnonzero(~gr.finite(x))
    assert len(bad) >= 3 and (res["count"][bad] == 0).all() and not np.isin(res["idx"], bad).any() and res["count"].max() >= 5
    xyz = dev(x[None])
    csr = vcrnet_amd.search_radius(xyz, radius)
    assert np.array_equal(csr[0][0].cpu().numpy(), res["idx"]) and np.array_equal(csr[1][0].cpu().numpy(), res["row_start"])
    o = run(rows4(xyz), csr, variant=form)
    same({k: v[0] for k, v in o.items()}, restated(x, res["idx"], res["row_start"]), form)
    assert (o["normals"][0][:, bad] == np.asarray([[0], [0], [1]], np.float32)).all() and not o["spfh"][0][bad].any()


@pytest.mark.parametrize("form", FORMS)
def test_a_cloud_that_is_not_served_comes_back_void_and_leaves_the_others_alone(form):
    """total[b] > capacity (search_radius' "does not fit": every idx -1), and a row_start that does not ascend from 0 to total:
    that cloud is NaN / zero, the others are the bits of their single-cloud call."""
    vcrnet_amd, _ = mods()
    B, N, radius = 3, 300, 0.2
    x = fr.cloud(B, N)
    totals = [rr.radius_rows(x[b], radius)["total"] for b in range(B)]
    order = np.argsort(totals)
    assert totals[order[1]] < totals[order[2]]
    cap = int(totals[order[2]]) - 1                          # the cloud with the most neighbours does not fit
    xyz = dev(x)
    x4 = rows4(xyz)
    csr = vcrnet_amd.search_radius(xyz, radius, capacity=cap)
    big = int(order[2])
    assert int(csr[2][big]) == totals[big] > cap and (csr[0][big] == -1).all()
    alone = []
    for b in range(B):
        one = vcrnet_amd.search_radius(xyz[b:b + 1], radius, capacity=cap)
        alone.append(run(x4[b:b + 1], one, variant=form))
    o = run(x4, csr, variant=form)
    void(o, big, "does not fit")
    void(alone[big], 0, "does not fit, alone")
    for b in set(range(B)) - {big}:
        same({k: v[b] for k, v in o.items()}, {k: v[0] for k, v in alone[b].items()}, (form, b))
    fits = vcrnet_amd.search_radius(xyz, radius)
    whole = run(x4, fits, variant=form)
    assert np.isfinite(whole["fpfh"]).all()
    for what, edit in (("descends", lambda rs, tot: rs.__setitem__((1, 150), rs[1, 149] - 1)),
                       ("does not start at 0", lambda rs, tot: rs.__setitem__((1, 0), 1)),
                       ("does not end at total", lambda rs, tot: tot.__setitem__(1, tot[1] + 1)),
                       ("negative", lambda rs, tot: rs.__setitem__((1, 0), -4)),
                       ("total above capacity", lambda rs, tot: tot.__setitem__(1, fits[0].shape[1] + 1))):
        rs, tot = fits[1].clone(), fits[2].clone()
        edit(rs, tot)
        got = run(x4, (fits[0], rs, tot), variant=form)
        void(got, 1, what)
        for b in (0, 2):
            same({k: v[b] for k, v in got.items()}, {k: v[b] for k, v in whole.items()}, (form, what, b))


# ------------------------------------------------------------------------------------------------- independence of the launch

def test_a_batch_is_its_clouds_and_the_two_forms_are_the_same_bits():
    vcrnet_amd, _ = mods()
    B, N, radius = 3, 257, 0.25
    x = fr.cloud(B, N)
    xyz = dev(x)
    x4 = rows4(xyz)
    view = dev(np.asarray([[0.5, 0.5, 3.0]] * B, np.float32))
    csr = vcrnet_amd.search_radius(xyz, radius)
    assert int((csr[1][:, 1:] - csr[1][:, :-1]).max()) > 64
    got = {form: run(x4, csr, variant=form, viewpoint=view) for form in FORMS + (0,)}
    same(got["lane"], got["wave"], "forms")
    same(got["lane"], got[0], "the plan's form")
    for b in range(B):
        one = tuple(t[b:b + 1] for t in csr)
        for form in FORMS:
            same({k: v[b] for k, v in got[form].items()}, {k: v[0] for k, v in run(x4[b:b + 1], one, variant=form, viewpoint=view[b:b + 1]).items()},
                 (form, b))


# ------------------------------------------------------------------------------------------------------------- the public calls

def test_the_public_calls_are_their_staged_calls():
    vcrnet_amd, rows = mods()
    B, N, radius = 2, 300, 0.2
    xyz = dev(fr.cloud(B, N))
    x4 = rows4(xyz)
    csr = vcrnet_amd.search_radius(xyz, radius)
    cap = csr[0].shape[1]
    eq = lambda a, b: torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))    # noqa: E731
    for m in (None, 7, 100):
        n0, c0 = rows.normals(x4, *csr, max_nn=m)
        f0 = rows.fpfh(x4, *csr, rows.spfh(x4, n0, *csr, max_nn=m), max_nn=m)
        for capacity in (None, cap, cap + 17):
            kw = dict(search="radius", radius=radius, max_nn=m, capacity=capacity)
            n, c, got = vcrnet_amd.estimate_normals(xyz, want_curvature=True, want_idx=True, **kw)
            assert eq(n, n0) and eq(c, c0) and len(got) == 3 and got[0].shape[1] == (cap if capacity is None else capacity)
            assert eq(got[0][:, :cap], csr[0]) and eq(got[1], csr[1]) and eq(got[2], csr[2])
            assert eq(vcrnet_amd.estimate_normals(xyz, k=5, **kw), n0)                       # (k is not read)
            f, n, got = vcrnet_amd.compute_fpfh_feature(xyz, want_normals=True, want_idx=True, **kw)
            assert eq(f, f0) and eq(n, n0) and eq(got[1], csr[1])
            given = torch.flip(n0, dims=[2]).contiguous()
            f1 = rows.fpfh(x4, *csr, rows.spfh(x4, given, *csr, max_nn=m), max_nn=m)
            assert eq(vcrnet_amd.compute_fpfh_feature(xyz, given, **kw), f1) and not eq(f1, f0)
    view = dev(np.asarray([[0.5, 0.5, 3.0]] * B, np.float32))
    assert eq(vcrnet_amd.estimate_normals(xyz, viewpoint=view, search="radius", radius=radius), rows.normals(x4, *csr, viewpoint=view)[0])
    # a capacity below a cloud's total: that cloud is NaN, nothing is raised
    short = vcrnet_amd.compute_fpfh_feature(xyz, search="radius", radius=radius, capacity=int(csr[2].min()) - 1)
    assert torch.isnan(short).all()


def test_the_default_calls_return_what_they_returned():
    """estimate_normals and compute_fpfh_feature without the new keywords, against the staged calls of the fixed-width path."""
    vcrnet_amd, _ = mods()
    from vcrnet_amd import fpfh, native, plane
    xyz = dev(fr.cloud(2, 300))
    x4 = rows4(xyz)
    eq = lambda a, b: torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))    # noqa: E731
    idx = native.knn(x4, None, 20)
    n0, c0 = plane.normals(x4, idx)
    n, c, got = vcrnet_amd.estimate_normals(xyz, want_curvature=True, want_idx=True)
    assert eq(n, n0) and eq(c, c0) and eq(got, idx)
    idx = native.knn(x4, None, 30)
    n0 = plane.normals(x4, idx, want_curvature=False)[0]
    assert eq(vcrnet_amd.compute_fpfh_feature(xyz), fpfh.fpfh(x4, idx, fpfh.spfh(x4, n0, idx)))
    idx = vcrnet_amd.search_knn(xyz, 30)
    n0 = plane.normals(x4, idx, want_curvature=False)[0]
    r = 0.15
    assert eq(vcrnet_amd.compute_fpfh_feature(xyz, k=30, radius=r, search="grid"), fpfh.fpfh(x4, idx, fpfh.spfh(x4, n0, idx, r), r))
    assert eq(vcrnet_amd.estimate_normals(xyz, 30, search="grid"), n0)


def test_register_features_over_radius_rows_runs_the_chain():
    """A 600-point torus pair under a known pose, features over Open3D's hybrid neighbourhood of 100: the call is the
    composition of its calls, and its fitness is score_registration's for the pose it returns."""
    vcrnet_amd, _ = mods()
    p = fr_pair.pair(7, 600, 600, "torus")
    src, tgt = dev(p["src"][None]), dev(p["tgt"][None])
    radius, max_dist, T = 0.2, 0.05, 4096
    kw = dict(search="radius", radius=radius, max_nn=100)
    res = vcrnet_amd.register_features(src, tgt, max_dist, trials=T, seed=3, **kw)
    fs, ft = vcrnet_amd.compute_fpfh_feature(src, **kw), vcrnet_amd.compute_fpfh_feature(tgt, **kw)
    assert torch.isfinite(fs).all() and torch.isfinite(ft).all()
    corr = vcrnet_amd.match_features(fs, ft, mutual=True)
    assert torch.equal(res["corr"], corr)
    r = vcrnet_amd.ransac_correspondences(src, tgt, corr, max_dist, T, seed=3)
    sc = vcrnet_amd.score_registration(src, tgt, res["R"], res["t"], max_dist)
    for key, want in (("R", r["R"]), ("t", r["t"]), ("fitness", sc["fitness"]), ("inlier_rmse", sc["inlier_rmse"]), ("inliers", sc["inliers"])):
        assert torch.equal(res[key].view(torch.int32), want.view(torch.int32)), key
    print("register_features(search='radius', max_nn=100): fitness", float(res["fitness"][0]), "pairs", int(res["pairs"][0]))
    fg = vcrnet_amd.register_features(src, tgt, max_dist, method="fgr", **kw)
    assert torch.equal(fg["corr"], corr)
