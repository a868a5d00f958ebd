"""vcr_rows_iss_saliency_f32, vcr_rows_iss_nms_f32, vcr_iss_select_f32, ``compute_iss_keypoints``, ``model_resolution`` and
register_features(keypoints="iss") on the GPU (include/keypoint/vcr_hip_iss.h).

Every comparison is bit-equal -- the fp64 saliency and eigenvalues as uint64, the flags, count and index, the points' bits -- with
the numpy restatement (tests/iss_restated.py) fed the DEVICE'S OWN rows, and for ``compute_iss_keypoints`` also with the
restatement on the definition's rows (radius_restated.radius_rows).  Every raw call runs with its outputs (and the selection's
workspace) prefilled with the byte 0xA5 and 64 elements of guard behind the outputs; the suppression runs in the plan's form, as a
lane a row and as a wave a row, and the three must agree."""
import functools

import numpy as np
import pytest
import torch

import iss_restated as ir
import match_restated as mr
import radius_restated as rr

pytestmark = pytest.mark.gpu

BYTE = 0xA5
GUARD = 64
FORMS = (0, "lane", "wave")
F32 = np.float32


def mods():
    import vcrnet_amd
    from vcrnet_amd import iss
    return vcrnet_amd, iss


def dev(x):
    return torch.from_numpy(np.array(x, order="C")).cuda()              # (a copy: the shared cases are read-only)


def checked(out, raw, name):
    """The output as numpy; all of it must have been overwritten, none of the band behind it."""
    buf, n = raw[name], out.numel()
    size = buf.element_size()
    band = buf[n:].view(torch.uint8).cpu().numpy()
    assert band.size == GUARD * size and (band == BYTE).all(), (name, "guard band written")
    body = buf[:n].view(torch.uint8).cpu().numpy().reshape(n, size)
    assert not (body == BYTE).all(axis=1).any(), (name, "element left unwritten")
    return out.cpu().numpy()


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view({4: np.uint32, 8: np.uint64}[a.dtype.itemsize])


def run(x, csr, nms_csr=None, d2=None, r2_nm=None, gammas=ir.GAMMAS[0], min_neighbors=5):
    """The three raw calls on x numpy [B,3,N] and device rows -> dict of numpy [B, ...]; the suppression in every form."""
    vcrnet_amd, iss = mods()
    from vcrnet_amd import native
    xyz = dev(x)
    o = iss.saliency_rows(native.to_rows4(xyz), *csr, gammas[0], gammas[1], min_neighbors, want_eigen=True, guard=GUARD, prefill=BYTE)
    torch.cuda.synchronize()
    got = {k: checked(o[k], o["_raw"], k) for k in ("saliency", "eigen")}
    only = iss.saliency_rows(native.to_rows4(xyz), *csr, gammas[0], gammas[1], min_neighbors)
    assert set(only) == {"saliency"} and np.array_equal(bits(only["saliency"].cpu().numpy()), bits(got["saliency"]))
    flags = []
    for variant in FORMS:
        f = iss.nms_rows(*(csr if nms_csr is None else nms_csr), o["saliency"], min_neighbors, d2=d2, r2_nm=r2_nm, variant=variant,
                         guard=GUARD, prefill=BYTE)
        torch.cuda.synchronize()
        flags.append(checked(f["keypoint"], f["_raw"], "keypoint"))
        assert np.array_equal(flags[-1], flags[0]), variant
    got["keypoint"] = flags[0]
    s = iss.select(xyz, dev(flags[0]), guard=GUARD, prefill=BYTE)
    torch.cuda.synchronize()
    got.update({k: checked(s[k], s["_raw"], k) for k in ("points", "count", "index")})
    return got


def host(csr):
    return [t.cpu().numpy() for t in csr]


def agree(got, b, want, what):
    for k in ("saliency", "eigen", "points"):
        assert np.array_equal(bits(got[k][b]), bits(want[k])), (what, k, int((bits(got[k][b]) != bits(want[k])).sum()))
    assert np.array_equal(got["keypoint"][b], want["keypoint"]), (what, int((got["keypoint"][b] != want["keypoint"]).sum()))
    assert int(got["count"][b]) == want["count"] and np.array_equal(got["index"][b], want["index"]), what


def against_the_restatement(x, csr, nms_csr=None, d2=None, r2_nm=None, gammas=ir.GAMMAS[0], min_neighbors=5, what=""):
    """run() against iss_restated.definition on the same rows, cloud by cloud -> run()'s dict."""
    got = run(x, csr, nms_csr, d2, r2_nm, gammas, min_neighbors)
    c, n = host(csr), None if nms_csr is None else host(nms_csr)
    dd = None if d2 is None else d2.cpu().numpy()
    for b in range(x.shape[0]):
        want = ir.definition(x[b], (c[0][b], c[1][b], c[2][b]), None if n is None else (n[0][b], n[1][b], n[2][b]),
                             None if dd is None else dd[b], r2_nm, gammas[0], gammas[1], min_neighbors,
                             capacity=c[0].shape[1], nms_capacity=None if n is None else n[0].shape[1])
        agree(got, b, want, (what, b))
    return got


@functools.lru_cache(maxsize=None)
def batches():
    """The four clouds as batches of two and three, with Open3D's default radii of each batch's first cloud."""
    out = {"surfaces": np.stack([ir.torus(600), ir.bumpy(600)]), "bumpy1500": np.stack([ir.bumpy(1500, 1), ir.bumpy(1500, 2)]),
           "cubes": np.stack([ir.cube(700, 2), ir.cube(700, 3), ir.cube(700, 4)])}
    for v in out.values():
        v.setflags(write=False)
    return {k: (v, ir.default_radii(v[0])) for k, v in out.items()}


# ----------------------------------------------------------------------------------------------- the restatement on real rows

def test_the_cloud_worked_by_hand():
    x, rows, nms_rows, d2 = ir.hand_cloud()
    csr = tuple(dev(a) for a in ir.batch([rows]))
    ncsr = tuple(dev(a) for a in ir.batch([nms_rows]))
    got = against_the_restatement(x[None], csr, ncsr, what="whole rows")
    assert got["saliency"][0, 0] == 2.0 / 7.0 and got["saliency"][0, 7] == 0.5 / 7.0 and got["keypoint"][0].tolist() == [1] + [0] * 13
    assert got["eigen"][0, 0].tolist() == [2.0 / 7.0, 8.0 / 7.0, 32.0 / 7.0]
    cut = against_the_restatement(x[None], csr, ncsr, dev(d2[None]), 99.0, what="prefix")
    assert cut["keypoint"][0].tolist() == [1] + [0] * 6 + [1] + [0] * 6 and cut["count"].tolist() == [2]


@pytest.mark.parametrize("gammas", ir.GAMMAS)
@pytest.mark.parametrize("name", ["surfaces", "bumpy1500", "cubes"])
def test_the_four_clouds_in_batches(name, gammas):
    """search_radius' rows at the salient radius, the suppression on their d2 prefix -- and on a second search's rows: the same
    flags.  The cubes' rows hold about 107 entries: two steps of 64."""
    vcrnet_amd, iss = mods()
    x, (sr, nr) = batches()[name]
    xyz = dev(x)
    idx, row_start, total, d2 = vcrnet_amd.search_radius(xyz, sr, want_d2=True)
    got = against_the_restatement(x, (idx, row_start, total), None, d2, float(rr.r2_of(nr)), gammas, what=name)
    small = vcrnet_amd.search_radius(xyz, nr)
    two = against_the_restatement(x, (idx, row_start, total), small, None, None, gammas, what=name + " two searches")
    for k in ("keypoint", "count", "index"):
        assert np.array_equal(got[k], two[k]), k
    assert (got["count"] >= 2).all() and ((got["saliency"] > 0).sum(1) >= 20).all()
    print(name, gammas, "keypoints", got["count"].tolist(), "salient", (got["saliency"] > 0).sum(1).tolist(),
          "entries a row", (total.cpu().numpy() / x.shape[2]).round(1).tolist())
    if name == "surfaces" and gammas == ir.GAMMAS[0]:       # the public call against the definition on the definition's rows
        points, count, index, flag, sal = vcrnet_amd.compute_iss_keypoints(xyz, sr, nr, want_flag=True, want_saliency=True)
        wide = vcrnet_amd.compute_iss_keypoints(xyz, nr, sr, want_flag=True)
        for b in range(x.shape[0]):
            want = ir.of_cloud(x[b], sr, nr)
            mine = {"saliency": sal.cpu().numpy(), "eigen": want["eigen"][None].repeat(b + 1, 0), "keypoint": flag.cpu().numpy(),
                    "points": points.cpu().numpy(), "count": count.cpu().numpy(), "index": index.cpu().numpy()}
            agree(mine, b, want, ("compute_iss_keypoints", b))
            assert np.array_equal(wide[3][b].cpu().numpy(), ir.of_cloud(x[b], nr, sr)["keypoint"]), ("two searches", b)
        three = vcrnet_amd.compute_iss_keypoints(xyz, sr, nr)
        assert len(three) == 3 and torch.equal(three[1], count) and torch.equal(three[2], index)


@pytest.mark.parametrize("min_neighbors", [1, 5, 200])
def test_caller_built_rows_of_every_length(min_neighbors):
    """Rows of 0, 1, 2, 63, 64, 65, 128 and 129 entries on 300 points, entries outside [0, N) among them, 200 neighbours above
    every row; the suppression on the same rows, whole and cut by a d2 that ends the prefixes anywhere."""
    N = 300
    x = np.stack([ir.torus(N), ir.bumpy(N)])
    rows = [ir.rows_of_lengths(N, seed=4), ir.rows_of_lengths(N, ir.LENGTHS[::-1], seed=5)]
    idx, row_start, total = ir.batch(rows, slack=3)
    assert set(np.diff(row_start[0]).tolist()) == set(ir.LENGTHS) and (idx[0, :total[0]] < 0).any() and (idx[0, :total[0]] >= N).any()
    csr = (dev(idx), dev(row_start), dev(total))
    got = against_the_restatement(x, csr, min_neighbors=min_neighbors, what="whole")
    d2 = np.random.RandomState(6).uniform(0, 1, idx.shape).astype(F32)
    cut = against_the_restatement(x, csr, None, dev(d2), 0.8, min_neighbors=min_neighbors, what="cut")
    if min_neighbors == 200:
        assert not got["saliency"].any() and not got["eigen"].any() and not got["count"].any()
    else:
        assert (got["count"] > 0).all() and (cut["count"] > 0).all() and not np.array_equal(got["keypoint"], cut["keypoint"])


@pytest.mark.parametrize("N", [1, 3, 5, 257])
def test_small_clouds_and_a_last_workgroup_with_idle_waves(N):
    """Every point lists every other: rows of N - 1 entries (256 at N = 257: four steps); N = 1 has capacity 0 and no idx."""
    x = np.stack([ir.bumpy(N, 7), ir.cube(N, 8)])
    rows = ir.flat([[j for j in range(N) if j != i] for i in range(N)])
    idx, row_start, total = ir.batch([rows, rows])
    assert idx.shape == (2, N * (N - 1))
    csr = (dev(idx), dev(row_start), dev(total))
    for mn in (1, 5):
        got = against_the_restatement(x, csr, min_neighbors=mn, what=(N, mn))
        if N < mn:
            assert not got["saliency"].any() and not got["count"].any()
    if N == 257:
        assert (got["count"] >= 1).all()                    # one neighbourhood for all: the largest l0 wins
    if N == 1:
        assert not got["saliency"].any() and got["keypoint"].tolist() == [[0], [0]]


def test_degenerate_clouds():
    """A NaN and an infinite point (C not finite in the rows that list them), an exact plane (l0 <= 0: never a keypoint),
    collinear points (l0 = l1 = 0 or rounding: the NaN or the negative ratio), copies of points -- on caller-built rows of
    twelve entries, and the copies through the search as well."""
    vcrnet_amd, _ = mods()
    N = 64
    rs = np.random.RandomState(9)
    bad = ir.bumpy(N, 3)
    bad[:, 3] = np.nan
    bad[1, 7] = np.inf
    plane = np.stack([rs.randint(-200, 200, N), rs.randint(-200, 200, N), np.zeros(N)]).astype(F32) * F32(2.0 ** -6)
    line = np.stack([rs.uniform(-1, 1, N), np.zeros(N), np.zeros(N)]).astype(F32)
    copies = ir.bumpy(N, 4)
    copies[:, N // 2:] = copies[:, :N // 2]
    x = np.stack([bad, plane, line, copies])
    half = [rs.permutation(N // 2)[:6].tolist() for _ in range(N // 2)]
    rows = ir.flat([[j for j in rs.permutation(N) if j != i][:12] for i in range(N)])
    same = ir.flat([sorted(set(r) | {k + N // 2 for k in r}) for r in half] * 2)        # a point and its copy: the same row
    idx, row_start, total = ir.batch([rows, rows, rows, same])
    csr = (dev(idx), dev(row_start), dev(total))
    got = against_the_restatement(x, csr, what="degenerate")
    assert np.isnan(got["eigen"][0]).any() and not np.isnan(got["saliency"][0]).any() and (got["keypoint"][0] >= 0).all()
    assert (got["saliency"][1] <= 0).all() and not got["count"][1] and (got["eigen"][1][:, 2] > 0).all()
    assert not got["count"][2] and not (got["saliency"][2] > 0).any()
    k = got["keypoint"][3]
    assert np.array_equal(bits(got["saliency"][3][:N // 2]), bits(got["saliency"][3][N // 2:])) and np.array_equal(k[:N // 2], k[N // 2:])
    # through the search: the copy of a keypoint is a keypoint
    y = ir.bumpy(300, seed=5)
    sr, nr = ir.default_radii(y)
    first = int(ir.of_cloud(y, sr, nr)["index"][0])
    y = np.concatenate([y, y[:, first:first + 1]], axis=1)
    flag = vcrnet_amd.compute_iss_keypoints(dev(y[None]), sr, nr, want_flag=True)[3][0].cpu().numpy()
    assert flag[first] == flag[300] == 1 and np.array_equal(flag, ir.of_cloud(y, sr, nr)["keypoint"])


# ------------------------------------------------------------------------------------------------------------------ invariances

@functools.lru_cache(maxsize=None)
def mixed():
    x = np.stack([ir.torus(600), ir.bumpy(600), ir.cube(600, 5)])
    x.setflags(write=False)
    return x


def test_a_cloud_alone_returns_the_bits_it_returns_in_the_batch():
    vcrnet_amd, _ = mods()
    x = mixed()
    sr, nr = ir.default_radii(x[0])
    xyz = dev(x)
    idx, row_start, total, d2 = vcrnet_amd.search_radius(xyz, sr, want_d2=True)
    r2 = float(rr.r2_of(nr))
    o = run(x, (idx, row_start, total), None, d2, r2)
    for b in range(x.shape[0]):
        i1, s1, t1, d1 = vcrnet_amd.search_radius(xyz[b:b + 1], sr, want_d2=True)
        one = run(x[b:b + 1], (i1, s1, t1), None, d1, r2)
        for k in o:
            assert np.array_equal(bits(one[k][0]), bits(o[k][b])), (b, k)


def test_a_cloud_that_is_not_served_is_voided_and_leaves_the_others_alone():
    """total[b] > capacity (search_radius' "does not fit": every idx -1), and a row_start that does not ascend from 0 to total."""
    vcrnet_amd, _ = mods()
    x = mixed()
    B, _, N = x.shape
    sr, nr = ir.default_radii(x[0])
    r2 = float(rr.r2_of(nr))
    xyz = dev(x)
    fits = vcrnet_amd.search_radius(xyz, sr, want_d2=True)
    totals = fits[2].cpu().numpy()
    big = int(np.argmax(totals))
    cap = int(np.sort(totals)[-2])
    assert cap < totals[big]
    whole = run(x, fits[:3], None, fits[3], r2)

    def voided(o, b):
        assert np.isnan(o["saliency"][b]).all() and np.isnan(o["eigen"][b]).all() and (o["keypoint"][b] == -2).all()
        assert o["count"][b] == 0 and (o["index"][b] == -1).all() and np.isnan(o["points"][b]).all()
    csr = vcrnet_amd.search_radius(xyz, sr, want_d2=True, capacity=cap)
    assert int(csr[2][big]) == totals[big] > cap and (csr[0][big] == -1).all()
    o = against_the_restatement(x, csr[:3], None, csr[3], r2, what="does not fit")
    for b in range(B):
        if b == big:
            voided(o, b)
        else:
            for k in o:
                assert np.array_equal(bits(o[k][b]), bits(whole[k][b])), (b, k)
    points, count, index, flag = vcrnet_amd.compute_iss_keypoints(xyz, sr, nr, capacity=cap, want_flag=True)     # (it does not raise)
    assert np.array_equal(flag.cpu().numpy(), o["keypoint"]) and np.array_equal(count.cpu().numpy(), o["count"])
    for what, edit in (("descends", lambda rs, tot: rs.__setitem__((1, 150), rs[1, 149] - 1)),
                       ("does not start at 0", lambda rs, tot: rs.__setitem__((1, 0), 1)),
                       ("does not end at total", lambda rs, tot: tot.__setitem__(1, tot[1] + 1)),
                       ("negative", lambda rs, tot: rs.__setitem__((1, 0), -4)),
                       ("total above capacity", lambda rs, tot: tot.__setitem__(1, fits[0].shape[1] + 1))):
        rs, tot = fits[1].clone(), fits[2].clone()
        edit(rs, tot)
        o = run(x, (fits[0], rs, tot), None, fits[3], r2)
        for b in range(B):
            if b == 1:
                voided(o, b)
            else:
                for k in o:
                    assert np.array_equal(bits(o[k][b]), bits(whole[k][b])), (what, b, k)
    # served rows under the suppression, a NaN in the saliency: that cloud's flags alone are -2
    _, iss = mods()
    sal = dev(whole["saliency"])
    sal[2, 17] = float("nan")
    for variant in FORMS:
        f = iss.nms_rows(*fits[:3], sal, d2=fits[3], r2_nm=r2, variant=variant)["keypoint"].cpu().numpy()
        assert (f[2] == -2).all() and np.array_equal(f[:2], whole["keypoint"][:2]), variant


# --------------------------------------------------------------------------------------------------------------- the public calls

@pytest.mark.parametrize("B", [1, 2])
def test_the_default_radii_are_the_model_resolution(B):
    vcrnet_amd, _ = mods()
    x = mixed()[:B]
    xyz = dev(x)
    res = vcrnet_amd.model_resolution(xyz)
    assert res.dtype == torch.float64 and res.is_cuda and tuple(res.shape) == (B,)
    res = res.cpu().numpy()
    for b in range(B):
        want = ir.model_resolution(x[b])
        assert abs(res[b] - want) <= 1e-12 * want, (b, res[b], want)
    got = vcrnet_amd.compute_iss_keypoints(xyz, want_flag=True, want_saliency=True)
    assert len(got) == 5 and got[0].shape == (B, 3, x.shape[2]) and got[3].dtype == torch.int32 and got[4].dtype == torch.float64
    for b in range(B):
        sr, nr = float(F32(6.0 * res[b])), float(F32(4.0 * res[b]))
        one = vcrnet_amd.compute_iss_keypoints(xyz[b:b + 1], sr, nr, want_flag=True, want_saliency=True)
        for u, v in zip(got, one):
            assert np.array_equal(bits(u[b].cpu().numpy()), bits(v[0].cpu().numpy())), b
        half = vcrnet_amd.compute_iss_keypoints(xyz[b:b + 1], non_max_radius=nr, want_flag=True)      # (one radius given, one not)
        assert torch.equal(half[3], one[3])
    assert int(got[1].min()) >= 2
    bad = x[:1].copy()
    bad[0, :, 5] = np.nan
    r = float(vcrnet_amd.model_resolution(dev(bad))[0])
    want = ir.model_resolution(bad[0])
    assert abs(r - want) <= 1e-12 * want


@pytest.mark.parametrize("method", ["ransac", "fgr"])
def test_register_features_with_iss_keypoints_is_the_chain_composed_by_hand(method):
    """surface(600) at k = 20: FPFH on both clouds -> match_features -> -1 where the source point is no keypoint -> RANSAC or FGR
    -> score, bit for bit; keypoints=None is the call without the keyword."""
    vcrnet_amd, _ = mods()
    c = mr.surface(600)
    k = 20
    src, tgt = dev(c["src"][None]), dev(c["tgt"][None])
    kw = dict(trials=4096, seed=mr.SEED) if method == "ransac" else dict(method="fgr")
    opts = dict(gamma_21=0.8, gamma_32=0.8, min_neighbors=4)
    res = vcrnet_amd.register_features(src, tgt, mr.MAX_DIST, k=k, mutual=False, keypoints="iss", iss=opts, **kw)
    flag = vcrnet_amd.compute_iss_keypoints(src, want_flag=True, **opts)[3]
    every = vcrnet_amd.match_features(vcrnet_amd.compute_fpfh_feature(src, None, k=k), vcrnet_amd.compute_fpfh_feature(tgt, None, k=k),
                                      mutual=False)
    corr = torch.where(flag > 0, every, torch.full_like(every, -1))
    if method == "ransac":
        r = vcrnet_amd.ransac_correspondences(src, tgt, corr, mr.MAX_DIST, 4096, seed=mr.SEED)
        want = dict(R=r["R"], t=r["t"], best_trial=r["best_trial"], pairs=r["pairs"], ransac_inliers=r["inliers"])
    else:
        r = vcrnet_amd.fast_global_registration(src, tgt, corr)
        want = {key: r[key] for key in ("R", "t", "pairs", "tuples", "used", "status")}
    want.update(vcrnet_amd.score_registration(src, tgt, want["R"], want["t"], mr.MAX_DIST), corr=corr)
    same = lambda a, b: a.dtype == b.dtype and a.shape == b.shape and torch.equal(a.contiguous().view(torch.uint8), b.contiguous().view(torch.uint8))  # noqa: E731
    assert set(res) == set(want)
    for key, v in want.items():
        assert same(res[key], v), key
    n = int((flag > 0).sum())
    assert 2 <= n < 600 and int((corr >= 0).sum()) <= n
    if method == "ransac":
        assert int(res["pairs"][0]) == int((corr >= 0).sum())
    print(method, "keypoints", n, "pairs", int(res["pairs"][0]), "fitness", float(res["fitness"][0]))
    plain = vcrnet_amd.register_features(src, tgt, mr.MAX_DIST, k=k, mutual=False, **kw)
    none = vcrnet_amd.register_features(src, tgt, mr.MAX_DIST, k=k, mutual=False, keypoints=None, **kw)
    assert set(plain) == set(none) and torch.equal(plain["corr"], every)
    for key in plain:
        assert same(plain[key], none[key]), key
