"""vcr_fgr_f32 on the GPU (include/vcr_hip_fgr.h) against the numpy restatement (tests/fgr_restated.py),
and register_features(method="fgr") end to end.

Everything in front of the first update is integer, fp32 or fp64 arithmetic in a stated order and is held bit for bit: the pair
count, the kept tuples and their list, the normalisation, the 27 sums of the first iteration, mu.  From the first update on
the device's sincos is not numpy's, so the whole loop is held within an allowance computed from the restatement alone.  Every
call runs with 4096 elements of guard behind outputs prefilled with 0xFF (NaN as a float, -1 as an int), the workspace
prefilled likewise."""
import functools

import numpy as np
import pytest
import torch

import fgr_restated as fg
import match_restated as mr

pytestmark = pytest.mark.gpu

GUARD = 4096
BYTE = 0xFF
F32 = np.float32
KEYS = ("R", "t", "pairs", "tuples", "used", "status", "tuple_list", "norm", "pose64", "sums", "mu")
IDENTITY = np.asarray([1, 0, 0, 0, 1, 0, 0, 0, 1, 0, 0, 0], np.float64)


def mods():
    import vcrnet_amd
    from vcrnet_amd import fgr
    return vcrnet_amd, fgr


def dev(x):
    return torch.tensor(np.array(x)).cuda()                  # (a copy: the cached cases are read-only)


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.int64 if a.dtype.itemsize == 8 else np.int32)


def same(a, b):
    return a.shape == np.shape(b) and np.array_equal(bits(a), bits(np.asarray(b, a.dtype)))


def run(src, tgt, corr, **kw):
    """src [B,3,Ns], tgt [B,3,Nt], corr [B,Ns] numpy -> dict of numpy arrays, every stage; the guard bands are checked."""
    _, fgr = mods()
    o = fgr.fgr(dev(np.asarray(src, F32)), dev(np.asarray(tgt, F32)), dev(np.asarray(corr).astype(np.int32)), want_stages=True,
                guard=GUARD, prefill=BYTE, **kw)
    torch.cuda.synchronize()
    for name, buf in o["_raw"].items():
        n = o[name].numel()
        band = buf[n:].view(torch.uint8).cpu().numpy()
        assert band.size == GUARD * buf.element_size() and (band == BYTE).all(), (name, "guard band written")
    out = {k: o[k].cpu().numpy() for k in KEYS}
    for b in range(out["R"].shape[0]):                       # what holds for every cloud of every call
        assert same(out["R"][b].reshape(9), out["pose64"][b, :9].astype(F32)), "R_out is pose64 rounded once"
        assert same(out["t"][b], out["pose64"][b, 9:].astype(F32)), "t_out is pose64 rounded once"
        assert (out["tuple_list"][b, out["used"][b] if out["tuples"][b] else 0:] == -1).all(), "behind L nothing is written"
    return out


def one(c, **kw):
    return run(c["src"][None], c["tgt"][None], c["corr"][None], **kw)


@functools.lru_cache(maxsize=None)
def planted(M, share, seed=0):
    c = mr.planted(M, share, seed=seed, extra=5)
    for v in c.values():
        v.setflags(write=False)
    return c


# ------------------------------------------------------------------------------------------------------------------ the tuples

def with_pairs(c, M):
    """The recipe's cloud with only its first M pairs."""
    corr = c["corr"].copy()
    corr[M:] = -1
    return dict(c, corr=corr)


@pytest.mark.parametrize("M,T,K", [(40, 4000, 1000), (257, 2048, 1000), (40, 65, 1), (40, 65, 7), (40, 4000, 7), (40, 4000, 5000),
                                   (40, 1, 1000), (0, 512, 1000), (2, 512, 1000)])
def test_the_kept_tuples_are_the_restatements(M, T, K):
    """T = 100 M; T below 100 M and no multiple of 256; the cut met at small and at large T; K above the passes; one trial; no
    pair and two pairs, where no trial can pass (a repeated pick has a zero edge)."""
    c = planted(257, 0.3) if M == 257 else with_pairs(planted(40, 0.5), M)
    want_M, ntup, lst = fg.tuples(c["src"], c["tgt"], c["corr"], 0.95, T, K, 5)
    o = one(c, tuple_trials=T, max_tuples=K, seed=5)
    print(f"tuples M {M} T {T} K {K}: {int(o['tuples'][0])} kept, L {int(o['used'][0])}")
    assert (o["pairs"][0], o["tuples"][0], o["used"][0]) == (want_M, ntup, 3 * ntup) == (M, ntup, len(lst))
    assert np.array_equal(o["tuple_list"][0, :len(lst)], lst)
    if K in (1, 7):
        assert ntup == K                                     # (the cut is met)
    if K == 5000 or M < 3 or T == 1:
        assert ntup < K and (M >= 3 or ntup == 0)
    assert o["status"][0] == (1 if 3 * ntup < 10 else 0)
    other = one(c, tuple_trials=T, max_tuples=K, seed=6)
    assert ntup < 2 or not np.array_equal(other["tuple_list"], o["tuple_list"])   # the seed is the RANSAC's: it moves the draws


# ----------------------------------------------------------------------------------------------------------- the normalisation

@pytest.mark.parametrize("Ns,Nt", [(1, 5), (257, 300), (1000, 777)])
def test_the_normalisation_is_the_restatements_bits(Ns, Nt):
    rs = np.random.RandomState(40 + Ns)
    src = (rs.uniform(-1, 1, (2, 3, Ns)) * [[[1.0], [3.0], [0.2]]] + 0.7).astype(F32)
    tgt = (rs.uniform(-2, 1, (2, 3, Nt)) - [[[5.0], [0.0], [1.0]]]).astype(F32)
    o = run(src, tgt, np.full((2, Ns), -1))                  # no pairs: nothing but the normalisation runs
    for b in range(2):
        ms, mt, scale = fg.normalise(src[b], tgt[b])
        assert same(o["norm"][b], np.concatenate([ms, mt, [scale]])), (b, o["norm"][b], ms, mt, scale)
        assert o["status"][b] == 1 and same(o["pose64"][b], IDENTITY) and o["pairs"][b] == 0


# ------------------------------------------------------------------------------------------------------------------- the sums

@pytest.mark.parametrize("L,tuple_scale", [(10, 0.0), (255, 0.0), (256, 0.0), (257, 0.0), (3000, 0.95), (3001, 0.0)])
def test_the_first_iterations_sums_are_the_restatements_bits(L, tuple_scale):
    c = planted(1000, 0.5) if tuple_scale else planted(L, 0.5)
    kw = dict(tuple_scale=tuple_scale, T=20000, K=1000, seed=2, iterations=1)
    want = fg.fgr(c["src"], c["tgt"], c["corr"], **kw)
    assert want["used"] == L and want["status"] == 0
    o = one(c, tuple_scale=tuple_scale, tuple_trials=20000, max_tuples=1000, seed=2, iterations=1)
    assert o["used"][0] == L and o["status"][0] == 0 and same(o["norm"][0], want["norm"])
    worst = np.abs(o["sums"][0] - want["sums"]).max()
    print(f"sums L {L}: largest difference {worst:.3g}")
    assert same(o["sums"][0], want["sums"]), (o["sums"][0] - want["sums"])
    assert same(o["mu"], [1.0 / 1.4])                        # iteration 0 shrinks mu once
    assert np.abs(o["pose64"][0] - want["pose64"]).max() <= 1e-12      # (one update: the sincos alone differs)


@pytest.mark.parametrize("decrease_mu", [True, False])
def test_mu_after_the_loop(decrease_mu):
    c = planted(40, 0.5)
    for iterations, division_factor, mu_floor in ((64, 1.4, 0.025), (7, 1.4, 0.025), (64, 3.0, 0.5), (0, 1.4, 0.025), (5, 1.1, 1e-9)):
        want = fg.fgr(c["src"], c["tgt"], c["corr"], iterations=iterations, division_factor=division_factor, mu_floor=mu_floor,
                      decrease_mu=decrease_mu, T=4000)
        o = one(c, iterations=iterations, division_factor=division_factor, mu_floor=mu_floor, decrease_mu=decrease_mu,
                tuple_trials=4000)
        assert same(o["mu"], [want["mu"]]), (iterations, division_factor, o["mu"], want["mu"])
        assert decrease_mu or o["mu"][0] == 1.0


def test_no_iteration_returns_the_difference_of_the_means():
    c = planted(257, 0.3)
    o = one(c, iterations=0)
    ms, mt, _ = fg.normalise(c["src"], c["tgt"])
    assert np.array_equal(o["R"][0], np.eye(3, dtype=F32)) and same(o["t"][0], (mt - ms).astype(F32))
    assert same(o["pose64"][0, 9:], mt - ms) and not o["sums"].any() and o["mu"][0] == 1.0 and o["status"][0] == 0


# ------------------------------------------------------------------------------------------------------------- the whole loop

@functools.lru_cache(maxsize=None)
def loop_case(M, share):
    """The restatement's pose and the allowance for the device's: 64 x the largest change of that pose when every entry of
    every Ri is moved one ulp up, or one ulp down -- a few ulps for each of the 64 sincos calls."""
    c = planted(M, share)
    want = fg.fgr(c["src"], c["tgt"], c["corr"])
    spread = 0.0
    for way in (np.inf, -np.inf):
        moved = fg.fgr(c["src"], c["tgt"], c["corr"], nudge=lambda it, Ri, way=way: np.nextafter(Ri, way))
        spread = max(spread, float(np.abs(moved["pose64"] - want["pose64"]).max()))
    return c, want, spread


@pytest.mark.parametrize("M,share,T", mr.RANSAC_SHAPES)
def test_the_whole_loop_is_the_restatement_within_the_sincos_allowance(M, share, T):
    c, want, spread = loop_case(M, share)
    o = one(c)
    diff = float(np.abs(o["pose64"][0] - want["pose64"]).max())
    print(f"loop M {M}: device - restatement {diff:.3g}, one-ulp spread {spread:.3g}, allowance {64 * spread:.3g}")
    assert 0 < spread < 1e-13
    assert (o["pairs"][0], o["tuples"][0], o["used"][0], o["status"][0]) == (M, want["tuples"], want["used"], 0)
    assert diff <= 64 * spread, (diff, spread)
    assert same(o["mu"], [want["mu"]])


# ------------------------------------------------------------------------------------------------------------------- behaviour

@pytest.mark.parametrize("M,share,T", mr.RANSAC_SHAPES)
def test_the_device_recovers_the_planted_pose(M, share, T):
    """The CPU test's bounds: 0.1 degree and 1e-3 with the tuple test, 2 degrees and 3e-2 without."""
    clouds = [planted(M, share, seed) for seed in range(3)]
    s = {k: np.stack([c[k] for c in clouds]) for k in ("src", "tgt", "corr")}
    for tuple_scale, rot, shift in ((0.95, 0.1, 1e-3), (0.0, 2.0, 3e-2)):
        o = run(s["src"], s["tgt"], s["corr"], tuple_scale=tuple_scale)
        for b, c in enumerate(clouds):
            dr = fg.rotation_error_deg(o["pose64"][b, :9].reshape(3, 3), c["R"])
            dt = float(np.abs(o["pose64"][b, 9:] - c["t"]).max())
            print(f"fgr device M {M} seed {b} tuple_scale {tuple_scale}: {int(o['tuples'][b])} tuples, {int(o['used'][b])} entries, "
                  f"rotation {dr:.4f} deg, |dt| {dt:.2e}")
            assert o["status"][b] == 0 and dr <= rot and dt <= shift, (dr, dt)
            assert np.abs(o["R"][b].astype(np.float64) - c["R"]).max() <= 2 * np.radians(rot)


def test_a_batch_is_its_clouds_alone():
    clouds = [with_pairs(planted(257, 0.3, seed), M) for seed, M in ((0, 257), (1, 100), (2, 40))]
    s = {k: np.stack([c[k] for c in clouds]) for k in ("src", "tgt", "corr")}
    for tuple_scale in (0.95, 0.0):
        o = run(s["src"], s["tgt"], s["corr"], tuple_scale=tuple_scale, tuple_trials=8192)
        assert o["pairs"].tolist() == [257, 100, 40] and (o["status"] == 0).all()
        for b, c in enumerate(clouds):
            alone = one(c, tuple_scale=tuple_scale, tuple_trials=8192)
            for k in KEYS:
                assert same(alone[k][0], o[k][b]), (tuple_scale, b, k)
    vcrnet_amd, _ = mods()
    r = vcrnet_amd.fast_global_registration(dev(s["src"]), dev(s["tgt"]), dev(s["corr"]), tuple_scale=0.0, tuple_trials=8192)
    assert set(r) == {"R", "t", "pairs", "tuples", "used", "status"}
    for k in r:
        assert same(r[k].cpu().numpy(), o[k]), k


def test_fewer_than_ten_entries_return_the_identity():
    c = planted(40, 0.5)
    for tuple_scale, kw, L in ((0.0, {}, 9), (0.95, dict(max_tuples=3), 9), (0.0, {}, 0)):
        o = one(with_pairs(c, 40 if tuple_scale else L), tuple_scale=tuple_scale, tuple_trials=4000, **kw)
        assert (o["used"][0], o["status"][0]) == (L, 1) and same(o["pose64"][0], IDENTITY)
        assert np.array_equal(o["R"][0], np.eye(3, dtype=F32)) and not o["t"].any() and o["mu"][0] == 1.0 and not o["sums"].any()
    assert one(with_pairs(c, 10), tuple_scale=0.0)["status"][0] == 0
    assert one(c, tuple_trials=4000, max_tuples=4)["status"][0] == 0


def test_a_nan_coordinate_spoils_its_own_cloud_alone():
    clouds = [planted(257, 0.3, seed) for seed in range(3)]
    s = {k: np.stack([c[k] for c in clouds]) for k in ("src", "tgt", "corr")}
    clean = run(s["src"], s["tgt"], s["corr"])
    for which, spot in (("src", (1, 2, 250)), ("tgt", (1, 0, 3))):
        bad = {k: v.copy() for k, v in s.items()}
        bad[which][spot] = np.nan
        o = run(bad["src"], bad["tgt"], bad["corr"])
        assert o["status"].tolist() == [0, 2, 0]
        assert np.isnan(o["R"][1]).all() and np.isnan(o["t"][1]).all() and np.isnan(o["pose64"][1]).all()
        for b in (0, 2):
            for k in KEYS:
                assert same(o[k][b], clean[k][b]), (which, b, k)


def test_points_on_a_line_make_every_system_singular():
    c = planted(40, 0.5)
    line = np.zeros((3, 45), F32)
    line[0] = np.linspace(0, 1, 45)
    want = fg.fgr(line, line[:, :40], c["corr"], tuple_scale=0.0)
    o = run(line[None], line[None, :, :40], c["corr"][None], tuple_scale=0.0)
    assert want["status"] == 16 and o["status"][0] == 16
    assert np.array_equal(o["R"][0], np.eye(3, dtype=F32))
    for k in ("pose64", "norm", "sums", "mu", "used"):       # no update, no sincos: the restatement's bits
        assert same(o[k][0], want[k]), k


# ------------------------------------------------------------------------------------------------------------------ end to end

@pytest.mark.parametrize("N,k", [(600, 20), (1500, 30)])
def test_register_features_with_fgr_on_a_surface_without_symmetries(N, k):
    """tests/test_hip_match.py's surface: with normals oriented alike and mutual matching (the CPU chain's shares of correct
    pairs: 0.998 / 1.0) the ICP behind the FGR's pose recovers the planted one within the 1e-5 the RANSAC's test holds.  With
    estimated normals (arbitrary signs: 54 % / 98 % correct among the mutual pairs) the figures are printed only."""
    vcrnet_amd, _ = mods()
    c = mr.surface(N)
    src, tgt = dev(c["src"][None]), dev(c["tgt"][None])
    ups = mr.surface_up(c)
    ns, nt = (dev(mr.orient(vcrnet_amd.estimate_normals(x, k)[0].cpu().numpy(), up)[None]) for x, up in zip((src, tgt), ups))
    for oriented in (False, True):
        kw = dict(src_normals=ns, tgt_normals=nt) if oriented else {}
        res = vcrnet_amd.register_features(src, tgt, mr.MAX_DIST, k=k, method="fgr", refine=mr.MAX_DIST, **kw)
        Rr, tr = res["refined"]["R"][0].cpu().numpy().astype(np.float64), res["refined"]["t"][0].cpu().numpy().astype(np.float64)
        dR, dt = np.abs(Rr - c["R"]).max(), np.abs(tr - c["t"]).max()
        print(f"register_features fgr N {N} k {k} oriented {oriented}: {int(res['pairs'][0])} pairs, {int(res['tuples'][0])} tuples, "
              f"status {int(res['status'][0])}, FGR rotation {fg.rotation_error_deg(res['R'][0].cpu().numpy(), c['R']):.4f} deg, fitness "
              f"{float(res['fitness'][0]):.4f}, refined |dR| {dR:.2e} |dt| {dt:.2e} in {int(res['refined']['iterations'][0])} rounds")
        assert "best_trial" not in res and "ransac_inliers" not in res
        if oriented:
            assert int(res["status"][0]) == 0 and int(res["used"][0]) == 3 * int(res["tuples"][0])
            assert dR <= 1e-5 and dt <= 1e-5, (dR, dt)
    # the composition, bit for bit (oriented, as the last run above), with keywords of its own
    opts = dict(tuple_scale=0.9, max_tuples=500, seed=3)
    res = vcrnet_amd.register_features(src, tgt, mr.MAX_DIST, k=k, method="fgr", fgr=opts, refine=mr.MAX_DIST, src_normals=ns, tgt_normals=nt)
    fs, ft = vcrnet_amd.compute_fpfh_feature(src, ns, k=k), vcrnet_amd.compute_fpfh_feature(tgt, nt, k=k)
    corr = vcrnet_amd.match_features(fs, ft, mutual=True)
    r = vcrnet_amd.fast_global_registration(src, tgt, corr, **opts)
    sc = vcrnet_amd.score_registration(src, tgt, r["R"], r["t"], mr.MAX_DIST)
    rf = vcrnet_amd.refine_registration(src, tgt, r["R"], r["t"], mr.MAX_DIST)
    assert torch.equal(res["corr"], corr) and int(r["tuples"][0]) <= 500
    for key, want in (("R", r["R"]), ("t", r["t"]), ("pairs", r["pairs"]), ("tuples", r["tuples"]), ("used", r["used"]),
                      ("status", r["status"]), ("fitness", sc["fitness"]), ("inlier_rmse", sc["inlier_rmse"]), ("inliers", sc["inliers"])):
        assert torch.equal(res[key].view(torch.int32), want.view(torch.int32)), key
    assert set(res["refined"]) == set(rf)
    for key in rf:
        assert torch.equal(res["refined"][key].view(torch.int32), rf[key].view(torch.int32)), key
    assert set(res) == {"fitness", "inlier_rmse", "inliers", "R", "t", "pairs", "tuples", "used", "status", "corr", "refined"}


def test_the_ransac_method_is_the_call_without_the_keyword():
    vcrnet_amd, _ = mods()
    c = mr.surface(600)
    src, tgt = dev(c["src"][None]), dev(c["tgt"][None])
    kw = dict(k=20, trials=2048, seed=mr.SEED, refine=mr.MAX_DIST)
    plain = vcrnet_amd.register_features(src, tgt, mr.MAX_DIST, **kw)
    named = vcrnet_amd.register_features(src, tgt, mr.MAX_DIST, method="ransac", **kw)
    assert set(plain) == set(named) and "best_trial" in plain and "tuples" not in plain
    for key in plain:
        if key == "refined":
            for k2 in plain[key]:
                assert torch.equal(plain[key][k2].view(torch.int32), named[key][k2].view(torch.int32)), k2
        else:
            assert torch.equal(plain[key].view(torch.int32), named[key].view(torch.int32)), key
