"""vcr_feat_nn_f32 and vcr_ransac_f32 on the GPU (include/vcr_hip_match.h) against the numpy restatement
(tests/match_restated.py), and register_features end to end.

The search has a defined order and an exact restatement: index and d2 are held bit for bit, in every launch form.  The RANSAC
is held in stages, every one on the device's own per-trial arrays: the draws and the two early tests exactly; the solve -- a
Jacobi SVD on the device, LAPACK's in numpy -- by properties (a proper rotation, optimal for the three pairs' covariance); the
distance check and the count from the device's own fp32 poses exactly again; the winner by the arg-max rule applied to the
device's own counts.  Every call runs with 4096 elements of guard behind outputs prefilled with 0xFF (NaN as a float, -1 as an
int), the workspace prefilled likewise."""
import functools

import numpy as np
import pytest
import torch

import fpfh_restated as fr
import match_restated as mr

pytestmark = pytest.mark.gpu

GUARD = 4096
BYTE = 0xFF
F32 = np.float32


def mods():
    import vcrnet_amd
    from vcrnet_amd import match
    return vcrnet_amd, match


def dev(x):
    return torch.tensor(np.array(x)).cuda()                  # (a copy: the cached cases are read-only)


def bits(a):
    return np.ascontiguousarray(a).view(np.int32)


def guards_untouched(o):
    """Nothing behind any output was written."""
    for name, buf in o["_raw"].items():
        n = o[name].numel()
        band = buf[n:].view(torch.uint8).cpu().numpy()
        assert band.size == GUARD * buf.element_size() and (band == BYTE).all(), (name, "guard band written")


def run_nn(a, b, **kw):
    """-> dict of numpy arrays (nn_idx, nn_d2, and rev_idx where asked for)."""
    _, match = mods()
    o = match.feat_nn(dev(a), dev(b), guard=GUARD, prefill=BYTE, **kw)
    torch.cuda.synchronize()
    guards_untouched(o)
    out = {k: v.cpu().numpy() for k, v in o.items() if k != "_raw"}
    assert not np.isnan(out["nn_d2"]).any()                  # every d2 written: a d2 is finite or +inf, never the prefill's NaN
    return out


@functools.lru_cache(maxsize=None)
def feat_case(B, Ns, Nt):
    """One shape's inputs and restatement, computed once: (a, b, nn_idx [B,Ns], nn_d2, rev_idx [B,Nt])."""
    a, b = mr.features(B, Ns, Nt)
    return (a, b) + restated_nn(a, b)


def restated_nn(a, b):
    idx, d2, rev = [], [], []
    for k in range(a.shape[0]):
        m = mr.d2_chain(a[k], b[k])
        i, d = mr.nearest(m)
        idx.append(i); d2.append(d); rev.append(mr.nearest_rev(m)[0])
    out = (np.stack(idx).astype(np.int32), np.stack(d2), np.stack(rev).astype(np.int32))
    for v in out:
        v.setflags(write=False)
    return out


def same_nn(o, idx, d2, label):
    assert np.array_equal(o["nn_idx"], idx), (label, "index")
    assert np.array_equal(bits(o["nn_d2"]), bits(d2)), (label, "d2")


@pytest.mark.parametrize("B,Ns,Nt", mr.FEAT_SHAPES)
def test_the_search_is_the_restatement_bit_for_bit(B, Ns, Nt):
    a, b, idx, d2, rev = feat_case(B, Ns, Nt)
    o = run_nn(a, b, want_rev=True)
    same_nn(o, idx, d2, (B, Ns, Nt))
    assert np.array_equal(o["rev_idx"], rev)
    assert idx.min() >= 0 and idx.max() < Nt


@pytest.mark.parametrize("B,Ns,Nt", [(1, 5, 3), (3, 257, 300), (2, 1000, 777)])
def test_every_launch_form_returns_the_same_bits(B, Ns, Nt):
    """1, 2 and 4 rows per lane, 1, 2, 7 and 128 splits (more splits than rows at the small shapes: empty segments), each
    direction of the mutual search in the forced form too."""
    _, match = mods()
    a, b, idx, d2, rev = feat_case(B, Ns, Nt)
    both = np.stack([mr.mutual(idx[k], rev[k]) for k in range(B)])
    for q in match.QUERIES_PER_LANE:
        for s in (1, 2, 7, match.MAX_SPLITS):
            v = match.variant(q, s)
            assert match.feat_nn_form(B, Ns, Nt, 256, v)[:2] == (q, s)
            same_nn(run_nn(a, b, variant=v), idx, d2, (q, s))
        o = run_nn(a, b, variant=match.variant(q, 7), mutual=True, want_rev=True)
        assert np.array_equal(o["nn_idx"], both) and np.array_equal(o["rev_idx"], rev) and np.array_equal(bits(o["nn_d2"]), bits(d2))


def test_a_batch_is_its_clouds_alone():
    a, b, idx, d2, rev = feat_case(3, 257, 300)
    for k in range(3):
        o = run_nn(a[k:k + 1], b[k:k + 1], want_rev=True)
        same_nn(o, idx[k:k + 1], d2[k:k + 1], k)
        assert np.array_equal(o["rev_idx"], rev[k:k + 1])


def test_mutual_is_the_two_one_way_results():
    a, b, idx, d2, rev = feat_case(2, 1000, 777)
    one = run_nn(a, b)
    back = run_nn(b, a)                                      # the one-way search of the other direction
    assert np.array_equal(back["nn_idx"], rev)
    o = run_nn(a, b, mutual=True, want_rev=True)
    assert np.array_equal(o["rev_idx"], back["nn_idx"]) and np.array_equal(bits(o["nn_d2"]), bits(one["nn_d2"]))
    i = np.arange(1000)
    for k in range(2):
        j = one["nn_idx"][k]
        assert np.array_equal(o["nn_idx"][k], np.where(back["nn_idx"][k][j] == i, j, -1))
    kept = (o["nn_idx"] >= 0).sum()
    assert 0 < kept < 2 * 777                                # at most one source row per target row
    without = run_nn(a, b, mutual=True)                      # the reverse result in the workspace
    assert np.array_equal(without["nn_idx"], o["nn_idx"])


def test_duplicated_target_rows_return_the_lowest_index():
    a, b, _, _, _ = feat_case(3, 257, 300)
    dup = np.ascontiguousarray(b[:, :, np.arange(300) % 10])   # ten distinct rows, each thirty times
    idx, d2, rev = restated_nn(a, dup)
    assert idx.max() < 10
    _, match = mods()
    for v in (0, match.variant(1, 7), match.variant(2, 128), match.variant(4, 2)):
        same_nn(run_nn(a, dup, variant=v), idx, d2, v)
    same = np.ascontiguousarray(np.repeat(a[:, :, :1], 300, axis=2))            # every target row equals source row 0: d2 = 0 there
    o = run_nn(a, same, want_rev=True)
    assert (o["nn_idx"] == 0).all() and (o["nn_d2"][:, 0] == 0).all() and (o["rev_idx"] == 0).all()


def test_non_finite_rows_are_never_chosen():
    a, b, idx, d2, rev = feat_case(3, 257, 300)
    bad_a, bad_b = a.copy(), b.copy()
    bad_a[0, 5, 17] = np.nan
    bad_a[1, 32, 200] = np.inf
    bad_a[1, 0, 256] = -np.inf
    jn, ji = int(idx[0, 3]), int(idx[2, 100])                # spoil target rows that ARE somebody's neighbour
    bad_b[0, 20, jn] = np.nan
    bad_b[2, 7, ji] = np.inf
    o = run_nn(bad_a, bad_b, want_rev=True)
    ridx, rd2, rrev = restated_nn(bad_a, bad_b)
    same_nn(o, ridx, rd2, "non-finite")
    assert np.array_equal(o["rev_idx"], rrev)
    for k, i in ((0, 17), (1, 200), (1, 256)):
        assert o["nn_idx"][k, i] == -1 and np.isposinf(o["nn_d2"][k, i])
        assert not (o["rev_idx"][k] == i).any()
    assert not (o["nn_idx"][0] == jn).any() and not (o["nn_idx"][2] == ji).any()
    assert o["rev_idx"][0, jn] == -1 and o["rev_idx"][2, ji] == -1
    # every other row is the clean batch's, bit for bit
    clean = np.ones((3, 257), bool)
    clean[0, 17] = clean[1, 200] = clean[1, 256] = False
    clean[0] &= idx[0] != jn
    clean[2] &= idx[2] != ji
    assert clean.sum() < 3 * 257 - 3
    assert np.array_equal(o["nn_idx"][clean], idx[clean]) and np.array_equal(bits(o["nn_d2"][clean]), bits(d2[clean]))
    m = run_nn(bad_a, bad_b, mutual=True)
    assert np.array_equal(m["nn_idx"], np.stack([mr.mutual(ridx[k], rrev[k]) for k in range(3)]))


def test_the_choice_on_fpfh_rows_against_float64():
    """The device's own FPFH rows of the torus recipe, cloud 0 against cloud 1: the chosen neighbour's float64 distance is the
    float64 minimum within match_restated.CHOICE_E, derived there from the chain's roundings."""
    vcrnet_amd, match = mods()
    x = fr.cloud(2, 1000)
    feat = vcrnet_amd.compute_fpfh_feature(dev(x), k=20)
    a, b = feat[0:1].contiguous(), feat[1:2].contiguous()
    o = match.feat_nn(a, b, guard=GUARD, prefill=BYTE)
    torch.cuda.synchronize()
    guards_untouched(o)
    an, bn = a[0].cpu().numpy(), b[0].cpu().numpy()
    j = o["nn_idx"][0].cpu().numpy()
    assert j.min() >= 0 and j.max() < 1000
    chosen, least = mr.d2_64(an, bn, j), mr.min_d2_64(an, bn)
    print(f"fpfh rows: |row|^2 up to {float((an.astype(np.float64) ** 2).sum(0).max()):.3g}, worst chosen / min - 1 = "
          f"{float((chosen / np.maximum(least, 1e-300)).max() - 1):.2e} (bound {mr.CHOICE_E:.2e})")
    assert ((1 - mr.CHOICE_E) * chosen <= least).all()
    d2 = o["nn_d2"][0].cpu().numpy().astype(np.float64)
    assert (np.abs(d2 - chosen) <= 36 * mr.U * chosen).all()  # (the chain's 35 roundings a term, first order, and its own)
    ridx, rd2, _ = restated_nn(an[None], bn[None])            # ... and the restatement's bits here too
    assert np.array_equal(j, ridx[0]) and np.array_equal(bits(o["nn_d2"].cpu().numpy()), bits(rd2))


# ------------------------------------------------------------------------------------------------------------------ the RANSAC

POSE_KEYS = ("R", "t", "best_trial", "inliers", "pairs", "trial_status", "trial_picks", "trial_pose", "trial_inliers")


def run_ransac(src, tgt, corr, T, seed=mr.SEED, max_dist=mr.MAX_DIST, similarity=mr.SIMILARITY):
    """src [B,3,Ns], tgt [B,3,Nt], corr [B,Ns] numpy -> dict of numpy arrays, want_trials."""
    _, match = mods()
    o = match.ransac(dev(src), dev(tgt), dev(corr.astype(np.int32)), max_dist, T, similarity, seed, want_trials=True,
                     guard=GUARD, prefill=BYTE)
    torch.cuda.synchronize()
    guards_untouched(o)
    return {k: o[k].cpu().numpy() for k in POSE_KEYS}


def stack(clouds):
    return {k: np.stack([c[k] for c in clouds]) for k in ("src", "tgt", "corr")}


def staged(o, b, src, tgt, corr, T, seed=mr.SEED, max_dist=mr.MAX_DIST, similarity=mr.SIMILARITY):
    """The four stages on cloud b of the device's result o; returns the number of valid trials."""
    src, tgt, corr = np.asarray(src, F32), np.asarray(tgt, F32), np.asarray(corr, np.int64)
    status, pose, count = o["trial_status"][b], o["trial_pose"][b], o["trial_inliers"][b]
    pl = mr.pair_list(corr, tgt.shape[1])
    M = len(pl)
    assert o["pairs"][b] == M
    assert status.shape == (T,) and np.isin(status, (0, 1, 2, 3, 4)).all()
    if M == 0:
        assert (status == 1).all() and (o["trial_picks"][b] == -1).all() and (count == -1).all() and not pose.any()
        assert o["best_trial"][b] == -1 and o["inliers"][b] == 0
        return 0
    P, Q = np.ascontiguousarray(src[:, pl].T), np.ascontiguousarray(tgt[:, corr[pl]].T)
    at = mr.picks(seed, T, M)
    # stage 1: the draws and the two early tests, exactly
    assert np.array_equal(o["trial_picks"][b], pl[at])
    early = mr.early_status(P, Q, at, similarity)
    assert np.array_equal(status == 1, early == 1) and np.array_equal(status == 2, early == 2)
    if M < 3:
        assert (status == 1).all()
    assert not pose[early != 0].any()                        # twelve zeros where nothing was solved
    # stage 2: every solved pose is a proper rotation and optimal for its three pairs (test_hip_refine's bounds for a step)
    solved = np.nonzero(early == 0)[0]
    finite = np.isfinite(pose[solved]).all(1)
    assert np.array_equal(status[solved] == 3, ~finite)
    for t in solved[finite]:
        R, tr = pose[t, :9].reshape(3, 3), pose[t, 9:]
        ortho = np.abs(R.T @ R - np.eye(3, dtype=F32)).max()
        det = abs(np.linalg.det(R.astype(F32)) - 1)
        assert ortho <= 1e-5 and det <= 1e-5, (t, ortho, det)
        s = mr.solve3(P[at[t]], Q[at[t]])
        R64 = R.astype(np.float64)
        short = (s["opt"] - np.trace(R64 @ s["H"])) / s["s1"]
        dt = np.abs(tr.astype(np.float64) - (s["qm"] - R64 @ s["pm"])).max()
        assert short <= 2e-6, (t, short)
        assert dt <= 1e-6 * max(1.0, np.abs(tr).max()), (t, dt)
    # stage 3: the distance check and the count from the device's own poses, exactly
    live = solved[finite]
    far, cnt = mr.check_and_count(P, Q, at[live], pose[live], max_dist)
    assert np.array_equal(status[live] == 4, far)
    assert np.array_equal(status[live] == 0, ~far)
    assert np.array_equal(count[live[~far]], cnt[~far])
    assert (count[status != 0] == -1).all()
    # stage 4: the winner is the arg-max rule on the device's own counts
    bt, inl = mr.best(count, status == 0)
    assert (o["best_trial"][b], o["inliers"][b]) == (bt, inl)
    want = pose[bt] if bt >= 0 else np.asarray([1, 0, 0, 0, 1, 0, 0, 0, 1, 0, 0, 0], F32)
    assert np.array_equal(bits(o["R"][b].reshape(9)), bits(want[:9])) and np.array_equal(bits(o["t"][b]), bits(want[9:]))
    return int((status == 0).sum())


def planted_recovered(o, b, c):
    """The count is the planted one, and every planted pair lies within max_dist under the returned pose."""
    good = np.nonzero(c["good"])[0]
    assert o["inliers"][b] == len(good), (o["inliers"][b], len(good))
    moved = o["R"][b].astype(np.float64) @ c["src"][:, good].astype(np.float64) + o["t"][b].astype(np.float64)[:, None]
    dist = np.sqrt(((moved - c["tgt"][:, c["corr"][good]].astype(np.float64)) ** 2).sum(0))
    assert dist.max() <= mr.MAX_DIST, dist.max()
    assert c["good"][o["trial_picks"][b, o["best_trial"][b]]].all()


@functools.lru_cache(maxsize=None)
def ransac_case(M, share, T):
    """Two clouds of the recipe (two seeds) and the device's run, computed once."""
    clouds = (mr.planted(M, share), mr.planted(M, share, seed=1))
    s = stack(clouds)
    o = run_ransac(s["src"], s["tgt"], s["corr"], T)
    for v in o.values():
        v.setflags(write=False)
    return clouds, s, o


@pytest.mark.parametrize("M,share,T", mr.RANSAC_SHAPES)
def test_ransac_staged_on_planted_correspondences(M, share, T):
    clouds, s, o = ransac_case(M, share, T)
    for b in range(2):
        valid = staged(o, b, s["src"][b], s["tgt"][b], s["corr"][b], T)
        print(f"ransac M {M} share {share} T {T} cloud {b}: {valid} valid trials, statuses "
              f"{np.bincount(o['trial_status'][b], minlength=5).tolist()}, best {o['best_trial'][b]} with {o['inliers'][b]}")
        assert valid >= 1
    planted_recovered(o, 0, clouds[0])                       # the recipe's own cloud; the second seed is held by the stages


@pytest.mark.parametrize("M,share,T", [(40, 0.5, 1), (40, 0.5, 65), (3, 1.0, 65), (2, 1.0, 65), (257, 0.3, 257)])
def test_ransac_at_the_edges_of_its_shapes(M, share, T):
    c = mr.planted(M, share)
    o = run_ransac(c["src"][None], c["tgt"][None], c["corr"][None], T)
    valid = staged(o, 0, c["src"], c["tgt"], c["corr"], T)
    if M == 3:
        assert valid >= 1
        planted_recovered(o, 0, c)
    if M == 2:                                               # no trial is valid: the identity
        assert valid == 0 and o["best_trial"][0] == -1 and o["inliers"][0] == 0 and (o["trial_status"] == 1).all()
        assert np.array_equal(o["R"][0], np.eye(3, dtype=F32)) and not o["t"].any() and (o["trial_inliers"] == -1).all()


def test_corr_entries_outside_the_target_are_no_pairs():
    c = mr.planted(40, 0.5, extra=5)                         # five source points at the end without a partner
    corr = c["corr"].astype(np.int64)
    bad = np.nonzero(~c["good"][:40])[0][:3]
    corr[bad[0]], corr[bad[1]], corr[bad[2]] = -1, 40, 2 ** 30
    o = run_ransac(c["src"][None], c["tgt"][None], corr[None], 512)
    assert o["pairs"][0] == 37
    assert staged(o, 0, c["src"], c["tgt"], corr, 512) >= 1
    assert not np.isin(o["trial_picks"][0], np.concatenate([bad, np.arange(40, 45)])).any()
    planted_recovered(o, 0, c)
    none = run_ransac(c["src"][None], c["tgt"][None], np.full((1, 45), -1), 65)
    assert staged(none, 0, c["src"], c["tgt"], np.full(45, -1), 65) == 0
    assert np.array_equal(none["R"][0], np.eye(3, dtype=F32)) and not none["t"].any()


@pytest.mark.parametrize("similarity", [mr.SIMILARITY, 0.0])
def test_a_nan_source_point_spoils_only_the_trials_that_pick_it(similarity):
    """The point is one of the pairs but not a planted one.  A trial that draws it fails the edge test (a NaN fails) -- or, with
    the edge test off, its pose is NaN: status 3; every other trial keeps its status, pose and count bit for bit."""
    c = mr.planted(257, 0.3)
    T = 2048
    clean = run_ransac(c["src"][None], c["tgt"][None], c["corr"][None], T, similarity=similarity)
    i0 = int(np.nonzero(~c["good"])[0][4])
    src = c["src"].copy()
    src[1, i0] = np.nan
    o = run_ransac(src[None], c["tgt"][None], c["corr"][None], T, similarity=similarity)
    staged(o, 0, src, c["tgt"], c["corr"], T, similarity=similarity)
    assert np.array_equal(o["trial_picks"], clean["trial_picks"])
    hit = (o["trial_picks"][0] == i0).any(1)
    assert 0 < hit.sum() < T
    for k in ("trial_status", "trial_inliers"):
        assert np.array_equal(o[k][0][~hit], clean[k][0][~hit]), k
    assert np.array_equal(bits(o["trial_pose"][0][~hit]), bits(clean["trial_pose"][0][~hit]))
    assert np.isin(o["trial_status"][0][hit], (1, 2) if similarity else (1, 3)).all()
    if not similarity:
        assert (o["trial_status"][0][hit] == 3).any() and np.isnan(o["trial_pose"][0][o["trial_status"][0] == 3]).all()
    for k in ("best_trial", "inliers", "R", "t"):
        assert np.array_equal(o[k], clean[k]), k


def test_a_batch_of_ransacs_is_its_clouds_alone_and_a_seed_changes_the_picks():
    clouds = [mr.planted(257, 0.3, seed=s) for s in range(3)]
    s = stack(clouds)
    T = 1024
    o = run_ransac(s["src"], s["tgt"], s["corr"], T)
    for b in range(3):
        alone = run_ransac(s["src"][b:b + 1], s["tgt"][b:b + 1], s["corr"][b:b + 1], T)
        for k in POSE_KEYS:
            assert np.array_equal(alone[k][0].view(np.int32), o[k][b].view(np.int32)), (b, k)
    assert np.array_equal(o["trial_picks"][0], o["trial_picks"][1])              # (all pairs valid: the same draws in every cloud)
    other = run_ransac(s["src"], s["tgt"], s["corr"], T, seed=mr.SEED + 1)
    assert not np.array_equal(other["trial_picks"], o["trial_picks"])
    staged(other, 2, s["src"][2], s["tgt"][2], s["corr"][2], T, seed=mr.SEED + 1)
    vcrnet_amd, _ = mods()
    r = vcrnet_amd.ransac_correspondences(dev(s["src"]), dev(s["tgt"]), dev(s["corr"]), mr.MAX_DIST, T, mr.SIMILARITY, mr.SEED)
    assert set(r) == {"R", "t", "best_trial", "inliers", "pairs"}
    for k in r:
        assert np.array_equal(r[k].cpu().numpy().view(np.int32), o[k].view(np.int32)), k


# ------------------------------------------------------------------------------------------------------------------ end to end

@pytest.mark.parametrize("N,k", [(600, 20), (1500, 30)])
def test_register_features_on_a_surface_without_symmetries(N, k):
    """The source is a rotated, shifted and permuted copy of the target.  The test counts the correct pairs among the device's
    own correspondences -- their share is the CPU chain's (match_restated.SURFACE_SHARES) within a few points, with estimated
    normals, whose sign is arbitrary (18 % of the one-way matches at 600 points, on the CPU too), and with normals oriented
    alike (99.7 %) --: the RANSAC's count must reach them, the closing fitness too; from there the ICP recovers the pose within
    the 1e-5 tests/test_hip_refine.py holds a loop on exact copies to; and the call is the composition of its calls."""
    vcrnet_amd, match = mods()
    c = mr.surface(N)
    src, tgt = dev(c["src"][None]), dev(c["tgt"][None])
    T = 4096
    ups = mr.surface_up(c)
    ns, nt = (dev(mr.orient(vcrnet_amd.estimate_normals(x, k)[0].cpu().numpy(), up)[None]) for x, up in zip((src, tgt), ups))
    for oriented, mutual in ((False, False), (False, True), (True, False), (True, True)):
        kw = dict(src_normals=ns, tgt_normals=nt) if oriented else {}
        res = vcrnet_amd.register_features(src, tgt, mr.MAX_DIST, k=k, mutual=mutual, trials=T, seed=mr.SEED, refine=mr.MAX_DIST, **kw)
        corr = res["corr"][0].cpu().numpy()
        paired = corr >= 0
        correct = int((corr[paired] == c["twin"][paired]).sum())
        share = correct / max(1, int(paired.sum()))
        Rr, tr = res["refined"]["R"][0].cpu().numpy().astype(np.float64), res["refined"]["t"][0].cpu().numpy().astype(np.float64)
        dR, dt = np.abs(Rr - c["R"]).max(), np.abs(tr - c["t"]).max()
        print(f"register_features N {N} k {k} oriented {oriented} mutual {mutual}: {int(paired.sum())} pairs, {correct} correct "
              f"({share:.3f}; CPU {mr.SURFACE_SHARES[(N, k, oriented, mutual)]}), RANSAC inliers {int(res['ransac_inliers'][0])} at trial "
              f"{int(res['best_trial'][0])}, fitness {float(res['fitness'][0]):.4f}, refined |dR| {dR:.2e} |dt| {dt:.2e} in "
              f"{int(res['refined']['iterations'][0])} rounds")
        assert int(res["pairs"][0]) == int(paired.sum()) and (paired.all() or mutual)
        assert share >= mr.SURFACE_SHARES[(N, k, oriented, mutual)] - mr.SHARE_SLACK
        assert int(res["ransac_inliers"][0]) >= correct
        assert float(res["fitness"][0]) >= F32(correct) / F32(N)
        assert dR <= 1e-5 and dt <= 1e-5, (dR, dt)
    # the composition, bit for bit (oriented and mutual, as the last run above)
    fs, ft = vcrnet_amd.compute_fpfh_feature(src, ns, k=k), vcrnet_amd.compute_fpfh_feature(tgt, nt, k=k)
    corr = vcrnet_amd.match_features(fs, ft, mutual=True)
    r = vcrnet_amd.ransac_correspondences(src, tgt, corr, mr.MAX_DIST, T, seed=mr.SEED)
    sc = vcrnet_amd.score_registration(src, tgt, r["R"], r["t"], mr.MAX_DIST)
    rf = vcrnet_amd.refine_registration(src, tgt, r["R"], r["t"], mr.MAX_DIST)
    assert torch.equal(res["corr"], corr)
    for key, want in (("R", r["R"]), ("t", r["t"]), ("best_trial", r["best_trial"]), ("pairs", r["pairs"]),
                      ("ransac_inliers", r["inliers"]), ("fitness", sc["fitness"]), ("inlier_rmse", sc["inlier_rmse"]),
                      ("inliers", sc["inliers"])):
        assert torch.equal(res[key].view(torch.int32), want.view(torch.int32)), key
    assert set(res["refined"]) == set(rf)
    for key in rf:
        assert torch.equal(res["refined"][key].view(torch.int32), rf[key].view(torch.int32)), key
    plain = vcrnet_amd.register_features(src, tgt, mr.MAX_DIST, k=k, trials=T, seed=mr.SEED, src_normals=ns, tgt_normals=nt)
    assert "refined" not in plain and torch.equal(plain["R"], r["R"]) and torch.equal(plain["corr"], corr)
    idx, d2 = vcrnet_amd.match_features(fs, ft, want_d2=True)
    one = match.feat_nn(fs, ft)
    assert torch.equal(idx, one["nn_idx"]) and torch.equal(d2, one["nn_d2"]) and idx.dtype == torch.int32
