"""vcr_consistency_f32 on the GPU (include/consistency/vcr_hip_consistency.h) against the numpy
restatement (tests/consistency_restated.py), held in stages as the RANSAC is in tests/test_hip_match.py: every stage is the
restatement fed the DEVICE's previous stage.  The degrees, the kept pairs, the adjacency's words, the members' words and
counts, the statuses, every seed's count, the winner and its pose's bits are equal exactly; a seed's pose -- a Jacobi SVD on
the device, LAPACK's in numpy -- is held by properties to the allowance the RANSAC's staged test uses for the same solve.
Every call runs with 4096 elements of guard behind outputs prefilled with 0xFF, the workspace prefilled likewise."""
import functools

import numpy as np
import pytest
import torch

import consistency_restated as cr
import match_restated as mr

pytestmark = pytest.mark.gpu

GUARD = 4096
BYTE = 0xFF
F32 = np.float32
TAU = 0.01
KEYS = ("R", "t", "best_seed", "inliers", "pairs", "deg", "kept", "adj", "seed_status", "seed_members", "seed_inliers",
        "seed_pose", "member")
SIZES = (0, 1, 2, 3, 63, 64, 65, 257, 1000, 5000)             # M: P < keep, P = keep, a full row of 4096 bits at 5000
KEEPS = (64, 128, 4096)


def mods():
    import vcrnet_amd
    from vcrnet_amd import consistency
    return vcrnet_amd, consistency


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


def run(src, tgt, corr, keep, seeds, tau=TAU, max_dist=TAU, ratio=0.5, min_length=0.0, variant=0):
    """src [B,3,Ns], tgt [B,3,Nt], corr [B,Ns] numpy -> dict of numpy arrays, want_stages."""
    _, consistency = mods()
    o = consistency.consistency(dev(src), dev(tgt), dev(np.asarray(corr).astype(np.int32)), max_dist, tau, keep, seeds, ratio,
                                min_length, want_stages=True, variant=variant, guard=GUARD, prefill=BYTE)
    torch.cuda.synchronize()
    guards_untouched(o)
    return {k: o[k].cpu().numpy() for k in KEYS}


def same(a, b, keys=KEYS):
    for k in keys:
        assert np.array_equal(np.ascontiguousarray(a[k]).view(np.uint8), np.ascontiguousarray(b[k]).view(np.uint8)), k


@functools.lru_cache(maxsize=None)
def cloud(M):
    """One cloud of M pairs and five source points without a partner: the RANSAC's planted recipe, a fifth of the pairs right."""
    if M == 0:
        c = dict(mr.planted(40, 0.5, extra=5))
        c["corr"] = np.full(45, -1, np.int32)
    else:
        c = dict(mr.planted(M, 1.0 if M <= 3 else 0.2, extra=5))
    for v in c.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return c


@functools.lru_cache(maxsize=None)
def restated_degree(M, min_length=0.0):
    c = cloud(M)
    pl, P, Q = cr.rows(c["src"], c["tgt"], c["corr"])
    return cr.degree(P, Q, TAU, min_length)


@functools.lru_cache(maxsize=None)
def restated_adjacency(M, keep):
    """From the restated degrees: the staged check uses it only after the device's degrees and kept pairs equalled them."""
    c = cloud(M)
    pl, P, Q = cr.rows(c["src"], c["tgt"], c["corr"])
    order = cr.kept_order(restated_degree(M), keep)
    return cr.adjacency(P[order], Q[order], TAU)


def staged(o, b, src, tgt, corr, keep, seeds, tau=TAU, max_dist=TAU, ratio=0.5, min_length=0.0, deg=None, adj=None):
    """The seven stages on cloud b of the device's result o.  deg, adj: the restatement's, where a cache holds them for these
    inputs.  Returns the number of valid seeds."""
    src, tgt, corr = np.asarray(src, F32), np.asarray(tgt, F32), np.asarray(corr, np.int64)
    Ns, W = src.shape[1], keep // 64
    pl, P, Q = cr.rows(src, tgt, corr)
    M = len(pl)
    assert o["pairs"][b] == M
    # stage 1: the degrees, in the source's numbering
    deg = cr.degree(P, Q, tau, min_length) if deg is None else deg
    assert np.array_equal(o["deg"][b], cr.deg_by_source(deg, pl, Ns))
    # stage 2: the kept pairs from the device's degrees
    order = cr.kept_order(o["deg"][b][pl], keep)
    Pn = len(order)
    assert Pn == min(M, keep)
    assert np.array_equal(o["kept"][b][:Pn], pl[order]) and (o["kept"][b][Pn:] == -1).all()
    # stage 3: the adjacency of the device's kept pairs
    at = np.searchsorted(pl, o["kept"][b][:Pn])
    Pk, Qk = P[at], Q[at]
    adj = cr.adjacency(Pk, Qk, tau, min_length) if adj is None else adj
    words = o["adj"][b].view(np.uint64)
    assert words.shape == (keep, W)
    assert np.array_equal(words[:Pn], cr.pack(adj, keep)) and not words[Pn:].any()
    # stage 4: the members from the device's adjacency
    S = min(Pn, seeds)
    adj_d = cr.unpack(words[:Pn], Pn)
    w, wmax = cr.second_order(adj_d, S)
    mem = cr.members(adj_d, w, wmax, ratio)
    member = o["member"][b].view(np.uint64)
    assert member.shape == (seeds, W)
    assert np.array_equal(member[:S], cr.pack(mem, keep)) and not member[S:].any()
    assert np.array_equal(o["seed_members"][b][:S], mem.sum(1)) and not o["seed_members"][b][S:].any()
    # stage 5: the statuses, and every solved pose a proper rotation that is optimal for its members' covariance -- the
    # allowance of test_hip_match.staged for the same solve (test_hip_refine's bounds for a step)
    status, pose, count = o["seed_status"][b], o["seed_pose"][b], o["seed_inliers"][b]
    assert status.shape == (seeds,) and np.isin(status, (0, 1, 3)).all()
    hyp = cr.hypotheses(Pk, Qk, cr.unpack(member[:S], Pn))
    for r, h in enumerate(hyp):
        if h is None:
            assert status[r] == 1 and not pose[r].any(), r
            continue
        finite = np.isfinite(pose[r]).all()
        assert status[r] == (0 if finite else 3), r
        if h["H"] is None:                                    # a non-finite sum: the pose is NaN
            assert np.isnan(pose[r]).all(), r
            continue
        assert finite, r
        R, tr = pose[r, :9].reshape(3, 3), pose[r, 9:]
        ortho = np.abs(R.T @ R - np.eye(3, dtype=F32)).max()
        det = abs(np.linalg.det(R.astype(F32)) - 1)
        assert ortho <= 1e-5 and det <= 1e-5, (r, ortho, det)
        R64 = R.astype(np.float64)
        short = (h["opt"] - np.trace(R64 @ h["H"])) / h["s1"]
        dt = np.abs(tr.astype(np.float64) - (h["qm"] - R64 @ h["pm"])).max()
        assert short <= 2e-6, (r, short)
        assert dt <= 1e-6 * max(1.0, np.abs(tr).max()), (r, dt)
    assert (status[S:] == 1).all() and not pose[S:].any()
    # stage 6: every valid seed's count over ALL pairs from the device's own pose
    live = np.nonzero(status == 0)[0]
    if len(live):
        assert np.array_equal(count[live], cr.counts(P, Q, pose[live], max_dist))
    assert (count[status != 0] == -1).all()
    # stage 7: the winner is the arg-max rule on the device's own counts
    bs, inl = mr.best(count, status == 0)
    assert (o["best_seed"][b], o["inliers"][b]) == (bs, inl)
    want = pose[bs] if bs >= 0 else cr.IDENTITY
    assert np.array_equal(bits(o["R"][b].reshape(9)), bits(want[:9])) and np.array_equal(bits(o["t"][b]), bits(want[9:]))
    return len(live)


@functools.lru_cache(maxsize=None)
def device_case(M, keep, seeds):
    c = cloud(M)
    o = run(c["src"][None], c["tgt"][None], c["corr"][None], keep, seeds)
    for v in o.values():
        v.setflags(write=False)
    return o


@pytest.mark.parametrize("keep", KEEPS)
@pytest.mark.parametrize("M", SIZES)
def test_consistency_staged_on_planted_correspondences(M, keep):
    c = cloud(M)
    good = np.nonzero(c["good"])[0]
    for seeds in (1, 8, keep):
        o = device_case(M, keep, seeds)
        valid = staged(o, 0, c["src"], c["tgt"], c["corr"], keep, seeds, deg=restated_degree(M), adj=restated_adjacency(M, keep))
        print(f"consistency M {M} keep {keep} seeds {seeds}: {valid} valid seeds, statuses "
              f"{np.bincount(o['seed_status'][0], minlength=4).tolist()}, best {o['best_seed'][0]} with {o['inliers'][0]}")
        if M == 0:
            assert (o["kept"] == -1).all() and (o["deg"] == -1).all() and not o["adj"].any() and not o["member"].any()
        if M < 3:                                             # no seed is valid: the identity
            assert valid == 0 and o["best_seed"][0] == -1 and o["inliers"][0] == 0 and (o["seed_inliers"] == -1).all()
            assert np.array_equal(o["R"][0], np.eye(3, dtype=F32)) and not o["t"].any()
        else:                                                 # the winner's members: the kept planted pairs and no other
            assert valid >= 1 and o["inliers"][0] >= len(good)
            kept = o["kept"][0][:min(M, keep)]
            members = kept[cr.unpack(o["member"][0, o["best_seed"][0]], min(M, keep))]
            assert np.array_equal(np.sort(members), np.intersect1d(good, kept))


@pytest.mark.parametrize("B", [1, 2])
def test_every_form_of_the_degree_pass_returns_the_same_bits(B):
    _, consistency = mods()
    clouds = [cloud(1000), mr.planted(1000, 0.2, seed=1, extra=5)][:B]
    s = {k: np.stack([c[k] for c in clouds]) for k in ("src", "tgt", "corr")}
    plan = run(s["src"], s["tgt"], s["corr"], 128, 8)
    assert np.array_equal(plan["deg"][0], cr.deg_by_source(restated_degree(1000), np.arange(1000), 1005))
    for Q, S in ((1, 1), (2, 1), (4, 1), (1, 3), (2, 7), (4, 128), (1, 128), (0, 5), (4, 0), (0, 0)):
        for pretest in (False, True):
            forced = run(s["src"], s["tgt"], s["corr"], 128, 8, variant=consistency.variant(Q, S, pretest))
            same(forced, plan)


def test_a_batch_is_its_clouds_alone():
    """Three clouds with different M (entries of corr set to -1): each returns its solo bits, and the public calls are views."""
    vcrnet_amd, _ = mods()
    clouds = [mr.planted(257, 0.3, seed=s, extra=5) for s in range(3)]
    s = {k: np.stack([c[k] for c in clouds]) for k in ("src", "tgt", "corr")}
    s["corr"][1, 100:] = -1
    s["corr"][2, ::3] = -1
    o = run(s["src"], s["tgt"], s["corr"], 128, 8)
    assert o["pairs"].tolist() == [257, 100, 171]
    for b in range(3):
        alone = run(s["src"][b:b + 1], s["tgt"][b:b + 1], s["corr"][b:b + 1], 128, 8)
        for k in KEYS:
            assert np.array_equal(np.ascontiguousarray(alone[k][0]).view(np.uint8), np.ascontiguousarray(o[k][b]).view(np.uint8)), (b, k)
        assert staged(o, b, s["src"][b], s["tgt"][b], s["corr"][b], 128, 8) >= 1
    args = dev(s["src"]), dev(s["tgt"]), dev(s["corr"])
    r = vcrnet_amd.consistency_registration(*args, TAU, keep=128, seeds=8)
    assert set(r) == {"R", "t", "inliers", "pairs", "best_seed"}
    for k in r:
        assert np.array_equal(bits(r[k].cpu().numpy()), bits(o[k])), k
    full = vcrnet_amd.consistency_registration(*args, TAU, keep=128, seeds=8, want_stages=True)
    assert set(full) == set(KEYS)
    for k in KEYS:
        assert np.array_equal(full[k].cpu().numpy().view(np.uint8), np.ascontiguousarray(o[k]).view(np.uint8)), k
    deg = vcrnet_amd.correspondence_consistency(*args, TAU)
    assert deg.dtype == torch.int32 and np.array_equal(deg.cpu().numpy(), o["deg"])
    pruned = vcrnet_amd.prune_correspondences(*args, TAU, 128).cpu().numpy()
    for b in range(3):
        stays = np.zeros(262, bool)
        stays[o["kept"][b][o["kept"][b] >= 0]] = True
        assert np.array_equal(pruned[b], np.where(stays, s["corr"][b], -1)) and (pruned[b] >= 0).sum() == min(128, o["pairs"][b])


def test_corr_entries_outside_the_target_are_no_pairs():
    c = mr.planted(40, 0.5, extra=5)                         # five source points at the end without a partner
    corr = c["corr"].astype(np.int64)
    bad = np.nonzero(~c["good"][:40])[0][:3]
    corr[bad[0]], corr[bad[1]], corr[bad[2]] = -1, 40, 2 ** 30
    o = run(c["src"][None], c["tgt"][None], corr[None], 64, 8)
    assert o["pairs"][0] == 37 and (o["deg"][0][np.concatenate([bad, np.arange(40, 45)])] == -1).all()
    assert staged(o, 0, c["src"], c["tgt"], corr, 64, 8) >= 1
    assert not np.isin(o["kept"][0], np.concatenate([bad, np.arange(40, 45)])).any()
    assert o["inliers"][0] == c["good"].sum()


@pytest.mark.parametrize("min_length", [0.0, 0.05])
def test_shared_target_points_and_duplicated_pairs(min_length):
    """Five wrong source points share the target point of a right pair (dt2 = 0 between them), and one of them is also a copy of
    that pair's source point (ds2 = dt2 = 0: compatible with its twin without a minimum length, not with one).  The twins see
    every other pair alike, so their degrees are equal and the lower position is kept first."""
    c = mr.planted(257, 0.3)
    src, corr = c["src"].copy(), c["corr"].copy()
    g = int(np.nonzero(c["good"])[0][5])
    wrong = np.nonzero(~c["good"])[0]
    share = wrong[wrong > g][:5]
    corr[share] = corr[g]
    twin = int(share[-1])
    src[:, twin] = src[:, g]
    o = run(src[None], c["tgt"][None], corr[None], 128, 8, min_length=min_length)
    assert staged(o, 0, src, c["tgt"], corr, 128, 8, min_length=min_length) >= 1
    deg, kept = o["deg"][0], o["kept"][0].tolist()
    assert deg[g] == deg[twin] and kept.index(g) < kept.index(twin)
    plain = run(c["src"][None], c["tgt"][None], c["corr"][None], 128, 8, min_length=min_length)
    assert deg[g] == plain["deg"][0][g] + (0 if min_length else 1)


def test_a_nan_source_point_has_degree_zero_and_spoils_no_other_vote():
    c = mr.planted(257, 0.3)
    i0 = int(np.nonzero(~c["good"])[0][4])
    src, without = c["src"].copy(), c["corr"].copy()
    src[1, i0] = np.nan
    without[i0] = -1
    o = run(src[None], c["tgt"][None], c["corr"][None], 4096, 8)
    staged(o, 0, src, c["tgt"], c["corr"], 4096, 8)
    clean = run(c["src"][None], c["tgt"][None], without[None], 4096, 8)
    others = np.arange(257) != i0
    assert o["deg"][0][i0] == 0 and np.array_equal(o["deg"][0][others], clean["deg"][0][others])
    same(o, clean, ("R", "t", "best_seed", "inliers", "seed_status", "seed_members", "seed_inliers", "seed_pose"))


def test_the_pre_test_hands_every_test_on_its_band_to_the_definition():
    """Points on a lattice along a line, source at 0.25 i, partner at 0.25 i + (i % 2) / 64, and tau = 1 / 64: every length is
    exact in fp32, and |ds - dt| is 0 or EXACTLY tau -- half of all tests sit on the limit, inside the pre-test's band, and take
    its fallback to the definition's expression.  Eight pairs share the partner of pair 0 (dt2 = 0: the other fallback).  Both
    forms of every pair count return the restatement's degrees, and the same bits in every output."""
    _, consistency = mods()
    M, tau = 600, 1.0 / 64
    i = np.arange(M)
    src, tgt = np.zeros((3, M), F32), np.zeros((3, M), F32)
    src[0], tgt[0] = 0.25 * i, 0.25 * i + (i % 2) * tau
    src[1], tgt[2] = 0.5, -1.0
    corr = i.astype(np.int32)
    corr[300:308] = 0
    pl, P, Q = cr.rows(src, tgt, corr)
    want = cr.deg_by_source(cr.degree(P, Q, tau), pl, M)
    on_the_limit = np.abs(np.abs(P[:, None, 0] - P[None, :, 0]) - np.abs(Q[:, None, 0] - Q[None, :, 0])) == F32(tau)
    assert on_the_limit.mean() > 0.4 and want.max() >= M - 10     # the limit is met, and it counts as compatible
    plain = run(src[None], tgt[None], corr[None], 128, 8, tau=tau, variant=consistency.variant(pretest=False))
    assert np.array_equal(plain["deg"][0], want)
    for Q_ in (1, 2, 4):
        for pretest in (False, True):
            same(run(src[None], tgt[None], corr[None], 128, 8, tau=tau, variant=consistency.variant(Q_, 3, pretest)), plain)


# ------------------------------------------------------------------------------------------------------------------ end to end

def pose_error(R, t, c):
    """(the angle of R R_planted^T in degrees, by its skew part; the largest |dt|)."""
    E = np.asarray(R, np.float64) @ c["R"].T
    sine = 0.5 * np.linalg.norm([E[2, 1] - E[1, 2], E[0, 2] - E[2, 0], E[1, 0] - E[0, 1]])
    return float(np.degrees(np.arctan2(sine, (np.trace(E) - 1) / 2))), float(np.abs(np.asarray(t, np.float64) - c["t"]).max())


def test_one_right_pair_in_a_hundred_returns_the_planted_pose():
    """planted(4000, 0.01): 40 right pairs among 4000.  (What ransac_correspondences makes of the same input is the ledger's to
    report: profiles/consistency_ledger.txt.)  The bounds are the restatement's in tests/test_consistency_cpu.py."""
    vcrnet_amd, _ = mods()
    c = mr.planted(4000, 0.01)
    r = vcrnet_amd.consistency_registration(dev(c["src"][None]), dev(c["tgt"][None]), dev(c["corr"][None]), TAU, keep=512,
                                            seeds=32, want_stages=True)
    good = np.nonzero(c["good"])[0]
    bs = int(r["best_seed"][0])
    kept = r["kept"][0].cpu().numpy()
    members = kept[cr.unpack(r["member"][0, bs].cpu().numpy(), 512)]
    deg, dt = pose_error(r["R"][0].cpu().numpy(), r["t"][0].cpu().numpy(), c)
    print(f"consistency_registration planted(4000, 0.01): best seed {bs}, {int(r['inliers'][0])} inliers, rotation {deg:.2e} deg, "
          f"|dt| {dt:.2e}")
    assert bs >= 0 and np.array_equal(np.sort(members), good) and int(r["inliers"][0]) >= len(good)
    assert deg <= 2e-5 and dt <= 2e-7, (deg, dt)


def test_register_features_by_consistency_on_a_surface_without_symmetries():
    """tests/test_hip_match.py's end-to-end case at 600 points with method="consistency": with estimated normals (18 % of the
    one-way matches right) and with normals oriented alike, one-way and mutual; from the global pose the ICP recovers the planted
    one within that test's 1e-5; and the call is the composition of its calls."""
    vcrnet_amd, _ = mods()
    N, k = 600, 20
    c = mr.surface(N)
    src, tgt = dev(c["src"][None]), dev(c["tgt"][None])
    ups = mr.surface_up(c)
    ns, nt = (dev(mr.orient(vcrnet_amd.estimate_normals(x, k)[0].cpu().numpy(), up)[None]) for x, up in zip((src, tgt), ups))
    for oriented, mutual in ((False, False), (False, True), (True, False), (True, True)):
        kw = dict(src_normals=ns, tgt_normals=nt) if oriented else {}
        res = vcrnet_amd.register_features(src, tgt, mr.MAX_DIST, k=k, mutual=mutual, refine=mr.MAX_DIST, method="consistency", **kw)
        corr = res["corr"][0].cpu().numpy()
        paired = corr >= 0
        correct = int((corr[paired] == c["twin"][paired]).sum())
        Rr, tr = res["refined"]["R"][0].cpu().numpy().astype(np.float64), res["refined"]["t"][0].cpu().numpy().astype(np.float64)
        dR, dt = np.abs(Rr - c["R"]).max(), np.abs(tr - c["t"]).max()
        print(f"register_features consistency N {N} oriented {oriented} mutual {mutual}: {int(paired.sum())} pairs, {correct} correct, "
              f"consistency inliers {int(res['consistency_inliers'][0])} at seed {int(res['best_seed'][0])}, fitness "
              f"{float(res['fitness'][0]):.4f}, refined |dR| {dR:.2e} |dt| {dt:.2e}")
        assert int(res["pairs"][0]) == int(paired.sum())
        assert int(res["consistency_inliers"][0]) >= correct
        assert dR <= 1e-5 and dt <= 1e-5, (dR, dt)
    fs, ft = vcrnet_amd.compute_fpfh_feature(src, ns, k=k), vcrnet_amd.compute_fpfh_feature(tgt, nt, k=k)
    corr = vcrnet_amd.match_features(fs, ft, mutual=True)
    kw = dict(keep=256, seeds=16, tau=0.02)
    r = vcrnet_amd.consistency_registration(src, tgt, corr, mr.MAX_DIST, **kw)
    sc = vcrnet_amd.score_registration(src, tgt, r["R"], r["t"], mr.MAX_DIST)
    res = vcrnet_amd.register_features(src, tgt, mr.MAX_DIST, k=k, method="consistency", consistency=kw, src_normals=ns, tgt_normals=nt)
    assert set(res) == {"fitness", "inlier_rmse", "inliers", "R", "t", "pairs", "best_seed", "consistency_inliers", "corr"}
    assert torch.equal(res["corr"], corr)
    for key, want in (("R", r["R"]), ("t", r["t"]), ("best_seed", r["best_seed"]), ("pairs", r["pairs"]),
                      ("consistency_inliers", r["inliers"]), ("fitness", sc["fitness"]), ("inlier_rmse", sc["inlier_rmse"]),
                      ("inliers", sc["inliers"])):
        assert torch.equal(res[key].view(torch.int32), want.view(torch.int32)), key


# ------------------------------------------------------------------------------------------------- streams and graph capture

def stream_call(src, tgt, corr):
    _, consistency = mods()
    return consistency.consistency(src, tgt, corr, TAU, keep=128, seeds=8, want_stages=True)


def stream_data(seed):
    c = mr.planted(1000, 0.2, seed=seed, extra=5)
    return {k: c[k][None] for k in ("src", "tgt", "corr")}


def test_the_call_is_ordered_on_a_side_stream_and_replays_from_a_graph():
    """tests/test_hip_streams.py's checks (a) and (b) with its harness: behind a delayed overwrite of its inputs on a side stream
    the call returns while the stream is busy and its outputs are the eager call's on the new data, byte for byte; captured
    once, its replays follow the buffers' contents."""
    import test_hip_streams as hs
    a, b = stream_data(1), stream_data(2)
    on_a, on_b = hs.eager(stream_call, a), hs.eager(stream_call, b)
    assert set(on_b) == set(KEYS) and hs.wrong(on_a, on_b)   # (the two data sets differ in what they return)
    busy, out = hs.side_stream(stream_call, a, b)
    assert busy, "the side stream was idle when the call returned: the delay is too short, or the call waits"
    assert not hs.wrong(out, on_b)
    first, again, back = hs.captured(stream_call, a, b)
    bad = hs.wrong(first, on_b), hs.wrong(again, on_b), hs.wrong(back, on_a)
    assert not any(bad), f"replays on (B, B again, A) differ from the eager calls in {bad}"
