"""vcr_nn_score_f32 on the GPU: nearest neighbours, fitness and inlier RMSE of a registration on the full clouds
(include/vcr_hip_score.h).

Where every step of the arithmetic is exact (points on a 0.25 lattice, signed-permutation poses) the comparison with the numpy
restatement (tests/nnscore_restated.py) is bit for bit, ties included; on random clouds the kernel's fp32 d2 is held to the
float64 distances of the same fp32 points within bounds derived from its rounding steps (u = 2^-24):
  d2 = fl(dz^2 + fl(dy^2 + fl(dx^2))) with dx = fl(p - q): each difference carries a relative u, squared 2u (+ u^2), and the
  three roundings of the chain add at most 3u  ->  |d2 - d64| <= 6u d64 (second-order terms are below 1e-13 d64);
  the kernel picks the smallest fp32 d2, so the float64 distance of its pick exceeds the float64 minimum by at most the two
  errors together, 12u relative -- and wherever the runner-up is further away than that, the pick IS the float64 arg-min.
Every launch form must return the same bits; every output element is written and nothing behind it."""
import numpy as np
import pytest
import torch

import nnscore_restated as nr
from test_hip_fps import lattice

pytestmark = pytest.mark.gpu

U = nr.U
SENTINEL_BYTE = 0x5A
GUARD = 64
OUTPUTS = ("nn_idx", "nn_d2", "inliers", "sum_d2", "fitness", "rmse")


def mods():
    import vcrnet_amd  # noqa: F401
    from vcrnet_amd import native, score
    return native, score


def forms():
    """Every pair of (source points per lane, target splits) the tests force, besides 0 = the plan's own."""
    _, score = mods()
    return [score.variant(q, s) for q in score.QUERIES_PER_LANE for s in (1, 2, 3)] + [score.variant(1, 128), score.variant(4, 7)]


def uniform(seed, B, N):
    return np.random.RandomState(seed).uniform(-1.0, 1.0, size=(B, 3, N)).astype(np.float32)


def lattice_batch(seed, B, N):
    return np.stack([lattice(seed + 31 * b, N) for b in range(B)])


def dev(x):
    return None if x is None else torch.from_numpy(np.ascontiguousarray(x)).cuda()


def run(src, tgt, R=None, t=None, max_dist=0.1, variant=0, check_fill=True):
    """numpy in, dict of numpy out; every output buffer is prefilled with the sentinel and carries a guard band: all of the
    output must have been overwritten, none of the band."""
    _, score = mods()
    o = score.nn_score(dev(src), dev(tgt), dev(R), dev(t), max_dist, variant=variant, guard=GUARD, prefill=SENTINEL_BYTE)
    torch.cuda.synchronize()
    out = {k: o[k].cpu().numpy() for k in OUTPUTS}
    if check_fill:
        for k in OUTPUTS:
            raw = o["_raw"][k]
            n = o[k].numel()
            band = raw[n:].view(torch.uint8).cpu().numpy()
            assert band.size == GUARD * raw.element_size() and (band == SENTINEL_BYTE).all(), (k, "guard band written")
            body = raw[:n].view(torch.uint8).cpu().numpy().reshape(n, -1)
            assert not (body == SENTINEL_BYTE).all(axis=1).any(), (k, "element left unwritten")
    return out


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view({4: np.int32, 8: np.int64}[a.dtype.itemsize])


def assert_same_bits(a, b, what):
    for k in OUTPUTS:
        assert np.array_equal(bits(a[k]), bits(b[k])), (what, k)


SIGNED_PERMUTATION = np.asarray([[0, -1, 0], [0, 0, 1], [-1, 0, 0]], np.float32)
LATTICE_SHIFT = np.asarray([0.5, -0.25, 0.75], np.float32)


@pytest.mark.parametrize("Ns,Nt", [(700, 40), (300, 2500), (1100, 1030)])
@pytest.mark.parametrize("posed", [False, True])
def test_exact_lattice_bit_for_bit_in_every_form(Ns, Nt, posed):
    """Every d2 is exact and ties are everywhere: the neighbour is numpy's first arg-min, d2 and the whole summary are the
    restatement's bits, at a max_dist that sits ON a lattice distance (d2 == max_dist^2 counts as an inlier)."""
    B = 2
    src, tgt = lattice_batch(11 + Ns, B, Ns), lattice_batch(12 + Nt, B, Nt)
    R = np.stack([SIGNED_PERMUTATION, SIGNED_PERMUTATION.T]) if posed else None
    t = np.stack([LATTICE_SHIFT, -LATTICE_SHIFT]) if posed else None
    max_dist = 0.5 if posed else 0.25                        # d2 = 0.25 / 0.0625: two lattice steps / one along an axis
    limit = np.float32(max_dist * max_dist)
    want = nr.score(src, tgt, R, t, max_dist)
    if Nt == 40 or posed:
        assert (want["nn_d2"] == limit).any() and (want["nn_d2"] > limit).any()   # the <= case is met, and so is its other side
    assert 0 < want["inliers"].min() and (want["nn_idx"] >= 0).all()
    for v in [0] + forms():
        got = run(src, tgt, R, t, max_dist, variant=v)
        assert np.array_equal(got["nn_idx"], want["nn_idx"]), v
        assert_same_bits(got, want, v)


def random_pose(seed, B):
    rs = np.random.RandomState(seed)
    R = []
    for _ in range(B):
        q, r = np.linalg.qr(rs.normal(size=(3, 3)))
        q = q * np.sign(np.diag(r))
        if np.linalg.det(q) < 0:
            q[:, 0] = -q[:, 0]
        R.append(q)
    return np.stack(R).astype(np.float32), rs.uniform(-0.5, 0.5, size=(B, 3)).astype(np.float32)


def test_the_transform_is_pose_steps():
    """score(src, tgt, R, t) == score(pose_step(R, t, src), tgt) in every output bit: the kernel moves the source as
    vcr_pose_step_f32 does."""
    native, _ = mods()
    B = 2
    src, tgt = uniform(21, B, 1500), uniform(22, B, 1300)
    R, t = random_pose(23, B)
    moved = native.pose_step(dev(R), dev(t), dev(src))[0].cpu().numpy()
    assert not np.array_equal(moved, src)
    base = run(moved, tgt, max_dist=0.08)
    assert 0 < base["inliers"].min() and base["inliers"].max() < 1500
    for v in [0] + forms():
        assert_same_bits(run(src, tgt, R, t, max_dist=0.08, variant=v), base, v)


def held_to_float64(got_idx, got_d2, p, q):
    """The three random-cloud checks on one cloud (p [3, n] the rows checked, q [3, Nt]); returns the rows left out of the
    arg-min check (runner-up within a relative 12u of the best)."""
    am, D, second = nr.nearest_f64(p, q)
    n = p.shape[1]
    assert (got_idx >= 0).all() and (got_idx < q.shape[1]).all()
    picked = sum((p[c].astype(np.float64) - q[c, got_idx].astype(np.float64)) ** 2 for c in range(3))
    assert (np.abs(got_d2.astype(np.float64) - picked) <= 6 * U * picked).all()
    assert (picked <= D * (1 + 12 * U)).all()
    clear = (second - D) > 12 * U * D
    assert np.array_equal(got_idx[clear], am[clear])
    return n - int(clear.sum())


@pytest.mark.parametrize("seed", [101, 102])
def test_random_clouds_against_float64(seed):
    B, Ns, Nt = 2, 3000, 5000
    src, tgt = uniform(seed, B, Ns), uniform(seed + 50, B, Nt)
    got = run(src, tgt, max_dist=0.05)
    left_out = sum(held_to_float64(got["nn_idx"][b], got["nn_d2"][b], src[b], tgt[b]) for b in range(B))
    assert left_out <= 1e-3 * B * Ns, left_out
    for b in range(B):                                       # the summary follows from the kernel's own neighbours
        c, s, f, r = nr.summary(got["nn_idx"][b], got["nn_d2"][b], 0.05)
        assert (got["inliers"][b], got["sum_d2"][b], got["fitness"][b], got["rmse"][b]) == (c, s, f, r)
        assert 0 < c < Ns


# one below, at and one above every capacity: the source points of a workgroup at 1, 2 and 4 per lane (256, 512, 1024), the LDS
# tile (1024 target points, and its multiple), a segment boundary of every forced split (Nt = 2 x 1024, 3 x 341, 7 x 147; with
# 128 splits most segments are empty or one point), the wave (64), and 1 and 2
EDGE_NS = [1, 2, 63, 64, 65, 255, 256, 257, 511, 512, 513, 1023, 1024, 1025, 2049]
EDGE_NT = [1, 2, 63, 64, 65, 127, 128, 129, 1022, 1023, 1024, 1025, 1028, 1029, 1030, 2047, 2048, 2049]


@pytest.mark.parametrize("Ns", EDGE_NS)
def test_edges_of_the_plan(Ns):
    """Ns x every Nt of the list (both Ns < Nt and Ns > Nt occur), lattice and random input: every forced form returns the bits
    of the automatic one, the lattice results are the restatement's, the random ones are held to float64, every output element
    is written and no guard band is."""
    left_out = rows = 0
    for k, Nt in enumerate(EDGE_NT):
        lat = k % 2 == 0
        src = lattice_batch(Ns + k, 1, Ns) if lat else uniform(Ns + k, 1, Ns)
        tgt = lattice_batch(Nt + 7 * k, 1, Nt) if lat else uniform(Nt + 7 * k, 1, Nt)
        auto = run(src, tgt, max_dist=0.25)
        if lat:
            want = nr.score(src, tgt, max_dist=0.25)
            assert np.array_equal(auto["nn_idx"], want["nn_idx"]), (Ns, Nt)
            assert_same_bits(auto, want, (Ns, Nt))
        else:
            left_out += held_to_float64(auto["nn_idx"][0], auto["nn_d2"][0], src[0], tgt[0])
            rows += Ns
        for v in forms():
            assert_same_bits(run(src, tgt, max_dist=0.25, variant=v), auto, (Ns, Nt, v))
    assert left_out <= 1e-3 * rows, (left_out, rows)


def test_edges_with_a_batch_and_a_pose():
    """B = 3 through the workgroup decode (cloud, source block, segment) at sizes on no boundary, Ns != Nt in both directions."""
    for Ns, Nt in ((777, 1300), (1300, 777)):
        src, tgt = lattice_batch(Ns, 3, Ns), lattice_batch(Nt + 1, 3, Nt)
        R = np.stack([SIGNED_PERMUTATION, np.eye(3, dtype=np.float32), SIGNED_PERMUTATION.T])
        t = np.stack([LATTICE_SHIFT, 0 * LATTICE_SHIFT, -LATTICE_SHIFT])
        want = nr.score(src, tgt, R, t, 0.5)
        for v in [0] + forms():
            got = run(src, tgt, R, t, 0.5, variant=v)
            assert np.array_equal(got["nn_idx"], want["nn_idx"]), (Ns, Nt, v)
            assert_same_bits(got, want, (Ns, Nt, v))


def test_large_once():
    """B = 1, Ns = 70 001, Nt = 131 072: 512 sampled rows against float64, inliers against a count of the kernel's own nn_d2."""
    Ns, Nt, max_dist = 70001, 131072, 0.02
    src, tgt = uniform(70001, 1, Ns), uniform(131072, 1, Nt)
    got = run(src, tgt, max_dist=max_dist)
    rows = np.sort(np.random.RandomState(9).choice(Ns, 512, replace=False))
    rows[0], rows[-1] = 0, Ns - 1
    left_out = held_to_float64(got["nn_idx"][0][rows], got["nn_d2"][0][rows], src[0][:, rows], tgt[0])
    assert left_out <= 1, left_out                           # 0.1 % of 512 rows, rounded up
    inl = got["nn_d2"][0] <= np.float32(max_dist) * np.float32(max_dist)
    assert got["inliers"][0] == inl.sum() and 0.05 * Ns < inl.sum() < 0.95 * Ns
    c, s, f, r = nr.summary(got["nn_idx"][0], got["nn_d2"][0], max_dist)
    assert (got["inliers"][0], got["sum_d2"][0], got["fitness"][0], got["rmse"][0]) == (c, s, f, r)


def test_non_finite_points():
    """NaN / +-inf target points are never chosen; a NaN source point reports (-1, +inf) and is no inlier; fitness and rmse stay
    finite; an all-NaN target cloud scores fitness 0, rmse 0."""
    B, Ns, Nt = 3, 600, 1500
    src, tgt = uniform(41, B, Ns), uniform(42, B, Nt)
    bad = [0, 5, 700, 1023, 1024, Nt - 1]
    tgt[0, 0, bad[0]] = np.nan
    tgt[0, 1, bad[1]] = np.inf
    tgt[0, 2, bad[2]] = -np.inf
    tgt[0, :, bad[3]] = np.nan
    tgt[0, 0, bad[4]] = np.inf
    tgt[0, 2, bad[5]] = np.nan
    src[0, 1, 17] = np.nan
    src[1, 0, 599] = np.inf
    tgt[2] = np.nan
    clean = np.delete(tgt[0], bad, axis=1)
    remap = np.delete(np.arange(Nt), bad)
    for v in [0] + forms():
        got = run(src, tgt, max_dist=0.1, variant=v)
        idx, d2 = got["nn_idx"], got["nn_d2"]
        assert not np.isin(idx[0], bad).any()
        for b, n in ((0, 17), (1, 599)):
            assert idx[b, n] == -1 and np.isposinf(d2[b, n])
        ok = np.ones(Ns, bool)
        ok[17] = False
        assert held_to_float64(remap.searchsorted(idx[0][ok]), d2[0][ok], src[0][:, ok], clean) == 0
        assert np.array_equal(remap[remap.searchsorted(idx[0][ok])], idx[0][ok])
        assert (idx[2] == -1).all() and np.isposinf(d2[2]).all()
        assert got["inliers"][2] == 0 and got["fitness"][2] == 0.0 and got["rmse"][2] == 0.0 and got["sum_d2"][2] == 0.0
        assert np.isfinite(got["fitness"]).all() and np.isfinite(got["rmse"]).all() and np.isfinite(got["sum_d2"]).all()
        for b in range(B):
            c, s, f, r = nr.summary(idx[b], d2[b], 0.1)
            assert (got["inliers"][b], got["sum_d2"][b], got["fitness"][b], got["rmse"][b]) == (c, s, f, r), (v, b)
        assert 0 < got["inliers"][0] < Ns - 1 and 0 < got["inliers"][1] < Ns - 1
    # max_dist^2 overflows to +inf: a point without a neighbour is still no inlier
    got = run(src, tgt, max_dist=1e30)
    assert got["inliers"].tolist() == [Ns - 1, Ns - 1, 0] and np.isfinite(got["rmse"]).all()


def test_run_to_run_on_two_streams():
    _, score = mods()
    src, tgt = dev(uniform(51, 2, 5000)), dev(uniform(52, 2, 7000))
    torch.cuda.synchronize()
    outs = []
    for _ in range(2):
        st = torch.cuda.Stream()
        with torch.cuda.stream(st):
            o = score.nn_score(src, tgt, max_dist=0.05)
        st.synchronize()
        outs.append({k: o[k].cpu().numpy() for k in OUTPUTS})
    assert_same_bits(outs[0], outs[1], "two streams")
    assert 0 < outs[0]["inliers"].min()


# ---------------------------------------------------------------- the Python API

def test_score_registration_api():
    import vcrnet_amd
    native, score = mods()
    B, Ns, Nt = 2, 900, 1400
    src, tgt = dev(uniform(61, B, Ns)), dev(uniform(62, B, Nt))
    Rn, tn = random_pose(63, B)
    R, t = dev(Rn), dev(tn)
    res = vcrnet_amd.score_registration(src, tgt, R, t, max_dist=0.1)
    assert sorted(res) == ["fitness", "inlier_rmse", "inliers"]
    assert res["fitness"].dtype == torch.float32 and res["inlier_rmse"].dtype == torch.float32 and res["inliers"].dtype == torch.int32
    assert all(v.shape == (B,) and v.is_cuda for v in res.values())
    full = vcrnet_amd.score_registration(src, tgt, R, t, max_dist=0.1, symmetric=True, want_nn=True)
    assert sorted(full) == ["fitness", "fitness_ba", "inlier_rmse", "inlier_rmse_ba", "inliers", "inliers_ba", "nn_d2", "nn_idx"]
    assert full["nn_idx"].dtype == torch.int64 and full["nn_idx"].shape == (B, Ns)
    assert full["nn_d2"].dtype == torch.float32 and full["nn_d2"].shape == (B, Ns)
    low = score.nn_score(src, tgt, R, t, 0.1)
    for a, b in (("fitness", "fitness"), ("inlier_rmse", "rmse"), ("inliers", "inliers"), ("nn_d2", "nn_d2")):
        assert torch.equal(full[a], low[b]) and (a == "nn_d2" or torch.equal(res[a], low[b]))
    assert torch.equal(full["nn_idx"], low["nn_idx"].long())
    assert torch.equal(full["inliers"], (low["nn_d2"] <= float(np.float32(0.1) * np.float32(0.1))).sum(1).int())
    # the _ba half: the swapped clouds under pose_step's inverse
    _, _, _, R_ba, t_ba = native.pose_step(R, t)
    back = score.nn_score(tgt, src, R_ba, t_ba, 0.1)
    for a, b in (("fitness_ba", "fitness"), ("inlier_rmse_ba", "rmse"), ("inliers_ba", "inliers")):
        assert torch.equal(full[a], back[b]) and full[a].shape == (B,)
    assert 0 < int(full["inliers_ba"].min()) and int(full["inliers_ba"].max()) < Nt
    # no pose: the identity, both ways
    ident = vcrnet_amd.score_registration(src, tgt, max_dist=0.1, symmetric=True)
    assert torch.equal(ident["fitness"], score.nn_score(src, tgt, max_dist=0.1)["fitness"])
    assert torch.equal(ident["fitness_ba"], score.nn_score(tgt, src, max_dist=0.1)["fitness"])


def test_score_registration_error_messages():
    import vcrnet_amd
    native, score = mods()
    a, b = torch.zeros(2, 3, 300, device="cuda"), torch.zeros(2, 3, 410, device="cuda")
    R, t = torch.eye(3, device="cuda").repeat(2, 1, 1), torch.zeros(2, 3, device="cuda")
    with pytest.raises(native.VcrHipError, match="no CPU fallback"):
        vcrnet_amd.score_registration(a.cpu(), b, max_dist=0.1)
    with pytest.raises(native.VcrHipError, match="same number of clouds"):
        vcrnet_amd.score_registration(a, torch.zeros(3, 3, 410, device="cuda"), max_dist=0.1)
    with pytest.raises(native.VcrHipError, match=r"\[B, 3, N\]"):
        vcrnet_amd.score_registration(a.transpose(1, 2), b, max_dist=0.1)
    for bad in (-0.1, float("nan"), float("inf")):
        with pytest.raises(native.VcrHipError, match="max_dist must be finite and >= 0"):
            vcrnet_amd.score_registration(a, b, max_dist=bad)
    with pytest.raises(native.VcrHipError, match="both R and t"):
        vcrnet_amd.score_registration(a, b, R=R, max_dist=0.1)
    with pytest.raises(native.VcrHipError, match=r"R must be \[B, 3, 3\]"):
        vcrnet_amd.score_registration(a, b, R=R[:1], t=t, max_dist=0.1)
    with pytest.raises(native.VcrHipError, match="vcr_nn_score_f32"):
        score.nn_score(a, b, max_dist=0.1, variant=3)
    with pytest.raises(native.VcrHipError, match="unsupported"):
        vcrnet_amd.score_registration(torch.zeros(1, 3, 131073, device="cuda"), b[:1], max_dist=0.1)


def test_a_pose_recovered_from_an_exact_rigid_copy_scores_fitness_one():
    """tgt = R src + t on the full clouds (2000 points, rounded to fp32 once); the pose is solved from 256 farthest-point
    samples and their twins.  max_dist is DERIVED: per coordinate the moved source differs from its twin by at most
      |R^ - R| |p| + |t^ - t|        the solve's error, measured against the true pose
      + g4 (|R^| |p| + |t^|)         the kernel's transform: a product, two fmas and an add, g4 = 4u / (1 - 4u)
      + u |q|                        the twin's own rounding
    (|.| summed over the row), and the twin is one of the candidates, so every nearest distance is within sqrt(3) times that;
    (1 + 8u) covers the 6u of the kernel's d2 and the rounding of max_dist^2."""
    import vcrnet_amd
    native, _ = mods()
    B, N, npoint = 2, 2000, 256
    src = uniform(71, B, N)
    Rn, tn = random_pose(72, B)
    tgt = (np.einsum("bij,bjn->bin", Rn.astype(np.float64), src.astype(np.float64)) + tn.astype(np.float64)[:, :, None]).astype(np.float32)
    s, q = dev(src), dev(tgt)
    idx, src_s = native.fps(s, npoint)
    twins = torch.gather(q, 2, idx.long().unsqueeze(1).expand(B, 3, npoint))
    rows = lambda x: torch.cat([x.transpose(1, 2), torch.zeros(B, npoint, 1, device="cuda")], 2).contiguous()   # noqa: E731
    R, t, _, _ = native.rigid_svd(rows(src_s), rows(twins))
    Rh, th = R.cpu().numpy().astype(np.float64), t.cpu().numpy().astype(np.float64)
    g4 = 4 * U / (1 - 4 * U)
    bound = 0.0
    for b in range(B):
        p = np.abs(src[b].astype(np.float64)).max(axis=1)                     # per-axis |p| maxima
        for c in range(3):
            e = (np.abs(Rh[b, c] - Rn[b, c].astype(np.float64)) * p).sum() + abs(th[b, c] - float(tn[b, c])) \
                + g4 * ((np.abs(Rh[b, c]) * p).sum() + abs(th[b, c])) + U * np.abs(tgt[b, c]).max()
            bound = max(bound, e)
    max_dist = np.sqrt(3.0) * bound * (1 + 8 * U)
    assert max_dist < 1e-4, max_dist                                          # (a pose error this size would be a failed solve)
    res = vcrnet_amd.score_registration(s, q, R, t, max_dist=max_dist, want_nn=True)
    assert res["fitness"].tolist() == [1.0, 1.0] and res["inliers"].tolist() == [N, N]
    assert float(res["inlier_rmse"].max()) <= max_dist
    # (the clouds are uniform: at this scale the nearest target point is the twin itself)
    assert torch.equal(res["nn_idx"], torch.arange(N, device="cuda").expand(B, N))


def test_register_sampled_with_a_score():
    """score=d: a ninth element, the dict for the FULL clouds under the returned pose; the first eight are bit-identical to the
    call without it, which still returns eight."""
    import vcrnet_amd
    from test_hip_forward import build_net
    from test_hip_fps import _pair
    net, _ = build_net()
    src, tgt = _pair(3000, 4100)
    s, t = dev(src), dev(tgt)
    with torch.no_grad():
        plain = vcrnet_amd.register_sampled(net, s, t, 1024)
        scored = vcrnet_amd.register_sampled(net, s, t, 1024, score=0.1)
    assert len(plain) == 8 and len(scored) == 9
    for a, b in zip(plain, scored[:8]):
        assert a.dtype == b.dtype and torch.equal(a.view(torch.int32) if a.dtype == torch.float32 else a,
                                                  b.view(torch.int32) if b.dtype == torch.float32 else b)
    direct = vcrnet_amd.score_registration(s, t, scored[2], scored[3], max_dist=0.1)
    assert sorted(scored[8]) == ["fitness", "inlier_rmse", "inliers"]
    for k in direct:
        assert torch.equal(scored[8][k], direct[k]) and scored[8][k].shape == (2,)
