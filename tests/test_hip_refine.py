"""vcr_refine_f32 on the GPU: the trimmed ICP on the full clouds (include/vcr_hip_refine.h).

The input is tests/refine_restated.py's recipe: a target of Nb points under a planted 40-degree pose, a source of Ns of them
plus 37 far points, a start 6 degrees and 0.04 off, max_dist 0.1.  What is checked:
  * recovery: every clean point ends on its twin, the pose is the planted one within the project's 1e-5 for an ICP loop
    (test_icp_loop), the residual within what that tolerance implies;
  * one step against the restatement's fp64 covariance, built from the device's own neighbours: the update is a proper
    rotation and optimal for that covariance (test_rigid_solve's bound and derivation);
  * in EVERY test the closing invariant: each returned evaluation output is bit-equal to nn_score(src, tgt, R_out, t_out);
  * every launch form, a cloud alone against the cloud in a batch, a NaN-prefilled workspace: the same bits;
  * every output element written, no guard band touched."""
import numpy as np
import pytest
import torch

import refine_restated as rr

pytestmark = pytest.mark.gpu

SENTINEL_BYTE = 0x5A
GUARD = 64
EVAL = ("nn_idx", "nn_d2", "inliers", "sum_d2", "fitness", "rmse")
POSE = ("R", "t", "R_ba", "t_ba", "iterations", "converged")
FAR = rr.FAR


def mods():
    import vcrnet_amd  # noqa: F401
    from vcrnet_amd import native, refine, score
    return native, refine, score


def dev(x):
    return None if x is None else torch.tensor(np.ascontiguousarray(x)).cuda()         # (a copy: the recipes are read-only)


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view({4: np.int32, 8: np.int64}[a.dtype.itemsize])


def assert_same_bits(a, b, what, keys=EVAL + POSE):
    for k in keys:
        assert np.array_equal(bits(a[k]), bits(b[k])), (what, k)


def run(src, tgt, R=None, t=None, max_dist=rr.MAX_DIST, prefill=SENTINEL_BYTE, **kw):
    """numpy in, dict of numpy out.  Every output buffer (and the workspace) is prefilled and carries a guard band: all of the
    output must have been overwritten, none of the band; and the closing invariant: the evaluation returned is nn_score's for
    the pose returned, bit for bit."""
    _, refine, score = mods()
    o = refine.refine(dev(src), dev(tgt), dev(R), dev(t), max_dist, guard=GUARD, prefill=prefill, **kw)
    torch.cuda.synchronize()
    out = {k: o[k].cpu().numpy() for k in EVAL + POSE}
    for k in EVAL + POSE:
        raw = o["_raw"][k]
        n = o[k].numel()
        band = raw[n:].view(torch.uint8).cpu().numpy()
        assert band.size == GUARD * raw.element_size() and (band == prefill).all(), (k, "guard band written")
        body = raw[:n].view(torch.uint8).cpu().numpy().reshape(n, -1)
        assert not (body == prefill).all(axis=1).any(), (k, "element left unwritten")
    s = score.nn_score(dev(src), dev(tgt), o["R"], o["t"], max_dist)
    assert_same_bits(out, {k: s[k].cpu().numpy() for k in EVAL}, "closing invariant", EVAL)
    Nt = tgt.shape[2]
    assert (out["nn_idx"] >= -1).all() and (out["nn_idx"] < Nt).all()
    # the inverse is pose_step's of the fp32 pose: the transpose's bits, and -R^T t
    assert np.array_equal(bits(out["R_ba"]), bits(out["R"].transpose(0, 2, 1)))
    ok = np.isfinite(out["t"]).all(axis=1)
    want = -np.einsum("bji,bj->bi", out["R"].astype(np.float64), out["t"].astype(np.float64))
    assert (np.abs(out["t_ba"][ok] - want[ok]) <= 1e-6 * np.maximum(1.0, np.abs(want[ok]).max(axis=1, keepdims=True))).all()
    return out


_RECIPES = {}


def recipe(seed, Nb, Ns, kind="cube", undisturbed=()):
    key = (seed, Nb, Ns, kind, tuple(undisturbed))
    if key not in _RECIPES:
        c = rr.batch(seed, Nb, Ns, kind, undisturbed)
        for v in c.values():
            v.setflags(write=False)
        _RECIPES[key] = c
    return _RECIPES[key]


def assert_recovered(o, c, Ns, clouds=range(3)):
    """The recovery checks on the clouds given: see test_recovery."""
    for b in clouds:
        assert o["converged"][b] == 1 and 1 <= o["iterations"][b] < 30, (b, o["iterations"][b])
        assert o["inliers"][b] == Ns and (o["nn_d2"][b, Ns:] > np.float32(rr.MAX_DIST) ** 2).all()
        assert np.array_equal(o["nn_idx"][b, :Ns], c["twin"][b]), b
        assert np.abs(o["R"][b] - c["R"][b]).max() <= 1e-5 and np.abs(o["t"][b] - c["t"][b]).max() <= 1e-5
        # per coordinate the residual of a pose that far off: three |dR| |p| and |dt|
        assert o["rmse"][b] <= np.sqrt(3.0) * (3e-5 * np.abs(c["src"][b, :, :Ns]).max() + 1e-5)
        assert o["fitness"][b] == np.float32(Ns) / np.float32(Ns + FAR)


@pytest.mark.parametrize("Nb,Ns", rr.SHAPES)
@pytest.mark.parametrize("kind", ["cube", "torus"])
def test_recovery(kind, Nb, Ns):
    c = recipe(10 + Ns, Nb, Ns, kind)
    o = run(c["src"], c["tgt"], c["R0"], c["t0"])
    assert_recovered(o, c, Ns)


@pytest.mark.parametrize("Nb,Ns", [(1500, 1100), (700, 300)])
def test_one_step_against_the_restatement(Nb, Ns):
    """max_iterations = 1, thresholds 0.  The update is recovered in fp64 from the composed (R_out, t_out) and the start, and
    held to the fp64 covariance of the device's own iteration-0 neighbours:
      a proper rotation          |R R^T - I|, |det - 1| <= 1e-6 (entries rounded to fp32 allow 1.8e-7, twice: R_out and R0)
      optimal                    (opt - tr(R H64)) / s1 <= 2e-6 (test_rigid_solve's bound: second order in the pose error, and
                                 rounding R to fp32 moves the trace by at most 9 * 2^-24 s1)
      t = qm - R pm              within 1e-6 max(1, |t|)."""
    _, _, score = mods()
    c = recipe(20 + Ns, Nb, Ns)
    zero = run(c["src"], c["tgt"], c["R0"], c["t0"], max_iterations=0)
    s = score.nn_score(dev(c["src"]), dev(c["tgt"]), dev(c["R0"]), dev(c["t0"]), rr.MAX_DIST)
    assert_same_bits(zero, {k: s[k].cpu().numpy() for k in EVAL}, "iteration-0 neighbours", EVAL)
    assert zero["iterations"].tolist() == [0, 0, 0] and zero["converged"].tolist() == [0, 0, 0]
    assert np.array_equal(bits(zero["R"]), bits(c["R0"])) and np.array_equal(bits(zero["t"]), bits(c["t0"]))
    one = run(c["src"], c["tgt"], c["R0"], c["t0"], max_iterations=1, rel_fitness=0.0, rel_rmse=0.0)
    assert one["iterations"].tolist() == [1, 1, 1] and one["converged"].tolist() == [0, 0, 0]
    for b in range(3):
        up = rr.step(c["src"][b], c["tgt"][b], c["R0"][b], c["t0"][b], zero["nn_idx"][b], zero["nn_d2"][b], rr.MAX_DIST)
        assert up["n"] == zero["inliers"][b] and 3 <= up["n"] < Ns + FAR
        R0, t0 = c["R0"][b].astype(np.float64), c["t0"][b].astype(np.float64)
        R = one["R"][b].astype(np.float64) @ R0.T               # R_out = R R0, t_out = R t0 + t
        t = one["t"][b].astype(np.float64) - R @ t0
        ortho, det = np.abs(R @ R.T - np.eye(3)).max(), abs(np.linalg.det(R) - 1)
        short = (up["opt"] - np.trace(R @ up["H"])) / up["s1"]
        dt = np.abs(t - (up["qm"] - R @ up["pm"])).max()
        print(f"refine step Nb {Nb} Ns {Ns} cloud {b}: n {up['n']} |RR^T-I| {ortho:.1e} |det-1| {det:.1e} (opt-tr(R H64))/s1 "
              f"{short:.1e} |t-(qm-R pm)| {dt:.1e} |R-R64| {np.abs(R - up['R']).max():.1e}")
        assert ortho <= 1e-6 and det <= 1e-6, (ortho, det)
        assert short <= 2e-6, short
        assert dt <= 1e-6 * max(1.0, np.abs(t).max()), dt
        assert 0 < np.abs(one["R"][b] - c["R0"][b]).max()        # (a step was taken)


def test_every_launch_form_returns_the_same_bits():
    """Ns = 1100 (+ 37), Nt = 1500: past one 1024-point tile, a ragged last tile, a ragged last block."""
    _, refine, _ = mods()
    c = recipe(31, 1500, 1100)
    auto = run(c["src"], c["tgt"], c["R0"], c["t0"])
    assert_recovered(auto, c, 1100)
    for q in (1, 2, 4):
        for s in (1, 3, 128):
            v = refine.variant(q, s)
            assert_same_bits(run(c["src"], c["tgt"], c["R0"], c["t0"], variant=v), auto, (q, s))


def test_a_cloud_does_not_depend_on_its_batch():
    """B = 3 against the three clouds alone.  Cloud 1 starts ON the planted pose and stops rounds before the others: they run on
    behind its closed gate, and its outputs stay as its last evaluation wrote them."""
    c = recipe(41, 1500, 1100, undisturbed=(1,))
    whole = run(c["src"], c["tgt"], c["R0"], c["t0"])
    assert_recovered(whole, c, 1100)
    assert whole["iterations"][1] + 2 <= min(whole["iterations"][0], whole["iterations"][2]), whole["iterations"]
    for b in range(3):
        alone = run(c["src"][b:b + 1], c["tgt"][b:b + 1], c["R0"][b:b + 1], c["t0"][b:b + 1])
        assert_same_bits(alone, {k: whole[k][b:b + 1] for k in EVAL + POSE}, b)


@pytest.mark.parametrize("Ns", [255, 256, 257])
def test_edges_of_the_source_block_against_five_target_points(Ns):
    """Nt = 5: every source point is one of the five target points, jittered by 0.01 and moved off by a small pose."""
    rs = np.random.RandomState(Ns)
    tgt = rs.uniform(0, 1, (1, 3, 5)).astype(np.float32)
    pick = rs.randint(0, 5, Ns)
    clean = tgt[0][:, pick].astype(np.float64) + rs.uniform(-0.01, 0.01, (3, Ns))
    Rd, td = rr.rotation(rs.normal(size=3), 2.0), rs.uniform(-0.01, 0.01, 3)
    src = (Rd.T @ (clean - td[:, None])).astype(np.float32)[None]
    o = run(src, tgt)
    assert o["converged"][0] == 1 and 1 <= o["iterations"][0] < 30 and o["inliers"][0] == Ns
    assert np.array_equal(o["nn_idx"][0], pick)
    R = o["R"][0].astype(np.float64)
    assert np.abs(R @ R.T - np.eye(3)).max() <= 1e-6 and abs(np.linalg.det(R) - 1) <= 1e-6
    assert o["rmse"][0] <= 0.01 * np.sqrt(3.0)
    for v in (257, 4 | (2 << 8)):                            # (1, 1) and (4, 2) forced
        assert_same_bits(run(src, tgt, variant=v), o, (Ns, v))


def test_too_few_inliers_leave_the_pose():
    c = recipe(10 + 300, 700, 300)
    # one point against one point
    one = run(c["src"][:1, :, :1], c["tgt"][:1, :, :1], c["R0"][:1], c["t0"][:1], max_dist=10.0)
    assert one["inliers"].tolist() == [1] and one["iterations"].tolist() == [0] and one["converged"].tolist() == [0]
    assert np.array_equal(bits(one["R"]), bits(c["R0"][:1])) and np.array_equal(bits(one["t"]), bits(c["t0"][:1]))
    # two clean points and two far ones against the clean two, from the identity
    src = np.ascontiguousarray(c["src"][:1][:, :, [0, 1, 300, 301]])
    two = run(src, np.ascontiguousarray(src[:, :, :2]))
    assert two["inliers"].tolist() == [2] and two["iterations"].tolist() == [0] and two["converged"].tolist() == [0]
    assert np.array_equal(two["R"][0], np.eye(3, dtype=np.float32)) and not two["t"].any()
    assert two["nn_idx"][0, :2].tolist() == [0, 1] and two["fitness"][0] == 0.5 and two["rmse"][0] == 0.0


def test_more_source_than_target_points():
    """Ns = 2100 (+ 37) against Nt = 700: the source repeats target points."""
    c = recipe(51, 700, 2100)
    o = run(c["src"], c["tgt"], c["R0"], c["t0"])
    assert_recovered(o, c, 2100)


def test_no_iterations_and_no_distance():
    _, _, score = mods()
    c = recipe(20 + 1100, 1500, 1100)
    # max_iterations = 0: the score of the input pose (run() has compared it with nn_score's), from the identity too
    o = run(c["src"], c["tgt"], max_iterations=0)
    assert np.array_equal(o["R"], np.broadcast_to(np.eye(3, dtype=np.float32), (3, 3, 3))) and not o["t"].any()
    assert o["iterations"].tolist() == [0, 0, 0] and o["converged"].tolist() == [0, 0, 0]
    # max_dist = 0 from a disturbed start: nothing coincides, nothing moves
    o = run(c["src"], c["tgt"], c["R0"], c["t0"], max_dist=0.0)
    assert o["inliers"].tolist() == [0, 0, 0] and o["iterations"].tolist() == [0, 0, 0] and o["converged"].tolist() == [0, 0, 0]
    assert np.array_equal(bits(o["R"]), bits(c["R0"])) and o["fitness"].tolist() == [0.0] * 3 and o["rmse"].tolist() == [0.0] * 3
    # max_dist = 0 on a copy: every point is its own neighbour at distance 0; the update is the identity up to fp64 rounding
    cp = np.ascontiguousarray(c["tgt"][:, :, :900])
    o = run(cp, c["tgt"], max_dist=0.0)
    assert o["inliers"].tolist() == [900] * 3 and o["converged"].tolist() == [1, 1, 1] and o["iterations"].tolist() == [1, 1, 1]
    assert np.array_equal(o["nn_idx"], np.broadcast_to(np.arange(900), (3, 900))) and o["rmse"].tolist() == [0.0] * 3
    assert np.abs(o["R"] - np.eye(3, dtype=np.float32)).max() <= 1e-6 and np.abs(o["t"]).max() <= 1e-6


def test_a_nan_prefilled_workspace_changes_nothing():
    c = recipe(31, 1500, 1100)
    assert_same_bits(run(c["src"], c["tgt"], c["R0"], c["t0"], prefill=0xFF), run(c["src"], c["tgt"], c["R0"], c["t0"]), "prefill")


def test_a_nan_source_point_stays_in_its_cloud():
    """One NaN coordinate in cloud 0 (a clean point, so that cloud ends one inlier short): clouds 1 and 2 are bit-identical to
    the clean batch, every nn_idx stays in [-1, Nt) (run() checks it), the point itself has no neighbour."""
    c = recipe(31, 1500, 1100)
    clean = run(c["src"], c["tgt"], c["R0"], c["t0"])
    src = c["src"].copy()
    src[0, 1, 123] = np.nan
    o = run(src, c["tgt"], c["R0"], c["t0"])
    assert_same_bits({k: o[k][1:] for k in EVAL + POSE}, {k: clean[k][1:] for k in EVAL + POSE}, "the other clouds")
    assert o["nn_idx"][0, 123] == -1 and np.isposinf(o["nn_d2"][0, 123])
    assert o["inliers"][0] == 1100 - 1 and o["converged"][0] == 1 and np.isfinite(o["R"]).all() and np.isfinite(o["rmse"]).all()
    keep = np.arange(1100) != 123
    assert np.array_equal(o["nn_idx"][0, :1100][keep], c["twin"][0][keep])
    assert np.abs(o["R"][0] - c["R"][0]).max() <= 1e-5 and np.abs(o["t"][0] - c["t"][0]).max() <= 1e-5


# ---------------------------------------------------------------- the Python API

def test_refine_registration_api_and_error_messages():
    import vcrnet_amd
    native, refine, _ = mods()
    c = recipe(10 + 300, 700, 300)
    s, q, R0, t0 = dev(c["src"]), dev(c["tgt"]), dev(c["R0"]), dev(c["t0"])
    res = vcrnet_amd.refine_registration(s, q, R0, t0, max_dist=rr.MAX_DIST)
    assert sorted(res) == ["R", "R_ba", "converged", "fitness", "inlier_rmse", "inliers", "iterations", "t", "t_ba"]
    full = vcrnet_amd.refine_registration(s, q, R0, t0, max_dist=rr.MAX_DIST, want_nn=True)
    assert sorted(full) == sorted(list(res) + ["nn_idx", "nn_d2"])
    assert full["nn_idx"].dtype == torch.int64 and full["nn_idx"].shape == (3, 300 + FAR) and full["nn_d2"].dtype == torch.float32
    low = refine.refine(s, q, R0, t0, rr.MAX_DIST)
    closing = vcrnet_amd.score_registration(s, q, full["R"], full["t"], max_dist=rr.MAX_DIST, want_nn=True)
    for k in ("fitness", "inlier_rmse", "inliers", "nn_idx", "nn_d2"):           # the closing invariant, through the public API
        assert torch.equal(full[k], closing[k]), k
    for a, b in (("R", "R"), ("t", "t"), ("R_ba", "R_ba"), ("t_ba", "t_ba"), ("fitness", "fitness"), ("inlier_rmse", "rmse"),
                 ("inliers", "inliers"), ("iterations", "iterations"), ("converged", "converged")):
        assert torch.equal(res[a], low[b]) and torch.equal(full[a], low[b]) and res[a].is_cuda, a
    assert torch.equal(full["nn_idx"], low["nn_idx"].long()) and torch.equal(full["nn_d2"], low["nn_d2"])
    assert res["inliers"].dtype == res["iterations"].dtype == res["converged"].dtype == torch.int32
    assert res["R"].shape == (3, 3, 3) and res["t"].shape == (3, 3) and res["converged"].tolist() == [1, 1, 1]
    with pytest.raises(native.VcrHipError, match="no CPU fallback"):
        vcrnet_amd.refine_registration(s.cpu(), q, max_dist=0.1)
    with pytest.raises(native.VcrHipError, match="same number of clouds"):
        vcrnet_amd.refine_registration(s, q[:2], max_dist=0.1)
    with pytest.raises(native.VcrHipError, match=r"\[B, 3, N\]"):
        vcrnet_amd.refine_registration(s.transpose(1, 2), q, max_dist=0.1)
    for name in ("max_dist", "rel_fitness", "rel_rmse"):
        for bad in (-0.1, float("nan"), float("inf")):
            with pytest.raises(native.VcrHipError, match=f"{name} must be finite and >= 0"):
                vcrnet_amd.refine_registration(s, q, **{"max_dist": 0.1, name: bad})
    with pytest.raises(native.VcrHipError, match="max_iterations must be >= 0"):
        vcrnet_amd.refine_registration(s, q, max_dist=0.1, max_iterations=-1)
    with pytest.raises(native.VcrHipError, match="both R and t"):
        vcrnet_amd.refine_registration(s, q, R=R0, max_dist=0.1)
    with pytest.raises(native.VcrHipError, match=r"R must be \[B, 3, 3\]"):
        vcrnet_amd.refine_registration(s, q, R=R0[:1], t=t0, max_dist=0.1)
    with pytest.raises(native.VcrHipError, match="vcr_refine_f32"):
        refine.refine(s, q, max_dist=0.1, variant=3)
    with pytest.raises(native.VcrHipError, match="unsupported"):
        vcrnet_amd.refine_registration(torch.zeros(1, 3, 131073, device="cuda"), q[:1], max_dist=0.1)
    with pytest.raises(native.VcrHipError, match="unsupported"):
        vcrnet_amd.refine_registration(s, q, max_dist=0.1, max_iterations=refine.MAX_ITERATIONS + 1)


def test_register_sampled_with_a_refinement():
    """refine=d: one more element, the dict for the FULL clouds from the network's pose, after the score's if both are given;
    elements 0-7 are bit-identical to the call without it."""
    import vcrnet_amd
    from test_hip_forward import build_net
    from test_hip_fps import _pair
    net, _ = build_net()
    src, tgt = _pair(3000, 4100)
    s, t = dev(src), dev(tgt)
    with torch.no_grad():
        plain = vcrnet_amd.register_sampled(net, s, t, 1024)
        refined = vcrnet_amd.register_sampled(net, s, t, 1024, refine=0.1)
        both = vcrnet_amd.register_sampled(net, s, t, 1024, score=0.1, refine=0.1)
    assert len(plain) == 8 and len(refined) == 9 and len(both) == 10
    for other in (refined, both):
        for a, b in zip(plain, other[:8]):
            assert a.dtype == b.dtype and torch.equal(a.view(torch.int32) if a.dtype == torch.float32 else a,
                                                      b.view(torch.int32) if b.dtype == torch.float32 else b)
    direct = vcrnet_amd.refine_registration(s, t, plain[2], plain[3], max_dist=0.1)
    closing = vcrnet_amd.score_registration(s, t, refined[8]["R"], refined[8]["t"], max_dist=0.1)
    for k in ("fitness", "inlier_rmse", "inliers"):                              # the closing invariant
        assert torch.equal(refined[8][k].view(torch.int32), closing[k].view(torch.int32)), k
    scored = vcrnet_amd.score_registration(s, t, plain[2], plain[3], max_dist=0.1)
    assert sorted(refined[8]) == sorted(direct) and sorted(both[8]) == sorted(scored)
    for k in direct:
        for got in (refined[8], both[9]):
            a, b = got[k], direct[k]
            assert a.shape == b.shape and a.shape[0] == 2
            assert torch.equal(a.view(torch.int32) if a.dtype == torch.float32 else a, b.view(torch.int32) if b.dtype == torch.float32 else b), k
    for k in scored:
        assert torch.equal(both[8][k], scored[k])
