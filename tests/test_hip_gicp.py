"""vcr_refine_gicp_f32 on the GPU: the plane-to-plane refinement on the full clouds (include/vcr_hip_gicp.h, DESIGN.md section
4.13).

The input is tests/gicp_restated.py's recipe -- refine_restated.batch on the torus at its first two shapes, B = 3, with the
analytic normals of both clouds -- and one tiny case (B = 1, Ns = 5, Nt = 7).  Ns is never a multiple of 256 and the FAR points
are lanes within Ns that pair with nothing: both kinds of lane the merge has to mask.  What is checked:
  * one update from the given start against gicp_restated.gicp_step on the device's own iteration-0 neighbours (the scan is
    bit-defined): |dR|, |dt| <= 2^-22 + 64 cond(A) 2^-53 (tests/test_gicp_cpu.py holds every recipe to cond(A) <= 1e6);
  * the whole loop, ten updates, against gicp_restated.gicp_icp and the planted pose: the device's rotation and translation
    errors are at most twice the restatement's plus 2^-20 (the margin: neighbour sets may part after the first round);
  * every launch form, a cloud alone against the cloud in a batch, the normals under any change of sign: the same bits;
  * the stops, NaN normals, the mask;
  * in EVERY run the closing invariant -- each returned evaluation output is bit-equal to nn_score(src, tgt, R_out, t_out) --
    every output element written and no guard band touched;
  * refine_registration and register_sampled with method "generalized", and the other methods as they were."""
import os

import numpy as np
import pytest
import torch

import gicp_restated as gr
import plane_restated as pr
import refine_restated as rr

pytestmark = pytest.mark.gpu

SENTINEL_BYTE = 0x5A
GUARD = 64
EVAL = ("nn_idx", "nn_d2", "inliers", "sum_d2", "fitness", "rmse")
POSE = ("R", "t", "R_ba", "t_ba", "iterations", "converged")
FAR = rr.FAR
SHAPES = rr.SHAPES[:2]
LEDGER = []


def _emit(line):
    print(line)
    LEDGER.append(line)
    out = os.environ.get("VCR_LEDGER_DIR", "")
    if os.path.isdir(out):
        path = os.path.join(out, "gicp_ledger.txt")
        if len(LEDGER) == 1:                                 # a new table: which kernel sources it measures
            import vcrnet_amd  # noqa: F401
            from vcrnet_amd import build as vb
            with open(path, "w") as f:
                f.write(f"# kernel_sources_sha16={vb.sources_sha16()}\n")
        with open(path, "a") as f:
            f.write(line + "\n")


def mods():
    import vcrnet_amd  # noqa: F401
    from vcrnet_amd import gicp, refine, score
    return gicp, refine, score


def dev(x):
    return None if x is None else torch.tensor(np.ascontiguousarray(x)).cuda()         # (a copy: the recipes are read-only)


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view({4: np.int32, 8: np.int64}[a.dtype.itemsize])


def assert_same_bits(a, b, what, keys=EVAL + POSE):
    for k in keys:
        assert np.array_equal(bits(a[k]), bits(b[k])), (what, k)


def run(src, tgt, nrm_s, nrm_t, R=None, t=None, max_dist=rr.MAX_DIST, prefill=SENTINEL_BYTE, **kw):
    """numpy in, dict of numpy out; test_hip_plane.run's checks: every output overwritten, no guard band touched, the closing
    invariant, the inverse pose."""
    gicp, _, score = mods()
    o = gicp.refine_gicp(dev(src), dev(tgt), dev(nrm_s), dev(nrm_t), dev(R), dev(t), max_dist, guard=GUARD, prefill=prefill, **kw)
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
    assert (out["nn_idx"] >= -1).all() and (out["nn_idx"] < tgt.shape[2]).all()
    assert np.array_equal(bits(out["R_ba"]), bits(out["R"].transpose(0, 2, 1)))
    return out


def go(c, **kw):
    return run(c["src"], c["tgt"], c["nrm_s"], c["nrm_t"], c["R0"], c["t0"], **kw)


def cloud(c, b):
    return {k: c[k][b:b + 1] for k in ("src", "tgt", "nrm_s", "nrm_t", "R0", "t0")}


_RECIPES = {}


def recipe(seed, Nb, Ns, undisturbed=()):
    """gicp_restated.batch, computed once, read-only."""
    key = (seed, Nb, Ns, tuple(undisturbed))
    if key not in _RECIPES:
        _RECIPES[key] = gr.batch(seed, Nb, Ns, undisturbed)
    return _RECIPES[key]


def _one_update(c, name, B):
    _, _, score = mods()
    zero = go(c, max_iterations=0)
    s = score.nn_score(dev(c["src"]), dev(c["tgt"]), dev(c["R0"]), dev(c["t0"]), rr.MAX_DIST)
    assert_same_bits(zero, {k: s[k].cpu().numpy() for k in EVAL}, "max_iterations = 0: the score of the start", EVAL)
    assert zero["iterations"].tolist() == [0] * B and zero["converged"].tolist() == [0] * B
    assert np.array_equal(bits(zero["R"]), bits(c["R0"])) and np.array_equal(bits(zero["t"]), bits(c["t0"]))
    one = go(c, max_iterations=1, rel_fitness=0.0, rel_rmse=0.0)
    assert one["iterations"].tolist() == [1] * B and one["converged"].tolist() == [0] * B
    for b in range(B):
        up = gr.gicp_step(c["src"][b], c["tgt"][b], c["nrm_s"][b], c["nrm_t"][b], c["R0"][b], c["t0"][b], zero["nn_idx"][b],
                          zero["nn_d2"][b], rr.MAX_DIST)
        assert up["n"] == zero["inliers"][b] >= 3
        R0, t0 = c["R0"][b].astype(np.float64), c["t0"][b].astype(np.float64)
        dR = np.abs(one["R"][b] - up["R"] @ R0).max()
        dt = np.abs(one["t"][b] - (up["R"] @ t0 + up["t"])).max()
        bound = 2.0 ** -22 + 64 * up["cond"] * 2.0 ** -53
        _emit(f"gicp step {name} cloud {b}: n {up['n']} cond(A) {up['cond']:.3e} |dR| {dR:.2e} |dt| {dt:.2e} bound {bound:.2e}")
        assert up["cond"] <= 1e6
        assert dR <= bound and dt <= bound, (dR, dt, bound)
        assert 0 < np.abs(one["R"][b] - c["R0"][b]).max()        # (a step was taken)
    return zero, one


@pytest.mark.parametrize("Nb,Ns", SHAPES)
def test_one_update_against_the_restatement(Nb, Ns):
    zero, _ = _one_update(recipe(20 + Ns, Nb, Ns), f"Nb {Nb} Ns {Ns}", 3)
    assert (zero["inliers"] < Ns + FAR).all()                   # (lanes within Ns that are no inliers)


def test_one_update_of_the_tiny_case():
    c = gr.tiny()
    assert c["src"].shape == (1, 3, 5) and c["tgt"].shape == (1, 3, 7)
    zero, _ = _one_update(c, "tiny Ns 5 Nt 7", 1)
    assert zero["inliers"].tolist() == [5]


@pytest.mark.parametrize("Nb,Ns", SHAPES)
def test_the_whole_loop_against_the_restatement(Nb, Ns):
    c = recipe(10 + Ns, Nb, Ns)
    o = go(c, max_iterations=10, rel_fitness=0.0, rel_rmse=0.0)
    assert o["iterations"].tolist() == [10, 10, 10] and o["converged"].tolist() == [0, 0, 0]
    for b in range(3):
        ref = gr.gicp_icp(c["src"][b], c["tgt"][b], c["nrm_s"][b], c["nrm_t"][b], c["R0"][b], c["t0"][b], rr.MAX_DIST, 10, 0.0, 0.0)
        assert ref["iterations"] == 10
        e_dev = pr.pose_error(o["R"][b], o["t"][b], c["R"][b], c["t"][b])
        e_ref = pr.pose_error(ref["R"], ref["t"], c["R"][b], c["t"][b])
        e_0 = pr.pose_error(c["R0"][b], c["t0"][b], c["R"][b], c["t"][b])
        _emit(f"gicp loop Nb {Nb} Ns {Ns} cloud {b}: start rot {e_0[0]:.3e} t {e_0[1]:.3e}  device rot {e_dev[0]:.3e} t {e_dev[1]:.3e} "
              f"inliers {o['inliers'][b]} rmse {o['rmse'][b]:.3e}  restated rot {e_ref[0]:.3e} t {e_ref[1]:.3e} inliers {ref['inliers']}")
        assert e_dev[0] <= 2 * e_ref[0] + 2.0 ** -20 and e_dev[1] <= 2 * e_ref[1] + 2.0 ** -20, (e_dev, e_ref)


def test_the_clouds_stop_on_their_own_and_do_not_depend_on_their_batch():
    """The default thresholds.  Cloud 1 starts ON the planted pose and stops rounds before the others: they run on behind its
    closed gate, and its outputs stay as its last evaluation wrote them."""
    Nb, Ns = SHAPES[1]
    c = recipe(41, Nb, Ns, undisturbed=(1,))
    whole = go(c)
    assert whole["converged"].tolist() == [1, 1, 1] and (whole["iterations"] >= 1).all() and (whole["iterations"] < 30).all()
    assert whole["iterations"][1] + 2 <= min(whole["iterations"][0], whole["iterations"][2]), whole["iterations"]
    for b in range(3):
        assert_same_bits(go(cloud(c, b)), {k: whole[k][b:b + 1] for k in EVAL + POSE}, b)
    assert_same_bits(go(c, prefill=0xFF), whole, "a NaN-prefilled workspace")


@pytest.mark.parametrize("Nb,Ns,forms", [SHAPES[0] + (((1, 1), (2, 3), (4, 128)),),
                                         SHAPES[1] + (tuple((q, s) for q in (1, 2, 4) for s in (1, 3, 128)),)])
def test_every_launch_form_returns_the_same_bits(Nb, Ns, forms):
    _, refine, _ = mods()
    c = recipe(10 + Ns, Nb, Ns)
    auto = go(c)
    assert auto["converged"].tolist() == [1, 1, 1]
    for q, s in forms:
        assert_same_bits(go(c, variant=refine.variant(q, s)), auto, (q, s))


def test_the_sign_of_a_normal_does_not_enter():
    Nb, Ns = SHAPES[0]
    c = recipe(10 + Ns, Nb, Ns)
    clean = go(c)
    rs = np.random.RandomState(4)
    half_s = rs.choice([-1.0, 1.0], c["nrm_s"].shape[::2]).astype(np.float32)[:, None, :]
    half_t = rs.choice([-1.0, 1.0], c["nrm_t"].shape[::2]).astype(np.float32)[:, None, :]
    assert (half_s < 0).any() and (half_s > 0).any() and (half_t < 0).any() and (half_t > 0).any()
    for what, fs, ft in (("every source normal", -1.0, 1.0), ("every target normal", 1.0, -1.0), ("a random half of each", half_s, half_t)):
        o = run(c["src"], c["tgt"], (c["nrm_s"] * fs).astype(np.float32), (c["nrm_t"] * ft).astype(np.float32), c["R0"], c["t0"])
        assert_same_bits(o, clean, what)


def test_the_stops():
    Nb, Ns = SHAPES[0]
    c = recipe(10 + Ns, Nb, Ns)
    # fewer than three pairs: a tiny max_dist from the disturbed start
    o = go(c, max_dist=1e-4)
    assert (o["inliers"] < 3).all() and o["iterations"].tolist() == [0, 0, 0] and o["converged"].tolist() == [0, 0, 0]
    assert np.array_equal(bits(o["R"]), bits(c["R0"])) and np.array_equal(bits(o["t"]), bits(c["t0"]))
    # two points against themselves
    two = np.ascontiguousarray(c["tgt"][:, :, :2])
    n2 = np.ascontiguousarray(c["nrm_t"][:, :, :2])
    o = run(two, two, n2, n2)
    assert o["inliers"].tolist() == [2, 2, 2] and o["iterations"].tolist() == [0, 0, 0] and o["converged"].tolist() == [0, 0, 0]
    assert np.array_equal(o["R"], np.broadcast_to(np.eye(3, dtype=np.float32), (3, 3, 3))) and not o["t"].any()
    # three collinear inliers: the system is singular
    k = gr.collinear()
    o = run(k["src"], k["tgt"], k["nrm_s"], k["nrm_t"])
    assert o["inliers"].tolist() == [3] and o["iterations"].tolist() == [0] and o["converged"].tolist() == [0]
    assert np.array_equal(o["R"][0], np.eye(3, dtype=np.float32)) and not o["t"].any()
    # (max_iterations = 0 evaluates only: test_one_update_against_the_restatement)


def test_nan_normals_give_a_nan_pose():
    """Non-finite sums: the update is NaN, the next evaluation finds no inlier and the cloud stops -- the other clouds are
    bit-identical to the clean batch.  A NaN in a source normal of an inlier; in the target normal an inlier pairs with."""
    Nb, Ns = SHAPES[0]
    c = recipe(10 + Ns, Nb, Ns)
    clean = go(c)
    zero = go(c, max_iterations=0)
    limit = np.float32(rr.MAX_DIST) * np.float32(rr.MAX_DIST)
    for which, b in (("nrm_s", 0), ("nrm_t", 2)):
        i = int(np.flatnonzero((zero["nn_idx"][b] >= 0) & (zero["nn_d2"][b] <= limit))[5])    # an inlier of the first round
        nrm = {k: c[k].copy() for k in ("nrm_s", "nrm_t")}
        nrm[which][b, 1, i if which == "nrm_s" else zero["nn_idx"][b][i]] = np.nan
        o = run(c["src"], c["tgt"], nrm["nrm_s"], nrm["nrm_t"], c["R0"], c["t0"])
        assert np.isnan(o["R"][b]).all() and np.isnan(o["t"][b]).all() and o["iterations"][b] == 1 and o["inliers"][b] == 0
        rest = [x for x in range(3) if x != b]
        assert_same_bits({k: o[k][rest] for k in EVAL + POSE}, {k: clean[k][rest] for k in EVAL + POSE}, (which, "the other clouds"))
    # a NaN normal nothing pairs with changes nothing: a FAR source point's
    nrm_s = c["nrm_s"].copy()
    nrm_s[:, :, Ns:] = np.nan
    assert_same_bits(run(c["src"], c["tgt"], nrm_s, c["nrm_t"], c["R0"], c["t0"]), clean, "NaN normals of the FAR points")


def _with_far(c, extra, seed=5):
    rs = np.random.RandomState(seed)
    far = rs.uniform(2.0, 3.0, (3, 3, extra)).astype(np.float32)
    junk = rs.normal(size=(3, 3, extra)).astype(np.float32)     # (not unit, not read)
    return dict(c, src=np.concatenate([c["src"], far], axis=2), nrm_s=np.concatenate([c["nrm_s"], junk], axis=2))


def test_lanes_that_are_no_inliers_are_masked():
    """200 more FAR source points behind a recipe change neither A nor g, seen through the pose after one update: within the
    one-update bound wherever they land, and not by one bit where they come as whole trailing workgroups (a source of 256
    points, 256 more)."""
    kw = dict(max_iterations=1, rel_fitness=0.0, rel_rmse=0.0)
    Nb, Ns = SHAPES[0]
    c = recipe(10 + Ns, Nb, Ns)
    a, b = go(c, **kw), go(_with_far(c, 200), **kw)
    assert np.array_equal(a["inliers"], b["inliers"]) and np.array_equal(bits(a["sum_d2"]), bits(b["sum_d2"]))
    zero = go(c, max_iterations=0)
    for i in range(3):
        up = gr.gicp_step(c["src"][i], c["tgt"][i], c["nrm_s"][i], c["nrm_t"][i], c["R0"][i], c["t0"][i], zero["nn_idx"][i],
                          zero["nn_d2"][i], rr.MAX_DIST)
        bound = 2.0 ** -22 + 64 * up["cond"] * 2.0 ** -53
        dR, dt = np.abs(a["R"][i] - b["R"][i]).max(), np.abs(a["t"][i] - b["t"][i]).max()
        _emit(f"gicp mask Ns {Ns}+{FAR} +200 FAR cloud {i}: |dR| {dR:.2e} |dt| {dt:.2e} bound {bound:.2e}")
        assert dR <= bound and dt <= bound, (dR, dt, bound)
    c = recipe(77, 700, 256 - FAR)
    assert c["src"].shape[2] == 256
    assert_same_bits(go(c, **kw), go(_with_far(c, 256), **kw), "whole trailing workgroups", POSE + ("inliers", "sum_d2"))


def _same(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(a.view(torch.int32) if a.dtype == torch.float32 else a,
                                                                      b.view(torch.int32) if b.dtype == torch.float32 else b)


PUBLIC = (("R", "R"), ("t", "t"), ("R_ba", "R_ba"), ("t_ba", "t_ba"), ("fitness", "fitness"), ("inlier_rmse", "rmse"),
          ("inliers", "inliers"), ("iterations", "iterations"), ("converged", "converged"))


def test_the_python_api_and_its_unchanged_defaults():
    import vcrnet_amd
    from vcrnet_amd import plane
    gicp, refine, _ = mods()
    Nb, Ns = SHAPES[0]
    c = recipe(10 + Ns, Nb, Ns)
    s, q, R0, t0 = dev(c["src"]), dev(c["tgt"]), dev(c["R0"]), dev(c["t0"])
    ns, nt = dev(c["nrm_s"]), dev(c["nrm_t"])
    # given normals: gicp.refine_gicp
    low = gicp.refine_gicp(s, q, ns, nt, R0, t0, rr.MAX_DIST)
    res = vcrnet_amd.refine_registration(s, q, R0, t0, max_dist=rr.MAX_DIST, method="generalized", src_normals=ns, tgt_normals=nt)
    assert sorted(res) == sorted(a for a, _ in PUBLIC) and all(_same(res[a], low[b]) for a, b in PUBLIC)
    eps = vcrnet_amd.refine_registration(s, q, R0, t0, max_dist=rr.MAX_DIST, method="generalized", src_normals=ns, tgt_normals=nt,
                                         epsilon=1e-2)
    assert all(_same(eps[a], gicp.refine_gicp(s, q, ns, nt, R0, t0, rr.MAX_DIST, epsilon=1e-2)[b]) for a, b in PUBLIC)
    assert not _same(eps["R"], res["R"])                      # (epsilon is read)
    # None: estimate_normals(cloud, normal_k) of each cloud, 20 by default
    es, et = vcrnet_amd.estimate_normals(s, 20), vcrnet_amd.estimate_normals(q, 20)
    given = vcrnet_amd.refine_registration(s, q, R0, t0, max_dist=rr.MAX_DIST, method="generalized", src_normals=es, tgt_normals=et,
                                           want_nn=True)
    for kw in (dict(), dict(src_normals=es), dict(tgt_normals=et), dict(normal_k=20)):
        inside = vcrnet_amd.refine_registration(s, q, R0, t0, max_dist=rr.MAX_DIST, method="generalized", want_nn=True, **kw)
        assert sorted(inside) == sorted(given) and inside["nn_idx"].dtype == torch.int64
        assert all(_same(inside[k], given[k]) for k in given), kw
    closing = vcrnet_amd.score_registration(s, q, given["R"], given["t"], max_dist=rr.MAX_DIST, want_nn=True)
    for key in ("fitness", "inlier_rmse", "inliers", "nn_idx", "nn_d2"):             # the closing invariant, through the public API
        assert torch.equal(given[key], closing[key]), key
    # the other methods with the new keywords at their defaults: the calls below them, as before
    point = refine.refine(s, q, R0, t0, rr.MAX_DIST)
    for r in (vcrnet_amd.refine_registration(s, q, R0, t0, max_dist=rr.MAX_DIST),
              vcrnet_amd.refine_registration(s, q, R0, t0, max_dist=rr.MAX_DIST, method="point_to_point", src_normals=None, epsilon=1e-3)):
        assert all(_same(r[a], point[b]) for a, b in PUBLIC)
    lowp = plane.refine_plane(s, q, nt, R0, t0, rr.MAX_DIST)
    pl = vcrnet_amd.refine_registration(s, q, R0, t0, max_dist=rr.MAX_DIST, method="point_to_plane", tgt_normals=nt)
    assert all(_same(pl[a], lowp[b]) for a, b in PUBLIC)
    assert not _same(pl["R"], res["R"]) and not _same(point["R"], low["R"])          # (three fits)
    from vcrnet_amd.native import VcrHipError
    with pytest.raises(VcrHipError, match=r"src_normals must be \[B, 3, Ns\]"):
        vcrnet_amd.refine_registration(s, q, max_dist=0.1, method="generalized", src_normals=q)
    with pytest.raises(VcrHipError, match="device of the clouds"):
        vcrnet_amd.refine_registration(s, q, max_dist=0.1, method="generalized", src_normals=s.cpu())
    with pytest.raises(VcrHipError, match="method='generalized' only"):
        vcrnet_amd.refine_registration(s, q, max_dist=0.1, method="point_to_plane", src_normals=ns)
    with pytest.raises(VcrHipError, match="unsupported"):
        gicp.refine_gicp(s, q, ns, nt, max_dist=0.1, max_iterations=refine.MAX_ITERATIONS + 1)


def test_register_sampled_passes_the_method_on():
    """refine_method="generalized" returns refine_registration(method="generalized") on the network's pose: on the equal-size
    route for the batch, on the voxel route cloud by cloud."""
    import vcrnet_amd
    from test_hip_forward import build_net
    from test_hip_fps import _pair
    net, _ = build_net()
    src, tgt = _pair(3000, 4100)
    s, t = dev(src), dev(tgt)
    with torch.no_grad():
        plain = vcrnet_amd.register_sampled(net, s, t, 1024)
        gen = vcrnet_amd.register_sampled(net, s, t, 1024, refine=0.1, refine_method="generalized")
        assert len(plain) == 8 and len(gen) == 9 and all(_same(a, b) for a, b in zip(plain, gen[:8]))
        direct = vcrnet_amd.refine_registration(s, t, plain[2], plain[3], max_dist=0.1, method="generalized")
        assert sorted(gen[8]) == sorted(direct) == sorted(a for a, _ in PUBLIC) and all(_same(gen[8][k], direct[k]) for k in direct)
        point = vcrnet_amd.register_sampled(net, s, t, 1024, refine=0.1)
        assert not _same(point[8]["R"], gen[8]["R"])
        h = float(np.ptp(src, axis=2).max()) / 16.0
        vox = vcrnet_amd.register_sampled(net, s, t, 768, voxel=h, refine=0.1, refine_method="generalized")
        assert len(vox) == 10 and isinstance(vox[8], list) and len(vox[8]) == src.shape[0]
        for b in range(src.shape[0]):
            sb, tb = vox[9][0][b].unsqueeze(0), vox[9][1][b].unsqueeze(0)
            direct = vcrnet_amd.refine_registration(sb, tb, vox[2][b:b + 1], vox[3][b:b + 1], max_dist=0.1, method="generalized")
            assert sorted(vox[8][b]) == sorted(direct) and all(_same(vox[8][b][k], direct[k]) for k in direct), b
