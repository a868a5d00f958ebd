"""vcr_refine_plane_f32 on the GPU: the point-to-plane refinement on the full clouds (include/vcr_hip_plane.h, DESIGN.md
section 4.10).

The input is tests/refine_restated.py's recipe on the torus at its first two shapes, B = 3; the target's normals are
estimate_normals' (k = 20).  What is checked:
  * one update from the given start against plane_restated.plane_step on the device's own iteration-0 neighbours (the scan is
    bit-defined): |dR|, |dt| <= 2^-22 + 64 cond(A) 2^-53, cond(A) < 1e6;
  * the whole loop, ten updates, against plane_restated.plane_icp and the planted pose: the device's rotation and translation
    errors are at most twice the restatement's plus 2^-20 (the margin: neighbour sets may part after the first round);
  * the stops; a cloud alone against the cloud in a batch; every launch form: the same bits;
  * in EVERY run the closing invariant -- each returned evaluation output is bit-equal to nn_score(src, tgt, R_out, t_out) --
    every output element written and no guard band touched;
  * the defaults of refine_registration and register_sampled: what they returned before."""
import os

import numpy as np
import pytest
import torch

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
        path = os.path.join(out, "plane_ledger.txt")
        if len(LEDGER) == 1:                                 # a new table: which kernel sources it measures
            import vcrnet_amd  # noqa: F401
            from vcrnet_amd import build as vb
            with open(path, "w") as f:
                f.write(f"# kernel_sources_sha16={vb.sources_sha16()}\n")
        with open(path, "a") as f:
            f.write(line + "\n")


def mods():
    import vcrnet_amd  # noqa: F401
    from vcrnet_amd import plane, refine, score
    return plane, refine, score


def dev(x):
    return None if x is None else torch.tensor(np.ascontiguousarray(x)).cuda()         # (a copy: the recipes are read-only)


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view({4: np.int32, 8: np.int64}[a.dtype.itemsize])


def assert_same_bits(a, b, what, keys=EVAL + POSE):
    for k in keys:
        assert np.array_equal(bits(a[k]), bits(b[k])), (what, k)


def run(src, tgt, nrm, R=None, t=None, max_dist=rr.MAX_DIST, prefill=SENTINEL_BYTE, **kw):
    """numpy in, dict of numpy out; test_hip_refine.run's checks: every output overwritten, no guard band touched, the closing
    invariant, the inverse pose."""
    plane, _, score = mods()
    o = plane.refine_plane(dev(src), dev(tgt), dev(nrm), dev(R), dev(t), max_dist, guard=GUARD, prefill=prefill, **kw)
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


_RECIPES = {}


def recipe(seed, Nb, Ns, undisturbed=()):
    """refine_restated.batch on the torus, plus "nrm": estimate_normals of the target (computed once, read-only)."""
    import vcrnet_amd
    key = (seed, Nb, Ns, tuple(undisturbed))
    if key not in _RECIPES:
        c = rr.batch(seed, Nb, Ns, "torus", undisturbed)
        c["nrm"] = vcrnet_amd.estimate_normals(dev(c["tgt"]), 20).cpu().numpy()
        for v in c.values():
            v.setflags(write=False)
        _RECIPES[key] = c
    return _RECIPES[key]


@pytest.mark.parametrize("Nb,Ns", SHAPES)
def test_one_update_against_the_restatement(Nb, Ns):
    _, _, score = mods()
    c = recipe(20 + Ns, Nb, Ns)
    zero = run(c["src"], c["tgt"], c["nrm"], c["R0"], c["t0"], max_iterations=0)
    s = score.nn_score(dev(c["src"]), dev(c["tgt"]), dev(c["R0"]), dev(c["t0"]), rr.MAX_DIST)
    assert_same_bits(zero, {k: s[k].cpu().numpy() for k in EVAL}, "max_iterations = 0: the score of the start", EVAL)
    assert zero["iterations"].tolist() == [0, 0, 0] and zero["converged"].tolist() == [0, 0, 0]
    assert np.array_equal(bits(zero["R"]), bits(c["R0"])) and np.array_equal(bits(zero["t"]), bits(c["t0"]))
    one = run(c["src"], c["tgt"], c["nrm"], c["R0"], c["t0"], max_iterations=1, rel_fitness=0.0, rel_rmse=0.0)
    assert one["iterations"].tolist() == [1, 1, 1] and one["converged"].tolist() == [0, 0, 0]
    for b in range(3):
        up = pr.plane_step(c["src"][b], c["tgt"][b], c["nrm"][b], c["R0"][b], c["t0"][b], zero["nn_idx"][b], zero["nn_d2"][b], rr.MAX_DIST)
        assert up["n"] == zero["inliers"][b] and 6 <= up["n"] < Ns + FAR
        R0, t0 = c["R0"][b].astype(np.float64), c["t0"][b].astype(np.float64)
        dR = np.abs(one["R"][b] - up["R"] @ R0).max()
        dt = np.abs(one["t"][b] - (up["R"] @ t0 + up["t"])).max()
        bound = 2.0 ** -22 + 64 * up["cond"] * 2.0 ** -53
        _emit(f"plane step Nb {Nb} Ns {Ns} cloud {b}: n {up['n']} cond(A) {up['cond']:.3e} |dR| {dR:.2e} |dt| {dt:.2e} bound {bound:.2e}")
        assert up["cond"] < 1e6
        assert dR <= bound and dt <= bound, (dR, dt, bound)
        assert 0 < np.abs(one["R"][b] - c["R0"][b]).max()        # (a step was taken)


@pytest.mark.parametrize("Nb,Ns", SHAPES)
def test_the_whole_loop_against_the_restatement(Nb, Ns):
    c = recipe(10 + Ns, Nb, Ns)
    o = run(c["src"], c["tgt"], c["nrm"], c["R0"], c["t0"], max_iterations=10, rel_fitness=0.0, rel_rmse=0.0)
    assert o["iterations"].tolist() == [10, 10, 10] and o["converged"].tolist() == [0, 0, 0]
    for b in range(3):
        ref = pr.plane_icp(c["src"][b], c["tgt"][b], c["nrm"][b], c["R0"][b], c["t0"][b], rr.MAX_DIST, 10, 0.0, 0.0)
        assert ref["iterations"] == 10
        e_dev = pr.pose_error(o["R"][b], o["t"][b], c["R"][b], c["t"][b])
        e_ref = pr.pose_error(ref["R"], ref["t"], c["R"][b], c["t"][b])
        e_0 = pr.pose_error(c["R0"][b], c["t0"][b], c["R"][b], c["t"][b])
        _emit(f"plane loop Nb {Nb} Ns {Ns} cloud {b}: start rot {e_0[0]:.3e} t {e_0[1]:.3e}  device rot {e_dev[0]:.3e} t {e_dev[1]:.3e} "
              f"inliers {o['inliers'][b]} rmse {o['rmse'][b]:.3e}  restated rot {e_ref[0]:.3e} t {e_ref[1]:.3e} inliers {ref['inliers']}")
        assert e_dev[0] <= 2 * e_ref[0] + 2.0 ** -20 and e_dev[1] <= 2 * e_ref[1] + 2.0 ** -20, (e_dev, e_ref)


def test_the_clouds_stop_on_their_own_and_do_not_depend_on_their_batch():
    """The default thresholds.  Cloud 1 starts ON the planted pose and stops rounds before the others: they run on behind its
    closed gate, and its outputs stay as its last evaluation wrote them."""
    Nb, Ns = SHAPES[1]
    c = recipe(41, Nb, Ns, undisturbed=(1,))
    whole = run(c["src"], c["tgt"], c["nrm"], c["R0"], c["t0"])
    assert whole["converged"].tolist() == [1, 1, 1] and (whole["iterations"] >= 1).all() and (whole["iterations"] < 30).all()
    assert whole["iterations"][1] + 2 <= min(whole["iterations"][0], whole["iterations"][2]), whole["iterations"]
    for b in range(3):
        alone = run(c["src"][b:b + 1], c["tgt"][b:b + 1], c["nrm"][b:b + 1], c["R0"][b:b + 1], c["t0"][b:b + 1])
        assert_same_bits(alone, {k: whole[k][b:b + 1] for k in EVAL + POSE}, b)
    assert_same_bits(run(c["src"], c["tgt"], c["nrm"], c["R0"], c["t0"], prefill=0xFF), whole, "a NaN-prefilled workspace")


@pytest.mark.parametrize("Nb,Ns,forms", [SHAPES[0] + (((1, 1), (2, 3), (4, 128)),),
                                         SHAPES[1] + (tuple((q, s) for q in (1, 2, 4) for s in (1, 3, 128)),)])
def test_every_launch_form_returns_the_same_bits(Nb, Ns, forms):
    _, refine, _ = mods()
    c = recipe(10 + Ns, Nb, Ns)
    auto = run(c["src"], c["tgt"], c["nrm"], c["R0"], c["t0"])
    assert auto["converged"].tolist() == [1, 1, 1]
    for q, s in forms:
        assert_same_bits(run(c["src"], c["tgt"], c["nrm"], c["R0"], c["t0"], variant=refine.variant(q, s)), auto, (q, s))


def test_a_flat_target_and_too_few_inliers_leave_the_pose():
    Nb, Ns = SHAPES[0]
    c = recipe(10 + Ns, Nb, Ns)
    # a planar target with equal normals: three of the six unknowns are free
    rs = np.random.RandomState(3)
    flat = np.concatenate([rs.uniform(0, 1, (3, 2, 400)), np.full((3, 1, 400), 0.25)], axis=1).astype(np.float32)
    up_n = np.zeros((3, 3, 400), np.float32)
    up_n[:, 2] = 1
    src = np.ascontiguousarray(flat[:, :, :200])
    R0 = np.stack([rr.rotation([1, 2, 3], 0.5).astype(np.float32)] * 3)
    t0 = np.full((3, 3), 0.002, np.float32)
    o = run(src, flat, up_n, R0, t0)
    assert (o["inliers"] >= 190).all() and o["iterations"].tolist() == [0, 0, 0] and o["converged"].tolist() == [0, 0, 0]
    assert np.array_equal(bits(o["R"]), bits(R0)) and np.array_equal(bits(o["t"]), bits(t0))
    # fewer than six inliers: a tiny max_dist from the disturbed start, and five points against themselves
    o = run(c["src"], c["tgt"], c["nrm"], c["R0"], c["t0"], max_dist=1e-4)
    assert (o["inliers"] < 6).all() and o["iterations"].tolist() == [0, 0, 0] and o["converged"].tolist() == [0, 0, 0]
    assert np.array_equal(bits(o["R"]), bits(c["R0"])) and np.array_equal(bits(o["t"]), bits(c["t0"]))
    five = np.ascontiguousarray(c["tgt"][:, :, :5])
    o = run(five, five, np.ascontiguousarray(c["nrm"][:, :, :5]))
    assert o["inliers"].tolist() == [5, 5, 5] and o["iterations"].tolist() == [0, 0, 0] and o["converged"].tolist() == [0, 0, 0]
    assert np.array_equal(o["R"], np.broadcast_to(np.eye(3, dtype=np.float32), (3, 3, 3))) and not o["t"].any()


def test_nan_normals_give_a_nan_pose():
    """Non-finite sums: the update is NaN, the next evaluation finds no inlier and the cloud stops -- clouds 1 and 2 are
    bit-identical to the clean batch."""
    Nb, Ns = SHAPES[0]
    c = recipe(10 + Ns, Nb, Ns)
    clean = run(c["src"], c["tgt"], c["nrm"], c["R0"], c["t0"])
    nrm = c["nrm"].copy()
    nrm[0] = np.nan
    o = run(c["src"], c["tgt"], nrm, c["R0"], c["t0"])
    assert np.isnan(o["R"][0]).all() and np.isnan(o["t"][0]).all() and o["iterations"][0] == 1 and o["inliers"][0] == 0
    assert_same_bits({k: o[k][1:] for k in EVAL + POSE}, {k: clean[k][1:] for k in EVAL + POSE}, "the other clouds")


def test_the_python_api_and_its_unchanged_defaults():
    import vcrnet_amd
    plane, refine, _ = mods()
    Nb, Ns = SHAPES[0]
    c = recipe(10 + Ns, Nb, Ns)
    s, q, R0, t0 = dev(c["src"]), dev(c["tgt"]), dev(c["R0"]), dev(c["t0"])
    # point to point: the default, named or not, is refine.refine
    low = refine.refine(s, q, R0, t0, rr.MAX_DIST)
    for res in (vcrnet_amd.refine_registration(s, q, R0, t0, max_dist=rr.MAX_DIST),
                vcrnet_amd.refine_registration(s, q, R0, t0, max_dist=rr.MAX_DIST, method="point_to_point")):
        assert sorted(res) == ["R", "R_ba", "converged", "fitness", "inlier_rmse", "inliers", "iterations", "t", "t_ba"]
        for a, b in (("R", "R"), ("t", "t"), ("R_ba", "R_ba"), ("t_ba", "t_ba"), ("fitness", "fitness"), ("inlier_rmse", "rmse"),
                     ("inliers", "inliers"), ("iterations", "iterations"), ("converged", "converged")):
            assert res[a].dtype == low[b].dtype and torch.equal(res[a].view(torch.int32), low[b].view(torch.int32)), a
    # point to plane: the normals estimated inside are estimate_normals(tgt, normal_k)
    for k in (20, 12):
        inside = vcrnet_amd.refine_registration(s, q, R0, t0, max_dist=rr.MAX_DIST, method="point_to_plane", normal_k=k, want_nn=True)
        given = vcrnet_amd.refine_registration(s, q, R0, t0, max_dist=rr.MAX_DIST, method="point_to_plane",
                                               tgt_normals=vcrnet_amd.estimate_normals(q, k), want_nn=True)
        assert sorted(inside) == sorted(list(res) + ["nn_idx", "nn_d2"]) and inside["nn_idx"].dtype == torch.int64
        for key in inside:
            a, b = inside[key], given[key]
            assert torch.equal(a.view(torch.int32) if a.dtype == torch.float32 else a, b.view(torch.int32) if b.dtype == torch.float32 else b), key
        closing = vcrnet_amd.score_registration(s, q, inside["R"], inside["t"], max_dist=rr.MAX_DIST, want_nn=True)
        for key in ("fitness", "inlier_rmse", "inliers", "nn_idx", "nn_d2"):         # the closing invariant, through the public API
            assert torch.equal(inside[key], closing[key]), key
    lowp = plane.refine_plane(s, q, dev(c["nrm"]), R0, t0, rr.MAX_DIST)
    pl = vcrnet_amd.refine_registration(s, q, R0, t0, max_dist=rr.MAX_DIST, method="point_to_plane", tgt_normals=dev(c["nrm"]))
    assert torch.equal(pl["R"].view(torch.int32), lowp["R"].view(torch.int32)) and torch.equal(pl["iterations"], lowp["iterations"])
    assert not torch.equal(pl["R"].view(torch.int32), low["R"].view(torch.int32))    # (another fit)
    from vcrnet_amd.native import VcrHipError
    with pytest.raises(VcrHipError, match="method must be one of"):
        vcrnet_amd.refine_registration(s, q, max_dist=0.1, method="plane")
    with pytest.raises(VcrHipError, match=r"tgt_normals must be \[B, 3, Nt\]"):
        vcrnet_amd.refine_registration(s, q, max_dist=0.1, method="point_to_plane", tgt_normals=s)
    with pytest.raises(VcrHipError, match="device of the clouds"):
        vcrnet_amd.refine_registration(s, q, max_dist=0.1, method="point_to_plane", tgt_normals=q.cpu())
    with pytest.raises(VcrHipError, match="unsupported"):
        plane.refine_plane(s, q, dev(c["nrm"]), max_dist=0.1, max_iterations=refine.MAX_ITERATIONS + 1)


def test_register_sampled_passes_the_method_on():
    """refine=d alone returns what it returned before -- refine_registration's default on the network's pose -- and
    refine_method="point_to_plane" that call with the method."""
    import vcrnet_amd
    from test_hip_forward import build_net
    from test_hip_fps import _pair
    net, _ = build_net()
    src, tgt = _pair(3000, 4100)
    s, t = dev(src), dev(tgt)
    same = lambda a, b: a.shape == b.shape and torch.equal(a.view(torch.int32) if a.dtype == torch.float32 else a,   # noqa: E731
                                                           b.view(torch.int32) if b.dtype == torch.float32 else b)
    with torch.no_grad():
        plain = vcrnet_amd.register_sampled(net, s, t, 1024)
        point = vcrnet_amd.register_sampled(net, s, t, 1024, refine=0.1)
        planes = vcrnet_amd.register_sampled(net, s, t, 1024, refine=0.1, refine_method="point_to_plane")
    assert len(plain) == 8 and len(point) == 9 and len(planes) == 9
    for other in (point, planes):
        assert all(same(a, b) for a, b in zip(plain, other[:8]))
    from vcrnet_amd import refine
    before = refine.refine(s, t, plain[2], plain[3], 0.1, want_nn=False)   # the call of the parent's path
    for a, b in (("R", "R"), ("t", "t"), ("R_ba", "R_ba"), ("t_ba", "t_ba"), ("fitness", "fitness"), ("inlier_rmse", "rmse"),
                 ("inliers", "inliers"), ("iterations", "iterations"), ("converged", "converged")):
        assert same(point[8][a], before[b]), a
    assert sorted(point[8]) == sorted(planes[8]) == ["R", "R_ba", "converged", "fitness", "inlier_rmse", "inliers", "iterations", "t", "t_ba"]
    direct = vcrnet_amd.refine_registration(s, t, plain[2], plain[3], max_dist=0.1, method="point_to_plane")
    assert all(same(planes[8][k], direct[k]) for k in direct)
