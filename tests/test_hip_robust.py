"""vcr_refine_robust_f32 and vcr_information_f32 on the GPU: the point-to-plane refinement with a robust weight per pair, and
the information matrix of a registered pair (include/robust/vcr_hip_robust.h).

The clean input is test_hip_plane.py's: tests/refine_restated.py's recipe on the torus at its first two shapes, B = 3 (337 and
1137 source points: partials span workgroups and the last block is ragged), the target's normals estimate_normals' (k = 20).
The contaminated input is robust_restated.contaminated with the TRUE normals.  What is checked:
  * L2, and Huber with a k no residual reaches, return vcr_refine_plane_f32's outputs bit for bit;
  * one update per loss against robust_restated.robust_step on the device's own iteration-0 neighbours:
    |dR|, |dt| <= 2^-22 + 64 cond(A) 2^-53, cond(A) < 1e6;
  * ten updates per loss against robust_restated.robust_icp and the planted pose: the device's rotation and translation errors
    are at most twice the restatement's plus 2^-20 (test_hip_plane.py's rule);
  * on the contaminated pair, Cauchy and the two-stage Tukey by that rule against the restatement, and strictly better than the
    device's own least squares (tests/test_robust_cpu.py holds the ratio, on the restatement);
  * every launch form, the grid, a cloud alone: the same bits; the stops;
  * the information matrix bit for bit against robust_restated.information on the device's own neighbours;
  * in EVERY run the closing invariant -- each returned evaluation output is bit-equal to nn_score(src, tgt, R_out, t_out) --
    every output element written and no guard band touched.
The scales k of the clean-input tests: wide enough that the loop stays in the basin the restatement stays in (these tests are
about the arithmetic, not about robustness) and narrow enough that the weights differ across the inliers, whose residuals reach
max_dist = 0.1 at the start: Huber and Cauchy 0.02, GM 0.01 (a squared length: 0.1^2), Tukey 0.1."""
import os

import numpy as np
import pytest
import torch

import plane_restated as pr
import refine_restated as rr
import robust_restated as ro

pytestmark = pytest.mark.gpu

SENTINEL_BYTE = 0x5A
GUARD = 64
EVAL = ("nn_idx", "nn_d2", "inliers", "sum_d2", "fitness", "rmse")
POSE = ("R", "t", "R_ba", "t_ba", "iterations", "converged")
FAR = rr.FAR
SHAPES = rr.SHAPES[:2]
SCALE = {"l2": 1.0, "huber": 0.02, "cauchy": 0.02, "gm": 0.01, "tukey": 0.1}
LEDGER = []


def _emit(line):
    print(line)
    LEDGER.append(line)
    out = os.environ.get("VCR_LEDGER_DIR", "")
    if os.path.isdir(out):
        path = os.path.join(out, "robust_ledger.txt")
        if len(LEDGER) == 1:                                 # a new table: which kernel sources it measures
            import vcrnet_amd  # noqa: F401
            from vcrnet_amd import build as vb
            with open(path, "w") as f:
                f.write(f"# kernel_sources_sha16={vb.sources_sha16()}\n")
        with open(path, "a") as f:
            f.write(line + "\n")


def mods():
    import vcrnet_amd  # noqa: F401
    from vcrnet_amd import plane, refine, robust, score
    return plane, refine, robust, score


def dev(x):
    return None if x is None else torch.tensor(np.ascontiguousarray(x)).cuda()         # (a copy: the recipes are read-only)


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view({4: np.int32, 8: np.int64}[a.dtype.itemsize])


def assert_same_bits(a, b, what, keys=EVAL + POSE):
    for k in keys:
        assert np.array_equal(bits(a[k]), bits(b[k])), (what, k)


def _checked(o, keys, src, tgt, max_dist, prefill, search):
    """test_hip_plane.run's checks on a call's raw buffers: every output overwritten, no guard band touched, the closing
    invariant (by the same search: the grid reports -1 / +inf where the scan reports the far neighbour), the inverse pose."""
    _, _, _, score = mods()
    torch.cuda.synchronize()
    out = {k: o[k].cpu().numpy() for k in keys}
    for k in keys:
        raw = o["_raw"][k]
        n = o[k].numel()
        band = raw[n:].view(torch.uint8).cpu().numpy()
        assert band.size == GUARD * raw.element_size() and (band == prefill).all(), (k, "guard band written")
        body = raw[:n].view(torch.uint8).cpu().numpy().reshape(n, -1)
        assert not (body == prefill).all(axis=1).any(), (k, "element left unwritten")
    s = score.nn_score(dev(src), dev(tgt), o["R"], o["t"], max_dist, search=search)
    assert_same_bits(out, {k: s[k].cpu().numpy() for k in EVAL}, "closing invariant", EVAL)
    assert (out["nn_idx"] >= -1).all() and (out["nn_idx"] < tgt.shape[2]).all()
    assert np.array_equal(bits(out["R_ba"]), bits(out["R"].transpose(0, 2, 1)))
    return out


def run(src, tgt, nrm, R=None, t=None, loss="tukey", k=None, max_dist=rr.MAX_DIST, prefill=SENTINEL_BYTE, search="scan", **kw):
    """numpy in, dict of numpy out, through robust.refine_robust."""
    _, _, robust, _ = mods()
    o = robust.refine_robust(dev(src), dev(tgt), dev(nrm), dev(R), dev(t), max_dist, loss, SCALE[loss] if k is None else k,
                             guard=GUARD, prefill=prefill, search=search, **kw)
    return _checked(o, EVAL + POSE, src, tgt, max_dist, prefill, search)


def run_plane(src, tgt, nrm, R, t, max_dist=rr.MAX_DIST, **kw):
    plane, _, _, _ = mods()
    o = plane.refine_plane(dev(src), dev(tgt), dev(nrm), dev(R), dev(t), max_dist, **kw)
    torch.cuda.synchronize()
    return {k: o[k].cpu().numpy() for k in EVAL + POSE}


def run_info(src, tgt, R=None, t=None, max_dist=rr.MAX_DIST, prefill=SENTINEL_BYTE, search="scan", **kw):
    """numpy in, dict of numpy out, through robust.information: run's checks, the matrix among the outputs; the pose given
    comes back, and no update is counted."""
    _, _, robust, _ = mods()
    o = robust.information(dev(src), dev(tgt), dev(R), dev(t), max_dist, guard=GUARD, prefill=prefill, search=search, **kw)
    out = _checked(o, EVAL + POSE + ("information",), src, tgt, max_dist, prefill, search)
    B = src.shape[0]
    R = np.broadcast_to(np.eye(3, dtype=np.float32), (B, 3, 3)) if R is None else R
    t = np.zeros((B, 3), np.float32) if t is None else t
    assert np.array_equal(bits(out["R"]), bits(R)) and np.array_equal(bits(out["t"]), bits(t))
    assert not out["iterations"].any() and not out["converged"].any()
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
def test_l2_and_a_wide_huber_are_the_plane_fit_bit_for_bit(Nb, Ns):
    c = recipe(10 + Ns, Nb, Ns)
    a = (c["src"], c["tgt"], c["nrm"], c["R0"], c["t0"])
    for kw in (dict(), dict(max_iterations=3, rel_fitness=0.0, rel_rmse=0.0)):
        ref = run_plane(*a, **kw)
        assert (ref["iterations"] >= 1).all()
        assert_same_bits(run(*a, loss="l2", **kw), ref, ("l2", kw))
        assert_same_bits(run(*a, loss="l2", k=1e-30, **kw), ref, ("l2 does not read k", kw))
        assert_same_bits(run(*a, loss="huber", k=1e30, **kw), ref, ("huber 1e30", kw))
        assert not np.array_equal(bits(run(*a, loss="huber", k=0.005, **kw)["R"]), bits(ref["R"]))       # (a weight that bites)


@pytest.mark.parametrize("loss", ro.LOSSES)
@pytest.mark.parametrize("Nb,Ns", SHAPES)
def test_one_update_against_the_restatement(Nb, Ns, loss):
    c = recipe(20 + Ns, Nb, Ns)
    a = (c["src"], c["tgt"], c["nrm"], c["R0"], c["t0"])
    zero = run(*a, loss=loss, max_iterations=0)
    assert zero["iterations"].tolist() == [0, 0, 0] and zero["converged"].tolist() == [0, 0, 0]
    assert np.array_equal(bits(zero["R"]), bits(c["R0"])) and np.array_equal(bits(zero["t"]), bits(c["t0"]))
    one = run(*a, loss=loss, max_iterations=1, rel_fitness=0.0, rel_rmse=0.0)
    assert one["iterations"].tolist() == [1, 1, 1] and one["converged"].tolist() == [0, 0, 0]
    for b in range(3):
        up = ro.robust_step(c["src"][b], c["tgt"][b], c["nrm"][b], c["R0"][b], c["t0"][b], zero["nn_idx"][b], zero["nn_d2"][b],
                            rr.MAX_DIST, loss, SCALE[loss])
        assert up["n"] == zero["inliers"][b] and 6 <= up["n"] < Ns + FAR
        R0, t0 = c["R0"][b].astype(np.float64), c["t0"][b].astype(np.float64)
        dR = np.abs(one["R"][b] - up["R"] @ R0).max()
        dt = np.abs(one["t"][b] - (up["R"] @ t0 + up["t"])).max()
        bound = 2.0 ** -22 + 64 * up["cond"] * 2.0 ** -53
        _emit(f"robust step {loss} k {SCALE[loss]} Nb {Nb} Ns {Ns} cloud {b}: n {up['n']} cond(A) {up['cond']:.3e} |dR| {dR:.2e} |dt| {dt:.2e} "
              f"bound {bound:.2e}")
        assert up["cond"] < 1e6
        assert dR <= bound and dt <= bound, (dR, dt, bound)
        assert 0 < np.abs(one["R"][b] - c["R0"][b]).max()        # (a step was taken)


@pytest.mark.parametrize("loss", ro.LOSSES)
@pytest.mark.parametrize("Nb,Ns", SHAPES)
def test_the_whole_loop_against_the_restatement(Nb, Ns, loss):
    c = recipe(10 + Ns, Nb, Ns)
    o = run(c["src"], c["tgt"], c["nrm"], c["R0"], c["t0"], loss=loss, max_iterations=10, rel_fitness=0.0, rel_rmse=0.0)
    assert o["iterations"].tolist() == [10, 10, 10] and o["converged"].tolist() == [0, 0, 0]
    for b in range(3):
        ref = ro.robust_icp(c["src"][b], c["tgt"][b], c["nrm"][b], c["R0"][b], c["t0"][b], rr.MAX_DIST, loss, SCALE[loss], 10, 0.0, 0.0)
        assert ref["iterations"] == 10
        e_dev = pr.pose_error(o["R"][b], o["t"][b], c["R"][b], c["t"][b])
        e_ref = pr.pose_error(ref["R"], ref["t"], c["R"][b], c["t"][b])
        e_0 = pr.pose_error(c["R0"][b], c["t0"][b], c["R"][b], c["t"][b])
        _emit(f"robust loop {loss} k {SCALE[loss]} Nb {Nb} Ns {Ns} cloud {b}: start rot {e_0[0]:.3e} t {e_0[1]:.3e}  device rot {e_dev[0]:.3e} "
              f"t {e_dev[1]:.3e} inliers {o['inliers'][b]} rmse {o['rmse'][b]:.3e}  restated rot {e_ref[0]:.3e} t {e_ref[1]:.3e} "
              f"inliers {ref['inliers']}")
        assert e_dev[0] <= 2 * e_ref[0] + 2.0 ** -20 and e_dev[1] <= 2 * e_ref[1] + 2.0 ** -20, (e_dev, e_ref)


@pytest.mark.parametrize("seed", (5, 6))
def test_the_robust_fits_hold_the_pose_least_squares_loses(seed):
    """A quarter of the source pushed 0.03 - 0.07 off the surface, inside max_dist: twenty updates of least squares, of Cauchy
    (k = 0.01) from the same start, and of Tukey (k = 0.02) from the least-squares result -- each by the rule of the whole
    loop against its restatement, and both robust fits strictly below the device's own least squares."""
    Nb, Ns = SHAPES[1]
    f = ro.fits(seed, Nb, Ns)
    c = f["c"]
    one = lambda x: np.ascontiguousarray(np.asarray(x)[None])    # noqa: E731
    a = (one(c["src"]), one(c["tgt"]), one(c["nrm"]))
    kw = dict(max_iterations=20, rel_fitness=0.0, rel_rmse=0.0)
    ls = run(*a, one(c["R0"]), one(c["t0"]), loss="l2", **kw)
    cauchy = run(*a, one(c["R0"]), one(c["t0"]), loss="cauchy", k=0.01, **kw)
    tukey = run(*a, ls["R"], ls["t"], loss="tukey", k=0.02, **kw)
    err = lambda o: pr.pose_error(o["R"][0] if np.ndim(o["R"]) == 3 else o["R"], o["t"][0] if np.ndim(o["t"]) == 2 else o["t"],   # noqa: E731
                                  c["R"], c["t"])
    e_ls = err(ls)
    for name, o in (("least squares", ls), ("cauchy k 0.01", cauchy), ("tukey k 0.02 from least squares", tukey)):
        assert o["iterations"].tolist() == [20]
        e_dev, e_ref = err(o), err(f[{"l": "ls", "c": "cauchy", "t": "tukey"}[name[0]]])
        _emit(f"robust accuracy Nb {Nb} Ns {Ns} seed {seed} {name}: device rot {e_dev[0]:.3e} t {e_dev[1]:.3e} inliers {o['inliers'][0]} "
              f"restated rot {e_ref[0]:.3e} t {e_ref[1]:.3e}")
        assert e_dev[0] <= 2 * e_ref[0] + 2.0 ** -20 and e_dev[1] <= 2 * e_ref[1] + 2.0 ** -20, (name, e_dev, e_ref)
        if o is not ls:
            assert e_dev[0] < e_ls[0] and e_dev[1] < e_ls[1], (name, e_dev, e_ls)


@pytest.mark.parametrize("Nb,Ns,forms", [SHAPES[0] + (((1, 1), (2, 3), (4, 128)),),
                                         SHAPES[1] + (tuple((q, s) for q in (1, 2, 4) for s in (1, 3, 128)),)])
def test_every_launch_form_and_the_grid_return_the_same_bits(Nb, Ns, forms):
    _, refine, _, _ = mods()
    c = recipe(10 + Ns, Nb, Ns)
    a = (c["src"], c["tgt"], c["nrm"], c["R0"], c["t0"])
    auto = run(*a)
    assert (auto["iterations"] >= 2).all() and (auto["iterations"] < 30).all() and auto["converged"].tolist() == [1, 1, 1]
    for q, s in forms:
        assert_same_bits(run(*a, variant=refine.variant(q, s)), auto, (q, s))
    assert_same_bits(run(*a, prefill=0xFF), auto, "a NaN-prefilled workspace")
    for order in (0, 1, 2):
        grid = run(*a, search="grid", order=order)
        assert_same_bits(grid, auto, ("grid", order), ("inliers", "sum_d2", "fitness", "rmse") + POSE)
        lost = grid["nn_idx"] < 0                                # the grid's documented difference: no partner within max_dist
        assert lost[:, Ns:].all() and np.isinf(grid["nn_d2"][lost]).all() and (auto["nn_d2"][lost] > np.float32(rr.MAX_DIST) ** 2).all()
        assert np.array_equal(grid["nn_idx"][~lost], auto["nn_idx"][~lost]) and np.array_equal(bits(grid["nn_d2"][~lost]), bits(auto["nn_d2"][~lost]))
    for b in range(3):                                          # a cloud's result does not depend on its batch
        alone = run(*(x[b:b + 1] for x in a))
        assert_same_bits(alone, {k: auto[k][b:b + 1] for k in EVAL + POSE}, b)


def test_the_stops():
    Nb, Ns = SHAPES[0]
    c = recipe(10 + Ns, Nb, Ns)
    a = (c["src"], c["tgt"], c["nrm"], c["R0"], c["t0"])
    same_pose = lambda o: np.array_equal(bits(o["R"]), bits(c["R0"])) and np.array_equal(bits(o["t"]), bits(c["t0"]))   # noqa: E731
    # every weight zero: A = 0 is singular, and the cloud stops with the pose it has
    o = run(*a, loss="tukey", k=1e-9)
    assert (o["inliers"] >= 6).all() and o["iterations"].tolist() == [0, 0, 0] and o["converged"].tolist() == [0, 0, 0] and same_pose(o)
    # fewer than six inliers: a tiny max_dist from the disturbed start, and five points against themselves
    for loss in ("cauchy", "tukey"):
        o = run(*a, loss=loss, max_dist=1e-4)
        assert (o["inliers"] < 6).all() and o["iterations"].tolist() == [0, 0, 0] and o["converged"].tolist() == [0, 0, 0] and same_pose(o)
    five = np.ascontiguousarray(c["tgt"][:, :, :5])
    o = run(five, five, np.ascontiguousarray(c["nrm"][:, :, :5]), loss="gm")
    assert o["inliers"].tolist() == [5, 5, 5] and o["iterations"].tolist() == [0, 0, 0] and o["converged"].tolist() == [0, 0, 0]
    assert np.array_equal(o["R"], np.broadcast_to(np.eye(3, dtype=np.float32), (3, 3, 3))) and not o["t"].any()
    # NaN normals: non-finite sums, a NaN update; the next evaluation finds no inlier and the cloud stops; the others keep their bits
    clean = run(*a)
    nrm = c["nrm"].copy()
    nrm[0] = np.nan
    o = run(c["src"], c["tgt"], nrm, c["R0"], c["t0"])
    assert np.isnan(o["R"][0]).all() and np.isnan(o["t"][0]).all() and o["iterations"][0] == 1 and o["inliers"][0] == 0
    assert_same_bits({k: o[k][1:] for k in EVAL + POSE}, {k: clean[k][1:] for k in EVAL + POSE}, "the other clouds")


_LONG = {}


def long_pair():
    """16 385 source points against 700 target points, one cloud: 65 partials, one more than CHUNK."""
    if not _LONG:
        p = rr.pair(77, 700, 16385 - FAR, "torus")
        assert p["src"].shape == (3, 16385)
        _LONG.update({k: np.ascontiguousarray(np.asarray(v)[None]).astype(np.float32 if k in ("R0", "t0") else np.asarray(v).dtype)
                      for k, v in p.items()})
    return _LONG


def _matrix_checks(o, tgt, max_dist, what):
    for b in range(tgt.shape[0]):
        ref = ro.information(tgt[b], o["nn_idx"][b], o["nn_d2"][b], max_dist)
        I = o["information"][b]
        assert np.array_equal(bits(I), bits(ref)), (what, b, np.abs(I - ref).max())
        assert np.array_equal(I, I.T) and I[3, 3] == I[4, 4] == I[5, 5] == o["inliers"][b], (what, b)


@pytest.mark.parametrize("Nb,Ns", SHAPES)
def test_the_information_matrix_bit_for_bit(Nb, Ns):
    import vcrnet_amd
    _, refine, _, score = mods()
    c = recipe(10 + Ns, Nb, Ns)
    a = (c["src"], c["tgt"], c["R0"], c["t0"])
    o = run_info(*a)
    assert (o["inliers"] >= 6).all() and (o["inliers"] < Ns + FAR).all()
    _matrix_checks(o, c["tgt"], rr.MAX_DIST, "scan")
    for b in range(3):
        G = ro.information_gtg(c["tgt"][b], o["nn_idx"][b], o["nn_d2"][b], rr.MAX_DIST)
        assert np.abs(o["information"][b] - G).max() <= 1e-12 * np.abs(G).max()
    s = score.nn_score(dev(c["src"]), dev(c["tgt"]), dev(c["R0"]), dev(c["t0"]), rr.MAX_DIST)
    assert_same_bits(o, {k: s[k].cpu().numpy() for k in EVAL}, "the evaluation is vcr_nn_score_f32's", EVAL)
    # every form of the scan, a NaN-prefilled workspace, the grid, a cloud alone: the same matrix
    for v in (refine.variant(1, 1), refine.variant(2, 3), refine.variant(4, 128)):
        assert_same_bits(run_info(*a, variant=v), o, v, EVAL + POSE + ("information",))
    assert_same_bits(run_info(*a, prefill=0xFF), o, "prefill", EVAL + POSE + ("information",))
    for order in (0, 2):
        g = run_info(*a, search="grid", order=order)
        assert_same_bits(g, o, ("grid", order), ("information", "inliers", "sum_d2", "fitness", "rmse") + POSE)
        _matrix_checks(g, c["tgt"], rr.MAX_DIST, "grid")
    alone = run_info(*(x[1:2] for x in a))
    assert_same_bits(alone, {k: o[k][1:2] for k in EVAL + POSE + ("information",)}, "alone", EVAL + POSE + ("information",))
    # no pair within max_dist = 0 (no source point is a target point under the disturbed start): the zero matrix
    z = run_info(*a, max_dist=0.0)
    assert not z["inliers"].any() and not z["information"].any()
    # the public call: the matrix, and with want_score score_registration's dict, bit for bit
    for search in ("scan", "grid"):
        I, sc = vcrnet_amd.information_matrix(dev(c["src"]), dev(c["tgt"]), dev(c["R0"]), dev(c["t0"]), rr.MAX_DIST, search=search,
                                              want_score=True)
        assert I.dtype == torch.float64 and tuple(I.shape) == (3, 6, 6) and np.array_equal(bits(I.cpu().numpy()), bits(o["information"]))
        ref = vcrnet_amd.score_registration(dev(c["src"]), dev(c["tgt"]), dev(c["R0"]), dev(c["t0"]), rr.MAX_DIST, search=search)
        assert sorted(sc) == sorted(ref) == ["fitness", "inlier_rmse", "inliers"]
        for k in ref:
            assert sc[k].dtype == ref[k].dtype and torch.equal(sc[k].view(torch.int32), ref[k].view(torch.int32)), (search, k)
    only = vcrnet_amd.information_matrix(dev(c["src"]), dev(c["tgt"]), dev(c["R0"]), dev(c["t0"]), rr.MAX_DIST)
    assert torch.is_tensor(only) and torch.equal(only, I)
    ident = vcrnet_amd.information_matrix(dev(c["src"]), dev(c["tgt"]), max_dist=rr.MAX_DIST)           # R = t = None: the identity
    eye = run_info(c["src"], c["tgt"])
    assert np.array_equal(bits(ident.cpu().numpy()), bits(eye["information"]))


def test_the_information_matrix_over_more_partials_than_a_chunk():
    c = long_pair()
    o = run_info(c["src"], c["tgt"], c["R0"], c["t0"])
    assert 6 <= o["inliers"][0] <= 16385 - FAR
    _matrix_checks(o, c["tgt"], rr.MAX_DIST, "65 partials")
    g = run_info(c["src"], c["tgt"], c["R0"], c["t0"], search="grid")
    assert_same_bits(g, o, "grid", ("information", "inliers", "sum_d2", "fitness", "rmse"))


def test_the_python_api():
    import vcrnet_amd
    _, _, robust, _ = mods()
    from vcrnet_amd.native import VcrHipError
    Nb, Ns = SHAPES[0]
    c = recipe(10 + Ns, Nb, Ns)
    s, q, R0, t0, nrm = dev(c["src"]), dev(c["tgt"]), dev(c["R0"]), dev(c["t0"]), dev(c["nrm"])
    same = lambda a, b: a.dtype == b.dtype and torch.equal(a.view(torch.int32) if a.dtype == torch.float32 else a,   # noqa: E731
                                                           b.view(torch.int32) if b.dtype == torch.float32 else b)
    pairs = (("R", "R"), ("t", "t"), ("R_ba", "R_ba"), ("t_ba", "t_ba"), ("fitness", "fitness"), ("inlier_rmse", "rmse"),
             ("inliers", "inliers"), ("iterations", "iterations"), ("converged", "converged"))
    for loss, search in (("tukey", "scan"), ("cauchy", "scan"), ("gm", "grid"), ("huber", "scan"), ("l2", "grid")):
        low = robust.refine_robust(s, q, nrm, R0, t0, rr.MAX_DIST, loss, SCALE[loss], search=search)
        res = vcrnet_amd.refine_registration_robust(s, q, R0, t0, max_dist=rr.MAX_DIST, loss=loss, k=SCALE[loss], tgt_normals=nrm, search=search)
        assert sorted(res) == ["R", "R_ba", "converged", "fitness", "inlier_rmse", "inliers", "iterations", "t", "t_ba"]
        for a, b in pairs:
            assert same(res[a], low[b]), (loss, a)
    # the default loss is Tukey; the normals estimated inside are estimate_normals(tgt, normal_k); want_nn as refine_registration's
    default = vcrnet_amd.refine_registration_robust(s, q, R0, t0, max_dist=rr.MAX_DIST, k=SCALE["tukey"], tgt_normals=nrm)
    assert all(same(default[k], res_k) for k, res_k in vcrnet_amd.refine_registration_robust(
        s, q, R0, t0, max_dist=rr.MAX_DIST, loss="tukey", k=SCALE["tukey"], tgt_normals=nrm).items())
    for k in (20, 12):
        inside = vcrnet_amd.refine_registration_robust(s, q, R0, t0, max_dist=rr.MAX_DIST, loss="cauchy", k=0.02, normal_k=k, want_nn=True)
        given = vcrnet_amd.refine_registration_robust(s, q, R0, t0, max_dist=rr.MAX_DIST, loss="cauchy", k=0.02,
                                                      tgt_normals=vcrnet_amd.estimate_normals(q, k), want_nn=True)
        assert sorted(inside) == sorted(list(default) + ["nn_idx", "nn_d2"]) and inside["nn_idx"].dtype == torch.int64
        assert all(same(inside[key], given[key]) for key in inside)
        closing = vcrnet_amd.score_registration(s, q, inside["R"], inside["t"], max_dist=rr.MAX_DIST, want_nn=True)
        for key in ("fitness", "inlier_rmse", "inliers", "nn_idx", "nn_d2"):         # the closing invariant, through the public API
            assert torch.equal(inside[key], closing[key]), key
    # l2 is refine_registration's point to plane
    pl = vcrnet_amd.refine_registration(s, q, R0, t0, max_dist=rr.MAX_DIST, method="point_to_plane", tgt_normals=nrm)
    l2 = vcrnet_amd.refine_registration_robust(s, q, R0, t0, max_dist=rr.MAX_DIST, loss="l2", k=1.0, tgt_normals=nrm)
    assert all(same(l2[k], pl[k]) for k in pl) and not same(default["R"], pl["R"])
    with pytest.raises(VcrHipError, match="k has no default"):
        vcrnet_amd.refine_registration_robust(s, q, R0, t0, max_dist=rr.MAX_DIST)
    with pytest.raises(VcrHipError, match="loss must be one of"):
        vcrnet_amd.refine_registration_robust(s, q, R0, t0, max_dist=rr.MAX_DIST, loss="l1", k=0.02)
    with pytest.raises(VcrHipError, match="k must be finite and > 0"):
        robust.refine_robust(s, q, nrm, R0, t0, rr.MAX_DIST, "tukey", 0.0)
    with pytest.raises(VcrHipError, match=r"tgt_normals must be \[B, 3, Nt\]"):
        vcrnet_amd.refine_registration_robust(s, q, max_dist=0.1, k=0.02, tgt_normals=s)
    with pytest.raises(VcrHipError, match="device of the clouds"):
        vcrnet_amd.refine_registration_robust(s, q, max_dist=0.1, k=0.02, tgt_normals=q.cpu())
    with pytest.raises(VcrHipError, match="unsupported"):
        robust.refine_robust(s, q, nrm, max_dist=0.1, k=0.02, max_iterations=4097)


def test_centre_far_from_the_origin_is_the_run_near_it():
    """Both clouds on the 2^-14 grid (fp32's spacing at 512), then moved by offsets on that grid to coordinates near 512 --
    exactly, and so that the planted translation between them stays small: centre=True subtracts each cloud's mean, which is
    on the grid too, so the centred clouds are those of the run near the origin about the same points (given as centre=(c_src,
    c_tgt) there).  The same iterations and converged; the pose errors, taken where the cloud is (the rotation, and the
    pose's action on the source's centre), within the near run's + 2^-18."""
    import vcrnet_amd
    Nb, Ns = SHAPES[0]
    c = recipe(10 + Ns, Nb, Ns)
    grid = lambda x: (np.round(np.asarray(x, np.float64) * 2.0 ** 14) / 2.0 ** 14)      # noqa: E731
    src, tgt = grid(c["src"]), grid(c["tgt"])
    off_s = np.asarray([512.0, -512.0, 512.0])
    off_t = grid(np.einsum("bij,j->bi", c["R"], off_s))           # about R off_s: the far frames' planted t stays below 1
    far_s, far_t = (src + off_s[None, :, None]).astype(np.float32), (tgt + off_t[:, :, None]).astype(np.float32)
    assert np.array_equal(far_s.astype(np.float64) - off_s[None, :, None], src) and np.abs(far_s).min() > 500       # (exact)
    assert np.array_equal(far_t.astype(np.float64) - off_t[:, :, None], tgt)
    # q' = R (p' - off_s) + t + off_t: the planted pose and the start in the far frames; the near start is the far one's, carried back
    shift = lambda R: off_t - np.einsum("bij,j->bi", R.astype(np.float64), off_s)       # noqa: E731
    t_true_far = c["t"] + shift(c["R"])
    t0_far = (c["t0"].astype(np.float64) + shift(c["R0"])).astype(np.float32)
    t0_near = (t0_far.astype(np.float64) - shift(c["R0"])).astype(np.float32)
    assert np.abs(t_true_far).max() < 1
    nrm = dev(c["nrm"])
    kw = dict(max_dist=rr.MAX_DIST, loss="cauchy", k=0.02, tgt_normals=nrm)
    S, Q = dev(far_s), dev(far_t)
    _, c_s = vcrnet_amd.centred(S)
    _, c_t = vcrnet_amd.centred(Q)
    near_centres = (c_s - dev(off_s.astype(np.float32))[None], c_t - dev(off_t.astype(np.float32)))
    far = vcrnet_amd.refine_registration_robust(S, Q, dev(c["R0"]), dev(t0_far), centre=True, want_nn=True, **kw)
    near = vcrnet_amd.refine_registration_robust(dev(src.astype(np.float32)), dev(tgt.astype(np.float32)), dev(c["R0"]), dev(t0_near),
                                                 centre=near_centres, **kw)
    closing = vcrnet_amd.score_registration(S, Q, far["R"], far["t"], max_dist=rr.MAX_DIST, want_nn=True)
    for key in ("fitness", "inlier_rmse", "inliers", "nn_idx", "nn_d2"):
        assert torch.equal(far[key], closing[key]), key
    assert torch.equal(far["iterations"], near["iterations"]) and torch.equal(far["converged"], near["converged"])
    assert (far["iterations"] >= 2).all() and far["converged"].tolist() == [1, 1, 1]
    for b in range(3):
        errs = []
        for o, p, t_true in ((far, far_s[b], t_true_far[b]), (near, src[b], c["t"][b])):
            Rb, tb = o["R"][b].cpu().numpy().astype(np.float64), o["t"][b].cpu().numpy().astype(np.float64)
            mid = np.asarray(p, np.float64)[:, :Ns].mean(axis=1)
            errs.append((pr.pose_error(Rb, tb, c["R"][b], t_true)[0], float(np.linalg.norm((Rb @ mid + tb) - (c["R"][b] @ mid + t_true)))))
        (rot_f, t_f), (rot_n, t_n) = errs
        _emit(f"robust centre=True near 512 cloud {b}: rot {rot_f:.6e} t at the cloud {t_f:.6e}; near the origin rot {rot_n:.6e} t {t_n:.6e}; "
              f"updates {int(far['iterations'][b])}")
        assert rot_f <= rot_n + 2.0 ** -18 and t_f <= t_n + 2.0 ** -18, (b, errs)
