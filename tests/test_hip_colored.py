"""vcr_color_gradient_f32 and vcr_refine_colored_f32 on the GPU: the refinement by colour and shape on the full clouds
(include/colored/vcr_hip_colored.h).

The input is tests/colored_restated.py's recipe -- the textured patch, flat and bowl, at (Nt, Ns) = (700, 300) and (1500, 900),
B = 3 -- and one tiny case (B = 1, Ns = 6, Nt = 7: six pairs are the fewest a step takes).  What is checked:
  * the gradient against colored_restated.gradient on the device's own neighbour rows, per point within
    2^-22 |x| + 64 cond(M) 2^-53; rows with -1 entries, the point itself, repeats, a radius, fewer than three entries, a NaN
    intensity; a batch against its clouds;
  * one update against colored_restated.colored_step on the device's own iteration-0 neighbours: |dR|, |dt| <=
    2^-22 + 64 cond(A) 2^-53, cond(A) <= 1e6;
  * the whole loop, ten updates, against colored_restated.colored_icp and the planted pose;
  * what the feature is for: where point to plane stops or slides, this one does not;
  * lambda_geometric = 1 is plane.refine_plane bit for bit; the intensity is the channels' mean; a constant added to both
    clouds' colours changes no pose beyond the one-update bound;
  * every launch form, the grid sibling, a cloud alone against the cloud in a batch, Ns around the merge's 256, far points;
  * the stops and NaN colours;
  * in EVERY run the closing invariant, every output element written and no guard band touched;
  * the Python API."""
import os

import numpy as np
import pytest
import torch

import colored_restated as cr
import plane_restated as pr
import refine_restated as rr

pytestmark = pytest.mark.gpu

SENTINEL_BYTE = 0x5A
GUARD = 64
EVAL = ("nn_idx", "nn_d2", "inliers", "sum_d2", "fitness", "rmse")
POSE = ("R", "t", "R_ba", "t_ba", "iterations", "converged")
MAX_DIST = cr.MAX_DIST
LEDGER = []
CASES = [(kind, Nt, Ns) for kind in cr.KINDS for Nt, Ns in cr.SHAPES]


def _emit(line):
    print(line)
    LEDGER.append(line)
    out = os.environ.get("VCR_LEDGER_DIR", "")
    if os.path.isdir(out):
        path = os.path.join(out, "colored_ledger.txt")
        if len(LEDGER) == 1:                                 # a new table: which kernel sources it measures
            import vcrnet_amd  # noqa: F401
            from vcrnet_amd import build as vb
            with open(path, "w") as f:
                f.write(f"# kernel_sources_sha16={vb.sources_sha16()}\n")
        with open(path, "a") as f:
            f.write(line + "\n")


def mods():
    import vcrnet_amd  # noqa: F401
    from vcrnet_amd import colored, native, score
    return colored, native, score


def dev(x):
    return None if x is None else torch.tensor(np.ascontiguousarray(x)).cuda()         # (a copy: the recipes are read-only)


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view({4: np.int32, 8: np.int64}[a.dtype.itemsize])


def assert_same_bits(a, b, what, keys=EVAL + POSE):
    for k in keys:
        assert np.array_equal(bits(a[k]), bits(b[k])), (what, k)


def _guards(raw, view, prefill, name):
    n = view.numel()
    band = raw[n:].view(torch.uint8).cpu().numpy()
    assert band.size == GUARD * raw.element_size() and (band == prefill).all(), (name, "guard band written")
    body = raw[:n].view(torch.uint8).cpu().numpy().reshape(n, -1)
    assert not (body == prefill).all(axis=1).any(), (name, "element left unwritten")


# ------------------------------------------------------------------------------------------------------------ the gradient

def device_gradient(x, nrm, inten, idx, radius=0.0):
    """numpy in ([B,3,N], [B,3,N], [B,N], int [B,N,k]) -> float32 [B,3,N]: one launch, the guards checked."""
    colored, native, _ = mods()
    xyz4 = native.to_rows4(dev(x))
    g, raw = colored.color_gradient(xyz4, dev(np.asarray(idx, np.int32)), dev(nrm), dev(inten), radius, guard=GUARD, prefill=SENTINEL_BYTE)
    torch.cuda.synchronize()
    _guards(raw["gradient"], g, SENTINEL_BYTE, "gradient")
    return g.cpu().numpy()


def device_rows(x, k):
    _, native, _ = mods()
    return native.knn(native.to_rows4(dev(x)), None, k).cpu().numpy()


def _hold_gradient(name, got, x, nrm, inten, idx, radius=0.0):
    """Per cloud and point: |got - restated| <= 2^-22 |x| + 64 cond(M) 2^-53, exact zeros where the restatement says zero."""
    worst = 0.0
    for b in range(x.shape[0]):
        g32, g64, cond, m = cr.gradient(x[b], nrm[b], inten[b], idx[b], radius, want_cond=True)
        zero = ~np.isfinite(cond)
        assert not got[b][:, zero].any(), (name, b, "an exact zero expected")
        if (~zero).any():
            bound = 2.0 ** -22 * np.abs(g64).max(0) + 64 * cond * 2.0 ** -53
            diff = np.abs(got[b].astype(np.float64) - g64).max(0)
            ratio = (diff[~zero] / bound[~zero]).max()
            worst = max(worst, ratio)
            _emit(f"colored gradient {name} cloud {b}: points {int((~zero).sum())} zeros {int(zero.sum())} cond(M) max {cond[~zero].max():.3e} "
                  f"|d| max {diff[~zero].max():.2e} worst |d| / bound {ratio:.3f}")
            assert (diff[~zero] <= bound[~zero]).all(), (name, b, ratio)
    return worst


@pytest.mark.parametrize("N,k", [(300, 20), (300, 62), (5, 4)])
def test_the_gradient_against_the_restatement(N, k):
    c = cr.batch("bowl", 30 + k, N, 10)
    x, nrm, inten = c["tgt"], c["nrm_t"], c["I_t"]
    idx = device_rows(x, k)
    assert idx.shape == (3, N, k)
    got = device_gradient(x, nrm, inten, idx)
    _hold_gradient(f"N {N} k {k}", got, x, nrm, inten, idx)
    assert np.abs((got.astype(np.float64) * nrm).sum(1)).max() <= 1e-5       # in the tangent plane, to fp32
    # a batch equals its clouds run one by one
    for b in range(3):
        assert np.array_equal(bits(device_gradient(x[b:b + 1], nrm[b:b + 1], inten[b:b + 1], idx[b:b + 1])[0]), bits(got[b])), b


def test_the_gradient_of_one_point_and_of_rows_with_holes():
    c = cr.batch("bowl", 31, 300, 10)
    x, nrm, inten = c["tgt"], c["nrm_t"], c["I_t"]
    # N = 1: nothing but the point itself
    for row in ([0], [-1], [0, 0, 7]):
        g = device_gradient(x[:1, :, :1], nrm[:1, :, :1], inten[:1, :1], np.asarray([[row]]))
        assert g.shape == (1, 3, 1) and not g.any()
    idx = device_rows(x, 8).astype(np.int64)
    base = device_gradient(x, nrm, inten, idx)
    own = np.broadcast_to(np.arange(300)[None, :, None], (3, 300, 1))
    full = lambda v: np.full((3, 300, 1), v, np.int64)         # noqa: E731
    # -1 entries, indices beyond N, the point itself: skipped, the same bits
    padded = np.concatenate([full(-1), idx[:, :, :4], own, full(300), idx[:, :, 4:], full(2 ** 31 - 1)], axis=2)
    assert np.array_equal(bits(device_gradient(x, nrm, inten, padded)), bits(base))
    # a repeated entry counts twice
    twice = np.concatenate([idx, idx[:, :, :1]], axis=2)
    got = device_gradient(x, nrm, inten, twice)
    assert not np.array_equal(got, base)
    _hold_gradient("a repeated entry", got, x, nrm, inten, twice)
    # m < 3: an exact zero
    assert not device_gradient(x, nrm, inten, idx[:, :, :2]).any() and device_gradient(x, nrm, inten, idx[:, :, :3]).any()
    # a radius drops the far part of a row, and with it some rows below three entries
    d = np.linalg.norm(np.take_along_axis(x.astype(np.float64), idx[:, None, :, 4], axis=2) - x, axis=1)
    r = float(np.median(d))
    m = np.stack([cr.gradient_system(x[b], nrm[b], inten[b], idx[b], r)[2] for b in range(3)])
    assert m.min() < 3 and m.max() == 8 and (m < 8).mean() > 0.3
    got = device_gradient(x, nrm, inten, idx, r)
    _hold_gradient(f"radius {r:.3f}", got, x, nrm, inten, idx, r)
    assert not np.array_equal(got, base)
    # a NaN intensity stays in the rows that hold it
    bad = inten.copy()
    bad[1, 17] = np.nan
    got = device_gradient(x, nrm, bad, idx)
    holds = (idx[1] == 17).any(1) | (np.arange(300) == 17)
    assert holds.sum() > 1 and not got[1][:, holds].any() and not np.isnan(got).any()
    assert np.array_equal(bits(got[1][:, ~holds]), bits(base[1][:, ~holds]))
    assert np.array_equal(bits(got[[0, 2]]), bits(base[[0, 2]]))


# ------------------------------------------------------------------------------------------------------------- the fit

def run(c, R="R0", t="t0", max_dist=MAX_DIST, prefill=SENTINEL_BYTE, **kw):
    """c: a prepared batch (numpy) -> dict of numpy; test_hip_gicp.run's checks: every output overwritten, no guard band
    touched, the closing invariant, the inverse pose."""
    colored, _, score = mods()
    R, t = (c[R] if isinstance(R, str) else R), (c[t] if isinstance(t, str) else t)
    o = colored.refine_colored(dev(c["src"]), dev(c["tgt"]), dev(c["I_s"]), dev(c["I_t"]), dev(c["nrm_t"]), dev(c["grad"]), dev(R), dev(t),
                               max_dist, guard=GUARD, prefill=prefill, **kw)
    torch.cuda.synchronize()
    out = {k: o[k].cpu().numpy() for k in EVAL + POSE}
    for k in EVAL + POSE:
        _guards(o["_raw"][k], o[k], prefill, k)
    s = score.nn_score(dev(c["src"]), dev(c["tgt"]), o["R"], o["t"], max_dist, search=kw.get("search", "scan"))
    assert_same_bits(out, {k: s[k].cpu().numpy() for k in EVAL}, "closing invariant", EVAL)
    assert (out["nn_idx"] >= -1).all() and (out["nn_idx"] < c["tgt"].shape[2]).all()
    assert np.array_equal(bits(out["R_ba"]), bits(out["R"].transpose(0, 2, 1)))
    return out


_PREPARED = {}
KEYS = ("src", "tgt", "nrm_t", "grad", "I_t", "I_s", "R0", "t0", "R", "t")


def prepared(kind, Nt, Ns, seed=None):
    """colored_restated.batch plus "grad": the DEVICE's gradients over its own 20 nearest neighbours and the analytic normals.
    Computed once, read-only."""
    seed = 10 + Ns if seed is None else seed
    key = (kind, Nt, Ns, seed)
    if key not in _PREPARED:
        c = dict(cr.batch(kind, seed, Nt, Ns))
        c["grad"] = device_gradient(c["tgt"], c["nrm_t"], c["I_t"], device_rows(c["tgt"], cr.K))
        c["grad"].setflags(write=False)
        _PREPARED[key] = c
    return _PREPARED[key]


def cloud(c, b):
    return {k: c[k][b:b + 1] for k in KEYS}


def one(c, b):
    return {k: c[k][b] for k in KEYS}


def _one_update(c, name, B, min_inliers=6):
    _, _, score = mods()
    zero = run(c, max_iterations=0)
    s = score.nn_score(dev(c["src"]), dev(c["tgt"]), dev(c["R0"]), dev(c["t0"]), MAX_DIST)
    assert_same_bits(zero, {k: s[k].cpu().numpy() for k in EVAL}, "max_iterations = 0: the score of the start", EVAL)
    assert zero["iterations"].tolist() == [0] * B and zero["converged"].tolist() == [0] * B
    assert np.array_equal(bits(zero["R"]), bits(c["R0"])) and np.array_equal(bits(zero["t"]), bits(c["t0"]))
    first = run(c, max_iterations=1, rel_fitness=0.0, rel_rmse=0.0)
    assert first["iterations"].tolist() == [1] * B and first["converged"].tolist() == [0] * B
    bounds = []
    for b in range(B):
        up = cr.colored_step(one(c, b), c["R0"][b], c["t0"][b], zero["nn_idx"][b], zero["nn_d2"][b], MAX_DIST)
        assert up["n"] == zero["inliers"][b] >= min_inliers
        R0, t0 = c["R0"][b].astype(np.float64), c["t0"][b].astype(np.float64)
        dR = np.abs(first["R"][b] - up["R"] @ R0).max()
        dt = np.abs(first["t"][b] - (up["R"] @ t0 + up["t"])).max()
        bound = 2.0 ** -22 + 64 * up["cond"] * 2.0 ** -53
        _emit(f"colored step {name} cloud {b}: n {up['n']} cond(A) {up['cond']:.3e} |dR| {dR:.2e} |dt| {dt:.2e} bound {bound:.2e}")
        assert up["cond"] <= 1e6
        assert dR <= bound and dt <= bound, (dR, dt, bound)
        assert 0 < np.abs(first["R"][b] - c["R0"][b]).max()      # (a step was taken)
        bounds.append(bound)
    return zero, first, bounds


@pytest.mark.parametrize("kind,Nt,Ns", CASES)
def test_one_update_against_the_restatement(kind, Nt, Ns):
    _one_update(prepared(kind, Nt, Ns, 20 + Ns), f"{kind} Nt {Nt} Ns {Ns}", 3)


def test_one_update_of_the_tiny_case():
    c = dict(cr.tiny())
    c["grad"] = c["grad_t"].astype(np.float32)
    assert c["src"].shape == (1, 3, 6) and c["tgt"].shape == (1, 3, 7)
    zero, _, _ = _one_update(c, "tiny Ns 6 Nt 7", 1)
    assert zero["inliers"].tolist() == [6]


@pytest.mark.parametrize("kind,Nt,Ns", CASES)
def test_the_whole_loop_against_the_restatement(kind, Nt, Ns):
    c = prepared(kind, Nt, Ns)
    o = run(c, max_iterations=10, rel_fitness=0.0, rel_rmse=0.0)
    assert o["iterations"].tolist() == [10, 10, 10] and o["converged"].tolist() == [0, 0, 0]
    for b in range(3):
        ref = cr.colored_icp(one(c, b), c["R0"][b], c["t0"][b], MAX_DIST, 10, 0.0, 0.0)
        assert ref["iterations"] == 10
        e_dev = pr.pose_error(o["R"][b], o["t"][b], c["R"][b], c["t"][b])
        e_ref = pr.pose_error(ref["R"], ref["t"], c["R"][b], c["t"][b])
        e_0 = pr.pose_error(c["R0"][b], c["t0"][b], c["R"][b], c["t"][b])
        _emit(f"colored loop {kind} Nt {Nt} Ns {Ns} cloud {b}: start rot {e_0[0]:.3e} t {e_0[1]:.3e}  device rot {e_dev[0]:.3e} t {e_dev[1]:.3e} "
              f"inliers {o['inliers'][b]} rmse {o['rmse'][b]:.3e}  restated rot {e_ref[0]:.3e} t {e_ref[1]:.3e} inliers {ref['inliers']}")
        assert e_dev[0] <= 2 * e_ref[0] + 2.0 ** -20 and e_dev[1] <= 2 * e_ref[1] + 2.0 ** -20, (e_dev, e_ref)
        assert e_dev[0] <= e_0[0] / 10 and e_dev[1] <= e_0[1] / 10, (e_dev, e_0)


@pytest.mark.parametrize("Nt,Ns", cr.SHAPES)
def test_it_holds_the_pose_where_point_to_plane_cannot(Nt, Ns):
    """The public calls, with the device's own normals (estimate_normals) and gradients.  Flat: point to plane takes no update
    (its system is singular) and the colored call takes the slide back.  Bowl: point to plane ends at least five times further
    off in translation than the colored call."""
    import vcrnet_amd
    for kind in cr.KINDS:
        c = prepared(kind, Nt, Ns)
        s, q, R0, t0 = dev(c["src"]), dev(c["tgt"]), dev(c["R0"]), dev(c["t0"])
        pl = vcrnet_amd.refine_registration(s, q, R0, t0, max_dist=MAX_DIST, method="point_to_plane")
        co = vcrnet_amd.refine_registration_colored(s, q, dev(c["I_s"]), dev(c["I_t"]), R0, t0, max_dist=MAX_DIST)
        for b in range(3):
            e_p = pr.pose_error(pl["R"][b].cpu().numpy(), pl["t"][b].cpu().numpy(), c["R"][b], c["t"][b])
            e_c = pr.pose_error(co["R"][b].cpu().numpy(), co["t"][b].cpu().numpy(), c["R"][b], c["t"][b])
            e_0 = pr.pose_error(c["R0"][b], c["t0"][b], c["R"][b], c["t"][b])
            _emit(f"colored against point to plane {kind} Nt {Nt} Ns {Ns} cloud {b}: start t {e_0[1]:.3e}  point to plane rot {e_p[0]:.3e} "
                  f"t {e_p[1]:.3e} updates {int(pl['iterations'][b])}  colored rot {e_c[0]:.3e} t {e_c[1]:.3e} updates {int(co['iterations'][b])}")
            assert e_c[0] <= e_0[0] / 10 and e_c[1] <= e_0[1] / 10, (kind, b, e_c)
            if kind == "flat":
                assert int(pl["iterations"][b]) == 0
            else:
                assert e_p[1] >= 5 * e_c[1], (b, e_p, e_c)


def test_lambda_one_is_point_to_plane_and_the_intensity_is_the_mean_of_the_channels():
    import vcrnet_amd
    from vcrnet_amd import plane
    Nt, Ns = cr.SHAPES[0]
    c = prepared("bowl", Nt, Ns)
    geo = run(c, lambda_geometric=1.0)
    s, q = dev(c["src"]), dev(c["tgt"])
    pl = plane.refine_plane(s, q, dev(c["nrm_t"]), dev(c["R0"]), dev(c["t0"]), MAX_DIST)
    assert_same_bits(geo, {k: pl[k].cpu().numpy() for k in EVAL + POSE}, "lambda_geometric = 1")
    assert (geo["iterations"] >= 1).all()
    assert not np.array_equal(run(c)["R"], geo["R"])               # (the colours are read below 1)
    # RGB: swapping two channels of both clouds changes no bit
    rs = np.random.RandomState(3)
    def rgb(I):                                                  # three channels whose mean is about I
        w = rs.uniform(-0.2, 0.2, (I.shape[0], 2, I.shape[1])).astype(np.float32)
        return np.stack([I + w[:, 0], I + w[:, 1], I - w[:, 0] - w[:, 1]], axis=1).astype(np.float32)
    cs, ct = rgb(c["I_s"]), rgb(c["I_t"])
    kw = dict(max_dist=MAX_DIST, tgt_normals=dev(c["nrm_t"]), want_nn=True)
    a = vcrnet_amd.refine_registration_colored(s, q, dev(cs), dev(ct), dev(c["R0"]), dev(c["t0"]), **kw)
    b = vcrnet_amd.refine_registration_colored(s, q, dev(cs[:, [1, 0, 2]]), dev(ct[:, [1, 0, 2]]), dev(c["R0"]), dev(c["t0"]), **kw)
    assert sorted(a) == sorted(b) and all(torch.equal(a[k], b[k]) for k in a)
    mean = lambda x: ((x[:, 0] + x[:, 1]) + x[:, 2]) / np.float32(3)   # noqa: E731
    i = vcrnet_amd.refine_registration_colored(s, q, dev(mean(cs)), dev(mean(ct)), dev(c["R0"]), dev(c["t0"]), **kw)
    assert all(torch.equal(a[k], i[k]) for k in a)


def test_a_constant_added_to_both_clouds_colours_changes_no_pose_beyond_the_step_bound():
    """The residual reads I_t - I_s and the gradient I_j - I_i: a constant cancels up to the rounding of the shifted fp32
    colours (0.25 is exact, the sums are not).  One update, the gradients recomputed from the shifted colours."""
    Nt, Ns = cr.SHAPES[0]
    c = prepared("bowl", Nt, Ns, 20 + Ns)
    _, first, bounds = _one_update(c, f"bowl Nt {Nt} Ns {Ns} (the constant's base)", 3)
    d = dict(c, I_s=(c["I_s"] + np.float32(0.25)).astype(np.float32), I_t=(c["I_t"] + np.float32(0.25)).astype(np.float32))
    d["grad"] = device_gradient(d["tgt"], d["nrm_t"], d["I_t"], device_rows(d["tgt"], cr.K))
    moved = run(d, max_iterations=1, rel_fitness=0.0, rel_rmse=0.0)
    for b in range(3):
        dR, dt = np.abs(moved["R"][b] - first["R"][b]).max(), np.abs(moved["t"][b] - first["t"][b]).max()
        # the shifted colours round at 2^-24 of 0.75: against gradients of about 1.4 over spacings of 0.03 that is 1e-6 of the step
        _emit(f"colored constant +0.25 cloud {b}: |dR| {dR:.2e} |dt| {dt:.2e} bound {bounds[b]:.2e}")
        assert dR <= bounds[b] and dt <= bounds[b], (b, dR, dt, bounds[b])


@pytest.mark.parametrize("kind,Nt,Ns,forms", [("bowl",) + cr.SHAPES[0] + (((1, 1), (2, 3), (4, 128)),),
                                              ("flat",) + cr.SHAPES[1] + (tuple((q, s) for q in (1, 2, 4) for s in (1, 3, 128)),)])
def test_every_launch_form_and_the_grid_return_the_same_bits(kind, Nt, Ns, forms):
    from vcrnet_amd import refine
    c = prepared(kind, Nt, Ns)
    auto = run(c)
    assert (auto["iterations"] >= 3).all()                     # (a cloud may run all thirty: the rel_* test is not the subject here)
    for q, s in forms:
        assert_same_bits(run(c, variant=refine.variant(q, s)), auto, (q, s))
    assert_same_bits(run(c, prefill=0xFF), auto, "a NaN-prefilled workspace")
    # the grid sibling: the same bits but the -1 / +inf of a point without a partner
    limit = np.float32(MAX_DIST) * np.float32(MAX_DIST)
    for kw in (dict(), dict(cell=0.11), dict(order=1), dict(order=2)):
        g = run(c, search="grid", **kw)
        assert_same_bits(g, auto, ("grid", kw), POSE + ("inliers", "sum_d2", "fitness", "rmse"))
        out = ~((auto["nn_idx"] >= 0) & (auto["nn_d2"] <= limit))
        assert np.array_equal(g["nn_idx"], np.where(out, -1, auto["nn_idx"]))
        assert np.array_equal(bits(g["nn_d2"]), bits(np.where(out, np.float32(np.inf), auto["nn_d2"])))
    # a cloud's result does not depend on its batch
    for b in range(3):
        assert_same_bits(run(cloud(c, b)), {k: auto[k][b:b + 1] for k in EVAL + POSE}, b)


def _with_far(c, extra, seed=5):
    rs = np.random.RandomState(seed)
    B = c["src"].shape[0]
    far = rs.uniform(2.0, 3.0, (B, 3, extra)).astype(np.float32)
    junk = rs.normal(size=(B, extra)).astype(np.float32)
    return dict(c, src=np.concatenate([c["src"], far], axis=2), I_s=np.concatenate([c["I_s"], junk], axis=1))


@pytest.mark.parametrize("Ns", [255, 256, 257])
def test_source_sizes_around_the_merges_workgroup(Ns):
    """Ns = 255 / 256 / 257 against the restatement (one update); lanes beyond Ns and far source points add exact zeros: with
    whole trailing workgroups of far points not one bit of a pose moves, with far points inside the last workgroup the pose
    stays within the one-update bound (the butterfly pairs other lanes)."""
    kw = dict(max_iterations=1, rel_fitness=0.0, rel_rmse=0.0)
    c = prepared("bowl", 700, Ns, 40)
    _, first, bounds = _one_update(c, f"bowl Nt 700 Ns {Ns}", 3)
    far = run(_with_far(c, 37), **kw)
    assert np.array_equal(first["inliers"], far["inliers"]) and np.array_equal(bits(first["sum_d2"]), bits(far["sum_d2"]))
    for b in range(3):
        dR, dt = np.abs(first["R"][b] - far["R"][b]).max(), np.abs(first["t"][b] - far["t"][b]).max()
        assert dR <= bounds[b] and dt <= bounds[b], (b, dR, dt)
    if Ns == 256:
        assert_same_bits(first, run(_with_far(c, 256), **kw), "whole trailing workgroups", POSE + ("inliers", "sum_d2"))


def test_the_stops():
    Nt, Ns = cr.SHAPES[0]
    c = prepared("flat", Nt, Ns)
    # fewer than six pairs: a tiny max_dist from the start; the tiny case with five source points
    o = run(c, max_dist=1e-4)
    assert (o["inliers"] < 6).all() and o["iterations"].tolist() == [0, 0, 0] and o["converged"].tolist() == [0, 0, 0]
    assert np.array_equal(bits(o["R"]), bits(c["R0"])) and np.array_equal(bits(o["t"]), bits(c["t0"]))
    five = dict(cr.tiny(Ns=5))
    five["grad"] = five["grad_t"].astype(np.float32)
    o = run(five)
    assert o["inliers"].tolist() == [5] and o["iterations"].tolist() == [0] and o["converged"].tolist() == [0]
    assert np.array_equal(o["R"][0], np.eye(3, dtype=np.float32)) and not o["t"].any()
    # one colour on a flat patch: singular, as point to plane's
    grey = dict(c, I_s=np.full_like(c["I_s"], 0.5), I_t=np.full_like(c["I_t"], 0.5))
    grey["grad"] = device_gradient(grey["tgt"], grey["nrm_t"], grey["I_t"], device_rows(grey["tgt"], cr.K))
    assert not grey["grad"].any()
    o = run(grey)
    assert (o["inliers"] >= 6).all() and o["iterations"].tolist() == [0, 0, 0] and o["converged"].tolist() == [0, 0, 0]
    assert np.array_equal(bits(o["R"]), bits(c["R0"])) and np.array_equal(bits(o["t"]), bits(c["t0"]))


def test_nan_colours_give_a_nan_pose():
    """Non-finite sums: the update is NaN, the next evaluation finds no inlier and the cloud stops -- the other clouds are
    bit-identical to the clean batch.  A NaN in the colour of a source point that is an inlier; in the colour of the target
    point an inlier pairs with; in that point's gradient."""
    Nt, Ns = cr.SHAPES[0]
    c = prepared("bowl", Nt, Ns)
    clean = run(c)
    zero = run(c, max_iterations=0)
    limit = np.float32(MAX_DIST) * np.float32(MAX_DIST)
    for which, b in (("I_s", 0), ("I_t", 2), ("grad", 1)):
        i = int(np.flatnonzero((zero["nn_idx"][b] >= 0) & (zero["nn_d2"][b] <= limit))[5])    # an inlier of the first round
        d = dict(c, **{which: c[which].copy()})
        if which == "I_s":
            d[which][b, i] = np.nan
        elif which == "I_t":
            d[which][b, zero["nn_idx"][b][i]] = np.nan
        else:
            d[which][b, 1, zero["nn_idx"][b][i]] = np.nan
        o = run(d)
        assert np.isnan(o["R"][b]).all() and np.isnan(o["t"][b]).all() and o["iterations"][b] == 1 and o["inliers"][b] == 0
        rest = [x for x in range(3) if x != b]
        assert_same_bits({k: o[k][rest] for k in EVAL + POSE}, {k: clean[k][rest] for k in EVAL + POSE}, (which, "the other clouds"))
    # a NaN colour nothing pairs with changes nothing: far source points'
    far = _with_far(c, 40)
    nan = dict(far, I_s=far["I_s"].copy())
    nan["I_s"][:, Ns:] = np.nan
    assert_same_bits(run(nan), run(far), "NaN colours of far points")


def _same(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(a.view(torch.int32) if a.dtype == torch.float32 else a,
                                                                      b.view(torch.int32) if b.dtype == torch.float32 else b)


PUBLIC = (("R", "R"), ("t", "t"), ("R_ba", "R_ba"), ("t_ba", "t_ba"), ("fitness", "fitness"), ("inlier_rmse", "rmse"),
          ("inliers", "inliers"), ("iterations", "iterations"), ("converged", "converged"))


def test_the_python_api():
    import vcrnet_amd
    from vcrnet_amd.native import VcrHipError
    colored, native, _ = mods()
    Nt, Ns = cr.SHAPES[0]
    c = prepared("bowl", Nt, Ns)
    s, q, R0, t0 = dev(c["src"]), dev(c["tgt"]), dev(c["R0"]), dev(c["t0"])
    Is, It, nt, gt = dev(c["I_s"]), dev(c["I_t"]), dev(c["nrm_t"]), dev(c["grad"])
    # everything given: colored.refine_colored
    low = colored.refine_colored(s, q, Is, It, nt, gt, R0, t0, MAX_DIST)
    res = vcrnet_amd.refine_registration_colored(s, q, Is, It, R0, t0, max_dist=MAX_DIST, tgt_normals=nt, tgt_gradient=gt)
    assert sorted(res) == sorted(a for a, _ in PUBLIC) and all(_same(res[a], low[b]) for a, b in PUBLIC)
    # tgt_gradient=None: compute_color_gradient with the normals in use, 20 neighbours, no radius -- the brute force's rows
    g20 = vcrnet_amd.compute_color_gradient(q, nt, It)
    assert _same(g20, gt) and _same(g20, vcrnet_amd.compute_color_gradient(q, nt, It, k=20, radius=None, search="knn"))
    grid_rows = vcrnet_amd.search_knn(q, 20)
    assert _same(vcrnet_amd.compute_color_gradient(q, nt, It, search="grid"), vcrnet_amd.compute_color_gradient(q, nt, It, idx=grid_rows))
    for kw in (dict(), dict(gradient_k=20), dict(tgt_gradient=g20)):
        r = vcrnet_amd.refine_registration_colored(s, q, Is, It, R0, t0, max_dist=MAX_DIST, tgt_normals=nt, **kw)
        assert all(_same(r[k], res[k]) for k in res), kw
    r12 = vcrnet_amd.refine_registration_colored(s, q, Is, It, R0, t0, max_dist=MAX_DIST, tgt_normals=nt, gradient_k=12, gradient_radius=0.08)
    assert _same(vcrnet_amd.compute_color_gradient(q, nt, It, k=12, radius=0.08), colored.color_gradient(
        native.to_rows4(q), native.knn(native.to_rows4(q), None, 12), nt, It, 0.08)) and not _same(r12["R"], res["R"])
    # tgt_normals=None: estimate_normals(tgt, normal_k), and the gradient from THOSE normals
    en = vcrnet_amd.estimate_normals(q, 20)
    given = vcrnet_amd.refine_registration_colored(s, q, Is, It, R0, t0, max_dist=MAX_DIST, tgt_normals=en, want_nn=True,
                                                   tgt_gradient=vcrnet_amd.compute_color_gradient(q, en, It))
    for kw in (dict(), dict(normal_k=20), dict(tgt_normals=en)):
        inside = vcrnet_amd.refine_registration_colored(s, q, Is, It, R0, t0, max_dist=MAX_DIST, want_nn=True, **kw)
        assert sorted(inside) == sorted(given) and inside["nn_idx"].dtype == torch.int64
        assert all(_same(inside[k], given[k]) for k in given), kw
    closing = vcrnet_amd.score_registration(s, q, given["R"], given["t"], max_dist=MAX_DIST, want_nn=True)
    for key in ("fitness", "inlier_rmse", "inliers", "nn_idx", "nn_d2"):             # the closing invariant, through the public API
        assert torch.equal(given[key], closing[key]), key
    # lambda_geometric is read; search="grid" returns the scan's poses
    assert not _same(vcrnet_amd.refine_registration_colored(s, q, Is, It, R0, t0, max_dist=MAX_DIST, tgt_normals=nt, lambda_geometric=0.5)["R"], res["R"])
    gr = vcrnet_amd.refine_registration_colored(s, q, Is, It, R0, t0, max_dist=MAX_DIST, tgt_normals=nt, search="grid")
    assert all(_same(gr[k], res[k]) for k in res)
    # the refusals
    with pytest.raises(VcrHipError, match=r"tgt_normals must be \[B, 3, N\]"):
        vcrnet_amd.refine_registration_colored(s, q, Is, It, max_dist=0.1, tgt_normals=s)
    with pytest.raises(VcrHipError, match=r"tgt_gradient must be \[B, 3, N\]"):
        vcrnet_amd.refine_registration_colored(s, q, Is, It, max_dist=0.1, tgt_normals=nt, tgt_gradient=s)
    with pytest.raises(VcrHipError, match=r"src_colors must be \[B, 3, N\] RGB or \[B, N\]"):
        vcrnet_amd.refine_registration_colored(s, q, It, It, max_dist=0.1)
    with pytest.raises(VcrHipError, match=r"tgt_colors must be \[B, 3, N\] RGB or \[B, N\]"):
        vcrnet_amd.refine_registration_colored(s, q, Is, Is, max_dist=0.1)
    with pytest.raises(VcrHipError, match="device of the clouds"):
        vcrnet_amd.refine_registration_colored(s, q, Is.cpu(), It, max_dist=0.1)
    with pytest.raises(VcrHipError, match="device of the clouds"):
        vcrnet_amd.refine_registration_colored(s, q, Is, It, max_dist=0.1, tgt_normals=nt.cpu())
    with pytest.raises(VcrHipError, match="give both R and t"):
        vcrnet_amd.refine_registration_colored(s, q, Is, It, R0, None, max_dist=0.1)
    with pytest.raises(VcrHipError, match="k must be in"):
        vcrnet_amd.compute_color_gradient(q, nt, It, k=63)
    with pytest.raises(VcrHipError, match="unsupported"):
        colored.refine_colored(s, q, Is, It, nt, gt, max_dist=0.1, max_iterations=4097)


def test_centre_returns_the_pose_in_the_callers_frame():
    """The patch moved 100 extents from the origin (an offset on the fp32 grid of the coordinates, so the subtraction is
    exact): centre=True works about the clouds' centres and carries the pose back; it ends within a tenth of the start's
    error, as the loop near the origin."""
    import vcrnet_amd
    Nt, Ns = cr.SHAPES[0]
    c = prepared("bowl", Nt, Ns)
    off_s, off_t = np.asarray([100.0, -75.0, 50.0]), np.asarray([-50.0, 100.0, 75.0])
    src = (c["src"].astype(np.float64) + off_s[None, :, None]).astype(np.float32)
    tgt = (c["tgt"].astype(np.float64) + off_t[None, :, None]).astype(np.float32)
    # q = R (p - off_s) + t + off_t: the planted pose and the start in the moved frames
    far_t = lambda R, t: (t.astype(np.float64) + off_t - np.einsum("bij,j->bi", R.astype(np.float64), off_s))   # noqa: E731
    t_true, t_start = far_t(c["R"], c["t"]), far_t(c["R0"], c["t0"])
    s, q = dev(src), dev(tgt)
    o = vcrnet_amd.refine_registration_colored(s, q, dev(c["I_s"]), dev(c["I_t"]), dev(c["R0"]), dev(t_start.astype(np.float32)),
                                               max_dist=MAX_DIST, centre=True, want_nn=True)
    closing = vcrnet_amd.score_registration(s, q, o["R"], o["t"], max_dist=MAX_DIST, want_nn=True)
    for key in ("fitness", "inlier_rmse", "inliers", "nn_idx", "nn_d2"):
        assert torch.equal(o[key], closing[key]), key
    for b in range(3):
        # compared where the patch is: the pose's action on the source's centre, not t at the far origin
        Rb, tb = o["R"][b].cpu().numpy().astype(np.float64), o["t"][b].cpu().numpy().astype(np.float64)
        mid = src[b].astype(np.float64).mean(axis=1)
        e_rot = pr.pose_error(Rb, tb, c["R"][b], t_true[b])[0]
        e_t = float(np.linalg.norm((Rb @ mid + tb) - (c["R"][b] @ mid + t_true[b])))
        e_0 = pr.pose_error(c["R0"][b], c["t0"][b], c["R"][b], c["t"][b])
        _emit(f"colored centre=True 100 extents off cloud {b}: rot {e_rot:.3e} t at the patch {e_t:.3e} (start {e_0[0]:.3e} {e_0[1]:.3e}) "
              f"updates {int(o['iterations'][b])}")
        assert int(o["iterations"][b]) >= 1 and e_rot <= e_0[0] / 10 and e_t <= e_0[1] / 10, (b, e_rot, e_t)
