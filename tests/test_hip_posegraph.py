"""vcr_posegraph_optimize_f64 on the GPU (include/posegraph/vcr_hip_posegraph.h) against
tests/posegraph_restated.py, and register_multiway on five views of the torus.

The graphs are the restatement's recipes: the ring (K = 8, E = 14, one wrong closure), the triangle with a duplicate edge (K = 3,
E = 4), chains up to K = 128.  Every run fills its outputs and its workspace with a sentinel byte first and checks that every
output element was written and no guard band touched.

Allowances (eps = 2^-53):
  * l, residual0, H, b of the initial linearisation.  Both sides form an entry from the same elementary products in the same
    order and differ in sin / cos / atan2 alone (a few eps on r), so an entry of H or b, a sum of n products l J info J (36 an
    edge of its block), is held to (n + 8) eps sum |products|, the products the restatement's own.  q = r^T info r is such a
    sum of 36; l = (mu / (mu + q))^2 follows q with |dl/dq| = 2 l / (mu + q) and takes 8 eps of its own for its three
    operations; residual0 adds E terms l q + mu (s - 1)^2, each with its allowance, and (E + 8) eps of their sum.
  * the first solve: |d - numpy.linalg.solve(H + lambda I, b)| <= 64 cond(H + lambda I) eps |d|, section 4.31's form, on the
    DEVICE's system.
  * poses after a loop: the sum over the restatement's solves of 64 cond eps (a step moves a pose entry by at most |d| <= 1,
    each solve is off by its bound), plus 64 eps for the composition of the poses themselves."""
import os

import numpy as np
import pytest
import torch

import posegraph_restated as pgr
import refine_restated as rr

pytestmark = pytest.mark.gpu

EPS = 2.0 ** -53
SENTINEL_BYTE = 0x5A
GUARD = 16
ZERO = dict(min_relative_increment=0.0, min_relative_residual_increment=0.0, min_right_term=0.0, min_residual=0.0)
LEDGER = []
OUT = ("R", "t", "weight", "kept", "residual", "iterations", "converged")


def _emit(line):
    print(line)
    LEDGER.append(line)
    out = os.environ.get("VCR_LEDGER_DIR", "")
    if os.path.isdir(out):
        path = os.path.join(out, "posegraph_ledger.txt")
        if len(LEDGER) == 1:                                 # a new table: which kernel sources it measures
            import vcrnet_amd  # noqa: F401
            from vcrnet_amd import build as vb
            with open(path, "w") as f:
                f.write(f"# kernel_sources_sha16={vb.sources_sha16()}\n")
        with open(path, "a") as f:
            f.write(line + "\n")


def mod():
    import vcrnet_amd  # noqa: F401
    from vcrnet_amd import posegraph
    return posegraph


def dev(x, dtype):
    return torch.as_tensor(np.array(x)).to("cuda", dtype)


def tensors(g, R0, t0):
    """The graph and its poses as the device takes them (src, dst on the device: no host check)."""
    return (dev(R0, torch.float64), dev(t0, torch.float64), dev(g.src, torch.int32), dev(g.dst, torch.int32), dev(g.Re, torch.float64),
            dev(g.te, torch.float64), dev(g.info, torch.float64), dev(g.unc, torch.int32))


def run(args, prefill=SENTINEL_BYTE, **kw):
    """posegraph.optimize with guarded, prefilled outputs -> numpy dict; every element written, no guard band touched."""
    o = mod().optimize(*args, max_correspondence_distance=pgr.MCD, guard=GUARD, prefill=prefill, **kw)
    torch.cuda.synchronize()
    raw = o.pop("_raw")
    skip = {"delta0"} if (kw.get("criteria") or {}).get("max_iteration", 100) == 0 else set()
    for name, buf in raw.items():
        b = buf.view(torch.uint8).cpu().numpy()
        n = buf.numel() - GUARD
        assert (b[n * buf.element_size():] == prefill).all(), name
        if name not in skip and n:
            words = b[:n * buf.element_size()].reshape(n, buf.element_size())
            assert not (words == prefill).all(axis=1).any(), f"{name}: an element was not written"
    return {k: v.cpu().numpy() for k, v in o.items()}


def same_bits(a, b, keys=OUT):
    for k in keys:
        assert a[k].tobytes() == b[k].tobytes(), k


@pytest.mark.parametrize("name", ["ring", "triangle"])
def test_the_linearisation_is_the_restatements(name):
    rc = getattr(pgr, name)()
    g, R0, t0 = rc["graph"], rc["R0"], rc["t0"]
    o = run(tensors(g, R0, t0), criteria=dict(max_iteration=0), want_system=True)
    mu = pgr.mu_of(g, g.valid, pgr.MCD)
    lin = pgr.linearise(g, R0, t0, g.valid, mu, 0, want_abs=True)
    r = pgr.residuals(R0, t0, g.s, g.d, g.Re, g.te)
    qabs = np.einsum("ep,epq,eq->e", np.abs(r), np.abs(g.info), np.abs(r))
    l = lin["s"] ** 2
    tol_q = (36 + 8) * EPS * qabs
    tol_l = np.where(g.unc, 2 * l / (mu + lin["q"]) * tol_q + 8 * EPS * l, 0.0)
    d_l = np.abs(o["l0"] - l)
    assert (d_l <= tol_l).all(), (d_l, tol_l)
    terms = pgr.residual_terms(lin["q"], lin["s"], g.unc, g.valid, mu)
    tol_terms = l * tol_q + lin["q"] * tol_l + np.where(g.unc, 2 * mu * np.abs(lin["s"] - 1) * tol_l / (2 * np.maximum(lin["s"], 1e-300)), 0.0) + 8 * EPS * terms
    tol_res = tol_terms.sum() + (g.E + 8) * EPS * np.abs(terms).sum()
    d_res = abs(float(o["residual0"]) - lin["res"])
    assert d_res <= tol_res, (d_res, tol_res)
    assert o["residual"][0] == o["residual0"] == o["residual"][1]
    tol_H, tol_b = (lin["Hn"] + 8) * EPS * lin["Habs"], (lin["bn"] + 8) * EPS * lin["babs"]
    d_H, d_b = np.abs(o["H"] - lin["H"]), np.abs(o["b"] - lin["b"])
    assert (d_H <= tol_H).all(), float((d_H - tol_H).max())
    assert (d_b <= tol_b).all(), float((d_b - tol_b).max())
    assert np.array_equal(o["H"], o["H"].T)                 # symmetric to the bit
    eye = np.zeros((6, 6 * g.K))
    eye[:, :6] = np.eye(6)
    assert np.array_equal(o["H"][:6], eye) and np.array_equal(o["H"][:, :6], eye.T) and not o["b"][:6].any()
    assert np.array_equal(o["R"], R0) and np.array_equal(o["t"], t0) and o["converged"] == 0 and not o["iterations"].any()
    assert float(o["lambda0"]) == 1e-5 * np.max(np.diag(o["H"]))
    with np.errstate(divide="ignore", invalid="ignore"):
        _emit(f"linearisation {name}: max |dH| / allowance {np.nanmax(np.where(tol_H > 0, d_H / tol_H, 0)):.3f} (max |dH| {d_H.max():.3e}), "
              f"|db| / allowance {np.nanmax(np.where(tol_b > 0, d_b / tol_b, 0)):.3f} (max |db| {d_b.max():.3e}), max |dl| {d_l.max():.3e}, "
              f"|dresidual0| {d_res:.3e} (allowance {tol_res:.3e})")


@pytest.mark.parametrize("name", ["ring", "triangle"])
def test_the_first_solve_solves_the_devices_system(name):
    rc = getattr(pgr, name)()
    o = run(tensors(rc["graph"], rc["R0"], rc["t0"]), criteria=dict(ZERO, max_iteration=1, max_iteration_lm=1), want_system=True)
    A = o["H"] + float(o["lambda0"]) * np.eye(len(o["b"]))
    ref = np.linalg.solve(A, o["b"])
    cond = np.linalg.cond(A)
    err = np.abs(o["delta0"] - ref).max() / np.abs(ref).max()
    _emit(f"first solve {name}: cond {cond:.3e}, relative error {err:.3e} (allowance {64 * cond * EPS:.3e})")
    assert cond < 1e9 and err <= 64 * cond * EPS
    assert not o["delta0"][:6].any()                        # the anchor does not move
    assert o["trials"].tolist() == [1, 1] or o["trials"].tolist() == [1, 0]


def _against_restatement(rc, criteria, label, **kw):
    g, R0, t0 = rc["graph"], rc["R0"], rc["t0"]
    conds = []
    ref = pgr.optimize(g, R0, t0, pgr.MCD, criteria=criteria, conds=conds, **kw)
    o = run(tensors(g, R0, t0), criteria=criteria, want_system=True, **kw)
    tol = 64 * EPS * (sum(conds) + 1)
    dR, dt = np.abs(o["R"] - ref["R"]).max(), np.abs(o["t"] - ref["t"]).max()
    _emit(f"{label}: iterations {o['iterations'].tolist()}, trials {o['trials'].tolist()}, converged {int(o['converged'])}, max cond "
          f"{max(conds):.3e}, |dR| {dR:.3e}, |dt| {dt:.3e} (allowance {tol:.3e})")
    assert np.array_equal(o["kept"], ref["kept"])
    # the first pass' trials too; the second starts next to the minimum, where res - res_new is rounding noise once the
    # thresholds are 0 and the number of rejected trials is nobody's to predict
    assert o["iterations"].tolist() == ref["iterations"].tolist() and o["trials"][0] == ref["trials"][0]
    assert int(o["converged"]) == ref["converged"]
    assert dR <= tol and dt <= tol
    return o, ref, tol


def test_six_iterations_follow_the_restatement():
    rc = pgr.ring()
    o, ref, _ = _against_restatement(rc, dict(ZERO, max_iteration=6), "ring, six iterations, thresholds 0")
    assert o["iterations"].tolist() == [6, 6] and o["converged"] == 0
    assert o["kept"][rc["wrong_edge"]] == 0 and o["kept"].sum() == rc["graph"].E - 1
    assert o["residual"][1] <= o["residual"][0]
    assert np.array_equal(o["R"][0], rc["R0"][0]) and np.array_equal(o["t"][0], rc["t0"][0])
    _against_restatement(pgr.triangle(), dict(ZERO, max_iteration=4), "triangle, four iterations, thresholds 0")


def test_the_default_criteria_converge_to_the_restatements_poses():
    rc = pgr.ring()
    o, ref, tol = _against_restatement(rc, None, "ring, default criteria")
    assert o["converged"] == 1
    e_dev = pgr.pose_error(o["R"], o["t"], rc["R_true"], rc["t_true"])
    e_ref = pgr.pose_error(ref["R"], ref["t"], rc["R_true"], rc["t_true"])
    e_odo = pgr.pose_error(rc["R0"], rc["t0"], rc["R_true"], rc["t_true"])
    _emit(f"ring, default criteria: pose error (rad, length) device {e_dev[0]:.6e} {e_dev[1]:.6e}, restatement {e_ref[0]:.6e} {e_ref[1]:.6e}, "
          f"chained odometry {e_odo[0]:.6e} {e_odo[1]:.6e}")
    assert e_dev[0] <= e_ref[0] + 2 * tol and e_dev[1] <= e_ref[1] + 2 * tol
    o1, _, _ = _against_restatement(rc, None, "ring, default criteria, prune=False", prune=False)
    assert o1["kept"].all() and o1["iterations"][1] == 0 and o1["weight"][rc["wrong_edge"]] < 0.25


def _first_global_K():
    pg = mod()
    K = next(K for K in range(1, 129) if pg.posegraph_form(K)[0] == pg.FORM_GLOBAL)
    assert pg.posegraph_form(K - 1)[0] == pg.FORM_LDS
    return K


def test_the_two_forms_and_any_workspace_give_the_same_bits():
    pg = mod()
    rc = pgr.ring()
    a = tensors(rc["graph"], rc["R0"], rc["t0"])
    crit = dict(max_iteration=8)
    base = run(a, criteria=crit)
    same_bits(base, run(a, criteria=crit, variant=pg.FORM_LDS))
    same_bits(base, run(a, criteria=crit, variant=pg.FORM_GLOBAL))
    same_bits(base, run(a, criteria=crit, variant=pg.FORM_GLOBAL, prefill=0xFF))     # a workspace of NaNs
    same_bits(base, run(a, criteria=crit, prefill=0xFF))
    Kg = _first_global_K()
    for K in (Kg - 1, Kg):                                  # the last K of the LDS form, the first of the global form
        ch = pgr.chain(K, 4, 7)
        a = tensors(ch["graph"], ch["R0"], ch["t0"])
        glob = run(a, criteria=crit, variant=pg.FORM_GLOBAL)
        same_bits(glob, run(a, criteria=crit))
        if K < Kg:
            same_bits(glob, run(a, criteria=crit, variant=pg.FORM_LDS))
        else:
            with pytest.raises(pg.VcrHipError):
                run(a, criteria=crit, variant=pg.FORM_LDS)
        ref = pgr.optimize(ch["graph"], ch["R0"], ch["t0"], pgr.MCD, criteria=crit)
        assert np.array_equal(glob["kept"], ref["kept"]) and glob["iterations"].tolist() == ref["iterations"].tolist()


def _padded(rc, K, E, slots=None):
    """The recipe's graph in K nodes and E edge slots: further nodes at the identity, further slots blank; slots: where the
    edges go (ascending), default the first ones."""
    g = rc["graph"]
    slots = np.arange(g.E) if slots is None else np.asarray(slots)
    R, t = np.tile(np.eye(3), (K, 1, 1)), np.zeros((K, 3))
    R[:g.K], t[:g.K] = rc["R0"], rc["t0"]
    src, dst, unc = np.full(E, -1), np.full(E, -1), np.zeros(E, int)
    Re, te, info = np.full((E, 3, 3), np.nan), np.full((E, 3), np.nan), np.full((E, 6, 6), np.nan)   # a blank's payload is never read into a sum
    src[slots], dst[slots], unc[slots], Re[slots], te[slots], info[slots] = g.src, g.dst, g.unc, g.Re, g.te, g.info
    return R, t, src, dst, Re, te, info, unc


def test_a_graph_does_not_depend_on_its_batch_or_on_where_its_blanks_are():
    ring, tri = pgr.ring(), pgr.triangle()
    K, E = 8, 14
    alone = run(tensors(ring["graph"], ring["R0"], ring["t0"]))
    members = [_padded(tri, K, E), _padded(ring, K, E), _padded(tri, K, E, slots=[1, 5, 9, 13])]
    batch = [np.stack([m[i] for m in members]) for i in range(8)]
    types = (torch.float64, torch.float64, torch.int32, torch.int32, torch.float64, torch.float64, torch.float64, torch.int32)
    o = run(tuple(dev(x, ty) for x, ty in zip(batch, types)))
    same_bits(alone, {k: v[1] for k, v in o.items()})
    tri_alone = run(tensors(tri["graph"], tri["R0"], tri["t0"]))
    assert tri_alone["converged"] == 1
    for b, slots in ((0, np.arange(4)), (2, np.array([1, 5, 9, 13]))):
        assert o["R"][b, :3].tobytes() == tri_alone["R"].tobytes() and o["t"][b, :3].tobytes() == tri_alone["t"].tobytes()
        assert o["weight"][b][slots].tobytes() == tri_alone["weight"].tobytes() and np.array_equal(o["kept"][b][slots], tri_alone["kept"])
        assert o["residual"][b].tobytes() == tri_alone["residual"].tobytes() and o["converged"][b] == tri_alone["converged"]
        blank = np.setdiff1d(np.arange(E), slots)
        assert np.isnan(o["weight"][b][blank]).all() and not o["kept"][b][blank].any()
        assert np.array_equal(o["R"][b, 3:], np.tile(np.eye(3), (K - 3, 1, 1))) and not o["t"][b, 3:].any()   # a node no edge touches stays
    # the ring's edges interleaved with blanks in 40 slots against the same edges compacted
    slots = np.sort(np.random.RandomState(1).choice(40, 14, replace=False))
    inter = run(tuple(dev(x, ty) for x, ty in zip(_padded(ring, 8, 40, slots), types)))
    for k in ("R", "t", "residual", "iterations", "converged"):
        assert inter[k].tobytes() == alone[k].tobytes(), k
    assert inter["weight"][slots].tobytes() == alone["weight"].tobytes() and np.array_equal(inter["kept"][slots], alone["kept"])
    # on the device an edge with an index >= K or with src == dst is a blank
    R, t, src, dst, Re, te, info, unc = _padded(ring, 8, 16)
    src[14], dst[14], src[15], dst[15] = 3, 8, 5, 5
    Re[14:], te[14:], info[14:] = np.eye(3), 0.0, np.eye(6)
    bad = run(tuple(dev(x, ty) for x, ty in zip((R, t, src, dst, Re, te, info, unc), types)))
    for k in ("R", "t", "residual", "iterations", "converged"):
        assert bad[k].tobytes() == alone[k].tobytes(), k
    assert not bad["kept"][14:].any() and np.isnan(bad["weight"][14:]).all()


def test_the_edges_of_the_domain():
    pg = mod()
    one = run((dev(np.eye(3)[None], torch.float64), dev(np.zeros((1, 3)), torch.float64), torch.zeros(0, dtype=torch.int32, device="cuda"),
               torch.zeros(0, dtype=torch.int32, device="cuda"), torch.zeros(0, 3, 3, dtype=torch.float64, device="cuda"),
               torch.zeros(0, 3, dtype=torch.float64, device="cuda"), torch.zeros(0, 6, 6, dtype=torch.float64, device="cuda"),
               torch.zeros(0, dtype=torch.int32, device="cuda")))
    assert one["converged"] == 1 and np.array_equal(one["R"], np.eye(3)[None]) and not one["t"].any() and not one["residual"].any()
    # every uncertain edge pruned: closures that all disagree wildly with the odometry
    rc = pgr.ring()
    g = rc["graph"]
    Re, te = g.Re.copy(), g.te.copy()
    rs = np.random.RandomState(2)
    for e in np.nonzero(g.unc)[0]:
        Rn, tn = pgr.euler(rs.uniform(0.5, 0.9, 6) * rs.choice([-1, 1], 6))
        Re[e], te[e] = pgr.compose(Rn, tn, Re[e], te[e])
    gw = pgr.Graph(g.src, g.dst, Re, te, g.info, g.unc, g.K)
    o, _, _ = _against_restatement(dict(rc, graph=gw), None, "ring, every closure wrong")
    assert not o["kept"][g.unc].any() and o["kept"][~g.unc].all() and o["converged"] == 1
    # a NaN in one information matrix: that graph stops with the poses given, the others of the batch do not see it
    R, t, src, dst, Re, te, info, unc = (np.stack([x, x, x]) for x in _padded(rc, 8, 14))
    info[1, 3, 2, 2] = np.nan
    types = (torch.float64, torch.float64, torch.int32, torch.int32, torch.float64, torch.float64, torch.float64, torch.int32)
    o = run(tuple(dev(x, ty) for x, ty in zip((R, t, src, dst, Re, te, info, unc), types)))
    alone = run(tensors(g, rc["R0"], rc["t0"]))
    for b in (0, 2):
        same_bits(alone, {k: v[b] for k, v in o.items()})
    assert o["converged"][1] == 0 and np.array_equal(o["R"][1], rc["R0"]) and np.array_equal(o["t"][1], rc["t0"])
    assert o["iterations"][1].tolist() == [1, 0]
    # the largest graph: a chain of 128 with closures, once
    ch = pgr.chain()
    crit = dict(max_iteration=30)
    o = run(tensors(ch["graph"], ch["R0"], ch["t0"]), criteria=crit)
    ref = pgr.optimize(ch["graph"], ch["R0"], ch["t0"], pgr.MCD, criteria=crit)
    assert np.isfinite(o["R"]).all() and np.isfinite(o["t"]).all() and o["converged"] == 1 == ref["converged"]
    assert o["residual"][1] <= o["residual"][0] and np.array_equal(o["kept"], ref["kept"])
    assert pg.posegraph_form(128)[0] == pg.FORM_GLOBAL


def _views(seed=4, K=5, n=700):
    """K views of the torus, each its own sample of the surface, view i moved by the planted T_i^-1 (so that T_i takes it back
    into view 0's frame); neighbours differ by the recipe's 6 degrees and 0.04."""
    rs = np.random.RandomState(seed)
    R_true, t_true = [np.eye(3)], [np.zeros(3)]
    for i in range(1, K):
        d = rs.normal(size=3)
        Rn, tn = rr.rotation(rs.normal(size=3), 6.0), 0.04 * d / np.linalg.norm(d)
        Ri, ti = pgr.compose(R_true[-1], t_true[-1], Rn, tn)
        R_true.append(Ri); t_true.append(ti)
    clouds = []
    for i in range(K):
        base = rr.base_cloud(rs, n, "torus")
        Rinv, tinv = pgr.inverse(R_true[i], t_true[i])
        clouds.append((Rinv @ base + tinv[:, None]).astype(np.float32))
    return np.stack(clouds), np.array(R_true), np.array(t_true)


def test_register_multiway_on_five_views_of_the_torus():
    import vcrnet_amd
    pg = mod()
    clouds, R_true, t_true = _views()
    x = dev(clouds, torch.float32)
    coarse, fine = 0.15, 0.05
    res = vcrnet_amd.register_multiway(x, coarse, fine)
    g = res["graph"]
    torch.cuda.synchronize()
    assert g["pairs"] == pg.all_pairs(5) and g["uncertain"].tolist() == [0 if j == i + 1 else 1 for i, j in g["pairs"]]
    for n, (i, j) in enumerate(g["pairs"]):                 # the batch's pairs are the pairs alone, bit for bit
        c = vcrnet_amd.refine_registration(x[i:i + 1], x[j:j + 1], None, None, coarse, method="point_to_plane")
        f = vcrnet_amd.refine_registration(x[i:i + 1], x[j:j + 1], c["R"], c["t"], fine, method="point_to_plane")
        info = vcrnet_amd.information_matrix(x[i:i + 1], x[j:j + 1], f["R"], f["t"], fine)
        assert torch.equal(f["R"][0], g["R_edge"][n]) and torch.equal(f["t"][0], g["t_edge"][n]) and torch.equal(info[0], g["information"][n]), (i, j)
        assert torch.equal(f["fitness"][0], g["fitness"][n]) and torch.equal(f["inlier_rmse"][0], g["inlier_rmse"][n])
    Re, te = g["R_edge"].double().cpu().numpy(), g["t_edge"].double().cpu().numpy()
    gr = pgr.Graph(g["src"].cpu().numpy(), g["dst"].cpu().numpy(), Re, te, g["information"].cpu().numpy(), g["uncertain"].cpu().numpy(), 5)
    R0, t0 = [np.eye(3)], [np.zeros(3)]
    for i in range(4):
        Ri, ti = pgr.inverse(Re[g["pairs"].index((i, i + 1))], te[g["pairs"].index((i, i + 1))])
        Rn, tn = pgr.compose(R0[-1], t0[-1], Ri, ti)
        R0.append(Rn); t0.append(tn)
    assert np.abs(g["R"].cpu().numpy() - np.array(R0)).max() < 1e-13 and np.abs(g["t"].cpu().numpy() - np.array(t0)).max() < 1e-13
    conds = []
    ref = pgr.optimize(gr, g["R"].cpu().numpy(), g["t"].cpu().numpy(), fine, conds=conds)
    o = {k: v.cpu().numpy() for k, v in res["optimized"].items()}
    tol = 64 * EPS * (sum(conds) + 1)
    assert np.array_equal(o["kept"], ref["kept"]) and o["iterations"].tolist() == ref["iterations"].tolist() and o["converged"] == ref["converged"]
    assert np.abs(o["R"] - ref["R"]).max() <= tol and np.abs(o["t"] - ref["t"]).max() <= tol
    assert res["R"] is res["optimized"]["R"] and torch.equal(res["kept"], res["optimized"]["kept"])
    e_opt, e_odo = pgr.pose_error(o["R"], o["t"], R_true, t_true), pgr.pose_error(np.array(R0), np.array(t0), R_true, t_true)
    pruned = [p for p, k in zip(g["pairs"], o["kept"]) if not k]
    _emit(f"register_multiway, five 700-point torus views (not asserted): pose error (rad, length) optimised {e_opt[0]:.4e} {e_opt[1]:.4e}, "
          f"chained odometry {e_odo[0]:.4e} {e_odo[1]:.4e}; pruned pairs {pruned}; fitness {np.round(g['fitness'].cpu().numpy(), 3).tolist()}; "
          f"max cond {max(conds):.3e}, |dR| {np.abs(o['R'] - ref['R']).max():.3e} (allowance {tol:.3e})")
