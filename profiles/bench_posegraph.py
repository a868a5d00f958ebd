#!/usr/bin/env python
"""Pose-graph optimisation (vcr_posegraph_optimize_f64) measured, by bench_plane.py's protocol (section
4.8's: device events around repeated blocks after a warm-up, contenders alternated block by block, the median block with the
fastest and the slowest).  Two parts, each of which can run alone (--part):

  o  the optimiser at (G, K, E) = (1, 8, 14), (16, 32, 120), (1, 128, 1000): the whole call (ITER outer iterations, thresholds
     0, no pruning, so that every contender does the same work), in both forms where the LDS form exists; one linearisation
     (max_iteration = 0) and one linearisation plus one trial, whose difference is a solve with its trial residual; and the
     yardstick, the same loop in torch device ops in fp64 -- the edge terms as batched matrix products, index_put_ into H,
     torch.linalg.cholesky and cholesky_solve on the assembled system, a host decision (.item()) a trial -- for the first
     graph of the batch alone (it has no batch form), so its time stands against the call's time divided by G.
  m  register_multiway at K = 8 clouds of 16 384 points (views of the torus, neighbours 6 degrees and 0.04 apart), split into
     pose_graph_from_clouds (28 pairs: two refinements and an information matrix each, batched) and optimize_pose_graph.

No time is asserted anywhere: the file records what was measured.

  python profiles/bench_posegraph.py [--part om] [--blocks 5] [--out profiles/posegraph_bench.txt] [--append]
"""
import argparse
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import vcrnet_amd  # noqa: E402,F401
from vcrnet_amd import build, posegraph  # noqa: E402
from bench_refine import rotation  # noqa: E402
from bench_plane import LINES, run_blocks, say, torus  # noqa: E402

SHAPES = ((1, 8, 14), (16, 32, 120), (1, 128, 1000))
ITER = 5
MCD = 0.05
ZERO = dict(min_relative_increment=0.0, min_relative_residual_increment=0.0, min_right_term=0.0, min_residual=0.0)


def euler(x):
    s0, c0, s1, c1, s2, c2 = np.sin(x[0]), np.cos(x[0]), np.sin(x[1]), np.cos(x[1]), np.sin(x[2]), np.cos(x[2])
    return np.array([[c2 * c1, c2 * s1 * s0 - s2 * c0, c2 * s1 * c0 + s2 * s0], [s2 * c1, s2 * s1 * s0 + c2 * c0, s2 * s1 * c0 - c2 * s0],
                     [-s1, c1 * s0, c1 * c0]]), np.asarray(x[3:6], np.float64)


def graph(seed, K, E):
    """A chain of K planted poses with K - 1 noisy odometry edges and E - K + 1 true closures between random nodes (a little
    noise), information matrices G^T G of 200 random points; the start is the chained odometry."""
    rs = np.random.RandomState(seed)
    Rt, tt = [np.eye(3)], [np.zeros(3)]
    for _ in range(1, K):
        Ri, ti = euler(np.concatenate([rs.uniform(-0.1, 0.1, 3), rs.uniform(-0.2, 0.2, 3) + [0.3, 0, 0]]))
        Rt.append(Ri @ Rt[-1]); tt.append(Ri @ tt[-1] + ti)
    pairs = [(i, i + 1, 0) for i in range(K - 1)]
    while len(pairs) < E:
        i, j = sorted(rs.choice(K, 2, replace=False))
        if j > i + 1:
            pairs.append((int(i), int(j), 1))
    src, dst, unc = (np.array(x, np.int32) for x in zip(*pairs))
    Re, te, info = np.empty((E, 3, 3)), np.empty((E, 3)), np.empty((E, 6, 6))
    for e, (i, j, _) in enumerate(pairs):
        Rn, tn = euler(rs.normal(0, 0.003, 6))
        Rx, tx = Rt[j].T @ Rt[i], Rt[j].T @ (tt[i] - tt[j])
        Re[e], te[e] = Rn @ Rx, Rn @ tx + tn
        q = rs.uniform(-0.5, 0.5, (200, 3))
        Gm = np.zeros((200, 3, 6))
        Gm[:, 0, 1], Gm[:, 0, 2], Gm[:, 1, 0], Gm[:, 1, 2], Gm[:, 2, 0], Gm[:, 2, 1] = q[:, 2], -q[:, 1], -q[:, 2], q[:, 0], q[:, 1], -q[:, 0]
        Gm[:, 0, 3] = Gm[:, 1, 4] = Gm[:, 2, 5] = 1
        info[e] = np.einsum("nri,nrj->ij", Gm, Gm)
    R0, t0 = [np.eye(3)], [np.zeros(3)]
    for e in range(K - 1):
        R0.append(R0[-1] @ Re[e].T); t0.append(t0[-1] - R0[-1] @ te[e])
    return np.array(R0), np.array(t0), src, dst, Re, te, info, unc


def batch(G, K, E):
    parts = [graph(100 * K + g, K, E) for g in range(G)]
    types = (torch.float64, torch.float64, torch.int32, torch.int32, torch.float64, torch.float64, torch.float64, torch.int32)
    return tuple(torch.as_tensor(np.stack([p[i] for p in parts])).to("cuda", ty) for i, ty in enumerate(types))


# ---- the yardstick: the same loop in torch device ops, one graph, a host decision a trial

def t_vec6(R, t):
    sy = torch.sqrt(R[:, 0, 0] ** 2 + R[:, 1, 0] ** 2)
    return torch.stack([torch.atan2(R[:, 2, 1], R[:, 2, 2]), torch.atan2(-R[:, 2, 0], sy), torch.atan2(R[:, 1, 0], R[:, 0, 0]), t[:, 0], t[:, 1], t[:, 2]], 1)


def t_euler(x):
    s, c = torch.sin(x[:, :3]), torch.cos(x[:, :3])
    s0, s1, s2, c0, c1, c2 = s[:, 0], s[:, 1], s[:, 2], c[:, 0], c[:, 1], c[:, 2]
    return torch.stack([c2 * c1, c2 * s1 * s0 - s2 * c0, c2 * s1 * c0 + s2 * s0, s2 * c1, s2 * s1 * s0 + c2 * c0, s2 * s1 * c0 - c2 * s0,
                        -s1, c1 * s0, c1 * c0], 1).view(-1, 3, 3), x[:, 3:]


GEN = torch.zeros(3, 3, 3, dtype=torch.float64)
for _k in range(3):
    GEN[_k, (_k + 2) % 3, (_k + 1) % 3], GEN[_k, (_k + 1) % 3, (_k + 2) % 3] = 1.0, -1.0


def t_residual(R, t, src, dst, Re, te):
    Rs, ts, Rd, td = R[src], t[src], R[dst], t[dst]
    RP = Re.transpose(1, 2) @ Rd.transpose(1, 2)
    tM = (Re.transpose(1, 2) @ (Rd.transpose(1, 2) @ (ts - td)[..., None] - te[..., None]))[..., 0]
    return t_vec6(RP @ Rs, tM), RP, Rs, ts


def t_system(R, t, src, dst, Re, te, info, unc, mu, K, gen):
    r, RP, Rs, ts = t_residual(R, t, src, dst, Re, te)
    E = src.numel()
    J = torch.zeros(E, 6, 6, dtype=torch.float64, device=R.device)
    for k in range(3):
        N = RP @ gen[k] @ Rs
        J[:, 0, k], J[:, 1, k], J[:, 2, k] = (N[:, 2, 1] - N[:, 1, 2]) / 2, (N[:, 0, 2] - N[:, 2, 0]) / 2, (N[:, 1, 0] - N[:, 0, 1]) / 2
        J[:, 3:, k] = (RP @ (gen[k] @ ts[..., None]))[..., 0]
    J[:, 3:, 3:] = RP
    q = torch.einsum("ep,epq,eq->e", r, info, r)
    s = torch.where(unc, mu / (mu + q), torch.ones_like(q))
    l = s * s
    W = l[:, None, None] * (J.transpose(1, 2) @ info @ J)
    gv = l[:, None] * torch.einsum("epk,epq,eq->ek", J, info, r)
    H = torch.zeros(K, K, 6, 6, dtype=torch.float64, device=R.device)
    H.index_put_((src, src), W, accumulate=True); H.index_put_((dst, dst), W, accumulate=True)
    H.index_put_((src, dst), -W, accumulate=True); H.index_put_((dst, src), -W, accumulate=True)
    b = torch.zeros(K, 6, dtype=torch.float64, device=R.device)
    b.index_put_((src,), -gv, accumulate=True); b.index_put_((dst,), gv, accumulate=True)
    H = H.permute(0, 2, 1, 3).reshape(6 * K, 6 * K).clone()
    b = b.reshape(-1).clone()
    H[:6], H[:, :6], b[:6] = 0.0, 0.0, 0.0
    H[:6, :6] = torch.eye(6, dtype=torch.float64, device=R.device)
    return H, b, s, (l * q + torch.where(unc, mu * (s - 1) ** 2, torch.zeros_like(q))).sum()


def torch_lm(R, t, src, dst, Re, te, info, unc, iters, lsf=1.0 / 3.0):
    src, dst, unc, K = src.long(), dst.long(), unc.bool(), R.shape[0]
    gen = GEN.to(R.device)
    mu = MCD * MCD * info[unc][:, 5, 5].mean()
    H, b, s, res = t_system(R, t, src, dst, Re, te, info, unc, mu, K, gen)
    lam, nu, trials = 1e-5 * H.diagonal().max(), 2.0, 0
    eye = torch.eye(6 * K, dtype=torch.float64, device=R.device)
    for _ in range(iters):
        for _ in range(20):
            trials += 1
            d = torch.cholesky_solve(b[:, None], torch.linalg.cholesky(H + lam * eye))[:, 0]
            Ri, ti = t_euler(d.view(K, 6))
            Rn, tn = Ri @ R, (Ri @ t[..., None])[..., 0] + ti
            r, _, _, _ = t_residual(Rn, tn, src, dst, Re, te)
            q = torch.einsum("ep,epq,eq->e", r, info, r)
            res_new = (s * s * q + torch.where(unc, mu * (s - 1) ** 2, torch.zeros_like(q))).sum()
            rho = (res - res_new) / (d @ (lam * d + b) + 1e-3)
            if rho.item() > 0:                               # the host decides: one synchronisation a trial
                R, t, res = Rn, tn, res_new
                lam, nu = lam * torch.clamp(1 - (2 * rho - 1) ** 3, min=lsf), 2.0
                H, b, s, _ = t_system(R, t, src, dst, Re, te, info, unc, mu, K, gen)
                break
            lam, nu = lam * nu, nu * 2.0
    return R, t, trials


def part_o(blocks):
    say(f"## o. the optimiser: {ITER} outer iterations, thresholds 0, prune=False; one linearisation; one trial; the torch loop on one graph")
    for G, K, E in SHAPES:
        a = batch(G, K, E)
        one = tuple(x[0] for x in a)
        plan = posegraph.posegraph_form(K, G, E)
        head = f"G={G:2d} K={K:3d} E={E:5d}"
        res = {}
        crit = dict(ZERO, max_iteration=ITER)
        call = lambda name, **kw: res.__setitem__(name, posegraph.optimize(*a, max_correspondence_distance=MCD, prune=False, want_system=True, **kw))   # noqa: E731
        contenders = [("global form", lambda: call("global form", criteria=crit, variant=posegraph.FORM_GLOBAL))]
        if plan[0] == posegraph.FORM_LDS:
            contenders.insert(0, ("LDS form", lambda: call("LDS form", criteria=crit, variant=posegraph.FORM_LDS)))
        contenders += [("one linearisation", lambda: call("lin", criteria=dict(ZERO, max_iteration=0))),
                       ("one linearisation + one trial", lambda: call("trial", criteria=dict(ZERO, max_iteration=1, max_iteration_lm=1))),
                       ("torch loop, first graph", lambda: res.__setitem__("torch", torch_lm(*one, ITER)))]
        med, times, calls = run_blocks(contenders, blocks)
        for name, _ in contenders:
            v = times[name]
            say(f"{head}  {name:30s} {med[name]:10.4f} ms/call  (blocks min {min(v):.4f} max {max(v):.4f}; {blocks} x {calls[name]} calls)")
        o = res["global form"]
        tr = o["trials"].view(-1, 2)[:, 0].tolist()
        same = "LDS form" not in res or all(torch.equal(res["LDS form"][k], o[k]) for k in ("R", "t", "weight", "residual", "iterations"))
        dR = (res["torch"][0] - o["R"].view(-1, K, 3, 3)[0]).abs().max().item()
        say(f"{head}  plan: form {plan[0]}, {plan[1]} B of LDS, workspace {plan[2]} B; trials a graph {tr[:4]}{' ...' if G > 4 else ''}, torch's {res['torch'][2]}; "
            f"converged {o['converged'].view(-1).tolist()[:4]}; both forms the same bits: {same}; |R - torch's R| {dR:.2e}")
        t_call = med["LDS form"] if "LDS form" in med else med["global form"]
        say(f"{head}  a trial (solve + trial residual) {med['one linearisation + one trial'] - med['one linearisation']:.4f} ms; the call a trial "
            f"{t_call / max(1, sum(tr) / len(tr)):.4f} ms; the call a graph {t_call / G:.4f} ms against torch's {med['torch loop, first graph']:.4f} ms "
            f"(x{med['torch loop, first graph'] / (t_call / G):.1f})")
        say()


def views(K, n, seed=4):
    rs = np.random.RandomState(seed)
    Rt, tt, out = np.eye(3), np.zeros(3), []
    for i in range(K):
        if i:
            d = rs.normal(size=3)
            Rn, tn = rotation(rs.normal(size=3), 6.0), 0.04 * d / np.linalg.norm(d)
            Rt, tt = Rt @ Rn, Rt @ tn + tt
        out.append((Rt.T @ (torus(rs, n) - tt[:, None])).astype(np.float32))
    return torch.from_numpy(np.stack(out)).cuda()


def part_m(blocks):
    K, n, coarse, fine = 8, 16384, 0.15, 0.05
    say(f"## m. register_multiway at K = {K} x {n} points (coarse {coarse}, fine {fine}, point to plane, scan): the pairwise stage and the optimiser")
    x = views(K, n)
    res = {}
    g = vcrnet_amd.pose_graph_from_clouds(x, coarse, fine)
    opt = lambda: vcrnet_amd.optimize_pose_graph(g["R"], g["t"], g["src"], g["dst"], g["R_edge"], g["t_edge"], g["information"], g["uncertain"], fine)   # noqa: E731
    contenders = [("pose_graph_from_clouds", lambda: res.__setitem__("g", vcrnet_amd.pose_graph_from_clouds(x, coarse, fine))),
                  ("optimize_pose_graph", lambda: res.__setitem__("o", opt())),
                  ("register_multiway", lambda: res.__setitem__("m", vcrnet_amd.register_multiway(x, coarse, fine)))]
    med, times, calls = run_blocks(contenders, blocks)
    for name, _ in contenders:
        v = times[name]
        say(f"K={K} N={n}  {name:24s} {med[name]:10.4f} ms/call  (blocks min {min(v):.4f} max {max(v):.4f}; {blocks} x {calls[name]} calls)")
    o = res["o"]
    say(f"K={K} N={n}  the optimiser's share of register_multiway: {100 * med['optimize_pose_graph'] / med['register_multiway']:.2f} %; "
        f"iterations {o['iterations'].tolist()}, converged {int(o['converged'])}, kept {int(o['kept'].sum())} of {o['kept'].numel()} edges, "
        f"pairwise fitness {g['fitness'].min().item():.3f} ... {g['fitness'].max().item():.3f}")
    say()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--part", default="om")
    ap.add_argument("--blocks", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "posegraph_bench.txt"))
    ap.add_argument("--append", action="store_true", help="add to --out instead of replacing it (one part per run)")
    a = ap.parse_args()
    if not a.append:
        say(f"# kernel_sources_sha16={build.sources_sha16()}")
        say(f"# profiles/bench_posegraph.py --blocks {a.blocks}: device {torch.cuda.get_device_name(0)}, "
            f"{torch.cuda.get_device_properties(0).multi_processor_count} CUs; ms per call = median of the blocks")
        say()
    if "o" in a.part:
        part_o(a.blocks)
    if "m" in a.part:
        part_m(a.blocks)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "a" if a.append else "w") as fh:
        fh.write("\n".join(LINES) + "\n")


if __name__ == "__main__":
    main()
