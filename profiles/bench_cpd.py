#!/usr/bin/env python
"""Rigid Coherent Point Drift on the device (include/cpd/vcr_hip_cpd.h), by bench_nnscore.py's protocol
as bench_plane.py runs it: ms per call from device events around `--blocks` repeated blocks of calls after a warm-up, contenders
alternated block by block; the median block, the fastest and the slowest.

a. At B x N = 16 x 1024, 16 x 16 384 and 1 x 131 072 points a side (two samplings of one surface, 0.3 rad and 0.1 apart,
   sigma2 = 0.01): one E-step (cpd_expectation) by the plan and by every forced form, with pairs/s; the share of the two streamed
   passes in it (kernel times from torch.profiler); the loop at 30 updates; the same E-step and M-step in torch device ops
   (chunked cdist -> exp -> sum / matmul, torch.linalg.svd); one round of grid point-to-plane refine_registration beside them.
b. The ledger: the tests' measured tolerances, the basin of the torus recipe for CPD, CPD then point-to-plane, point-to-plane
   and NDT, target-side clutter against w, and what the fp32 weights cost against a dense fp64 CPD.

  python profiles/bench_cpd.py [--blocks 3] [--out profiles/cpd_bench.txt] [--ledger profiles/cpd_ledger.txt] [--skip-bench]
"""
import argparse
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))                # the recipes of the tests
import vcrnet_amd  # noqa: E402
from vcrnet_amd import build, cpd  # noqa: E402
from bench_plane import LINES, NORMALS_SHAPES as SHAPES, run_blocks, say  # noqa: E402
import cpd_restated as cr  # noqa: E402

F32 = np.float32
SIGMA2, W = 0.01, 0.1
FORM_NAMES = ("plan", "LDS x1", "LDS x2", "LDS x4", "scalar x1", "scalar x2", "scalar x4")   # operand x points a lane


def clouds(B, N, seed):
    """(src, tgt) [B,3,N] device tensors: two samplings of one surface, the source 0.3 rad and 0.1 off."""
    Rg, tg = cr.pose(0.3, 0.1, seed)
    src = np.stack([(Rg.T @ (cr.torus(seed + 2 * b, N, noise=0.005).astype(np.float64) - tg[:, None])).astype(F32) for b in range(B)])
    tgt = np.stack([cr.torus(seed + 2 * b + 1, N, noise=0.005) for b in range(B)])
    return torch.from_numpy(src).cuda(), torch.from_numpy(tgt).cuda()


def torch_round(src, tgt, sigma2, w):
    """The contender: one E-step and one M-step of rigid CPD from the identity in torch device ops, fp32 weights in chunks of
    source rows, fp64 update."""
    B, _, M = src.shape
    N = tgt.shape[2]
    Y, X = src.transpose(1, 2).contiguous(), tgt.transpose(1, 2).contiguous()       # [B,M,3], [B,N,3]
    c = (2 * np.pi * sigma2) ** 1.5 * w / (1 - w) * M / N
    rows = max(1, min(M, (1 << 26) // (N * B)))
    S = torch.zeros(B, N, device=src.device)
    for m0 in range(0, M, rows):
        S += torch.exp(torch.cdist(Y[:, m0:m0 + rows], X) ** 2 * (-0.5 / sigma2)).sum(1)
    inv = 1.0 / (S + c)
    P1 = torch.empty(B, M, device=src.device)
    PX = torch.empty(B, M, 3, device=src.device)
    for m0 in range(0, M, rows):
        p = torch.exp(torch.cdist(Y[:, m0:m0 + rows], X) ** 2 * (-0.5 / sigma2)) * inv[:, None, :]
        P1[:, m0:m0 + rows] = p.sum(2)
        PX[:, m0:m0 + rows] = p @ X
    Pt1, P1, PX, Yd, Xd = (S * inv).double(), P1.double(), PX.double(), Y.double(), X.double()
    Np = P1.sum(1)
    mux, muy = PX.sum(1) / Np[:, None], (P1[:, :, None] * Yd).sum(1) / Np[:, None]
    Yh = Yd - muy[:, None, :]
    A = (PX - P1[:, :, None] * mux[:, None, :]).transpose(1, 2) @ Yh
    U, _, Vt = torch.linalg.svd(A)
    d = torch.det(U @ Vt)
    C = torch.diag_embed(torch.stack([torch.ones_like(d), torch.ones_like(d), d], 1))
    R = U @ C @ Vt
    trAR = (A * R).sum((1, 2))
    t = mux - (R @ muy[:, :, None])[:, :, 0]
    xPx = (Pt1 * ((Xd - mux[:, None, :]) ** 2).sum(2)).sum(1)
    yPy = (P1 * (Yh ** 2).sum(2)).sum(1)
    return R, t, (xPx - 2 * trAR + yPy) / (3 * Np), P1, PX


def pass_share(src, tgt):
    """The share of the two streamed passes in one E-step's kernel time, from torch.profiler's device durations."""
    try:
        from torch.profiler import ProfilerActivity, profile
        cpd.cpd_expectation(src, tgt, SIGMA2, w=W)
        torch.cuda.synchronize()
        with profile(activities=[ProfilerActivity.CUDA, ProfilerActivity.CPU]) as prof:
            for _ in range(3):
                cpd.cpd_expectation(src, tgt, SIGMA2, w=W)
            torch.cuda.synchronize()
        mine = [(e.key, getattr(e, "device_time_total", None) or getattr(e, "cuda_time_total", 0.0)) for e in prof.key_averages() if "cpd_" in e.key]
        total = sum(t for _, t in mine)
        passes = sum(t for k, t in mine if "cpd_pass_kernel" in k)
        return f"{100 * passes / total:.1f} % of the call's kernel time ({passes / 3e3:.4f} of {total / 3e3:.4f} ms a call)" if total else "no kernel times came back"
    except Exception as e:                                     # noqa: BLE001  (the figure is a report, not a gate)
        return f"not measured ({type(e).__name__}: {e})"


def part_a(blocks):
    say(f"## a. ms per call; E-step = cpd_expectation(sigma2 = {SIGMA2}, w = {W}); loop = coherent_point_drift(max_iterations = 30, tolerance = 0)")
    for B, N in SHAPES:
        src, tgt = clouds(B, N, 7 + N)
        normals = vcrnet_amd.estimate_normals(tgt, 20)
        eye, zero = torch.eye(3, device="cuda").repeat(B, 1, 1), torch.zeros(B, 3, device="cuda")
        res = {}
        contenders = [(f"E-step ({FORM_NAMES[v]})", (lambda v=v: cpd.cpd_expectation(src, tgt, SIGMA2, w=W, variant=v))) for v in range(cpd.FORMS + 1)]
        contenders += [
            ("loop, 30 updates", lambda: res.__setitem__("cpd", cpd.coherent_point_drift(src, tgt, w=W, max_iterations=30, tolerance=0.0))),
            ("torch round", lambda: res.__setitem__("torch", torch_round(src, tgt, SIGMA2, W))),
            ("plane, 1 round", lambda: vcrnet_amd.refine_registration(src, tgt, eye, zero, max_iterations=1, max_dist=0.3, method="point_to_plane",
                                                                      tgt_normals=normals, search="grid")),
        ]
        med, times, calls = run_blocks(contenders, blocks)
        form, s1, s2, ws = cpd.cpd_form(B, N, N, loop=False, cu_count=0)
        say(f"{B} x {N} a side: the plan takes form {form} ({FORM_NAMES[form]}), pass 1 dealt to {s1} and pass 2 to {s2} workgroups a block of points; "
            f"workspace {ws / 2 ** 20:.1f} MiB; loop iterations {res['cpd']['iterations'].float().mean().item():.1f}")
        pairs = float(B) * N * N
        for name, _ in contenders:
            extra = f"  {pairs / med[name] / 1e6:8.1f} G pairs/s" if name.startswith("E-step") else ""
            say(f"    {name:20s} {med[name]:10.4f} ms  (fastest {min(times[name]):.4f}, slowest {max(times[name]):.4f}, {calls[name]} calls a block){extra}")
        best = min(range(1, cpd.FORMS + 1), key=lambda v: med[f"E-step ({FORM_NAMES[v]})"])
        say(f"    the passes: {pass_share(src, tgt)}")
        say(f"    fastest forced form: {FORM_NAMES[best]}; plan / fastest x{med['E-step (plan)'] / med[f'E-step ({FORM_NAMES[best]})']:.3f}; "
            + "; ".join(f"plan / {FORM_NAMES[v]} x{med['E-step (plan)'] / med[f'E-step ({FORM_NAMES[v]})']:.3f}" for v in range(1, cpd.FORMS + 1)))
        e = cpd.cpd_expectation(src, tgt, SIGMA2, w=W)
        P1t, PXt = res["torch"][3], res["torch"][4]
        say(f"    loop / 31 E-steps x{med['loop, 30 updates'] / (31 * med['E-step (plan)']):.3f}; E-step / torch round x{med['E-step (plan)'] / med['torch round']:.4f}; "
            f"E-step / plane round x{med['E-step (plan)'] / med['plane, 1 round']:.2f}; against torch: |P1| {float((e.P1 - P1t).abs().max()):.2e} of "
            f"{float(P1t.abs().max()):.2e}, |PX| {float((e.PX.transpose(1, 2) - PXt).abs().max()):.2e} of {float(PXt.abs().max()):.2e}")
        say()


def to_dev(x):
    return torch.from_numpy(np.ascontiguousarray(x)).cuda()


def errors(o, Rg, tg, b=0):
    return cr.pose_error(o["R"][b].cpu().numpy(), o["t"][b].cpu().numpy(), Rg, tg)


def expect(src, tgt, sigma2, R, t, scale, w):
    """numpy in, numpy out, with the staged weights; sigma2 and scale one per cloud."""
    res = cpd.cpd_expectation(to_dev(src), to_dev(tgt), to_dev(np.asarray(sigma2, np.float64)), to_dev(R), to_dev(t),
                              to_dev(np.asarray(scale, np.float64)), w, want_e=True)
    return {k: v.cpu().numpy() for k, v in res._asdict().items()}


def ledger(path):
    from vcrnet_amd import ndt
    out = [f"# kernel_sources_sha16={build.sources_sha16()}",
           "# profiles/bench_cpd.py: the recipe of tests/cpd_restated.py (torus(11, 700) as target, torus(12, 500) as source, w = 0.1, tolerance 1e-4)"]

    def note(line=""):
        print(line, flush=True)
        out.append(line)
    # the measured tolerances of tests/test_hip_cpd.py, over the cases it stages e for
    worst = {}
    for M, N in cr.TILE_SHAPES:
        src, tgt, R, t, scale, sigma2 = cr.clouds(M, N, 100 + M + N)
        o = expect(src, tgt, sigma2, R, t, scale, 0.1)
        worst["tile"] = max(worst.get("tile", 0.0), max(cr.exp2_ratio(o, src, tgt, R, t, scale, sigma2, 0.1, b) for b in range(3)))
    for M, N in cr.SEGMENT_SHAPES:
        src, tgt, R, t, scale, sigma2 = (x[:1] for x in cr.clouds(M, N, 300 + M + N))
        o = expect(src, tgt, sigma2, R, t, scale, 0.1)
        worst["segment"] = max(worst.get("segment", 0.0), cr.exp2_ratio(o, src, tgt, R, t, scale, sigma2, 0.1, 0))
    src, tgt, R, t, scale, sigma2 = cr.clouds(300, 257, 7)
    sigma2 = np.array([0.01, 0.01, 0.01])
    tgt[:, :, 100] += F32(100.0 * 0.1 * 3.0)
    o = expect(src, tgt, sigma2, R, t, scale, 0.0)
    worst["w = 0"] = max(cr.exp2_ratio(o, src, tgt, R, t, scale, sigma2, 0.0, b) for b in range(3))
    note("largest |device output - restated output| / (2^-24 sum |term|), numpy's exp2 where e >= 2^-100, over the cases of tests/test_hip_cpd.py "
         "that stage e: " + ", ".join(f"{k} {v:.3f}" for k, v in worst.items()) + f"; K_MEASURED = {max(worst.values()):.3f}")
    cases = [cr.recipe(a, cr.SHIFT, s) for a in cr.ANGLES for s in cr.SEEDS]
    src, tgt = np.stack([c[0] for c in cases]), np.stack([c[1] for c in cases])
    o = cpd.coherent_point_drift(to_dev(src), to_dev(tgt), w=0.1, tolerance=1e-4, max_iterations=150, want_trace=True)
    o = {k: v.cpu().numpy() for k, v in o.items()}
    r = cr.cpd(src[0], tgt[0], w=0.1, tolerance=1e-4, max_iterations=150)
    d_trace = float(np.max(np.abs(o["trace"][0][:6] - r["trace"][:6]) / r["trace"][:6]))
    d_pose = max(float(np.abs(o["R"][0].astype(np.float64) - r["R"]).max()), float(np.abs(o["t"][0].astype(np.float64) - r["t"]).max()),
                 abs(float(o["scale"][0]) - r["scale"]))
    note(f"restated loop against the device's on the recipe from 0.8 rad, seed 0: sigma2 over the first five updates {d_trace:.3e} relative "
         f"(TRACE_MEASURED), R, t, s at the end {d_pose:.3e} (POSE_MEASURED), iterations {int(o['iterations'][0])} against {r['iterations']} (COUNT_MEASURED "
         f"{abs(int(o['iterations'][0]) - r['iterations'])})")
    for b, (_, _, Rg, tg) in enumerate(cases):
        ea, es = cr.pose_error(o["R"][b], o["t"][b], Rg, tg)
        note(f"device recipe {b} ({cr.ANGLES[b // 3]} rad, seed {cr.SEEDS[b % 3]}): status {cr.STATUS[o['status'][b]]} iterations {o['iterations'][b]} "
             f"angle {ea:.4e} shift {es:.4e} sigma2 {o['sigma2'][b]:.4e}")
    note()
    note("## basin: pose error (angle rad, shift) from the recipe's surfaces, shift 0.3, seeds 0 ... 3; cpd = coherent_point_drift(w 0.1, 150 updates at most),")
    note("## cpd+plane = grid point-to-plane (max_dist 0.3, normals k 20, 30 iterations) from CPD's pose, plane = the same from the identity, ndt = h 0.3")
    T = to_dev(cr.torus(11, 700)[None])
    normals = vcrnet_amd.estimate_normals(T, 20)
    plane = dict(method="point_to_plane", tgt_normals=normals, search="grid")
    for angle in (0.4, 0.8, 1.2, 1.6, 2.0):
        rows = []
        for seed in range(4):
            s_, _, Rg, tg = cr.recipe(angle, 0.3, seed)
            S = to_dev(s_[None])
            c = cpd.coherent_point_drift(S, T, w=0.1, max_iterations=150)
            cp = vcrnet_amd.refine_registration(S, T, c["R"], c["t"], 0.3, **plane)
            p = vcrnet_amd.refine_registration(S, T, None, None, 0.3, **plane)
            n = ndt.refine_registration_ndt(S, T, resolution=0.3)
            rows.append(errors(c, Rg, tg) + errors(cp, Rg, tg) + errors(p, Rg, tg) + errors(n, Rg, tg) + (int(c["iterations"][0]),))
        note(f"from {angle:g} rad: " + "; ".join(f"cpd {r[0]:.1e} {r[1]:.1e} ({r[8]} it) cpd+plane {r[2]:.1e} {r[3]:.1e} plane {r[4]:.1e} {r[5]:.1e} ndt {r[6]:.1e} {r[7]:.1e}"
                                                 for r in rows))
        note(f"    within (0.07 rad, 0.02): cpd {sum(r[0] <= 7e-2 and r[1] <= 2e-2 for r in rows)}/4; within (0.01, 0.005): cpd+plane "
             f"{sum(r[2] <= 1e-2 and r[3] <= 5e-3 for r in rows)}/4, plane {sum(r[4] <= 1e-2 and r[5] <= 5e-3 for r in rows)}/4, ndt {sum(r[6] <= 1e-2 and r[7] <= 5e-3 for r in rows)}/4")
    note()
    note("## target-side clutter: 140 uniform points of the bounding box added to the 700 target points (20 %), from 0.8 rad, seeds 0 ... 3")
    for w in (0.0, 0.1, 0.3):
        rows = []
        for seed in range(4):
            s_, t_, Rg, tg = cr.recipe(0.8, 0.3, seed)
            rs = np.random.RandomState(500 + seed)
            lo, hi = t_.min(1, keepdims=True), t_.max(1, keepdims=True)
            noisy = np.concatenate([t_, (lo + (hi - lo) * rs.uniform(0, 1, (3, 140))).astype(F32)], axis=1)
            c = cpd.coherent_point_drift(to_dev(s_[None]), to_dev(noisy[None]), w=w, max_iterations=150)
            rows.append(errors(c, Rg, tg) + (cr.STATUS[int(c["status"][0])], int(c["iterations"][0])))
        note(f"w {w:g}: " + "; ".join(f"{r[0]:.2e} {r[1]:.2e} ({r[2]}, {r[3]} it)" for r in rows))
    note()
    note("## precision: the device's loop (fp32 weights) against a dense fp64 CPD (tests/cpd_restated.py's dense_cpd_round) on the recipe")
    for b in (0, 4):
        s_, t_, Rg, tg = cases[b]
        Y, X = s_.astype(np.float64), t_.astype(np.float64)
        R, t, s, s2 = np.eye(3), np.zeros(3), 1.0, float(((X[:, None, :] - Y[:, :, None]) ** 2).sum() / (3 * 500 * 700))
        it = 0
        while it < 150:
            R, t, s, new = cr.dense_cpd_round(Y, X, R, t, s, s2, 0.1)
            it += 1
            done = abs(new - s2) <= 1e-4 * s2
            s2 = new
            if done:
                break
        ea, es = cr.pose_error(R, t, Rg, tg)
        da, ds = cr.pose_error(o["R"][b], o["t"][b], Rg, tg)
        note(f"recipe {b}: fp64 iterations {it} sigma2 {s2:.6e} angle {ea:.4e} shift {es:.4e}; device iterations {o['iterations'][b]} sigma2 {o['sigma2'][b]:.6e} "
             f"angle {da:.4e} shift {ds:.4e}; |R - R64| {np.abs(o['R'][b] - R).max():.2e} |t - t64| {np.abs(o['t'][b] - t).max():.2e}")
    with open(path, "w") as fh:
        fh.write("\n".join(out) + "\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--blocks", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "cpd_bench.txt"))
    ap.add_argument("--ledger", default=os.path.join(ROOT, "profiles", "cpd_ledger.txt"))
    ap.add_argument("--skip-bench", action="store_true")
    ap.add_argument("--skip-ledger", action="store_true")
    a = ap.parse_args()
    if not a.skip_ledger:
        ledger(a.ledger)
    if a.skip_bench:
        return
    say(f"# kernel_sources_sha16={build.sources_sha16()}")
    say(f"# profiles/bench_cpd.py --blocks {a.blocks}: device {torch.cuda.get_device_name(0)}, "
        f"{torch.cuda.get_device_properties(0).multi_processor_count} CUs; ms per call = median of the blocks")
    say()
    part_a(a.blocks)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        fh.write("\n".join(LINES) + "\n")


if __name__ == "__main__":
    main()
