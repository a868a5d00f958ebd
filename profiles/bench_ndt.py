#!/usr/bin/env python
"""The Normal Distributions Transform on the device (include/ndt/vcr_hip_ndt.h), by bench_nnscore.py's
protocol as bench_plane.py runs it: ms per call from device events around `--blocks` repeated blocks of calls after a warm-up,
contenders alternated block by block; the median block, the fastest and the slowest.

a. At B x N = 16 x 1024, 16 x 16 384 and 1 x 131 072 points (source and target two samplings of one cloud, the start pose 0.03 rad
   and 0.02 off), at edges aimed at 8 and 64 points a voxel (every row says what came out), on uniform cubes and on surfaces: the map build, one derivative round
   on a built map (the plan's form and the forced lane-a-point form, which is the one form built: the same kernel), the whole call
   on a built map (max_iterations 30); beside them a grid point-to-plane refine_registration of one round and of thirty on the
   same clouds and start (normals given, max_dist = two voxel edges), and the same derivative sums in torch device ops from the
   device's own voxel assignment.
b. The ledger: the restated loop's and the device loop's error on the tests' recovery recipe, the largest ratio of a device sum's
   difference to 2^-52 times its absolute terms over the tests' cases, and the pose error after NDT and after grid point-to-plane
   from five start offsets on the recipe's surfaces.

  python profiles/bench_ndt.py [--blocks 3] [--out profiles/ndt_bench.txt] [--ledger profiles/ndt_ledger.txt]
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
from vcrnet_amd import build, ndt  # noqa: E402
from bench_plane import LINES, NORMALS_SHAPES as SHAPES, run_blocks, say  # noqa: E402
import ndt_restated as nd  # noqa: E402

F32 = np.float32
OFFSETS = ((0.05, 0.03), (0.1, 0.05), (0.2, 0.1), (0.4, 0.2), (0.8, 0.4))


def clouds(kind, B, N, seed):
    """(src, tgt) [B,3,N] device tensors: two samplings of one cloud, the source moved 0.03 rad and 0.02 off."""
    out = []
    for which in (0, 1):
        xs = []
        for b in range(B):
            s = seed + 2 * b + which
            xs.append(nd.torus(s, N, noise=0.005) if kind == "surface" else np.random.RandomState(s).uniform(-1, 1, (3, N)).astype(F32))
        out.append(np.stack(xs))
    Rg, tg = nd.pose(0.03, 0.02, seed)
    src = np.stack([(Rg.T @ (x.astype(np.float64) - tg[:, None])).astype(F32) for x in out[0]])
    return torch.from_numpy(src).cuda(), torch.from_numpy(out[1]).cuda()


def edge(kind, N, per_voxel):
    """The voxel edge at which the cloud holds about per_voxel points a voxel: a cube of volume 8, a surface of area about 12."""
    return float(F32((8.0 * per_voxel / N) ** (1 / 3.0) if kind == "uniform" else (12.0 * per_voxel / N) ** 0.5))


def torch_sums(src, m, voxel, d2):
    """The contender: f, g, H of the identity pose in torch device ops from the device's voxel assignment [B,Ns,7]."""
    B, _, Ns = src.shape
    at = voxel >= 0
    b, n, _ = at.nonzero(as_tuple=True)
    v = voxel[at].long()
    P = src.double()[b, :, n]
    mu = m.mean[b, :, v]
    a = m.inv_cov[b, :, v]
    A = torch.stack([a[:, 0], a[:, 1], a[:, 2], a[:, 1], a[:, 3], a[:, 4], a[:, 2], a[:, 4], a[:, 5]], 1).view(-1, 3, 3)
    r = P - mu
    Ar = torch.einsum("nij,nj->ni", A, r)
    e = torch.exp(-0.5 * d2 * (r * Ar).sum(1))
    zero = torch.zeros_like(P[:, 0])
    J = torch.stack([torch.stack([zero, -P[:, 2], P[:, 1]], 1), torch.stack([P[:, 2], zero, -P[:, 0]], 1),
                     torch.stack([-P[:, 1], P[:, 0], zero], 1)], 2)
    J = torch.cat([J, torch.eye(3, dtype=P.dtype, device=P.device).expand(len(P), 3, 3)], 2)         # [n,3,6]
    u = torch.einsum("ni,nia->na", Ar, J)
    w = d2 * e
    H = torch.einsum("nia,nij,njb->nab", J, A, J) - d2 * u[:, :, None] * u[:, None, :]
    S = torch.zeros_like(H)
    S[:, :3, :3] = Ar[:, :, None] * P[:, None, :]
    S[:, :3, :3] = torch.triu(S[:, :3, :3]) + torch.triu(S[:, :3, :3], 1).transpose(1, 2)
    S[:, :3, :3] -= torch.eye(3, dtype=P.dtype, device=P.device) * (Ar * P).sum(1)[:, None, None]
    H = (H + S) * w[:, None, None]
    f = torch.zeros(B, dtype=P.dtype, device=P.device).index_add_(0, b, -e)
    g = torch.zeros(B, 6, dtype=P.dtype, device=P.device).index_add_(0, b, w[:, None] * u)
    return f, g, torch.zeros(B, 6, 6, dtype=P.dtype, device=P.device).index_add_(0, b, H)


def part_a(blocks):
    say("## a. ms per call; map = ndt_map, round = ndt_derivatives on a built map, call = refine_registration_ndt(map=, 30 iterations)")
    for kind in ("uniform", "surface"):
        for B, N in SHAPES:
            for per_voxel in (8, 64):
                h = edge(kind, N, per_voxel)
                src, tgt = clouds(kind, B, N, 7 + N)
                m = ndt.ndt_map(tgt, h)
                normals = vcrnet_amd.estimate_normals(tgt, 20)
                eye, zero = torch.eye(3, device="cuda").repeat(B, 1, 1), torch.zeros(B, 3, device="cuda")
                d = ndt.ndt_derivatives(src, m, want_stages=True)
                _, d2 = ndt.constants(0.55, h)
                res = {}
                plane = dict(max_dist=2 * h, method="point_to_plane", tgt_normals=normals, search="grid")
                contenders = [
                    ("map", lambda: ndt.ndt_map(tgt, h)),
                    ("round (plan)", lambda: ndt.ndt_derivatives(src, m)),
                    ("round (variant 1)", lambda: ndt.ndt_derivatives(src, m, variant=1)),
                    ("call", lambda: res.__setitem__("ndt", ndt.refine_registration_ndt(src, None, map=m))),
                    ("plane, 1 round", lambda: vcrnet_amd.refine_registration(src, tgt, eye, zero, max_iterations=1, **plane)),
                    ("plane, call", lambda: res.__setitem__("plane", vcrnet_amd.refine_registration(src, tgt, eye, zero, **plane))),
                    ("torch sums", lambda: res.__setitem__("torch", torch_sums(src, m, d["voxel"], d2))),
                ]
                med, times, calls = run_blocks(contenders, blocks)
                V, ok = int(m.count.clamp(min=0).sum()), int(m.valid.sum())
                say(f"{kind} {B} x {N}, h {h:.4f}: {V / B:.0f} voxels a cloud ({N * B / max(V, 1):.1f} points each), {ok / B:.0f} valid; "
                    f"hits {d['hits'].float().mean().item():.0f}; ndt iterations {res['ndt']['iterations'].float().mean().item():.1f} "
                    f"trials {res['ndt']['trials'].float().mean().item():.1f}; plane iterations {res['plane']['iterations'].float().mean().item():.1f}")
                for name, _ in contenders:
                    say(f"    {name:18s} {med[name]:9.4f} ms  (fastest {min(times[name]):.4f}, slowest {max(times[name]):.4f}, {calls[name]} calls a block)")
                tf, tg, _ = res["torch"]
                say(f"    torch against the call's sums: |f| {float((tf - d['score']).abs().max()):.3g} of {float(d['score'].abs().max()):.3g}, "
                    f"|g| {float((tg - d['g']).abs().max()):.3g} of {float(d['g'].abs().max()):.3g}")
                say(f"    round / plane round x{med['round (plan)'] / med['plane, 1 round']:.2f}; call / plane call x{med['call'] / med['plane, call']:.2f}; "
                    f"round / torch sums x{med['round (plan)'] / med['torch sums']:.3f}")
            say()


def ledger(path):
    import test_hip_ndt as th
    out = [f"# kernel_sources_sha16={build.sources_sha16()}",
           "# profiles/bench_ndt.py: the recovery recipe of tests/ndt_restated.py (700 target and 500 source points of one surface, h = 0.3)"]

    def note(line):
        print(line, flush=True)
        out.append(line)
    for i, (angle, shift) in enumerate(nd.RECOVERY):
        src, tgt, R0, t0, Rg, tg = nd.recovery_case(i)
        o = nd.ndt(src, nd.ndt_map(tgt, nd.RECOVERY_H), R0, t0)
        ea, es = nd.pose_error(o["R"], o["t"], Rg, tg)
        note(f"restated recovery {i} from ({angle:g} rad, {shift:g}): iterations {o['iterations']} trials {o['trials']} status "
             f"{nd.STATUS[o['status']]} angle {ea:.6e} shift {es:.6e}")
        o = ndt.refine_registration_ndt(torch.from_numpy(src[None]).cuda(), torch.from_numpy(tgt[None]).cuda(), resolution=nd.RECOVERY_H)
        ea, es = nd.pose_error(o["R"][0].cpu().numpy(), o["t"][0].cpu().numpy(), Rg, tg)
        note(f"device recovery {i} from ({angle:g} rad, {shift:g}): iterations {int(o['iterations'][0])} trials {int(o['trials'][0])} status "
             f"{nd.STATUS[int(o['status'][0])]} angle {ea:.6e} shift {es:.6e}")
    note("")
    tgt, h, maps = th.scene()
    m = th.scene_map()
    worst = 0.0
    for Ns in th.SCAN_SIZES:
        src = np.stack([nd.torus(50 + Ns, Ns, noise=0.01), nd.torus(51 + Ns, Ns, noise=0.01)])
        for kind in ("all", "some", "none"):
            R, t = th.poses(kind)
            o = th.derive(src, m, R, t)
            for b in range(2):
                worst = max(worst, th.ratios(o, nd.derivatives(src[b], maps[b], R[b], t[b]), b))
    note(f"largest |device sum - restated sum| / (2^-52 sum |term|) over tests/test_hip_ndt.py's derivative cases: {worst:.3f} "
         f"(the test's K_MEASURED is {th.K_MEASURED}; it allows {th.K_ALLOWED:.3f})")
    note("")
    note("## pose error (angle rad, shift) after refine_registration_ndt (h 0.3) and after grid point-to-plane (max_dist 0.6, normals k 20), 30 iterations")
    tgt = nd.torus(11, 700)
    T = torch.from_numpy(tgt[None]).cuda()
    normals = vcrnet_amd.estimate_normals(T, 20)
    for angle, shift in OFFSETS:
        row = []
        for seed in range(4):
            Rg, tg = nd.pose(angle, shift, seed=10 + seed)
            src = (Rg.T @ (nd.torus(12, 500).astype(np.float64) - tg[:, None])).astype(F32)
            S = torch.from_numpy(src[None]).cuda()
            a = ndt.refine_registration_ndt(S, T, resolution=nd.RECOVERY_H)
            p = vcrnet_amd.refine_registration(S, T, None, None, 0.6, method="point_to_plane", tgt_normals=normals, search="grid")
            row.append(nd.pose_error(a["R"][0].cpu().numpy(), a["t"][0].cpu().numpy(), Rg, tg)
                       + nd.pose_error(p["R"][0].cpu().numpy(), p["t"][0].cpu().numpy(), Rg, tg))
        note(f"from ({angle:g} rad, {shift:g}): " + "; ".join(f"ndt {r[0]:.2e} {r[1]:.2e} plane {r[2]:.2e} {r[3]:.2e}" for r in row)
             + f"   ndt nearer in {sum(r[0] < r[2] for r in row)}/4 (angle) {sum(r[1] < r[3] for r in row)}/4 (shift)")
    with open(path, "w") as fh:
        fh.write("\n".join(out) + "\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--blocks", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ndt_bench.txt"))
    ap.add_argument("--ledger", default=os.path.join(ROOT, "profiles", "ndt_ledger.txt"))
    a = ap.parse_args()
    ledger(a.ledger)
    say(f"# kernel_sources_sha16={build.sources_sha16()}")
    say(f"# profiles/bench_ndt.py --blocks {a.blocks}: device {torch.cuda.get_device_name(0)}, "
        f"{torch.cuda.get_device_properties(0).multi_processor_count} CUs; ms per call = median of the blocks")
    say()
    part_a(a.blocks)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        fh.write("\n".join(LINES) + "\n")


if __name__ == "__main__":
    main()
