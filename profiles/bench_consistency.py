#!/usr/bin/env python
"""Pairwise-consistency voting on the device (vcr_consistency_f32), by bench_nnscore.py's protocol as
bench_plane.py runs it: ms per call from device events around `--blocks` repeated blocks of calls after a warm-up, contenders
alternated block by block, each contender run once untimed before its block; the median block, the fastest and the slowest.

a. The call and its passes at B x M = 16 x 1024, 16 x 16 384 and 1 x 131 072 pairs (every source point has a partner, 5 % of
   them the right one, the rest uniform; keep = 1024, seeds = 64, tau = max_dist = 0.01): the whole call, the call stopped behind
   the degree pass and behind the kept pairs (the passes are the differences), every form of the degree pass (1, 2, 4 pairs per
   lane at the plan's splits for each, with and without the pre-test on the raw square roots), ransac_correspondences at its
   default 100 000 trials and fast_global_registration on the same correspondences, and the same stages in torch device ops: chunked `cdist` on both sides, compare, `sum`, `topk`, the
   kept pairs' boolean matrix and its product -- with the share of identical degrees and of identical kept pairs.
b. The ledger: tests/match_restated.py's `planted` (M = 4000) at shares 0.20, 0.05, 0.02 and 0.01 and its `surface` recipe (600
   points) with estimated and with oriented normals, eight seeds each: how many end within 1 degree and 1e-2 of the planted pose,
   for the three global methods (no refinement).

  python profiles/bench_consistency.py [--blocks 3] [--out profiles/consistency_bench.txt] [--ledger profiles/consistency_ledger.txt]
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
from vcrnet_amd import build, consistency  # noqa: E402
from bench_plane import LINES, NORMALS_SHAPES as SHAPES, run_blocks, say  # noqa: E402
import match_restated as mr  # noqa: E402

TAU, KEEP, SEEDS, SHARE = 0.01, 1024, 64, 0.05
LEDGER_M, LEDGER_KEEP, LEDGER_SEEDS = 4000, 512, 32


def planted_batch(B, M, share, seed):
    """B clouds of M pairs on the device: src uniform in the unit cube, the right partners under one pose per cloud, the others
    uniform in [-1, 2]^3, the target shuffled."""
    rs = np.random.RandomState(seed)
    src = rs.uniform(0, 1, (B, 3, M)).astype(np.float32)
    tgt = np.empty((B, 3, M), np.float32)
    corr = np.empty((B, M), np.int32)
    for b in range(B):
        A = mr.rr.rotation(rs.normal(size=3), 65.0)
        t = rs.uniform(-0.5, 0.5, 3)
        good = rs.uniform(size=M) < share
        partner = np.where(good[None], A @ src[b].astype(np.float64) + t[:, None], rs.uniform(-1, 2, (3, M))).astype(np.float32)
        perm = rs.permutation(M)
        tgt[b][:, perm] = partner
        corr[b] = perm
    return torch.from_numpy(src).cuda(), torch.from_numpy(tgt).cuda(), torch.from_numpy(corr).cuda()


def torch_stages(src, tgt, corr, keep, seeds):
    """The contender: (deg [B,M], kept [B,keep], w [B,seeds,keep]) by chunked cdist, compare, sum, topk and a matrix product."""
    B, _, M = src.shape
    P = src.transpose(1, 2).contiguous()
    Q = torch.gather(tgt, 2, corr.long()[:, None, :].expand(B, 3, M)).transpose(1, 2).contiguous()
    step = max(1, min(M, (1 << 27) // (B * M)))
    deg = torch.cat([((torch.cdist(P[:, i:i + step], P) - torch.cdist(Q[:, i:i + step], Q)).abs() <= TAU).sum(2)
                     for i in range(0, M, step)], 1) - 1     # (a pair agrees with itself)
    k = min(keep, M)
    kept = torch.topk(deg, k, dim=1).indices
    Pk = torch.gather(P, 1, kept[:, :, None].expand(B, k, 3))
    Qk = torch.gather(Q, 1, kept[:, :, None].expand(B, k, 3))
    adj = ((torch.cdist(Pk, Pk) - torch.cdist(Qk, Qk)).abs() <= TAU) & ~torch.eye(k, dtype=torch.bool, device=src.device)
    a = adj.float()
    w = torch.where(adj[:, :seeds], a[:, :seeds] @ a.transpose(1, 2), torch.zeros((), device=src.device))
    return deg, kept, w


def part_a(blocks):
    say(f"## a. the call and its passes: keep {KEEP}, seeds {SEEDS}, tau = max_dist = {TAU}, {int(100 * SHARE)} % right pairs")
    for B, M in SHAPES:
        src, tgt, corr = planted_batch(B, M, SHARE, 11 + M)
        res = {}
        kw = dict(keep=KEEP, seeds=SEEDS)
        plan = consistency.consistency_form(B, M, M, KEEP, SEEDS, 0)[:2]
        forms = {q: consistency.consistency_form(B, M, M, KEEP, SEEDS, 0, consistency.variant(q, 0))[:2] for q in consistency.PAIRS_PER_LANE}
        planned = consistency.consistency_form(B, M, M, KEEP, SEEDS, 0, want_pretest=True)[3]
        name_of = lambda q, pre: f"  degrees, forced Q={q} S={forms[q][1]} {'pre-test' if pre else 'plain'}"   # noqa: E731
        contenders = [("vcr_consistency_f32 (plan)", lambda: res.__setitem__("hip", consistency.consistency(src, tgt, corr, TAU, want_stages=True, **kw))),
                      ("  behind the degrees", lambda: consistency.consistency(src, tgt, corr, TAU, stop_after=1, **kw)),
                      ("  behind the kept pairs", lambda: consistency.consistency(src, tgt, corr, TAU, stop_after=2, **kw))]
        contenders += [(name_of(q, pre), lambda q=q, pre=pre: consistency.consistency(src, tgt, corr, TAU, stop_after=1,
                                                                                 variant=consistency.variant(q, 0, pre), **kw))
                       for q in consistency.PAIRS_PER_LANE for pre in (False, True)]
        contenders += [("ransac_correspondences", lambda: res.__setitem__("ransac", vcrnet_amd.ransac_correspondences(src, tgt, corr, TAU))),
                       ("fast_global_registration", lambda: res.__setitem__("fgr", vcrnet_amd.fast_global_registration(src, tgt, corr))),
                       ("torch stages", lambda: res.__setitem__("torch", torch_stages(src, tgt, corr, KEEP, SEEDS)))]
        med, times, calls = run_blocks(contenders, blocks)
        for name, _ in contenders:
            v = times[name]
            say(f"B={B:2d} M={M:6d}  {name:38s} {med[name]:10.4f} ms/call  (blocks min {min(v):.4f} max {max(v):.4f}; "
                f"{blocks} x {calls[name]} calls)")
        whole, d1, d2 = med["vcr_consistency_f32 (plan)"], med["  behind the degrees"], med["  behind the kept pairs"]
        forced = {(q, pre): med[name_of(q, pre)] for q in consistency.PAIRS_PER_LANE for pre in (False, True)}
        fastest = min(forced, key=forced.get)
        mine = (plan[0], planned)
        tests = float(B) * M * M
        say(f"B={B:2d} M={M:6d}  passes: pairs + degrees + merge {d1:.4f} ms ({tests / (d1 * 1e-3) / 1e12:.3f} T tests/s), sort + kept "
            f"{d2 - d1:.4f} ms, adjacency + seeds + count + best {whole - d2:.4f} ms")
        say(f"B={B:2d} M={M:6d}  plan Q={plan[0]} S={plan[1]} {'pre-test' if planned else 'plain'}: {forced[mine]:.4f} ms; the fastest "
            f"forced form is Q={fastest[0]} {'pre-test' if fastest[1] else 'plain'} at {forced[fastest]:.4f} ms (plan / fastest "
            f"x{forced[mine] / forced[fastest]:.3f}); the others: "
            + ", ".join(f"Q={q} {'pre-test' if pre else 'plain'} x{forced[(q, pre)] / forced[mine]:.3f}" for q, pre in forced if (q, pre) != mine)
            + " of the plan's")
        hip = res["hip"]
        tdeg, tkept, _ = res["torch"]
        same_deg = float((tdeg == hip["deg"]).float().mean())
        k = min(KEEP, M)
        common = np.mean([len(np.intersect1d(tkept[b].cpu().numpy(), hip["kept"][b, :k].cpu().numpy())) / k for b in range(B)])
        say(f"B={B:2d} M={M:6d}  call / ransac (100 000 trials) x{whole / med['ransac_correspondences']:.2f}; call / fgr "
            f"x{whole / med['fast_global_registration']:.2f}; torch stages / call x{med['torch stages'] / whole:.2f}; torch's degree is "
            f"the kernel's on {100 * same_deg:.3f} % of the pairs, its kept pairs on {100 * common:.2f} %")
        say(f"B={B:2d} M={M:6d}  inliers: consistency {hip['inliers'].tolist()}, ransac {res['ransac']['inliers'].tolist()}")
        say()


def pose_ok(R, t, c):
    E = np.asarray(R, np.float64) @ c["R"].T
    sine = 0.5 * np.linalg.norm([E[2, 1] - E[1, 2], E[0, 2] - E[2, 0], E[1, 0] - E[0, 1]])
    deg = np.degrees(np.arctan2(sine, (np.trace(E) - 1) / 2))
    return bool(deg <= 1.0 and np.abs(np.asarray(t, np.float64) - c["t"]).max() <= 1e-2)


def ledger(path):
    out = []

    def note(line=""):
        print(line, flush=True)
        out.append(line)
    note(f"# kernel_sources_sha16={build.sources_sha16()}")
    note("# profiles/bench_consistency.py: of eight seeds, how many end within 1 degree and 1e-2 of the planted pose (the global pose, "
         "no refinement)")
    note(f"## planted(M = {LEDGER_M}, share), max_dist = tau = {TAU}; consistency keep {LEDGER_KEEP} seeds {LEDGER_SEEDS}; ransac 100 000 "
         "trials, similarity 0.9; fgr defaults")
    for share in (0.20, 0.05, 0.02, 0.01):
        cs = [mr.planted(LEDGER_M, share, seed=s) for s in range(8)]
        src, tgt, corr = (torch.from_numpy(np.stack([c[k] for c in cs])).cuda() for k in ("src", "tgt", "corr"))
        runs = {"consistency": vcrnet_amd.consistency_registration(src, tgt, corr, TAU, keep=LEDGER_KEEP, seeds=LEDGER_SEEDS),
                "ransac": vcrnet_amd.ransac_correspondences(src, tgt, corr, TAU),
                "fgr": vcrnet_amd.fast_global_registration(src, tgt, corr)}
        note(f"share {share:.2f} ({int(round(share * LEDGER_M))} right pairs): " + ", ".join(
            f"{name} {sum(pose_ok(r['R'][b].cpu().numpy(), r['t'][b].cpu().numpy(), cs[b]) for b in range(8))}/8"
            + (f" (inliers {r['inliers'].tolist()})" if "inliers" in r else "") for name, r in runs.items()))
    note()
    note(f"## surface(600, seed), register_features(max_dist {mr.MAX_DIST}, k 20, mutual), the method's defaults")
    for oriented in (False, True):
        hits = {"consistency": 0, "ransac": 0, "fgr": 0}
        for s in range(8):
            c = mr.surface(600, seed=s)
            src, tgt = (torch.from_numpy(c[k][None]).cuda() for k in ("src", "tgt"))
            kw = {}
            if oriented:
                ups = mr.surface_up(c)
                kw = dict(zip(("src_normals", "tgt_normals"),
                              (torch.from_numpy(mr.orient(vcrnet_amd.estimate_normals(x, 20)[0].cpu().numpy(), up)[None]).cuda()
                               for x, up in zip((src, tgt), ups))))
            for method in hits:
                r = vcrnet_amd.register_features(src, tgt, mr.MAX_DIST, k=20, method=method, **kw)
                hits[method] += pose_ok(r["R"][0].cpu().numpy(), r["t"][0].cpu().numpy(), c)
        note(f"{'oriented' if oriented else 'estimated'} normals: " + ", ".join(f"{m} {n}/8" for m, n in hits.items()))
    with open(path, "w") as fh:
        fh.write("\n".join(out) + "\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--blocks", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "consistency_bench.txt"))
    ap.add_argument("--ledger", default=os.path.join(ROOT, "profiles", "consistency_ledger.txt"))
    a = ap.parse_args()
    ledger(a.ledger)
    say(f"# kernel_sources_sha16={build.sources_sha16()}")
    say(f"# profiles/bench_consistency.py --blocks {a.blocks}: device {torch.cuda.get_device_name(0)}, "
        f"{torch.cuda.get_device_properties(0).multi_processor_count} CUs; ms per call = median of the blocks")
    say()
    part_a(a.blocks)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        fh.write("\n".join(LINES) + "\n")


if __name__ == "__main__":
    main()
