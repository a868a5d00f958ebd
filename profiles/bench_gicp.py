#!/usr/bin/env python
"""The plane-to-plane refinement (vcr_refine_gicp_f32) against the other two fits, by bench_plane.py's
protocol (section 4.8's: device events around repeated blocks after a warm-up, contenders alternated block by block, the median
block with the fastest and the slowest).  Two parts, each of which can run alone (--part):

  b  a generalized round against a point-to-plane round and a point-to-point round at bench_refine.py's four shapes and inputs
     (K rounds, thresholds 0: no cloud converges), the normals of both clouds random unit vectors -- a uniform cube has no
     surface, and the round's cost does not depend on their values.
  c  bench_plane.py's convergence table with a third row per size: the torus with source and target drawn INDEPENDENTLY, a
     planted 40-degree pose, a start 6 degrees and 0.04 off, the default thresholds; the normals estimate_normals(cloud, 20).

  python profiles/bench_gicp.py [--part bc] [--blocks 5] [--out profiles/gicp_bench.txt] [--append]
"""
import argparse
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import vcrnet_amd  # noqa: E402,F401
from vcrnet_amd import build, gicp, plane, refine  # noqa: E402
from bench_refine import SHAPES as REFINE_SHAPES, MAX_DIST, ROUNDS, rotation  # noqa: E402
from bench_plane import LINES, angle, run_blocks, say, torus  # noqa: E402


def unit(rs, shape):
    n = rs.normal(size=shape)
    return n / np.linalg.norm(n, axis=1, keepdims=True)


def part_b(blocks):
    say(f"## b. a generalized round against a point-to-plane and a point-to-point round ({ROUNDS} rounds, thresholds 0, max_dist {MAX_DIST})")
    for B, Ns, Nt in REFINE_SHAPES:
        rs = np.random.RandomState(B + Ns + Nt)                # bench_refine.py's inputs
        tgt_n = rs.uniform(-1, 1, (B, 3, Nt))
        src_n = np.empty((B, 3, Ns))
        for b in range(B):
            Rd, td = rotation(rs.normal(size=3), 2.0), rs.uniform(-0.01, 0.01, 3)
            clean = tgt_n[b][:, rs.choice(Nt, Ns, replace=Ns > Nt)] + rs.uniform(-0.002, 0.002, (3, Ns))
            src_n[b] = Rd.T @ (clean - td[:, None])
        nt_n, ns_n = unit(rs, (B, 3, Nt)), unit(rs, (B, 3, Ns))
        src, tgt, nt, ns = (torch.from_numpy(x.astype(np.float32)).cuda() for x in (src_n, tgt_n, nt_n, ns_n))
        R0, t0 = torch.eye(3, device="cuda").repeat(B, 1, 1), torch.zeros(B, 3, device="cuda")
        res = {}
        kw = dict(max_iterations=ROUNDS - 1, rel_fitness=0.0, rel_rmse=0.0, want_nn=False)
        contenders = [
            ("generalized", lambda: res.__setitem__("gicp", gicp.refine_gicp(src, tgt, ns, nt, R0, t0, MAX_DIST, **kw))),
            ("point to plane", lambda: res.__setitem__("plane", plane.refine_plane(src, tgt, nt, R0, t0, MAX_DIST, **kw))),
            ("point to point", lambda: res.__setitem__("point", refine.refine(src, tgt, R0, t0, MAX_DIST, **kw))),
        ]
        med, times, calls = run_blocks(contenders, blocks)
        head = f"B={B:2d} Ns={Ns:6d} Nt={Nt:6d}"
        for name, _ in contenders:
            v = times[name]
            say(f"{head}  {name:16s} {med[name]:10.4f} ms/call  (blocks min {min(v):.4f} max {max(v):.4f}; {blocks} x {calls[name]} calls)")
        for name in ("gicp", "plane", "point"):                # a cloud that stopped early would make its rounds cheaper: say so
            if res[name]["iterations"].tolist() != [ROUNDS - 1] * B:
                say(f"{head}  NOTE {name}: updates applied {res[name]['iterations'].tolist()}, not {ROUNDS - 1} each")
        say(f"{head}  a generalized round {med['generalized'] / ROUNDS:.4f} ms, a plane round {med['point to plane'] / ROUNDS:.4f} ms, "
            f"a point round {med['point to point'] / ROUNDS:.4f} ms: generalized - plane "
            f"{(med['generalized'] - med['point to plane']) / ROUNDS:+.4f} ms, generalized - point "
            f"{(med['generalized'] - med['point to point']) / ROUNDS:+.4f} ms")
        say()


def part_c():
    say("## c. convergence on the torus, source and target drawn independently (B = 4; default thresholds, at most 50 updates)")
    for N, max_dist in ((2048, 0.1), (16384, 0.05)):
        B = 4
        rs = np.random.RandomState(N)                          # bench_plane.py's draws
        src_n, tgt_n, R_n, t_n, R0_n, t0_n = [], [], [], [], [], []
        for b in range(B):
            R, t = rotation(rs.normal(size=3), 40.0), rs.uniform(-0.5, 0.5, 3)
            d = rs.normal(size=3)
            src_n.append(torus(rs, N))
            tgt_n.append(R @ torus(rs, N) + t[:, None])
            R_n.append(R); t_n.append(t)
            R0_n.append(R @ rotation(rs.normal(size=3), 6.0)); t0_n.append(t + 0.04 * d / np.linalg.norm(d))
        f = lambda v: torch.from_numpy(np.stack(v).astype(np.float32)).cuda()   # noqa: E731
        src, tgt, R, t, R0, t0 = f(src_n), f(tgt_n), f(R_n), f(t_n), f(R0_n), f(t0_n)
        say(f"N={N:6d} max_dist {max_dist}: start rotation error {np.rad2deg(angle(R0, R).cpu().numpy()).round(3).tolist()} degrees, "
            f"translation error {(t0 - t).norm(dim=1).cpu().numpy().round(4).tolist()}")
        for method in ("point_to_point", "point_to_plane", "generalized"):
            o = vcrnet_amd.refine_registration(src, tgt, R0, t0, max_dist=max_dist, max_iterations=50, method=method)
            say(f"N={N:6d}  {method:15s} updates {o['iterations'].tolist()} converged {o['converged'].tolist()}  rotation error "
                f"{np.rad2deg(angle(o['R'], R).cpu().numpy()).round(4).tolist()} degrees  translation error "
                f"{(o['t'] - t).norm(dim=1).cpu().numpy().round(5).tolist()}  fitness {o['fitness'].cpu().numpy().round(4).tolist()} "
                f"rmse {o['inlier_rmse'].cpu().numpy().round(5).tolist()}")
        say()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--part", default="bc")
    ap.add_argument("--blocks", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "gicp_bench.txt"))
    ap.add_argument("--append", action="store_true", help="add to --out instead of replacing it (one part per run)")
    a = ap.parse_args()
    if not a.append:
        say(f"# kernel_sources_sha16={build.sources_sha16()}")
        say(f"# profiles/bench_gicp.py --blocks {a.blocks}: device {torch.cuda.get_device_name(0)}, "
            f"{torch.cuda.get_device_properties(0).multi_processor_count} CUs; ms per call = median of the blocks")
        say()
    if "b" in a.part:
        part_b(a.blocks)
    if "c" in a.part:
        part_c()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "a" if a.append else "w") as fh:
        fh.write("\n".join(LINES) + "\n")


if __name__ == "__main__":
    main()
