#!/usr/bin/env python
"""The robust point-to-plane refinement and the information matrix (vcr_refine_robust_f32, vcr_information_f32, DESIGN.md
section 4.31) against the entry points they extend, by bench_plane.py's protocol (section 4.8's: device events around repeated
blocks after a warm-up, contenders alternated block by block, the median block with the fastest and the slowest).  Shapes and
inputs: bench_gicp.py's part b (bench_refine.py's four shapes, the target's normals random unit vectors -- a round's cost does
not depend on their values).  Two parts, each of which can run alone (--part):

  b  a robust round per loss against a point-to-plane round, by scan and by grid (K rounds, thresholds 0: no cloud converges).
  i  information_matrix against score_registration at the same pose, by scan and by grid: the same search and merge, nine sums
     more a point and one small launch more.

Both yardsticks (vcr_refine_plane_f32, vcr_nn_score_f32 and their grid siblings) are entry points this feature does not touch.
No time is asserted anywhere: the file records what was measured.

  python profiles/bench_robust.py [--part bi] [--blocks 5] [--out profiles/robust_bench.txt] [--append]
"""
import argparse
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import vcrnet_amd  # noqa: E402,F401
from vcrnet_amd import build, plane, robust  # noqa: E402
from bench_refine import SHAPES as REFINE_SHAPES, MAX_DIST, ROUNDS, rotation  # noqa: E402
from bench_plane import LINES, run_blocks, say  # noqa: E402

K = {"l2": 1.0, "huber": 0.02, "cauchy": 0.02, "gm": 0.02 * 0.02, "tukey": 0.02}   # (GM's scale is a squared length)


def inputs(B, Ns, Nt):
    """bench_gicp.py's part b: a uniform cube, the source a 2-degree, 0.01 disturbance of noisy target points."""
    rs = np.random.RandomState(B + Ns + Nt)
    tgt_n = rs.uniform(-1, 1, (B, 3, Nt))
    src_n = np.empty((B, 3, Ns))
    for b in range(B):
        Rd, td = rotation(rs.normal(size=3), 2.0), rs.uniform(-0.01, 0.01, 3)
        clean = tgt_n[b][:, rs.choice(Nt, Ns, replace=Ns > Nt)] + rs.uniform(-0.002, 0.002, (3, Ns))
        src_n[b] = Rd.T @ (clean - td[:, None])
    nt_n = rs.normal(size=(B, 3, Nt))
    nt_n /= np.linalg.norm(nt_n, axis=1, keepdims=True)
    src, tgt, nt = (torch.from_numpy(x.astype(np.float32)).cuda() for x in (src_n, tgt_n, nt_n))
    return src, tgt, nt, torch.eye(3, device="cuda").repeat(B, 1, 1), torch.zeros(B, 3, device="cuda")


def part_b(blocks):
    say(f"## b. a robust round per loss against a point-to-plane round, scan and grid ({ROUNDS} rounds, thresholds 0, max_dist {MAX_DIST}; "
        f"k = {K['tukey']}, GM {K['gm']:g})")
    for B, Ns, Nt in REFINE_SHAPES:
        src, tgt, nt, R0, t0 = inputs(B, Ns, Nt)
        res = {}
        kw = dict(max_iterations=ROUNDS - 1, rel_fitness=0.0, rel_rmse=0.0, want_nn=False)
        head = f"B={B:2d} Ns={Ns:6d} Nt={Nt:6d}"
        for search in ("scan", "grid"):
            rob = lambda loss: robust.refine_robust(src, tgt, nt, R0, t0, MAX_DIST, loss, K[loss], search=search, **kw)   # noqa: E731
            contenders = [("point to plane", lambda: res.__setitem__("point to plane", plane.refine_plane(src, tgt, nt, R0, t0, MAX_DIST, search=search, **kw)))]
            for loss in robust.LOSSES:
                contenders.append((loss, lambda loss=loss: res.__setitem__(loss, rob(loss))))
            med, times, calls = run_blocks(contenders, blocks)
            for name, _ in contenders:
                v = times[name]
                say(f"{head} {search}  {name:14s} {med[name]:10.4f} ms/call  (blocks min {min(v):.4f} max {max(v):.4f}; {blocks} x {calls[name]} calls)")
            for name, _ in contenders:                          # a cloud that stopped early would make its rounds cheaper: say so
                if res[name]["iterations"].tolist() != [ROUNDS - 1] * B:
                    say(f"{head} {search}  NOTE {name}: updates applied {res[name]['iterations'].tolist()}, not {ROUNDS - 1} each")
            same = all(torch.equal(res["l2"][k].view(torch.int32), res["point to plane"][k].view(torch.int32)) for k in ("R", "t", "fitness", "rmse"))
            b = med["point to plane"]
            say(f"{head} {search}  a plane round {b / ROUNDS:.4f} ms; robust - plane a round: "
                + ", ".join(f"{loss} {(med[loss] - b) / ROUNDS:+.4f} ms ({100 * (med[loss] - b) / b:+.1f} %)" for loss in robust.LOSSES)
                + f"; l2 returns the plane fit's bits: {same}")
        say()


def part_i(blocks):
    say(f"## i. information_matrix against score_registration at the same pose, scan and grid (max_dist {MAX_DIST})")
    for B, Ns, Nt in REFINE_SHAPES:
        src, tgt, _, R0, t0 = inputs(B, Ns, Nt)
        res, head = {}, f"B={B:2d} Ns={Ns:6d} Nt={Nt:6d}"
        for search in ("scan", "grid"):                         # a search at a time, as part b: like against like in a block
            contenders = [(f"information_matrix, {search}", lambda: res.__setitem__(
                               "info " + search, vcrnet_amd.information_matrix(src, tgt, R0, t0, MAX_DIST, search=search, want_score=True))),
                          (f"score_registration, {search}", lambda: res.__setitem__(
                               "score " + search, vcrnet_amd.score_registration(src, tgt, R0, t0, MAX_DIST, search=search)))]
            med, times, calls = run_blocks(contenders, blocks)
            for name, _ in contenders:
                v = times[name]
                say(f"{head}  {name:26s} {med[name]:10.4f} ms/call  (blocks min {min(v):.4f} max {max(v):.4f}; {blocks} x {calls[name]} calls)")
            a, b = med[f"information_matrix, {search}"], med[f"score_registration, {search}"]
            same = all(torch.equal(res["info " + search][1][k], res["score " + search][k]) for k in ("fitness", "inlier_rmse", "inliers"))
            say(f"{head}  {search}: information - score {a - b:+.4f} ms ({100 * (a - b) / b:+.1f} %); the same evaluation: {same}")
        say(f"{head}  scan and grid give the same matrix: {torch.equal(res['info scan'][0], res['info grid'][0])}; inliers "
            f"{res['info scan'][1]['inliers'].tolist()[:4]}{' ...' if B > 4 else ''}")
        say()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--part", default="bi")
    ap.add_argument("--blocks", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "robust_bench.txt"))
    ap.add_argument("--append", action="store_true", help="add to --out instead of replacing it (one part per run)")
    a = ap.parse_args()
    if not a.append:
        say(f"# kernel_sources_sha16={build.sources_sha16()}")
        say(f"# profiles/bench_robust.py --blocks {a.blocks}: device {torch.cuda.get_device_name(0)}, "
            f"{torch.cuda.get_device_properties(0).multi_processor_count} CUs; ms per call = median of the blocks")
        say()
    if "b" in a.part:
        part_b(a.blocks)
    if "i" in a.part:
        part_i(a.blocks)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "a" if a.append else "w") as fh:
        fh.write("\n".join(LINES) + "\n")


if __name__ == "__main__":
    main()
