#!/usr/bin/env python
"""Refining a registration on the full clouds (vcr_refine_f32): what a round costs, against one
vcr_nn_score_f32 call at the same shape (the difference is what the refinement's merge and per-cloud kernels add to the search),
what a round costs once every cloud has stopped (three launches that return at their gate), and the same loop in torch device
ops -- chunked distance blocks as in bench_nnscore.py, a masked covariance, torch.linalg.svd -- on the same GPU, the same
inputs, in the same process.

Shapes (B, Ns, Nt) are bench_nnscore.py's four.  The target is uniform in [-1,1]^3; the source is Ns of its points, jittered by
0.002 and moved off by 2 degrees and 0.01; max_dist 0.05.  Contenders:
  refine K rounds      max_iterations = K - 1, both thresholds 0 (no cloud ever converges): ms per call / K
  nn_score             one call under the start pose
  refine, stopped      thresholds 1: every cloud converges in its second round; (ms at 34 rounds - ms at 2 rounds) / 32
  torch K rounds       the loop in torch ops: ms per call / K
ms per call from device events around `--blocks` repeated blocks of calls after a warm-up, contenders alternated block by
block, each block's round starting at another contender and each contender run once untimed before its block; the median
block, the fastest and the slowest.

  python profiles/bench_refine.py [--blocks 5] [--quick] [--out profiles/refine_bench.txt]
"""
import argparse
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import vcrnet_amd  # noqa: E402,F401
from vcrnet_amd import build, refine, score  # noqa: E402

SHAPES = ((16, 1024, 1024), (16, 16384, 16384), (1, 1024, 131072), (1, 131072, 131072))
MAX_DIST = 0.05
ROUNDS = 8
TAIL = (2, 34)
LINES = []


def say(line=""):
    print(line, flush=True)
    LINES.append(line)


def rotation(axis, degrees):
    a = np.asarray(axis, np.float64)
    a = a / np.linalg.norm(a)
    K = np.asarray([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    th = np.deg2rad(degrees)
    return np.eye(3) + np.sin(th) * K + (1 - np.cos(th)) * (K @ K)


def torch_icp(src, tgt, R, t, max_dist, rounds, block_elems=1 << 24):
    """The contender: `rounds` evaluations and rounds - 1 updates, no stop test (no host synchronisation either)."""
    B, _, Ns = src.shape
    Nt = tgt.shape[2]
    q = tgt.transpose(1, 2)                                            # [B, Nt, 3]
    rows = max(1, block_elems // (B * Nt))
    R, t = R.double(), t.double()
    for k in range(rounds):
        p = (torch.bmm(R.float(), src) + t.float()[:, :, None]).transpose(1, 2)      # [B, Ns, 3]
        d2, idx = [], []
        for i in range(0, Ns, rows):
            m = ((p[:, i:i + rows, None, :] - q[:, None, :, :]) ** 2).sum(-1).min(2)
            d2.append(m.values)
            idx.append(m.indices)
        d2, idx = torch.cat(d2, 1), torch.cat(idx, 1)
        inl = (d2 <= max_dist * max_dist)
        n = inl.sum(1).clamp(min=1).double()
        if k + 1 == rounds:
            break
        w = inl.double()[:, :, None]
        pd, qd = p.double() * w, torch.gather(q, 1, idx[:, :, None].expand(B, Ns, 3)).double() * w
        pm, qm = pd.sum(1) / n[:, None], qd.sum(1) / n[:, None]
        H = torch.bmm(pd.transpose(1, 2), qd) - n[:, None, None] * pm[:, :, None] * qm[:, None, :]
        U, _, Vh = torch.linalg.svd(H)
        V = Vh.transpose(1, 2)
        d = torch.sign(torch.linalg.det(torch.bmm(V, U.transpose(1, 2))))
        V = torch.cat([V[:, :, :2], V[:, :, 2:] * d[:, None, None]], 2)
        Ri = torch.bmm(V, U.transpose(1, 2))
        ti = qm - torch.bmm(Ri, pm[:, :, None])[:, :, 0]
        R, t = torch.bmm(Ri, R), torch.bmm(Ri, t[:, :, None])[:, :, 0] + ti
    return R.float(), t.float(), inl.sum(1).float() / Ns, torch.sqrt((d2.double() * inl).sum(1) / n).float()


def timed(fn, calls):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(calls):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / calls


def bench_shape(B, Ns, Nt, blocks):
    rs = np.random.RandomState(B + Ns + Nt)
    tgt_n = rs.uniform(-1, 1, (B, 3, Nt))
    src_n = np.empty((B, 3, Ns))
    for b in range(B):
        Rd, td = rotation(rs.normal(size=3), 2.0), rs.uniform(-0.01, 0.01, 3)
        clean = tgt_n[b][:, rs.choice(Nt, Ns, replace=Ns > Nt)] + rs.uniform(-0.002, 0.002, (3, Ns))
        src_n[b] = Rd.T @ (clean - td[:, None])
    src, tgt = (torch.from_numpy(x.astype(np.float32)).cuda() for x in (src_n, tgt_n))
    R0, t0 = torch.eye(3, device="cuda").repeat(B, 1, 1), torch.zeros(B, 3, device="cuda")
    cu = torch.cuda.get_device_properties(0).multi_processor_count
    form = refine.refine_form(B, Ns, Nt, cu_count=cu)[:2]
    assert form == score.nn_score_form(B, Ns, Nt, cu_count=cu)[:2]
    torch_rounds = ROUNDS if Ns * Nt * B < 1 << 30 else 2            # (two rounds of the big shapes are 100 ... 400 ms already)
    res = {}
    run = lambda name, **kw: (name, lambda: res.__setitem__(name, refine.refine(src, tgt, R0, t0, MAX_DIST, want_nn=False, **kw)))   # noqa: E731
    contenders = [
        run("refine K rounds", max_iterations=ROUNDS - 1, rel_fitness=0.0, rel_rmse=0.0),
        ("nn_score", lambda: res.__setitem__("nn_score", score.nn_score(src, tgt, R0, t0, MAX_DIST, want_nn=False))),
        run("stopped, 2 rounds", max_iterations=TAIL[0] - 1, rel_fitness=1.0, rel_rmse=1.0),
        run("stopped, 34 rounds", max_iterations=TAIL[1] - 1, rel_fitness=1.0, rel_rmse=1.0),
        ("torch K rounds", lambda: res.__setitem__("torch", torch_icp(src, tgt, R0, t0, MAX_DIST, torch_rounds))),
    ]
    times, calls = {}, {}
    for name, fn in contenders:                               # warm every contender; size its block to ~30 ms, 2 ... 50 calls
        fn()
        torch.cuda.synchronize()
        one = timed(fn, 1)
        calls[name] = int(min(50, max(2, 30.0 / max(one, 1e-3))))
        times[name] = []
    for i in range(blocks):                                   # alternated; the round starts one contender later every block
        k = i * len(contenders) // blocks
        for name, fn in contenders[k:] + contenders[:k]:
            fn()
            times[name].append(timed(fn, calls[name]))
    full, s2, s34 = res["refine K rounds"], res["stopped, 2 rounds"], res["stopped, 34 rounds"]
    assert full["iterations"].tolist() == [ROUNDS - 1] * B and full["converged"].tolist() == [0] * B
    assert s34["iterations"].tolist() == [1] * B and s34["converged"].tolist() == [1] * B
    for k in ("R", "t", "fitness", "rmse", "inliers", "sum_d2"):                 # the closed gate leaves the result alone
        assert torch.equal(s2[k], s34[k]), k
    closing = score.nn_score(src, tgt, full["R"], full["t"], MAX_DIST, want_nn=False)
    for k in ("fitness", "rmse", "inliers", "sum_d2"):
        assert torch.equal(closing[k], full[k]), k
    med = {n: float(np.median(v)) for n, v in times.items()}
    for name, _ in contenders:
        v = times[name]
        say(f"B={B:2d} Ns={Ns:6d} Nt={Nt:6d}  {name:20s} {med[name]:10.4f} ms/call  (blocks min {min(v):.4f} max {max(v):.4f}; "
            f"{blocks} x {calls[name]} calls)")
    per_round = med["refine K rounds"] / ROUNDS
    tail = (med["stopped, 34 rounds"] - med["stopped, 2 rounds"]) / (TAIL[1] - TAIL[0])
    tr = med["torch K rounds"] / torch_rounds
    tR, tt, tfit, trmse = res["torch"]
    say(f"B={B:2d} Ns={Ns:6d} Nt={Nt:6d}  search Q{form[0]} S{form[1]}: a round {per_round:.4f} ms; nn_score {med['nn_score']:.4f} ms; "
        f"merge + per-cloud kernels over nn_score's merge + final {per_round - med['nn_score']:+.4f} ms; a stopped round "
        f"{tail:.4f} ms; torch a round {tr:.4f} ms ({torch_rounds} rounds) = x{tr / per_round:.1f}; after {ROUNDS - 1} updates fitness "
        f"{float(full['fitness'][0]):.4f} rmse {float(full['rmse'][0]):.5f}"
        + (f" (torch {float(tfit[0]):.4f} {float(trmse[0]):.5f}, max |R - torch R| {float((full['R'] - tR).abs().max()):.1e})"
           if torch_rounds == ROUNDS else ""))
    say()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--blocks", type=int, default=5)
    ap.add_argument("--quick", action="store_true", help="the two small-source shapes only")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "refine_bench.txt"))
    a = ap.parse_args()
    say(f"# kernel_sources_sha16={build.sources_sha16()}")
    say(f"# profiles/bench_refine.py --blocks {a.blocks}: device {torch.cuda.get_device_name(0)}, "
        f"{torch.cuda.get_device_properties(0).multi_processor_count} CUs; max_dist {MAX_DIST}; ms per call = median of the blocks")
    say()
    for B, Ns, Nt in (SHAPES[0], SHAPES[2]) if a.quick else SHAPES:
        bench_shape(B, Ns, Nt, a.blocks)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        fh.write("\n".join(LINES) + "\n")


if __name__ == "__main__":
    main()
