#!/usr/bin/env python
"""Fast Global Registration on the device (vcr_fgr_f32), by bench_match.py's protocol: ms per call from
device events around `--blocks` repeated blocks of calls after a warm-up, contenders alternated block by block; the median
block, the fastest and the slowest.

B x N = 16 x 1024, 16 x 16 384, 1 x 131 072 (Ns = Nt = N): bench_match.py's RANSAC input -- the jittered torus and a posed,
permuted copy, 30 % of the correspondences the true partner, the rest uniform.  Contenders:
  * vcr_fgr_f32 at its defaults (tuple_scale 0.95, K = 1000, 64 iterations, T = min(100 N, 2^20));
  * the same call cut down, to time its kernels apart: without iterations (the pair list, the tuple test and its compaction,
    the normalisation and the first sweep's stores), and without iterations and tuple test (the pair list and the
    normalisation; its first sweep stores all M pairs); the differences are the loop and the tuple kernels;
  * the SAME loop in batched torch device ops, fp64, from the device's own tuple list: the normalisation, then per iteration
    the residuals and weights, the 6 x 6 systems by one einsum, torch.linalg.solve, the Euler rotation and the moved points --
    no host synchronisation inside (mu's schedule does not depend on the data);
  * vcr_ransac_f32 at its default 100 000 trials (similarity 0.9, max_dist 0.05) on the same correspondences.
A per-kernel table from torch.profiler follows each shape where the profiler reports device kernels.  There is no speed
condition: the file records what was measured.

  python profiles/bench_fgr.py [--blocks 5] [--out profiles/fgr_bench.txt]
"""
import argparse
import os
import sys
import warnings

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import vcrnet_amd  # noqa: E402,F401
from vcrnet_amd import build, fgr, match  # noqa: E402
from bench_plane import LINES, NORMALS_SHAPES as SHAPES, run_blocks, say, torus  # noqa: E402

MAX_DIST, SIMILARITY, SEED, SHARE = 0.05, 0.9, 7, 0.3
ITERATIONS, DIVISION, FLOOR = 64, 1.4, 0.025


def torch_fgr(src, tgt, corr, lst, used):
    """The contender: src [B,3,Ns], tgt [B,3,Nt], corr [B,Ns], lst int [B,3K] (the device's tuple list, `used` entries each --
    the same number in every cloud here) -> (R [B,3,3], t [B,3]) float64."""
    B = src.shape[0]
    s64, t64 = src.double(), tgt.double()
    ms, mt = s64.mean(2), t64.mean(2)
    scale = torch.maximum(((s64 - ms[:, :, None]) ** 2).sum(1).amax(1), ((t64 - mt[:, :, None]) ** 2).sum(1).amax(1)).sqrt()
    i = lst[:, :used].long()
    j = torch.gather(corr.long(), 1, i)
    q = (torch.gather(s64, 2, i[:, None, :].expand(B, 3, used)) - ms[:, :, None]) / scale[:, None, None]      # [B,3,L]
    p = (torch.gather(t64, 2, j[:, None, :].expand(B, 3, used)) - mt[:, :, None]) / scale[:, None, None]
    R = torch.eye(3, dtype=torch.float64, device=src.device).expand(B, 3, 3).contiguous()
    t = torch.zeros(B, 3, dtype=torch.float64, device=src.device)
    zero, one = torch.zeros_like(q[:, 0]), torch.ones_like(q[:, 0])
    mu = 1.0
    for it in range(ITERATIONS):
        r = p - q
        w = mu / ((r * r).sum(1) + mu)
        s = w * w
        J = torch.stack([torch.stack([zero, -q[:, 2], q[:, 1], -one, zero, zero], 1),
                         torch.stack([q[:, 2], zero, -q[:, 0], zero, -one, zero], 1),
                         torch.stack([-q[:, 1], q[:, 0], zero, zero, zero, -one], 1)], 1)               # [B,3,6,L]
        A = torch.einsum("brul,brvl,bl->buv", J, J, s)
        g = torch.einsum("brul,brl,bl->bu", J, r, s)
        x = torch.linalg.solve(A, -g)
        s0, c0, s1, c1, s2, c2 = x[:, 0].sin(), x[:, 0].cos(), x[:, 1].sin(), x[:, 1].cos(), x[:, 2].sin(), x[:, 2].cos()
        Ri = torch.stack([c2 * c1, c2 * s1 * s0 - s2 * c0, c2 * s1 * c0 + s2 * s0,
                          s2 * c1, s2 * s1 * s0 + c2 * c0, s2 * s1 * c0 - c2 * s0,
                          -s1, c1 * s0, c1 * c0], 1).view(B, 3, 3)
        R, t = Ri @ R, (Ri @ t[:, :, None])[:, :, 0] + x[:, 3:]
        q = Ri @ q + x[:, 3:, None]
        if it % 4 == 0 and mu > FLOOR:
            mu /= DIVISION
    return R, scale[:, None] * t + mt - (R @ ms[:, :, None])[:, :, 0]


def kernel_table(fn):
    """Device time per kernel of three calls, by torch.profiler (None where it reports no device kernels)."""
    try:
        from torch.profiler import ProfilerActivity, profile
        fn()
        torch.cuda.synchronize()
        warnings.simplefilter("ignore")
        with profile(activities=[ProfilerActivity.CUDA]) as prof:
            for _ in range(3):
                fn()
            torch.cuda.synchronize()
        rows = []
        for e in prof.key_averages():
            us = getattr(e, "device_time_total", None)
            us = getattr(e, "cuda_time_total", 0.0) if us is None else us
            if "kernel" in e.key and us > 0:
                rows.append((e.key.replace("(anonymous namespace)::", "").replace("void ", "").split("(")[0], us / e.count, e.count))
        return rows or None
    except Exception as exc:                                  # the table is an extra: the call variants above stand without it
        say(f"    (torch.profiler: {type(exc).__name__}: {exc})")
        return None


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--blocks", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "fgr_bench.txt"))
    a = ap.parse_args()
    say(f"# kernel_sources_sha16={build.sources_sha16()}")
    say(f"# profiles/bench_fgr.py --blocks {a.blocks}: device {torch.cuda.get_device_name(0)}, "
        f"{torch.cuda.get_device_properties(0).multi_processor_count} CUs; ms per call = median of the blocks")
    say()
    say(f"## Fast Global Registration, defaults (K = 1000, {ITERATIONS} iterations), {int(100 * SHARE)} % true partners")
    for B, N in SHAPES:
        rs = np.random.RandomState(7 + N)
        tgt = torch.from_numpy(np.stack([torus(rs, N, 0.002) for _ in range(B)]).astype(np.float32)).cuda()
        th = 0.9
        A = torch.tensor([[np.cos(th), -np.sin(th), 0], [np.sin(th), np.cos(th), 0], [0, 0, 1]], dtype=torch.float32).cuda()
        perm = torch.from_numpy(np.stack([rs.permutation(N) for _ in range(B)])).cuda()
        src = torch.gather(A.t() @ (tgt - 0.25), 2, perm[:, None, :].expand(B, 3, N)).contiguous()     # tgt = A src + 0.25
        true = torch.from_numpy(rs.uniform(size=(B, N)) < SHARE).cuda()
        corr = torch.where(true, perm, torch.from_numpy(rs.randint(0, N, (B, N))).cuda()).int()
        full = fgr.fgr(src, tgt, corr, seed=SEED, want_stages=True)
        used = int(full["used"].min())
        assert used == int(full["used"].max()) and int(full["status"].max()) == 0, (full["used"], full["status"])
        lst = full["tuple_list"]
        res = {}
        contenders = [("vcr_fgr_f32", lambda: res.__setitem__("hip", fgr.fgr(src, tgt, corr, seed=SEED))),
                      ("  without iterations", lambda: fgr.fgr(src, tgt, corr, seed=SEED, iterations=0)),
                      ("  ... and tuple test", lambda: fgr.fgr(src, tgt, corr, seed=SEED, iterations=0, tuple_scale=0.0)),
                      ("torch loop, same tuples", lambda: res.__setitem__("torch", torch_fgr(src, tgt, corr, lst, used))),
                      ("vcr_ransac_f32 T=100000", lambda: res.__setitem__("ransac", match.ransac(src, tgt, corr, MAX_DIST, 100000, SIMILARITY, SEED)))]
        med, times, calls = run_blocks(contenders, a.blocks)
        for name, _ in contenders:
            v = times[name]
            say(f"B={B:2d} N={N:6d}  {name:26s} {med[name]:10.4f} ms/call  (blocks min {min(v):.4f} max {max(v):.4f}; "
                f"{a.blocks} x {calls[name]} calls)")
        Rh, th_ = res["hip"]["R"].double(), res["hip"]["t"].double()
        Rt, tt = res["torch"]
        Rr = res["ransac"]["R"].double()
        want = A.double()
        say(f"B={B:2d} N={N:6d}  loop = call - without iterations: {med['vcr_fgr_f32'] - med['  without iterations']:.4f} ms; tuple kernels = "
            f"without iterations - without both: {med['  without iterations'] - med['  ... and tuple test']:.4f} ms; torch / kernel "
            f"x{med['torch loop, same tuples'] / med['vcr_fgr_f32']:.1f}; RANSAC / FGR x{med['vcr_ransac_f32 T=100000'] / med['vcr_fgr_f32']:.2f}")
        say(f"B={B:2d} N={N:6d}  {used} entries a cloud; |R - planted| FGR {float((Rh - want).abs().max()):.2e}, torch "
            f"{float((Rt - want).abs().max()):.2e}, RANSAC {float((Rr - want).abs().max()):.2e}; |FGR - torch| R "
            f"{float((Rh - Rt).abs().max()):.2e} t {float((th_ - tt).abs().max()):.2e}")
        rows = kernel_table(lambda: fgr.fgr(src, tgt, corr, seed=SEED))
        for name, us, count in rows or ():
            say(f"    {name:24s} {us / 1000:10.4f} ms/launch  ({count} launches)")
        say()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        fh.write("\n".join(LINES) + "\n")


if __name__ == "__main__":
    main()
