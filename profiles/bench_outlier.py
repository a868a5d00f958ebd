#!/usr/bin/env python
"""The outlier filters (vcr_outlier_radius_f32, vcr_outlier_stat_f32) against what a user had before
them: the same results in torch device ops -- chunked cdist + a count for the radius filter, chunked cdist + topk for the
statistical one -- on the same GPU, the same inputs, in the same process; and, in the same session, score_registration's scan
(vcr_nn_score_f32) at the same B, N, N, which the count scan is modelled on.

Shapes (B, N): (16, 1024), (16, 16 384), (1, 131 072) on a uniform cube; the radius holds about 12 points, nb_points = 9; the
statistical filter runs nb_neighbors = 20, std_ratio = 2.  Per shape and filter: ms per call from device events around
`--blocks` repeated blocks of calls after a warm-up, contenders alternated block by block, each block's round starting at
another contender and each contender run once untimed before its block; the median block, the fastest and the slowest (their
distance is the spread every comparison is read against).  The forced forms of the radius scan are bit-identical to the
automatic one (asserted while timing).  torch's fp32 decisions near a threshold need not be the kernels': the number of points
on which they disagree is REPORTED, not asserted.  Then the per-kernel split from the profiler's kernel records.

  python profiles/bench_outlier.py [--blocks 5] [--quick] [--out profiles/outlier_bench.txt]
"""
import argparse
import os
import re
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import vcrnet_amd  # noqa: E402,F401
from vcrnet_amd import build, native, outlier, score  # noqa: E402

CASES = ((16, 1024), (16, 16384), (1, 131072))
INSIDE, NB_POINTS, NB_NEIGHBORS, STD_RATIO = 12.0, 9, 20, 2.0
CHUNK = 1 << 25                                            # elements of one block of a distance matrix (128 MB of fp32)
LINES = []


def say(line=""):
    print(line, flush=True)
    LINES.append(line)


def torch_radius(xyz, radius, nb_points):
    """The contender: keep [B, N] bool by chunked cdist and a count."""
    B, _, N = xyz.shape
    rows = xyz.transpose(1, 2).contiguous()
    keep = torch.empty(B, N, dtype=torch.bool, device=xyz.device)
    step = max(1, CHUNK // N)
    for b in range(B):
        for i in range(0, N, step):
            d = torch.cdist(rows[b, i:i + step], rows[b])
            keep[b, i:i + step] = (d <= radius).sum(1) > nb_points
    return keep


def torch_stat(xyz, nb_neighbors, std_ratio):
    """The contender: keep [B, N] bool by chunked cdist, topk (the point itself among the nb_neighbors), mean and std."""
    B, _, N = xyz.shape
    rows = xyz.transpose(1, 2).contiguous()
    mean = torch.empty(B, N, dtype=torch.float32, device=xyz.device)
    step = max(1, CHUNK // N)
    for b in range(B):
        for i in range(0, N, step):
            d = torch.cdist(rows[b, i:i + step], rows[b])
            mean[b, i:i + step] = d.topk(nb_neighbors, dim=1, largest=False).values.mean(1)
    m = mean.double()
    thr = m.mean(1, keepdim=True) + std_ratio * m.std(1, keepdim=True)
    return m <= thr


def timed(fn, calls):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(calls):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / calls


def kernel_split(fn, calls=5):
    """{kernel name: ms per call} of the outlier_ and nn_ kernels over `calls` calls, from the profiler's device records."""
    from torch.profiler import ProfilerActivity, profile
    with profile(activities=[ProfilerActivity.CUDA]) as prof:
        for _ in range(calls):
            fn()
        torch.cuda.synchronize()
    split = {}
    for e in prof.key_averages():
        m = re.search(r"(outlier_\w+|nn_\w+_kernel)", e.key)
        if m:
            t = getattr(e, "device_time_total", getattr(e, "cuda_time_total", 0.0)) / 1e3 / calls
            split[m.group(1)] = split.get(m.group(1), 0.0) + t
    return split


def race(tag, contenders, blocks):
    """Time the contenders (name, fn) by the protocol above -> {name: [ms per call of every block]}; says a line for each."""
    times, calls = {}, {}
    for name, fn in contenders:                               # warm every contender; size its block to ~30 ms, 2 ... 50 calls
        fn()
        torch.cuda.synchronize()
        one = timed(fn, 1)
        calls[name] = int(min(50, max(2, 30.0 / max(one, 1e-3))))
        times[name] = []
    for i in range(blocks):                                   # alternated, and the round starts one contender later every block
        k = i * len(contenders) // blocks
        for name, fn in contenders[k:] + contenders[:k]:
            fn()                                              # untimed: every contender is timed behind itself
            times[name].append(timed(fn, calls[name]))
    base = float(np.median(times[contenders[0][0]]))
    for name, _ in contenders:
        v = times[name]
        say(f"{tag} {name:22s} {np.median(v):10.4f} ms/call  (blocks min {min(v):.4f} max {max(v):.4f}; "
            f"{blocks} x {calls[name]} calls)  x{np.median(v) / base:8.2f} of the first")
    return times


def split_line(tag, fn, keep):
    split = {k: v for k, v in kernel_split(fn).items() if keep(k)}
    say(f"{tag} per kernel: " + ", ".join(f"{k} {v:.4f}" for k, v in sorted(split.items(), key=lambda kv: -kv[1]))
        + f" ms; sum {sum(split.values()):.4f} ms")
    return split


def bench_radius(B, N, blocks):
    rs = np.random.RandomState(B + N)
    xyz = torch.from_numpy(rs.uniform(-1, 1, (B, 3, N)).astype(np.float32)).cuda()
    radius = float(np.float32(2.0 * (3.0 * INSIDE / (4.0 * np.pi * N)) ** (1.0 / 3.0)))
    cu = torch.cuda.get_device_properties(0).multi_processor_count
    res, seen, contenders = {}, set(), []
    for s in (0, 1, 2, 4, 8, 16, 32, 64, 128):
        form = outlier.radius_form(B, N, cu_count=cu, variant=outlier.variant(s))[1]
        if s and form in seen:
            continue
        seen.add(form)
        name = ("auto = " if not s else "forced ") + f"S{form}"
        contenders.append((name, lambda s=s: res.__setitem__(s, outlier.radius_filter(xyz, radius, NB_POINTS, outlier.variant(s)))))
    forms = len(contenders)
    contenders.append(("score_registration", lambda: res.__setitem__("score", score.nn_score(xyz, xyz, max_dist=radius))))
    contenders.append(("torch cdist + count", lambda: res.__setitem__("torch", torch_radius(xyz, radius, NB_POINTS))))
    tag = f"radius B={B:2d} N={N:6d}:"
    times = race(tag, contenders, blocks)
    auto = res[0]
    for s in res:
        if s not in (0, "score", "torch"):
            for k in ("points", "count", "index", "neighbours"):
                assert torch.equal(auto[k].view(torch.int32), res[s][k].view(torch.int32)), (s, k)
    mine = auto["neighbours"] > NB_POINTS
    med = {n: float(np.median(v)) for n, v in times.items()}
    a = times[contenders[0][0]]
    best = min((n for n, _ in contenders[:forms]), key=lambda n: med[n])
    base, spread = med[contenders[0][0]], max(a) - min(a)
    say(f"{tag} kept {auto['count'].tolist()[:4]}{' ...' if B > 4 else ''} of {N}; torch / auto = x{med['torch cdist + count'] / base:.2f}; "
        f"torch's keep disagrees on {int((mine != res['torch']).sum())} of {B * N} points; fastest form: {best} "
        f"({med[best]:.4f} ms, auto {base:.4f} ms, auto's spread {spread:.4f} ms"
        f"{'' if base - med[best] <= spread else ': BEATS auto by more than the spread'}); forms bit-identical")
    split_line(tag + " auto,", contenders[0][1], lambda k: k.startswith("outlier_"))
    split_line(tag + " score_registration,", contenders[forms][1], lambda k: k.startswith("nn_"))
    say()


def bench_stat(B, N, blocks):
    rs = np.random.RandomState(B + N + 1)
    xyz = torch.from_numpy(rs.uniform(-1, 1, (B, 3, N)).astype(np.float32)).cuda()
    rows = native.to_rows4(xyz)
    idx = native.knn(rows, None, NB_NEIGHBORS - 1)
    res = {}
    contenders = [("remove_statistical", lambda: res.__setitem__("api", outlier.remove_statistical_outlier(xyz, NB_NEIGHBORS, STD_RATIO))),
                  ("the filter alone", lambda: res.__setitem__("filter", outlier.stat_filter(rows, idx, STD_RATIO))),
                  ("the kNN alone", lambda: res.__setitem__("knn", native.knn(rows, None, NB_NEIGHBORS - 1))),
                  ("torch cdist + topk", lambda: res.__setitem__("torch", torch_stat(xyz, NB_NEIGHBORS, STD_RATIO)))]
    tag = f"statistical B={B:2d} N={N:6d}:"
    times = race(tag, contenders, blocks)
    med = {n: float(np.median(v)) for n, v in times.items()}
    o = res["filter"]
    mine = torch.zeros(B, N, dtype=torch.bool, device=xyz.device)
    for b in range(B):
        mine[b, o["index"][b, :int(o["count"][b])].long()] = True
    say(f"{tag} kept {o['count'].tolist()[:4]}{' ...' if B > 4 else ''} of {N}; torch / remove_statistical = "
        f"x{med['torch cdist + topk'] / med['remove_statistical']:.2f}; the filter / the kNN = "
        f"{med['the filter alone'] / med['the kNN alone']:.3f}; torch's keep disagrees on {int((mine != res['torch']).sum())} of {B * N} points")
    split_line(tag + " the filter,", contenders[1][1], lambda k: k.startswith("outlier_"))
    say()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--blocks", type=int, default=5)
    ap.add_argument("--quick", action="store_true", help="the smallest shape only")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "outlier_bench.txt"))
    a = ap.parse_args()
    say(f"# kernel_sources_sha16={build.sources_sha16()}")
    say(f"# profiles/bench_outlier.py --blocks {a.blocks}: device {torch.cuda.get_device_name(0)}, "
        f"{torch.cuda.get_device_properties(0).multi_processor_count} CUs; uniform cube [-1, 1]^3; ms per call = median of the blocks")
    say()
    for B, N in CASES[:1] if a.quick else CASES:
        bench_radius(B, N, a.blocks)
        bench_stat(B, N, a.blocks)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        fh.write("\n".join(LINES) + "\n")


if __name__ == "__main__":
    main()
