#!/usr/bin/env python
"""DBSCAN over ragged radius rows (vcr_rows_dbscan_f32, ``cluster_dbscan``), on one GPU, in one process:

  the rows call   vcr_rows_dbscan_f32 on the rows ``search_radius`` returns, in both launch forms (a lane a row, a wave a row;
                  bit-identical, asserted while timing) and the plan's; split by launch from the profiler's device records, so
                  the hook and the label pass can be compared form by form
  the whole call  cluster_dbscan(xyz, eps, min_points, capacity=...) against search_radius alone on the same cloud: the search's
                  share of the call
  torch           the same labels from torch device ops on the same rows -- scatter_reduce(amin) label propagation over the core
                  edges plus pointer jumping, iterated to a fixed point, then the roots' rank and the border minimum -- checked
                  once against the kernels' labels, timed apart

Shapes (B, N): (16, 1024), (16, 16 384), (1, 131 072); three clouds: a uniform cube, a sphere's surface and eight blobs
(profiles/bench_grid.py's clouds); two radii, for about 12 and about 100 entries a row (the mean and the longest row are printed);
min_points = half the aimed row length.  One more case stands apart: a path of 131 072 points 1 apart, indices scrambled -- one
component as long as the cloud, the union-find's worst case.  Per case: ms per call from device events around `--blocks` repeated
blocks of calls after a warm-up, contenders alternated block by block (section 4.8's protocol); the median block, the fastest and
the slowest.  A contender "beats" another when its SLOWEST block is below the other's FASTEST.  The closing lines collect the
cases in which the wave form beats the lane form, per pass: vcr_rows_dbscan_form's thresholds are read off them.

  python profiles/bench_dbscan.py [--blocks 5] [--quick] [--out profiles/dbscan_bench.txt]
"""
import argparse
import math
import os
import re
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import vcrnet_amd  # noqa: E402,F401
from vcrnet_amd import build, dbscan, radius  # noqa: E402
import bench_grid as bg  # noqa: E402  (the clouds, the race and the spread rule)

CASES = ((16, 1024), (16, 16384), (1, 131072))
DENSITIES = ("uniform", "surface", "blobs")
INSIDE = (12, 100)
PASSES = {"core": "dbscan_core_kernel", "hook": "dbscan_hook_kernel", "label": "dbscan_label_kernel"}
say = bg.say


def radius_for(density, N, inside):
    """About `inside` other points within reach: of a uniform cube [-1, 1]^3 of N points, of the unit sphere's surface, or at
    the centre of one of eight Gaussian blobs of sigma 0.02 (N / 8 points each; fewer towards its rim)."""
    if density == "uniform":
        return float(np.float32(2.0 * (3.0 * inside / (4.0 * np.pi * N)) ** (1.0 / 3.0)))
    if density == "surface":
        return float(np.float32(2.0 * math.sqrt(inside / N)))
    return float(np.float32(0.02 * (inside * 8.0 * (2.0 * np.pi) ** 1.5 * 3.0 / (4.0 * np.pi * N)) ** (1.0 / 3.0)))


def path_cloud(N, seed=11):
    perm = np.random.RandomState(seed).permutation(N)
    x = np.zeros((1, 3, N), np.float32)
    x[0, 0, perm] = np.arange(N)
    return torch.from_numpy(x).cuda()


def torch_dbscan(xyz, csr, min_points, jumps=4):
    """The contender: labels int32 [B,N] from the same rows by torch device ops.  One host synchronisation per round (the fixed
    point's test)."""
    idx, row_start, total = csr
    B, N = row_start.shape[0], row_start.shape[1] - 1
    dev = idx.device
    count = (row_start[:, 1:] - row_start[:, :-1]).reshape(-1)
    finite = torch.isfinite(xyz).all(1).reshape(-1)
    core = (count + 1 >= min_points) & finite
    me = torch.arange(B * N, device=dev)
    src = torch.repeat_interleave(me, count)
    used = torch.arange(idx.shape[1], device=dev)[None, :] < total[:, None]
    dst = (idx.long() + (torch.arange(B, device=dev) * N)[:, None])[used]
    both = core[src] & core[dst]
    a, b = src[both], dst[both]
    low = me.clone()
    while True:
        m = torch.minimum(low[a], low[b])
        new = low.scatter_reduce(0, a, m, "amin").scatter_reduce(0, b, m, "amin")
        for _ in range(jumps):
            new = new[new]
        if torch.equal(new, low):
            break
        low = new
    root = core & (low == me)
    rank = torch.cumsum(root.view(B, N).long(), 1).view(-1) - 1
    labels = torch.where(core, rank[low], torch.full_like(low, -1))
    border = ~core[src] & finite[src] & core[dst]
    big = torch.iinfo(torch.int64).max
    best = torch.full_like(low, big).scatter_reduce(0, src[border], labels[dst[border]], "amin")
    labels = torch.where(~core & (best != big), best, labels)
    return labels.view(B, N).int()


def kernel_split(fn, calls=5):
    """{kernel name: ms per call} of the dbscan_ kernels over `calls` calls, from the profiler's device records."""
    from torch.profiler import ProfilerActivity, profile
    with profile(activities=[ProfilerActivity.CUDA]) as prof:
        for _ in range(calls):
            fn()
        torch.cuda.synchronize()
    split = {}
    for e in prof.key_averages():
        m = re.search(r"(dbscan_[a-z]+_kernel)", e.key)
        if m:
            t = getattr(e, "device_time_total", getattr(e, "cuda_time_total", 0.0)) / 1e3 / calls
            split[m.group(1)] = split.get(m.group(1), 0.0) + t
    return split


def bench_rows(tag, xyz, r, mp, blocks, wins, key):
    B, _, N = xyz.shape
    csr = radius.search_radius(xyz, r)
    n_i = (csr[1][:, 1:] - csr[1][:, :-1])
    mean_row, longest, cap = n_i.float().mean().item(), int(n_i.max()), csr[0].shape[1]
    plan = dbscan.form(B, N, cap)
    names = {1: "lane", 2: "wave"}
    res = {}
    call = lambda v, k: res.__setitem__(k, dbscan.cluster_rows(*csr, N, mp, xyz=xyz, want_sizes=True, variant=v))  # noqa: E731
    call(0, "plan")
    n = res["plan"]["n_clusters"]
    noise = (res["plan"]["labels"] == -1).float().mean().item()
    say(f"{tag} radius {r:.5f}, min_points {mp}, capacity {cap} a cloud, mean row {mean_row:.1f}, longest {longest}; clusters a cloud "
        f"{n.float().mean().item():.1f} (most {int(n.max())}), noise {100 * noise:.1f} %; the plan's forms: hook {names[plan[0]]}, "
        f"labels {names[plan[1]]}; workspace {plan[2]} B")
    times = bg.race(tag, [("rows call, a lane a row", lambda: call("lane", "lane")), ("rows call, a wave a row", lambda: call("wave", "wave")),
                          ("rows call, the plan's", lambda: call(0, "plan"))], blocks)
    for k in ("labels", "n_clusters", "sizes"):
        assert torch.equal(res["lane"][k], res["wave"][k]) and torch.equal(res["lane"][k], res["plan"][k]), k
    split = {v: kernel_split(lambda v=v: call(v, v)) for v in ("lane", "wave")}
    for v in ("lane", "wave"):
        say(f"{tag} launches, {v}: " + ", ".join(f"{k[7:-7]} {t:.4f}" for k, t in sorted(split[v].items())) + " ms")
    for what, kern in PASSES.items():
        lane, wave = split["lane"].get(kern, 0.0), split["wave"].get(kern, 0.0)
        say(f"{tag} {what}: lane / wave = x{lane / max(wave, 1e-9):.2f} (from the launches' device times)")
        wins.setdefault(what, []).append(key + (round(mean_row, 1), cap // N, round(lane / max(wave, 1e-9), 2)))
    l, w = times["rows call, a lane a row"], times["rows call, a wave a row"]
    wins.setdefault("call", []).append(key + (round(mean_row, 1), cap // N, round(float(np.median(l) / np.median(w)), 2), bg.beats(w, l),
                                             bg.beats(l, w)))
    return csr, cap, res["plan"], float(np.median(times["rows call, the plan's"]))


def bench_whole(tag, xyz, r, mp, cap, blocks):
    times = bg.race(tag, [("cluster_dbscan(capacity=...)", lambda: dbscan.cluster_dbscan(xyz, r, mp, capacity=cap)),
                          ("search_radius(capacity=...)", lambda: radius.search_radius(xyz, r, capacity=cap))], blocks)
    whole, search = (float(np.median(times[k])) for k in times)
    say(f"{tag} the search is {100 * search / whole:.1f} % of cluster_dbscan")


def bench_torch(tag, xyz, csr, mp, mine, t_mine):
    theirs = torch_dbscan(xyz, csr, mp)
    torch.cuda.synchronize()
    assert torch.equal(theirs, mine["labels"]), "torch and the kernels disagree"
    t = bg.timed(lambda: torch_dbscan(xyz, csr, mp), 2)
    say(f"{tag} torch device ops on the same rows {t:.4f} ms/call, the rows call {t_mine:.4f} ms (timed apart): x{t / t_mine:.1f}; "
        f"the same labels")
    say()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--blocks", type=int, default=5)
    ap.add_argument("--quick", action="store_true", help="the smallest shape only")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "dbscan_bench.txt"))
    a = ap.parse_args()
    say(f"# kernel_sources_sha16={build.sources_sha16()}")
    say(f"# profiles/bench_dbscan.py --blocks {a.blocks}: device {torch.cuda.get_device_name(0)}, "
        f"{torch.cuda.get_device_properties(0).multi_processor_count} CUs; ms per call = median of the blocks; thresholds in this "
        f"build: hook {dbscan.WAVE_HOOK}, labels {dbscan.WAVE_LABEL}")
    say()
    wins = {}
    for B, N in CASES[:1] if a.quick else CASES:
        for density in DENSITIES:
            for inside in INSIDE:
                xyz = bg.cloud("clustered" if density == "blobs" else density, B, N, B + N + inside)
                r, mp = radius_for(density, N, inside), max(4, inside // 2)
                tag = f"{density:8s} B={B:2d} N={N:6d} inside={inside:3d}:"
                csr, cap, mine, t_mine = bench_rows(tag, xyz, r, mp, a.blocks, wins, (density, B, N, inside))
                bench_whole(tag, xyz, r, mp, cap, a.blocks)
                bench_torch(tag, xyz, csr, mp, mine, t_mine)
                del xyz, csr, mine
                torch.cuda.empty_cache()
    if not a.quick:
        N = 131072
        xyz = path_cloud(N)
        tag = f"path     B= 1 N={N:6d} inside=  2:"
        csr, cap, mine, t_mine = bench_rows(tag, xyz, 1.0, 2, a.blocks, wins, ("path", 1, N, 2))
        assert int(mine["n_clusters"][0]) == 1 and int(mine["sizes"][0, 0]) == N
        bench_whole(tag, xyz, 1.0, 2, cap, a.blocks)
        bench_torch(tag, xyz, csr, 2, mine, t_mine)
    for what in PASSES:
        say(f"# {what}: lane / wave by launch at (cloud, B, N, inside, mean row, capacity / N, ratio): " + ", ".join(str(k) for k in wins[what]))
    say("# the whole rows call: the wave form beats the lane form beyond the spread at (cloud, B, N, inside, mean row, capacity / N, "
        "lane / wave): " + (", ".join(str(k[:7]) for k in wins["call"] if k[7]) or "nowhere"))
    say("# the whole rows call: the lane form beats the wave form beyond the spread at: "
        + (", ".join(str(k[:7]) for k in wins["call"] if k[8]) or "nowhere"))
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        fh.write("\n".join(bg.LINES) + "\n")


if __name__ == "__main__":
    main()
