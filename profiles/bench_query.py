#!/usr/bin/env python
"""The searches from any query positions (vcr_query_knn_f32, vcr_query_radius_f32) on the GPU, in one
process, against

  (a) the same result from torch device ops: chunked cdist + topk (kNN), chunked cdist + nonzero + two stable sorts (radius);
  (b) the self searches that were there before, vcr_grid_knn_f32 / vcr_grid_radius_f32, on the same cloud at M = N with the
      points themselves as the queries (the cross rows then hold the point itself in front: k + 1 and n_i + 1 entries);
  (c) both orders the queries can be served in: sorted by their cell in the points' grid (1), and in index order (2).

Shapes (B, N points, M queries): (16, 1 024, 1 024), (16, 16 384, 16 384), (1, 131 072, 131 072), (1, 16 384, 131 072) and
(1, 131 072, 16 384); a uniform cube and a sphere's surface (profiles/bench_grid.py's clouds); queries `jitter` (points of the
cloud plus noise of an automatic cell) and `outside` (uniform in the box scaled x3 about its centre: 26 of 27 lie beyond it);
k = 1 and 20; radii for about 12 and about 100 points of the UNIFORM cube inside (the mean row is printed).

Per case: ms per call from device events around `--blocks` repeated blocks of calls after a warm-up, contenders alternated block
by block, each block's round starting at another contender and each contender run once untimed before its block (section 4.8's
protocol); the median block, the fastest and the slowest.  A contender "beats" another when its SLOWEST block is below the
other's FASTEST.  The torch contenders are timed apart (one warm-up, two calls).  Both orders are asserted bit-identical while
timing.

  python profiles/bench_query.py [--blocks 5] [--quick] [--shapes 0,1,2,3,4] [--out profiles/query_bench.txt]
"""
import argparse
import os
import re
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import vcrnet_amd  # noqa: E402,F401
from vcrnet_amd import build, grid, query, radius  # noqa: E402
import bench_grid as bg  # noqa: E402  (the clouds, the race and the spread rule)
from bench_radius import apart, radius_for, verdict  # noqa: E402

SHAPES = ((16, 1024, 1024), (16, 16384, 16384), (1, 131072, 131072), (1, 16384, 131072), (1, 131072, 16384))
DENSITIES = ("uniform", "surface")
QUERIES = ("jitter", "outside")
KS = (1, 20)
INSIDE = (12, 100)
LIMIT_SLOTS = 1 << 27                                      # B * capacity beyond which the full radius call is not timed here
CHUNK = 1 << 24                                            # elements of a cdist block
say = bg.say


def queries_of(kind, xyz, M, seed):
    """[B,3,M] on the device: `jitter` or `outside` (tests/query_restated.py's recipes of those names)."""
    g = torch.Generator(device="cpu").manual_seed(seed)
    B, _, N = xyz.shape
    lo, hi = xyz.min(2, keepdim=True).values, xyz.max(2, keepdim=True).values
    if kind == "jitter":
        pick = torch.randint(0, N, (B, 1, M), generator=g).cuda().expand(B, 3, M)
        return (xyz.gather(2, pick) + torch.randn(B, 3, M, generator=g).cuda() * bg.auto_edge(xyz)).contiguous()
    u = torch.rand(B, 3, M, generator=g).cuda() * 3.0 - 1.5
    return (0.5 * (lo + hi) + u * (hi - lo)).contiguous()


def torch_knn(xyz, q, k):
    """(a) for the kNN: per cloud chunked cdist + topk -> (d [B,M,k], idx [B,M,k])."""
    B, _, N = xyz.shape
    M = q.shape[2]
    pts, qs = xyz.transpose(1, 2).contiguous(), q.transpose(1, 2).contiguous()
    step = max(1, CHUNK // N)
    d = torch.empty(B, M, k, device=xyz.device)
    idx = torch.empty(B, M, k, dtype=torch.int64, device=xyz.device)
    for b in range(B):
        for i in range(0, M, step):
            d[b, i:i + step], idx[b, i:i + step] = torch.cdist(qs[b, i:i + step], pts[b]).topk(min(k, N), dim=1, largest=False)
    return d, idx


def torch_radius(xyz, q, r):
    """(a) for the radius rows: per cloud chunked cdist + nonzero, then two stable sorts (by distance, then by row)."""
    B, _, N = xyz.shape
    M = q.shape[2]
    pts, qs = xyz.transpose(1, 2).contiguous(), q.transpose(1, 2).contiguous()
    step = max(1, CHUNK // N)
    out = []
    for b in range(B):
        rr, cc, dd = [], [], []
        for i in range(0, M, step):
            d = torch.cdist(qs[b, i:i + step], pts[b])
            row, c = (d <= r).nonzero(as_tuple=True)
            rr.append(row + i); cc.append(c); dd.append(d[row, c])
        row, c, d = torch.cat(rr), torch.cat(cc), torch.cat(dd)
        o = d.sort(stable=True).indices
        o = o[row[o].sort(stable=True).indices]
        out.append((row[o], c[o], d[o]))
    return out


def kernel_split(fn, calls=5):
    """{kernel name: ms per call} of the library's kernels over `calls` calls, from the profiler's device records."""
    from torch.profiler import ProfilerActivity, profile
    with profile(activities=[ProfilerActivity.CUDA]) as prof:
        for _ in range(calls):
            fn()
        torch.cuda.synchronize()
    split = {}
    for e in prof.key_averages():
        m = re.search(r"((?:grid|radius|rows|query)_\w+_kernel)", e.key)
        if m:
            t = getattr(e, "device_time_total", getattr(e, "cuda_time_total", 0.0)) / 1e3 / calls
            split[m.group(1)] = split.get(m.group(1), 0.0) + t
    return split


def split_line(tag, fn):
    split = kernel_split(fn)
    say(f"{tag} per kernel: " + ", ".join(f"{n} {v:.4f}" for n, v in sorted(split.items(), key=lambda kv: -kv[1]))
        + f" ms; sum {sum(split.values()):.4f} ms")


def same(a, b, names):
    return all(torch.equal(a[k].view(torch.int32) if a[k].dtype == torch.float32 else a[k],
                           b[k].view(torch.int32) if b[k].dtype == torch.float32 else b[k]) for k in names)


def order_verdict(times, orders):
    c, i = times["cell order"], times["index order"]
    orders.append((bg.beats(c, i), bg.beats(i, c), float(np.median(i) / np.median(c))))
    return f"index / cell = x{np.median(i) / np.median(c):.2f}: {verdict(c, i, 'cell order', 'index order')}"


def bench_knn(density, B, N, M, kind, k, blocks, orders):
    xyz = bg.cloud(density, B, N, B + N + k)
    q = queries_of(kind, xyz, M, N + M + k)
    tag = f"knn    {density:8s} B={B:2d} N={N:6d} M={M:6d} {kind:8s} k={k:2d}:"
    res = {}
    times = bg.race(tag, [("the plan's order", lambda: res.__setitem__(0, query.grid_knn(xyz, q, k))),
                          ("cell order", lambda: res.__setitem__(1, query.grid_knn(xyz, q, k, variant=1))),
                          ("index order", lambda: res.__setitem__(2, query.grid_knn(xyz, q, k, variant=2)))], blocks)
    assert same(res[1], res[0], ("idx", "d2")) and same(res[2], res[0], ("idx", "d2"))
    plan = times["the plan's order"]
    t = apart(lambda: res.__setitem__("torch", torch_knn(xyz, q, k)))
    agree = (res["torch"][1] == res[0]["idx"]).float().mean().item()
    say(f"{tag} {order_verdict(times, orders[('knn', kind, B, N, M)])}; torch cdist + topk {t:10.4f} ms/call (timed apart), "
        f"x{t / np.median(plan):.1f} of the plan's; its neighbours agree in {agree:.6f} of the slots")
    say()


def bench_radius(density, B, N, M, kind, inside, blocks, orders):
    xyz = bg.cloud(density, B, N, B + N + inside)
    q = queries_of(kind, xyz, M, N + M + inside)
    r = radius_for(N, inside)
    tag = f"radius {density:8s} B={B:2d} N={N:6d} M={M:6d} {kind:8s} inside={inside:3d}:"
    counted = query.grid_radius(xyz, q, r, 0, want_idx=False)
    cap = int(counted["total"].max())
    mean_row, longest = counted["count"].float().mean().item(), int(counted["count"].max())
    if B * cap >= LIMIT_SLOTS or cap == 0:
        say(f"{tag} capacity {cap} a cloud, mean row {mean_row:.1f}, longest {longest}: not timed here")
        say()
        return
    res = {}
    names = ("count", "row_start", "total", "idx", "d2")
    times = bg.race(tag, [("count only", lambda: query.grid_radius(xyz, q, r, 0, want_idx=False)),
                          ("the plan's order", lambda: res.__setitem__(0, query.grid_radius(xyz, q, r, cap))),
                          ("cell order", lambda: res.__setitem__(1, query.grid_radius(xyz, q, r, cap, variant=1))),
                          ("index order", lambda: res.__setitem__(2, query.grid_radius(xyz, q, r, cap, variant=2)))], blocks)
    assert same(res[1], res[0], names) and same(res[2], res[0], names)
    plan = times["the plan's order"]
    t = apart(lambda: res.__setitem__("torch", torch_radius(xyz, q, r)))
    agree = sum(int(len(res["torch"][b][1]) == int(res[0]["total"][b])) for b in range(B))
    say(f"{tag} capacity {cap} a cloud, mean row {mean_row:.1f}, longest {longest}; {order_verdict(times, orders[('radius', kind, B, N, M)])}; "
        f"torch cdist + nonzero + sorts {t:10.4f} ms/call (timed apart), x{t / np.median(plan):.1f} of the plan's; its totals agree in "
        f"{agree} of {B} clouds")
    say()


def bench_self(density, B, N, blocks):
    """(b): the cloud searched in itself -- the self searches against the cross searches with the points as the queries."""
    xyz = bg.cloud(density, B, N, B + N + 7)
    for k in KS:
        tag = f"self   {density:8s} B={B:2d} N={N:6d} k={k:2d}:"
        times = bg.race(tag, [("search_knn (the self search)", lambda: grid.grid_knn(xyz, k)),
                              ("cross, k + 1, queries = the points", lambda: query.grid_knn(xyz, xyz, k + 1))], blocks)
        s, c = times["search_knn (the self search)"], times["cross, k + 1, queries = the points"]
        say(f"{tag} cross / self = x{np.median(c) / np.median(s):.2f}: {verdict(c, s, 'the cross search', 'the self search')}")
        if N == 131072:
            split_line(tag + " self ", lambda: grid.grid_knn(xyz, k))
            split_line(tag + " cross", lambda: query.grid_knn(xyz, xyz, k + 1))
        say()
    for inside in INSIDE:
        r = radius_for(N, inside)
        tag = f"self   {density:8s} B={B:2d} N={N:6d} inside={inside:3d}:"
        cap = int(radius.grid_radius(xyz, r, 0, want_idx=False)["total"].max())
        if B * (cap + N) >= LIMIT_SLOTS:
            say(f"{tag} capacity {cap} a cloud: not timed here")
            continue
        times = bg.race(tag, [("search_radius (the self search)", lambda: radius.grid_radius(xyz, r, cap)),
                              ("cross, queries = the points", lambda: query.grid_radius(xyz, xyz, r, cap + N))], blocks)
        s, c = times["search_radius (the self search)"], times["cross, queries = the points"]
        say(f"{tag} capacity {cap} (+ N for the cross rows); cross / self = x{np.median(c) / np.median(s):.2f}: "
            f"{verdict(c, s, 'the cross search', 'the self search')}")
        if N == 131072:
            split_line(tag + " self ", lambda: radius.grid_radius(xyz, r, cap))
            split_line(tag + " cross", lambda: query.grid_radius(xyz, xyz, r, cap + N))
        say()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--blocks", type=int, default=5)
    ap.add_argument("--quick", action="store_true", help="the smallest shape only")
    ap.add_argument("--shapes", default=",".join(str(i) for i in range(len(SHAPES))), help="indices into SHAPES")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "query_bench.txt"))
    a = ap.parse_args()
    say(f"# kernel_sources_sha16={build.sources_sha16()}")
    say(f"# profiles/bench_query.py --blocks {a.blocks} --shapes {a.shapes}: device {torch.cuda.get_device_name(0)}, "
        f"{torch.cuda.get_device_properties(0).multi_processor_count} CUs; ms per call = median of the blocks")
    say()
    shapes = SHAPES[:1] if a.quick else [SHAPES[int(i)] for i in a.shapes.split(",")]
    from collections import defaultdict
    orders = defaultdict(list)
    for B, N, M in shapes:
        for density in DENSITIES:
            for kind in QUERIES:
                for k in KS:
                    bench_knn(density, B, N, M, kind, k, a.blocks, orders)
                for inside in INSIDE:
                    bench_radius(density, B, N, M, kind, inside, a.blocks, orders)
            if N == M:
                bench_self(density, B, N, a.blocks)
    say("# (c) the queries' order, per search, query kind and shape: cases where cell order beats index order beyond the spread / "
        "where index order beats cell order / all cases; the median ratio index / cell")
    for key, rows in sorted(orders.items(), key=str):
        say(f"#   {key}: {sum(r[0] for r in rows)} / {sum(r[1] for r in rows)} / {len(rows)}; x{np.median([r[2] for r in rows]):.2f}")
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        fh.write("\n".join(bg.LINES) + "\n")


if __name__ == "__main__":
    main()
