#!/usr/bin/env python
"""The radius search and the radius filter on the grid (vcr_grid_radius_f32, vcr_outlier_radius_grid_f32)
against what was there before them, on the same GPU, in the same process:

  the filter   vcr_outlier_radius_grid_f32 against vcr_outlier_radius_f32 (the scan: the path remove_radius_outlier had, and
               keeps by default) and against the torch device ops of profiles/bench_outlier.py (chunked cdist + a count)
  the search   vcr_grid_radius_f32 -- the count-only call, the full call at the capacity the count reports, the ordering forced
               to a wave per row and to a lane per row -- against torch device ops: chunked cdist + nonzero + two stable sorts
               (by distance, then by row)

Shapes (B, N): (16, 1024), (16, 16 384), (1, 131 072); three densities: a uniform cube, a sphere's surface and eight blobs
(profiles/bench_grid.py's clouds); two radii: outlier_restated.radius_for's formula for about 12 and about 70 points of the
UNIFORM cube inside (the other densities hold what they hold: the mean row is printed).  Per case: ms per call from device events
around `--blocks` repeated blocks of calls after a warm-up, contenders alternated block by block, each block's round starting at
another contender and each contender run once untimed before its block (section 4.8's protocol); the median block, the fastest
and the slowest.  A contender "beats" another when its SLOWEST block is below the other's FASTEST.  The torch contenders are
timed apart (one warm-up, two calls): they are 50 to 1000 times slower and would only stretch the blocks.

Per case also the per-kernel split of both calls from the profiler's kernel records (the share of the count, of the
one-workgroup offsets and of the ordering), and a sweep of the forced edge at 0.5, 1 and 2 x radius for both calls -- every
form bit-identical to the first (asserted while timing).

  python profiles/bench_radius.py [--blocks 5] [--quick] [--out profiles/radius_bench.txt]
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
from vcrnet_amd import build, outlier, radius  # noqa: E402
import bench_grid as bg  # noqa: E402  (the clouds, the race and the spread rule)

CASES = ((16, 1024), (16, 16384), (1, 131072))
DENSITIES = ("uniform", "surface", "clustered")
INSIDE = (12, 70)
EDGES = (0.5, 1.0, 2.0)                                     # forced edges, as multiples of the radius
NB_POINTS = 9
LIMIT_SLOTS = 1 << 28                                      # B * capacity beyond which the full call is not timed here
LONGEST = 4096                                             # ... and the longest row
LANE_LONGEST = 512                                         # the longest row the lane form is timed at (its cost is n^2 a LANE)
CHUNK = 1 << 24                                            # elements of a cdist block (bench_outlier's)
say = bg.say


def radius_for(N, inside):
    """tests/outlier_restated.radius_for: about `inside` points of a uniform cube [-1, 1]^3 of N points within reach."""
    return float(np.float32(2.0 * (3.0 * inside / (4.0 * np.pi * N)) ** (1.0 / 3.0)))


def torch_filter(xyz, r):
    """bench_outlier's contender: keep [B, N] bool by chunked cdist and a count."""
    B, _, N = xyz.shape
    rows = xyz.transpose(1, 2).contiguous()
    keep = torch.empty(B, N, dtype=torch.bool, device=xyz.device)
    step = max(1, CHUNK // N)
    for b in range(B):
        for i in range(0, N, step):
            keep[b, i:i + step] = (torch.cdist(rows[b, i:i + step], rows[b]) <= r).sum(1) > NB_POINTS
    return keep


def torch_search(xyz, r):
    """The search's contender: per cloud chunked cdist + nonzero, then two stable sorts (by distance, then by row) -> per cloud
    (row [T], idx [T], d [T])."""
    B, _, N = xyz.shape
    rows = xyz.transpose(1, 2).contiguous()
    step = max(1, CHUNK // N)
    out = []
    for b in range(B):
        rr, cc, dd = [], [], []
        for i in range(0, N, step):
            d = torch.cdist(rows[b, i:i + step], rows[b])
            hit = d <= r
            hit[torch.arange(hit.shape[0], device=d.device), torch.arange(i, i + hit.shape[0], device=d.device)] = False
            q, c = hit.nonzero(as_tuple=True)
            rr.append(q + i); cc.append(c); dd.append(d[q, c])
        q, c, d = torch.cat(rr), torch.cat(cc), torch.cat(dd)
        o = d.sort(stable=True).indices
        o = o[q[o].sort(stable=True).indices]
        out.append((q[o], c[o], d[o]))
    return out


def apart(fn):
    """ms per call of a slow contender: one warm-up, two timed calls."""
    fn()
    torch.cuda.synchronize()
    return bg.timed(fn, 2)


def kernel_split(fn, calls=5):
    """{kernel name: ms per call} of the library's kernels over `calls` calls, from the profiler's device records."""
    from torch.profiler import ProfilerActivity, profile
    with profile(activities=[ProfilerActivity.CUDA]) as prof:
        for _ in range(calls):
            fn()
        torch.cuda.synchronize()
    split = {}
    for e in prof.key_averages():
        m = re.search(r"((?:grid|radius|rows|outlier)_\w+_kernel)", e.key)
        if m:
            t = getattr(e, "device_time_total", getattr(e, "cuda_time_total", 0.0)) / 1e3 / calls
            split[m.group(1)] = split.get(m.group(1), 0.0) + t
    return split


def split_line(tag, fn):
    split = kernel_split(fn)
    build_ms = sum(v for n, v in split.items() if n.startswith("grid_"))
    rest = {n: v for n, v in split.items() if not n.startswith("grid_")}
    say(f"{tag} per kernel: the grid's five {build_ms:.4f}, " + ", ".join(f"{n} {v:.4f}" for n, v in sorted(rest.items(), key=lambda kv: -kv[1]))
        + f" ms; sum {sum(split.values()):.4f} ms")


def same(a, b, names):
    return all(torch.equal(a[k].view(torch.int32) if a[k].dtype == torch.float32 else a[k],
                           b[k].view(torch.int32) if b[k].dtype == torch.float32 else b[k]) for k in names)


def verdict(g, s, what_g, what_s):
    return (f"{what_g} BEATS {what_s} beyond the spread" if bg.beats(g, s) else
            f"{what_s} BEATS {what_g} beyond the spread" if bg.beats(s, g) else "within the blocks' spread")


def bench_filter(density, B, N, inside, blocks, won, edge_wins):
    xyz = bg.cloud(density, B, N, B + N + inside)
    r = radius_for(N, inside)
    tag = f"filter {density:9s} B={B:2d} N={N:6d} inside={inside:2d}:"
    res = {}
    names = ("points", "count", "index", "neighbours")
    times = bg.race(tag, [("grid (edge = radius)", lambda: res.__setitem__("grid", radius.radius_filter_grid(xyz, r, NB_POINTS))),
                          ("scan (the parent's path)", lambda: res.__setitem__("scan", outlier.radius_filter(xyz, r, NB_POINTS)))], blocks)
    assert same(res["grid"], res["scan"], names)
    g, s = times["grid (edge = radius)"], times["scan (the parent's path)"]
    t = apart(lambda: res.__setitem__("torch", torch_filter(xyz, r)))
    mine = res["grid"]["neighbours"] > NB_POINTS
    say(f"{tag} torch cdist + count {t:10.4f} ms/call (timed apart); its keep disagrees on {int((mine != res['torch']).sum())} of {B * N} points")
    say(f"{tag} mean c_i {res['grid']['neighbours'].float().mean().item():.1f}, kept {res['grid']['count'].tolist()[:4]}{' ...' if B > 4 else ''} of {N}; "
        f"scan / grid = x{np.median(s) / np.median(g):.2f}, torch / grid = x{t / np.median(g):.1f}; grid's slowest block {max(g):.4f} ms, "
        f"scan's fastest {min(s):.4f} ms: {verdict(g, s, 'the grid', 'the scan')}; all four outputs bit-identical")
    won[(density, B, N, inside)] = bg.beats(g, s)
    split_line(tag, lambda: radius.radius_filter_grid(xyz, r, NB_POINTS))
    sweep = bg.race(tag + " edge", [(f"cell = {f:3.1f} x radius", lambda f=f: res.__setitem__(f, radius.radius_filter_grid(xyz, r, NB_POINTS, cell=f * r)))
                                    for f in EDGES], blocks)
    for f in EDGES:
        assert same(res[f], res["grid"], names), f
    rule = sweep["cell = 1.0 x radius"]
    for f in EDGES:
        if f != 1.0:
            edge_wins.setdefault(("filter", f), []).append((density, B, N, inside, bg.beats(sweep[f"cell = {f:3.1f} x radius"], rule)))
    say()


def bench_search(density, B, N, inside, blocks, edge_wins):
    xyz = bg.cloud(density, B, N, B + N + inside)
    r = radius_for(N, inside)
    tag = f"search {density:9s} B={B:2d} N={N:6d} inside={inside:2d}:"
    counted = radius.grid_radius(xyz, r, 0, want_idx=False)
    cap = int(counted["total"].max())
    mean_row = counted["count"].float().mean().item()
    longest = int(counted["count"].max())
    if B * cap >= LIMIT_SLOTS or longest > LONGEST:
        # the radius spans a blob: not a neighbourhood.  The ordering is quadratic in a row's length (the header says so)
        t = bg.race(tag, [("count only", lambda: radius.grid_radius(xyz, r, 0, want_idx=False))], blocks)
        say(f"{tag} capacity {cap} a cloud, mean row {mean_row:.1f}, longest {longest}: rows beyond {LONGEST} entries or {LIMIT_SLOTS} slots "
            f"-- the full call is not timed here")
        say()
        return
    form = radius.radius_form(B, N, cap)[2]
    res = {}
    names = ("count", "row_start", "total", "idx", "d2")
    lane_too = longest <= LANE_LONGEST
    contenders = [("count only", lambda: radius.grid_radius(xyz, r, 0, want_idx=False)),
                  (f"full, the plan's form ({'wave' if form == 1 else 'lane'})", lambda: res.__setitem__(0, radius.grid_radius(xyz, r, cap))),
                  ("full, a wave per row", lambda: res.__setitem__(1, radius.grid_radius(xyz, r, cap, variant=radius.variant(0, 1)))),
                  ("full, index order", lambda: res.__setitem__(3, radius.grid_radius(xyz, r, cap, variant=radius.variant(2, 0))))]
    if lane_too:
        contenders.insert(3, ("full, a lane per row", lambda: res.__setitem__(2, radius.grid_radius(xyz, r, cap, variant=radius.variant(0, 2)))))
    times = bg.race(tag, contenders, blocks)
    for k in res:
        assert same(res[k], res[0], names), k
    t = apart(lambda: res.__setitem__("torch", torch_search(xyz, r)))
    agree = sum(int(len(res["torch"][b][1]) == int(res[0]["total"][b])) for b in range(B))
    w, l = times["full, a wave per row"], times.get("full, a lane per row")
    full = times[contenders[1][0]]
    say(f"{tag} capacity {cap} a cloud, mean row {mean_row:.1f}, longest {longest}; torch cdist + nonzero + sorts {t:10.4f} ms/call (timed apart), "
        f"x{t / np.median(full):.1f} of the full call; its totals agree in {agree} of {B} clouds")
    if lane_too:
        say(f"{tag} ordering: {verdict(l, w, 'a lane per row', 'a wave per row')} (lane {np.median(l):.4f}, wave {np.median(w):.4f} ms)")
    else:
        say(f"{tag} ordering: the longest row has {longest} entries: a lane per row is not timed beyond {LANE_LONGEST}")
    split_line(tag, lambda: radius.grid_radius(xyz, r, cap))
    sweep = bg.race(tag + " edge", [(f"cell = {f:3.1f} x radius", lambda f=f: res.__setitem__(("e", f), radius.grid_radius(xyz, r, cap, cell=f * r)))
                                    for f in EDGES], blocks)
    for f in EDGES:
        assert same(res[("e", f)], res[0], names), f
    rule = sweep["cell = 1.0 x radius"]
    for f in EDGES:
        if f != 1.0:
            edge_wins.setdefault(("search", f), []).append((density, B, N, inside, bg.beats(sweep[f"cell = {f:3.1f} x radius"], rule)))
    say()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--blocks", type=int, default=5)
    ap.add_argument("--quick", action="store_true", help="the smallest shape only")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "radius_bench.txt"))
    a = ap.parse_args()
    say(f"# kernel_sources_sha16={build.sources_sha16()}")
    say(f"# profiles/bench_radius.py --blocks {a.blocks}: device {torch.cuda.get_device_name(0)}, "
        f"{torch.cuda.get_device_properties(0).multi_processor_count} CUs; ms per call = median of the blocks; nb_points = {NB_POINTS}")
    say()
    won, edge_wins = {}, {}
    for B, N in CASES[:1] if a.quick else CASES:
        for density in DENSITIES:
            for inside in INSIDE:
                bench_filter(density, B, N, inside, a.blocks, won, edge_wins)
                bench_search(density, B, N, inside, a.blocks, edge_wins)
    must = [key for key in won if key[2] == 131072 and key[0] in ("uniform", "surface")]
    say("# the condition (1 x 131 072, uniform and surface: the filter on the grid's slowest block below the scan's fastest): "
        + ("MET in every case" if must and all(won[key] for key in must) else "not run" if not must else
           "MISSED in " + ", ".join(str(key) for key in must if not won[key])))
    say("# where the filter on the grid does NOT beat the scan: " + (", ".join(str(key) for key in won if not won[key]) or "nowhere"))
    for (call, f), rows in sorted(edge_wins.items()):
        by_density = {d: [r[4] for r in rows if r[0] == d] for d in DENSITIES}
        everywhere = all(v and all(v) for v in by_density.values())
        say(f"# edge sweep, {call}: cell = {f:3.1f} x radius beats cell = radius beyond the spread in "
            f"{sum(r[4] for r in rows)} of {len(rows)} cases ({', '.join(f'{d} {sum(v)}/{len(v)}' for d, v in by_density.items())})"
            f"{': on ALL three densities, every case' if everywhere else ': not on all three densities -- the rule h = radius stands'}")
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        fh.write("\n".join(bg.LINES) + "\n")


if __name__ == "__main__":
    main()
