#!/usr/bin/env python
"""Scoring and refining on the target's grid (include/vcr_hip_gridnn.h) against the SCAN form -- the
brute-force nn_scan_kernel every call ran before it, unchanged -- on the same clouds, on the same GPU, in the same process.

Protocol (section 4.8's, profiles/bench_grid.py's): ms per call from device events around `--blocks` repeated blocks of calls
after a warm-up, contenders alternated block by block, each block's round starting at another contender and each contender
run once untimed before its block; the median block, the fastest and the slowest.  A contender "beats" another when its
SLOWEST block is below the other's FASTEST.  Every grid result is compared with the scan's while timing (inliers, sum_d2,
fitness, rmse and poses bit for bit).

  a  one evaluation (nn_score) and refinement rounds (refine, ROUNDS updates with thresholds 0: no cloud converges; a round =
     the call / (ROUNDS + 1)) at B x N = 16 x 1024, 16 x 16 384, 1 x 131 072 (Ns = Nt = N): a full-overlap pair and a
     partial-overlap pair with a third of the source far from the target; a uniform cube, a sphere's surface, eight blobs;
     the scan, the grid with order 1 (the source's cell order) and with order 2 (index order); max_dist = two automatic edges.
     The once-a-call build -- the target's grid, the source's permutation -- from the profiler's kernel records.
  b  a whole refine_registration at its defaults, the three methods, on the plane benchmark's clouds (a torus, source and
     target drawn independently, a planted 40-degree pose, a start 6 degrees and 0.04 off; normals estimated beforehand):
     ms and rounds, scan against grid.
  c  a max_dist sweep at 0.5, 1, 2, 4, 8 and 16 times the target's automatic edge h (1 x 131 072 source points, the three
     densities) on a pair whose partner-less third lies INSIDE the target's box -- the target lacks the middle third of its
     points along x, so the source points in the gap walk rings until the cap stops them --: the scan, the grid on the
     automatic edge, and the grid with the edge tied to max_dist.
  d  the crossover in points a cloud: B = 1 and B = 16, N = 256 ... 65 536, uniform, full overlap, max_dist = 2 h.

  python profiles/bench_gridnn.py [--part abcd] [--blocks 5] [--out profiles/gridnn_bench.txt] [--append]
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
from vcrnet_amd import build, plane, refine, score  # noqa: E402

CASES = ((16, 1024), (16, 16384), (1, 131072))
DENSITIES = ("uniform", "surface", "clustered")
ROUNDS = 4
SWEEP = (0.5, 1.0, 2.0, 4.0, 8.0, 16.0)
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


def cloud(rs, density, B, N):
    """bench_grid.py's three densities, float64 [B,3,N]."""
    if density == "uniform":
        return rs.uniform(-1, 1, (B, 3, N))
    if density == "surface":
        x = rs.normal(size=(B, 3, N))
        return x / np.linalg.norm(x, axis=1, keepdims=True)
    centres = rs.uniform(-1, 1, (B, 3, 8))
    pick = rs.randint(0, 8, (B, N))
    return np.take_along_axis(centres, np.broadcast_to(pick[:, None, :], (B, 3, N)), 2) + rs.normal(size=(B, 3, N)) * 0.02


def auto_edge(x):
    """The header's automatic edge of cloud 0 of a numpy batch (before any widening)."""
    e = x[0].max(1) - x[0].min(1)
    live = e[e > 0]
    return float((np.prod(live) / x.shape[2]) ** (1.0 / len(live)))


def pair(density, B, N, partial, seed):
    """-> (src, tgt, R0, t0, h): the target; the source = the target's points, permuted, jittered by a tenth of the automatic edge
    h and carried into a frame of its own -- with `partial`, a third of them first moved three extents away along x; with
    partial = "hole" the target instead loses the middle third of its points along x (Nt = N - N // 3), so a third of the
    source has no partner INSIDE the target's box --; the start (R0, t0) = the way back, half a degree and h / 2 off."""
    rs = np.random.RandomState(seed)
    tgt = cloud(rs, density, B, N)
    h = auto_edge(tgt)
    own = tgt[:, :, rs.permutation(N)] + rs.normal(size=(B, 3, N)) * 0.1 * h
    if partial == "hole":
        rank = np.argsort(np.argsort(tgt[:, 0], axis=1), axis=1)
        keep = (rank < N // 3) | (rank >= 2 * (N // 3))
        tgt = np.stack([tgt[b][:, keep[b]] for b in range(B)])
        h = auto_edge(tgt)
    elif partial:
        own[:, 0, : N // 3] += 3.0 * (tgt[:, 0].max() - tgt[:, 0].min())
    src, R0, t0 = [], [], []
    for b in range(B):
        R, t = rotation(rs.normal(size=3), 40.0), rs.uniform(-0.5, 0.5, 3)
        src.append(R.T @ (own[b] - t[:, None]))                             # tgt ~ R src + t
        d = rs.normal(size=3)
        R0.append(R @ rotation(rs.normal(size=3), 0.5)); t0.append(t + 0.5 * h * d / np.linalg.norm(d))
    f = lambda v: torch.from_numpy(np.ascontiguousarray(np.stack(v) if isinstance(v, list) else v).astype(np.float32)).cuda()   # noqa: E731
    return f(src), f(tgt), f(R0), f(t0), h


def timed(fn, calls):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(calls):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / calls


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
        say(f"{tag} {name:28s} {np.median(v):10.4f} ms/call  (blocks min {min(v):.4f} max {max(v):.4f}; "
            f"{blocks} x {calls[name]} calls)  x{base / np.median(v):8.2f} the first's speed")
    return times


def beats(a, b):
    return max(a) < min(b)


def verdict(g, s):
    return "the grid BEATS the scan beyond the spread" if beats(g, s) else \
        "the scan BEATS the grid beyond the spread" if beats(s, g) else "within the blocks' spread"


def kernel_split(fn, calls=5):
    """{kernel name: ms per call} of the grid_ kernels over `calls` calls, from the profiler's device records."""
    from torch.profiler import ProfilerActivity, profile
    with profile(activities=[ProfilerActivity.CUDA]) as prof:
        for _ in range(calls):
            fn()
        torch.cuda.synchronize()
    split = {}
    for e in prof.key_averages():
        m = re.search(r"(grid_\w+_kernel)", e.key)
        if m:
            t = getattr(e, "device_time_total", getattr(e, "cuda_time_total", 0.0)) / 1e3 / calls
            split[m.group(1)] = split.get(m.group(1), 0.0) + t
    return split


def same(a, b, keys):
    for k in keys:
        x, y = a[k], b[k]
        assert torch.equal(x.view(torch.int32) if x.dtype == torch.float32 else x.view(torch.int64) if x.dtype == torch.float64 else x,
                           y.view(torch.int32) if y.dtype == torch.float32 else y.view(torch.int64) if y.dtype == torch.float64 else y), k


SCORE_KEYS = ("inliers", "sum_d2", "fitness", "rmse")
REFINE_KEYS = SCORE_KEYS + ("R", "t", "iterations", "converged")


def score_contenders(src, tgt, R0, t0, max_dist, res, forms):
    """forms: (name, kwargs of the grid form, or None = the scan)."""
    def one(name, kw):
        return (name, lambda: res.__setitem__(name, score.nn_score(src, tgt, R0, t0, max_dist, want_nn=False,
                                                                    **({} if kw is None else dict(kw, search="grid")))))
    return [one(name, kw) for name, kw in forms]


def part_a(blocks):
    say(f"## a. one evaluation and one refinement round (refine: {ROUNDS} updates, thresholds 0), max_dist = 2 automatic edges")
    for B, N in CASES:
        for density in DENSITIES:
            for partial in (False, True):
                src, tgt, R0, t0, h = pair(density, B, N, partial, B + N + partial)
                max_dist = 2.0 * h
                tag = f"{density:9s} {'partial' if partial else 'full   '} B={B:2d} N={N:6d}:"
                res = {}
                forms = [("score scan", None), ("score grid order 1", dict(order=1)), ("score grid order 2", dict(order=2))]
                t = race(tag, score_contenders(src, tgt, R0, t0, max_dist, res, forms), blocks)
                for name, _ in forms[1:]:
                    same(res[name], res["score scan"], SCORE_KEYS)
                kw = dict(max_iterations=ROUNDS, rel_fitness=0.0, rel_rmse=0.0, want_nn=False)
                rforms = [("refine scan", {}), ("refine grid order 1", dict(search="grid", order=1)),
                          ("refine grid order 2", dict(search="grid", order=2))]
                rt = race(tag, [(name, lambda name=name, g=g: res.__setitem__(name, refine.refine(src, tgt, R0, t0, max_dist, **kw, **g)))
                                for name, g in rforms], blocks)
                for name, _ in rforms[1:]:
                    same(res[name], res["refine scan"], REFINE_KEYS)
                fit = res["score scan"]["fitness"].float().mean().item()
                s1, g1, g2 = (np.median(t[n]) for n, _ in forms)
                r0, r1, r2 = (np.median(rt[n]) / (ROUNDS + 1) for n, _ in rforms)
                say(f"{tag} fitness {fit:.3f}; evaluation scan / grid = x{s1 / g1:.2f} (order 1), x{s1 / g2:.2f} (order 2): "
                    f"{verdict(t['score grid order 1'], t['score scan'])}; order 1 against order 2: "
                    f"{'order 1 wins' if beats(t['score grid order 1'], t['score grid order 2']) else 'order 2 wins' if beats(t['score grid order 2'], t['score grid order 1']) else 'within the spread'}")
                say(f"{tag} a round: scan {r0:.4f}, grid order 1 {r1:.4f}, order 2 {r2:.4f} ms: x{r0 / r1:.2f}, x{r0 / r2:.2f}: "
                    f"{verdict(rt['refine grid order 1'], rt['refine scan'])}; order 1 against order 2: "
                    f"{'order 1 wins' if beats(rt['refine grid order 1'], rt['refine grid order 2']) else 'order 2 wins' if beats(rt['refine grid order 2'], rt['refine grid order 1']) else 'within the spread'}")
                two = kernel_split(lambda: score.nn_score(src, tgt, R0, t0, max_dist, want_nn=False, search="grid", order=2))
                one = kernel_split(lambda: score.nn_score(src, tgt, R0, t0, max_dist, want_nn=False, search="grid", order=1))
                build2 = sum(v for n, v in two.items() if n != "grid_nn_kernel")
                build1 = sum(v for n, v in one.items() if n != "grid_nn_kernel")
                say(f"{tag} kernels: the target's grid (five launches) {build2:.4f} ms, the source's permutation (six) "
                    f"{build1 - build2:.4f} ms, once a call; grid_nn_kernel {one.get('grid_nn_kernel', 0):.4f} ms (order 1), "
                    f"{two.get('grid_nn_kernel', 0):.4f} ms (order 2)")
                say()


def torus(rs, n):
    """profiles/bench_plane.py's torus: [3, n] float64 inside the unit cube."""
    u, v = rs.uniform(0, 2 * np.pi, n), rs.uniform(0, 2 * np.pi, n)
    r = 0.12 * (1 + 0.3 * np.sin(5 * u) * np.cos(3 * v))
    ring = 0.33 + r * np.cos(v)
    return np.stack([0.5 + ring * np.cos(u), 0.5 + ring * np.sin(u), 0.5 + r * np.sin(v) + 0.05 * np.sin(2 * u)])


def part_b(blocks):
    say("## b. a whole refine_registration at its defaults on the plane benchmark's clouds (the torus, source and target drawn "
        "independently; normals estimated beforehand)")
    for B, N, max_dist in ((4, 2048, 0.1), (4, 16384, 0.05), (1, 131072, 0.02)):
        rs = np.random.RandomState(N)
        src_n, tgt_n, R0_n, t0_n = [], [], [], []
        for b in range(B):
            R, t = rotation(rs.normal(size=3), 40.0), rs.uniform(-0.5, 0.5, 3)
            d = rs.normal(size=3)
            src_n.append(torus(rs, N))
            tgt_n.append(R @ torus(rs, N) + t[:, None])
            R0_n.append(R @ rotation(rs.normal(size=3), 6.0)); t0_n.append(t + 0.04 * d / np.linalg.norm(d))
        f = lambda v: torch.from_numpy(np.stack(v).astype(np.float32)).cuda()   # noqa: E731
        src, tgt, R0, t0 = f(src_n), f(tgt_n), f(R0_n), f(t0_n)
        search = "grid" if N > 16384 else "knn"
        ns, nt = plane.estimate_normals(src, 20, search=search), plane.estimate_normals(tgt, 20, search=search)
        for method in refine.METHODS:
            kw = dict(method=method)
            if method != "point_to_point":
                kw["tgt_normals"] = nt
            if method == "generalized":
                kw["src_normals"] = ns
            res = {}
            tag = f"B={B} N={N:6d} max_dist {max_dist} {method:15s}:"
            t = race(tag, [(s, lambda s=s: res.__setitem__(s, vcrnet_amd.refine_registration(src, tgt, R0, t0, max_dist=max_dist,
                                                                                              search=s, **kw))) for s in ("scan", "grid")], blocks)
            same(res["grid"], res["scan"], ("R", "t", "fitness", "inlier_rmse", "inliers", "iterations", "converged"))
            say(f"{tag} updates {res['scan']['iterations'].tolist()} converged {res['scan']['converged'].tolist()} fitness "
                f"{res['scan']['fitness'].cpu().numpy().round(3).tolist()}; scan / grid = x{np.median(t['scan']) / np.median(t['grid']):.2f}: "
                f"{verdict(t['grid'], t['scan'])}; all outputs bit-identical")
        say()


def part_c(blocks):
    say("## c. max_dist sweep (1 x 131 072 source points; the target lacks its middle third along x): the scan, the grid on the "
        "automatic edge h, the grid on an edge tied to max_dist")
    B, N = CASES[2]
    tied_wins = {}
    for density in DENSITIES:
        src, tgt, R0, t0, h = pair(density, B, N, "hole", 77)
        for f in SWEEP:
            max_dist = f * h
            res = {}
            forms = [("scan", None), ("grid, automatic edge", dict())]
            if f > 1:
                forms.append(("grid, edge = max_dist", dict(cell=max_dist)))
                forms.append(("grid, edge = max_dist / 2", dict(cell=max_dist / 2)))
            tag = f"{density:9s} max_dist = {f:4.1f} h ({max_dist:.5f}):"
            t = race(tag, score_contenders(src, tgt, R0, t0, max_dist, res, forms), blocks)
            for name, _ in forms[1:]:
                same(res[name], res["scan"], SCORE_KEYS)
            line = f"{tag} fitness {res['scan']['fitness'].item():.3f}; scan / grid (automatic) = x{np.median(t['scan']) / np.median(t['grid, automatic edge']):.2f}: " \
                   f"{verdict(t['grid, automatic edge'], t['scan'])}"
            if f > 1:
                for name in ("grid, edge = max_dist", "grid, edge = max_dist / 2"):
                    w = beats(t[name], t["grid, automatic edge"])
                    tied_wins.setdefault(name, []).append((density, f, w))
                    line += f"; {name}: x{np.median(t['grid, automatic edge']) / np.median(t[name]):.2f} of the automatic edge" \
                            f"{' (BEATS it beyond the spread)' if w else ''}"
            say(line)
        say()
    for name, rows in tied_wins.items():
        per = {d: all(w for dd, _, w in rows if dd == d) for d in DENSITIES}
        say(f"# {name}: beats the automatic edge beyond the spread at every max_dist > h on: "
            f"{[d for d in DENSITIES if per[d]] or 'no density'}")
    say()


def part_d(blocks):
    say("## d. the crossover in points a cloud (uniform, full overlap, max_dist = 2 h; the plan's order)")
    for B in (1, 16):
        for N in (256, 512, 1024, 2048, 4096, 8192, 16384, 32768, 65536):
            if B * N > 16 * 32768:
                continue
            src, tgt, R0, t0, h = pair("uniform", B, N, False, B + N)
            max_dist = 2.0 * h
            res = {}
            tag = f"B={B:2d} N={N:6d}:"
            t = race(tag, score_contenders(src, tgt, R0, t0, max_dist, res, [("score scan", None), ("score grid", dict())]), blocks)
            same(res["score grid"], res["score scan"], SCORE_KEYS)
            kw = dict(max_iterations=ROUNDS, rel_fitness=0.0, rel_rmse=0.0, want_nn=False)
            rt = race(tag, [("refine scan", lambda: res.__setitem__("rs", refine.refine(src, tgt, R0, t0, max_dist, **kw))),
                            ("refine grid", lambda: res.__setitem__("rg", refine.refine(src, tgt, R0, t0, max_dist, search="grid", **kw)))],
                      blocks)
            same(res["rg"], res["rs"], REFINE_KEYS)
            say(f"{tag} evaluation scan / grid = x{np.median(t['score scan']) / np.median(t['score grid']):.2f} "
                f"({verdict(t['score grid'], t['score scan'])}); {ROUNDS + 1} rounds scan / grid = "
                f"x{np.median(rt['refine scan']) / np.median(rt['refine grid']):.2f} ({verdict(rt['refine grid'], rt['refine scan'])})")
        say()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--part", default="abcd")
    ap.add_argument("--blocks", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "gridnn_bench.txt"))
    ap.add_argument("--append", action="store_true")
    a = ap.parse_args()
    say(f"# kernel_sources_sha16={build.sources_sha16()}")
    say(f"# profiles/bench_gridnn.py --part {a.part} --blocks {a.blocks}: device {torch.cuda.get_device_name(0)}, "
        f"{torch.cuda.get_device_properties(0).multi_processor_count} CUs; ms per call = median of the blocks")
    say()
    for p, fn in (("a", part_a), ("b", part_b), ("c", part_c), ("d", part_d)):
        if p in a.part:
            fn(a.blocks)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "a" if a.append else "w") as fh:
        fh.write("\n".join(LINES) + "\n")


if __name__ == "__main__":
    main()
