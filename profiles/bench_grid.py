#!/usr/bin/env python
"""The grid kNN (vcr_grid_knn_f32) against the search its consumers had before it: native.knn, the
brute-force kNN, on the same clouds' xyz4 rows, on the same GPU, in the same process.

Shapes (B, N): (16, 1024), (16, 16 384), (1, 131 072); k = 20 and 30; three densities: a uniform cube, a sphere's surface (what a
scan looks like, and what a dense grid serves worst) and a clustered cloud (eight blobs).  Per case: ms per call from device
events around `--blocks` repeated blocks of calls after a warm-up, contenders alternated block by block, each block's round
starting at another contender and each contender run once untimed before its block (section 4.8's protocol); the median block,
the fastest and the slowest.  A contender "beats" another when its SLOWEST block is below the other's FASTEST.

Per case also: the grid call's per-kernel split from the profiler's kernel records; a sweep of forced cell edges around the
automatic one, and the queries served in index order instead of cell order -- every one of them bit-identical to the automatic
form (asserted while timing).  Then estimate_normals (k = 20) and compute_fpfh_feature (k = 30) end to end with both searches.

  python profiles/bench_grid.py [--blocks 5] [--quick] [--out profiles/grid_bench.txt]
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
from vcrnet_amd import build, fpfh, grid, native, plane  # noqa: E402

CASES = ((16, 1024), (16, 16384), (1, 131072))
KS = (20, 30)
SWEEP = (0.5, 0.707, 1.414, 2.0, 2.828)                     # forced edges, as multiples of the automatic one
LINES = []


def say(line=""):
    print(line, flush=True)
    LINES.append(line)


def cloud(density, B, N, seed):
    rs = np.random.RandomState(seed)
    if density == "uniform":
        x = rs.uniform(-1, 1, (B, 3, N))
    elif density == "surface":
        x = rs.normal(size=(B, 3, N))
        x /= np.linalg.norm(x, axis=1, keepdims=True)
    else:                                                   # clustered: eight blobs of sigma 0.02 in the cube
        centres = rs.uniform(-1, 1, (B, 3, 8))
        pick = rs.randint(0, 8, (B, N))
        x = np.take_along_axis(centres, np.broadcast_to(pick[:, None, :], (B, 3, N)), 2) + rs.normal(size=(B, 3, N)) * 0.02
    return torch.from_numpy(x.astype(np.float32)).cuda()


def auto_edge(xyz):
    """The header's automatic edge of cloud 0 (before any widening): (V / N)^(1 / D) over the axes that are not flat."""
    e = (xyz[0].max(1).values - xyz[0].min(1).values).double().cpu().numpy()
    live = e[e > 0]
    return float((np.prod(live) / xyz.shape[2]) ** (1.0 / len(live)))


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
        say(f"{tag} {name:24s} {np.median(v):10.4f} ms/call  (blocks min {min(v):.4f} max {max(v):.4f}; "
            f"{blocks} x {calls[name]} calls)  x{np.median(v) / base:8.2f} of the first")
    return times


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


def beats(a, b):
    return max(a) < min(b)


def bench_search(density, B, N, k, blocks):
    xyz = cloud(density, B, N, B + N + k)
    rows = native.to_rows4(xyz)
    res = {}
    tag = f"{density:9s} B={B:2d} N={N:6d} k={k}:"
    times = race(tag, [("grid (automatic)", lambda: res.__setitem__("grid", grid.search_knn(xyz, k))),
                       ("native.knn (brute force)", lambda: res.__setitem__("knn", native.knn(rows, None, k)))], blocks)
    g, b = times["grid (automatic)"], times["native.knn (brute force)"]
    same = (res["grid"].sort(2).values == res["knn"].sort(2).values).all(2).float().mean().item()
    verdict = "the grid BEATS the brute force beyond the spread" if beats(g, b) else \
        "the brute force BEATS the grid beyond the spread" if beats(b, g) else "within the blocks' spread"
    say(f"{tag} brute force / grid = x{np.median(b) / np.median(g):.2f}; grid's slowest block {max(g):.4f} ms, brute force's fastest "
        f"{min(b):.4f} ms: {verdict}; rows with the same neighbour set: {same:.6f}")
    split = kernel_split(lambda: grid.search_knn(xyz, k))
    say(f"{tag} per kernel: " + ", ".join(f"{n} {v:.4f}" for n, v in sorted(split.items(), key=lambda kv: -kv[1]))
        + f" ms; sum {sum(split.values()):.4f} ms")
    h = auto_edge(xyz)
    auto = res["grid"]

    def forced(f=None, variant=0):
        o = grid.grid_knn(xyz, k, 0.0 if f is None else f * h, want_d2=False, variant=variant)["idx"]
        res[(f, variant)] = o
    contenders = [("automatic", lambda: forced())] + [(f"cell = {f:5.3f} x automatic", lambda f=f: forced(f)) for f in SWEEP]
    contenders.append(("automatic, index order", lambda: forced(None, grid.variant(2))))
    sweep = race(tag + " sweep", contenders, blocks)
    for key, o in res.items():
        if isinstance(key, tuple):
            assert torch.equal(o, auto), key
    a = sweep["automatic"]
    best = min((n for n, _ in contenders[:-1]), key=lambda n: float(np.median(sweep[n])))
    say(f"{tag} sweep: automatic edge {h:.5f}; fastest edge: {best} ({np.median(sweep[best]):.4f} ms, automatic {np.median(a):.4f} ms"
        f"{': BEATS the automatic edge beyond the spread' if best != 'automatic' and beats(sweep[best], a) else ': within the spread of the automatic edge' if best != 'automatic' else ''}"
        f"); all forms bit-identical")
    say()
    return beats(g, b)


def bench_consumers(density, B, N, blocks):
    xyz = cloud(density, B, N, B + N + 7)
    res = {}
    tag = f"{density:9s} B={B:2d} N={N:6d}:"
    times = race(tag, [('estimate_normals k=20 grid', lambda: res.__setitem__(0, plane.estimate_normals(xyz, 20, search="grid"))),
                       ('estimate_normals k=20 knn', lambda: res.__setitem__(1, plane.estimate_normals(xyz, 20, search="knn"))),
                       ('compute_fpfh k=30 grid', lambda: res.__setitem__(2, fpfh.compute_fpfh_feature(xyz, None, 30, search="grid"))),
                       ('compute_fpfh k=30 knn', lambda: res.__setitem__(3, fpfh.compute_fpfh_feature(xyz, None, 30, search="knn")))], blocks)
    med = {n: float(np.median(v)) for n, v in times.items()}
    nk, ng, fk, fg = (med[n] for n in ("estimate_normals k=20 knn", "estimate_normals k=20 grid", "compute_fpfh k=30 knn", "compute_fpfh k=30 grid"))
    say(f"{tag} estimate_normals knn / grid = x{nk / ng:.2f}; compute_fpfh_feature knn / grid = x{fk / fg:.2f}")
    say()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--blocks", type=int, default=5)
    ap.add_argument("--quick", action="store_true", help="the smallest shape only")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "grid_bench.txt"))
    a = ap.parse_args()
    say(f"# kernel_sources_sha16={build.sources_sha16()}")
    say(f"# profiles/bench_grid.py --blocks {a.blocks}: device {torch.cuda.get_device_name(0)}, "
        f"{torch.cuda.get_device_properties(0).multi_processor_count} CUs; ms per call = median of the blocks")
    say()
    won = {}
    for B, N in CASES[:1] if a.quick else CASES:
        for density in ("uniform", "surface", "clustered"):
            for k in KS:
                won[(density, B, N, k)] = bench_search(density, B, N, k, a.blocks)
    for B, N in CASES[:1] if a.quick else CASES:
        for density in ("uniform", "surface"):
            bench_consumers(density, B, N, a.blocks)
    must = [key for key in won if key[2] == 131072 and key[0] in ("uniform", "surface")]
    say("# the condition (1 x 131 072, uniform and surface: the grid's slowest block below the brute force's fastest): "
        + ("MET in every case" if must and all(won[key] for key in must) else "not run" if not must else
           "MISSED in " + ", ".join(str(key) for key in must if not won[key])))
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        fh.write("\n".join(LINES) + "\n")


if __name__ == "__main__":
    main()
