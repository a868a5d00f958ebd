#!/usr/bin/env python
"""The voxel grid by a radix sort (vcr_voxel_sort_f32) against the scan form (vcr_voxel_f32, section
4.11) and against the torch contender of profiles/bench_voxel.py (torch.unique + index_add_ in fp64, cloud by cloud) -- on the
same GPU, the same inputs, in the same process, on the five rows of section 4.11's table.

Per row: the scan form (its plan's), the sort form at the plan's digit width and at every forced width (all bit-identical to the
scan form: asserted while timing) and the torch contender -- section 4.8's protocol: ms per call from device events around
`--blocks` repeated blocks of calls after a warm-up, contenders alternated block by block, each block's round starting at another
contender and each contender run once untimed before its block; the median block, the fastest and the slowest.  The SPREAD of a
row is the larger of the scan's and the sort's (max - min over their blocks): the sort "wins" only by more than that.  Then the
per-kernel split of the sort form at the plan's width from the profiler's kernel records.  Last, scan against sort alone on
sizes between the rows: where the sort starts to win.

  python profiles/bench_voxel_sort.py [--blocks 5] [--quick] [--out profiles/voxel_sort_bench.txt]
"""
import argparse
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import vcrnet_amd  # noqa: E402,F401
from vcrnet_amd import build, voxel, voxel_sort  # noqa: E402
from bench_voxel import CASES, OUTPUTS, timed, torch_voxel  # noqa: E402

CROSSOVER = ((1, 2048), (1, 4096), (1, 8192), (1, 16384), (1, 32768), (16, 2048), (16, 4096), (16, 8192))   # (B, N)
LINES = []


def say(line=""):
    print(line, flush=True)
    LINES.append(line)


def kernel_split(fn, calls=5):
    """{kernel name: ms per call} of the sort form's kernels over `calls` calls, from the profiler's device records."""
    from torch.profiler import ProfilerActivity, profile
    with profile(activities=[ProfilerActivity.CUDA]) as prof:
        for _ in range(calls):
            fn()
        torch.cuda.synchronize()
    split = {}
    for e in prof.key_averages():
        for tag in ("vs_", "rs_"):
            if tag in e.key:
                name = e.key[e.key.index(tag):].split("(")[0].split("<")[0]
                split[name] = split.get(name, 0.0) + getattr(e, "device_time_total", getattr(e, "cuda_time_total", 0.0)) / 1e3 / calls
                break
    return split


def bench_case(B, N, per, blocks, widths=True):
    rs = np.random.RandomState(B + N)
    xyz = torch.from_numpy(rs.uniform(-1, 1, (B, 3, N)).astype(np.float32)).cuda()
    h = {"own": 1e-5, "one": 100.0}[per] if isinstance(per, str) else float(np.float32(2.0 * (per / N) ** (1.0 / 3.0)))
    what = {"own": "every point its own voxel", "one": "one voxel"}[per] if isinstance(per, str) else f"~{per:g} points a voxel"
    plan = voxel_sort.voxel_sort_form(B, N)[0]
    res = {}
    contenders = [("scan (auto)", lambda: res.__setitem__("scan", voxel.voxel_grid(xyz, h))),
                  (f"sort plan=d{plan}", lambda: res.__setitem__(0, voxel_sort.voxel_grid_sort(xyz, h)))]
    for d in voxel_sort.DIGIT_BITS if widths else ():
        contenders.append((f"sort forced d{d}", lambda d=d: res.__setitem__(d, voxel_sort.voxel_grid_sort(xyz, h, digit_bits=d))))
    contenders.append(("torch unique", lambda: res.__setitem__("torch", torch_voxel(xyz, h))))
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
    for s in res:
        if s not in ("scan", "torch"):
            for k in OUTPUTS:
                assert torch.equal(res["scan"][k].view(torch.int32), res[s][k].view(torch.int32)), (s, k)
    med = {n: float(np.median(v)) for n, v in times.items()}
    scan, sort = contenders[0][0], contenders[1][0]
    tag = f"B={B:2d} N={N:6d} {what}:"
    for name, _ in contenders:
        v = times[name]
        say(f"{tag} {name:16s} {med[name]:10.4f} ms/call  (blocks min {min(v):.4f} max {max(v):.4f}; "
            f"{blocks} x {calls[name]} calls)  x{med[name] / med[scan]:8.3f} of scan")
    spread = max(max(times[scan]) - min(times[scan]), max(times[sort]) - min(times[sort]))
    gain = med[scan] - med[sort]
    verdict = ("sort FASTER than scan by more than the spread" if gain > spread else
               "sort SLOWER than scan by more than the spread" if -gain > spread else "sort and scan within the spread")
    best = min((n for n, _ in contenders[1:-1]), key=lambda n: med[n])
    say(f"{tag} voxels {res['scan']['count'].tolist()[:4]}{' ...' if B > 4 else ''}; scan / sort = x{med[scan] / med[sort]:.2f} "
        f"(scan - sort = {gain:.4f} ms, spread {spread:.4f} ms: {verdict}); sort / torch = x{med[sort] / med['torch unique']:.2f}; "
        f"fastest width: {best} ({med[best]:.4f} ms); all forms bit-identical to the scan's")
    if not widths:
        say()
        return
    split = kernel_split(contenders[1][1])
    total = sum(split.values())
    say(f"{tag} per kernel ({sort}): " + ", ".join(f"{k[:-7]} {v:.4f}" for k, v in sorted(split.items(), key=lambda kv: -kv[1]))
        + f" ms; sum {total:.4f} ms")
    say()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--blocks", type=int, default=5)
    ap.add_argument("--quick", action="store_true", help="the smallest shape only")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "voxel_sort_bench.txt"))
    a = ap.parse_args()
    say(f"# kernel_sources_sha16={build.sources_sha16()}")
    say(f"# profiles/bench_voxel_sort.py --blocks {a.blocks}: device {torch.cuda.get_device_name(0)}, "
        f"{torch.cuda.get_device_properties(0).multi_processor_count} CUs; uniform cube [-1, 1]^3; ms per call = median of the blocks")
    say()
    for B, N, per in CASES[:1] if a.quick else CASES:
        bench_case(B, N, per, a.blocks)
    if not a.quick:
        say("# the crossover: scan and sort (the plan's width) alone, ~8 points a voxel")
        say()
        for B, N in CROSSOVER:
            bench_case(B, N, 8.0, a.blocks, widths=False)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        fh.write("\n".join(LINES) + "\n")


if __name__ == "__main__":
    main()
