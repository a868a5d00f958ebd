#!/usr/bin/env python
"""Down-sampling on a voxel grid (vcr_voxel_f32) against what a user had before it: the same result in
torch device ops, cloud by cloud (three 21-bit cells fill the 64-bit key, so a batch cannot share one torch.unique): fp64
cells, torch.unique(return_inverse=True, return_counts=True), index_add_ in fp64 -- on the same GPU, the same inputs, in the
same process.  The contender keeps neither the voxels' order nor the sums'; its means must agree within 1 ulp of fp32.

Shapes (B, N): (16, 1024), (16, 16 384), (1, 131 072) on a uniform cube at about 8 points a voxel, and at (1, 131 072) the two
extremes: every point its own voxel, and one voxel.  Per shape: the automatic form, the scan forced into 1, 2, 4 ... 128 segments
(all bit-identical: asserted while timing) and the torch contender -- ms per call from device events around `--blocks` repeated
blocks of calls after a warm-up, contenders alternated block by block, each block's round starting at another contender and
each contender run once untimed before its block; the median block, the fastest and the slowest (their distance is the spread
every comparison is read against).  Then the per-kernel split of the automatic form from the profiler's kernel records.

  python profiles/bench_voxel.py [--blocks 5] [--quick] [--out profiles/voxel_bench.txt]
"""
import argparse
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import vcrnet_amd  # noqa: E402,F401
from vcrnet_amd import build, voxel  # noqa: E402

# (B, N, points per voxel or the name of an extreme)
CASES = ((16, 1024, 8.0), (16, 16384, 8.0), (1, 131072, 8.0), (1, 131072, "own"), (1, 131072, "one"))
OUTPUTS = ("points", "count", "point_voxel", "voxel_points")
LINES = []


def say(line=""):
    print(line, flush=True)
    LINES.append(line)


def torch_voxel(xyz, h):
    """The contender: per cloud (means [3, M] in key order, inverse [n finite], finite [N])."""
    out = []
    for x32 in xyz:
        finite = torch.isfinite(x32).all(0)
        x = x32[:, finite].double()
        origin = x.amin(1) - 0.5 * h
        c = torch.floor((x - origin[:, None]) / h).long()
        _, inv, cnt = torch.unique(c[2] << 42 | c[1] << 21 | c[0], return_inverse=True, return_counts=True)
        sums = torch.zeros(3, cnt.numel(), dtype=torch.float64, device=x.device).index_add_(1, inv, x)
        out.append(((sums / cnt).float(), inv, finite))
    return out


def timed(fn, calls):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(calls):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / calls


def kernel_split(fn, calls=5):
    """{kernel name: ms per call} of the voxel_ kernels over `calls` calls, from the profiler's device records."""
    from torch.profiler import ProfilerActivity, profile
    with profile(activities=[ProfilerActivity.CUDA]) as prof:
        for _ in range(calls):
            fn()
        torch.cuda.synchronize()
    split = {}
    for e in prof.key_averages():
        if "voxel_" in e.key:
            name = e.key[e.key.index("voxel_"):].split("(")[0]
            split[name] = split.get(name, 0.0) + getattr(e, "device_time_total", getattr(e, "cuda_time_total", 0.0)) / 1e3 / calls
    return split


def bench_case(B, N, per, blocks):
    rs = np.random.RandomState(B + N)
    xyz = torch.from_numpy(rs.uniform(-1, 1, (B, 3, N)).astype(np.float32)).cuda()
    h = {"own": 1e-5, "one": 100.0}[per] if isinstance(per, str) else float(np.float32(2.0 * (per / N) ** (1.0 / 3.0)))
    what = {"own": "every point its own voxel", "one": "one voxel"}[per] if isinstance(per, str) else f"~{per:g} points a voxel"
    cu = torch.cuda.get_device_properties(0).multi_processor_count
    res, seen, contenders = {}, set(), []
    for s in (0, 1, 2, 4, 8, 16, 32, 64, 128):
        form = voxel.voxel_form(B, N, cu_count=cu, variant=voxel.variant(s))[1]
        if s and form in seen:
            continue
        seen.add(form)
        name = ("auto = " if not s else "forced ") + f"S{form}"
        contenders.append((name, lambda s=s: res.__setitem__(s, voxel.voxel_grid(xyz, h, variant=voxel.variant(s)))))
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
    auto = res[0]
    for s in res:
        if s not in (0, "torch"):
            for k in OUTPUTS:
                assert torch.equal(auto[k].view(torch.int32), res[s][k].view(torch.int32)), (s, k)
    worst = 0.0
    for b, (means, inv, finite) in enumerate(res["torch"]):
        M = int(auto["count"][b])
        assert M == means.shape[1], (b, M, means.shape)
        mine = auto["points"][b][:, auto["point_voxel"][b][finite].long()]          # per finite point: its voxel's mean
        theirs = means[:, inv]
        ulp = (mine - theirs).abs() / torch.maximum(mine.abs(), theirs.abs()).clamp(min=1e-30) * 2.0 ** 23
        worst = max(worst, float(ulp.max()))
    assert worst <= 1.0, worst
    med = {n: float(np.median(v)) for n, v in times.items()}
    base = med[contenders[0][0]]
    tag = f"B={B:2d} N={N:6d} {what}:"
    for name, _ in contenders:
        v = times[name]
        say(f"{tag} {name:14s} {med[name]:10.4f} ms/call  (blocks min {min(v):.4f} max {max(v):.4f}; "
            f"{blocks} x {calls[name]} calls)  x{med[name] / base:8.2f} of auto")
    a = times[contenders[0][0]]
    best = min((n for n, _ in contenders[:-1]), key=lambda n: med[n])
    spread = max(a) - min(a)
    say(f"{tag} voxels {auto['count'].tolist()[:4]}{' ...' if B > 4 else ''}; torch / auto = x{med['torch unique'] / base:.2f}; "
        f"fastest form: {best} ({med[best]:.4f} ms, auto {base:.4f} ms, auto's spread {spread:.4f} ms"
        f"{'' if base - med[best] <= spread else ': BEATS auto by more than the spread'}); forms bit-identical; "
        f"means within {worst:.2f} ulp of torch's")
    split = kernel_split(contenders[0][1])
    total = sum(split.values())
    say(f"{tag} per kernel (auto): " + ", ".join(f"{k[6:-7]} {v:.4f}" for k, v in sorted(split.items(), key=lambda kv: -kv[1]))
        + f" ms; sum {total:.4f} ms")
    say()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--blocks", type=int, default=5)
    ap.add_argument("--quick", action="store_true", help="the smallest shape only")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "voxel_bench.txt"))
    a = ap.parse_args()
    say(f"# kernel_sources_sha16={build.sources_sha16()}")
    say(f"# profiles/bench_voxel.py --blocks {a.blocks}: device {torch.cuda.get_device_name(0)}, "
        f"{torch.cuda.get_device_properties(0).multi_processor_count} CUs; uniform cube [-1, 1]^3; ms per call = median of the blocks")
    say()
    for B, N, per in CASES[:1] if a.quick else CASES:
        bench_case(B, N, per, a.blocks)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        fh.write("\n".join(LINES) + "\n")


if __name__ == "__main__":
    main()
