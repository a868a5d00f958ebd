#!/usr/bin/env python
"""The RANSAC plane fit (vcr_plane_ransac_f32, ``segment_plane``), on one GPU, in one process:

  the whole call  segment.plane_ransac in the plan's form and with each form forced (bit-identical, asserted while timing)
  the count       the count launch alone, from the profiler's device records, in both forms over a ladder of split counts; with
                  it the device time of the call's other launches: the share of the call spent outside the count
  torch           the same counts and the same winner in torch device ops from the SAME trial planes: per chunk of trials a
                  [T,4] x [4,N] product (the plane (n, -n.p0) against homogeneous points), abs() <= thr, sum; then argmax.  Its
                  distances are not the header's bit for bit (a GEMM's own order, no differences), so its counts may differ by
                  the points that lie on the threshold; the number of trials whose count differs is printed, nothing asserted

Shapes (B, N): (16, 1024), (16, 16 384), (1, 131 072); T in {100, 1 000, 10 000}; clouds: half the points near a plane, half
uniform in the unit cube.  Per case: ms per call from device events around `--blocks` repeated blocks of calls after a warm-up,
contenders alternated block by block (section 4.8's protocol); the median block, the fastest and the slowest.  A contender
"beats" another when its SLOWEST block is below the other's FASTEST.  The closing lines collect, per shape, the fastest count
launch of each form: vcr_plane_ransac_form's thresholds are read off them.

  python profiles/bench_segment.py [--blocks 5] [--quick] [--out profiles/segment_bench.txt]
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
from vcrnet_amd import build, segment  # noqa: E402
import bench_grid as bg  # noqa: E402  (the race and the spread rule)

CASES = ((16, 1024), (16, 16384), (1, 131072))
TRIALS = (100, 1000, 10000)
THR = 0.02
say = bg.say


def cloud(B, N, seed):
    rs = np.random.RandomState(seed)
    x = rs.uniform(0, 1, (B, 3, N))
    near = rs.uniform(size=(B, N)) < 0.5
    x[:, 2] = np.where(near, 0.3 * x[:, 0] - 0.2 * x[:, 1] + 0.4 + rs.uniform(-0.01, 0.01, (B, N)), x[:, 2])
    return torch.from_numpy(x.astype(np.float32)).cuda()


def kernel_split(fn, calls=3):
    """{kernel name: ms per call} of the plane_ kernels over `calls` calls, from the profiler's device records."""
    from torch.profiler import ProfilerActivity, profile
    with profile(activities=[ProfilerActivity.CUDA]) as prof:
        for _ in range(calls):
            fn()
        torch.cuda.synchronize()
    split = {}
    for e in prof.key_averages():
        m = re.search(r"(plane_[a-z_]+_kernel)", e.key)
        if m:
            t = getattr(e, "device_time_total", getattr(e, "cuda_time_total", 0.0)) / 1e3 / calls
            split[m.group(1)] = split.get(m.group(1), 0.0) + t
    return split


def torch_counts(xyz, rows, status, chunk=1024):
    """(count int64 [B,T], best [B]) from the trial planes rows [B,T,8] by GEMM-shaped device ops."""
    B, _, N = xyz.shape
    hom = torch.cat([xyz, torch.ones(B, 1, N, device=xyz.device)], 1)               # [B,4,N]
    n, p0 = rows[..., 0:3], rows[..., 4:7]
    planes = torch.cat([n, -(n * p0).sum(-1, keepdim=True)], -1)                    # [B,T,4]
    out = []
    for lo in range(0, rows.shape[1], chunk):
        out.append(((planes[:, lo:lo + chunk] @ hom).abs() <= THR).sum(-1))
    count = torch.where(status == 0, torch.cat(out, 1), torch.full_like(status, -1).long())
    return count, count.argmax(1)


def ladder(form, B, N, T):
    plan = segment.form(B, N, T, variant=form)[1]
    if form == "trial":
        steps = {1, 4, 16, 64, plan}
        return sorted(s for s in steps if s == plan or s <= max(1, N // 64))
    return sorted({max(1, plan // 4), max(1, plan // 2), plan, min(segment.MAX_SPLITS, 2 * plan)})


def bench(B, N, T, blocks, best):
    xyz = cloud(B, N, B + N + T)
    tag = f"B={B:2d} N={N:6d} T={T:5d}:"
    names = {1: "trial", 2: "point"}
    plan = segment.form(B, N, T, cu_count=torch.cuda.get_device_properties(0).multi_processor_count)
    res = {}
    call = lambda v, k, trials=False: res.__setitem__(k, segment.plane_ransac(xyz, THR, 3, T, 1, want_trials=trials, variant=v))  # noqa: E731
    call(0, "full", True)
    say(f"{tag} the plan: {names[plan[0]]} form, {plan[1]} splits; workspace {plan[2]} B; winner's inliers a cloud "
        f"{res['full']['count'].float().mean().item():.0f}, valid trials {100 * (res['full']['trial_status'] == 0).float().mean().item():.1f} %")
    times = bg.race(tag, [("whole call, the plan's", lambda: call(0, "plan")), ("whole call, TRIAL form", lambda: call("trial", "trial")),
                          ("whole call, POINT form", lambda: call("point", "point"))], blocks)
    for k in ("plane", "inlier", "count", "best_trial"):
        assert torch.equal(res["plan"][k].view(torch.int32), res["trial"][k].view(torch.int32)), k
        assert torch.equal(res["plan"][k].view(torch.int32), res["point"][k].view(torch.int32)), k
    t_plan = float(np.median(times["whole call, the plan's"]))
    fastest = {}
    for form in ("trial", "point"):
        for s in ladder(form, B, N, T):
            split = kernel_split(lambda: call((form, s), "v"))
            count = sum(t for k, t in split.items() if "count" in k)
            rest = sum(t for k, t in split.items() if "count" not in k)
            mark = "  <- the plan" if (segment.FORMS[form], s) == plan[:2] else ""
            say(f"{tag} count launch, {form:5s} form, {s:3d} splits: {count:8.4f} ms; the other launches {rest:.4f} ms "
                f"({100 * rest / (count + rest):.0f} % of the device time){mark}")
            assert torch.equal(res["v"]["count"], res["plan"]["count"])
            if form not in fastest or count < fastest[form][1]:
                fastest[form] = (s, round(count, 4))
            if mark:
                others = ", ".join(f"{k[6:-7]} {t:.4f}" for k, t in sorted(split.items()) if "count" not in k)
                say(f"{tag} the plan's other launches: {others} ms")
    rows, status = res["full"]["trial_plane"], res["full"]["trial_status"]
    theirs, their_best = torch_counts(xyz, rows, status)
    torch.cuda.synchronize()
    off = int((theirs != res["full"]["trial_count"]).sum())
    t_torch = bg.timed(lambda: torch_counts(xyz, rows, status), 3)
    same = bool((their_best == res["full"]["best_trial"]).all())
    say(f"{tag} torch device ops from the same planes {t_torch:.4f} ms/call (counts and argmax only), the whole call {t_plan:.4f} ms "
        f"(timed apart): torch / call = x{t_torch / t_plan:.2f}; trials whose count differs {off} of {B * T}, the same winner: {same}")
    say()
    best.append((B, N, T, names[plan[0]], plan[1], fastest["trial"], fastest["point"], round(t_plan, 4), round(t_torch, 4)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--blocks", type=int, default=5)
    ap.add_argument("--quick", action="store_true", help="the smallest shape only")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "segment_bench.txt"))
    a = ap.parse_args()
    say(f"# kernel_sources_sha16={build.sources_sha16()}")
    say(f"# profiles/bench_segment.py --blocks {a.blocks}: device {torch.cuda.get_device_name(0)}, "
        f"{torch.cuda.get_device_properties(0).multi_processor_count} CUs; ms per call = median of the blocks; the plan in this build: "
        f"POINT from {segment.POINT_MIN_N} points a cloud or {segment.POINT_MIN_T} trials, TRIAL below with {segment.FILL} workgroups a CU and ranges of "
        f"{segment.TRIAL_MIN_RANGE} points or more")
    say()
    best = []
    for B, N in CASES[:1] if a.quick else CASES:
        for T in TRIALS:
            bench(B, N, T, a.blocks, best)
            torch.cuda.empty_cache()
    say("# per shape (B, N, T, the plan's form, its splits, fastest TRIAL (splits, ms), fastest POINT (splits, ms), whole call ms, torch ms):")
    for row in best:
        say("#   " + str(row))
    say("# the library loses to torch (whole call slower than torch's counts and argmax) at: "
        + (", ".join(str(r[:3]) for r in best if r[7] > r[8]) or "nowhere"))
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        fh.write("\n".join(bg.LINES) + "\n")


if __name__ == "__main__":
    main()
