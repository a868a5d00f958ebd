#!/usr/bin/env python
"""Boundary points over ragged radius rows (vcr_border_angles_f32, vcr_border_gap_f32, vcr_border_near_f32,
``compute_boundary_points``), on one GPU, in one process:

  the launches    the angles pass (a wave a row, its only form), the gap pass in both forms (a lane a row, a wave a row;
                  bit-identical, asserted while timing) and the spreading, on the rows ``search_radius`` returns
  the whole call  compute_boundary_points(xyz, normals, radius, max_nn=None, capacity=...) against search_radius alone on the
                  same cloud: the search's share of the call
  torch           the same flags from torch device ops on the same rows padded to the longest -- a gather, the frame, atan2,
                  sort, diff, max -- compared with the kernels' flags (the share of points that agree: another atan2 and a
                  sorted difference, not the same bits) and timed apart

Shapes (B, N): (16, 1024), (16, 16 384), (1, 131 072); two clouds: a uniform cube (its normals estimated over the same rows: a
volume has none, the pass does not care) and a sphere's surface with its own normals (profiles/bench_grid.py's clouds); two radii
a cloud, chosen for rows of about 12 and about 100 entries.  Per case: ms per call from device events around `--blocks` repeated
blocks of calls after a warm-up, contenders alternated block by block (section 4.8's protocol); the median block, the fastest and
the slowest.  A contender "beats" another when its SLOWEST block is below the other's FASTEST.  The closing lines collect where
either form of the gap pass beats the other: vcr_border_form's threshold is read off them.

  python profiles/bench_border.py [--blocks 5] [--quick] [--out profiles/border_bench.txt]
"""
import argparse
import math
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import vcrnet_amd  # noqa: E402,F401
from vcrnet_amd import border, build, native, radius, rows  # noqa: E402
import bench_grid as bg  # noqa: E402  (the clouds, the race and the spread rule)

CASES = ((16, 1024), (16, 16384), (1, 131072))
DENSITIES = ("uniform", "surface")
ROWS = (12, 100)
THRESHOLD = border.radians(90.0)
MIN_NEIGHBORS = 3
say = bg.say


def radius_for(density, N, entries):
    """The radius at which a point away from the cloud's edge has about `entries` neighbours."""
    if density == "uniform":                                # N points in a cube of volume 8
        return (entries * 8.0 * 3.0 / (4.0 * math.pi * N)) ** (1.0 / 3.0)
    return math.sqrt(4.0 * entries / N)                     # N points on a sphere of area 4 pi


def torch_border(xyz, normals, csr):
    """The yardstick: flags bool [B,N] from the same rows by torch device ops."""
    idx, row_start, total = csr
    B, _, N = xyz.shape
    dev = xyz.device
    n = row_start[:, 1:] - row_start[:, :-1]
    W = max(int(n.max()), 1)
    slot = torch.arange(W, device=dev)[None, None, :]
    used = slot < n[:, :, None]
    at = (row_start[:, :N, None] + slot).clamp(max=idx.shape[1] - 1)
    j = torch.where(used, torch.gather(idx, 1, at.view(B, -1)).view(B, N, W).long(), torch.arange(N, device=dev)[None, :, None])
    p = xyz.transpose(1, 2)                                 # [B,N,3]
    d = (torch.gather(p, 1, j.view(B, -1, 1).expand(-1, -1, 3)).view(B, N, W, 3) - p[:, :, None, :]).double()
    nh = torch.nn.functional.normalize(normals.transpose(1, 2).double(), dim=2)
    e = torch.nn.functional.one_hot(nh.abs().argmin(2), 3).double()
    u = torch.linalg.cross(nh, e)
    v = torch.linalg.cross(nh, u)
    pu, pv = (d * u[:, :, None, :]).sum(3), (d * v[:, :, None, :]).sum(3)
    counted = used & ((pu != 0) | (pv != 0))
    inf = torch.full((), float("inf"), dtype=torch.float64, device=dev)
    a = torch.where(counted, torch.atan2(pv, pu), inf).sort(2).values
    c = counted.sum(2)
    step = torch.where(torch.isfinite(a[:, :, 1:]), a[:, :, 1:] - a[:, :, :-1], -inf).amax(2) if W > 1 else torch.full_like(a[:, :, 0], -1.0)
    last = torch.gather(a, 2, (c - 1).clamp(min=0)[:, :, None])[:, :, 0]
    gap = torch.maximum(step, (2.0 * math.pi - last) + a[:, :, 0])
    return (n + 1 >= MIN_NEIGHBORS) & (c > 0) & (gap > THRESHOLD)


def bench_case(tag, density, xyz, entries, blocks, wins, key):
    B, _, N = xyz.shape
    r = radius_for(density, N, entries)
    idx, row_start, total, d2 = radius.search_radius(xyz, r, want_d2=True)
    csr = (idx, row_start, total)
    n_i = row_start[:, 1:] - row_start[:, :-1]
    cap, mean_row, longest = idx.shape[1], n_i.float().mean().item(), int(n_i.max())
    xyz4 = native.to_rows4(xyz)
    normals = xyz.clone() if density == "surface" else rows.normals(xyz4, *csr, want_curvature=False)[0]
    out = {}
    names = {1: "lane", 2: "wave"}
    say(f"{tag} radius {r:.5f}, capacity {cap} a cloud (est {cap // N}), mean row {mean_row:.1f}, longest {longest}; "
        f"the plan's form: {names[border.form(B, N, cap)]}")
    ang_call = lambda: out.__setitem__("a", border.angles_rows(xyz4, normals, *csr, want_frame=True))  # noqa: E731
    ang_call()
    gap_call = lambda v: out.__setitem__(v, border.gap_rows(out["a"]["angle"], row_start, total, MIN_NEIGHBORS, THRESHOLD,  # noqa: E731
                                                            frame=out["a"]["frame"], variant=v))
    gap_call("lane")
    near_call = lambda: out.__setitem__("near", border.near_rows(out["lane"]["flag"], *csr)["near"])  # noqa: E731
    times = bg.race(tag, [("angles (a wave a row)", ang_call), ("gap, a lane a row", lambda: gap_call("lane")),
                          ("gap, a wave a row", lambda: gap_call("wave")), ("near (a lane a row)", near_call)], blocks)
    assert torch.equal(out["lane"]["flag"], out["wave"]["flag"])
    assert torch.equal(out["lane"]["gap"].view(torch.int64), out["wave"]["gap"].view(torch.int64))
    flagged = int((out["lane"]["flag"] > 0).sum())
    say(f"{tag} boundary points {flagged} of {B * N}, near them {int((out['near'] > 0).sum())}")
    l, w = times["gap, a lane a row"], times["gap, a wave a row"]
    wins.append(key + (round(mean_row, 1), cap // N, round(float(np.median(l) / np.median(w)), 2), bg.beats(w, l), bg.beats(l, w)))
    whole = lambda: out.__setitem__("whole", border.compute_boundary_points(xyz, normals, r, max_nn=None, capacity=cap, want_flag=True))  # noqa: E731
    t = bg.race(tag, [("compute_boundary_points", whole), ("search_radius", lambda: radius.search_radius(xyz, r, capacity=cap))], blocks)
    assert torch.equal(out["whole"][3], out["lane"]["flag"])
    tw, ts = (float(np.median(t[k])) for k in t)
    say(f"{tag} the search is {100 * ts / tw:.1f} % of compute_boundary_points")
    mine = float(np.median(times["angles (a wave a row)"])) + min(float(np.median(l)), float(np.median(w)))
    theirs = torch_border(xyz, normals, csr)
    torch.cuda.synchronize()
    tt = bg.timed(lambda: torch_border(xyz, normals, csr), 2)
    agree = (theirs == (out["lane"]["flag"] > 0)).float().mean().item()
    say(f"{tag} torch device ops on the same rows {tt:.3f} ms/call, the two passes {mine:.4f} ms (timed apart): x{tt / mine:.1f}; "
        f"flags that agree {100 * agree:.3f} %, torch boundary points {int(theirs.sum())}")
    say()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--blocks", type=int, default=5)
    ap.add_argument("--quick", action="store_true", help="the smallest shape only")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "border_bench.txt"))
    a = ap.parse_args()
    say(f"# kernel_sources_sha16={build.sources_sha16()}")
    say(f"# profiles/bench_border.py --blocks {a.blocks}: device {torch.cuda.get_device_name(0)}, "
        f"{torch.cuda.get_device_properties(0).multi_processor_count} CUs; ms per call = median of the blocks; threshold in this "
        f"build: gap wave from est {border.WAVE_GAP}")
    say()
    wins = []
    for density in DENSITIES:
        for B, N in CASES[:1] if a.quick else CASES:
            xyz = bg.cloud(density, B, N, B + N)
            for entries in ROWS:
                bench_case(f"{density:8s} B={B:2d} N={N:6d} rows~{entries:3d}:", density, xyz, entries, a.blocks, wins, (density, B, N))
            del xyz
            torch.cuda.empty_cache()
    say("# gap: lane / wave at (cloud, B, N, mean row, capacity / N, ratio): " + ", ".join(str(k[:6]) for k in wins))
    say("# gap: the wave form beats the lane form beyond the spread at: " + (", ".join(str(k[:6]) for k in wins if k[6]) or "nowhere"))
    say("# gap: the lane form beats the wave form beyond the spread at: " + (", ".join(str(k[:6]) for k in wins if k[7]) or "nowhere"))
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        fh.write("\n".join(bg.LINES) + "\n")


if __name__ == "__main__":
    main()
