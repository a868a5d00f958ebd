#!/usr/bin/env python
"""Moving least squares over ragged radius rows (vcr_mls_weights_f32, vcr_mls_fit_f32, ``smooth_mls``), on
one GPU, in one process:

  the launches    stage A (the origins and the weights) and stage B (the fit) with both combines -- every sum through the six
                  exchanges, and the transposing one; bit-identical, asserted while timing -- on the rows ``search_radius`` returns
  the whole call  smooth_mls(xyz, radius, normals, capacity=...) against search_radius alone on the same cloud: the search's share
  torch           the same points from torch device ops on the same rows padded to the longest -- a gather, the frame, exp, einsum
                  for the 6 x 6 systems, torch.linalg.cholesky_ex and cholesky_solve -- compared with the kernels' points (the
                  largest difference: another order of summation, not the same bits) and timed apart

Shapes (B, N): (16, 1024), (16, 16 384), (1, 131 072); two clouds: a uniform cube (its normals estimated over the same rows: a
volume has none, the passes do not care) and a sphere's surface with its own normals (profiles/bench_grid.py's clouds); two radii
a cloud, chosen for rows of about 12 and about 100 entries.  Per case: ms per call from device events around `--blocks` repeated
blocks of calls after a warm-up, contenders alternated block by block (section 4.8's protocol); the median block, the fastest and
the slowest.  A contender "beats" another when its SLOWEST block is below the other's FASTEST.  The closing lines collect where
either combine beats the other: the plan's combine is read off them.

  python profiles/bench_mls.py [--blocks 5] [--quick] [--out profiles/mls_bench.txt]
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
from vcrnet_amd import build, mls, native, radius, rows  # noqa: E402
import bench_grid as bg  # noqa: E402  (the clouds, the race and the spread rule)

CASES = ((16, 1024), (16, 16384), (1, 131072))
DENSITIES = ("uniform", "surface")
ROWS = (12, 100)
MIN_NEIGHBORS = 3
say = bg.say


def radius_for(density, N, entries):
    """The radius at which a point away from the cloud's edge has about `entries` neighbours."""
    if density == "uniform":                                # N points in a cube of volume 8
        return (entries * 8.0 * 3.0 / (4.0 * math.pi * N)) ** (1.0 / 3.0)
    return math.sqrt(4.0 * entries / N)                     # N points on a sphere of area 4 pi


def torch_mls(xyz, normals, csr, h2):
    """The yardstick: (points [B,3,N], fit [B,N]) from the same rows by torch device ops, order 2."""
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
    uh = torch.nn.functional.normalize(torch.linalg.cross(nh, e), dim=2)
    v = torch.linalg.cross(nh, uh)
    m = (n + 1).double()
    mu = (d * used[..., None]).sum(2) / m[..., None]
    o = (mu * nh).sum(2, keepdim=True) * nh                 # [B,N,3]
    q = torch.cat([d - o[:, :, None, :], -o[:, :, None, :]], 2)                  # the entries, then the point itself
    w = torch.exp(-(q * q).sum(3) / h2) * torch.cat([used, torch.ones_like(used[:, :, :1])], 2)
    uu, vv, f = (q * uh[:, :, None, :]).sum(3), (q * v[:, :, None, :]).sum(3), (q * nh[:, :, None, :]).sum(3)
    P = torch.stack([torch.ones_like(uu), vv, vv * vv, uu, uu * vv, uu * uu], 3)
    A = torch.einsum("bnwa,bnw,bnwc->bnac", P, w, P)
    r = torch.einsum("bnwa,bnw,bnw->bna", P, w, f)
    L, info = torch.linalg.cholesky_ex(A)
    c = torch.cholesky_solve(r[..., None], torch.where((info == 0)[..., None, None], L, torch.eye(6, dtype=L.dtype, device=dev)))
    quad = (info == 0) & (n + 1 >= 6)
    c0 = torch.where(quad, c[:, :, 0, 0], torch.zeros_like(c[:, :, 0, 0]))
    moved = (p.double() + (o + c0[..., None] * nh)).float()
    fit = torch.where(n + 1 >= MIN_NEIGHBORS, torch.where(quad, 2, 1), 0)
    return torch.where((fit > 0)[..., None], moved, p).transpose(1, 2), fit


def bench_case(tag, density, xyz, entries, blocks, wins, key):
    B, _, N = xyz.shape
    r = radius_for(density, N, entries)
    h2 = r * r
    csr = radius.search_radius(xyz, r)
    idx, row_start, total = csr
    n_i = row_start[:, 1:] - row_start[:, :-1]
    cap, mean_row, longest = idx.shape[1], n_i.float().mean().item(), int(n_i.max())
    xyz4 = native.to_rows4(xyz)
    normals = xyz.clone() if density == "surface" else rows.normals(xyz4, *csr, want_curvature=False)[0]
    out = {}
    say(f"{tag} radius {r:.5f}, capacity {cap} a cloud (est {cap // N}), mean row {mean_row:.1f}, longest {longest}")
    a_call = lambda: out.__setitem__("a", mls.weights_rows(xyz4, normals, *csr, h2))  # noqa: E731
    a_call()
    b_call = lambda v: out.__setitem__(v, mls.fit_rows(xyz4, normals, *csr, out["a"]["weight"], out["a"]["origin"],  # noqa: E731
                                                       out["a"]["w_self"], out["a"]["frame"], 2, MIN_NEIGHBORS, variant=v))
    times = bg.race(tag, [("stage A (origins, weights)", a_call), ("stage B, plain combine", lambda: b_call("plain")),
                          ("stage B, transposing combine", lambda: b_call("transpose"))], blocks)
    for k in ("points", "fit", "normals", "coeffs"):
        assert torch.equal(out["plain"][k].view(torch.uint8), out["transpose"][k].view(torch.uint8)), k
    fit = out["plain"]["fit"]
    say(f"{tag} fit 2 / 1 / 0: {int((fit == 2).sum())} / {int((fit == 1).sum())} / {int((fit == 0).sum())} of {B * N}")
    pl, tr = times["stage B, plain combine"], times["stage B, transposing combine"]
    wins.append(key + (round(mean_row, 1), cap // N, round(float(np.median(pl) / np.median(tr)), 2), bg.beats(tr, pl), bg.beats(pl, tr)))
    whole = lambda: out.__setitem__("whole", mls.smooth_mls(xyz, r, normals, capacity=cap))  # noqa: E731
    t = bg.race(tag, [("smooth_mls", whole), ("search_radius", lambda: radius.search_radius(xyz, r, capacity=cap))], blocks)
    assert torch.equal(out["whole"][1], fit)
    tw, ts = (float(np.median(t[k])) for k in t)
    say(f"{tag} the search is {100 * ts / tw:.1f} % of smooth_mls")
    mine = float(np.median(times["stage A (origins, weights)"])) + min(float(np.median(pl)), float(np.median(tr)))
    theirs, tfit = torch_mls(xyz, normals, csr, h2)
    torch.cuda.synchronize()
    tt = bg.timed(lambda: torch_mls(xyz, normals, csr, h2), 2)
    again, afit = torch_mls(xyz, normals, csr, h2)          # the yardstick against itself, and the kernels against themselves
    first = {k: v.clone() for k, v in out["plain"].items()}
    b_call("plain")
    for k in ("points", "fit", "normals", "coeffs"):
        assert torch.equal(out["plain"][k].view(torch.uint8), first[k].view(torch.uint8)), k
    steady = (afit == tfit).float().mean().item()
    moved = ((again - theirs).abs().amax(1) > 0).float().mean().item()
    if steady < 1.0 or moved > 0.0:
        say(f"{tag} torch's result is not the same twice: fit codes that repeat {100 * steady:.3f} %, points that moved "
            f"{100 * moved:.3f} % (the kernels' outputs repeat bit for bit)")
    del again, afit, first
    both = (tfit == 2) & (fit == 2)
    diff = (theirs - out["plain"]["points"]).abs().amax(1)[both].max().item() if both.any() else float("nan")
    say(f"{tag} torch device ops on the same rows {tt:.3f} ms/call, the two stages {mine:.4f} ms (timed apart): x{tt / mine:.1f}; "
        f"fit codes that agree {100 * (tfit == fit).float().mean().item():.3f} %, largest coordinate difference where both fit "
        f"the quadratic {diff:.3g}")
    del theirs, tfit
    torch.cuda.empty_cache()
    say()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--blocks", type=int, default=5)
    ap.add_argument("--quick", action="store_true", help="the smallest shape only")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mls_bench.txt"))
    a = ap.parse_args()
    say(f"# kernel_sources_sha16={build.sources_sha16()}")
    say(f"# profiles/bench_mls.py --blocks {a.blocks}: device {torch.cuda.get_device_name(0)}, "
        f"{torch.cuda.get_device_properties(0).multi_processor_count} CUs; ms per call = median of the blocks")
    say()
    wins = []
    for density in DENSITIES:
        for B, N in CASES[:1] if a.quick else CASES:
            xyz = bg.cloud(density, B, N, B + N)
            for entries in ROWS:
                bench_case(f"{density:8s} B={B:2d} N={N:6d} rows~{entries:3d}:", density, xyz, entries, a.blocks, wins, (density, B, N))
            del xyz
            torch.cuda.empty_cache()
    say("# stage B: plain / transposing at (cloud, B, N, mean row, capacity / N, ratio): " + ", ".join(str(k[:6]) for k in wins))
    say("# stage B: the transposing combine beats the plain one beyond the spread at: " + (", ".join(str(k[:6]) for k in wins if k[6]) or "nowhere"))
    say("# stage B: the plain combine beats the transposing one beyond the spread at: " + (", ".join(str(k[:6]) for k in wins if k[7]) or "nowhere"))
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        fh.write("\n".join(bg.LINES) + "\n")


if __name__ == "__main__":
    main()
