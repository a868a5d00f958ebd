#!/usr/bin/env python
"""Normals and FPFH over ragged radius rows (vcr_rows_normals_f32, vcr_rows_spfh_f32, vcr_rows_fpfh_f32),
on one GPU, in one process:

  the passes   each of the three on the rows ``search_radius`` returns, the two FPFH passes in both launch forms (a lane a row,
               a wave a row; bit-identical, asserted while timing)
  end to end   compute_fpfh_feature(search="radius", max_nn=30) against the parent's nearest equivalent,
               compute_fpfh_feature(k=30, radius=r, search="grid"), on the same clouds
  torch        the same result in torch device ops over the flat pair list (repeat_interleave, fp64 pair features, index_add) at
               about 100 entries a row, timed apart

Shapes (B, N): (16, 1024), (16, 16 384), (1, 131 072); two densities: a uniform cube and a sphere's surface
(profiles/bench_grid.py's clouds); four radii, for about 12, 30, 100 and 330 points a row (the mean and the longest row are
printed).  Per case: ms per call from device events around `--blocks` repeated blocks of calls after a warm-up, contenders
alternated block by block, each block's round starting at another contender and each contender run once untimed before its
block (section 4.8's protocol); the median block, the fastest and the slowest.  A contender "beats" another when its SLOWEST
block is below the other's FASTEST.  The closing lines collect, per pass, the cases in which the wave form beats the lane form:
vcr_rows_form's thresholds (VCR_ROWS_WAVE_SPFH / VCR_ROWS_WAVE_FPFH) are read off them.

  python profiles/bench_rows.py [--blocks 5] [--quick] [--out profiles/rows_bench.txt]
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
from vcrnet_amd import build, fpfh, native, radius, rows  # noqa: E402
import bench_grid as bg  # noqa: E402  (the clouds, the race and the spread rule)

CASES = ((16, 1024), (16, 16384), (1, 131072))
DENSITIES = ("uniform", "surface")
INSIDE = (12, 30, 100, 330)
say = bg.say


def radius_for(density, N, inside):
    """About `inside` other points within reach: of a uniform cube [-1, 1]^3 of N points, or of the unit sphere's surface."""
    if density == "uniform":
        return float(np.float32(2.0 * (3.0 * inside / (4.0 * np.pi * N)) ** (1.0 / 3.0)))
    return float(np.float32(2.0 * math.sqrt(inside / N)))


def torch_rows_fpfh(xyz4, nrm, csr):
    """The contender: fpfh float32 [B,33,N] from the same rows and normals, over each cloud's flat pair list."""
    idx, row_start, total = csr
    B, N, _ = xyz4.shape
    out = []
    for b in range(B):
        x, n = xyz4[b, :, :3], nrm[b].t()
        T = int(total[b])
        count = (row_start[b, 1:] - row_start[b, :-1])
        i = torch.repeat_interleave(torch.arange(N, device=x.device), count)
        j = idx[b, :T].long()
        d = (x[j] - x[i]).double()
        n1, n2 = n[i].double(), n[j].double()
        d2 = (d * d).sum(-1)
        L = d2.sqrt()
        a1, a2 = (n1 * d).sum(-1) / L, (n2 * d).sum(-1) / L
        swap = a1.abs() < a2.abs()
        s = swap[:, None]
        n1, n2, d = torch.where(s, n2, n1), torch.where(s, n1, n2), torch.where(s, -d, d)
        f2 = torch.where(swap, -a2, a1)
        v = torch.linalg.cross(d, n1)
        vn = v.norm(dim=-1)
        zero = (L == 0) | (vn == 0)
        v = v / vn[:, None]
        w = torch.linalg.cross(n1, v)
        f1 = (v * n2).sum(-1)
        f0 = torch.atan2((w * n2).sum(-1), (n1 * n2).sum(-1))
        coord = torch.stack([11.0 * (f0 + math.pi) / (2.0 * math.pi), 11.0 * (f1 + 1.0) * 0.5, 11.0 * (f2 + 1.0) * 0.5], -1)
        coord = torch.where(zero[:, None], torch.full_like(coord, 5.5), coord)
        bins = coord.floor().nan_to_num(0.0).clamp(0, 10).long() + torch.tensor([0, 11, 22], device=x.device)
        counts = torch.zeros(N, 33, dtype=torch.float64, device=x.device)
        counts.view(-1).index_add_(0, (i[:, None] * 33 + bins).view(-1), torch.ones(T * 3, dtype=torch.float64, device=x.device))
        c = count.double().clamp(min=1)[:, None]
        own = counts * (100.0 / c)
        wgt = torch.where(d2 > 0, 1.0 / d2, torch.zeros_like(d2))              # a neighbour at distance 0 is skipped
        acc = torch.zeros(N, 33, dtype=torch.float64, device=x.device).index_add_(0, i, own[j] * wgt[:, None]).view(N, 3, 11)
        tot = acc.sum(-1, keepdim=True)
        acc = torch.where(tot != 0, acc * (100.0 / tot), acc).view(N, 33)
        out.append((acc + own).float().t())
    return torch.stack(out).contiguous()


def eq(a, b):
    return torch.equal(a.view(torch.int32), b.view(torch.int32))


def bench_passes(density, B, N, inside, blocks, wins):
    xyz = bg.cloud(density, B, N, B + N + inside)
    r = radius_for(density, N, inside)
    tag = f"passes {density:8s} B={B:2d} N={N:6d} inside={inside:3d}:"
    csr = radius.search_radius(xyz, r)
    n_i = (csr[1][:, 1:] - csr[1][:, :-1])
    mean_row, longest, cap = n_i.float().mean().item(), int(n_i.max()), csr[0].shape[1]
    x4 = native.to_rows4(xyz)
    nrm = rows.normals(x4, *csr, want_curvature=False)[0]
    res = {}
    sp = rows.spfh(x4, nrm, *csr)
    plan = rows.form(B, N, cap)
    names = {1: "lane", 2: "wave"}
    say(f"{tag} radius {r:.5f}, capacity {cap} a cloud, mean row {mean_row:.1f}, longest {longest}; the plan's forms: first pass "
        f"{names[plan[0]]}, second pass {names[plan[1]]}")
    times = bg.race(tag, [("normals (a lane a row)", lambda: rows.normals(x4, *csr, want_curvature=False)),
                          ("spfh, a lane a row", lambda: res.__setitem__("sl", rows.spfh(x4, nrm, *csr, variant="lane"))),
                          ("spfh, a wave a row", lambda: res.__setitem__("sw", rows.spfh(x4, nrm, *csr, variant="wave"))),
                          ("fpfh, a lane a row", lambda: res.__setitem__("fl", rows.fpfh(x4, *csr, sp, variant="lane"))),
                          ("fpfh, a wave a row", lambda: res.__setitem__("fw", rows.fpfh(x4, *csr, sp, variant="wave")))], blocks)
    assert torch.equal(res["sl"], res["sw"]) and torch.equal(res["sl"], sp) and eq(res["fl"], res["fw"])
    for what, lane, wave in (("spfh", "spfh, a lane a row", "spfh, a wave a row"), ("fpfh", "fpfh, a lane a row", "fpfh, a wave a row")):
        l, w = times[lane], times[wave]
        verdict = ("the wave form BEATS the lane form beyond the spread" if bg.beats(w, l) else
                   "the lane form BEATS the wave form beyond the spread" if bg.beats(l, w) else "within the blocks' spread")
        say(f"{tag} {what}: lane / wave = x{np.median(l) / np.median(w):.2f}; wave's slowest block {max(w):.4f} ms, lane's fastest "
            f"{min(l):.4f} ms: {verdict}")
        wins.setdefault(what, []).append((density, B, N, inside, round(mean_row, 1), cap // N, bg.beats(w, l), bg.beats(l, w)))
    say()
    return xyz, r, csr, x4, nrm


def bench_end_to_end(tag, xyz, r, blocks):
    res = {}
    times = bg.race(tag, [('compute_fpfh_feature(search="radius", max_nn=30)',
                           lambda: res.__setitem__("rows", fpfh.compute_fpfh_feature(xyz, search="radius", radius=r, max_nn=30))),
                          ('compute_fpfh_feature(k=30, radius=r, search="grid") (the parent\'s)',
                           lambda: res.__setitem__("grid", fpfh.compute_fpfh_feature(xyz, k=30, radius=r, search="grid")))], blocks)
    a, b = (times[k] for k in times)
    alike = (res["rows"].view(torch.int32) == res["grid"].view(torch.int32)).all(1).float().mean().item()
    verdict = ("the rows path BEATS the fixed-width path beyond the spread" if bg.beats(a, b) else
               "the fixed-width path BEATS the rows path beyond the spread" if bg.beats(b, a) else "within the blocks' spread")
    say(f"{tag} rows / fixed-width = x{np.median(a) / np.median(b):.2f}: {verdict}; points with the same 33 values bit for bit: {alike:.4f} "
        f"(the fixed-width path estimates its normals from all k neighbours, the rows path from the row: they differ where the radius cuts)")
    say()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--blocks", type=int, default=5)
    ap.add_argument("--quick", action="store_true", help="the smallest shape only")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "rows_bench.txt"))
    a = ap.parse_args()
    say(f"# kernel_sources_sha16={build.sources_sha16()}")
    say(f"# profiles/bench_rows.py --blocks {a.blocks}: device {torch.cuda.get_device_name(0)}, "
        f"{torch.cuda.get_device_properties(0).multi_processor_count} CUs; ms per call = median of the blocks; thresholds in this "
        f"build: first pass {rows.WAVE_SPFH}, second pass {rows.WAVE_FPFH}")
    say()
    wins = {}
    for B, N in CASES[:1] if a.quick else CASES:
        for density in DENSITIES:
            for inside in INSIDE:
                xyz, r, csr, x4, nrm = bench_passes(density, B, N, inside, a.blocks, wins)
                if inside in (30, 100):
                    bench_end_to_end(f"end to end {density:8s} B={B:2d} N={N:6d} inside={inside:3d}:", xyz, r, a.blocks)
                if inside == 100:
                    tag = f"torch {density:8s} B={B:2d} N={N:6d} inside={inside:3d}:"
                    mine = rows.fpfh(x4, *csr, rows.spfh(x4, nrm, *csr))
                    torch.cuda.synchronize()
                    t_mine = bg.timed(lambda: rows.fpfh(x4, *csr, rows.spfh(x4, nrm, *csr)), 3)
                    theirs = torch_rows_fpfh(x4, nrm, csr)
                    torch.cuda.synchronize()
                    t = bg.timed(lambda: torch_rows_fpfh(x4, nrm, csr), 2)
                    say(f"{tag} the two passes {t_mine:.4f} ms, torch device ops on the same rows and normals {t:.4f} ms/call (timed apart): "
                        f"x{t / t_mine:.1f}; max |difference| {(mine - theirs).abs().max().item():.3e}")
                    say()
                del xyz, csr, x4, nrm
                torch.cuda.empty_cache()
    for what, rows_ in wins.items():
        say(f"# {what}: the wave form beats the lane form beyond the spread at (density, B, N, inside, mean row, capacity / N): "
            + (", ".join(str(k[:6]) for k in rows_ if k[6]) or "nowhere"))
        say(f"# {what}: the lane form beats the wave form beyond the spread at: " + (", ".join(str(k[:6]) for k in rows_ if k[7]) or "nowhere"))
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        fh.write("\n".join(bg.LINES) + "\n")


if __name__ == "__main__":
    main()
