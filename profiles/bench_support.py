#!/usr/bin/env python
"""Normals and FPFH at centres over a support cloud (vcr_support_*_f32), on one GPU, in one process:

  plans        compute_fpfh_feature(query_index=) under support="all" and support="needed" against the yardstick, the PARENT's
               compute_fpfh_feature(search="radius") of the whole cloud plus a gather of the asked columns (the same bits,
               asserted while timing); with given normals, and with estimated ones (where only "all" exists)
  parts        the query search, the self search, vcr_support_needed_f32, the search from the needed points, the centres' first
               pass in both launch forms (bit-identical, asserted), the second pass
  end to end   register_features(keypoints="iss") with describe="all" against describe="keypoints"

Shapes (B, N): (16, 1024), (16, 16 384), (1, 131 072); a uniform cube and a sphere's surface (profiles/bench_grid.py's clouds);
radii for about 12, 30 and 100 points a row (and 20 for the forms); M in (N / 100, N / 10, N) as a random subset of the points.
Every search takes an explicit capacity (read once, untimed), so no contender synchronises.  Per case: ms per call from device
events by profiles/bench_grid.py's race -- warm-up, contenders alternated block by block, the median block, the fastest and the
slowest; a contender "beats" another when its SLOWEST block is below the other's FASTEST.  The closing lines collect the coverage
(needed points / N) of every case with the plans' verdict, and est = capacity / M with the forms' verdict: the two thresholds
(VCR_SUPPORT_COVERAGE_PCT, VCR_SUPPORT_WAVE_SPFH) are read off them.

  python profiles/bench_support.py [--blocks 3] [--quick] [--out profiles/support_bench.txt]
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
from vcrnet_amd import build, fpfh, iss, match, native, radius, rows, support  # noqa: E402
import bench_grid as bg  # noqa: E402  (the clouds, the race and the spread rule)
from bench_rows import radius_for  # noqa: E402

CASES = ((16, 1024), (16, 16384), (1, 131072))
DENSITIES = ("uniform", "surface")
INSIDE = (12, 20, 30, 100)
SHARES = (100, 10, 1)                                       # M = N / share
say = bg.say


def eq(a, b):
    return torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


def verdict(a, b, na, nb):
    return f"{na} BEATS {nb} beyond the spread" if bg.beats(a, b) else f"{nb} BEATS {na} beyond the spread" if bg.beats(b, a) \
        else "within the blocks' spread"


def bench_case(density, B, N, inside, share, blocks, plans, forms):
    xyz = bg.cloud(density, B, N, B + N + inside)
    r = radius_for(density, N, inside)
    M = max(1, N // share)
    rs = np.random.RandomState(N + share)
    index = torch.from_numpy(np.stack([np.sort(rs.choice(N, M, replace=False)) for _ in range(B)]).astype(np.int32)).cuda()
    at = index.long()[:, None, :].expand(-1, 33, -1)
    tag = f"{density:8s} B={B:2d} N={N:6d} inside={inside:3d} M={M:6d}:"
    x4 = native.to_rows4(xyz)
    q = support.gather_positions(xyz, index)
    c4 = native.to_rows4(q)
    s_csr = radius.search_radius(xyz, r)
    q_csr = radius.search_radius(xyz, r, queries=q)
    cap_s, cap_q = s_csr[0].shape[1], q_csr[0].shape[1]
    nrm = rows.normals(x4, *s_csr, want_curvature=False)[0]
    need = support.needed(x4, c4, *q_csr, self_index=index)
    n_csr = radius.search_radius(xyz, r, queries=need["points"])
    cap_n = n_csr[0].shape[1]
    coverage = need["count"].float().mean().item() / N
    est = cap_q // M
    names = {1: "lane", 2: "wave"}
    say(f"{tag} radius {r:.5f}; rows a centre {cap_q / M:.1f} (est {est}), coverage {coverage:.3f} "
        f"(the host's bound {min(N, est * M) / N:.3f}); support.plan -> {support.plan(N, M, capacity=cap_q)}, support.form -> "
        f"{names[support.form(B, N, M, cap_q)]}")
    res = {}
    if inside != 20:
        feat = dict(search="radius", radius=r)
        con = [("parent: whole cloud + gather", lambda: res.__setitem__("p", torch.gather(fpfh.compute_fpfh_feature(xyz, nrm, capacity=cap_s, **feat), 2, at))),
               ('support="all"', lambda: res.__setitem__("a", fpfh.compute_fpfh_feature(xyz, nrm, capacity=(cap_q, cap_s), query_index=index, support="all", **feat))),
               ('support="needed"', lambda: res.__setitem__("n", fpfh.compute_fpfh_feature(xyz, nrm, capacity=(cap_q, cap_n), query_index=index, support="needed", **feat)))]
        if share == 10:
            con += [("parent, normals=None", lambda: res.__setitem__("p0", torch.gather(fpfh.compute_fpfh_feature(xyz, capacity=cap_s, **feat), 2, at))),
                    ('"all", normals=None', lambda: res.__setitem__("a0", fpfh.compute_fpfh_feature(xyz, capacity=(cap_q, cap_s), query_index=index, **feat)))]
        t = bg.race(tag, con, blocks)
        assert eq(res["p"], res["a"]) and eq(res["p"], res["n"]) and ("p0" not in res or eq(res["p0"], res["a0"]))
        p, a, n = t["parent: whole cloud + gather"], t['support="all"'], t['support="needed"']
        say(f'{tag} parent / "all" = x{np.median(p) / np.median(a):.2f}, parent / "needed" = x{np.median(p) / np.median(n):.2f}, '
            f'"all" / "needed" = x{np.median(a) / np.median(n):.2f}: {verdict(n, a, "needed", "all")}'
            + (f'; normals=None: parent / "all" = x{np.median(t["parent, normals=None"]) / np.median(t[chr(34) + "all" + chr(34) + ", normals=None"]):.2f}'
               if share == 10 else ""))
        plans.append((density, B, N, inside, M, round(coverage, 3), round(min(N, est * M) / N, 3), round(float(np.median(a) / np.median(n)), 2),
                      bg.beats(n, a), bg.beats(a, n), round(float(np.median(p) / np.median(min((a, n), key=np.median))), 2)))
    mine = support.spfh(x4, nrm, c4, support.gather_positions(nrm, index), *q_csr, self_index=index)
    qn = support.gather_positions(nrm, index)
    sup = rows.spfh(x4, nrm, *s_csr)
    parts = [("spfh centres, a lane", lambda: res.__setitem__("sl", support.spfh(x4, nrm, c4, qn, *q_csr, self_index=index, variant="lane"))),
             ("spfh centres, a wave", lambda: res.__setitem__("sw", support.spfh(x4, nrm, c4, qn, *q_csr, self_index=index, variant="wave")))]
    if inside != 20:
        parts = [("self search", lambda: radius.search_radius(xyz, r, capacity=cap_s)),
                 ("query search", lambda: radius.search_radius(xyz, r, capacity=cap_q, queries=q)),
                 ("needed", lambda: support.needed(x4, c4, *q_csr, self_index=index)),
                 ("search from the needed", lambda: radius.search_radius(xyz, r, capacity=cap_n, queries=need["points"])),
                 ("rows.spfh, whole support", lambda: rows.spfh(x4, nrm, *s_csr)),
                 ("normals at the centres", lambda: support.normals(x4, c4, *q_csr, want_curvature=False))] + parts + [
                 ("fpfh centres", lambda: support.fpfh(x4, c4, *q_csr, sup, mine, self_index=index))]
    t = bg.race(tag + " parts", parts, blocks)
    assert torch.equal(res["sl"], res["sw"]) and torch.equal(res["sl"], mine)
    lane, wave = t["spfh centres, a lane"], t["spfh centres, a wave"]
    say(f"{tag} first pass: lane / wave = x{np.median(lane) / np.median(wave):.2f}: {verdict(wave, lane, 'wave', 'lane')}")
    forms.append((density, B, N, inside, M, est, round(float(np.median(lane) / np.median(wave)), 2), bg.beats(wave, lane), bg.beats(lane, wave)))
    say()


def bench_register(B, N, blocks):
    xyz = bg.cloud("surface", B, N, 7 + N)
    ang = 0.4
    R = torch.tensor([[np.cos(ang), -np.sin(ang), 0], [np.sin(ang), np.cos(ang), 0], [0, 0, 1]], dtype=torch.float32, device="cuda")
    tgt = (R @ xyz + 0.1).flip(2).contiguous()
    res0 = float(iss.model_resolution(xyz)[0])
    opts = dict(salient_radius=6 * res0, non_max_radius=4 * res0)
    r = radius_for("surface", N, 30)
    kw = dict(search="radius", radius=r, keypoints="iss", iss=opts, mutual=False, trials=20000, nn_search="grid")
    tag = f"register_features surface  B={B:2d} N={N:6d}:"
    count = iss.compute_iss_keypoints(xyz, **opts)[1]
    out = {}
    t = bg.race(tag, [('describe="all"', lambda: out.__setitem__("a", match.register_features(xyz, tgt, 4 * res0, describe="all", **kw))),
                      ('describe="keypoints"', lambda: out.__setitem__("k", match.register_features(xyz, tgt, 4 * res0, describe="keypoints", **kw)))],
                blocks)
    assert all(eq(out["a"][k], out["k"][k]) for k in out["a"])
    a, k = t['describe="all"'], t['describe="keypoints"']
    say(f'{tag} keypoints a cloud {count.float().mean().item():.0f} of {N}; "all" / "keypoints" = x{np.median(a) / np.median(k):.2f}: '
        f"{verdict(k, a, 'keypoints', 'all')}; every key equal bit for bit")
    say()


def dump(path):
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    with open(path, "w") as fh:
        fh.write("\n".join(bg.LINES) + "\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--blocks", type=int, default=3)
    ap.add_argument("--quick", action="store_true", help="the smallest shape only")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "support_bench.txt"))
    a = ap.parse_args()
    say(f"# kernel_sources_sha16={build.sources_sha16()}")
    say(f"# profiles/bench_support.py --blocks {a.blocks}: device {torch.cuda.get_device_name(0)}, "
        f"{torch.cuda.get_device_properties(0).multi_processor_count} CUs; ms per call = median of the blocks; thresholds in this "
        f"build: wave form from est {support.WAVE_SPFH}, \"needed\" up to {support.COVERAGE_PCT} % coverage")
    say()
    plans, forms = [], []
    for B, N in CASES[:1] if a.quick else CASES:
        for density in DENSITIES:
            for inside in INSIDE:
                for share in SHARES:
                    bench_case(density, B, N, inside, share, a.blocks, plans, forms)
                    torch.cuda.empty_cache()
                    dump(a.out)                              # (kept case by case: a run cut short leaves what it measured)
    for B, N in ((16, 1024),) if a.quick else ((16, 16384), (1, 131072)):
        bench_register(B, N, a.blocks)
    say('# plans: (density, B, N, inside, M, coverage, the host\'s bound, "all" / "needed", needed beats all, all beats needed, parent / the better plan)')
    for p in sorted(plans, key=lambda p: p[5]):
        say("#   " + str(p))
    say("# forms: (density, B, N, inside, M, est, lane / wave, wave beats lane, lane beats wave)")
    for f in sorted(forms, key=lambda f: f[5]):
        say("#   " + str(f))
    dump(a.out)


if __name__ == "__main__":
    main()
