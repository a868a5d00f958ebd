#!/usr/bin/env python
"""ISS keypoints over ragged radius rows (vcr_rows_iss_saliency_f32, vcr_rows_iss_nms_f32, ``compute_iss_keypoints``, DESIGN.md
section 4.27), on one GPU, in one process:

  the launches    the saliency pass (a wave a row, its only form) and the suppression in both forms (a lane a row, a wave a row;
                  bit-identical, asserted while timing) on the rows ``search_radius`` returns at the salient radius, the
                  suppression on their d2 prefix
  the whole call  compute_iss_keypoints(xyz, salient_radius, non_max_radius, capacity=...) against search_radius alone on the
                  same cloud: the search's share of the call; and one search (non_max_radius <= salient_radius: the prefix)
                  against the two searches the call would run otherwise
  torch           the same keypoints from torch device ops on the same rows -- a padded gather, batched fp64 covariances,
                  torch.linalg.eigvalsh, the suppression as a gathered maximum -- compared with the kernels' flags (the share of
                  points that agree: another arithmetic, not the same bits) and timed apart; skipped with a line where its
                  projected time is above `--torch-limit` seconds
  matching        the one-way share of right matches (match_features' partner is the true one) on the test suite's surface
                  fixture over all source points and over the ISS keypoints alone

Shapes (B, N): (16, 1024), (16, 16 384), (1, 131 072); two clouds: a uniform cube and a sphere's surface (profiles/bench_grid.py's);
the radii are Open3D's defaults, 6 and 4 times the batch's mean ``model_resolution``.  Per case: ms per call from device events
around `--blocks` repeated blocks of calls after a warm-up, contenders alternated block by block (section 4.8's protocol); the
median block, the fastest and the slowest.  A contender "beats" another when its SLOWEST block is below the other's FASTEST.  The
closing lines collect where either form of the suppression beats the other: vcr_rows_iss_form's threshold is read off them.

  python profiles/bench_iss.py [--blocks 5] [--quick] [--out profiles/iss_bench.txt]
"""
import argparse
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import vcrnet_amd  # noqa: E402,F401
from vcrnet_amd import build, iss, native, radius  # noqa: E402
import bench_grid as bg  # noqa: E402  (the clouds, the race and the spread rule)

CASES = ((16, 1024), (16, 16384), (1, 131072))
DENSITIES = ("uniform", "surface")
GAMMA, MIN_NEIGHBORS = 0.975, 5
say = bg.say


def torch_iss(xyz, csr, d2, r2_nm):
    """The contender: flags bool [B,N] from the same rows by torch device ops (Open3D's arithmetic on differences)."""
    idx, row_start, total = csr
    B, _, N = xyz.shape
    dev = xyz.device
    n = row_start[:, 1:] - row_start[:, :-1]
    W = int(n.max())
    slot = torch.arange(W, device=dev)[None, None, :]
    used = slot < n[:, :, None]
    at = (row_start[:, :N, None] + slot).clamp(max=idx.shape[1] - 1)
    j = torch.where(used, torch.gather(idx, 1, at.view(B, -1)).view(B, N, W).long(), torch.arange(N, device=dev)[None, :, None])
    p = xyz.transpose(1, 2)                                 # [B,N,3]
    d = (torch.gather(p, 1, j.view(B, -1, 1).expand(-1, -1, 3)).view(B, N, W, 3) - p[:, :, None, :]).double()
    d = d * used[..., None]
    m = (n + 1).double()[:, :, None]
    mean = d.sum(2) / m
    C = torch.einsum("bnwi,bnwj->bnij", d, d) / m[..., None] - mean[..., :, None] * mean[..., None, :]
    lam = torch.linalg.eigvalsh(C)
    sal = torch.where((n + 1 >= MIN_NEIGHBORS) & (lam[..., 1] / lam[..., 2] < GAMMA) & (lam[..., 0] / lam[..., 1] < GAMMA),
                      lam[..., 0], torch.zeros((), dtype=torch.float64, device=dev))
    near = used & (torch.gather(d2, 1, at.view(B, -1)).view(B, N, W) <= r2_nm)
    best = torch.where(near, torch.gather(sal, 1, j.view(B, -1)).view(B, N, W), torch.full((), -1.0, dtype=torch.float64, device=dev)).amax(2) \
        if W else torch.full_like(sal, -1.0)
    return (sal > 0) & (near.sum(2) + 1 >= MIN_NEIGHBORS) & ~(sal < best)


def bench_case(tag, xyz, blocks, wins, key, torch_limit, per_matrix):
    B, _, N = xyz.shape
    res = float(iss.model_resolution(xyz).mean())
    sr, nr = float(np.float32(6.0 * res)), float(np.float32(4.0 * res))
    r2 = radius._radius("bench", nr)[1]
    idx, row_start, total, d2 = radius.search_radius(xyz, sr, want_d2=True)
    csr = (idx, row_start, total)
    n_i = row_start[:, 1:] - row_start[:, :-1]
    cap, mean_row, longest = idx.shape[1], n_i.float().mean().item(), int(n_i.max())
    small = radius.search_radius(xyz, nr)
    cap2 = small[0].shape[1]
    xyz4 = native.to_rows4(xyz)
    out = {}
    sal_call = lambda: out.__setitem__("sal", iss.saliency_rows(xyz4, *csr, GAMMA, GAMMA, MIN_NEIGHBORS)["saliency"])  # noqa: E731
    sal_call()
    nms_call = lambda v: out.__setitem__(v, iss.nms_rows(*csr, out["sal"], MIN_NEIGHBORS, d2=d2, r2_nm=r2, variant=v)["keypoint"])  # noqa: E731
    names = {1: "lane", 2: "wave"}
    say(f"{tag} model resolution {res:.5f}, radii {sr:.5f} / {nr:.5f}, capacity {cap} a cloud (est {cap // N}), mean row {mean_row:.1f}, "
        f"longest {longest}; non-max rows: mean {small[2].sum().item() / (B * N):.1f}; the plan's form: {names[iss.form(B, N, cap)]}")
    times = bg.race(tag, [("saliency (a wave a row)", sal_call), ("nms, a lane a row", lambda: nms_call("lane")),
                          ("nms, a wave a row", lambda: nms_call("wave"))], blocks)
    assert torch.equal(out["lane"], out["wave"])
    kp = int((out["lane"] > 0).sum())
    say(f"{tag} salient {int((out['sal'] > 0).sum())} of {B * N}, keypoints {kp}")
    l, w = times["nms, a lane a row"], times["nms, a wave a row"]
    wins.append(key + (round(mean_row, 1), cap // N, round(float(np.median(l) / np.median(w)), 2), bg.beats(w, l), bg.beats(l, w)))

    def two_searches():
        a = radius.search_radius(xyz, sr, capacity=cap)
        b = radius.search_radius(xyz, nr, capacity=cap2)
        s = iss.saliency_rows(xyz4, *a, GAMMA, GAMMA, MIN_NEIGHBORS)["saliency"]
        return iss.select(xyz, iss.nms_rows(*b, s, MIN_NEIGHBORS)["keypoint"])
    whole = lambda: out.__setitem__("whole", iss.compute_iss_keypoints(xyz, sr, nr, GAMMA, GAMMA, MIN_NEIGHBORS, capacity=cap, want_flag=True))  # noqa: E731
    t = bg.race(tag, [("compute_iss_keypoints", whole), ("search_radius(want_d2)", lambda: radius.search_radius(xyz, sr, want_d2=True, capacity=cap)),
                      ("two searches, no prefix", lambda: out.__setitem__("two", two_searches()))], blocks)
    assert torch.equal(out["whole"][3], out["lane"]) and torch.equal(out["two"]["count"], out["whole"][1])
    tw, ts, t2 = (float(np.median(t[k])) for k in t)
    say(f"{tag} the search is {100 * ts / tw:.1f} % of compute_iss_keypoints; two searches / one = x{t2 / tw:.2f}")
    mine = float(np.median(times["saliency (a wave a row)"])) + min(float(np.median(l)), float(np.median(w)))
    if per_matrix[0] is not None and per_matrix[0] * B * N > torch_limit:
        say(f"{tag} torch device ops: skipped, projected {per_matrix[0] * B * N:.0f} s from the smaller shape")
    else:
        theirs = torch_iss(xyz, csr, d2, r2)
        torch.cuda.synchronize()
        tt = bg.timed(lambda: torch_iss(xyz, csr, d2, r2), 1)
        per_matrix[0] = tt / 1e3 / (B * N)
        agree = (theirs == (out["lane"] > 0)).float().mean().item()
        say(f"{tag} torch device ops on the same rows {tt:.3f} ms/call, the two launches {mine:.4f} ms (timed apart): x{tt / mine:.1f}; "
            f"flags that agree {100 * agree:.3f} %, torch keypoints {int(theirs.sum())}")
    say()


def bench_matching():
    """The surface fixture: one-way matches over all source points and over the ISS keypoints."""
    import match_restated as mr
    for N, k in ((600, 20), (1500, 30)):
        c = mr.surface(N)
        src, tgt = (torch.from_numpy(np.ascontiguousarray(c[s][None])).cuda() for s in ("src", "tgt"))
        twin = torch.from_numpy(c["twin"]).cuda()
        flag = vcrnet_amd.compute_iss_keypoints(src, want_flag=True)[3][0] > 0
        for what, normals in (("estimated normals", lambda x: None),
                              ("tangent-oriented normals", lambda x: vcrnet_amd.orient_normals_consistent_tangent_plane(x, vcrnet_amd.estimate_normals(x, k)))):
            corr = vcrnet_amd.match_features(vcrnet_amd.compute_fpfh_feature(src, normals(src), k=k),
                                             vcrnet_amd.compute_fpfh_feature(tgt, normals(tgt), k=k), mutual=False)[0]
            right = corr == twin
            say(f"matching surface N={N} k={k} {what}: right matches {100 * right.float().mean().item():.1f} % of all {N} source points, "
                f"{100 * right[flag].float().mean().item():.1f} % of the {int(flag.sum())} ISS keypoints")
    say()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--blocks", type=int, default=5)
    ap.add_argument("--quick", action="store_true", help="the smallest shape only")
    ap.add_argument("--torch-limit", type=float, default=20.0, help="seconds a call of the torch contender may be projected to take")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "iss_bench.txt"))
    a = ap.parse_args()
    say(f"# kernel_sources_sha16={build.sources_sha16()}")
    say(f"# profiles/bench_iss.py --blocks {a.blocks}: device {torch.cuda.get_device_name(0)}, "
        f"{torch.cuda.get_device_properties(0).multi_processor_count} CUs; ms per call = median of the blocks; threshold in this "
        f"build: nms wave from est {iss.WAVE_NMS}")
    say()
    wins = []
    for density in DENSITIES:
        per_matrix = [None]
        for B, N in CASES[:1] if a.quick else CASES:
            xyz = bg.cloud(density, B, N, B + N)
            bench_case(f"{density:8s} B={B:2d} N={N:6d}:", xyz, a.blocks, wins, (density, B, N), a.torch_limit, per_matrix)
            del xyz
            torch.cuda.empty_cache()
    bench_matching()
    say("# nms: lane / wave at (cloud, B, N, mean row, capacity / N, ratio): " + ", ".join(str(k[:6]) for k in wins))
    say("# nms: the wave form beats the lane form beyond the spread at: " + (", ".join(str(k[:6]) for k in wins if k[6]) or "nowhere"))
    say("# nms: the lane form beats the wave form beyond the spread at: " + (", ".join(str(k[:6]) for k in wins if k[7]) or "nowhere"))
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        fh.write("\n".join(bg.LINES) + "\n")


if __name__ == "__main__":
    main()
