#!/usr/bin/env python
"""Feature matching and the RANSAC over its correspondences on the device (vcr_feat_nn_f32, vcr_ransac_f32; DESIGN.md section
4.15), by bench_nnscore.py's protocol as bench_plane.py runs it: ms per call from device events around `--blocks` repeated
blocks of calls after a warm-up, contenders alternated block by block, each block's round starting at another contender and each
contender run once untimed before its block; the median block, the fastest and the slowest.

a. Matching, B x N = 16 x 1024, 16 x 16 384, 1 x 131 072 (Ns = Nt = N): the device's own FPFH rows (k = 30) of two samplings of
   the jittered torus.  Contenders: vcr_feat_nn_f32 one way in the plan's form and with 1, 2 and 4 rows per lane forced (the
   plan's splits for each), the mutual search, and torch -- `cdist` + `argmin` over chunks of source rows (at most 2^28 matrix
   elements a chunk).  torch's distance is the expansion form in fp32; the rows on which its neighbour differs are counted.
b. The RANSAC, 16 x 1024 and 16 x 16 384 at T = 100 000: the torus and a posed, permuted copy, 30 % of the correspondences the
   true partner, the rest uniform.  Contenders: vcr_ransac_f32 alone, and a batched torch RANSAC from THE SAME picks (the
   device's trial_picks): the edge-length test on all trials, then -- on the trials that pass, compacted -- the centred
   covariance, `torch.linalg.svd` in fp64, the distance check and the count by a [V,3,M] product, cloud by cloud.

  python profiles/bench_match.py [--blocks 5] [--out profiles/match_bench.txt]
"""
import argparse
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import vcrnet_amd  # noqa: E402,F401
from vcrnet_amd import build, fpfh, match  # noqa: E402
from bench_plane import LINES, NORMALS_SHAPES as SHAPES, run_blocks, say, torus  # noqa: E402

K = 30
T = 100000
MAX_DIST, SIMILARITY, SEED, SHARE = 0.05, 0.9, 7, 0.3


def torch_nn(a, b):
    """[B,33,Ns], [B,33,Nt] -> int64 [B,Ns] by cdist + argmin over chunks of source rows."""
    B, _, Ns = a.shape
    Nt = b.shape[2]
    at, bt = a.transpose(1, 2).contiguous(), b.transpose(1, 2).contiguous()
    step = max(1, min(Ns, (1 << 28) // (B * Nt)))
    return torch.cat([torch.cdist(at[:, i:i + step], bt).argmin(2) for i in range(0, Ns, step)], 1)


def torch_ransac(src, tgt, corr, picks):
    """The contender: per cloud (best count, best trial) from the device's picks [B,T,3] (source indices)."""
    B = src.shape[0]
    s2, lim = SIMILARITY * SIMILARITY, MAX_DIST * MAX_DIST
    out = []
    for b in range(B):
        P, Q = src[b].t(), tgt[b].t()[corr[b].long().clamp(0, tgt.shape[2] - 1)]              # [Ns,3]: every source point is paired here
        pk = picks[b].long()
        p, q = P[pk], Q[pk]                                                                   # [T,3,3]
        ok = (pk[:, 0] != pk[:, 1]) & (pk[:, 0] != pk[:, 2]) & (pk[:, 1] != pk[:, 2])
        for u, v in ((0, 1), (0, 2), (1, 2)):
            ds2, dt2 = ((p[:, u] - p[:, v]) ** 2).sum(1), ((q[:, u] - q[:, v]) ** 2).sum(1)
            ok &= (ds2 >= s2 * dt2) & (dt2 >= s2 * ds2)
        keep = ok.nonzero()[:, 0]
        p, q = p[keep].double(), q[keep].double()
        pm, qm = p.mean(1, keepdim=True), q.mean(1, keepdim=True)
        H = (p - pm).transpose(1, 2) @ (q - qm)
        U, _, Vh = torch.linalg.svd(H)
        V = Vh.transpose(1, 2)
        d = torch.det(V @ U.transpose(1, 2))
        V = torch.cat([V[:, :, :2], V[:, :, 2:] * torch.where(d < 0, -1.0, 1.0)[:, None, None]], 2)
        R = (V @ U.transpose(1, 2)).float()
        t = (qm.transpose(1, 2) - R.double() @ pm.transpose(1, 2)).float()                    # [V,3,1]
        near = (((R @ p.float().transpose(1, 2) + t - q.float().transpose(1, 2)) ** 2).sum(1) <= lim).all(1)
        keep, R, t = keep[near], R[near], t[near]
        best_c, best_t = 0, -1
        for i in range(0, len(keep), 2048):
            c = (((R[i:i + 2048] @ P.t()[None] + t[i:i + 2048] - Q.t()[None]) ** 2).sum(1) <= lim).sum(1)
            j = int(c.argmax()) if len(c) else -1
            if j >= 0 and int(c[j]) > best_c:
                best_c, best_t = int(c[j]), int(keep[i + j])
        out.append((best_c, best_t))
    return out


def clouds(B, N, seed):
    rs = np.random.RandomState(seed)
    return torch.from_numpy(np.stack([torus(rs, N, 0.002) for _ in range(B)]).astype(np.float32)).cuda()


def part_a(blocks):
    say("## a. matching in the 33-d feature space, Ns = Nt = N")
    for B, N in SHAPES:
        a, b = (fpfh.compute_fpfh_feature(clouds(B, N, s + B + N), k=K) for s in (0, 1))
        res = {}
        forms = {q: match.feat_nn_form(B, N, N, 0, match.variant(q, 0))[:2] for q in match.QUERIES_PER_LANE}
        plan = match.feat_nn_form(B, N, N, 0)[:2]
        contenders = [("vcr_feat_nn_f32 (plan)", lambda: res.__setitem__("hip", match.feat_nn(a, b)))]
        contenders += [(f"  forced Q={q} S={forms[q][1]}", lambda q=q: match.feat_nn(a, b, variant=match.variant(q, 0)))
                       for q in match.QUERIES_PER_LANE]
        contenders += [("vcr_feat_nn_f32 mutual", lambda: match.feat_nn(a, b, mutual=True)),
                       ("torch cdist + argmin", lambda: res.__setitem__("torch", torch_nn(a, b)))]
        med, times, calls = run_blocks(contenders, blocks)
        for name, _ in contenders:
            v = times[name]
            say(f"B={B:2d} N={N:6d}  {name:24s} {med[name]:10.4f} ms/call  (blocks min {min(v):.4f} max {max(v):.4f}; "
                f"{blocks} x {calls[name]} calls)")
        hip = res["hip"]["nn_idx"].long()
        differ = int((hip != res["torch"]).sum())
        pairs = float(B) * N * N
        say(f"B={B:2d} N={N:6d}  plan Q={plan[0]} S={plan[1]}; {pairs * 33 / (med['vcr_feat_nn_f32 (plan)'] * 1e-3) / 1e12:.2f} T channel-steps/s; "
            f"torch / kernel x{med['torch cdist + argmin'] / med['vcr_feat_nn_f32 (plan)']:.2f}; torch's neighbour differs on "
            f"{differ} of {B * N} rows")
        say()


def part_b(blocks):
    say(f"## b. the RANSAC, T = {T}, {int(100 * SHARE)} % true partners, max_dist {MAX_DIST}, similarity {SIMILARITY}")
    for B, N in SHAPES[:2]:
        rs = np.random.RandomState(7 + N)
        tgt = clouds(B, N, 3 + N)
        th = 0.9
        A = torch.tensor([[np.cos(th), -np.sin(th), 0], [np.sin(th), np.cos(th), 0], [0, 0, 1]], dtype=torch.float32).cuda()
        perm = torch.from_numpy(np.stack([rs.permutation(N) for _ in range(B)])).cuda()
        src = torch.gather(A.t() @ (tgt - 0.25), 2, perm[:, None, :].expand(B, 3, N)).contiguous()     # tgt = A src + 0.25
        true = torch.from_numpy(rs.uniform(size=(B, N)) < SHARE).cuda()
        corr = torch.where(true, perm, torch.from_numpy(rs.randint(0, N, (B, N))).cuda()).int()
        full = match.ransac(src, tgt, corr, MAX_DIST, T, SIMILARITY, SEED, want_trials=True)
        picks = full["trial_picks"]
        res = {}
        contenders = [("vcr_ransac_f32", lambda: res.__setitem__("hip", match.ransac(src, tgt, corr, MAX_DIST, T, SIMILARITY, SEED))),
                      ("torch, same picks", lambda: res.__setitem__("torch", torch_ransac(src, tgt, corr, picks)))]
        med, times, calls = run_blocks(contenders, blocks)
        for name, _ in contenders:
            v = times[name]
            say(f"B={B:2d} N={N:6d}  {name:24s} {med[name]:10.4f} ms/call  (blocks min {min(v):.4f} max {max(v):.4f}; "
                f"{blocks} x {calls[name]} calls)")
        st = full["trial_status"]
        inl = res["hip"]["inliers"].tolist()
        say(f"B={B:2d} N={N:6d}  torch / kernel x{med['torch, same picks'] / med['vcr_ransac_f32']:.1f}; trials by status 0..4: "
            f"{[int((st == s).sum()) for s in range(5)]} of {B * T}; inliers {min(inl)} ... {max(inl)} of {int(true.sum(1).min())} ... "
            f"{int(true.sum(1).max())} true pairs; torch's best count equals the kernel's in "
            f"{sum(int(c == i) for (c, _), i in zip(res['torch'], inl))} of {B} clouds, its trial in "
            f"{sum(int(t == i) for (_, t), i in zip(res['torch'], res['hip']['best_trial'].tolist()))}")
        say()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--blocks", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "match_bench.txt"))
    a = ap.parse_args()
    say(f"# kernel_sources_sha16={build.sources_sha16()}")
    say(f"# profiles/bench_match.py --blocks {a.blocks}: device {torch.cuda.get_device_name(0)}, "
        f"{torch.cuda.get_device_properties(0).multi_processor_count} CUs; ms per call = median of the blocks")
    say()
    part_a(a.blocks)
    part_b(a.blocks)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        fh.write("\n".join(LINES) + "\n")


if __name__ == "__main__":
    main()
