#!/usr/bin/env python
"""FPFH features on the device (vcr_spfh_f32, vcr_fpfh_f32, compute_fpfh_feature), by bench_nnscore.py's
protocol as bench_plane.py runs it: ms per call from device events around `--blocks` repeated blocks of calls after a warm-up,
contenders alternated block by block, each block's round starting at another contender and each contender run once untimed
before its block; the median block, the fastest and the slowest.

The shapes are the normals': B x N = 16 x 1024, 16 x 16 384, 1 x 131 072 on a jittered torus, k = 30.  Contenders: each of the
two kernels alone (rows, neighbours and normals given); the search alone (vcr_rows4_f32 + vcr_knn_f32); the search and the
normals (estimate_normals with want_idx: everything in front of the two kernels); compute_fpfh_feature whole; and the two
kernels' computation in torch device ops from the same neighbours and normals -- gathers, the pair feature in fp64,
scatter_add for the histograms, a gather of the neighbours' histograms and a weighted sum.  (The torch form counts every pair:
right on these clouds, which are finite.)  Its agreement with the kernels is reported beside its time: the histogram rows that
are equal, the largest difference of a feature, and the pairs at distance 0 both skip in the second pass.

  python profiles/bench_fpfh.py [--blocks 5] [--out profiles/fpfh_bench.txt]
"""
import argparse
import math
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import vcrnet_amd  # noqa: E402,F401
from vcrnet_amd import build, fpfh, native, plane  # noqa: E402
from bench_plane import LINES, NORMALS_SHAPES as SHAPES, run_blocks, say, torus  # noqa: E402

K = 30


def torch_fpfh(xyz4, nrm, idx):
    """The contender: (fpfh float32 [B,33,N], counts [B,N,33], the number of pairs at distance 0) from the same rows, normals
    and neighbours."""
    B, N, k = idx.shape
    x, n = xyz4[:, :, :3], nrm.transpose(1, 2)
    flat = idx.long().reshape(B, N * k, 1)
    d = (torch.gather(x, 1, flat.expand(B, N * k, 3)).view(B, N, k, 3) - x[:, :, None, :]).double()
    n2 = torch.gather(n, 1, flat.expand(B, N * k, 3)).view(B, N, k, 3).double()
    n1 = n[:, :, None, :].double().expand_as(n2)
    d2 = (d * d).sum(-1)
    L = d2.sqrt()
    a1, a2 = (n1 * d).sum(-1) / L, (n2 * d).sum(-1) / L
    swap = a1.abs() < a2.abs()
    s = swap[..., None]
    n1, n2, d = torch.where(s, n2, n1), torch.where(s, n1, n2), torch.where(s, -d, d)
    f2 = torch.where(swap, -a2, a1)
    v = torch.linalg.cross(d, n1)
    vn = v.norm(dim=-1)
    zero = (L == 0) | (vn == 0)
    v = v / vn[..., None]
    w = torch.linalg.cross(n1, v)
    f1 = (v * n2).sum(-1)
    f0 = torch.atan2((w * n2).sum(-1), (n1 * n2).sum(-1))
    coord = torch.stack([11.0 * (f0 + math.pi) / (2.0 * math.pi), 11.0 * (f1 + 1.0) * 0.5, 11.0 * (f2 + 1.0) * 0.5], -1)
    coord = torch.where(zero[..., None], torch.full_like(coord, 5.5), coord)
    bins = coord.floor().nan_to_num(0.0).clamp(0, 10).long() + torch.tensor([0, 11, 22], device=idx.device)
    counts = torch.zeros(B, N, 33, dtype=torch.float64, device=idx.device)
    counts.scatter_add_(2, bins.view(B, N, k * 3), torch.ones(B, N, k * 3, dtype=torch.float64, device=idx.device))
    own = counts * (100.0 / k)
    nb = torch.gather(own, 1, flat.expand(B, N * k, 33)).view(B, N, k, 33)
    wgt = torch.where(d2 > 0, 1.0 / d2, torch.zeros_like(d2))                  # a neighbour at distance 0 is skipped
    acc = (nb * wgt[..., None]).sum(2).view(B, N, 3, 11)
    tot = acc.sum(-1, keepdim=True)
    acc = torch.where(tot != 0, acc * (100.0 / tot), acc).view(B, N, 33)
    return (acc + own).float().transpose(1, 2).contiguous(), counts, int((d2 == 0).sum())


def counts_of(sp):
    """uint8 [B,N,48] -> the 33 counts [B,N,33]."""
    B, N, _ = sp.shape
    return sp.view(B, N, 3, 16)[..., :11].reshape(B, N, 33).double()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--blocks", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "fpfh_bench.txt"))
    a = ap.parse_args()
    say(f"# kernel_sources_sha16={build.sources_sha16()}")
    say(f"# profiles/bench_fpfh.py --blocks {a.blocks}: device {torch.cuda.get_device_name(0)}, "
        f"{torch.cuda.get_device_properties(0).multi_processor_count} CUs; ms per call = median of the blocks; k = {K}")
    say()
    for B, N in SHAPES:
        rs = np.random.RandomState(B + N)
        x = torch.from_numpy(np.stack([torus(rs, N, 0.002) for _ in range(B)]).astype(np.float32)).cuda()
        xyz4 = native.to_rows4(x)
        idx = native.knn(xyz4, None, K)
        nrm, _ = plane.normals(xyz4, idx, want_curvature=False)
        sp = fpfh.spfh(xyz4, nrm, idx)
        res = {}
        contenders = [
            ("vcr_spfh_f32", lambda: fpfh.spfh(xyz4, nrm, idx)),
            ("vcr_fpfh_f32", lambda: res.__setitem__("hip", fpfh.fpfh(xyz4, idx, sp))),
            ("rows4 + knn", lambda: native.knn(native.to_rows4(x), None, K)),
            ("rows4 + knn + normals", lambda: plane.estimate_normals(x, K, want_idx=True)),
            ("compute_fpfh_feature", lambda: res.__setitem__("whole", fpfh.compute_fpfh_feature(x, k=K))),
            ("torch, same idx", lambda: res.__setitem__("torch", torch_fpfh(xyz4, nrm, idx))),
        ]
        med, times, calls = run_blocks(contenders, a.blocks)
        for name, _ in contenders:
            v = times[name]
            say(f"B={B:2d} N={N:6d}  {name:22s} {med[name]:10.4f} ms/call  (blocks min {min(v):.4f} max {max(v):.4f}; "
                f"{a.blocks} x {calls[name]} calls)")
        two = med["vcr_spfh_f32"] + med["vcr_fpfh_f32"]
        feat, counts, coincident = res["torch"]
        rows = (counts == counts_of(sp)).all(2)
        say(f"B={B:2d} N={N:6d}  torch / the two kernels x{med['torch, same idx'] / two:.1f}; the search is "
            f"{100 * med['rows4 + knn'] / med['compute_fpfh_feature']:.1f} % of compute_fpfh_feature, the two kernels "
            f"{100 * two / med['compute_fpfh_feature']:.1f} %; whole call == composition: "
            f"{bool(torch.equal(res['whole'].view(torch.int32), res['hip'].view(torch.int32)))}; against torch: "
            f"{int(rows.sum())} of {B * N} histogram rows equal, |feature difference| max "
            f"{float((feat - res['hip']).abs().max()):.1e} of 200, {coincident} of {B * N * K} pairs at distance 0 "
            f"({int((idx == torch.arange(N, device=idx.device)[None, :, None]).sum())} of them the point itself in its own idx)")
        say()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        fh.write("\n".join(LINES) + "\n")


if __name__ == "__main__":
    main()
