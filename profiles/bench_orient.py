#!/usr/bin/env python
"""Consistent normal orientation (vcr_orient_tangent_f32, ``orient_normals_consistent_tangent_plane``),
on one GPU, in one process:

  the raw call    vcr_orient_tangent_f32 on estimated normals and ``search_knn``'s rows: ms per call, the trees it found, and its
                  split by launch from the profiler's device records (init, the rounds' pick / hook / flatten summed over all
                  enqueued rounds -- those behind the last hooking round return at once --, top, out)
  the whole call  orient_normals_consistent_tangent_plane(xyz, normals, k) against search_knn alone: the search's share
  torch           the same rounds from torch device ops on the same rows -- scatter_reduce(amin) of the packed keys into both
                  trees' roots, the mutual-pair rule, pointer doubling by gathers -- with a host test per round and per doubling
                  step (which the kernels do not have); its flips are compared with the kernels' (its d is not an exact fmaf, so
                  a tie may break differently: the share of equal flips is printed, not asserted), timed apart
  registration    register_features(orient="tangent") against orient=None on a surface and its moved copy: the price of the
                  orientation and of the second run of the chain

Shapes (B, N): (16, 1024), (16, 16 384), (1, 131 072) at k = 12 and 30; clouds: a uniform cube, a sphere's surface
(profiles/bench_grid.py's clouds) and the in-order path with all normals equal -- every vertex hooks under its predecessor in
round one, the flatten's worst case (its rows have two entries, whatever k).  Per case: ms per call from device events around
`--blocks` repeated blocks of calls after a warm-up (section 4.8's protocol); the median block, the fastest and the slowest.

  python profiles/bench_orient.py [--blocks 5] [--quick] [--out profiles/orient_bench.txt]
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
from vcrnet_amd import build, grid, match, orient, plane  # noqa: E402
import bench_grid as bg  # noqa: E402  (the clouds, the race and the spread rule)

CASES = ((16, 1024), (16, 16384), (1, 131072))
KS = (12, 30)
say = bg.say
BIG = torch.iinfo(torch.int64).max


def path_case(B, N):
    """The in-order path: xyz, normals (all equal), idx int32 [B,N,2]."""
    i = torch.arange(N, dtype=torch.int32)
    idx = torch.stack([i - 1, torch.where(i + 1 < N, i + 1, torch.full_like(i, -1))], 1)
    pos = torch.arange(N, dtype=torch.float32)
    xyz = torch.stack([pos, torch.zeros(N), pos])
    nrm = torch.tensor([0.6, 0.0, -0.8])[:, None].expand(3, N)
    return tuple(t[None].expand((B,) + tuple(t.shape)).contiguous().cuda() for t in (xyz, nrm, idx))


def torch_orient(xyz, nrm, idx):
    """The contender: flip int32 [B,N] by the same rounds in torch device ops."""
    B, _, N = xyz.shape
    k = idx.shape[2]
    dev = xyz.device
    me = torch.arange(B * N, device=dev)
    off = (me // N) * N
    src = me.repeat_interleave(k)
    j = idx.reshape(-1).long()
    ok = (j >= 0) & (j < N) & (j != src % N)
    a, b = src[ok], j[ok] + off[src[ok]]
    n = nrm.permute(0, 2, 1).reshape(B * N, 3)
    n64 = n.double()

    def dot(p, q):                                          # fp32 roundings of exact products, one after another
        d = (n64[p, 0] * n64[q, 0]).float().double()
        d = (n64[p, 1] * n64[q, 1] + d).float().double()
        return (n64[p, 2] * n64[q, 2] + d).float()
    d = dot(a, b)
    fin = torch.isfinite(d)
    x = 1.0 - d.abs()
    w = torch.where(fin, torch.where(x > 0, x, torch.zeros_like(x)), torch.ones_like(x))
    lo, hi = torch.minimum(a, b) - off[a], torch.maximum(a, b) - off[a]
    key = ((w.view(torch.int32).long() - (1 << 29)) << 34) | (lo << 17) | hi       # (signed: the order is the unsigned key's)
    root, par = me.clone(), torch.zeros_like(me)
    while True:
        ra, rb = root[a], root[b]
        out = ra != rb
        if not bool(out.any()):
            break
        ko = key[out]
        best = torch.full_like(me, BIG).scatter_reduce(0, ra[out], ko, "amin").scatter_reduce(0, rb[out], ko, "amin")
        R = torch.nonzero(best != BIG).reshape(-1)
        kR = best[R]
        p, q = ((kR >> 17) & 0x1FFFF) + off[R], (kR & 0x1FFFF) + off[R]
        other = torch.where(root[p] == R, root[q], root[p])
        hook = ~((best[other] == kR) & (R < other))
        dd = dot(p, q)
        rev = (torch.isfinite(dd) & (dd < 0)).long()
        up, upp = me.clone(), torch.zeros_like(me)
        up[R[hook]] = other[hook]
        upp[R[hook]] = (par[p] ^ par[q] ^ rev)[hook]
        while True:
            g = up[up]
            if torch.equal(g, up):
                break
            up, upp = g, upp ^ upp[up]
        root, par = up[root], par ^ upp[root]
    z = xyz[:, 2].reshape(-1)
    zr = torch.where(torch.isfinite(z), z + 0.0, torch.full_like(z, -float("inf")))
    top = torch.full_like(zr, -float("inf")).scatter_reduce(0, root, zr, "amax")
    ref = torch.full_like(me, BIG).scatter_reduce(0, root, torch.where(zr == top[root], me, torch.full_like(me, BIG)), "amin")[root]
    return (par ^ par[ref] ^ (n[ref, 2] < 0).long()).view(B, N).int()


def kernel_split(fn, calls=5):
    from torch.profiler import ProfilerActivity, profile
    with profile(activities=[ProfilerActivity.CUDA]) as prof:
        for _ in range(calls):
            fn()
        torch.cuda.synchronize()
    split = {}
    for e in prof.key_averages():
        m = re.search(r"orient_([a-z]+)_kernel", e.key)
        if m:
            t = getattr(e, "device_time_total", getattr(e, "cuda_time_total", 0.0)) / 1e3 / calls
            split[m.group(1)] = split.get(m.group(1), 0.0) + t
    return split


def bench_raw(tag, xyz, nrm, idx, blocks, with_search_k=None):
    res = {}
    call = lambda: res.__setitem__("o", orient.orient_tangent(xyz, nrm, idx, want_flip=True, want_trees=True))   # noqa: E731
    contenders = [("vcr_orient_tangent_f32", call)]
    if with_search_k:
        contenders += [("orient_normals_consistent_tangent_plane", lambda: orient.orient_normals_consistent_tangent_plane(xyz, nrm, k=with_search_k)),
                       ("search_knn alone", lambda: grid.search_knn(xyz, with_search_k))]
    times = bg.race(tag, contenders, blocks)
    trees = res["o"]["n_trees"]
    split = kernel_split(call)
    say(f"{tag} trees a cloud {trees.float().mean().item():.1f} (most {int(trees.max())}), flipped {100 * res['o']['flip'].float().mean().item():.1f} %; "
        "launches: " + ", ".join(f"{k} {split.get(k, 0.0):.4f}" for k in ("init", "pick", "hook", "flatten", "top", "out")) + " ms")
    if with_search_k:
        whole, search = (float(np.median(times[k])) for k in ("orient_normals_consistent_tangent_plane", "search_knn alone"))
        say(f"{tag} the search is {100 * search / whole:.1f} % of orient_normals_consistent_tangent_plane")
    t_mine = float(np.median(times["vcr_orient_tangent_f32"]))
    theirs = torch_orient(xyz, nrm, idx)
    torch.cuda.synchronize()
    same = (theirs == res["o"]["flip"]).float().mean().item()
    t = bg.timed(lambda: torch_orient(xyz, nrm, idx), 2)
    say(f"{tag} torch device ops on the same rows {t:.4f} ms/call, the kernels {t_mine:.4f} ms (timed apart): x{t / t_mine:.1f}; "
        f"equal flips {same:.6f}")
    say()


def surface_pair(B, N, seed=5):
    """A surface without symmetries over the unit square and its rotated, shifted, permuted copy: (src, tgt) [B,3,N]."""
    rs = np.random.RandomState(seed + N)
    u, v = rs.uniform(0, 1, (B, N)), rs.uniform(0, 1, (B, N))
    z = (0.15 * np.sin(7 * u) * np.cos(5 * v) + 0.25 * u * v + 0.1 * np.exp(-((u - .3) ** 2 + (v - .6) ** 2) / 0.01)
         - 0.08 * np.exp(-((u - .75) ** 2 + (v - .25) ** 2) / 0.004))
    tgt = np.stack([u, v, z], 1)
    ax = np.asarray([0.3, -0.5, 0.8]) / np.linalg.norm([0.3, -0.5, 0.8])
    K = np.asarray([[0, -ax[2], ax[1]], [ax[2], 0, -ax[0]], [-ax[1], ax[0], 0]])
    th = np.deg2rad(160.0)                                  # past a right angle: the copy's top point is another one
    A = np.eye(3) + np.sin(th) * K + (1 - np.cos(th)) * K @ K
    src = np.stack([(A @ tgt[b] + np.asarray([[0.2], [-0.1], [0.3]]))[:, rs.permutation(N)] for b in range(B)])
    return torch.from_numpy(src.astype(np.float32)).cuda(), torch.from_numpy(tgt.astype(np.float32)).cuda()


def bench_register(B, N, k, blocks):
    src, tgt = surface_pair(B, N)
    tag = f"register B={B:2d} N={N:6d} k={k}:"
    for method in ("ransac", "fgr"):
        kw = dict(k=k, mutual=False, search="grid", nn_search="grid", method=method, **(dict(trials=4096) if method == "ransac" else {}))
        res = {}
        times = bg.race(f"{tag} {method}", [("orient=None", lambda: res.__setitem__(0, match.register_features(src, tgt, 0.05, **kw))),
                                           ('orient="tangent"', lambda: res.__setitem__(1, match.register_features(src, tgt, 0.05, orient="tangent", **kw))),
                                           ("estimate + orient, both clouds", lambda: [orient.orient_normals_consistent_tangent_plane(
                                               x, plane.estimate_normals(x, k, search="grid")) for x in (src, tgt)])], blocks)
        a, b, c = (float(np.median(times[n])) for n in ("orient=None", 'orient="tangent"', "estimate + orient, both clouds"))
        say(f"{tag} {method}: tangent / None = x{b / a:.2f} (+{b - a:.3f} ms, of which estimating and orienting both clouds' normals "
            f"{c:.3f} ms); fitness None {res[0]['fitness'].mean().item():.4f} (rmse {res[0]['inlier_rmse'].mean().item():.2e}), tangent "
            f"{res[1]['fitness'].mean().item():.4f} (rmse {res[1]['inlier_rmse'].mean().item():.2e}); flipped {int(res[1]['flipped'].sum())} of {B}")
    say()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--blocks", type=int, default=5)
    ap.add_argument("--quick", action="store_true", help="the smallest shape only")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "orient_bench.txt"))
    a = ap.parse_args()
    say(f"# kernel_sources_sha16={build.sources_sha16()}")
    say(f"# profiles/bench_orient.py --blocks {a.blocks}: device {torch.cuda.get_device_name(0)}, "
        f"{torch.cuda.get_device_properties(0).multi_processor_count} CUs; ms per call = median of the blocks")
    say()
    for B, N in CASES[:1] if a.quick else CASES:
        for density in ("uniform", "surface"):
            for k in KS:
                xyz = bg.cloud(density, B, N, B + N + k)
                nrm = plane.estimate_normals(xyz, k, search="grid")
                idx = grid.search_knn(xyz, k)
                bench_raw(f"{density:8s} B={B:2d} N={N:6d} k={k:2d}:", xyz, nrm, idx, a.blocks, with_search_k=k)
                del xyz, nrm, idx
                torch.cuda.empty_cache()
        bench_raw(f"path     B={B:2d} N={N:6d} k= 2:", *path_case(B, N), a.blocks)
    for B, N, k in ((16, 1024, 20),) if a.quick else ((16, 1024, 20), (4, 16384, 30)):
        bench_register(B, N, k, a.blocks)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        fh.write("\n".join(bg.LINES) + "\n")


if __name__ == "__main__":
    main()
