#!/usr/bin/env python
"""Normals on the device and the point-to-plane refinement (vcr_normals_f32, vcr_refine_plane_f32),
by bench_nnscore.py's protocol: ms per call from device events around `--blocks` repeated blocks of calls after a warm-up,
contenders alternated block by block, each block's round starting at another contender and each contender run once untimed
before its block; the median block, the fastest and the slowest.  Three parts, each of which can run alone (--part):

  a  normals at B x N = 16 x 1024, 16 x 16 384, 1 x 131 072, k = 20, on a jittered torus.  Contenders: vcr_normals_f32 alone
     (rows and neighbours given); the search alone (vcr_rows4_f32 + vcr_knn_f32); estimate_normals whole; and the kernel's
     computation in torch device ops from the same neighbours -- gather, batched fp64 covariance, torch.linalg.eigh, the sign.
  b  a point-to-plane round against a point-to-point round at bench_refine.py's four shapes and inputs (K rounds, thresholds 0:
     no cloud converges), the normals random unit vectors -- a uniform cube has no surface, and the round's cost does not
     depend on their values.
  c  convergence on the torus with source and target drawn INDEPENDENTLY (no point has a twin), a planted 40-degree pose, a
     start 6 degrees and 0.04 off, the default thresholds: rounds and final rotation / translation error of both methods from
     the same start, the normals estimate_normals(tgt, 20).

  python profiles/bench_plane.py [--part abc] [--blocks 5] [--out profiles/plane_bench.txt] [--append]
"""
import argparse
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import vcrnet_amd  # noqa: E402,F401
from vcrnet_amd import build, native, plane, refine  # noqa: E402
from bench_refine import SHAPES as REFINE_SHAPES, MAX_DIST, ROUNDS, rotation, timed  # noqa: E402

NORMALS_SHAPES = ((16, 1024), (16, 16384), (1, 131072))
K = 20
SLOW_MS = 2000.0                                               # a contender slower than this per call is timed once per block
LINES = []


def say(line=""):
    print(line, flush=True)
    LINES.append(line)


def torus(rs, n, jitter=0.0):
    """tests/refine_restated.py's torus: [3, n] float64 inside the unit cube."""
    u, v = rs.uniform(0, 2 * np.pi, n), rs.uniform(0, 2 * np.pi, n)
    r = 0.12 * (1 + 0.3 * np.sin(5 * u) * np.cos(3 * v))
    ring = 0.33 + r * np.cos(v)
    x = np.stack([0.5 + ring * np.cos(u), 0.5 + ring * np.sin(u), 0.5 + r * np.sin(v) + 0.05 * np.sin(2 * u)])
    return x + rs.uniform(-jitter, jitter, (3, n)) if jitter else x


def torch_normals(xyz4, idx):
    """The contender: vcr_normals_f32's computation from the same rows and neighbours (no viewpoint)."""
    B, N, k = idx.shape
    x = xyz4[:, :, :3]
    nb = torch.gather(x, 1, idx.long().reshape(B, N * k, 1).expand(B, N * k, 3)).view(B, N, k, 3)
    d = (nb - x[:, :, None, :]).double()
    m = float(k + 1)
    mean = d.sum(2) / m
    C = torch.einsum("bnki,bnkj->bnij", d, d) / m - mean[..., :, None] * mean[..., None, :]
    lam, V = torch.linalg.eigh(C)
    n = V[..., 0].float()
    big = torch.gather(n, 2, n.abs().argmax(2, keepdim=True))
    n = torch.where(big < 0, -n, n)
    return n.transpose(1, 2).contiguous(), (lam[..., 0] / lam.sum(-1)).float()


def run_blocks(contenders, blocks):
    times, calls = {}, {}
    for name, fn in contenders:                               # warm every contender; size its block to ~30 ms, 1 ... 50 calls
        fn()
        torch.cuda.synchronize()
        one = timed(fn, 1)
        calls[name] = 1 if one > SLOW_MS else int(min(50, max(2, 30.0 / max(one, 1e-3))))
        times[name] = []
    for i in range(blocks):                                   # alternated; the round starts one contender later every block
        k = i * len(contenders) // blocks
        for name, fn in contenders[k:] + contenders[:k]:
            fn()
            times[name].append(timed(fn, calls[name]))
    return {n: float(np.median(v)) for n, v in times.items()}, times, calls


def part_a(blocks):
    say("## a. normals, k = 20")
    for B, N in NORMALS_SHAPES:
        rs = np.random.RandomState(B + N)
        x = torch.from_numpy(np.stack([torus(rs, N, 0.002) for _ in range(B)]).astype(np.float32)).cuda()
        xyz4 = native.to_rows4(x)
        idx = native.knn(xyz4, None, K)
        res = {}
        contenders = [
            ("vcr_normals_f32", lambda: res.__setitem__("hip", plane.normals(xyz4, idx))),
            ("rows4 + knn", lambda: native.knn(native.to_rows4(x), None, K)),
            ("estimate_normals", lambda: plane.estimate_normals(x, K, want_curvature=True)),
            ("torch, same idx", lambda: res.__setitem__("torch", torch_normals(xyz4, idx))),
        ]
        med, times, calls = run_blocks(contenders, blocks)
        for name, _ in contenders:
            v = times[name]
            say(f"B={B:2d} N={N:6d}  {name:18s} {med[name]:10.4f} ms/call  (blocks min {min(v):.4f} max {max(v):.4f}; {blocks} x {calls[name]} calls)")
        (hn, hc), (tn, tc) = res["hip"], res["torch"]
        cos = (hn * tn).sum(1).abs()
        say(f"B={B:2d} N={N:6d}  torch / kernel x{med['torch, same idx'] / med['vcr_normals_f32']:.1f}; the search is "
            f"{100 * med['rows4 + knn'] / med['estimate_normals']:.1f} % of estimate_normals; against torch: 1 - |cos| max "
            f"{float((1 - cos).max()):.1e}, opposite signs {int(((hn * tn).sum(1) < 0).sum())} of {B * N}, |curvature difference| max "
            f"{float((hc - tc).abs().max()):.1e}")
        say()


def part_b(blocks):
    say(f"## b. a point-to-plane round against a point-to-point round ({ROUNDS} rounds, thresholds 0, max_dist {MAX_DIST})")
    for B, Ns, Nt in REFINE_SHAPES:
        rs = np.random.RandomState(B + Ns + Nt)                # bench_refine.py's inputs
        tgt_n = rs.uniform(-1, 1, (B, 3, Nt))
        src_n = np.empty((B, 3, Ns))
        for b in range(B):
            Rd, td = rotation(rs.normal(size=3), 2.0), rs.uniform(-0.01, 0.01, 3)
            clean = tgt_n[b][:, rs.choice(Nt, Ns, replace=Ns > Nt)] + rs.uniform(-0.002, 0.002, (3, Ns))
            src_n[b] = Rd.T @ (clean - td[:, None])
        nrm_n = rs.normal(size=(B, 3, Nt))
        nrm_n /= np.linalg.norm(nrm_n, axis=1, keepdims=True)
        src, tgt, nrm = (torch.from_numpy(x.astype(np.float32)).cuda() for x in (src_n, tgt_n, nrm_n))
        R0, t0 = torch.eye(3, device="cuda").repeat(B, 1, 1), torch.zeros(B, 3, device="cuda")
        res = {}
        kw = dict(max_iterations=ROUNDS - 1, rel_fitness=0.0, rel_rmse=0.0, want_nn=False)
        contenders = [
            ("point to plane", lambda: res.__setitem__("plane", plane.refine_plane(src, tgt, nrm, R0, t0, MAX_DIST, **kw))),
            ("point to point", lambda: res.__setitem__("point", refine.refine(src, tgt, R0, t0, MAX_DIST, **kw))),
        ]
        med, times, calls = run_blocks(contenders, blocks)
        for name, _ in contenders:
            v = times[name]
            say(f"B={B:2d} Ns={Ns:6d} Nt={Nt:6d}  {name:16s} {med[name]:10.4f} ms/call  (blocks min {min(v):.4f} max {max(v):.4f}; "
                f"{blocks} x {calls[name]} calls)")
        for name in ("plane", "point"):                        # a cloud that stopped early would make its rounds cheaper: say so
            if res[name]["iterations"].tolist() != [ROUNDS - 1] * B:
                say(f"B={B:2d} Ns={Ns:6d} Nt={Nt:6d}  NOTE {name}: updates applied {res[name]['iterations'].tolist()}, not {ROUNDS - 1} each")
        say(f"B={B:2d} Ns={Ns:6d} Nt={Nt:6d}  a plane round {med['point to plane'] / ROUNDS:.4f} ms, a point round "
            f"{med['point to point'] / ROUNDS:.4f} ms: {(med['point to plane'] - med['point to point']) / ROUNDS:+.4f} ms; after "
            f"{ROUNDS - 1} updates rmse {float(res['plane']['rmse'][0]):.5f} (plane) {float(res['point']['rmse'][0]):.5f} (point)")
        say()


def angle(R, R_true):
    D = R.double() @ R_true.double().transpose(1, 2)
    sin = 0.5 * torch.stack([D[:, 2, 1] - D[:, 1, 2], D[:, 0, 2] - D[:, 2, 0], D[:, 1, 0] - D[:, 0, 1]], 1).norm(dim=1)
    return torch.atan2(sin, (D.diagonal(dim1=1, dim2=2).sum(1) - 1) / 2)


def part_c():
    say("## c. convergence on the torus, source and target drawn independently (B = 4; default thresholds, at most 50 updates)")
    for N, max_dist in ((2048, 0.1), (16384, 0.05)):
        B = 4
        rs = np.random.RandomState(N)
        src_n, tgt_n, R_n, t_n, R0_n, t0_n = [], [], [], [], [], []
        for b in range(B):
            R, t = rotation(rs.normal(size=3), 40.0), rs.uniform(-0.5, 0.5, 3)
            d = rs.normal(size=3)
            src_n.append(torus(rs, N))
            tgt_n.append(R @ torus(rs, N) + t[:, None])
            R_n.append(R); t_n.append(t)
            R0_n.append(R @ rotation(rs.normal(size=3), 6.0)); t0_n.append(t + 0.04 * d / np.linalg.norm(d))
        f = lambda v: torch.from_numpy(np.stack(v).astype(np.float32)).cuda()   # noqa: E731
        src, tgt, R, t, R0, t0 = f(src_n), f(tgt_n), f(R_n), f(t_n), f(R0_n), f(t0_n)
        say(f"N={N:6d} max_dist {max_dist}: start rotation error {np.rad2deg(angle(R0, R).cpu().numpy()).round(3).tolist()} degrees, "
            f"translation error {(t0 - t).norm(dim=1).cpu().numpy().round(4).tolist()}")
        for method in ("point_to_point", "point_to_plane"):
            o = vcrnet_amd.refine_registration(src, tgt, R0, t0, max_dist=max_dist, max_iterations=50, method=method)
            say(f"N={N:6d}  {method:15s} updates {o['iterations'].tolist()} converged {o['converged'].tolist()}  rotation error "
                f"{np.rad2deg(angle(o['R'], R).cpu().numpy()).round(4).tolist()} degrees  translation error "
                f"{(o['t'] - t).norm(dim=1).cpu().numpy().round(5).tolist()}  fitness {o['fitness'].cpu().numpy().round(4).tolist()} "
                f"rmse {o['inlier_rmse'].cpu().numpy().round(5).tolist()}")
        say()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--part", default="abc")
    ap.add_argument("--blocks", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "plane_bench.txt"))
    ap.add_argument("--append", action="store_true", help="add to --out instead of replacing it (one part per run)")
    a = ap.parse_args()
    if not a.append:
        say(f"# kernel_sources_sha16={build.sources_sha16()}")
        say(f"# profiles/bench_plane.py --blocks {a.blocks}: device {torch.cuda.get_device_name(0)}, "
            f"{torch.cuda.get_device_properties(0).multi_processor_count} CUs; ms per call = median of the blocks")
        say()
    if "a" in a.part:
        part_a(a.blocks)
    if "b" in a.part:
        part_b(a.blocks)
    if "c" in a.part:
        part_c()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "a" if a.append else "w") as fh:
        fh.write("\n".join(LINES) + "\n")


if __name__ == "__main__":
    main()
