#!/usr/bin/env python
"""The colored refinement (vcr_color_gradient_f32, vcr_refine_colored_f32) by bench_plane.py's protocol
(section 4.8's: device events around repeated blocks after a warm-up, contenders alternated block by block, the median block
with the fastest and the slowest).  Inputs: the textured bowl of tests/colored_restated.py, source and target drawn
independently, at 16 x 1 024, 16 x 16 384 and 1 x 131 072 points.  Three parts, each of which can run alone (--part):

  a  the gradient launch (k = 20, rows given) against the same computation in torch device ops on the same rows.
  b  a colored round against a point-to-plane round, scan and grid (K rounds, thresholds 0: no cloud converges); the fit's
     seven values at the neighbour travel as strided loads (three of the normal through gather(), four by RfPoint's indices).
  c  the same round in torch device ops (the search in blocks, the sums in fp64, torch.linalg.solve), at the first two shapes.

  python profiles/bench_colored.py [--part abc] [--blocks 5] [--out profiles/colored_bench.txt] [--append]
"""
import argparse
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import vcrnet_amd  # noqa: E402,F401
from vcrnet_amd import build, colored, native, plane  # noqa: E402
from bench_refine import ROUNDS, rotation  # noqa: E402
from bench_plane import LINES, run_blocks, say  # noqa: E402

SHAPES = ((16, 1024), (16, 16384), (1, 131072))
K = 20
LAMBDA = 0.968


def patch(rs, n, lo, hi):
    """[3,n] points of the bowl over [lo,hi]^2, their unit normals and intensities (tests/colored_restated.py's)."""
    u, v = rs.uniform(lo, hi, n), rs.uniform(lo, hi, n)
    x = np.stack([u, v, 0.15 * (u - 0.5) ** 2 + 0.1 * (v - 0.5) ** 2])
    nrm = np.stack([-0.3 * (u - 0.5), -0.2 * (v - 0.5), np.ones(n)])
    inten = 0.5 + 0.25 * np.sin(9 * u + 1) * np.cos(7 * v) + 0.2 * np.sin(5 * v - 0.5 * u)
    return x, nrm / np.linalg.norm(nrm, axis=0), inten


def inputs(B, N):
    """B pairs: tgt, its normals and intensities under a planted pose; src and its intensities; the start 2 degrees about the
    patch's z axis and a slide of (0.03, -0.02, 0) off; max_dist four mean spacings."""
    rs = np.random.RandomState(B + N)
    out = {k: [] for k in ("src", "tgt", "nrm", "I_s", "I_t", "R0", "t0")}
    for _ in range(B):
        xt, nt, it = patch(rs, N, 0.0, 1.0)
        xs, _, is_ = patch(rs, N, 0.1, 0.9)
        R, t = rotation(rs.normal(size=3), 40.0), rs.uniform(-0.5, 0.5, 3)
        for k, v in (("src", xs), ("tgt", R @ xt + t[:, None]), ("nrm", R @ nt), ("I_s", is_), ("I_t", it),
                     ("R0", R @ rotation([0, 0, 1], 2.0)), ("t0", t + R @ np.asarray([0.03, -0.02, 0.0]))):
            out[k].append(v)
    c = {k: torch.from_numpy(np.stack(v).astype(np.float32)).cuda() for k, v in out.items()}
    c["max_dist"] = max(0.07, 4.0 / np.sqrt(N))
    return c


def torch_gradient(xyz4, idx, nrm, inten):
    """The contender of part a: the header's sums and system from the same rows (no radius, no skipped entries: kNN rows)."""
    B, N, k = idx.shape
    x = xyz4[:, :, :3]
    flat = idx.long().reshape(B, N * k)
    nb = torch.gather(x, 1, flat[:, :, None].expand(B, N * k, 3)).view(B, N, k, 3)
    d = (nb - x[:, :, None, :]).double()
    n = nrm.transpose(1, 2).double()                           # [B,N,3]
    a = d - (d * n[:, :, None, :]).sum(-1, keepdim=True) * n[:, :, None, :]
    di = (torch.gather(inten, 1, flat).view(B, N, k) - inten[:, :, None]).double()
    M = torch.einsum("bnki,bnkj->bnij", a, a) + float(k * k) * n[..., :, None] * n[..., None, :]
    rhs = torch.einsum("bnki,bnk->bni", a, di)
    return torch.linalg.solve(M, rhs).float().transpose(1, 2).contiguous()


def part_a(blocks):
    say(f"## a. the colour gradient, k = {K}, rows given")
    for B, N in SHAPES:
        c = inputs(B, N)
        xyz4 = native.to_rows4(c["tgt"])
        idx = native.knn(xyz4, None, K)
        res = {}
        contenders = [
            ("vcr_color_gradient_f32", lambda: res.__setitem__("hip", colored.color_gradient(xyz4, idx, c["nrm"], c["I_t"]))),
            ("vcr_normals_f32", lambda: plane.normals(xyz4, idx, want_curvature=False)),
            ("torch, same idx", lambda: res.__setitem__("torch", torch_gradient(xyz4, idx, c["nrm"], c["I_t"]))),
        ]
        med, times, calls = run_blocks(contenders, blocks)
        head = f"B={B:2d} N={N:6d}"
        for name, _ in contenders:
            v = times[name]
            say(f"{head}  {name:24s} {med[name]:10.4f} ms/call  (blocks min {min(v):.4f} max {max(v):.4f}; {blocks} x {calls[name]} calls)")
        diff = (res["hip"] - res["torch"]).abs().max().item()
        say(f"{head}  HIP against torch: max |difference| {diff:.2e} (gradients up to {res['torch'].abs().max().item():.2f}); "
            f"x{med['torch, same idx'] / med['vcr_color_gradient_f32']:.1f}")
        say()


def torch_colored_rounds(c, grad, rounds, block_elems=1 << 24):
    """The contender of part c: `rounds` searches and rounds - 1 colored updates, no stop test (no host synchronisation)."""
    src, tgt = c["src"], c["tgt"]
    B, _, Ns = src.shape
    Nt = tgt.shape[2]
    q_all = tgt.transpose(1, 2)
    rows = max(1, block_elems // (B * Nt))
    R, t = c["R0"].double(), c["t0"].double()
    wg, wi = float(np.sqrt(LAMBDA)), float(np.sqrt(1 - LAMBDA))
    for k in range(rounds):
        p = (torch.bmm(R.float(), src) + t.float()[:, :, None]).transpose(1, 2)
        d2, idx = [], []
        for i in range(0, Ns, rows):
            m = ((p[:, i:i + rows, None, :] - q_all[:, None, :, :]) ** 2).sum(-1).min(2)
            d2.append(m.values)
            idx.append(m.indices)
        d2, idx = torch.cat(d2, 1), torch.cat(idx, 1)
        if k + 1 == rounds:
            break
        w = (d2 <= c["max_dist"] ** 2).double()[:, :, None]
        at = idx[:, :, None].expand(B, Ns, 3)
        take = lambda x: torch.gather(x.transpose(1, 2), 1, at).double()   # noqa: E731
        p, q, n, d = p.double(), take(tgt), take(c["nrm"]), take(grad)
        It, Is = torch.gather(c["I_t"], 1, idx).double(), c["I_s"].double()
        s = ((p - q) * n).sum(-1, keepdim=True)
        Md = d - (d * n).sum(-1, keepdim=True) * n
        rG = wg * s[..., 0]
        rI = wi * (It + (d * ((p - s * n) - q)).sum(-1) - Is)
        JG = wg * torch.cat([torch.cross(p, n, dim=-1), n], -1) * w
        JI = wi * torch.cat([torch.cross(p, Md, dim=-1), Md], -1) * w
        A = torch.einsum("bni,bnj->bij", JG, JG) + torch.einsum("bni,bnj->bij", JI, JI)
        g = torch.einsum("bni,bn->bi", JG, rG) + torch.einsum("bni,bn->bi", JI, rI)
        x = torch.linalg.solve(A, -g)
        c0, s0, c1, s1, c2, s2 = x[:, 0].cos(), x[:, 0].sin(), x[:, 1].cos(), x[:, 1].sin(), x[:, 2].cos(), x[:, 2].sin()
        Ri = torch.stack([c2 * c1, c2 * s1 * s0 - s2 * c0, c2 * s1 * c0 + s2 * s0, s2 * c1, s2 * s1 * s0 + c2 * c0,
                          s2 * s1 * c0 - c2 * s0, -s1, c1 * s0, c1 * c0], 1).view(B, 3, 3)
        R, t = torch.bmm(Ri, R), torch.bmm(Ri, t[:, :, None])[:, :, 0] + x[:, 3:]
    return R.float(), t.float()


def part_bc(blocks, with_torch):
    say(f"## b. a colored round against a point-to-plane round, scan and grid ({ROUNDS} rounds, thresholds 0)"
        + (";  c. the same rounds in torch device ops" if with_torch else ""))
    for B, N in SHAPES:
        c = inputs(B, N)
        grad = colored.compute_color_gradient(c["tgt"], c["nrm"], c["I_t"], K)
        res = {}
        kw = dict(max_iterations=ROUNDS - 1, rel_fitness=0.0, rel_rmse=0.0, want_nn=False)
        col = lambda search: colored.refine_colored(c["src"], c["tgt"], c["I_s"], c["I_t"], c["nrm"], grad, c["R0"], c["t0"],   # noqa: E731
                                                    c["max_dist"], lambda_geometric=LAMBDA, search=search, **kw)
        pla = lambda search: plane.refine_plane(c["src"], c["tgt"], c["nrm"], c["R0"], c["t0"], c["max_dist"], search=search, **kw)   # noqa: E731
        contenders = [
            ("colored, scan", lambda: res.__setitem__("colored, scan", col("scan"))),
            ("point to plane, scan", lambda: res.__setitem__("point to plane, scan", pla("scan"))),
            ("colored, grid", lambda: res.__setitem__("colored, grid", col("grid"))),
            ("point to plane, grid", lambda: res.__setitem__("point to plane, grid", pla("grid"))),
        ]
        if with_torch and B * N <= 16 * 16384:
            contenders.append(("torch colored rounds", lambda: res.__setitem__("torch", torch_colored_rounds(c, grad, ROUNDS))))
        med, times, calls = run_blocks(contenders, blocks)
        head = f"B={B:2d} Ns=Nt={N:6d} max_dist {c['max_dist']:.3f}"
        for name, _ in contenders:
            v = times[name]
            say(f"{head}  {name:22s} {med[name]:10.4f} ms/call  (blocks min {min(v):.4f} max {max(v):.4f}; {blocks} x {calls[name]} calls)")
        for name in ("colored, scan", "point to plane, scan", "colored, grid", "point to plane, grid"):
            if res[name]["iterations"].tolist() != [ROUNDS - 1] * B:   # a cloud that stopped early would make its rounds cheaper
                say(f"{head}  NOTE {name}: updates applied {res[name]['iterations'].tolist()}, not {ROUNDS - 1} each")
        for s in ("scan", "grid"):
            a, b = med[f"colored, {s}"], med[f"point to plane, {s}"]
            say(f"{head}  {s}: a colored round {a / ROUNDS:.4f} ms, a plane round {b / ROUNDS:.4f} ms: colored - plane {(a - b) / ROUNDS:+.4f} ms "
                f"({100 * (a - b) / b:+.1f} %)")
        if "torch" in res:
            dR = (res["torch"][0] - res["colored, scan"]["R"]).abs().max().item()
            say(f"{head}  torch against HIP after {ROUNDS - 1} updates: max |dR| {dR:.2e}; x{med['torch colored rounds'] / med['colored, scan']:.1f} "
                f"the scan, x{med['torch colored rounds'] / med['colored, grid']:.1f} the grid")
        say()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--part", default="abc")
    ap.add_argument("--blocks", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "colored_bench.txt"))
    ap.add_argument("--append", action="store_true", help="add to --out instead of replacing it (one part per run)")
    a = ap.parse_args()
    if not a.append:
        say(f"# kernel_sources_sha16={build.sources_sha16()}")
        say(f"# profiles/bench_colored.py --blocks {a.blocks}: device {torch.cuda.get_device_name(0)}, "
            f"{torch.cuda.get_device_properties(0).multi_processor_count} CUs; ms per call = median of the blocks")
        say()
    if "a" in a.part:
        part_a(a.blocks)
    if "b" in a.part or "c" in a.part:
        part_bc(a.blocks, "c" in a.part)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "a" if a.append else "w") as fh:
        fh.write("\n".join(LINES) + "\n")


if __name__ == "__main__":
    main()
