"""CPU restatement of vcr_refine_f32 (include/vcr_hip_refine.h) in numpy -- what the tests compare the
kernels with -- and the input recipe the CPU and GPU tests share.

The search, the inlier rule and the evaluation are tests/nnscore_restated.py's (the kernel's fp32 chain, its summation order);
the covariance follows the same order (`covariance`: sixteen fp64 sums over the inliers, per 256 source points the wave
butterfly, the four waves ascending, the partials ascending); the solve is numpy.linalg.svd in fp64 with the reflection rule
(`solve`), where the device runs a Jacobi SVD -- so a step is held to this one by properties (a proper rotation, optimal for the
covariance), never bit for bit.  `step` runs one update from GIVEN neighbours, `icp` the whole loop for one cloud."""
import numpy as np

import nnscore_restated as nr

F32 = np.float32


def ordered_sum(values):
    """float64 [n] -> their sum in the kernels' order (nnscore_restated.block_partials, then ascending)."""
    total = np.float64(0.0)
    for s in nr.block_partials(np.asarray(values, np.float64)):
        total = total + s
    return total


def covariance(p, q, inl):
    """p [3,n] the moved source (fp32), q [3,n] its neighbours (fp32; anything where inl is False), inl bool [n] ->
    (count, S_p [3], S_q [3], S_pq [3,3]) in fp64.  The product of two fp32 values is exact in float64."""
    p = np.where(inl, np.asarray(p, F32), F32(0)).astype(np.float64)
    q = np.where(inl, np.asarray(q, F32), F32(0)).astype(np.float64)
    Sp = np.asarray([ordered_sum(p[c]) for c in range(3)])
    Sq = np.asarray([ordered_sum(q[c]) for c in range(3)])
    Spq = np.asarray([[ordered_sum(p[r] * q[c]) for c in range(3)] for r in range(3)])
    return int(inl.sum()), Sp, Sq, Spq


def cross(n, Sp, Sq, Spq):
    """H = S_pq - S_p S_q^T / n."""
    return Spq - np.outer(Sp, Sq) / np.float64(n)


def solve(H):
    """H = sum (p - pm)(q - qm)^T [3,3] fp64 -> (R with q ~ R p, opt = s1 + s2 + d s3, s1): R = V U^T, the column of V of the
    smallest singular value flipped when det < 0."""
    U, s, Vt = np.linalg.svd(H)
    V = Vt.T
    d = 1.0 if np.linalg.det(V @ U.T) >= 0 else -1.0
    R = V @ np.diag([1.0, 1.0, d]) @ U.T
    return R, s[0] + s[1] + d * s[2], s[0]


def step(src, tgt, R32, t32, nn_idx, nn_d2, max_dist):
    """One update from given neighbours: src [3,Ns], tgt [3,Nt] fp32 under the fp32 pose (R32, t32) ->
    dict(R, t: the update in fp64; H, n, pm, qm, opt, s1), or None with fewer than three inliers."""
    limit = F32(max_dist) * F32(max_dist)
    nn_idx = np.asarray(nn_idx)
    inl = (nn_idx >= 0) & (np.asarray(nn_d2, F32) <= limit)
    p = nr.moved(src, R32, t32)
    q = np.asarray(tgt, F32)[:, np.maximum(nn_idx, 0)]
    n, Sp, Sq, Spq = covariance(p, q, inl)
    if n < 3:
        return None
    H = cross(n, Sp, Sq, Spq)
    R, opt, s1 = solve(H)
    pm, qm = Sp / n, Sq / n
    return {"R": R, "t": qm - R @ pm, "H": H, "n": n, "pm": pm, "qm": qm, "opt": opt, "s1": s1}


def evaluate(src, tgt, R32, t32, max_dist):
    idx, d2 = nr.nearest_f32(nr.moved(src, R32, t32), np.ascontiguousarray(tgt, dtype=F32))
    c, s, f, r = nr.summary(idx, d2, max_dist)
    return {"nn_idx": idx, "nn_d2": d2, "inliers": c, "sum_d2": s, "fitness": f, "rmse": r}


def icp(src, tgt, R0=None, t0=None, max_dist=0.0, max_iterations=30, rel_fitness=1e-6, rel_rmse=1e-6):
    """The loop of include/vcr_hip_refine.h for ONE cloud: src [3,Ns], tgt [3,Nt] fp32.  The pose runs in float64; the search
    sees its fp32 rounding.  Returns the last evaluation's dict plus R, t (fp32), iterations, converged."""
    R = np.eye(3) if R0 is None else np.asarray(R0, F32).astype(np.float64)
    t = np.zeros(3) if t0 is None else np.asarray(t0, F32).astype(np.float64)
    ev = evaluate(src, tgt, R.astype(F32), t.astype(F32), max_dist)
    iterations, converged = 0, 0
    for _ in range(max_iterations):
        up = step(src, tgt, R.astype(F32), t.astype(F32), ev["nn_idx"], ev["nn_d2"], max_dist)
        if up is None:
            break
        R, t = up["R"] @ R, up["R"] @ t + up["t"]
        iterations += 1
        nxt = evaluate(src, tgt, R.astype(F32), t.astype(F32), max_dist)
        done = abs(F32(nxt["fitness"] - ev["fitness"])) < F32(rel_fitness) and abs(F32(nxt["rmse"] - ev["rmse"])) < F32(rel_rmse)
        ev = nxt
        if done:
            converged = 1
            break
    return dict(ev, R=R.astype(F32), t=t.astype(F32), iterations=iterations, converged=converged)


# ---------------------------------------------------------------------------------------------------------------- the recipe

FAR = 37                                                   # source points without a partner, in [2,3]^3
MAX_DIST = 0.1
SHAPES = ((700, 300), (1500, 1100), (2600, 2100))          # (Nb, Ns): target points, clean source points


def rotation(axis, degrees):
    a = np.asarray(axis, np.float64)
    a = a / np.linalg.norm(a)
    K = np.asarray([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    th = np.deg2rad(degrees)
    return np.eye(3) + np.sin(th) * K + (1 - np.cos(th)) * (K @ K)


def base_cloud(rs, n, kind):
    """[3, n] float64 inside the unit cube: uniform, or a torus whose tube radius varies along both angles."""
    if kind == "cube":
        return rs.uniform(0.0, 1.0, (3, n))
    u, v = rs.uniform(0, 2 * np.pi, n), rs.uniform(0, 2 * np.pi, n)
    r = 0.12 * (1 + 0.3 * np.sin(5 * u) * np.cos(3 * v))
    ring = 0.33 + r * np.cos(v)
    return np.stack([0.5 + ring * np.cos(u), 0.5 + ring * np.sin(u), 0.5 + r * np.sin(v) + 0.05 * np.sin(2 * u)])


def pair(seed, Nb, Ns, kind="cube", disturb=True):
    """One cloud of the recipe -> dict: tgt [3,Nb] fp32 = the Nb points under a random 40-degree pose, permuted; src
    [3,Ns+FAR] fp32 = Ns of the points (a random choice -- with repeats only where Ns > Nb -- the FAR far ones behind them);
    R, t the planted pose (float64); twin int [Ns]: the target index of every clean source point; R0, t0 (fp32) the start, the planted pose disturbed by 6
    degrees (about the source frame's origin) and 0.04 -- or the planted pose itself."""
    rs = np.random.RandomState(seed)
    base = base_cloud(rs, Nb, kind).astype(F32)
    R = rotation(rs.normal(size=3), 40.0)
    t = rs.uniform(-0.5, 0.5, 3)
    perm = rs.permutation(Nb)                               # target column j holds base point perm[j]
    tgt = (R @ base.astype(np.float64) + t[:, None]).astype(F32)[:, perm]
    where = np.empty(Nb, np.int64)
    where[perm] = np.arange(Nb)
    sel = rs.choice(Nb, Ns, replace=Ns > Nb)
    far = rs.uniform(2.0, 3.0, (3, FAR)).astype(F32)
    src = np.concatenate([base[:, sel], far], axis=1)
    R0, t0 = R, t
    if disturb:
        d = rs.normal(size=3)
        R0, t0 = R @ rotation(rs.normal(size=3), 6.0), t + 0.04 * d / np.linalg.norm(d)
    return {"src": np.ascontiguousarray(src), "tgt": np.ascontiguousarray(tgt), "R": R, "t": t, "twin": where[sel],
            "R0": R0.astype(F32), "t0": t0.astype(F32)}


def batch(seed, Nb, Ns, kind="cube", undisturbed=()):
    """Three clouds of the recipe, stacked: src [3,3,Ns+FAR], tgt [3,3,Nb], R, t, twin, R0, t0 with a leading 3."""
    ps = [pair(seed + 101 * b, Nb, Ns, kind, disturb=b not in undisturbed) for b in range(3)]
    return {k: np.stack([p[k] for p in ps]) for k in ps[0]}
