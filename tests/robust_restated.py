"""CPU restatement of include/robust/vcr_hip_robust.h in numpy -- what the tests compare the kernels
with -- and the contaminated input the CPU and GPU tests share.

`weight` is the header's five weights in its expressions; `robust_sums` are plane_restated.plane_sums with Jw = w J in front
of the products, `robust_step` one update from GIVEN neighbours, `robust_icp` the whole loop for one cloud -- on
plane_restated's `singular` and `update` and refine_restated's `ordered_sum` and `evaluate`.  `information` is the header's
matrix from nine ordered sums; `information_gtg` the plain float64 sum of G^T G over Open3D's three rows a pair, by which the
tests prove the layout.  `contaminated` is refine_restated's torus pair with a share of its clean source points pushed off the
surface, inside MAX_DIST."""
import functools

import numpy as np

import nnscore_restated as nr
import plane_restated as pr
import refine_restated as rr

F32 = np.float32
LOSSES = ("l2", "huber", "cauchy", "gm", "tukey")          # VCR_LOSS_*: a loss' value is its index


def weight(loss, k, r):
    """The header's weight of the residual r (float64, any shape) under `loss` with the scale k (the fp32 argument widened)."""
    r = np.asarray(r, np.float64)
    k = np.float64(F32(k))
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        if loss == "l2":
            return np.ones_like(r)
        if loss == "huber":
            a = np.abs(r)
            return np.where(a <= k, 1.0, k / a)
        if loss == "cauchy":
            u = r / k
            return 1.0 / (1.0 + u * u)
        if loss == "gm":
            s = k + r * r
            return k / (s * s)
        if loss == "tukey":
            a, u = np.abs(r), r / k
            v = 1.0 - u * u
            return np.where(a <= k, v * v, 0.0)
    raise ValueError(loss)


def robust_sums(p, q, nrm, inl, loss, k):
    """plane_restated.plane_sums with the weight: Jw = w J, A = sum Jw J^T, g = sum Jw r over the inliers, every sum in the
    kernels' order -> (count, A [6,6], g [6])."""
    z = lambda a: np.where(inl, np.asarray(a, F32), F32(0)).astype(np.float64)   # noqa: E731
    p, q, m = z(p), z(q), z(nrm)
    res = ((p[0] * m[0] + p[1] * m[1]) + p[2] * m[2]) - ((q[0] * m[0] + q[1] * m[1]) + q[2] * m[2])
    J = np.stack([p[1] * m[2] - p[2] * m[1], p[2] * m[0] - p[0] * m[2], p[0] * m[1] - p[1] * m[0], m[0], m[1], m[2]])
    with np.errstate(invalid="ignore", over="ignore"):
        Jw = weight(loss, k, res) * J
        A = np.zeros((6, 6))
        for r in range(6):
            for c in range(r, 6):
                A[r, c] = A[c, r] = rr.ordered_sum(Jw[r] * J[c])
        g = np.asarray([rr.ordered_sum(Jw[r] * res) for r in range(6)])
    return int(inl.sum()), A, g


def robust_step(src, tgt, nrm, R32, t32, nn_idx, nn_d2, max_dist, loss, k):
    """One update from given neighbours -> dict(R, t: the update in fp64; x, A, g, n, cond), or None with fewer than six
    inliers or a singular system.  Non-finite sums: a NaN update, as the device's."""
    limit = F32(max_dist) * F32(max_dist)
    nn_idx = np.asarray(nn_idx)
    inl = (nn_idx >= 0) & (np.asarray(nn_d2, F32) <= limit)
    at = np.maximum(nn_idx, 0)
    n, A, g = robust_sums(nr.moved(src, R32, t32), np.asarray(tgt, F32)[:, at], np.asarray(nrm, F32)[:, at], inl, loss, k)
    if n < pr.MIN_INLIERS:
        return None
    if not (np.isfinite(A).all() and np.isfinite(g).all()):
        return {"R": np.full((3, 3), np.nan), "t": np.full(3, np.nan), "x": np.full(6, np.nan), "A": A, "g": g, "n": n, "cond": np.nan}
    if pr.singular(A):
        return None
    x = np.linalg.solve(A, -g)
    R, t = pr.update(x)
    return {"R": R, "t": t, "x": x, "A": A, "g": g, "n": n, "cond": np.linalg.cond(A)}


def robust_icp(src, tgt, nrm, R0=None, t0=None, max_dist=0.0, loss="tukey", k=0.02, max_iterations=30, rel_fitness=1e-6,
               rel_rmse=1e-6):
    """plane_restated.plane_icp's loop with robust_step: one cloud, src [3,Ns], tgt and nrm [3,Nt] fp32."""
    R = np.eye(3) if R0 is None else np.asarray(R0, F32).astype(np.float64)
    t = np.zeros(3) if t0 is None else np.asarray(t0, F32).astype(np.float64)
    ev = rr.evaluate(src, tgt, R.astype(F32), t.astype(F32), max_dist)
    iterations, converged = 0, 0
    for _ in range(max_iterations):
        up = robust_step(src, tgt, nrm, R.astype(F32), t.astype(F32), ev["nn_idx"], ev["nn_d2"], max_dist, loss, k)
        if up is None:
            break
        R, t = up["R"] @ R, up["R"] @ t + up["t"]
        iterations += 1
        nxt = rr.evaluate(src, tgt, R.astype(F32), t.astype(F32), max_dist)
        done = abs(F32(nxt["fitness"] - ev["fitness"])) < F32(rel_fitness) and abs(F32(nxt["rmse"] - ev["rmse"])) < F32(rel_rmse)
        ev = nxt
        if done:
            converged = 1
            break
    return dict(ev, R=R.astype(F32), t=t.astype(F32), iterations=iterations, converged=converged)


# ------------------------------------------------------------------------------------------------------ the information matrix

def _inliers(nn_idx, nn_d2, max_dist):
    nn_idx = np.asarray(nn_idx)
    return (nn_idx >= 0) & (np.asarray(nn_d2, F32) <= F32(max_dist) * F32(max_dist))


def information(tgt, nn_idx, nn_d2, max_dist):
    """One cloud: tgt [3,Nt] fp32 and the neighbours of its source points -> the header's matrix, float64 [6,6], from nine sums
    in the kernels' order over the inliers' neighbours (a target point once per source point that chose it)."""
    inl = _inliers(nn_idx, nn_d2, max_dist)
    q = np.where(inl, np.asarray(tgt, F32)[:, np.maximum(np.asarray(nn_idx), 0)], F32(0)).astype(np.float64)
    x, y, z = q
    with np.errstate(invalid="ignore", over="ignore"):
        Sx, Sy, Sz, Sxx, Syy, Szz, Sxy, Sxz, Syz = (rr.ordered_sum(v) for v in (x, y, z, x * x, y * y, z * z, x * y, x * z, y * z))
        n = np.float64(inl.sum())
        return np.asarray([[Syy + Szz, -Sxy, -Sxz, 0, -Sz, Sy],
                           [-Sxy, Sxx + Szz, -Syz, Sz, 0, -Sx],
                           [-Sxz, -Syz, Sxx + Syy, -Sy, Sx, 0],
                           [0, Sz, -Sy, n, 0, 0],
                           [-Sz, 0, Sx, 0, n, 0],
                           [Sy, -Sx, 0, 0, 0, n]], np.float64)


def information_gtg(tgt, nn_idx, nn_d2, max_dist):
    """The same matrix as Open3D builds it: per inlier the three rows G_r = [ -[q]x | I ], summed as G^T G in plain float64."""
    inl = _inliers(nn_idx, nn_d2, max_dist)
    GTG = np.zeros((6, 6))
    for j in np.asarray(nn_idx)[inl]:
        x, y, z = np.asarray(tgt, F32)[:, j].astype(np.float64)
        G = np.asarray([[0, z, -y, 1, 0, 0],                    # Open3D: G_r1(1) = z, G_r1(2) = -y, G_r1(3) = 1
                        [-z, 0, x, 0, 1, 0],                    #         G_r2(0) = -z, G_r2(2) = x, G_r2(4) = 1
                        [y, -x, 0, 0, 0, 1]], np.float64)       #         G_r3(0) = y, G_r3(1) = -x, G_r3(5) = 1
        GTG += G.T @ G
    return GTG


# ---------------------------------------------------------------------------------------------------------------- the recipe

def contaminated(seed, Nb, Ns, share=0.25, lo=0.03, hi=0.07, direction=(0.6, 0, 0.8)):
    """rr.pair(seed, Nb, Ns, "torus") with `share` of its clean source points pushed lo ... hi along `direction` (in the
    source's frame: inside MAX_DIST of where they were, and wrong), plus "nrm": the target's TRUE normals
    (plane_restated.pair_normals) and "pushed": which source points moved.  The far points and the poses are the pair's."""
    p = rr.pair(seed, Nb, Ns, "torus")
    rs = np.random.RandomState(seed + 1000)                  # (draws of its own: the pair keeps rr.pair's)
    pushed = np.zeros(Ns + rr.FAR, bool)
    pushed[rs.choice(Ns, int(round(share * Ns)), replace=False)] = True
    d = np.asarray(direction, np.float64)
    d = d / np.linalg.norm(d)
    src = p["src"].astype(np.float64)
    src[:, pushed] += d[:, None] * rs.uniform(lo, hi, int(pushed.sum()))[None, :]
    return dict(p, src=np.ascontiguousarray(src.astype(F32)), clean=p["src"], pushed=pushed, nrm=pr.pair_normals(seed, Nb, p))


@functools.lru_cache(maxsize=None)
def fits(seed, Nb, Ns, updates=20):
    """The recipe's pair and the three restated fits the accuracy tests rest on, `updates` updates each with the thresholds 0:
    "ls" (least squares) and "cauchy" (k = 0.01) from the recipe's start, "tukey" (k = 0.02) from the least-squares result.
    Computed once a session and shared (read-only)."""
    c = contaminated(seed, Nb, Ns)
    a = (c["src"], c["tgt"], c["nrm"])
    ls = robust_icp(*a, c["R0"], c["t0"], rr.MAX_DIST, "l2", 1.0, updates, 0.0, 0.0)
    cauchy = robust_icp(*a, c["R0"], c["t0"], rr.MAX_DIST, "cauchy", 0.01, updates, 0.0, 0.0)
    tukey = robust_icp(*a, ls["R"], ls["t"], rr.MAX_DIST, "tukey", 0.02, updates, 0.0, 0.0)
    for d in (c, ls, cauchy, tukey):
        for v in d.values():
            if isinstance(v, np.ndarray):
                v.setflags(write=False)
    return {"c": c, "ls": ls, "cauchy": cauchy, "tukey": tukey}
