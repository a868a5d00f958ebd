"""CPU restatement of include/vcr_hip_plane.h in numpy -- what the tests compare the kernels with --
and the inputs the CPU and GPU tests share.

Normals: `covariance` / `covariances` are the header's nine fp64 sums in idx's order and its C; `normal` is numpy.linalg.eigh
with the header's sign rules (the device runs a Jacobi: held to this one by bounds, never bit for bit).  Point to plane:
`plane_sums` are the header's A and g in refine_restated.ordered_sum's order, `plane_step` one update from GIVEN neighbours by
numpy.linalg.solve, `plane_icp` the whole loop for one cloud.  The recipe is refine_restated's (`pair`, `base_cloud("torus")`);
`torus_frame` replays its draws to give the analytic normals of its torus."""
import numpy as np

import nnscore_restated as nr
import refine_restated as rr

F32 = np.float32
PIVOT = 1e-12
MIN_INLIERS = 6


# ------------------------------------------------------------------------------------------------------------------ normals

def covariances(x, idx):
    """x [3,N] fp32, idx int [N,k] -> C float64 [N,3,3] over the k + 1 rows {i} U idx[i] (an entry outside [0, N) reads as i):
    d = x_j - x_i in fp32, nine fp64 sums over j in idx's order, C = S_dd / m - (S_d / m)(S_d / m)^T."""
    x = np.asarray(x, F32)
    N, k = idx.shape
    own = np.arange(N)
    Sd, Sdd = np.zeros((N, 3)), np.zeros((N, 3, 3))
    for j in range(k):
        r = np.where((idx[:, j] >= 0) & (idx[:, j] < N), idx[:, j], own)
        d = (x[:, r] - x[:, own]).astype(np.float64).T           # the fp32 difference, widened
        Sd = Sd + d
        Sdd = Sdd + d[:, :, None] * d[:, None, :]                 # products of two fp32 values: exact
    m = np.float64(k + 1)
    mean = Sd / m
    with np.errstate(invalid="ignore", over="ignore"):
        return Sdd / m - mean[:, :, None] * mean[:, None, :]


def covariance(x, i, idx_row):
    """One point's C [3,3]: `covariances` for the row i alone."""
    idx = np.full((x.shape[1], len(idx_row)), -1, np.int64)
    idx[i] = idx_row
    return covariances(x, idx)[i]


def orient(n, x_i=None, viewpoint=None):
    """The header's sign rules on the fp32 normal n [3]."""
    n = np.asarray(n, F32)
    dot = 0.0
    if viewpoint is not None:
        w = np.asarray(viewpoint, F32).astype(np.float64) - np.asarray(x_i, F32).astype(np.float64)
        nd = n.astype(np.float64)
        dot = (nd[0] * w[0] + nd[1] * w[1]) + nd[2] * w[2]
    flip = dot < 0
    if not dot < 0 and not dot > 0:
        flip = n[int(np.argmax(np.abs(n)))] < 0                   # (argmax: the lowest index among equals)
    return -n if flip else n


def normal(C, x_i=None, viewpoint=None):
    """C [3,3] float64 -> (n fp32 [3], lambda [3] ascending, curvature fp32) by numpy.linalg.eigh and the header's rules."""
    if not np.isfinite(C).all():
        return np.asarray([0, 0, 1], F32), np.full(3, np.nan), F32(np.nan)
    if not C.any():
        return np.asarray([0, 0, 1], F32), np.zeros(3), F32(0)
    lam, V = np.linalg.eigh(C)
    tr = (lam[0] + lam[1]) + lam[2]
    return orient(V[:, 0].astype(F32), x_i, viewpoint), lam, F32(0) if tr == 0 else F32(lam[0] / tr)


def knn_f64(x, k):
    """x [3,N] fp32 -> int64 [N,k]: the k nearest rows in float64, the row itself first (a CPU stand-in for the library's kNN:
    the tests that compare with the device use the device's idx)."""
    x = np.asarray(x, F32).astype(np.float64)
    d = ((x[:, :, None] - x[:, None, :]) ** 2).sum(0)
    return np.argsort(d, axis=1, kind="stable")[:, :k]


def jittered_torus(seed, N, jitter=0.002):
    """[3,N] fp32: refine_restated's torus with every coordinate moved by up to `jitter` -- no exactly planar or collinear
    neighbourhood, and the two smallest eigenvalues apart almost everywhere."""
    rs = np.random.RandomState(seed)
    return (rr.base_cloud(rs, N, "torus") + rs.uniform(-jitter, jitter, (3, N))).astype(F32)


# ------------------------------------------------------------------------------------------------------------ point to plane

def plane_sums(p, q, nrm, inl):
    """p [3,n] the moved source, q [3,n] its neighbours, nrm [3,n] their normals (fp32; anything where inl is False) ->
    (count, A [6,6], g [6]) in float64: r = p.nrm - q.nrm, J = (p x nrm, nrm), A = sum J J^T, g = sum J r over the inliers,
    every sum in the kernels' order."""
    z = lambda a: np.where(inl, np.asarray(a, F32), F32(0)).astype(np.float64)   # noqa: E731
    p, q, m = z(p), z(q), z(nrm)
    res = ((p[0] * m[0] + p[1] * m[1]) + p[2] * m[2]) - ((q[0] * m[0] + q[1] * m[1]) + q[2] * m[2])
    J = np.stack([p[1] * m[2] - p[2] * m[1], p[2] * m[0] - p[0] * m[2], p[0] * m[1] - p[1] * m[0], m[0], m[1], m[2]])
    A = np.zeros((6, 6))
    for r in range(6):
        for c in range(r, 6):
            A[r, c] = A[c, r] = rr.ordered_sum(J[r] * J[c])
    g = np.asarray([rr.ordered_sum(J[r] * res) for r in range(6)])
    return int(inl.sum()), A, g


def singular(A):
    """The header's rule: a Cholesky pivot that is not finite or not above 1e-12 times its diagonal entry of A."""
    L = np.zeros((6, 6))
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        for j in range(6):
            s = A[j, j] - (L[j, :j] ** 2).sum()
            if not (np.isfinite(s) and s > PIVOT * A[j, j]):
                return True
            L[j, j] = np.sqrt(s)
            for i in range(j + 1, 6):
                L[i, j] = (A[i, j] - (L[i, :j] * L[j, :j]).sum()) / L[j, j]
    return False


def update(x):
    """x [6] -> (R_i = Rz(x2) Ry(x1) Rx(x0), t_i = x[3:]): Open3D's TransformVector6dToMatrix4d."""
    c, s = np.cos(x[:3]), np.sin(x[:3])
    Rx = np.asarray([[1, 0, 0], [0, c[0], -s[0]], [0, s[0], c[0]]])
    Ry = np.asarray([[c[1], 0, s[1]], [0, 1, 0], [-s[1], 0, c[1]]])
    Rz = np.asarray([[c[2], -s[2], 0], [s[2], c[2], 0], [0, 0, 1]])
    return Rz @ Ry @ Rx, np.asarray(x[3:], np.float64)


def plane_step(src, tgt, nrm, R32, t32, nn_idx, nn_d2, max_dist):
    """One update from given neighbours -> dict(R, t: the update in fp64; x, A, g, n, cond), or None with fewer than six
    inliers or a singular system."""
    limit = F32(max_dist) * F32(max_dist)
    nn_idx = np.asarray(nn_idx)
    inl = (nn_idx >= 0) & (np.asarray(nn_d2, F32) <= limit)
    at = np.maximum(nn_idx, 0)
    n, A, g = plane_sums(nr.moved(src, R32, t32), np.asarray(tgt, F32)[:, at], np.asarray(nrm, F32)[:, at], inl)
    if n < MIN_INLIERS or singular(A):
        return None
    x = np.linalg.solve(A, -g)
    R, t = update(x)
    return {"R": R, "t": t, "x": x, "A": A, "g": g, "n": n, "cond": np.linalg.cond(A)}


def plane_icp(src, tgt, nrm, R0=None, t0=None, max_dist=0.0, max_iterations=30, rel_fitness=1e-6, rel_rmse=1e-6):
    """refine_restated.icp's loop with plane_step: one cloud, src [3,Ns], tgt and nrm [3,Nt] fp32."""
    R = np.eye(3) if R0 is None else np.asarray(R0, F32).astype(np.float64)
    t = np.zeros(3) if t0 is None else np.asarray(t0, F32).astype(np.float64)
    ev = rr.evaluate(src, tgt, R.astype(F32), t.astype(F32), max_dist)
    iterations, converged = 0, 0
    for _ in range(max_iterations):
        up = plane_step(src, tgt, nrm, R.astype(F32), t.astype(F32), ev["nn_idx"], ev["nn_d2"], max_dist)
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


def pose_error(R, t, R_true, t_true):
    """(rotation error in radians, |t - t_true|).  The angle of R R_true^T from its skew part (sin) and its trace (cos): the
    arc cosine of the trace alone resolves nothing below the square root of the entries' rounding."""
    D = np.asarray(R, np.float64) @ np.asarray(R_true, np.float64).T
    sin = 0.5 * np.linalg.norm([D[2, 1] - D[1, 2], D[0, 2] - D[2, 0], D[1, 0] - D[0, 1]])
    return (float(np.arctan2(sin, (np.trace(D) - 1) / 2)),
            float(np.linalg.norm(np.asarray(t, np.float64) - np.asarray(t_true, np.float64))))


# ---------------------------------------------------------------------------------------------------------------- the recipe

def torus_normals(u, v):
    """Unit normals [3,n] of refine_restated.base_cloud's torus at the angles (u, v): P_u x P_v of its parametrisation."""
    r = 0.12 * (1 + 0.3 * np.sin(5 * u) * np.cos(3 * v))
    ru, rv = 0.12 * 0.3 * 5 * np.cos(5 * u) * np.cos(3 * v), -0.12 * 0.3 * 3 * np.sin(5 * u) * np.sin(3 * v)
    ring = 0.33 + r * np.cos(v)
    ring_u, ring_v = ru * np.cos(v), rv * np.cos(v) - r * np.sin(v)
    Pu = np.stack([ring_u * np.cos(u) - ring * np.sin(u), ring_u * np.sin(u) + ring * np.cos(u), ru * np.sin(v) + 0.1 * np.cos(2 * u)])
    Pv = np.stack([ring_v * np.cos(u), ring_v * np.sin(u), rv * np.sin(v) + r * np.cos(v)])
    n = np.cross(Pu, Pv, axis=0)
    return n / np.linalg.norm(n, axis=0)


def pair_normals(seed, Nb, p):
    """The true normals [3,Nb] fp32 of rr.pair(seed, Nb, ., "torus")'s target p["tgt"]: its first draws replayed."""
    rs = np.random.RandomState(seed)
    u, v = rs.uniform(0, 2 * np.pi, Nb), rs.uniform(0, 2 * np.pi, Nb)
    rs.normal(size=3)
    rs.uniform(-0.5, 0.5, 3)
    perm = rs.permutation(Nb)
    return (p["R"] @ torus_normals(u, v)).astype(F32)[:, perm]
