"""CPU restatement of include/vcr_hip_gicp.h in numpy -- what the tests compare the kernels with --
twice, and the inputs the CPU and GPU tests share.

1. In the header's order (`turned`, `weights`, `gicp_sums`, `gicp_step`, `gicp_icp`): float64 from the fp32 inputs, every
   expression associated as the header writes it, every sum by refine_restated.ordered_sum (the device's order), the pivot rule
   and the Euler step of plane_restated.  numpy's float64 arithmetic rounds as the device's does (no contraction on either
   side), so A and g are the device's up to nothing but the solve.
2. Independently (`independent_x`), to catch a formula copied wrongly into both the kernel and 1: an orthonormal basis
   completed around each normal, C = Rot diag(eps, 1, 1) Rot^T formed explicitly, M = C_t + R C_s R^T, numpy.linalg.inv, a
   square root of W, the rows W^(1/2) [-skew(p) | I] and W^(1/2) d stacked, numpy.linalg.lstsq.

The recipe is refine_restated's on the torus with the ANALYTIC normals of both clouds: plane_restated.pair_normals for the
target, `pair_source_normals` (torus_normals at the source's parameters) for the source."""
import numpy as np

import nnscore_restated as nr
import plane_restated as pr
import refine_restated as rr

F32 = np.float32
F64 = np.float64
MIN_INLIERS = 3
EPSILON = 1e-3


# ------------------------------------------------------------------------------------------------- 1: in the header's order

def turned(R, s):
    """R [3,3], s [3,n] -> n_c = (R[c,0] s0 + R[c,1] s1) + R[c,2] s2 in float64."""
    R, s = np.asarray(R, F64), np.asarray(s, F64)
    return np.stack([(R[c, 0] * s[0] + R[c, 1] * s[1]) + R[c, 2] * s[2] for c in range(3)])


def weights(m, n, epsilon):
    """m, n [3,k] float64 (the neighbour's normal, the turned source normal) -> W [3,3,k]: the header's M, cofactors and det."""
    kap = F64(1.0) - F64(F32(epsilon))
    M = [[None] * 3 for _ in range(3)]
    for i in range(3):
        for j in range(i, 3):
            M[i][j] = (2.0 if i == j else 0.0) - kap * (m[i] * m[j] + n[i] * n[j])
    K00 = M[1][1] * M[2][2] - M[1][2] * M[1][2]
    K01 = M[0][2] * M[1][2] - M[0][1] * M[2][2]
    K02 = M[0][1] * M[1][2] - M[0][2] * M[1][1]
    K11 = M[0][0] * M[2][2] - M[0][2] * M[0][2]
    K12 = M[0][1] * M[0][2] - M[0][0] * M[1][2]
    K22 = M[0][0] * M[1][1] - M[0][1] * M[0][1]
    det = (M[0][0] * K00 + M[0][1] * K01) + M[0][2] * K02
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        W00, W01, W02, W11, W12, W22 = (K / det for K in (K00, K01, K02, K11, K12, K22))
    return np.asarray([[W00, W01, W02], [W01, W11, W12], [W02, W12, W22]])


def _dot(r, p, v):
    """a_r . v for the columns a_r of [-skew(p) | I]."""
    if r == 0:
        return p[1] * v[2] - p[2] * v[1]
    if r == 1:
        return p[2] * v[0] - p[0] * v[2]
    if r == 2:
        return p[0] * v[1] - p[1] * v[0]
    return v[r - 3]


def _u(c, p, W):
    """u_c = W a_c [3,k]."""
    if c == 0:
        return p[1] * W[:, 2] - p[2] * W[:, 1]
    if c == 1:
        return p[2] * W[:, 0] - p[0] * W[:, 2]
    if c == 2:
        return p[0] * W[:, 1] - p[1] * W[:, 0]
    return W[:, c - 3]


def gicp_sums(p, q, m, s, R, inl, epsilon=EPSILON):
    """p [3,n] the moved source, q its neighbours, m their normals, s the source normals (anything where inl is False), R the
    pose that turns s -> (count, A [6,6], g [6]) in float64, every sum in the kernels' order.  A lane that is no inlier has
    zero inputs AND W = 0 (the mask)."""
    z = lambda a: np.where(inl, np.asarray(a, F64), 0.0)     # noqa: E731
    p, q, m, s = z(p), z(q), z(m), z(s)
    n = z(turned(R, s))
    W = np.where(inl, weights(m, n, epsilon), 0.0)
    d = p - q
    A = np.zeros((6, 6))
    with np.errstate(invalid="ignore", over="ignore"):
        for r in range(6):
            for c in range(r, 6):
                A[r, c] = A[c, r] = rr.ordered_sum(_dot(r, p, _u(c, p, W)))
        e = np.stack([(W[i, 0] * d[0] + W[i, 1] * d[1]) + W[i, 2] * d[2] for i in range(3)])
        g = np.asarray([rr.ordered_sum(_dot(r, p, e)) for r in range(6)])
    return int(np.asarray(inl).sum()), A, g


def gicp_step(src, tgt, src_nrm, tgt_nrm, R32, t32, nn_idx, nn_d2, max_dist, epsilon=EPSILON):
    """One update from given neighbours -> dict(R, t: the update in fp64; x, A, g, n, cond); None with fewer than three
    inliers or a singular system; R, t and x NaN where a sum is not finite."""
    limit = F32(max_dist) * F32(max_dist)
    nn_idx = np.asarray(nn_idx)
    with np.errstate(invalid="ignore"):
        inl = (nn_idx >= 0) & (np.asarray(nn_d2, F32) <= limit)
    at = np.maximum(nn_idx, 0)
    n, A, g = gicp_sums(nr.moved(src, R32, t32), np.asarray(tgt, F32)[:, at], np.asarray(tgt_nrm, F32)[:, at],
                        np.asarray(src_nrm, F32), np.asarray(R32, F32), inl, epsilon)
    if n < MIN_INLIERS:
        return None
    if not (np.isfinite(A).all() and np.isfinite(g).all()):
        nan = np.full(6, np.nan)
        return {"R": np.full((3, 3), np.nan), "t": nan[:3], "x": nan, "A": A, "g": g, "n": n, "cond": np.inf}
    if pr.singular(A):
        return None
    x = np.linalg.solve(A, -g)
    R, t = pr.update(x)
    return {"R": R, "t": t, "x": x, "A": A, "g": g, "n": n, "cond": np.linalg.cond(A)}


def gicp_icp(src, tgt, src_nrm, tgt_nrm, R0=None, t0=None, max_dist=0.0, max_iterations=30, rel_fitness=1e-6, rel_rmse=1e-6,
             epsilon=EPSILON):
    """refine_restated.icp's loop with gicp_step: one cloud, src and src_nrm [3,Ns], tgt and tgt_nrm [3,Nt] fp32."""
    R = np.eye(3) if R0 is None else np.asarray(R0, F32).astype(F64)
    t = np.zeros(3) if t0 is None else np.asarray(t0, F32).astype(F64)
    ev = rr.evaluate(src, tgt, R.astype(F32), t.astype(F32), max_dist)
    iterations, converged = 0, 0
    for _ in range(max_iterations):
        up = gicp_step(src, tgt, src_nrm, tgt_nrm, R.astype(F32), t.astype(F32), ev["nn_idx"], ev["nn_d2"], max_dist, epsilon)
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


# ----------------------------------------------------------------------------------------------------------- 2: independently

def basis(n):
    """A rotation whose first column is n / |n|: the other two complete it (Gram-Schmidt from the axis n is least along)."""
    n = np.asarray(n, F64)
    e0 = n / np.linalg.norm(n)
    a = np.zeros(3)
    a[int(np.argmin(np.abs(e0)))] = 1.0
    e1 = a - (a @ e0) * e0
    e1 = e1 / np.linalg.norm(e1)
    return np.stack([e0, e1, np.cross(e0, e1)], axis=1)


def skew(p):
    return np.asarray([[0, -p[2], p[1]], [p[2], 0, -p[0]], [-p[1], p[0], 0]], F64)


def independent_x(p, q, m, s, R, inl, epsilon=EPSILON):
    """The same inputs as gicp_sums -> x [6], the minimiser of sum |W^(1/2) ([-skew(p) | I] x + (p - q))|^2 over the inliers by
    numpy.linalg.lstsq, W = (C_t + R C_s R^T)^-1 from covariances formed explicitly."""
    p, q, m, s, R = (np.asarray(a, F64) for a in (p, q, m, s, R))
    eps = F64(F32(epsilon))
    D = np.diag([eps, 1.0, 1.0])
    rows, rhs = [], []
    for i in np.flatnonzero(inl):
        Bt, Bs = basis(m[:, i]), basis(s[:, i])
        Ct, Cs = Bt @ D @ Bt.T, Bs @ D @ Bs.T
        W = np.linalg.inv(Ct + R @ Cs @ R.T)
        lam, V = np.linalg.eigh((W + W.T) / 2)
        root = V @ np.diag(np.sqrt(lam)) @ V.T
        rows.append(root @ np.concatenate([-skew(p[:, i]), np.eye(3)], axis=1))
        rhs.append(root @ (p[:, i] - q[:, i]))
    x = np.linalg.lstsq(np.concatenate(rows), -np.concatenate(rhs), rcond=None)[0]
    return x


def idealised(m, s, R):
    """(m, s, R) as the definition takes them -- unit normals, a rotation -- to float64's precision: the fp32 normals
    renormalised in float64 and the fp32 pose's nearest rotation.  With fp32 inputs I - (1 - eps) n n^T and Rot diag(eps,1,1)
    Rot^T part by |n|^2 - 1 ~ 2^-23 along the normal, where M is 2 eps: four digits of W, not nine."""
    m, s = np.asarray(m, F64), np.asarray(s, F64)
    U, _, Vt = np.linalg.svd(np.asarray(R, F64))
    return m / np.linalg.norm(m, axis=0), s / np.linalg.norm(s, axis=0), U @ Vt


# ---------------------------------------------------------------------------------------------------------------- the recipe

def pair_source_normals(seed, Nb, Ns, far=(0.0, 0.0, 1.0)):
    """The true normals [3,Ns+FAR] fp32 of rr.pair(seed, Nb, Ns, "torus")'s source, in the source's frame: the recipe's draws
    replayed up to its choice of points, torus_normals at their parameters; the FAR points get `far`."""
    rs = np.random.RandomState(seed)
    u, v = rs.uniform(0, 2 * np.pi, Nb), rs.uniform(0, 2 * np.pi, Nb)
    rs.normal(size=3)
    rs.uniform(-0.5, 0.5, 3)
    rs.permutation(Nb)
    sel = rs.choice(Nb, Ns, replace=Ns > Nb)
    tail = np.tile(np.asarray(far, F64)[:, None], (1, rr.FAR))
    return np.concatenate([pr.torus_normals(u[sel], v[sel]), tail], axis=1).astype(F32)


def batch(seed, Nb, Ns, undisturbed=()):
    """rr.batch on the torus plus "nrm_t" [3,3,Nb] and "nrm_s" [3,3,Ns+FAR], read-only."""
    c = rr.batch(seed, Nb, Ns, "torus", undisturbed)
    ps = [{k: c[k][b] for k in c} for b in range(3)]
    c["nrm_t"] = np.stack([pr.pair_normals(seed + 101 * b, Nb, ps[b]) for b in range(3)])
    c["nrm_s"] = np.stack([pair_source_normals(seed + 101 * b, Nb, Ns) for b in range(3)])
    for v in c.values():
        v.setflags(write=False)
    return c


def tiny(seed=7):
    """B = 1, Ns = 5, Nt = 7: seven points of the torus and five of them, moved off by half a degree and 0.002; the start
    is the identity.  Keys as batch's (leading 1)."""
    rs = np.random.RandomState(seed)
    u, v = rs.uniform(0, 2 * np.pi, 7), rs.uniform(0, 2 * np.pi, 7)
    r = 0.12 * (1 + 0.3 * np.sin(5 * u) * np.cos(3 * v))
    ring = 0.33 + r * np.cos(v)
    tgt = np.stack([0.5 + ring * np.cos(u), 0.5 + ring * np.sin(u), 0.5 + r * np.sin(v) + 0.05 * np.sin(2 * u)])
    nrm = pr.torus_normals(u, v)
    R = rr.rotation([1, -2, 1], 0.5)
    t = np.asarray([0.002, -0.001, 0.0015])
    src = R.T @ (tgt[:, :5] - t[:, None])
    c = {"src": src.astype(F32)[None], "tgt": tgt.astype(F32)[None], "nrm_t": nrm.astype(F32)[None],
         "nrm_s": (R.T @ nrm[:, :5]).astype(F32)[None], "R": R[None], "t": t[None],
         "R0": np.eye(3, dtype=F32)[None], "t0": np.zeros((1, 3), F32), "twin": np.arange(5)[None]}
    for a in c.values():
        a.setflags(write=False)
    return c


def collinear():
    """B = 1, Ns = 3, Nt = 3: three points on a line (coordinates exact in fp32) against themselves moved by 1/64 along x, all
    normals +z: three inliers, a system the pivot rule calls singular (the rotation about the line is free)."""
    tgt = np.asarray([[0.25, 0.5, 0.75], [0.25, 0.5, 0.75], [0.5, 0.5, 0.5]], F32)
    src = tgt + np.asarray([[1 / 64], [0], [0]], F32)
    nrm = np.tile(np.asarray([[0], [0], [1]], F32), (1, 3))
    c = {"src": src[None], "tgt": tgt[None], "nrm_t": nrm[None], "nrm_s": nrm[None].copy()}
    for a in c.values():
        a.setflags(write=False)
    return c
