"""CPU restatement of include/colored/vcr_hip_colored.h in numpy -- what the tests compare the kernels
with -- and the inputs the CPU and GPU tests share.

1. In the header's order: `gradient` (the nine fp64 sums over a row in idx's order, the extra row m^2 n n^T, the pivot rule;
   the 3 x 3 solve is numpy's, where the device runs the Cholesky itself), `colored_sums` / `colored_step` / `colored_icp` (float64
   from the fp32 inputs, every expression associated as the header writes it, every sum by refine_restated.ordered_sum, the
   pivot rule and the Euler step of plane_restated).
2. Independently (`independent_x`, `residuals`): the stacked residual rows solved by numpy.linalg.lstsq, and the residuals as
   functions of the six unknowns for a finite-difference check of J_G and J_I.

The recipe (`pair`, `batch`): a textured patch over [0,1]^2 -- "flat" (z = 0) or "bowl" (z = 0.15 (u - 0.5)^2 + 0.1 (v - 0.5)^2) --
with analytic normals and the intensity I(u, v) below; the target Nt points uniform on the patch under a planted 40-degree
pose, the source Ns INDEPENDENT points on [0.1, 0.9]^2 (no source point is a target point); the start is the planted pose
composed with 2 degrees about the patch's z axis and a slide of (0.03, -0.02, 0) in the patch's frame: a slide along the
surface, which geometry alone cannot take back."""
import numpy as np

import nnscore_restated as nr
import plane_restated as pr
import refine_restated as rr

F32 = np.float32
F64 = np.float64
MIN_INLIERS = 6
LAMBDA = 0.968
MAX_DIST = 0.07
K = 20
PIVOT = 1e-12
SHAPES = ((700, 300), (1500, 900))                         # (Nt, Ns)
KINDS = ("flat", "bowl")
SLIDE = (0.03, -0.02, 0.0)
TWIST = 2.0                                                # degrees about the patch's z axis


# ---------------------------------------------------------------------------------------------------------------- the patch

def height(kind, u, v):
    return np.zeros_like(u) if kind == "flat" else 0.15 * (u - 0.5) ** 2 + 0.1 * (v - 0.5) ** 2


def patch_normals(kind, u, v):
    """Unit normals [3,n] in the patch's frame."""
    zu, zv = (np.zeros_like(u), np.zeros_like(v)) if kind == "flat" else (0.3 * (u - 0.5), 0.2 * (v - 0.5))
    n = np.stack([-zu, -zv, np.ones_like(u)])
    return n / np.linalg.norm(n, axis=0)


def intensity(u, v):
    return 0.5 + 0.25 * np.sin(9 * u + 1) * np.cos(7 * v) + 0.2 * np.sin(5 * v - 0.5 * u)


def intensity_gradient(kind, u, v):
    """The gradient of I ON the surface [3,n], in the patch's frame: the tangent vector g with g . P_u = I_u, g . P_v = I_v."""
    Iu = 0.25 * 9 * np.cos(9 * u + 1) * np.cos(7 * v) - 0.2 * 0.5 * np.cos(5 * v - 0.5 * u)
    Iv = -0.25 * 7 * np.sin(9 * u + 1) * np.sin(7 * v) + 0.2 * 5 * np.cos(5 * v - 0.5 * u)
    zu, zv = (np.zeros_like(u), np.zeros_like(v)) if kind == "flat" else (0.3 * (u - 0.5), 0.2 * (v - 0.5))
    E, Fm, G = 1 + zu * zu, zu * zv, 1 + zv * zv                # the first fundamental form of (u, v, z(u, v))
    det = E * G - Fm * Fm
    a, b = (G * Iu - Fm * Iv) / det, (E * Iv - Fm * Iu) / det
    return np.stack([a, b, a * zu + b * zv])


def pair(kind, seed, Nt, Ns):
    """One cloud of the recipe -> dict: tgt [3,Nt], src [3,Ns] fp32; nrm_t [3,Nt] the target's analytic normals and grad_t
    [3,Nt] its analytic colour gradients, both in the target's frame; I_t [Nt], I_s [Ns] fp32; R, t the planted pose (float64);
    R0, t0 (fp32) the start; uv_t [2,Nt]."""
    rs = np.random.RandomState(seed)
    us, vs = rs.uniform(0.1, 0.9, Ns), rs.uniform(0.1, 0.9, Ns)
    ut, vt = rs.uniform(0.0, 1.0, Nt), rs.uniform(0.0, 1.0, Nt)
    R = rr.rotation(rs.normal(size=3), 40.0)
    t = rs.uniform(-0.5, 0.5, 3)
    base_t = np.stack([ut, vt, height(kind, ut, vt)])
    base_s = np.stack([us, vs, height(kind, us, vs)]).astype(F32)
    tgt = (R @ base_t + t[:, None]).astype(F32)
    R0 = R @ rr.rotation([0, 0, 1], TWIST)
    t0 = t + R @ np.asarray(SLIDE)
    return {"src": np.ascontiguousarray(base_s), "tgt": np.ascontiguousarray(tgt),
            "nrm_t": (R @ patch_normals(kind, ut, vt)).astype(F32), "grad_t": R @ intensity_gradient(kind, ut, vt),
            "I_t": intensity(ut, vt).astype(F32), "I_s": intensity(us, vs).astype(F32), "R": R, "t": t,
            "R0": R0.astype(F32), "t0": t0.astype(F32), "uv_t": np.stack([ut, vt])}


def batch(kind, seed, Nt, Ns, B=3):
    """B clouds of the recipe (seeds seed + 101 b), stacked and read-only."""
    ps = [pair(kind, seed + 101 * b, Nt, Ns) for b in range(B)]
    c = {k: np.stack([p[k] for p in ps]) for k in ps[0]}
    for v in c.values():
        v.setflags(write=False)
    return c


def tiny(seed=7, Ns=6):
    """B = 1, Ns = 6, Nt = 7 on the bowl: seven points, the first Ns of them moved off by half a degree and 0.002 with their own
    colours; the start is the identity, every point an inlier.  Six is the fewest a step takes (MIN_INLIERS): Ns = 5 is the
    case that stops.  The gradients are the analytic ones.  Keys as batch's."""
    rs = np.random.RandomState(seed)
    u, v = rs.uniform(0.2, 0.8, 7), rs.uniform(0.2, 0.8, 7)
    tgt = np.stack([u, v, height("bowl", u, v)])
    R = rr.rotation([1, -2, 1], 0.5)
    t = np.asarray([0.002, -0.001, 0.0015])
    src = R.T @ (tgt[:, :Ns] - t[:, None])
    c = {"src": src.astype(F32)[None], "tgt": tgt.astype(F32)[None], "nrm_t": patch_normals("bowl", u, v).astype(F32)[None],
         "grad_t": intensity_gradient("bowl", u, v)[None], "I_t": intensity(u, v).astype(F32)[None],
         "I_s": intensity(u[:Ns], v[:Ns]).astype(F32)[None], "R": R[None], "t": t[None],
         "R0": np.eye(3, dtype=F32)[None], "t0": np.zeros((1, 3), F32)}
    for a in c.values():
        a.setflags(write=False)
    return c


# ------------------------------------------------------------------------------------------------------------ the gradient

def gradient_system(x, nrm, inten, idx, radius=0.0):
    """x [3,N] fp32, nrm [3,N] fp32, inten [N] fp32, idx int [N,k] -> (S_aa [N,3,3], S_ab [N,3], m [N]) in the header's words:
    the entries outside [0, N), equal to the point or beyond the radius skipped, the sums in the row's order."""
    x, inten = np.asarray(x, F32), np.asarray(inten, F32)
    n = np.asarray(nrm, F32).astype(F64)
    N, k = idx.shape
    own = np.arange(N)
    Saa, Sab, m = np.zeros((N, 3, 3)), np.zeros((N, 3)), np.zeros(N, np.int64)
    r2 = F32(radius) * F32(radius)
    with np.errstate(invalid="ignore", over="ignore"):
        for j in range(k):
            r = np.asarray(idx[:, j], np.int64)
            ok = (r >= 0) & (r < N) & (r != own)
            rc = np.where(ok, r, own)
            f = x[:, rc] - x[:, own]                            # fp32
            if radius > 0:
                ok &= ~((f[0] * f[0] + f[1] * f[1]) + f[2] * f[2] > r2)
            d = f.astype(F64)
            dn = (d[0] * n[0] + d[1] * n[1]) + d[2] * n[2]
            a = d - dn * n
            di = inten[rc].astype(F64) - inten.astype(F64)
            Saa = Saa + np.where(ok, a[:, None, :] * a[None, :, :], 0.0).transpose(2, 0, 1)
            Sab = Sab + np.where(ok, a * di, 0.0).T
            m = m + ok
    return Saa, Sab, m


def _singular3(M):
    L = np.zeros((3, 3))
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        for j in range(3):
            s = M[j, j] - (L[j, :j] ** 2).sum()
            if not (np.isfinite(s) and s > PIVOT * M[j, j]):
                return True
            L[j, j] = np.sqrt(s)
            for i in range(j + 1, 3):
                L[i, j] = (M[i, j] - (L[i, :j] * L[j, :j]).sum()) / L[j, j]
    return False


def gradient(x, nrm, inten, idx, radius=0.0, want_cond=False):
    """-> the gradient fp32 [3,N]; with want_cond also (x float64 [3,N], cond(M) [N], m [N]) (cond = inf where the result is
    the exact zero)."""
    Saa, Sab, m = gradient_system(x, nrm, inten, idx, radius)
    n = np.asarray(nrm, F32).astype(F64)
    N = n.shape[1]
    out, cond = np.zeros((3, N)), np.full(N, np.inf)
    for i in range(N):
        if m[i] < 3 or not (np.isfinite(Saa[i]).all() and np.isfinite(Sab[i]).all()):
            continue
        mm = F64(m[i]) * F64(m[i])
        M = Saa[i] + mm * (n[:, i][:, None] * n[:, i][None, :])
        if _singular3(M):
            continue
        out[:, i] = np.linalg.solve(M, Sab[i])
        cond[i] = np.linalg.cond(M)
    g = out.astype(F32)
    return (g, out, cond, m) if want_cond else g


def neighbours(x, k=K):
    """x [3,N] fp32 -> int64 [N,k]: the k nearest OTHER points in float64 (a CPU stand-in for the library's searches)."""
    return pr.knn_f64(x, k + 1)[:, 1:]


# ------------------------------------------------------------------------------------------------- the fit, the header's order

def weights(lam):
    lam = F64(F32(lam))
    return np.sqrt(lam), np.sqrt(F64(1.0) - lam)


def _cross(p, h):
    return [p[1] * h[2] - p[2] * h[1], p[2] * h[0] - p[0] * h[2], p[0] * h[1] - p[1] * h[0]]


def colored_terms(p, q, m, d, It, Is, inl, lam=LAMBDA):
    """The inputs of the lanes (anything where inl is False) -> (J_G [6,n], r_G [n], J_I [6,n], r_I [n]) in float64: a lane that
    is no inlier has zero inputs, and so zero terms."""
    z = lambda a: np.where(inl, np.asarray(a, F32), F32(0)).astype(F64)   # noqa: E731
    p, q, m, d, It, Is = z(p), z(q), z(m), z(d), z(It), z(Is)
    wg, wi = weights(lam)
    with np.errstate(invalid="ignore", over="ignore"):
        s = ((p[0] * m[0] + p[1] * m[1]) + p[2] * m[2]) - ((q[0] * m[0] + q[1] * m[1]) + q[2] * m[2])
        dn = (d[0] * m[0] + d[1] * m[1]) + d[2] * m[2]
        h = [d[c] - dn * m[c] for c in range(3)]
        e = [(p[c] - s * m[c]) - q[c] for c in range(3)]
        rG = wg * s
        rI = wi * ((It + ((d[0] * e[0] + d[1] * e[1]) + d[2] * e[2])) - Is)
        JG = np.stack([wg * v for v in _cross(p, m) + [m[0], m[1], m[2]]])
        JI = np.stack([wi * v for v in _cross(p, h) + h])
    return JG, rG, JI, rI


def colored_sums(p, q, m, d, It, Is, inl, lam=LAMBDA):
    """-> (count, A [6,6], g [6]) in float64, every sum in the kernels' order."""
    JG, rG, JI, rI = colored_terms(p, q, m, d, It, Is, inl, lam)
    A = np.zeros((6, 6))
    with np.errstate(invalid="ignore", over="ignore"):
        for r in range(6):
            for c in range(r, 6):
                A[r, c] = A[c, r] = rr.ordered_sum(JG[r] * JG[c] + JI[r] * JI[c])
        g = np.asarray([rr.ordered_sum(JG[r] * rG + JI[r] * rI) for r in range(6)])
    return int(np.asarray(inl).sum()), A, g


def _lanes(c, R32, t32, nn_idx, nn_d2, max_dist):
    """c: one cloud's dict (src, tgt, nrm_t, grad, I_t, I_s) -> the lanes' inputs and the inlier mask."""
    limit = F32(max_dist) * F32(max_dist)
    nn_idx = np.asarray(nn_idx)
    with np.errstate(invalid="ignore"):
        inl = (nn_idx >= 0) & (np.asarray(nn_d2, F32) <= limit)
    at = np.maximum(nn_idx, 0)
    return (nr.moved(c["src"], R32, t32), np.asarray(c["tgt"], F32)[:, at], np.asarray(c["nrm_t"], F32)[:, at],
            np.asarray(c["grad"], F32)[:, at], np.asarray(c["I_t"], F32)[at], np.asarray(c["I_s"], F32), inl)


def colored_step(c, R32, t32, nn_idx, nn_d2, max_dist, lam=LAMBDA):
    """One update from given neighbours -> dict(R, t: the update in fp64; x, A, g, n, cond); None with fewer than six inliers or
    a singular system; R, t and x NaN where a sum is not finite."""
    n, A, g = colored_sums(*_lanes(c, R32, t32, nn_idx, nn_d2, max_dist), lam)
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


def colored_icp(c, R0=None, t0=None, max_dist=MAX_DIST, max_iterations=30, rel_fitness=1e-6, rel_rmse=1e-6, lam=LAMBDA):
    """refine_restated.icp's loop with colored_step for ONE cloud c (src, tgt, nrm_t, grad [3,.] fp32, I_t, I_s)."""
    src, tgt = c["src"], c["tgt"]
    R = np.eye(3) if R0 is None else np.asarray(R0, F32).astype(F64)
    t = np.zeros(3) if t0 is None else np.asarray(t0, F32).astype(F64)
    ev = rr.evaluate(src, tgt, R.astype(F32), t.astype(F32), max_dist)
    iterations, converged = 0, 0
    for _ in range(max_iterations):
        up = colored_step(c, R.astype(F32), t.astype(F32), ev["nn_idx"], ev["nn_d2"], max_dist, lam)
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


def cloud(c, b, grad=None):
    """Cloud b of a batch as colored_step takes it; grad [3,Nt] fp32: the gradients in use (None: the analytic ones)."""
    g = c["grad_t"][b].astype(F32) if grad is None else np.asarray(grad, F32)
    return {"src": c["src"][b], "tgt": c["tgt"][b], "nrm_t": c["nrm_t"][b], "grad": g, "I_t": c["I_t"][b], "I_s": c["I_s"][b]}


# ----------------------------------------------------------------------------------------------------------- 2: independently

def residuals(x6, p, q, m, d, It, Is, lam=LAMBDA):
    """(r_G [n], r_I [n]) of the inlier lanes after the source points p moved by x6 = (rotation about x, y, z; translation):
    p' = Rz Ry Rx p + t, the geometric residual (p' - q) . n and the photometric one read at p' projected onto the neighbour's
    tangent plane -- from the definition, not from the header's Md."""
    R, t = pr.update(np.asarray(x6, F64))
    p, q, m, d = (np.asarray(a, F64) for a in (p, q, m, d))
    pp = R @ p + t[:, None]
    wg, wi = weights(lam)
    s = ((pp - q) * m).sum(0)
    foot = pp - s * m                                          # p' on the tangent plane of q
    return wg * s, wi * (np.asarray(It, F64) + (d * (foot - q)).sum(0) - np.asarray(Is, F64))


def independent_x(p, q, m, d, It, Is, inl, lam=LAMBDA):
    """The same inputs as colored_sums -> x [6], the minimiser of sum (r_G + J_G . x)^2 + (r_I + J_I . x)^2 over the inliers by
    numpy.linalg.lstsq on the stacked rows, the Jacobians taken by central differences of `residuals`."""
    at = np.flatnonzero(inl)
    a = [np.asarray(v, F64)[..., at] for v in (p, q, m, d, It, Is)]
    r0 = np.concatenate(residuals(np.zeros(6), *a, lam))
    J = np.zeros((r0.size, 6))
    h = 1e-6
    for k in range(6):
        e = np.zeros(6)
        e[k] = h
        J[:, k] = (np.concatenate(residuals(e, *a, lam)) - np.concatenate(residuals(-e, *a, lam))) / (2 * h)
    return np.linalg.lstsq(J, -r0, rcond=None)[0]
