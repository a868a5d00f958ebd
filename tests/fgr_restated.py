"""CPU restatement of include/vcr_hip_fgr.h in numpy -- what the tests compare the kernels with.

  * `fma64`: an EXACT fp64 fma, vectorised (Boldo and Melquiond's emulation: the product split exactly by Dekker's algorithm,
    TwoSum, one addition rounded to odd, one to nearest); tests/test_fgr_cpu.py holds it to a fractions.Fraction fma.  Values
    stay far from fp64's overflow and underflow thresholds here.
  * `wg_sum`: the header's `sum order` -- 256 lanes, each its items in ascending order, the wave butterfly, the waves ascending.
  * `tuples`: the tuple test and the ordered cut on match_restated's draws and edge lengths (integer and fp32: the device's
    bits); `normalise`, `values`, `sums`: fp64 arithmetic in the device's order (its bits too, division and square root being
    correctly rounded on both sides); `solve6` / `euler` restate the Cholesky solve and TransformVector6dToMatrix4d -- numpy's
    sin and cos are not the device's, so from the first update on a pose is held within an allowance, not to its bits.
  * `fgr` strings them together; `nudge` (a test's hook) perturbs every Ri before it is applied."""
import numpy as np

import match_restated as mr

F32 = np.float32
MIN_ENTRIES = 10
PIVOT = 1e-12
NZ = (0, 1, 2, 4, 5, 6, 7, 8, 10, 11, 12, 13, 15, 18, 20, 21, 22, 23, 24, 25, 26)   # the 27 values without the structural zeros


# ------------------------------------------------------------------------------------------------------------------ arithmetic

def _two_sum(a, b):
    s = a + b
    bb = s - a
    return s, (a - (s - bb)) + (b - bb)


def _two_prod(a, b):
    p = a * b
    ca, cb = 134217729.0 * a, 134217729.0 * b
    ah = ca - (ca - a)
    bh = cb - (cb - b)
    al, bl = a - ah, b - bh
    return p, ((ah * bh - p) + ah * bl + al * bh) + al * bl


def fma64(a, b, c):
    """round64(a * b + c) with ONE rounding, elementwise on float64 arrays (finite values, no overflow or underflow)."""
    a, b, c = np.broadcast_arrays(*(np.asarray(v, np.float64) for v in (a, b, c)))
    uh, ul = _two_prod(a, b)
    th, tl = _two_sum(c, uh)
    v, e = _two_sum(tl, ul)                                   # v = RO(tl + ul): where inexact, the neighbour with an odd mantissa
    v = np.atleast_1d(v).copy()
    e = np.atleast_1d(e)
    even = (v.view(np.uint64) & np.uint64(1)) == np.uint64(0)
    fix = (e != 0) & even
    v = np.where(fix, np.nextafter(v, np.where(e > 0, np.inf, -np.inf)), v)
    return (np.atleast_1d(th) + v).reshape(np.shape(th))[()]


def wg_sum(x):
    """x [n, ...] float64 -> [...]: the header's sum order over the first axis."""
    x = np.asarray(x, np.float64)
    n = x.shape[0]
    rows = -(-n // 256) if n else 0
    pad = np.zeros((rows * 256,) + x.shape[1:])
    pad[:n] = x
    acc = np.zeros((256,) + x.shape[1:])
    for r in range(rows):
        acc = acc + pad[256 * r:256 * (r + 1)]
    lane = np.arange(64)
    w = acc.reshape((4, 64) + x.shape[1:])
    for o in (32, 16, 8, 4, 2, 1):
        w = w + w[:, lane ^ o]
    return ((w[0, 0] + w[1, 0]) + w[2, 0]) + w[3, 0]


# ------------------------------------------------------------------------------------------------------------------ the tuples

def passes(P, Q, at, tuple_scale):
    """P, Q [M, 3] fp32 (the pairs' source points and partners), at int [n, 3] -> bool [n]: s2 ls2 < lt2 && s2 lt2 < ls2 on the
    three edges (fp32, strict)."""
    s2 = F32(tuple_scale) * F32(tuple_scale)
    ok = np.ones(at.shape[0], bool)
    with np.errstate(invalid="ignore", over="ignore"):
        for u, v in ((0, 1), (0, 2), (1, 2)):
            ls2, lt2 = mr.len2(P[at[:, u]], P[at[:, v]]), mr.len2(Q[at[:, u]], Q[at[:, v]])
            ok &= (s2 * ls2 < lt2) & (s2 * lt2 < ls2)
    return ok


def ordered_cut(ok, K):
    """bool [n] -> the first K set positions, ascending (the device: block counts, their exclusive scan, ranks)."""
    return np.nonzero(ok)[0][:K]


def tuples(src, tgt, corr, tuple_scale, T, K, seed):
    """-> (M, tuples, list int64 [L]): the list optimised, source indices."""
    pl = mr.pair_list(corr, tgt.shape[1])
    M = len(pl)
    if tuple_scale == 0:
        return M, 0, pl
    n = min(T, 100 * M)
    if n == 0:
        return M, 0, np.zeros(0, np.int64)
    P, Q = np.ascontiguousarray(src[:, pl].T), np.ascontiguousarray(tgt[:, np.asarray(corr, np.int64)[pl]].T)
    at = mr.picks(seed, n, M)
    kept = ordered_cut(passes(P, Q, at, tuple_scale), K)
    return M, len(kept), pl[at[kept]].reshape(-1)


# ------------------------------------------------------------------------------------------------------------ the optimisation

def normalise(src, tgt):
    """src [3,Ns], tgt [3,Nt] fp32 -> (mean_s [3], mean_t [3], scale), float64."""
    with np.errstate(invalid="ignore", over="ignore"):
        ms = wg_sum(src.T.astype(np.float64)) / float(src.shape[1])
        mt = wg_sum(tgt.T.astype(np.float64)) / float(tgt.shape[1])
        big = 0.0
        for x, m in ((src, ms), (tgt, mt)):
            d = x.T.astype(np.float64) - m
            if np.isfinite(d).all():
                n2 = fma64(d[:, 2], d[:, 2], fma64(d[:, 1], d[:, 1], d[:, 0] * d[:, 0]))
                big = max(big, float(n2.max()))
            else:
                big = np.nan
        return ms, mt, float(np.sqrt(big))


def values(p, q, mu):
    """p, q [L, 3] float64 -> [L, 27]: the header's values."""
    r = p - q
    rx, ry, rz = r.T
    qx, qy, qz = q.T
    d2 = fma64(rz, rz, fma64(ry, ry, rx * rx))
    w = mu / (d2 + mu)
    s = w * w
    v = np.zeros((p.shape[0], 27))
    v[:, 0] = s * (qz * qz + qy * qy)
    v[:, 1] = s * -(qy * qx)
    v[:, 2] = s * -(qz * qx)
    v[:, 4] = s * -qz
    v[:, 5] = s * qy
    v[:, 6] = s * (qz * qz + qx * qx)
    v[:, 7] = s * -(qz * qy)
    v[:, 8] = s * qz
    v[:, 10] = s * -qx
    v[:, 11] = s * (qy * qy + qx * qx)
    v[:, 12] = s * -qy
    v[:, 13] = s * qx
    v[:, 15] = s
    v[:, 18] = s
    v[:, 20] = s
    v[:, 21] = s * (qz * ry + -(qy * rz))
    v[:, 22] = s * (-(qz * rx) + qx * rz)
    v[:, 23] = s * (qy * rx + -(qx * ry))
    v[:, 24] = s * -rx
    v[:, 25] = s * -ry
    v[:, 26] = s * -rz
    return v


def solve6(a21, g):
    """A x = -g by the library's Cholesky, in its order -> (x [6], ok)."""
    A = np.zeros((6, 6))
    e = 0
    for r in range(6):
        for c in range(r, 6):
            A[r, c] = A[c, r] = a21[e]
            e += 1
    Lm = np.zeros((6, 6))
    ok = True
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        for j in range(6):
            s = A[j, j]
            for k in range(j):
                s -= Lm[j, k] * Lm[j, k]
            ok = ok and bool(np.isfinite(s)) and s > PIVOT * A[j, j]
            d = np.sqrt(s)
            Lm[j, j] = d
            for i in range(j + 1, 6):
                v = A[i, j]
                for k in range(j):
                    v -= Lm[i, k] * Lm[j, k]
                Lm[i, j] = v / d
        y, x = np.zeros(6), np.zeros(6)
        for i in range(6):
            v = -g[i]
            for k in range(i):
                v -= Lm[i, k] * y[k]
            y[i] = v / Lm[i, i]
        for i in range(5, -1, -1):
            v = y[i]
            for k in range(i + 1, 6):
                v -= Lm[k, i] * x[k]
            x[i] = v / Lm[i, i]
    return x, ok and bool(np.isfinite(x).all())


def euler(x):
    """Ri = Rz(x2) Ry(x1) Rx(x0), ti = x[3:] in the library's expressions."""
    s0, c0, s1, c1, s2, c2 = np.sin(x[0]), np.cos(x[0]), np.sin(x[1]), np.cos(x[1]), np.sin(x[2]), np.cos(x[2])
    Ri = np.asarray([[c2 * c1, (c2 * s1) * s0 - s2 * c0, (c2 * s1) * c0 + s2 * s0],
                     [s2 * c1, (s2 * s1) * s0 + c2 * c0, (s2 * s1) * c0 - c2 * s0],
                     [-s1, c1 * s0, c1 * c0]])
    return Ri, np.asarray(x[3:6], np.float64)


def moved(Ri, v):
    """m(v): v [..., 3] -> fma(Ri[r][2], v2, fma(Ri[r][1], v1, Ri[r][0] v0)) per row r."""
    return np.stack([fma64(Ri[r, 2], v[..., 2], fma64(Ri[r, 1], v[..., 1], Ri[r, 0] * v[..., 0])) for r in range(3)], -1)


def fgr(src, tgt, corr, tuple_scale=0.95, T=None, K=1000, seed=0, iterations=64, division_factor=1.4, mu_floor=0.025,
        decrease_mu=True, nudge=None):
    """One cloud pair: src [3,Ns], tgt [3,Nt] fp32, corr int [Ns] -> dict(pairs, tuples, used, status, list, norm [7], pose64 [12],
    R, t (fp32), sums [27], mu).  nudge(it, Ri) -> Ri: applied to every update's rotation (a test's perturbation)."""
    src, tgt = np.asarray(src, F32), np.asarray(tgt, F32)
    T = min(100 * src.shape[1], 1 << 20) if T is None else T
    M, ntup, lst = tuples(src, tgt, corr, tuple_scale, T, K, seed)
    L = len(lst)
    ms, mt, scale = normalise(src, tgt)
    out = {"pairs": M, "tuples": ntup, "used": L, "list": lst, "norm": np.concatenate([ms, mt, [scale]]), "sums": np.zeros(27),
           "mu": 1.0, "status": 0}
    R, t = np.eye(3), np.zeros(3)

    def close(pose64):
        with np.errstate(invalid="ignore", over="ignore"):
            out.update(pose64=pose64, R=pose64[:9].astype(F32).reshape(3, 3), t=pose64[9:].astype(F32))
        return out
    if L < MIN_ENTRIES:
        out["status"] = 1
        return close(np.concatenate([R.reshape(9), t]))
    if not (np.isfinite(ms).all() and np.isfinite(mt).all() and np.isfinite(scale) and scale != 0):
        out["status"] = 2
        return close(np.full(12, np.nan))
    j = np.asarray(corr, np.int64)[lst]
    q = (src[:, lst].T.astype(np.float64) - ms) / scale
    p = (tgt[:, j].T.astype(np.float64) - mt) / scale
    mu = 1.0
    for it in range(iterations):
        S = wg_sum(values(p, q, mu))
        out["sums"] = S
        x, ok = solve6(S[:21], S[21:])
        if not ok:
            out["status"] |= 16
        else:
            Ri, ti = euler(x)
            if nudge is not None:
                Ri = nudge(it, Ri)
            R = moved(Ri, R.T).T
            t = moved(Ri, t) + ti
            q = moved(Ri, q) + ti
        if decrease_mu and it % 4 == 0 and mu > mu_floor:
            mu = mu / division_factor
    out["mu"] = mu
    return close(np.concatenate([R.reshape(9), (scale * t + mt) - moved(R, ms)]))


def rotation_error_deg(R, want):
    c = (np.trace(np.asarray(R, np.float64).T @ want) - 1) / 2
    return float(np.degrees(np.arccos(np.clip(c, -1, 1))))
