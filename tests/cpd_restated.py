"""include/cpd/vcr_hip_cpd.h restated in numpy, from the paper's equations (Myronenko & Song 2010, figure 2 for the rigid case) and
the header: the moved source, the pair weights, the sum hierarchy of the two streamed passes (``hier_sum``), the refinements'
block order (``block_sum``), the M-step, the loop with its stops, and the recipes the CPU and GPU tests share.  The ONE value the
header leaves open is exp2: ``expectation`` takes numpy's, or the weights it is given (the device's e_stage).

One cloud is a float32 array [3, n]; src = Y moves, tgt = X is fixed."""
import math

import numpy as np

import grid_restated as gr
import ndt_restated as nd

F32 = np.float32
TILE, SEGMENT = 256, 4096
LOG2E = 1.4426950408889634
TWO_PI = 6.283185307179586
STATUS = ("converged", "max iterations", "collapsed", "no mass", "not finite")
same_bits = nd.same_bits
torus, pose, pose_error = nd.torus, nd.pose, nd.pose_error


def moved(src, R=None, t=None, s=1.0):
    """ty [3, M] fp32: r' = (float)(s R), t' = (float)t, fmaf(r'[3c+2], z, fmaf(r'[3c+1], y, r'[3c] * x)) + t'[c]."""
    R = np.eye(3) if R is None else np.asarray(R, np.float64)
    t = np.zeros(3) if t is None else np.asarray(t, np.float64)
    r = (float(s) * R).astype(F32)
    tt = t.astype(F32)
    x, y, z = (np.asarray(src[c], F32) for c in range(3))
    with np.errstate(all="ignore"):
        return np.stack([(gr.fmaf32(r[c, 2], z, gr.fmaf32(r[c, 1], y, (r[c, 0] * x).astype(F32))) + tt[c]).astype(F32) for c in range(3)])


def k_of(sigma2):
    return F32(-LOG2E / (2.0 * float(sigma2)))


def exponent(ty, x, sigma2):
    """d2 * k, fp32 [M, N]: d_c = x_c(n) - ty_c(m), d2 = (d_0 d_0 + d_1 d_1) + d_2 d_2."""
    with np.errstate(all="ignore"):
        d = [(x[c][None, :] - ty[c][:, None]).astype(F32) for c in range(3)]
        d2 = ((d[0] * d[0] + d[1] * d[1]).astype(F32) + d[2] * d[2]).astype(F32)
        return (d2 * k_of(sigma2)).astype(F32)


def weights(ty, x, sigma2):
    """e [M, N] fp32 with numpy's exp2 (results under 2^-126 flushed, as the hardware's are); zero rows and columns for
    non-finite points."""
    with np.errstate(all="ignore"):
        e = np.exp2(exponent(ty, x, sigma2)).astype(F32)
    e[e < F32(2.0 ** -126)] = 0
    return mask(e, ty, x)


def mask(e, ty, x):
    e = np.array(e, F32)
    e[~np.isfinite(ty).all(0), :] = 0
    e[:, ~np.isfinite(x).all(0)] = 0
    return e


def hier_sum(terms):
    """terms fp32 [K, L], streamed along K -> fp64 [L]: tiles of 256 as fp32 chains, segments of 4096 as fp64 sums of their
    tiles ascending from +0, the total as the fp64 sum of the segments ascending from +0."""
    K, L = terms.shape
    ntile = -(-K // TILE)
    pad = np.zeros((ntile * TILE, L), F32)
    pad[:K] = terms
    with np.errstate(all="ignore"):
        tiles = np.cumsum(pad.reshape(ntile, TILE, L), axis=1, dtype=F32)[:, -1, :].astype(np.float64)    # (a sequential chain)
        total = np.zeros(L)
        for s0 in range(0, ntile, SEGMENT // TILE):
            seg = np.zeros(L)
            for i in range(s0, min(s0 + SEGMENT // TILE, ntile)):
                seg = seg + tiles[i]
            total = total + seg
    return total


def block_sum(vals):
    """vals [..., count] fp64 -> [...]: per 256 points the butterfly 32 ... 1, the four waves ascending, the partials ascending
    from +0 -- the refinements' order."""
    vals = np.asarray(vals, np.float64)
    lead, count = vals.shape[:-1], vals.shape[-1]
    nblk = -(-count // 256)
    pad = np.zeros(lead + (nblk * 256,))
    pad[..., :count] = vals
    v = pad.reshape(lead + (nblk, 4, 64))
    lane = np.arange(64)
    with np.errstate(all="ignore"):
        for o in (32, 16, 8, 4, 2, 1):
            v = v + v[..., lane ^ o]
        w = v[..., 0]
        part = ((w[..., 0] + w[..., 1]) + w[..., 2]) + w[..., 3]
        tot = np.zeros(lead)
        for i in range(nblk):
            tot = tot + part[..., i]
    return tot


def outlier_constant(sigma2, w, M, N):
    q = TWO_PI * float(sigma2)
    return ((q * math.sqrt(q)) * (w / (1.0 - w))) * (float(M) / float(N))


def expectation(src, tgt, sigma2, R=None, t=None, s=1.0, w=0.0, e=None):
    """-> dict: Pt1 [N], P1 [M], PX [3, M], Np, e [M, N], and the sums of the absolute terms behind PX (absPX [3, M])."""
    x = np.asarray(tgt, F32)
    M, N = src.shape[1], x.shape[1]
    ty = moved(src, R, t, s)
    e = weights(ty, x, sigma2) if e is None else mask(e, ty, x)
    S = hier_sum(e)                                          # pass 1 streams m
    c = outlier_constant(sigma2, w, M, N)
    with np.errstate(all="ignore"):
        den = S + c
        rden = 1.0 / den
        live = den != 0.0
        inv = np.where(live, rden, 0.0).astype(F32)
        Pt1 = np.where(live, S * rden, 0.0)
        p = (e * inv[None, :]).astype(F32)
        xz = np.where(np.isfinite(x).all(0)[None, :], x, F32(0))
        P1 = hier_sum(p.T.copy())                            # pass 2 streams n
        prod = [(p * xz[c_][None, :]).astype(F32) for c_ in range(3)]
        PX = np.stack([hier_sum(q.T.copy()) for q in prod])
        absPX = np.stack([np.abs(q).astype(np.float64).sum(1) for q in prod])
    return {"Pt1": Pt1, "P1": P1, "PX": PX, "Np": float(block_sum(P1)), "e": e, "absPX": absPX}


def mstep(src, tgt, Pt1, P1, PX, with_scaling=False):
    """The header's M-step in its order of operations (the rotation by numpy's SVD: the Jacobi's differs in rounding only).
    -> None for Np == 0, else dict: finite, R, t, s, sigma2, Np."""
    y, x = np.asarray(src, np.float64), np.asarray(tgt, np.float64)
    with np.errstate(all="ignore"):
        first = block_sum(np.concatenate([P1[None], PX, P1[None] * y]))
        if not np.isfinite(first).all():
            return {"finite": False}
        Np = first[0]
        if Np == 0.0:
            return None
        mux, muy = first[1:4] / Np, first[4:7] / Np
        yh = y - muy[:, None]
        a = PX - P1[None] * mux[:, None]
        A = block_sum(a[:, None, :] * yh[None, :, :])        # [3, 3]
        yPy = block_sum(P1 * ((yh[0] * yh[0] + yh[1] * yh[1]) + yh[2] * yh[2]))
        xh = x - mux[:, None]
        xPx = block_sum(Pt1 * ((xh[0] * xh[0] + xh[1] * xh[1]) + xh[2] * xh[2]))
        if not (np.isfinite(A).all() and np.isfinite(yPy) and np.isfinite(xPx)):
            return {"finite": False}
        U, _, Vt = np.linalg.svd(A)
        Cm = np.diag([1.0, 1.0, np.linalg.det(U @ Vt)])
        R = U @ Cm @ Vt
        trAR = float((A * R).sum())
        s = trAR / yPy if with_scaling else 1.0
        t = mux - s * (R @ muy)
        sigma2 = ((xPx - (2.0 * s) * trAR) + (s * s) * yPy) / (3.0 * Np)
    ok = bool(np.isfinite(R).all() and np.isfinite(t).all() and np.isfinite(s) and np.isfinite(sigma2))
    return {"finite": ok, "R": R, "t": t, "s": float(s), "sigma2": float(sigma2), "Np": float(Np)}


def sigma2_start(src, tgt, R=None, t=None):
    """sum_n sum_m |x_n - T(y_m)|^2 / (3 M N) about the two means, in block order."""
    x = np.asarray(tgt, np.float64)
    ty = moved(src, R, t).astype(np.float64)
    M, N = ty.shape[1], x.shape[1]
    with np.errstate(all="ignore"):
        cx, cy = block_sum(x) / float(N), block_sum(ty) / float(M)
        dx, dy = x - cx[:, None], ty - cy[:, None]
        sxx = block_sum((dx[0] * dx[0] + dx[1] * dx[1]) + dx[2] * dx[2])
        syy = block_sum((dy[0] * dy[0] + dy[1] * dy[1]) + dy[2] * dy[2])
        d = cx - cy
        return float(((M * sxx + N * syy) + (float(M) * N) * ((d[0] * d[0] + d[1] * d[1]) + d[2] * d[2])) / ((3.0 * M) * N))


def cpd(src, tgt, R=None, t=None, w=0.1, max_iterations=50, tolerance=1e-4, with_scaling=False, sigma2=None, sigma2_floor=None):
    """The loop of the header.  -> dict: R, t (float32), scale, sigma2, Np, iterations, status, trace [max_iterations + 1], Pt1, P1,
    PX (the closing E-step's)."""
    R = np.eye(3) if R is None else np.asarray(R, F32).astype(np.float64)
    t = np.zeros(3) if t is None else np.asarray(t, F32).astype(np.float64)
    s = 1.0
    s2 = sigma2_start(src, tgt, R, t) if sigma2 is None else float(sigma2)
    trace = np.full(max_iterations + 1, np.nan)
    trace[0] = s2
    out = lambda status, it, E: dict(R=R.astype(F32), t=t.astype(F32), scale=s, sigma2=s2, Np=E["Np"], iterations=it, status=status,  # noqa: E731
                                     trace=trace, Pt1=E["Pt1"], P1=E["P1"], PX=E["PX"])
    if not (math.isfinite(s2) and s2 > 0.0):
        nanE = {"Np": np.nan, "Pt1": np.full(tgt.shape[1], np.nan), "P1": np.full(src.shape[1], np.nan), "PX": np.full((3, src.shape[1]), np.nan)}
        return out(4, 0, nanE)
    floor = 1e-8 * s2 if sigma2_floor is None else float(sigma2_floor)
    it = 0
    while True:
        E = expectation(src, tgt, s2, R, t, s, w)
        if it >= max_iterations:
            return out(1, it, E)
        m = mstep(src, tgt, E["Pt1"], E["P1"], E["PX"], with_scaling)
        if m is None:
            return out(3, it, E)
        if not m["finite"]:
            return out(4, it, E)
        R, t, s = m["R"].astype(F32).astype(np.float64), m["t"].astype(F32).astype(np.float64), m["s"]
        it += 1
        old = s2
        status = None
        if not m["sigma2"] > floor:
            s2, status = floor, 2
        else:
            s2 = m["sigma2"]
            if abs(s2 - old) <= tolerance * old:
                status = 0
            elif it >= max_iterations:
                status = 1
        trace[it] = s2
        if status is not None:
            return out(status, it, expectation(src, tgt, s2, R, t, s, w))


# ---- the recipes the CPU and GPU tests share ----

ANGLES, SEEDS, SHIFT = (0.8, 1.2), (0, 1, 3), 0.3


def recipe(angle, shift, seed):
    """The ledger's torus: torus(11, 700) as target, torus(12, 500) moved by the INVERSE of pose(angle, shift, seed) as source.
    -> (src [3,500], tgt [3,700] fp32, Rg, tg: the truth src -> tgt)."""
    tgt = torus(11, 700)
    Rg, tg = pose(angle, shift, seed=seed)
    s = torus(12, 500).astype(np.float64)
    return (Rg.T @ (s - tg[:, None])).astype(F32), tgt, Rg, tg


def exact_copy(seed=0):
    """500 of the 700 target points moved by the inverse of (0.8 rad, 0.3)."""
    tgt = torus(11, 700)
    Rg, tg = pose(0.8, 0.3, seed=seed)
    pick = np.random.RandomState(77 + seed).permutation(700)[:500]
    return (Rg.T @ (tgt[:, pick].astype(np.float64) - tg[:, None])).astype(F32), tgt, Rg, tg


def shrunk(seed=0, factor=1.3):
    """The recipe's source about its own mean shrunk by `factor` (the truth's scale is `factor`), from (0.2 rad, 0.1)."""
    src, tgt, Rg, tg = recipe(0.2, 0.1, seed)
    c = src.astype(np.float64).mean(1, keepdims=True)
    return ((src.astype(np.float64) - c) / factor + c).astype(F32), tgt, Rg, tg


# ---- what the GPU tests and profiles/bench_cpd.py share ----

# (M, N) across the tile's edges: every size of (1, 63, 64, 65, 255, 256, 257, 1000) on both sides
TILE_SHAPES = ((1, 1), (1, 257), (63, 1000), (64, 257), (65, 256), (255, 65), (256, 64), (257, 63), (1000, 255), (256, 1), (1000, 1000))
SEGMENT_SHAPES = ((4095, 300), (4096, 300), (4097, 300), (300, 4096), (300, 4097), (300, 8200))


def clouds(M, N, seed):
    """Three pairs of noisy torus samplings with a pose, a scale and a variance each."""
    src = np.stack([torus(seed + b, M, noise=0.02) for b in range(3)])
    tgt = np.stack([torus(seed + 10 + b, N, noise=0.02) for b in range(3)])
    Rt = [pose(0.1 * (b + 1), 0.05 * b, seed + b) for b in range(3)]
    R = np.stack([p[0] for p in Rt]).astype(F32)
    t = np.stack([p[1] for p in Rt]).astype(F32)
    return src, tgt, R, t, np.array([1.0, 0.9, 1.25]), np.array([0.3, 0.02, 0.002])


def ratio(o, r, b):
    """|device - restated| in units of 2^-24 times the sum of the absolute terms, over Pt1, P1, PX and Np."""
    worst = 0.0
    for got, want, scale in ((o["Pt1"][b], r["Pt1"], r["Pt1"]), (o["P1"][b], r["P1"], r["P1"]), (o["PX"][b], r["PX"], r["absPX"]),
                             (o["Np"][b], r["Np"], r["Np"])):
        got, want, scale = np.atleast_1d(got), np.atleast_1d(want), np.atleast_1d(scale) * 2.0 ** -24
        with np.errstate(invalid="ignore", divide="ignore"):
            q = np.where(scale > 0, np.abs(got - want) / scale, np.where(got == want, 0.0, np.inf))
        worst = max(worst, float(q.max()))
    return worst


def exp2_ratio(o, src, tgt, R, t, scale, sigma2, w, b):
    """ratio() of the device outputs o for cloud b against the restatement with numpy's own exp2 wherever that is >= 2^-100 and
    the device's staged e (o["e"]) below: the pairs that are compared."""
    own = weights(moved(src[b], R[b], t[b], scale[b]), tgt[b], sigma2[b])
    mixed = np.where(own >= F32(2.0 ** -100), own, o["e"][b])
    return ratio(o, expectation(src[b], tgt[b], sigma2[b], R[b], t[b], scale[b], w, e=mixed), b)


def dense_cpd_round(Y, X, R, t, s, s2, w, with_scaling=False):
    """One EM round of rigid CPD in fp64, straight from the paper's figure 2: the independent restatement."""
    M, N = Y.shape[1], X.shape[1]
    T = s * (R @ Y) + t[:, None]
    P = np.exp(-((X[:, None, :] - T[:, :, None]) ** 2).sum(0) / (2 * s2))         # [M, N]
    P = P / (P.sum(0) + (2 * np.pi * s2) ** 1.5 * w / (1 - w) * M / N)
    Np, mux, muy = P.sum(), X @ P.sum(0) / P.sum(), Y @ P.sum(1) / P.sum()
    Xh, Yh = X - mux[:, None], Y - muy[:, None]
    A = Xh @ P.T @ Yh.T
    U, _, Vt = np.linalg.svd(A)
    R = U @ np.diag([1, 1, np.linalg.det(U @ Vt)]) @ Vt
    yPy, xPx = (P.sum(1) * (Yh ** 2).sum(0)).sum(), (P.sum(0) * (Xh ** 2).sum(0)).sum()
    s = np.trace(A.T @ R) / yPy if with_scaling else 1.0
    return R, mux - s * R @ muy, s, (xPx - 2 * s * np.trace(A.T @ R) + s * s * yPy) / (3 * Np)
