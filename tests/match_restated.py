"""CPU restatement of include/vcr_hip_match.h in numpy -- what the tests compare the kernels with --
and the input recipes the CPU and GPU tests share.

  * `fma32`: an EXACT fmaf.  The feature distance is a chain of 33 fmaf on arbitrary fp32 values, so nnscore_restated.fma32
    (which rounds twice and is good on exact lattices only) does not serve.  The product of two fp32 values is exact in
    float64; the sum is taken by TwoSum, and where its error term is not zero and the float64 sum sits exactly on an fp32
    rounding boundary (the low 29 bits of its mantissa are 0x10000000) the sum is stepped one float64 ulp towards the error
    before the rounding to fp32.  tests/test_match_cpu.py holds it to a fractions.Fraction fmaf.  (Results in fp32's normal
    range; the recipes stay there.)
  * the search: `d2_chain` is the chain, `nearest` / `nearest_rev` apply nnscore_restated._first_min's rule along either axis.
  * the RANSAC, with two entrances: `picks`, `early_status` (status 1 and 2) are pure integer and fp32 arithmetic and are the
    device's bit for bit; `solve3` is refine_restated.solve (numpy's SVD), so a pose is held to the device's by properties
    only; `check_and_count` runs the distance check and the count from GIVEN fp32 poses -- the device's own -- bit for bit
    again; `best` is the arg-max rule.  `ransac` strings them together on the CPU's own poses."""
import numpy as np

import nnscore_restated as nr
import refine_restated as rr

F32 = np.float32
U = 2.0 ** -24                                             # fp32 unit roundoff
C = 33


def fma32(a, b, c):
    """round32(a * b + c) with ONE rounding, elementwise on fp32 arrays."""
    a, b, c = (np.asarray(v, F32).astype(np.float64) for v in (a, b, c))
    with np.errstate(invalid="ignore", over="ignore"):
        p = a * b                                           # exact: 24 x 24 bits
        s0 = p + c
        bb = s0 - p                                         # TwoSum: s0 + err == p + c exactly
        err = np.atleast_1d((p - (s0 - bb)) + (c - bb))
        s = np.atleast_1d(s0).copy()
        halfway = (s.view(np.uint64) & np.uint64(0x1FFFFFFF)) == np.uint64(0x10000000)
        fix = halfway & np.isfinite(s) & np.isfinite(err) & (err != 0)
        s = np.where(fix, np.nextafter(s, np.where(err > 0, np.inf, -np.inf)), s)
        return s.astype(F32).reshape(np.shape(s0))[()]


# ------------------------------------------------------------------------------------------------------------------ the search

def d2_chain(a, b):
    """a [33, n], b [33, m] fp32 -> [n, m] fp32: d_c = a_c - b_c; acc = d_0 d_0; acc = fmaf(d_c, d_c, acc), c = 1 .. 32."""
    a, b = np.asarray(a, F32), np.asarray(b, F32)
    with np.errstate(invalid="ignore", over="ignore"):
        d = a[0][:, None] - b[0][None, :]
        acc = d * d
        for c in range(1, a.shape[0]):
            d = a[c][:, None] - b[c][None, :]
            acc = fma32(d, d, acc)
    return acc


def nearest(d2):
    """[n, m] -> (nn_idx int64 [n], nn_d2 fp32 [n]): per row the smallest finite value, the lowest index among equals."""
    idx, best = nr._first_min(d2)
    return idx, best.astype(F32)


def nearest_rev(d2):
    """The search with the roles exchanged: (a - b)^2 and (b - a)^2 are the same bits, so it is the matrix's columns."""
    return nearest(np.ascontiguousarray(d2.T))


def mutual(nn_idx, rev_idx):
    """nn_idx[i] = j is kept iff rev_idx[j] == i."""
    j = np.maximum(nn_idx, 0)
    return np.where((nn_idx >= 0) & (rev_idx[j] == np.arange(nn_idx.shape[0])), nn_idx, -1)


def d2_64(a, b, j):
    """float64 squared feature distance of column i of a to column j[i] of b."""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return ((a - b[:, j]) ** 2).sum(0)


def min_d2_64(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return np.asarray([((a[:, i:i + 1] - b) ** 2).sum(0).min() for i in range(a.shape[1])])


# The chosen neighbour against the float64 minimum.  A computed d2 is sum_c d_c^2 with, per term, the subtraction's rounding
# twice (it is squared) and at most 33 roundings of the chain behind it (one product, 32 fmaf; every term is >= 0, so the
# relative errors do not amplify): d2 (1 - u)^35 <= computed <= d2 (1 + u)^35.  The chosen j has computed(j) <= computed(j*),
# so d2(j) ((1 - u) / (1 + u))^35 <= d2(j*): 70 u to first order; two more for the second order and the float64 yardstick.
CHOICE_E = 72 * U


# ------------------------------------------------------------------------------------------------------------------ the RANSAC

def mix32(x):
    x = np.asarray(x, np.uint32).copy()
    with np.errstate(over="ignore"):
        x ^= x >> np.uint32(16); x *= np.uint32(0x7feb352d); x ^= x >> np.uint32(15); x *= np.uint32(0x846ca68b)
        x ^= x >> np.uint32(16)
    return x


def picks(seed, T, M):
    """-> int64 [T, 3]: the positions in the pair list, ((uint64)mix32(seed ^ mix32(3 t + j)) * M) >> 32."""
    n = (3 * np.arange(T, dtype=np.uint32)[:, None] + np.arange(3, dtype=np.uint32)[None, :]).astype(np.uint32)
    h = mix32(np.uint32(seed) ^ mix32(n)).astype(np.uint64)
    return ((h * np.uint64(M)) >> np.uint64(32)).astype(np.int64)


def pair_list(corr, Nt):
    """corr int [Ns] -> the source indices with a partner in [0, Nt), ascending."""
    corr = np.asarray(corr, np.int64)
    return np.nonzero((corr >= 0) & (corr < Nt))[0]


def len2(u, v):
    """u, v [..., 3] fp32 -> fmaf(dz, dz, fmaf(dy, dy, dx dx)) of the fp32 differences."""
    with np.errstate(invalid="ignore", over="ignore"):
        d = np.asarray(u, F32) - np.asarray(v, F32)
        return fma32(d[..., 2], d[..., 2], fma32(d[..., 1], d[..., 1], d[..., 0] * d[..., 0]))


def early_status(P, Q, at, similarity):
    """P, Q [M, 3] fp32 (the pairs' source points and partners), at int [T, 3] -> int [T]: 1 two picks equal, 2 an edge pair
    fails ds2 >= s2 dt2 && dt2 >= s2 ds2 (similarity != 0), else 0."""
    status = np.zeros(at.shape[0], np.int64)
    same = (at[:, 0] == at[:, 1]) | (at[:, 0] == at[:, 2]) | (at[:, 1] == at[:, 2])
    if similarity != 0:
        s2 = F32(similarity) * F32(similarity)
        ok = np.ones(at.shape[0], bool)
        with np.errstate(invalid="ignore", over="ignore"):
            for u, v in ((0, 1), (0, 2), (1, 2)):
                ds2, dt2 = len2(P[at[:, u]], P[at[:, v]]), len2(Q[at[:, u]], Q[at[:, v]])
                ok &= (ds2 >= s2 * dt2) & (dt2 >= s2 * ds2)
        status[~ok] = 2
    status[same] = 1
    return status


def solve3(p, q):
    """p, q [3, 3] fp32 (rows = the three picks) -> dict(R, t float64; H, opt, s1, pm, qm): vcr_refine_f32's step with n = 3."""
    p, q = np.asarray(p, F32).astype(np.float64), np.asarray(q, F32).astype(np.float64)
    Sp, Sq = (p[0] + p[1]) + p[2], (q[0] + q[1]) + q[2]
    Spq = (np.outer(p[0], q[0]) + np.outer(p[1], q[1])) + np.outer(p[2], q[2])
    third = 1.0 / 3.0
    H = Spq - np.outer(Sp, Sq) * third
    R, opt, s1 = rr.solve(H)
    pm, qm = Sp * third, Sq * third
    return {"R": R, "t": qm - R @ pm, "H": H, "opt": opt, "s1": s1, "pm": pm, "qm": qm}


def d2_under(pose, x, y):
    """pose [T, 12] fp32 (R row-major, then t), x, y [..., 3] fp32 broadcastable against T -> fp32 d2 of every (trial, pair):
    vcr_hip_score.h's `moved source` and `distance`."""
    pose = np.asarray(pose, F32)
    with np.errstate(invalid="ignore", over="ignore"):
        m = [fma32(pose[:, 3 * c + 2, None], x[..., 2], fma32(pose[:, 3 * c + 1, None], x[..., 1], pose[:, 3 * c, None] * x[..., 0]))
             + pose[:, 9 + c, None] for c in range(3)]
        dx, dy, dz = (m[c] - y[..., c] for c in range(3))
        return fma32(dz, dz, fma32(dy, dy, dx * dx))


def check_and_count(P, Q, at, pose, max_dist, chunk=256):
    """The second entrance: P, Q [M, 3] fp32, at int [T, 3], pose [T, 12] fp32 GIVEN (finite) -> (far bool [T]: one of the
    three picks has d2 > max_dist^2, i.e. status 4; count int [T]: the pairs with d2 <= max_dist^2)."""
    limit = F32(max_dist) * F32(max_dist)
    T = at.shape[0]
    far, count = np.zeros(T, bool), np.zeros(T, np.int64)
    with np.errstate(invalid="ignore"):
        for lo in range(0, T, chunk):
            sl = slice(lo, lo + chunk)
            far[sl] = (d2_under(pose[sl], P[at[sl]], Q[at[sl]]) > limit).any(1)
            count[sl] = (d2_under(pose[sl], P[None], Q[None]) <= limit).sum(1)
    return far, count


def best(count, valid):
    """-> (best_trial, inliers): the valid trial with the highest count, the lowest t among equals; (-1, 0) without one."""
    if not valid.any():
        return -1, 0
    c = np.where(valid, count, -1)
    t = int(np.argmax(c))                                   # (the first among equals)
    return t, int(c[t])


def ransac(src, tgt, corr, max_dist, similarity, T, seed):
    """One cloud on the CPU's own poses: src [3,Ns], tgt [3,Nt] fp32, corr int [Ns] -> dict(status, picks, pose, count,
    best_trial, inliers, pairs, R, t)."""
    src, tgt = np.asarray(src, F32), np.asarray(tgt, F32)
    pl = pair_list(corr, tgt.shape[1])
    M = len(pl)
    pose = np.zeros((T, 12), F32)
    count = np.full(T, -1, np.int64)
    if M < 1:
        return {"status": np.ones(T, np.int64), "picks": np.full((T, 3), -1), "pose": pose, "count": count, "best_trial": -1,
                "inliers": 0, "pairs": 0, "R": np.eye(3, dtype=F32), "t": np.zeros(3, F32)}
    P, Q = np.ascontiguousarray(src[:, pl].T), np.ascontiguousarray(tgt[:, np.asarray(corr, np.int64)[pl]].T)
    at = picks(seed, T, M)
    status = early_status(P, Q, at, similarity)
    live = np.nonzero(status == 0)[0]
    for t in live:
        s = solve3(P[at[t]], Q[at[t]])
        with np.errstate(invalid="ignore", over="ignore"):
            pose[t] = np.concatenate([s["R"].reshape(9), s["t"]]).astype(F32)
        if not np.isfinite(pose[t]).all():
            status[t] = 3
    live = np.nonzero(status == 0)[0]
    if len(live):
        far, cnt = check_and_count(P, Q, at[live], pose[live], max_dist)
        status[live[far]] = 4
        count[live[~far]] = cnt[~far]
    bt, inl = best(count, status == 0)
    Rt = pose[bt] if bt >= 0 else np.asarray([1, 0, 0, 0, 1, 0, 0, 0, 1, 0, 0, 0], F32)
    return {"status": status, "picks": pl[at], "pose": pose, "count": count, "best_trial": bt, "inliers": inl, "pairs": M,
            "R": Rt[:9].reshape(3, 3), "t": Rt[9:]}


# ----------------------------------------------------------------------------------------------------------------- the recipes

FEAT_SHAPES = ((1, 1, 1), (1, 5, 3), (2, 64, 65), (3, 257, 300), (2, 1000, 777))       # (B, Ns, Nt)
RANSAC_SHAPES = ((40, 0.5, 512), (257, 0.3, 2048), (1000, 0.2, 8192))                  # (M, planted share, T)
MAX_DIST, SIMILARITY, SEED = 0.05, 0.9, 7


def features(B, Ns, Nt, seed=0):
    """(a [B,33,Ns], b [B,33,Nt]) random fp32 in [0, 200]."""
    rs = np.random.RandomState(1000 + seed + 7 * Ns + 13 * Nt)
    return (rs.uniform(0, 200, (B, C, Ns)).astype(F32), rs.uniform(0, 200, (B, C, Nt)).astype(F32))


def planted(M, share, seed=0, extra=0):
    """One cloud of the RANSAC recipe -> dict: src [3, M + extra] fp32 uniform in the unit cube, tgt [3, M] fp32 -- partner i
    is A p_i + t rounded to fp32 for the first round(share M) pairs (then shuffled) and uniform in [-1, 2]^3 for the rest --,
    corr int32 [M + extra] (the `extra` source points at the end have none: -1), good bool [M + extra], R, t (float64)."""
    rs = np.random.RandomState(500 + seed + M)
    n_good = int(round(share * M))
    src = rs.uniform(0, 1, (3, M + extra)).astype(F32)
    A = rr.rotation(rs.normal(size=3), 65.0)
    t = rs.uniform(-0.5, 0.5, 3)
    good = np.zeros(M + extra, bool)
    good[rs.permutation(M)[:n_good]] = True
    partner = np.where(good[None, :M], A @ src[:, :M].astype(np.float64) + t[:, None], rs.uniform(-1, 2, (3, M))).astype(F32)
    perm = rs.permutation(M)                                # target column perm[i] holds source point i's partner
    tgt = np.empty((3, M), F32)
    tgt[:, perm] = partner
    corr = np.full(M + extra, -1, np.int32)
    corr[:M] = perm
    return {"src": src, "tgt": tgt, "corr": corr, "good": good, "R": A, "t": t}


def surface(N, seed=0):
    """The end-to-end recipe: a surface without symmetries over the unit square -> dict: tgt [3,N] fp32, src [3,N] fp32 = the
    target under a pose (rounded to fp32), permuted; twin int [N]: the target index of every source point; R, t (float64):
    the pose src -> tgt."""
    rs = np.random.RandomState(900 + seed + N)
    u, v = rs.uniform(0, 1, N), rs.uniform(0, 1, N)
    z = (0.15 * np.sin(7 * u) * np.cos(5 * v) + 0.25 * u * v + 0.1 * np.exp(-((u - .3) ** 2 + (v - .6) ** 2) / 0.01)
         - 0.08 * np.exp(-((u - .75) ** 2 + (v - .25) ** 2) / 0.004))
    tgt = np.stack([u, v, z]).astype(F32)
    A = rr.rotation(rs.normal(size=3), 50.0)
    s = rs.uniform(-0.5, 0.5, 3)
    perm = rs.permutation(N)                                # source column i is target point perm[i]
    src = (A @ tgt.astype(np.float64) + s[:, None]).astype(F32)[:, perm]
    return {"src": np.ascontiguousarray(src), "tgt": tgt, "twin": perm, "R": A.T, "t": -A.T @ s}


def surface_up(c):
    """The recipe's `towards the sensor` directions, (source, target): +z of the target frame, carried into the source's."""
    ez = np.asarray([0.0, 0.0, 1.0])
    return c["R"].T @ ez, ez


def orient(normals, up):
    """normals [3,N] -> the same with every sign chosen so that n . up >= 0."""
    n = np.asarray(normals, np.float64)
    return (n * np.where(up @ n < 0, -1.0, 1.0)).astype(F32)


# The share of correct pairs (corr == twin) among the matches of the surface recipe by the CPU chain -- fpfh_restated's
# neighbours (float64), normals and features, the float64 feature distance -- as surface_shares() below computes them
# (tests/test_match_cpu.py holds the table to it): (N, k, oriented normals, mutual) -> share.  An estimated normal's sign is
# arbitrary and differs between a surface and its rotated copy; the feature changes with it.
SURFACE_SHARES = {(600, 20, False, False): 0.183, (600, 20, False, True): 0.542, (600, 20, True, False): 0.997,
                  (600, 20, True, True): 0.998, (1500, 30, False, False): 0.753, (1500, 30, False, True): 0.981,
                  (1500, 30, True, False): 1.0, (1500, 30, True, True): 1.0}
SHARE_SLACK = 0.05                                         # "a few points": the device's kNN and normals are fp32


def surface_shares(N, k, oriented):
    """-> (one-way share, mutual share) of the CPU chain on surface(N)."""
    import fpfh_restated as fr
    c = surface(N)
    feats = []
    for x, up in zip((c["src"], c["tgt"]), surface_up(c)):
        idx = fr.neighbours(x, k)
        nrm = fr.normals(x, idx)
        if oriented:
            nrm = orient(nrm, up)
        feats.append(fr.fpfh(x, idx, fr.spfh(x, nrm, idx)).astype(np.float64))
    a, b = feats
    d = ((a[:, :, None] - b[:, None, :]) ** 2).sum(0)
    j, rev = d.argmin(1), d.argmin(0)
    both = rev[j] == np.arange(N)
    return float((j == c["twin"]).mean()), float((j[both] == c["twin"][both]).mean())
