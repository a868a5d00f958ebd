"""CPU restatement of include/consistency/vcr_hip_consistency.h in numpy -- what the tests compare
the kernels with.  It shares no code with the device: the pair list, the fmaf chains, the exact fmaf and the recipes are
tests/match_restated.py's, the square root is numpy's on float32 (correctly rounded), the rigid step is refine_restated's
(`cross`, `solve`: numpy's SVD, so a pose is held to the device's by properties only), every integer stage is restated here.

Every stage has an entrance of its own, so that a test can feed it the device's previous stage:
  `rows`          corr -> the pair list and its points P, Q [M,3]
  `compatible`    the relation between two sets of rows
  `degree`        deg [M]
  `kept_order`    deg -> the kept positions, by rank
  `adjacency`     the kept rows -> bool [P,P];  `pack` / `unpack`: the header's bit layout in 64-bit words
  `second_order`  adj -> w [S,P], wmax [S];  `members` -> bool [S,P]
  `chain_sum`     the header's sum order;  `sums` / `hypothesis`: the rigid step of one member set
  `counts`        poses -> count over all M pairs (match_restated.d2_under);  `best`: match_restated.best
`consistency` strings them together on the CPU's own stages for one cloud."""
import numpy as np

import match_restated as mr
import refine_restated as rr

F32 = np.float32
KEY_TOP = 0x1FFFF


def rows(src, tgt, corr):
    """src [3,Ns], tgt [3,Nt] fp32, corr int [Ns] -> (pl int64 [M]: the source indices of the pairs, P, Q fp32 [M,3])."""
    src, tgt, corr = np.asarray(src, F32), np.asarray(tgt, F32), np.asarray(corr, np.int64)
    pl = mr.pair_list(corr, tgt.shape[1])
    return pl, np.ascontiguousarray(src[:, pl].T), np.ascontiguousarray(tgt[:, corr[pl]].T)


def compatible(Pa, Qa, Pb, Qb, tau, min_length=0.0):
    """rows a [n,3] x rows b [m,3] -> bool [n,m]: fabsf(ds - dt) <= tau && ds2 >= min_len2 && dt2 >= min_len2 (a == b is the
    caller's to exclude)."""
    min_len2 = F32(min_length) * F32(min_length)
    with np.errstate(invalid="ignore", over="ignore"):
        ds2 = mr.len2(Pa[:, None, :], Pb[None, :, :])
        dt2 = mr.len2(Qa[:, None, :], Qb[None, :, :])
        ds, dt = np.sqrt(ds2.astype(F32)), np.sqrt(dt2.astype(F32))
        return (np.abs(ds - dt) <= F32(tau)) & (ds2 >= min_len2) & (dt2 >= min_len2)


def degree(P, Q, tau, min_length=0.0, chunk=256):
    """-> int64 [M]: per pair the number of OTHER pairs compatible with it."""
    M = P.shape[0]
    deg = np.zeros(M, np.int64)
    for lo in range(0, M, chunk):
        ok = compatible(P[lo:lo + chunk], Q[lo:lo + chunk], P, Q, tau, min_length)
        n = ok.shape[0]
        ok[np.arange(n), lo + np.arange(n)] = False
        deg[lo:lo + chunk] = ok.sum(1)
    return deg


def deg_by_source(deg, pl, Ns):
    """deg [M] -> the optional output's layout: int [Ns] in the source's numbering, -1 for a point without a pair."""
    out = np.full(Ns, -1, np.int64)
    out[pl] = deg
    return out


def kept_order(deg, keep):
    """-> int64 [P], P = min(M, keep): the positions in the pair list by rank -- descending degree, the lower position among
    equals (a stable sort of 0x1FFFF - deg)."""
    key = KEY_TOP - np.asarray(deg, np.int64)
    return np.argsort(key, kind="stable")[:min(len(key), keep)]


def adjacency(Pk, Qk, tau, min_length=0.0):
    """The kept rows [P,3] -> bool [P,P], the diagonal False."""
    ok = compatible(Pk, Qk, Pk, Qk, tau, min_length)
    np.fill_diagonal(ok, False)
    return ok


def pack(bits, keep):
    """bool [..., n <= keep] -> uint64 [..., keep / 64]: bit c of a row is bit c % 64 of word c / 64."""
    bits = np.asarray(bits, bool)
    full = np.zeros(bits.shape[:-1] + (keep,), bool)
    full[..., :bits.shape[-1]] = bits
    w = full.reshape(bits.shape[:-1] + (keep // 64, 64)).astype(np.uint64)
    return (w << np.arange(64, dtype=np.uint64)).sum(-1, dtype=np.uint64)


def unpack(words, n):
    """uint64 / int64 [..., W] -> bool [..., n]."""
    w = np.ascontiguousarray(words).view(np.uint64)
    bits = ((w[..., :, None] >> np.arange(64, dtype=np.uint64)) & np.uint64(1)).astype(bool)
    return bits.reshape(w.shape[:-1] + (64 * w.shape[-1],))[..., :n]


def second_order(adj, S):
    """adj bool [P,P] -> (w int64 [S,P]: popcount(adj[r] & adj[c]) where adj[r][c], else 0; wmax int64 [S])."""
    a = adj.astype(F32)                                       # (counts up to 4096 are exact in fp32: the product may use BLAS)
    w = np.where(adj[:S], (a[:S] @ a.T).astype(np.int64), 0)
    return w, (w.max(1) if w.shape[1] else np.zeros(S, np.int64))


def members(adj, w, wmax, ratio):
    """-> bool [S,P]: r itself, and every c set in adj[r] with (float)w >= ratio * (float)wmax (an fp32 product)."""
    S = w.shape[0]
    m = adj[:S] & (w.astype(F32) >= F32(ratio) * wmax.astype(F32)[:, None])
    m[np.arange(S), np.arange(S)] = True
    return m


def chain_sum(values, member):
    """values float64 [P, ...] of the kept ranks, member bool [P] -> the header's sum: chain l adds the members c with c % 64
    == l in ascending c onto +0, the 64 chains are folded by the butterfly v_l += v_{l ^ o}, o = 32 ... 1."""
    values = np.asarray(values, np.float64)
    chains = np.zeros((64,) + values.shape[1:], np.float64)
    with np.errstate(invalid="ignore", over="ignore"):
        for c in np.nonzero(member)[0]:
            chains[c % 64] = chains[c % 64] + values[c]
        lanes = np.arange(64)
        for o in (32, 16, 8, 4, 2, 1):
            chains = chains + chains[lanes ^ o]
    return chains[0]


def chain_sums(values, mem):
    """chain_sum for many member sets at once: values float64 [P,k], mem bool [S,P] -> [S,k].  A rank that is no member adds
    +0 here, which leaves a chain that started at +0 as it is."""
    values = np.asarray(values, np.float64)
    S, P = mem.shape
    chains = np.zeros((S, 64, values.shape[1]), np.float64)
    with np.errstate(invalid="ignore", over="ignore"):
        for lo in range(0, P, 64):
            v, m = values[lo:lo + 64], mem[:, lo:lo + 64]
            chains[:, :v.shape[0]] = chains[:, :v.shape[0]] + np.where(m[:, :, None], v[None], 0.0)
        lanes = np.arange(64)
        for o in (32, 16, 8, 4, 2, 1):
            chains = chains + chains[:, lanes ^ o]
    return chains[:, 0]


def sums(Pk, Qk, member):
    """-> (n, S_p [3], S_q [3], S_pq [3,3]) in fp64 over the members of one seed."""
    p, q = np.asarray(Pk, F32).astype(np.float64), np.asarray(Qk, F32).astype(np.float64)
    with np.errstate(invalid="ignore", over="ignore"):
        return int(member.sum()), chain_sum(p, member), chain_sum(q, member), chain_sum(p[:, :, None] * q[:, None, :], member)


def hypotheses(Pk, Qk, mem):
    """hypothesis for every row of mem bool [S,P] -> list of S."""
    p, q = np.asarray(Pk, F32).astype(np.float64), np.asarray(Qk, F32).astype(np.float64)
    with np.errstate(invalid="ignore", over="ignore"):
        all15 = chain_sums(np.concatenate([p, q, (p[:, :, None] * q[:, None, :]).reshape(-1, 9)], 1), mem)
    return [hypothesis(Pk, Qk, mem[r], (int(mem[r].sum()), all15[r, :3], all15[r, 3:6], all15[r, 6:].reshape(3, 3)))
            for r in range(mem.shape[0])]


def hypothesis(Pk, Qk, member, given=None):
    """One seed's rigid step -> None with fewer than three members, else dict(n, R, t float64 (NaN for non-finite sums), H,
    opt, s1, pm, qm).  given: its (n, S_p, S_q, S_pq) where they were summed already."""
    n, Sp, Sq, Spq = sums(Pk, Qk, member) if given is None else given
    if n < 3:
        return None
    inv_n = 1.0 / np.float64(n)
    if not (np.isfinite(Sp).all() and np.isfinite(Sq).all() and np.isfinite(Spq).all()):
        return {"n": n, "R": np.full((3, 3), np.nan), "t": np.full(3, np.nan), "H": None}
    H = Spq - np.outer(Sp, Sq) * inv_n
    R, opt, s1 = rr.solve(H)
    pm, qm = Sp * inv_n, Sq * inv_n
    return {"n": n, "R": R, "t": qm - R @ pm, "H": H, "opt": opt, "s1": s1, "pm": pm, "qm": qm}


def counts(P, Q, pose, max_dist, chunk=64):
    """pose fp32 [T,12] GIVEN -> int64 [T]: the pairs of ALL M with d2 <= max_dist^2 under it (the RANSAC's expressions)."""
    limit = F32(max_dist) * F32(max_dist)
    pose = np.asarray(pose, F32)
    out = np.zeros(pose.shape[0], np.int64)
    with np.errstate(invalid="ignore", over="ignore"):
        for lo in range(0, pose.shape[0], chunk):
            out[lo:lo + chunk] = (mr.d2_under(pose[lo:lo + chunk], P[None], Q[None]) <= limit).sum(1)
    return out


IDENTITY = np.asarray([1, 0, 0, 0, 1, 0, 0, 0, 1, 0, 0, 0], F32)


def consistency(src, tgt, corr, max_dist, tau=None, keep=1024, seeds=64, ratio=0.5, min_length=0.0):
    """One cloud on the CPU's own stages -> dict(pairs, pl, deg [M], order [P], adj bool [P,P], w, wmax, member bool [S,P],
    status [seeds], n [seeds], pose fp32 [seeds,12], count [seeds], best_seed, inliers, R, t)."""
    tau = max_dist if tau is None else tau
    pl, P, Q = rows(src, tgt, corr)
    M = len(pl)
    deg = degree(P, Q, tau, min_length)
    order = kept_order(deg, keep)
    Pk, Qk = P[order], Q[order]
    adj = adjacency(Pk, Qk, tau, min_length)
    S = min(len(order), seeds)
    w, wmax = second_order(adj, S)
    mem = members(adj, w, wmax, ratio)
    status = np.ones(seeds, np.int64)
    n = np.zeros(seeds, np.int64)
    pose = np.zeros((seeds, 12), F32)
    count = np.full(seeds, -1, np.int64)
    for r, h in enumerate(hypotheses(Pk, Qk, mem)):
        n[r] = mem[r].sum()
        if h is None:
            continue
        with np.errstate(invalid="ignore", over="ignore"):
            pose[r] = np.concatenate([h["R"].reshape(9), h["t"]]).astype(F32)
        status[r] = 0 if np.isfinite(pose[r]).all() else 3
    live = np.nonzero(status == 0)[0]
    if len(live):
        count[live] = counts(P, Q, pose[live], max_dist)
    bs, inl = mr.best(count, status == 0)
    Rt = pose[bs] if bs >= 0 else IDENTITY
    return {"pairs": M, "pl": pl, "deg": deg, "order": order, "adj": adj, "w": w, "wmax": wmax, "member": mem, "status": status,
            "n": n, "pose": pose, "count": count, "best_seed": bs, "inliers": inl, "R": Rt[:9].reshape(3, 3), "t": Rt[9:]}
