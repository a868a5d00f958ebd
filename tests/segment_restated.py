"""CPU restatement of include/segment/vcr_hip_segment.h in numpy -- what the tests compare the kernels
with -- and the recipes the CPU and GPU tests share.  Built on match_restated's `mix32` / `picks` / `fma32` (the draws and the
exact fmaf).

  * `trials_loops` walks the trials one by one in a plain loop, scalar by scalar where the header is scalar; `trials_vector`
    is the same arithmetic on [T, M] arrays.  tests/test_segment_cpu.py holds the two to each other bit for bit.
  * `flags`, `refit_sums` (the header's order of addition: the wave butterfly, the four waves, the blocks ascending) and
    `outputs` finish a cloud; `outputs` takes the normal GIVEN (the device's own) or numpy.linalg.eigh's.
  * `segment_plane` strings them together; `segment_planes` peels."""
import numpy as np

import match_restated as mr

F32, F64 = np.float32, np.float64
BLOCK = 256


def candidates(x, mask=None):
    """x [3,N] fp32 -> the indices with three finite coordinates and a mask other than 0, ascending."""
    ok = np.isfinite(np.asarray(x, F32)).all(0)
    if mask is not None:
        ok &= np.asarray(mask) != 0
    return np.nonzero(ok)[0]


def _plane_of(p0, p1, p2):
    """Three points fp32 [3] -> (status 0 / 2, n32 fp32 [3])."""
    with np.errstate(all="ignore"):
        e1, e2 = (p1 - p0).astype(F32).astype(F64), (p2 - p0).astype(F32).astype(F64)
        n = np.asarray([e1[1] * e2[2] - e1[2] * e2[1], e1[2] * e2[0] - e1[0] * e2[2], e1[0] * e2[1] - e1[1] * e2[0]])
        nn = (n[0] * n[0] + n[1] * n[1]) + n[2] * n[2]
        aa = (e1[0] * e1[0] + e1[1] * e1[1]) + e1[2] * e1[2]
        bb = (e2[0] * e2[0] + e2[1] * e2[1]) + e2[2] * e2[2]
        if not nn > 2.0 ** -40 * (aa * bb):
            return 2, np.zeros(3, F32)
        return 0, (n / np.sqrt(nn)).astype(F32)


def distance(n32, p0, P):
    """n32, p0 fp32 [..., 3] against P fp32 [..., 3] (broadcast) -> fp32 d: fmaf(n.z, r.z, fmaf(n.y, r.y, n.x * r.x))."""
    with np.errstate(all="ignore"):
        r = (np.asarray(P, F32) - np.asarray(p0, F32)).astype(F32)
        return mr.fma32(n32[..., 2], r[..., 2], mr.fma32(n32[..., 1], r[..., 1], (n32[..., 0] * r[..., 0]).astype(F32)))


def trials_loops(x, thr, T, seed, mask=None):
    """One cloud, trial by trial -> dict(M, status [T], picks [T,3], plane fp32 [T,8], count [T])."""
    x = np.asarray(x, F32)
    cand = candidates(x, mask)
    M = len(cand)
    P = np.ascontiguousarray(x[:, cand].T)
    status, picks = np.zeros(T, np.int64), np.full((T, 3), -1, np.int64)
    plane, count = np.zeros((T, 8), F32), np.full(T, -1, np.int64)
    for t in range(T):
        if M < 1:
            status[t] = 1
            continue
        at = [int((int(mr.mix32(np.uint32(seed) ^ mr.mix32(np.uint32((3 * t + j) & 0xFFFFFFFF)))) * M) >> 32) for j in range(3)]
        picks[t] = cand[at]
        if at[0] == at[1] or at[0] == at[2] or at[1] == at[2]:
            status[t] = 1
            continue
        status[t], n32 = _plane_of(P[at[0]], P[at[1]], P[at[2]])
        if status[t]:
            continue
        plane[t, :3], plane[t, 4:7] = n32, P[at[0]]
        with np.errstate(invalid="ignore"):
            count[t] = int((np.abs(distance(n32[None], P[at[0]][None], P)) <= F32(thr)).sum())
    return {"M": M, "status": status, "picks": picks, "plane": plane, "count": count}


def trials_vector(x, thr, T, seed, mask=None, chunk=128):
    """The same on arrays."""
    x = np.asarray(x, F32)
    cand = candidates(x, mask)
    M = len(cand)
    status, picks = np.ones(T, np.int64), np.full((T, 3), -1, np.int64)
    plane, count = np.zeros((T, 8), F32), np.full(T, -1, np.int64)
    if M < 1:
        return {"M": M, "status": status, "picks": picks, "plane": plane, "count": count}
    P = np.ascontiguousarray(x[:, cand].T)
    at = mr.picks(seed, T, M)
    picks = cand[at]
    same = (at[:, 0] == at[:, 1]) | (at[:, 0] == at[:, 2]) | (at[:, 1] == at[:, 2])
    with np.errstate(all="ignore"):
        p0 = P[at[:, 0]]
        e1, e2 = (P[at[:, 1]] - p0).astype(F32).astype(F64), (P[at[:, 2]] - p0).astype(F32).astype(F64)
        n = np.stack([e1[:, 1] * e2[:, 2] - e1[:, 2] * e2[:, 1], e1[:, 2] * e2[:, 0] - e1[:, 0] * e2[:, 2],
                      e1[:, 0] * e2[:, 1] - e1[:, 1] * e2[:, 0]], 1)
        nn = (n[:, 0] * n[:, 0] + n[:, 1] * n[:, 1]) + n[:, 2] * n[:, 2]
        aa = (e1[:, 0] * e1[:, 0] + e1[:, 1] * e1[:, 1]) + e1[:, 2] * e1[:, 2]
        bb = (e2[:, 0] * e2[:, 0] + e2[:, 1] * e2[:, 1]) + e2[:, 2] * e2[:, 2]
        spans = nn > 2.0 ** -40 * (aa * bb)
        n32 = (n / np.sqrt(nn)[:, None]).astype(F32)
    status = np.where(same, 1, np.where(spans, 0, 2)).astype(np.int64)
    live = np.nonzero(status == 0)[0]
    plane[live, :3], plane[live, 4:7] = n32[live], p0[live]
    with np.errstate(invalid="ignore"):
        for lo in range(0, len(live), chunk):
            tl = live[lo:lo + chunk]
            count[tl] = (np.abs(distance(n32[tl][:, None, :], p0[tl][:, None, :], P[None])) <= F32(thr)).sum(1)
    return {"M": M, "status": status, "picks": picks, "plane": plane, "count": count}


def flags(x, thr, plane_row, mask=None):
    """The winner's inlier flags over ALL points: int32 [N]."""
    x = np.asarray(x, F32)
    out = np.zeros(x.shape[1], np.int32)
    cand = candidates(x, mask)
    with np.errstate(invalid="ignore"):
        d = distance(plane_row[None, :3], plane_row[None, 4:7], np.ascontiguousarray(x[:, cand].T))
        out[cand[np.abs(d) <= F32(thr)]] = 1
    return out


def refit_sums(x, inlier, o):
    """The nine fp64 sums (sx sy sz sxx sxy sxz syy syz szz) of r = x - o over the inliers, in the header's order."""
    x = np.asarray(x, F32)
    N = x.shape[1]
    nblk = (N + BLOCK - 1) // BLOCK
    with np.errstate(all="ignore"):
        r = (x - np.asarray(o, F32)[:, None]).astype(F32).astype(F64)
    r = np.where(np.asarray(inlier)[None] > 0, r, 0.0)      # (an inlier is finite)
    terms = np.zeros((9, nblk * BLOCK))
    terms[:, :N] = [r[0], r[1], r[2], r[0] * r[0], r[0] * r[1], r[0] * r[2], r[1] * r[1], r[1] * r[2], r[2] * r[2]]
    a = terms.reshape(9, nblk, 4, 64)
    lane = np.arange(64)
    for off in (32, 16, 8, 4, 2, 1):                        # the wave butterfly
        a = a + a[..., lane ^ off]
    w = a[..., 0]
    blocks = ((w[..., 0] + w[..., 1]) + w[..., 2]) + w[..., 3]
    tot = np.zeros(9)
    for blk in range(nblk):
        tot = tot + blocks[:, blk]
    return tot


def covariance(sums, cnt):
    m = sums[:3] / cnt
    C = np.empty((3, 3))
    for (i, j), k in zip(((0, 0), (0, 1), (0, 2), (1, 1), (1, 2), (2, 2)), range(3, 9)):
        C[i, j] = C[j, i] = sums[k] / cnt - m[i] * m[j]
    return m, C


def eigh_normal(sums, cnt, trial_n32):
    """numpy.linalg.eigh's normal of the sums (fp32, the sign rule applied) and the eigenvalues; None where the header falls
    back to the trial's own plane."""
    if cnt < 3:
        return None, None
    m, C = covariance(sums, cnt)
    if not np.isfinite(C).all() or not C.any():
        return None, None
    lam, V = np.linalg.eigh(C)
    n = (V[:, 0] / np.sqrt((V[0, 0] * V[0, 0] + V[1, 0] * V[1, 0]) + V[2, 0] * V[2, 0])).astype(F32)
    t = np.asarray(trial_n32, F32).astype(F64)
    if (n[0].astype(F64) * t[0] + n[1].astype(F64) * t[1]) + n[2].astype(F64) * t[2] < 0:
        n = -n
    return n, lam


def outputs(plane_row, sums, cnt, normal):
    """(plane fp32 [4], point fp32 [3]) from the winner's row, the sums and the refit's fp32 normal (None: the trial's own)."""
    o = plane_row[4:7].astype(F64)
    if normal is None:
        n, q = plane_row[:3].astype(F32), o
    else:
        n, q = np.asarray(normal, F32), o + sums[:3] / cnt
    nd = n.astype(F64)
    d = -((nd[0] * q[0] + nd[1] * q[1]) + nd[2] * q[2])
    return np.asarray([n[0], n[1], n[2], F32(d)], F32), q.astype(F32)


def head(o, T):
    """The first T trials of a trials dict: a trial is a function of (seed, t, the cloud) alone, never of the trial count."""
    return {k: (v if k == "M" else v[:T]) for k, v in o.items() if k in ("M", "status", "picks", "plane", "count")}


def finish(x, thr, o, mask=None):
    """The trials' dict -> the same plus best_trial, best_count, inlier, sums, fit (the plane [4]), point, normal, lam (the refit by
    numpy.linalg.eigh)."""
    x = np.asarray(x, F32)
    o = dict(o)
    bt, cnt = mr.best(o["count"], o["status"] == 0)
    o.update(best_trial=bt, best_count=cnt)
    if bt < 0:
        o.update(inlier=np.zeros(x.shape[1], np.int32), sums=np.zeros(9), fit=np.full(4, np.nan, F32),
                 point=np.full(3, np.nan, F32), normal=None, lam=None)
        return o
    row = o["plane"][bt]
    inl = flags(x, thr, row, mask)
    sums = refit_sums(x, inl, row[4:7])
    normal, lam = eigh_normal(sums, cnt, row[:3])
    fit, point = outputs(row, sums, cnt, normal)
    o.update(inlier=inl, sums=sums, fit=fit, point=point, normal=normal, lam=lam)
    return o


def segment_plane(x, thr, T, seed, mask=None, trials=trials_vector):
    """One cloud -> everything `finish` returns."""
    return finish(x, thr, trials(np.asarray(x, F32), thr, T, seed, mask), mask)


def segment_planes(x, thr, K, min_inliers, T, seed):
    """One cloud -> (labels int32 [N], counts [K], planes [K,4]) by peeling, round k with seed + k."""
    x = np.asarray(x, F32)
    labels, counts, planes = np.full(x.shape[1], -1, np.int32), np.zeros(K, np.int64), np.full((K, 4), np.nan, F32)
    for k in range(K):
        o = segment_plane(x, thr, T, seed + k, mask=(labels < 0).astype(np.int32))
        if o["best_count"] < max(min_inliers, 1):
            break
        labels[o["inlier"] > 0] = k
        counts[k], planes[k] = o["best_count"], o["fit"]
    return labels, counts, planes


# ----------------------------------------------------------------------------------------------------------------- the recipes

PLANTED = dict(N=2000, share=0.6, thr=0.02, T=256, seed=0)
PLANTED_NOISE = 0.25                                       # the planted points lie within this share of thr of their plane
# What a test may conclude from "every planted point is an inlier of the winner".  The planted points cover the whole cut of
# their plane with the box (the patch below reaches the box's half diagonal from its centre) and lie within PLANTED_NOISE thr of
# it; as inliers they lie within thr of the winner's plane.  Two planes that close over the patch differ by at most
# (1 + PLANTED_NOISE) thr anywhere on it, so EVERY inlier of the box is within (2 + PLANTED_NOISE) thr of the planted plane ...
EXTRA_WITHIN = 2.0 + PLANTED_NOISE
# ... and a plane fitted to points within that distance over a patch of half-width box / 2 or more cannot tilt by more than the
# rise EXTRA_WITHIN thr over the run box / 2 (a coarse bound; the tests print what is reached)


def angle_bound(thr, box=1.0):
    return float(np.arctan(EXTRA_WITHIN * thr / (box / 2)))


def planted(N, share=0.6, thr=0.02, seed=0, box=1.0):
    """-> dict: x fp32 [3,N] -- round(share N) points within PLANTED_NOISE thr of a plane through the centre of the box
    [0, box]^3, spread over a square patch of half-width sqrt(3) / 2 box in it, the rest uniform in the box, shuffled --,
    normal (float64, unit), d, on bool [N] (the planted points)."""
    rs = np.random.RandomState(4100 + seed + N)
    n = rs.normal(size=3)
    n /= np.linalg.norm(n)
    c = np.full(3, box / 2)
    u = np.cross(n, [1.0, 0.0, 0.0] if abs(n[0]) < 0.9 else [0.0, 1.0, 0.0])
    u /= np.linalg.norm(u)
    v = np.cross(n, u)
    n_on = int(round(share * N))
    half = np.sqrt(3.0) / 2 * box
    ab = rs.uniform(-half, half, (2, n_on))
    on_pts = (c[:, None] + u[:, None] * ab[0] + v[:, None] * ab[1]
              + n[:, None] * rs.uniform(-PLANTED_NOISE * thr, PLANTED_NOISE * thr, n_on))
    off_pts = rs.uniform(0, box, (3, N - n_on))
    perm = rs.permutation(N)
    x = np.concatenate([on_pts, off_pts], 1)[:, perm].astype(F32)
    on = (np.arange(N) < n_on)[perm]
    return {"x": x, "normal": n, "d": -float(n @ c), "on": on}


def angle(a, b):
    """The angle between two directions, sign ignored (radians)."""
    a, b = np.asarray(a, F64), np.asarray(b, F64)
    c = abs(a @ b) / (np.linalg.norm(a) * np.linalg.norm(b))
    return float(np.arccos(min(1.0, c)))


def cloud(N, seed=0):
    """A small cloud for the parity tests: a third near the plane z = 0.3 x + 0.1, the rest uniform in the unit cube."""
    rs = np.random.RandomState(77 + 13 * N + seed)
    x = rs.uniform(0, 1, (3, N))
    near = rs.uniform(0, 1, N) < 0.4
    x[2] = np.where(near, 0.3 * x[0] + 0.1 + rs.uniform(-0.01, 0.01, N), x[2])
    return x.astype(F32)
