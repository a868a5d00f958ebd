"""include/vcr_hip_gridnn.h restated in numpy: the DEFINITION of the capped nearest neighbour across two clouds as a brute-force
loop (``definition``), the walk that finds it on the target's grid (``walk``: the query clamped into the grid, Chebyshev rings,
the ring bound, the outside bound, the three stops) and the sources the tests run against ``grid_restated.RECIPES``' targets.
Everything is fp32 arithmetic spelled out, with ``grid_restated.fmaf32``'s exact fused multiply-add.

A moved source cloud p is float32 [3, n], a target q float32 [3, m]; a result is (idx int32 [n], d2 bits int32 [n])."""
import numpy as np

import grid_restated as gr

F32 = np.float32
INF_BITS = gr.INF_BITS
NONE_KEY = np.uint64(INF_BITS) << np.uint64(32) | np.uint64(0xFFFFFFFF)          # (+inf, -1)


def cap2_of(max_dist):
    with np.errstate(over="ignore"):
        return F32(max_dist) * F32(max_dist)                 # the fp32 product (1e30: +inf)


def d2_matrix(p, q):
    """The score's d2 of every (moved source point, target point), float32 [n, m]: p - q, then fmaf(dz, dz, fmaf(dy, dy, dx dx))."""
    with np.errstate(all="ignore"):
        dx, dy, dz = (p[c][:, None] - q[c][None, :] for c in range(3))
        return gr.fmaf32(dz, dz, gr.fmaf32(dy, dy, dx * dx))


def key_matrix(D):
    """(d2, j) as uint64 keys [n, m] and which of them are candidates (a d2 that is +inf or NaN never wins)."""
    bits = np.ascontiguousarray(D, F32).view(np.uint32)
    K = bits.astype(np.uint64) << np.uint64(32) | np.arange(D.shape[1], dtype=np.uint64)[None, :]
    return K, bits < INF_BITS


def unpack(best, cap2):
    """Best keys [n] -> (idx, d2 bits): (-1, +inf) where the best d2 is not within the cap."""
    d2 = (best >> np.uint64(32)).astype(np.uint32).view(F32)
    inl = d2 <= cap2
    idx = np.where(inl, (best & np.uint64(0xFFFFFFFF)).astype(np.uint32).view(np.int32), np.int32(-1))
    bits = np.where(inl, d2.view(np.int32), np.int32(INF_BITS))
    return idx.astype(np.int32), bits.astype(np.int32)


def scan(p, q, D=None):
    """The SCAN form's neighbours (include/vcr_hip_score.h): the smallest (d2, j) over the candidates, (-1, +inf) without one.
    D: d2_matrix(p, q), where the caller has it."""
    K, cand = key_matrix(d2_matrix(p, q) if D is None else D)
    best = np.where(cand, K, NONE_KEY).min(1) if q.shape[1] else np.full(p.shape[1], NONE_KEY)
    return unpack(best, F32(np.inf))


def definition(p, q, max_dist, D=None):
    """THE DEFINITION: the scan form's neighbour where it is an inlier (d2 <= cap2), (-1, +inf) where it is not."""
    idx, bits = scan(p, q, D)
    far = ~(bits.view(F32) <= cap2_of(max_dist))
    return np.where(far, np.int32(-1), idx), np.where(far, np.int32(INF_BITS), bits)


def walk(p, q, max_dist, cell=0.0, check=True, D=None):
    """The search as grid_nn_kernel runs it, all queries a ring at a time -> (idx, d2 bits, stats).  stats counts every (query,
    ring) bound and every outside bound taken, and how many of them an unseen candidate undercut (must be 0)."""
    p, q = np.ascontiguousarray(p, F32), np.ascontiguousarray(q, F32)
    n_q, m = p.shape[1], q.shape[1]
    okt, okq = gr.finite(q), gr.finite(p)
    lo, h, n = gr.make_grid(q, cell)
    hi = q[:, okt].max(1).astype(F32) if okt.any() else np.zeros(3, F32)
    face = [gr.faces(lo[c], h, n[c]) for c in range(3)]
    cap2 = cap2_of(max_dist)
    inf = F32(np.inf)
    D = d2_matrix(p, q) if D is None else D
    K, cand = key_matrix(D)
    cand = cand & okt[None, :]
    Dc = np.where(cand, D, inf)
    safe = np.where(okq[None, :], p, lo[:, None]).astype(F32)               # (a query that is not finite walks nothing)
    tcell = np.stack([gr.cells_of(np.where(okt, q[c], lo[c]), face[c], n[c]) for c in range(3)])
    qcell = np.stack([gr.cells_of(safe[c], face[c], n[c]) for c in range(3)])
    with np.errstate(all="ignore"):
        o = np.stack([np.where(safe[c] < lo[c], lo[c] - safe[c], np.where(safe[c] > hi[c], safe[c] - hi[c], F32(0))) for c in range(3)])
        out = (o * o).astype(F32).max(0)
    stats = dict(checks=0, violations=0, outside=int(okq.sum()), outside_violations=0, n=tuple(n), h=float(h), skipped=0,
                 stopped_by_cap=0, stopped_by_best=0)
    if check and m:
        stats["outside_violations"] = int((okq & (Dc.min(1) < out)).sum())
    active = okq & (out <= cap2) & (out < inf)
    stats["skipped"] = int((okq & ~active).sum())
    cheb = np.abs(tcell[:, None, :] - qcell[:, :, None]).max(0)             # [n_q, m]
    rmax = np.maximum(qcell, np.asarray(n)[:, None] - 1 - qcell).max(0)
    best = np.full(n_q, NONE_KEY, np.uint64)
    for r in range(max(n)):
        rows = np.nonzero(active & (rmax >= r))[0]
        if len(rows) == 0:
            break
        ring = cand[rows] & (cheb[rows] == r)
        best[rows] = np.minimum(best[rows], np.where(ring, K[rows], NONE_KEY).min(1) if m else NONE_KEY)
        bound = np.full(len(rows), inf, F32)
        with np.errstate(all="ignore"):
            for c in range(3):
                qc, x = qcell[c, rows], safe[c, rows]
                up = qc + r + 1 <= n[c] - 1
                g = (face[c][np.minimum(qc + r + 1, n[c])] - x).astype(F32)
                bound = np.where(up, np.minimum(bound, (g * g).astype(F32)), bound)
                down = qc - r >= 1
                g = (x - face[c][np.maximum(qc - r, 0)]).astype(F32)
                bound = np.where(down, np.minimum(bound, (g * g).astype(F32)), bound)
        bound = np.maximum(bound, out[rows])
        stats["checks"] += len(rows)
        if check and m:
            unseen = np.where(cheb[rows] > r, Dc[rows], inf).min(1)
            stats["violations"] += int((unseen < bound).sum())
        bd = (best[rows] >> np.uint64(32)).astype(np.uint32).view(F32)
        by_best, by_cap = bd < bound, bound > cap2                           # both STRICT
        stats["stopped_by_best"] += int((by_best & (r < rmax[rows])).sum())
        stats["stopped_by_cap"] += int((by_cap & ~by_best & (r < rmax[rows])).sum())
        active[rows[by_best | by_cap | (bound == inf)]] = False
    idx, bits = unpack(best, cap2)
    return idx, bits, stats


# ------------------------------------------------------------------------------------------------------------- the sources

FAR = 37                                                   # refine_restated.FAR: source points without a partner


def small_pose(seed=0):
    """A rotation of 3 degrees about a random axis and a shift of 0.01 (fp32)."""
    import refine_restated as rr
    rs = np.random.RandomState(1000 + seed)
    R = rr.rotation(rs.normal(size=3), 3.0)
    d = rs.normal(size=3)
    return R.astype(F32), (0.01 * d / np.linalg.norm(d)).astype(F32)


def extent(q):
    ok = gr.finite(q)
    if not ok.any():
        return np.ones(3, F32), np.zeros(3, F32)
    lo, hi = q[:, ok].min(1), q[:, ok].max(1)
    e = (hi - lo).astype(F32)
    return np.where(e > 0, e, F32(1)).astype(F32), lo.astype(F32)


def source_of(q, seed=0, copies=10):
    """A moved source for the target q [3, m]: the target turned by ``small_pose`` about its own corner, `copies` of its points
    untouched (exact partners: d2 = 0) and FAR points a cube's width beyond the box, shuffled.  float32 [3, m + copies + FAR]."""
    import nnscore_restated as nr
    rs = np.random.RandomState(2000 + seed)
    e, lo = extent(q)
    R, t = small_pose(seed)
    with np.errstate(all="ignore"):
        rel = (q - lo[:, None]).astype(F32)
        turned = (nr.moved(rel, R, t * e.max()) + lo[:, None]).astype(F32)
    twin = q[:, rs.randint(0, q.shape[1], copies)]
    far = (lo[:, None] + e[:, None] * rs.uniform(2.0, 3.0, (3, FAR))).astype(F32)
    p = np.concatenate([turned, twin, far], 1)
    return np.ascontiguousarray(p[:, rs.permutation(p.shape[1])])


def shifted(p, q, axes):
    """p moved a whole extent of q beyond q's box along the given axes (fp32, rounded)."""
    e, _ = extent(q)
    s = np.zeros(3, F32)
    s[list(axes)] = e[list(axes)]
    return (p + s[:, None]).astype(F32)


SHIFTS = ((), (0,), (1, 2), (0, 1, 2))
RECIPES = ("lattice", "copies", "equal", "flat", "collinear", "nonfinite", "outlier", "clustered", "tiny")
LARGE = ("lattice", "clustered")                           # the two recipes that also run at N = 2 000


def caps(q):
    """max_dist in {0, half the automatic edge, four edges, 1e30}."""
    h = float(gr.make_grid(q)[1])
    return [0.0, 0.5 * h, 4.0 * h, 1e30]
