"""include/query/vcr_hip_query.h restated in numpy: the DEFINITION of the two searches from any query positions as brute-force
loops (``knn``, ``radius_rows``), the walk that finds them on the POINTS' grid (``walk``: tests/grid_restated.py's grid and faces,
the query's cell clamped into the grid, the Chebyshev rings, the fp32 ring bound joined with the query's distances to the box, the two strict stops) and the
recipes of the queries the tests run over ``grid_restated.RECIPES``' clouds.  Everything is fp32 arithmetic spelled out on
grid_restated's ``fmaf32`` / ``keys``.

The points of one cloud are a float32 array [3, N], its queries a float32 array [3, M].  A kNN result is (idx int32 [M,k], d2 bits
int32 [M,k]); a radius result is radius_restated's dict over the M rows."""
import numpy as np

import grid_restated as gr
import radius_restated as rr

F32 = np.float32
INF_BITS = gr.INF_BITS
NONE_KEY = np.uint64(INF_BITS) << np.uint64(32) | np.uint64(0xFFFFFFFF)          # (+inf, -1): a slot without a neighbour
LOW = np.uint64(0xFFFFFFFF)


def d2_matrix(xyz, queries):
    """The definition's d2 of every (query, point), float32 [M, N]: x_j - q_i, then fmaf(dz, dz, fmaf(dy, dy, dx * dx))."""
    xyz, queries = np.ascontiguousarray(xyz, F32), np.ascontiguousarray(queries, F32)
    with np.errstate(all="ignore"):
        dx, dy, dz = (xyz[c][None, :] - queries[c][:, None] for c in range(3))
        return gr.fmaf32(dz, dz, gr.fmaf32(dy, dy, dx * dx)).reshape(queries.shape[1], xyz.shape[1])


def key_matrix(xyz, queries, D=None):
    """-> (keys uint64 [M, N] that order like (d2, j), candidates bool [M, N]): a finite point against a finite query whose d2
    is not +inf (or NaN)."""
    D = d2_matrix(xyz, queries) if D is None else D
    bits = np.ascontiguousarray(D, F32).view(np.uint32)
    K = bits.astype(np.uint64) << np.uint64(32) | np.arange(D.shape[1], dtype=np.uint64)[None, :]
    cand = (bits < INF_BITS) & gr.finite(np.asarray(xyz, F32))[None, :] & gr.finite(np.asarray(queries, F32))[:, None]
    return K, cand


def unpack(keys):
    return (keys & LOW).astype(np.uint32).view(np.int32), (keys >> np.uint64(32)).astype(np.uint32).view(np.int32)


def first_k(K, take, k):
    """The k smallest keys of every row among those taken, ascending; (+inf, -1) where there are fewer."""
    M = K.shape[0]
    full = np.full((M, k), NONE_KEY, np.uint64)
    masked = np.where(take, K, NONE_KEY)
    if masked.shape[1] > k:                                  # (the k smallest first: a full sort of every row is not needed)
        masked = np.partition(masked, k - 1, axis=1)[:, :k]
    srt = np.sort(masked, axis=1)
    full[:, :srt.shape[1]] = srt
    return full


def knn(xyz, queries, k, D=None):
    """THE DEFINITION.  -> (idx int32 [M,k], d2 bits int32 [M,k]): the k smallest candidates under (d2, j), no index excluded;
    -1 / +inf where a row is short (a query that is not finite, fewer than k candidates, k > N)."""
    K, cand = key_matrix(xyz, queries, D)
    return unpack(first_k(K, cand, k))


def rows_of(K, take):
    """Ascending key arrays, one a query -> radius_restated's result dict."""
    return rr.csr([np.sort(K[i][take[i]]) for i in range(K.shape[0])], K.shape[0])


def radius_rows(xyz, queries, radius, D=None):
    """THE DEFINITION.  For a finite query ALL candidates with d2 <= r2, ascending in (d2, j); an empty row otherwise."""
    D = d2_matrix(xyz, queries) if D is None else D
    K, cand = key_matrix(xyz, queries, D)
    with np.errstate(all="ignore"):
        return rows_of(K, cand & (D <= rr.r2_of(radius)))


# ---------------------------------------------------------------------------------------------------------------- the walk

def side(o, c, g):
    """What no point behind a side at distance g along axis c can undercut, for queries whose distances to the box are o [3, R]:
    its difference along c is at least max(g, o_c), along the other axes at least o_a, and d2's expression is monotone in each.
    Inside the box (o = 0) this is g * g, grid_restated's term, bit for bit."""
    m = [np.maximum(g, o[a]) if a == c else o[a] for a in range(3)]
    with np.errstate(all="ignore"):
        return gr.fmaf32(m[2], m[2], gr.fmaf32(m[1], m[1], (m[0] * m[0]).astype(F32))).reshape(g.shape)


def walk(xyz, queries, k=None, radius=None, cell=0.0, D=None):
    """The search as the kernels run it, all queries a ring at a time -> (result, stats): the kNN rows with k, the radius rows
    with radius.  The grid is the POINTS' (edge: grid_restated's rule for kNN, the radius for the radius search, `cell` where
    forced); a query's cell is clamped into it, and every side's term of the ring bound holds the query's distances to the
    points' box (``side``).  stats counts every (query, ring) bound taken and how many of them -- and of the outside bounds
    taken -- an unseen candidate undercut (must be 0)."""
    assert (k is None) != (radius is None)
    xyz, queries = np.ascontiguousarray(xyz, F32), np.ascontiguousarray(queries, F32)
    M = queries.shape[1]
    okp, okq = gr.finite(xyz), gr.finite(queries)
    edge = cell if cell > 0 else (0.0 if radius is None else F32(radius))
    lo, h, n = gr.make_grid(xyz, edge)
    hi = xyz[:, okp].max(1).astype(F32) if okp.any() else np.zeros(3, F32)
    face = [gr.faces(lo[c], h, n[c]) for c in range(3)]
    assert all((np.diff(f) >= 0).all() for f in face)                  # monotone
    inf = F32(np.inf)
    D = d2_matrix(xyz, queries) if D is None else D
    K, cand = key_matrix(xyz, queries, D)
    Dc = np.where(cand, D, inf)
    safe = np.where(okq[None, :], queries, lo[:, None]).astype(F32)         # (a query that is not finite walks nothing)
    pcell = np.stack([gr.cells_of(np.where(okp, xyz[c], lo[c]), face[c], n[c]) for c in range(3)])
    qcell = np.stack([gr.cells_of(safe[c], face[c], n[c]) for c in range(3)])          # clamped: below lo 0, above n - 1
    with np.errstate(all="ignore"):
        o = np.stack([np.where(safe[c] < lo[c], lo[c] - safe[c], np.where(safe[c] > hi[c], safe[c] - hi[c], F32(0))) for c in range(3)])
        out = (o * o).astype(F32).max(0)
        r2 = None if radius is None else rr.r2_of(radius)
    stats = dict(checks=0, violations=0, outside_violations=0, n=tuple(n), h=float(h), skipped=0, stopped_early=0, looked=0)
    active = okq & okp.any()                                                # (a cloud without a finite point: nothing is walked)
    stats["outside_violations"] = int((active & (Dc.min(1) < out)).sum()) if xyz.shape[1] else 0
    active &= (out < inf) if r2 is None else (out <= r2)                    # (+inf: every d2 overflows; > r2: no hit)
    stats["skipped"] = int((okq & ~active).sum())
    cheb = np.abs(pcell[:, None, :] - qcell[:, :, None]).max(0)             # [M, N]
    rmax = np.maximum(qcell, np.asarray(n)[:, None] - 1 - qcell).max(0)
    seen = np.zeros(D.shape, bool)
    for r in range(max(n)):
        rows = np.nonzero(active & (rmax >= r))[0]
        if len(rows) == 0:
            break
        seen[rows] |= cand[rows] & (cheb[rows] == r)
        stats["looked"] += int((okp[None, :] & (cheb[rows] == r)).sum())
        bound = np.full(len(rows), inf, F32)
        with np.errstate(all="ignore"):
            for c in range(3):
                qc, x = qcell[c, rows], safe[c, rows]
                up = qc + r + 1 <= n[c] - 1
                g = (face[c][np.minimum(qc + r + 1, n[c])] - x).astype(F32)
                bound = np.where(up, np.minimum(bound, side(o[:, rows], c, g)), bound)
                down = qc - r >= 1
                g = (x - face[c][np.maximum(qc - r, 0)]).astype(F32)
                bound = np.where(down, np.minimum(bound, side(o[:, rows], c, g)), bound)
        unseen = np.where(cheb[rows] > r, Dc[rows], inf).min(1) if xyz.shape[1] else np.full(len(rows), inf, F32)
        stats["checks"] += len(rows)
        if r2 is None:
            kth = (first_k(K[rows], seen[rows], k)[:, k - 1] >> np.uint64(32)).astype(np.uint32).view(F32)
            stats["violations"] += int((unseen < bound).sum())              # at every bound taken, as grid_restated.walk
            stop = kth < bound                                              # STRICTLY below
        else:
            stop = bound > r2                                               # STRICTLY above: a point at exactly r2 is a hit
            stats["violations"] += int((stop & (unseen <= r2)).sum())
        stats["stopped_early"] += int((stop & (r < rmax[rows])).sum())
        active[rows[stop]] = False
    if r2 is None:
        return unpack(first_k(K, seen, k)), stats
    with np.errstate(all="ignore"):
        return rows_of(K, seen & (D <= r2)), stats


# ------------------------------------------------------------------------------------------------------------- the queries

def box(xyz):
    """(lo, hi, extent with 1 for a flat axis) of the finite points, float32 [3] each."""
    ok = gr.finite(xyz)
    if not ok.any():
        return np.zeros(3, F32), np.zeros(3, F32), np.ones(3, F32)
    lo, hi = xyz[:, ok].min(1).astype(F32), xyz[:, ok].max(1).astype(F32)
    with np.errstate(all="ignore"):
        e = np.minimum(hi - lo, np.finfo(F32).max).astype(F32)
    return lo, hi, np.where(e > 0, e, F32(1)).astype(F32)


def q_same(xyz, M, seed=0):
    """The points themselves (again from the front where M > N)."""
    return np.ascontiguousarray(xyz[:, np.arange(M) % xyz.shape[1]])


def q_jitter(xyz, M, seed=0):
    """Points of the cloud plus noise of about a cell of its automatic grid."""
    rs = np.random.RandomState(3000 + seed)
    h = float(gr.make_grid(xyz)[1])
    base = xyz[:, rs.randint(0, xyz.shape[1], M)]
    with np.errstate(all="ignore"):
        return (base + rs.normal(size=(3, M)) * h).astype(F32)


def q_outside(xyz, M, seed=0):
    """Uniform in the box scaled x3 about its centre: beyond every face, edge and corner, and some inside."""
    rs = np.random.RandomState(4000 + seed)
    lo, hi, e = box(xyz)
    c = 0.5 * (lo.astype(np.float64) + hi)
    return (c[:, None] + (rs.uniform(-1.5, 1.5, (3, M)) * e[:, None])).astype(F32)


def q_faces(xyz, M, seed=0):
    """Exactly lo, exactly hi, and per coordinate a face of the automatic grid (fmaf(j, h, lo), the kernels' value)."""
    rs = np.random.RandomState(5000 + seed)
    lo, hi, _ = box(xyz)
    _, h, n = gr.make_grid(xyz)
    q = np.stack([gr.faces(lo[c], h, n[c])[rs.randint(0, n[c] + 1, M)] for c in range(3)]).astype(F32)
    q[:, 0] = lo
    if M > 1:
        q[:, 1] = hi
    for i in range(2, min(M, 8)):                                            # lo on some axes, hi on the others
        q[:, i] = np.where([(i >> c) & 1 for c in range(3)], hi, lo)
    return q


def q_far(xyz, M, seed=0):
    """Jittered queries moved 1e6 along one axis (the first half) and 3e19 (the second: every d2 overflows, the row is empty)."""
    q = q_jitter(xyz, M, seed)
    rs = np.random.RandomState(6000 + seed)
    axis, sign = rs.randint(0, 3, M), rs.choice([-1.0, 1.0], M)
    step = np.where(np.arange(M) < (M + 1) // 2, 1e6, 3e19) * sign
    with np.errstate(all="ignore"):
        q[axis, np.arange(M)] = (q[axis, np.arange(M)] + step).astype(F32)
    return q


def q_nonfinite(xyz, M, seed=0):
    """Jittered queries with NaN at query 0 and NaN, +inf and -inf elsewhere."""
    q = q_jitter(xyz, M, seed)
    q[0, 0] = np.nan
    if M > 7:
        q[1, 5], q[2, M // 2], q[0, M - 1] = np.inf, -np.inf, np.nan
        q[:, 7] = np.nan
    return q


def q_one(xyz, M, seed=0):
    """All queries equal: the cloud's first finite point (the first point where there is none)."""
    ok = np.flatnonzero(gr.finite(xyz))
    return np.ascontiguousarray(np.tile(xyz[:, ok[0] if len(ok) else 0][:, None], (1, M)))


QUERIES = {"same": q_same, "jitter": q_jitter, "outside": q_outside, "faces": q_faces, "far": q_far, "nonfinite": q_nonfinite,
           "one": q_one}
