"""include/vcr_hip_radius.h restated in numpy: the DEFINITION of the radius search's result as a brute-force loop
(``radius_rows``) and the walk that finds it (``walk_radius``: tests/grid_restated.py's grid, faces and cells by comparison, the
Chebyshev rings, the fp32 ring bound, and the STRICT stop bound > r2).  Everything is fp32 arithmetic spelled out on
grid_restated's ``d2_row`` / ``fmaf32``.

One cloud is a float32 array [3, N].  A result is a dict of count int32 [N] (n_i), row_start int64 [N + 1], total (int), idx
int32 [total] and bits int32 [total] (d2's bits): the rows one behind the other."""
import numpy as np

import grid_restated as gr

F32 = np.float32
INF_BITS = gr.INF_BITS
FAR = np.asarray([[1024.0], [-512.0], [256.0]], F32)       # the translation the tests move their clouds by


def r2_of(radius):
    """radius * radius in fp32, one rounding."""
    with np.errstate(over="ignore"):
        return F32(F32(radius) * F32(radius))


def d2_all(xyz):
    """The definition's d2 of every query against every point, float32 [N, N]: row i is grid_restated.d2_row(xyz, i)."""
    xyz = np.ascontiguousarray(xyz, F32)
    N = xyz.shape[1]
    return np.stack([gr.d2_row(xyz, i) for i in range(N)]) if N else np.zeros((0, 0), F32)


def csr(rows, N):
    """Ascending key arrays, one a query -> the result dict."""
    count = np.asarray([len(r) for r in rows], np.int32)
    row_start = np.zeros(N + 1, np.int64)
    np.cumsum(count, out=row_start[1:])
    flat = np.concatenate(rows) if len(rows) else np.zeros(0, np.uint64)
    flat = flat.astype(np.uint64)
    return {"count": count, "row_start": row_start, "total": int(row_start[N]),
            "idx": (flat & np.uint64(0xFFFFFFFF)).astype(np.int32),
            "bits": (flat >> np.uint64(32)).astype(np.uint32).view(np.int32)}


def radius_rows(xyz, radius, rows=None, d2=None):
    """THE DEFINITION.  For a finite query i every finite j != i with d2(i, j) <= r2, ascending in (d2, j); an empty row for a
    query that is not finite.  rows: the queries to answer (all by default; the dict then describes those rows alone).
    d2: d2_all(xyz), if the caller has it."""
    xyz = np.ascontiguousarray(xyz, F32)
    N = xyz.shape[1]
    ok = gr.finite(xyz)
    r2 = r2_of(radius)
    me = np.arange(N)
    out = []
    with np.errstate(all="ignore"):
        for i in (range(N) if rows is None else rows):
            i = int(i)
            if not ok[i]:
                out.append(np.zeros(0, np.uint64))
                continue
            d = gr.d2_row(xyz, i) if d2 is None else d2[i]
            j = np.nonzero(ok & (me != i) & (d <= r2))[0]                 # (a comparison with NaN is false)
            out.append(np.sort(gr.keys(d[j], j)))
    return csr(out, len(out))


def counts_c(xyz, radius, d2=None):
    """The filter's c_i: n_i + 1 for a finite i, 0 otherwise."""
    got = radius_rows(xyz, radius, d2=d2)
    return np.where(gr.finite(np.ascontiguousarray(xyz, F32)), got["count"] + 1, 0).astype(np.int32)


def walk_radius(xyz, radius, cell=0.0, budget=None, d2=None):
    """The search as the kernels run it -> (result dict, stats).  cell = 0 takes the radius for the edge.  stats: the (query,
    ring) stops taken, at how many of them an unseen hit existed (must be 0), the grid, the candidates looked at, the walks
    that stopped before the grid's end."""
    xyz = np.ascontiguousarray(xyz, F32)
    N = xyz.shape[1]
    ok = gr.finite(xyz)
    r2 = r2_of(radius)
    lo, h, n = gr.make_grid(xyz, cell if cell > 0 else F32(radius), budget)
    face = [gr.faces(lo[c], h, n[c]) for c in range(3)]
    assert all((np.diff(f) >= 0).all() for f in face)                  # monotone
    cell_c = np.zeros((3, N), np.int64)
    for c in range(3):
        cell_c[c, ok] = gr.cells_of(xyz[c, ok], face[c], n[c])
    stats = dict(checks=0, violations=0, n=tuple(n), h=float(h), looked=0, stopped_early=0)
    me = np.arange(N)
    inf = F32(np.inf)
    out = []
    with np.errstate(all="ignore"):
        for i in range(N):
            got = np.zeros(0, np.uint64)
            if ok[i]:
                q = cell_c[:, i]
                cheb = np.abs(cell_c - q[:, None]).max(0)
                d = gr.d2_row(xyz, i) if d2 is None else d2[i]
                cand = ok & (me != i)
                hit = cand & (d <= r2)
                rmax = int(max(max(q[c], n[c] - 1 - q[c]) for c in range(3)))
                for r in range(rmax + 1):
                    ring = cheb == r
                    stats["looked"] += int((cand & ring).sum())
                    j = np.nonzero(hit & ring)[0]
                    got = np.concatenate([got, gr.keys(d[j], j)])
                    bound = inf
                    for c in range(3):
                        if q[c] + r + 1 <= n[c] - 1:
                            g = F32(face[c][q[c] + r + 1] - xyz[c, i])
                            bound = min(bound, F32(g * g))
                        if q[c] - r >= 1:
                            g = F32(xyz[c, i] - face[c][q[c] - r])
                            bound = min(bound, F32(g * g))
                    stats["checks"] += 1
                    if bound > r2:                                     # STRICTLY above: a point at exactly r2 is a hit
                        if (hit & (cheb > r)).any():
                            stats["violations"] += 1
                        stats["stopped_early"] += r < rmax
                        break
            out.append(np.sort(got))
    return csr(out, N), stats


def same(a, b):
    """Two result dicts, bit for bit."""
    return a["total"] == b["total"] and all(np.array_equal(a[k], b[k]) for k in ("count", "row_start", "idx", "bits"))


def padded(res, capacity):
    """What the call writes for `capacity` slots: (idx int32 [capacity], d2 bits int32 [capacity]) -- the rows and -1 / +inf
    behind them where the cloud fits, -1 / +inf everywhere where it does not."""
    idx = np.full(capacity, -1, np.int32)
    bits = np.full(capacity, INF_BITS, np.int32)
    if res["total"] <= capacity:
        idx[:res["total"]], bits[:res["total"]] = res["idx"], res["bits"]
    return idx, bits


def cut(res, m):
    """The hybrid question: every row's first min(n_i, m) entries, as a result dict of its own."""
    N = len(res["count"])
    keep = np.concatenate([np.arange(res["row_start"][i], res["row_start"][i] + min(int(res["count"][i]), m)) for i in range(N)]
                          + [np.zeros(0, np.int64)]).astype(np.int64)
    count = np.minimum(res["count"], m).astype(np.int32)
    row_start = np.zeros(N + 1, np.int64)
    np.cumsum(count, out=row_start[1:])
    return {"count": count, "row_start": row_start, "total": int(row_start[N]), "idx": res["idx"][keep], "bits": res["bits"][keep]}


def spanning_radius(xyz):
    """A radius above the cloud's extent: every finite point is in every finite point's row."""
    xyz = np.ascontiguousarray(xyz, F32)
    ok = gr.finite(xyz)
    ext = float((xyz[:, ok].max(1) - xyz[:, ok].min(1)).max()) if ok.any() else 0.0
    return float(F32(2.0 * ext + 1.0))


def radius_with_longest_row(xyz, longest, d2=None):
    """(radius, the result there): a radius at which the LONGEST row of the cloud has exactly `longest` entries, chosen from the
    definition's distances and checked on its rows; None if the cloud has no such radius."""
    xyz = np.ascontiguousarray(xyz, F32)
    d2 = d2_all(xyz) if d2 is None else d2
    N = xyz.shape[1]
    srt = np.sort(np.where(np.eye(N, dtype=bool), np.inf, d2.astype(np.float64)), axis=1)
    # the longest row has >= L entries iff r2 >= min_i srt[i, L - 1]; it has > L entries iff r2 >= min_i srt[i, L]
    lo, hi = srt[:, longest - 1].min(), srt[:, longest].min()
    if not lo < hi:
        return None
    radius = float(F32(np.sqrt(0.5 * (lo + hi))))
    res = radius_rows(xyz, radius, d2=d2)
    return (radius, res) if int(res["count"].max()) == longest else None
