"""include/vcr_hip_grid.h restated in numpy: the DEFINITION of the grid kNN's result as a brute-force loop (``knn``), the walk
that finds it (``walk``: faces, cells by comparison, Chebyshev rings, the fp32 bound, the strict stop) and the recipes of the
clouds the tests run.  Everything is fp32 arithmetic spelled out: numpy's float32 subtraction and product round once, and
``fmaf32`` is an exact fused multiply-add (tests/test_grid_cpu.py holds it to a fractions.Fraction one).

One cloud is a float32 array [3, N]."""
import numpy as np

INF_BITS = 0x7F800000
MAX_K = 62


def cells_budget(N):
    """VCR_GRID_CELLS(N)."""
    return 2 * int(N) + 64


def fmaf32(a, b, c):
    """fl32(a * b + c), one rounding, for float32 arrays: the product of two float32 is exact in fp64, the fp64 sum's rounding
    error is recovered exactly (two-sum) and the sum is moved to the ODD neighbour when it is inexact, so the closing rounding to
    fp32 sees which side of every fp32 tie the exact value lies on."""
    a, b, c = (np.asarray(v, np.float32).astype(np.float64) for v in (a, b, c))
    with np.errstate(all="ignore"):
        p = a * b
        s = np.atleast_1d(p + c).copy()
        p, c = np.broadcast_to(p, s.shape), np.broadcast_to(c, s.shape)
        bb = s - p
        err = (p - (s - bb)) + (c - bb)
        fix = np.isfinite(s) & np.isfinite(err) & (err != 0) & ((s.view(np.int64) & 1) == 0)
        s[fix] = np.nextafter(s[fix], np.where(err[fix] > 0, np.inf, -np.inf))
        out = s.astype(np.float32)
    return out.reshape(np.broadcast(a, b, c).shape)


def finite(xyz):
    return np.isfinite(xyz).all(0)


def d2_row(xyz, i):
    """The definition's d2 of query i against every point, float32 [N]: differences, then fmaf(dz, dz, fmaf(dy, dy, dx * dx))."""
    with np.errstate(all="ignore"):
        dx, dy, dz = (xyz[c] - xyz[c, i] for c in range(3))
        return fmaf32(dz, dz, fmaf32(dy, dy, dx * dx))


def keys(d2, j):
    """(d2, j) as one uint64 that orders like the pair: d2 >= +0, so its bits order like its value."""
    return d2.astype(np.float32).view(np.uint32).astype(np.uint64) << np.uint64(32) | j.astype(np.uint64)


def candidates(xyz, i, ok):
    """Query i's candidates as ascending keys: the finite points j != i whose d2 is not +inf; none for a query that is not finite."""
    if not ok[i]:
        return np.zeros(0, np.uint64)
    d2 = d2_row(xyz, i)
    take = ok & (np.arange(xyz.shape[1]) != i) & (d2.view(np.uint32) < INF_BITS)
    j = np.nonzero(take)[0]
    return np.sort(keys(d2[j], j))


def row(sorted_keys, i, k):
    """The first k keys as (idx [k], d2 bits [k]): the query's own index and +inf where the row is short."""
    full = np.full(k, np.uint64(INF_BITS) << np.uint64(32) | np.uint64(i), np.uint64)
    m = min(k, len(sorted_keys))
    full[:m] = sorted_keys[:m]
    return (full & np.uint64(0xFFFFFFFF)).astype(np.int32), (full >> np.uint64(32)).astype(np.uint32).view(np.int32)


def knn(xyz, k, rows=None):
    """THE DEFINITION.  -> (idx int32 [R,k], d2 bits int32 [R,k]) for the queries `rows` (all of them by default)."""
    xyz = np.ascontiguousarray(xyz, np.float32)
    ok = finite(xyz)
    rows = range(xyz.shape[1]) if rows is None else rows
    out = [row(candidates(xyz, int(i), ok), int(i), k) for i in rows]
    return np.stack([o[0] for o in out]), np.stack([o[1] for o in out])


# ---------------------------------------------------------------------------------------------------------------- the walk

def make_grid(xyz, cell=0.0, budget=None):
    """The header's grid of one cloud: (lo float32 [3], h float32, n int [3])."""
    N = xyz.shape[1]
    budget = cells_budget(N) if budget is None else budget
    ok = finite(xyz)
    f32 = np.float32
    fmax, fmin = np.finfo(f32).max, np.finfo(f32).tiny
    with np.errstate(all="ignore"):
        lo = xyz[:, ok].min(1) if ok.any() else np.zeros(3, f32)
        hi = xyz[:, ok].max(1) if ok.any() else np.zeros(3, f32)
        e = np.minimum(hi - lo, fmax).astype(f32)
        h = f32(cell)
        if not h > 0:
            live = e[e > 0].astype(np.float64)
            h = f32(1.0) if len(live) == 0 else f32((np.prod(live) / N) ** (1.0 / len(live)))
        h = f32(min(max(h, fmin), fmax))
        n = [1, 1, 1]
        for _ in range(1024):
            q = e / h
            n = [int(v) + 1 if v < 1048575.0 else 1 << 20 for v in q]
            if n[0] * n[1] * n[2] <= budget:
                break
            n = [1, 1, 1]
            h = f32(min(h * f32(1.25), fmax))
    return lo.astype(f32), h, n


def faces(lo_c, h, n_c):
    """face[j] = fmaf((float)j, h, lo_c) for j = 0 ... n_c."""
    return fmaf32(np.arange(n_c + 1, dtype=np.float32), np.float32(h), np.float32(lo_c))


def cells_of(x, face, n_c):
    """By comparison: the largest j in [0, n_c) with face[j] <= x (the last cell is open above)."""
    return np.clip(np.searchsorted(face[:n_c], x, side="right") - 1, 0, n_c - 1)


def walk(xyz, k, cell=0.0, budget=None, check=True):
    """The search as the kernels run it -> (idx, d2 bits, stats).  stats: the (query, ring) bounds taken, how many of them an
    unseen candidate undercut (the prune rule's violations: must be 0), the grid, the candidates looked at."""
    xyz = np.ascontiguousarray(xyz, np.float32)
    N = xyz.shape[1]
    ok = finite(xyz)
    lo, h, n = make_grid(xyz, cell, budget)
    face = [faces(lo[c], h, n[c]) for c in range(3)]
    assert all((np.diff(f) >= 0).all() for f in face)                  # monotone
    cell_c = np.zeros((3, N), np.int64)
    for c in range(3):
        cell_c[c, ok] = cells_of(xyz[c, ok], face[c], n[c])
    stats = dict(checks=0, violations=0, n=tuple(n), h=float(h), looked=0, stopped_early=0)
    idx, bits = np.zeros((N, k), np.int32), np.zeros((N, k), np.int32)
    me = np.arange(N)
    inf = np.float32(np.inf)
    for i in range(N):
        got = np.zeros(0, np.uint64)
        if ok[i]:
            q = cell_c[:, i]
            cheb = np.abs(cell_c - q[:, None]).max(0)
            d2 = d2_row(xyz, i)
            cand = ok & (me != i) & (d2.view(np.uint32) < INF_BITS)
            rmax = int(max(max(q[c], n[c] - 1 - q[c]) for c in range(3)))
            for r in range(rmax + 1):
                j = np.nonzero(cand & (cheb == r))[0]
                stats["looked"] += len(j)
                got = np.sort(np.concatenate([got, keys(d2[j], j)]))[:k]
                bound = inf
                with np.errstate(all="ignore"):
                    for c in range(3):
                        if q[c] + r + 1 <= n[c] - 1:
                            g = np.float32(face[c][q[c] + r + 1] - xyz[c, i])
                            bound = min(bound, np.float32(g * g))
                        if q[c] - r >= 1:
                            g = np.float32(xyz[c, i] - face[c][q[c] - r])
                            bound = min(bound, np.float32(g * g))
                stats["checks"] += 1
                if check:
                    unseen = cand & (cheb > r)
                    if unseen.any() and d2[unseen].min() < bound:
                        stats["violations"] += 1
                kth = np.uint32(got[k - 1] >> np.uint64(32)).view(np.float32) if len(got) == k else inf
                if kth < bound:                                        # STRICTLY below
                    stats["stopped_early"] += r < rmax
                    break
        idx[i], bits[i] = row(got, i, k)
    return idx, bits, stats


# ------------------------------------------------------------------------------------------------------------- the recipes

def random_cloud(N, seed=0):
    return np.random.RandomState(seed).uniform(0, 1, (3, N)).astype(np.float32)


def lattice(N, seed=0):
    """N points of an integer lattice (shuffled): every point ON a face of a grid of edge 1 or 2, exact ties everywhere."""
    m = int(np.ceil(N ** (1 / 3)))
    g = np.stack(np.meshgrid(np.arange(m), np.arange(m), np.arange(m), indexing="ij")).reshape(3, -1)
    pick = np.random.RandomState(seed).permutation(g.shape[1])[:N]
    return g[:, pick].astype(np.float32)


def flat(N, seed=0):
    x = random_cloud(N, seed)
    x[2] = 0.5
    return x


def collinear(N, seed=0):
    x = random_cloud(N, seed)
    x[1], x[2] = 0.25, -0.75
    return x


def equal(N, seed=0):
    return np.tile(np.asarray([[0.3], [0.4], [0.5]], np.float32), (1, N))


def copies(N, seed=0):
    """Every point three times (the last group may be shorter), shuffled."""
    base = random_cloud((N + 2) // 3, seed)
    x = np.concatenate([base, base, base], 1)[:, :N]
    return x[:, np.random.RandomState(seed + 1).permutation(N)]


def nonfinite(N, seed=0):
    """NaN at point 0, +inf, -inf and NaN elsewhere."""
    x = random_cloud(N, seed)
    x[0, 0] = np.nan
    if N > 7:
        x[1, 5], x[2, N // 2], x[0, N - 1] = np.inf, -np.inf, np.nan
        x[:, 7] = np.nan
    return x


def nonfinite_late(N, seed=0):
    """Point 0 finite; NaN and inf elsewhere."""
    x = random_cloud(N, seed)
    x[2, 1], x[0, N - 1] = np.nan, np.inf
    return x


def outlier(N, seed=0):
    """One point far away: the automatic grid puts nearly every other point into one cell."""
    x = random_cloud(N, seed)
    x[:, N // 3] = 1.0e4
    return x


def tiny(N, seed=0):
    return (random_cloud(N, seed) * np.float32(1e-3)).astype(np.float32)


def clustered(N, seed=0):
    rs = np.random.RandomState(seed)
    centres = rs.uniform(0, 1, (3, 8))
    return (centres[:, rs.randint(0, 8, N)] + rs.normal(size=(3, N)) * 0.01).astype(np.float32)


def sphere(N, seed=0):
    v = np.random.RandomState(seed).normal(size=(3, N))
    return (v / np.linalg.norm(v, axis=0)).astype(np.float32)


RECIPES = {"random": random_cloud, "lattice": lattice, "flat": flat, "collinear": collinear, "equal": equal, "copies": copies,
           "nonfinite": nonfinite, "nonfinite_late": nonfinite_late, "outlier": outlier, "tiny": tiny, "clustered": clustered}


def moved(xyz, offset):
    """The cloud with `offset` added in fp32 (rounded: a new cloud, not the same one seen from elsewhere)."""
    return (xyz + np.float32(offset)).astype(np.float32)


def forced_cells(xyz):
    """Edges from "every point its own cell" (far below the spacing: widened to the budget) to "one cell", and the lattice's
    own 1 and 2 (points ON the faces)."""
    ok = finite(xyz)
    ext = float((xyz[:, ok].max(1) - xyz[:, ok].min(1)).max()) if ok.any() else 0.0
    ext = ext if ext > 0 and np.isfinite(ext) else 1.0
    return [1e-4 * ext, 0.03 * ext, 0.11 * ext, 0.37 * ext, 1.0, 2.0, 3.0 * ext]
