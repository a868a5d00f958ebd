"""include/cluster/vcr_hip_dbscan.h restated in numpy: what the tests compare the DBSCAN kernels with.

One cloud's neighbourhoods are rows (idx int [total or more], row_start int64 [N + 1]) -- what radius_restated.radius_rows
returns, or any caller's.  An entry outside [0, N) or equal to its row's index is ignored; L_i counts the others.
  core       L_i + 1 >= min_points, and the point is finite where `finite` is given
  clusters   connected components of the core points under "j is in row i or i is in row j", numbered by lowest index
  border     a finite point that is not core: the lowest label among the core entries of ITS OWN row, -1 without one
``sequential`` is THE DEFINITION: the textbook loop -- seeds in index order, a cluster expanded fully from a stack before the
next seed is looked at, a point labelled by the first cluster that reaches it -- on the lists made symmetric (on symmetric
rows, such as a radius search's, that changes nothing: it is Open3D's and scikit-learn's loop).  ``vectorised`` is the order-free
statement for large N: min-label propagation over the core edges with pointer jumping, to a fixed point.  The two must agree.

A result is a dict of labels int32 [N], core int32 [N], n_clusters (int) and sizes int32 [N] (slot c: the members of cluster c)."""
import numpy as np

import grid_restated as gr
import radius_restated as rr

F32 = np.float32
I32 = np.int32
NOISE, NOT_SERVED = -1, -2


def entries(idx, row_start, N):
    """-> (src int64 [E], dst int64 [E]): every entry that is not ignored, as the pair (its row, the index it holds)."""
    row_start = np.asarray(row_start, np.int64)
    idx = np.asarray(idx).astype(np.int64)[:int(row_start[N])]
    src = np.repeat(np.arange(N, dtype=np.int64), np.diff(row_start))
    keep = (idx >= 0) & (idx < N) & (idx != src)
    return src[keep], idx[keep]


def core_points(idx, row_start, N, min_points, finite=None):
    src, _ = entries(idx, row_start, N)
    L = np.bincount(src, minlength=N)
    core = L + 1 >= min_points
    return core if finite is None else core & np.asarray(finite, bool)


def _result(labels, core, N):
    labels = labels.astype(I32)
    n = int(labels.max()) + 1 if N and labels.max() >= 0 else 0
    sizes = np.zeros(N, I32)
    sizes[:n] = np.bincount(labels[labels >= 0], minlength=n)[:n]
    return {"labels": labels, "core": core.astype(I32), "n_clusters": n, "sizes": sizes}


def sequential(idx, row_start, N, min_points, finite=None):
    """THE DEFINITION."""
    fin = np.ones(N, bool) if finite is None else np.asarray(finite, bool)
    core = core_points(idx, row_start, N, min_points, finite)
    src, dst = entries(idx, row_start, N)
    # the lists made symmetric: a core point reaches the core points of its row and those whose row holds it; and it reaches a
    # point that is not core when THAT point's row holds it
    reach = [[] for _ in range(N)]
    for s, d in zip(src.tolist(), dst.tolist()):
        if core[s] and core[d]:
            reach[s].append(d)
            reach[d].append(s)
        elif core[d] and fin[s]:                            # s is not core: its own row names the core point d
            reach[d].append(s)
    labels = [NOISE] * N
    c = 0
    for seed in range(N):
        if not core[seed] or labels[seed] != NOISE:
            continue
        labels[seed] = c
        stack = [seed]
        while stack:
            p = stack.pop()
            for q in reach[p]:
                if labels[q] == NOISE:
                    labels[q] = c
                    if core[q]:
                        stack.append(q)
        c += 1
    return _result(np.asarray(labels, np.int64).reshape(N), core, N)


def vectorised(idx, row_start, N, min_points, finite=None):
    """The order-free statement: the lowest index of every core point's component by min-label propagation and pointer
    jumping, the rank of those lowest indices, the border minimum."""
    fin = np.ones(N, bool) if finite is None else np.asarray(finite, bool)
    core = core_points(idx, row_start, N, min_points, finite)
    src, dst = entries(idx, row_start, N)
    both = core[src] & core[dst]
    a, b = src[both], dst[both]
    low = np.arange(N, dtype=np.int64)
    while True:
        was = low.copy()
        m = np.minimum(low[a], low[b])
        np.minimum.at(low, a, m)
        np.minimum.at(low, b, m)
        while True:                                         # pointer jumping
            nxt = low[low]
            if np.array_equal(nxt, low):
                break
            low = nxt
        if np.array_equal(low, was):
            break
    roots = np.flatnonzero(core & (low == np.arange(N)))
    rank = np.full(N, -1, np.int64)
    rank[roots] = np.arange(len(roots))
    labels = np.where(core, rank[low], NOISE)
    border = ~core[src] & fin[src] & core[dst]
    best = np.full(N, np.iinfo(np.int64).max)
    np.minimum.at(best, src[border], labels[dst[border]])
    labels = np.where(~core & (best != np.iinfo(np.int64).max), best, labels)
    return _result(labels, core, N)


def not_served(N):
    return {"labels": np.full(N, NOT_SERVED, I32), "core": np.zeros(N, I32), "n_clusters": -1, "sizes": np.zeros(N, I32)}


def served(row_start, total, capacity):
    row_start = np.asarray(row_start, np.int64)
    return bool(0 <= total <= capacity and row_start[0] == 0 and row_start[-1] == total and (np.diff(row_start) >= 0).all())


def same(a, b):
    return a["n_clusters"] == b["n_clusters"] and all(np.array_equal(a[k], b[k]) for k in ("labels", "core", "sizes"))


def of_cloud(x, radius, min_points, form=sequential, d2=None):
    """A cloud [3,N] through the definition's radius rows -> (result, the rows)."""
    x = np.ascontiguousarray(x, F32)
    rows = rr.radius_rows(x, radius, d2=d2)
    return form(rows["idx"], rows["row_start"], x.shape[1], min_points, gr.finite(x)), rows


def contested(idx, row_start, N, res):
    """The border points whose rows hold core points of two clusters."""
    src, dst = entries(idx, row_start, N)
    core = res["core"].astype(bool)
    m = ~core[src] & core[dst] & (res["labels"][src] >= 0)
    lo = np.full(N, np.iinfo(np.int64).max)
    hi = np.full(N, -1)
    np.minimum.at(lo, src[m], res["labels"][dst[m]])
    np.maximum.at(hi, src[m], res["labels"][dst[m]])
    return np.flatnonzero((hi >= 0) & (lo != hi))


def largest(x, res):
    """largest_cluster for one cloud -> (points [3,N] with NaN behind the kept, count, index [N] with -1 behind them)."""
    N = x.shape[1]
    keep = np.zeros(N, bool)
    if res["sizes"].max(initial=0) > 0:
        keep = res["labels"] == int(np.argmax(res["sizes"]))         # (argmax: the first among equals)
    at = np.flatnonzero(keep)
    points = np.full((3, N), np.nan, F32)
    points[:, :len(at)] = x[:, at]
    index = np.full(N, -1, I32)
    index[:len(at)] = at
    return points, len(at), index


# ---------------------------------------------------------------------------------------------------------------- the recipes

HAND_EPS = 1.0
HAND_MIN_POINTS = 4


def hand_cloud():
    """Twelve points on the x axis, eps = 1, min_points = 4 (a point and three others), every distance exact.
      2, 3 (copies at 0), 4 (0.5), 6 (1)   core: cluster 0, whose lowest core index is 2
      5 (3), 8, 9 (copies at 3.5), 10 (4)  core: cluster 1, whose lowest core index is 5 ...
      0 (5)                                ... and whose lowest MEMBER is the border point 0: only 10 is within its reach
      7 (2)                                border, exactly 1 from the core points 6 (cluster 0) and 5 (cluster 1): its row lists 5
                                           first, and it takes the lower label, 0
      1 (20)                               noise
      11 (NaN)                             not finite: -1 whatever min_points is
    Both clusters have five members: largest_cluster must take cluster 0."""
    xs = [5.0, 20.0, 0.0, 0.0, 0.5, 3.0, 1.0, 2.0, 3.5, 3.5, 4.0, np.nan]
    x = np.zeros((3, len(xs)), F32)
    x[0] = xs
    return x


HAND_WANT = {4: dict(labels=[1, -1, 0, 0, 0, 1, 0, 0, 1, 1, 1, -1], core=[0, 0, 1, 1, 1, 1, 1, 0, 1, 1, 1, 0], n_clusters=2,
                     sizes=[5, 5]),
             # every finite point is core: the chain 2 ... 10, 0 is one component (lowest index 0), 1 stands alone
             1: dict(labels=[0, 1, 0, 0, 0, 0, 0, 0, 0, 0, 0, -1], core=[1] * 11 + [0], n_clusters=2, sizes=[10, 1]),
             13: dict(labels=[-1] * 12, core=[0] * 12, n_clusters=0, sizes=[])}


def path(n=4096, cuts=(), seed=11):
    """n points spaced 1 apart on a line, eps = 1, min_points = 2, their indices scrambled by a fixed permutation: the
    union-find's worst case, one component as long as the cloud.  cuts: positions behind which the next point lies 2 further,
    so the line falls into len(cuts) + 1 clusters.  -> (x [3,n], perm: position p on the line is index perm[p])."""
    perm = np.random.RandomState(seed).permutation(n)
    pos = np.arange(n, dtype=np.float64)
    for c in cuts:
        pos[c + 1:] += 2.0
    x = np.zeros((3, n), F32)
    x[0, perm] = pos
    return x, perm


PATH_CUTS = (300, 911, 1500, 2047, 2050, 3000, 4000)       # (a piece of three points among them; none of one: that is noise)
SHORT_PATH_CUTS = (20, 57, 93, 127, 130, 187, 250)         # the same on a path of 256


def path_want(n, perm, cuts=()):
    """The labels the path must get: its pieces numbered by their lowest index."""
    piece = np.zeros(n, np.int64)
    for c in cuts:
        piece[c + 1:] += 1
    lowest = np.full(len(cuts) + 1, n)
    np.minimum.at(lowest, piece, perm)
    rank = np.argsort(np.argsort(lowest))
    labels = np.zeros(n, I32)
    labels[perm] = rank[piece]
    return labels


def blobs(N, k=8, seed=0, spread=0.05, extent=2.0):
    """k Gaussian blobs in a cube and 5 % uniform clutter, spread among them in index."""
    rs = np.random.RandomState(seed)
    centres = rs.uniform(-extent, extent, (k, 3))
    x = centres[rs.randint(0, k, N)] + rs.normal(0, spread, (N, 3))
    far = rs.permutation(N)[:N // 20]
    x[far] = rs.uniform(-extent, extent, (len(far), 3))
    return np.ascontiguousarray(x.T, F32)


def uniform(N, seed=0, extent=2.0):
    return np.random.RandomState(seed).uniform(-extent / 2, extent / 2, (3, N)).astype(F32)
