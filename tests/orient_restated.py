"""CPU restatement of include/orient/vcr_hip_orient.h in numpy -- what the tests compare the kernels with
-- and the input recipes the CPU and GPU tests share.  Two restatements of one definition:

  * `definition`: the header read literally.  The graph's edges once each, their fp32 weights (match_restated.fma32 is an exact
    fmaf) and packed 64-bit keys, Kruskal's algorithm on the SORTED keys, then a walk from every tree's reference point that
    counts the reversing edges.
  * `boruvka`: the device's rounds.  Every tree takes the least key that leaves it, of two trees that chose the same edge the
    lower root stays, every other root hooks under the other tree's, and every vertex is pointed at its new root with its parity.

Both return a dict: flip int32 [N], ref int32 [N], n_trees int, oriented fp32 [3,N] (the sign bits inverted where flip is 1),
tree (the forest's keys, sorted uint64), weight (their w summed in float64)."""
import numpy as np

import fpfh_restated as fr
import match_restated as mr

F32 = np.float32
U64 = np.uint64
MAX_N = 131072
NONE = np.iinfo(np.uint64).max


# ------------------------------------------------------------------------------------------------------------------- the edges

def dot(nrm, i, j):
    """d of the header for the pairs (i, j): fmaf(nz_i, nz_j, fmaf(ny_i, ny_j, nx_i * nx_j)) in fp32."""
    n = np.asarray(nrm, F32)
    with np.errstate(all="ignore"):
        return mr.fma32(n[2, i], n[2, j], mr.fma32(n[1, i], n[1, j], n[0, i] * n[0, j]))


def weight(d):
    """d fp32 -> (w fp32 in [0, 1], reverses bool)."""
    d = np.asarray(d, F32)
    fin = np.isfinite(d)
    with np.errstate(all="ignore"):
        x = F32(1) - np.abs(d)
        w = np.where(fin, np.where(x > 0, x, F32(0)), F32(1)).astype(F32)
        return w, fin & (d < 0)


def pack(w, lo, hi):
    """(bits of w) << 34 | lo << 17 | hi as uint64."""
    bits = np.ascontiguousarray(w, F32).view(np.uint32).astype(U64)
    return (bits << U64(34)) | (np.asarray(lo).astype(U64) << U64(17)) | np.asarray(hi).astype(U64)


def edges(nrm, idx):
    """nrm [3,N] fp32, idx int [N,k] -> dict of the graph's edges, each once, ascending in (lo, hi): lo, hi int64 [E], d, w fp32
    [E], rev bool [E], key uint64 [E]."""
    idx = np.asarray(idx).astype(np.int64)
    N, k = idx.shape
    i = np.repeat(np.arange(N), k)
    j = idx.reshape(-1)
    ok = (j >= 0) & (j < N) & (j != i)
    i, j = i[ok], j[ok]
    pair = np.unique(np.minimum(i, j) * N + np.maximum(i, j))
    lo, hi = pair // N, pair % N
    d = np.asarray(dot(nrm, lo, hi), F32).reshape(-1)
    w, rev = weight(d)
    return {"lo": lo, "hi": hi, "d": d, "w": w, "rev": rev, "key": pack(w, lo, hi)}


# ------------------------------------------------------------------------------------------------------------------- the tails

def zrank(z):
    """z fp32 [N] -> float64 that orders as the header's reference rule: -inf for a z that is not finite, -0.0 as 0.0."""
    z = np.asarray(z, F32).astype(np.float64)
    return np.where(np.isfinite(z), z + 0.0, -np.inf)


def references(z, comp):
    """comp int [N] (any label per tree) -> ref int64 [N]: per tree the member with the largest z, the lowest index among
    equals."""
    N = len(comp)
    order = np.lexsort((np.arange(N), -zrank(z), comp))     # by tree, then z descending, then index ascending
    c = np.asarray(comp)[order]
    first = np.r_[True, c[1:] != c[:-1]]
    top = {int(t): int(v) for t, v in zip(c[first], order[first])}
    return np.asarray([top[int(t)] for t in comp], np.int64)


def finish(xyz, nrm, ref, parity, n_trees, tree, w):
    """parity [N]: the reversing edges between v and ITS REFERENCE, mod 2."""
    nrm = np.ascontiguousarray(nrm, F32)
    with np.errstate(invalid="ignore"):
        flip = (np.asarray(parity, np.int64) ^ (nrm[2, ref] < 0)).astype(np.uint32)
    oriented = (nrm.view(np.uint32) ^ (flip[None, :] << np.uint32(31))).view(F32)
    tree = np.sort(np.asarray(tree, U64))
    return {"flip": flip.astype(np.int32), "ref": ref.astype(np.int32), "n_trees": int(n_trees), "oriented": oriented,
            "tree": tree, "weight": float(np.asarray(w, np.float64).sum())}


# -------------------------------------------------------------------------------------------------------------- the definition

def definition(xyz, nrm, idx):
    """One cloud: xyz, nrm [3,N] fp32, idx int [N,k]."""
    N = np.asarray(idx).shape[0]
    e = edges(nrm, idx)
    order = np.argsort(e["key"], kind="stable")             # (the keys are distinct)
    parent = list(range(N))

    def find(x):
        while parent[x] != x:
            parent[x] = parent[parent[x]]
            x = parent[x]
        return x
    adj = [[] for _ in range(N)]
    kept = []
    lo, hi, rev = e["lo"].tolist(), e["hi"].tolist(), e["rev"].tolist()
    for t in order.tolist():
        a, b = find(lo[t]), find(hi[t])
        if a != b:
            parent[a] = b
            adj[lo[t]].append((hi[t], rev[t]))
            adj[hi[t]].append((lo[t], rev[t]))
            kept.append(t)
    comp = np.asarray([find(v) for v in range(N)])
    ref = references(np.asarray(xyz, F32)[2], comp)
    parity = np.full(N, -1, np.int64)
    for r in np.unique(ref).tolist():                       # the walk from every reference
        parity[r] = 0
        stack = [r]
        while stack:
            v = stack.pop()
            for u, rv in adj[v]:
                if parity[u] < 0:
                    parity[u] = parity[v] ^ int(rv)
                    stack.append(u)
    assert (parity >= 0).all()
    kept = np.asarray(kept, np.int64)
    return finish(xyz, nrm, ref, parity, N - len(kept), e["key"][kept], e["w"][kept])


# ------------------------------------------------------------------------------------------------------------------ the rounds

def boruvka(xyz, nrm, idx, want_rounds=False):
    """One cloud by the device's rounds; want_rounds: also the number of rounds that hooked."""
    N = np.asarray(idx).shape[0]
    e = edges(nrm, idx)
    by_key = np.argsort(e["key"], kind="stable")
    sorted_keys = e["key"][by_key]
    root, par = np.arange(N), np.zeros(N, np.int64)         # every vertex AT its root, with its parity towards it
    chosen, rounds = [], 0
    while True:
        ra, rb = root[e["lo"]], root[e["hi"]]
        out = ra != rb
        if not out.any():
            break
        best = np.full(N, NONE, U64)
        np.minimum.at(best, ra[out], e["key"][out])         # both trees see the edge, whichever row listed it
        np.minimum.at(best, rb[out], e["key"][out])
        R = np.nonzero(best != NONE)[0]
        assert (root[R] == R).all()
        t = by_key[np.searchsorted(sorted_keys, best[R])]   # the chosen edges
        a, c = e["lo"][t], e["hi"][t]
        other = np.where(root[a] == R, root[c], root[a])
        assert ((root[a] == R) ^ (root[c] == R)).all()
        stay = (best[other] == best[R]) & (R < other)       # both chose this edge: the lower root stays
        up, upp = np.arange(N), np.zeros(N, np.int64)
        up[R[~stay]] = other[~stay]
        upp[R[~stay]] = (par[a] ^ par[c] ^ e["rev"][t])[~stay]
        chosen.append(t)
        while True:                                         # pointer doubling to the new roots
            g = up[up]
            if (g == up).all():
                break
            up, upp = g, upp ^ upp[up]
        root, par = up[root], par ^ upp[root]
        rounds += 1
        assert rounds <= max(1, int(np.ceil(np.log2(max(N, 2)))))
    kept = np.unique(np.concatenate(chosen)) if chosen else np.zeros(0, np.int64)
    ref = references(np.asarray(xyz, F32)[2], root)
    res = finish(xyz, nrm, ref, par ^ par[ref], len(np.unique(root)), e["key"][kept], e["w"][kept])
    return (res, rounds) if want_rounds else res


def same(a, b):
    return (np.array_equal(a["flip"], b["flip"]) and np.array_equal(a["ref"], b["ref"]) and a["n_trees"] == b["n_trees"]
            and np.array_equal(a["oriented"].view(np.uint32), b["oriented"].view(np.uint32)) and np.array_equal(a["tree"], b["tree"]))


# ----------------------------------------------------------------------------------------------------------------- the recipes

def torus(N, seed=0):
    """(x [3,N] fp32, outward float64 [3,N]): uniform angles on a torus of radii 1 and 0.4."""
    rs = np.random.RandomState(4000 + seed + N)
    u, v = rs.uniform(0, 2 * np.pi, N), rs.uniform(0, 2 * np.pi, N)
    x = np.stack([(1 + 0.4 * np.cos(v)) * np.cos(u), (1 + 0.4 * np.cos(v)) * np.sin(u), 0.4 * np.sin(v)])
    return x.astype(F32), np.stack([np.cos(v) * np.cos(u), np.cos(v) * np.sin(u), np.sin(v)])


def sphere(N, seed=0):
    """(x [3,N] fp32, outward float64 [3,N]): uniform on the unit sphere."""
    rs = np.random.RandomState(5000 + seed + N)
    p = rs.normal(size=(3, N))
    p /= np.linalg.norm(p, axis=0)
    return p.astype(F32), p


def estimated(x, k):
    """-> (normals [3,N] fp32 of arbitrary sign, idx int32 [N,k]): the CPU chain's neighbours and normals."""
    idx = fr.neighbours(x, k)
    return fr.normals(x, idx), idx


def outward_share(oriented, outward):
    return float(((np.asarray(oriented, np.float64) * outward).sum(0) > 0).mean())


def agreement(oriented, wanted):
    """The share of normals equal in sign to `wanted`, up to one global sign."""
    s = float(((np.asarray(oriented, np.float64) * np.asarray(wanted, np.float64)).sum(0) > 0).mean())
    return max(s, 1.0 - s)


def path(N, scrambled=False, seed=3):
    """All normals equal, so every weight ties at 0 and the order is (lo, hi) alone: (xyz, nrm [3,N] fp32, idx int32 [N,2]) of
    a path whose i-th point has the neighbours before and behind it -- in index order the worst case of the flatten (every
    vertex hooks under its predecessor in round one), or the same path with its points renumbered at random.  z ascends
    along the path: the reference is its last point."""
    pos = np.random.RandomState(seed + N).permutation(N) if scrambled else np.arange(N)      # pos[v]: v's place on the path
    at = np.empty(N, np.int64)
    at[pos] = np.arange(N)                                  # at[p]: the vertex at place p
    idx = np.full((N, 2), -1, np.int32)
    idx[at[1:], 0] = at[:-1]
    idx[at[:-1], 1] = at[1:]
    xyz = np.stack([pos, np.zeros(N), pos]).astype(F32)
    nrm = np.tile(np.asarray([[0.6], [0.0], [-0.8]], F32), (1, N))
    return xyz, nrm, idx


def blobs(n_blobs, per=40, k=6, seed=0):
    """n_blobs well separated patches (x, estimated normals, idx): every row stays inside its blob, so there are n_blobs trees."""
    rs = np.random.RandomState(7000 + seed + n_blobs)
    xs, idxs = [], []
    for b in range(n_blobs):
        u, v = rs.uniform(0, 1, per), rs.uniform(0, 1, per)
        x = np.stack([u + 10.0 * b, v, 0.2 * np.sin(3 * u) * np.cos(2 * v) + 0.1 * b]).astype(F32)
        xs.append(x)
        idxs.append(fr.neighbours(x, k) + per * b)
    x, idx = np.concatenate(xs, axis=1), np.concatenate(idxs, axis=0).astype(np.int32)
    perm = rs.permutation(x.shape[1])                       # the blobs' members interleaved in index
    inv = np.empty_like(perm)
    inv[perm] = np.arange(len(perm))
    x, idx = x[:, perm], inv[idx[perm]].astype(np.int32)
    return x, fr.normals(x, idx), idx


def random_rows(N, k, seed=0):
    """Random normals of random length and random rows with self entries, out-of-range entries and duplicates: asymmetric."""
    rs = np.random.RandomState(8000 + seed + N + k)
    xyz = rs.uniform(-1, 1, (3, N)).astype(F32)
    nrm = rs.normal(size=(3, N)).astype(F32)
    idx = rs.randint(-2, N + 2, (N, k)).astype(np.int32)
    idx[::3, 0] = np.arange(N, dtype=np.int32)[::3]         # self entries
    if k > 1:
        idx[1::4, 1] = idx[1::4, 0]                         # duplicates
    return xyz, nrm, idx


def small_recipes():
    """name -> (xyz, nrm, idx) of the small cases both test files run: read-only."""
    out = {}
    out["one"] = (np.asarray([[1], [2], [3]], F32), np.asarray([[0], [0], [-1]], F32), np.asarray([[0]], np.int32))
    out["two"] = (np.asarray([[0, 1], [0, 0], [0, 0]], F32), np.asarray([[0, 0], [0, 0], [-1, 1]], F32), np.asarray([[1], [0]], np.int32))
    for N, k in ((65, 3), (300, 5)):
        out["rows-%d-%d" % (N, k)] = random_rows(N, k)
    x, _ = torus(65)
    out["torus-65-3"] = (x,) + estimated(x, 3)
    # an edge listed only by its far end: 0-1 and 2-3 by both, and 3 names 1 alone -- nothing in 0's or 1's row leaves their tree
    nrm = np.asarray([[0, 0, 0, 0], [0.1, -0.1, 0.2, 0.1], [1, 1, -1, 1]], F32)
    out["far-end"] = (np.asarray([[0, 1, 2, 3], [0, 0, 0, 0], [5, 1, 2, 3]], F32), nrm, np.asarray([[1, 1], [0, 0], [3, 3], [2, 1]], np.int32))
    # ... and must be SEEN by the tree that does not list it: a triangle with w(0,1) > w(1,2) > w(0,2), every edge listed by one
    # end.  A tree that took the least edge of its own rows alone would choose all three edges: a cycle
    ang = np.asarray([0.0, 0.5, 0.1])
    tri = np.stack([np.sin(ang), np.zeros(3), np.cos(ang)]).astype(F32)
    out["one-sided-triangle"] = (np.asarray([[0, 1, 2], [0, 0, 0], [0, 2, 1]], F32), tri, np.asarray([[1], [2], [0]], np.int32))
    out["path-64"] = path(64)
    out["path-257-scrambled"] = path(257, True)
    out["blobs-2"] = blobs(2)
    out["blobs-5"] = blobs(5)
    # equal z at the top: 7 points in a ring, the largest z at 5, 2 and 4 -- 2 is the reference
    ring = np.asarray([[(i + 1) % 7, (i - 1) % 7] for i in range(7)], np.int32)
    rx = np.asarray([[0, 1, 2, 3, 4, 5, 6], [0, 0, 0, 0, 0, 0, 0], [0, 1, 3, 2, 3, 3, -1]], F32)
    rn = np.random.RandomState(11).normal(size=(3, 7)).astype(F32)
    out["equal-top"] = (rx, rn, ring)
    zx = rx.copy()
    zx[2] = [0.0, -0.0, -1, -0.0, 0.0, -2, -3]              # -0.0 equals 0.0: the reference is 0
    out["signed-zero-top"] = (zx, rn, ring)
    # non-finite normals, a zero normal, non-finite z
    xyz, nrm, idx = random_rows(130, 4, seed=5)
    nrm[:, 7] = np.nan
    nrm[1, 19] = np.inf
    nrm[2, 33] = -np.inf
    nrm[:, 40] = 0
    nrm[:, 41] = [0.0, -0.0, -0.0]
    xyz[2, [3, 50]] = np.nan
    xyz[2, 90] = np.inf                                     # an infinite z ranks below every finite one too
    xyz[2, 91] = -np.inf
    out["nonfinite"] = (xyz, nrm, idx)
    # a tree whose every z is non-finite: the lowest index is its reference
    out["nonfinite-z-tree"] = (np.full((3, 5), np.nan, F32), np.random.RandomState(12).normal(size=(3, 5)).astype(F32),
                               np.asarray([[1], [2], [0], [4], [3]], np.int32))
    for v in out.values():
        for a in v:
            a.setflags(write=False)
    return out
