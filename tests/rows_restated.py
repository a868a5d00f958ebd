"""CPU restatement of include/ext/vcr_hip_rows.h in numpy -- what the tests compare the rows' kernels
with -- built per row on plane_restated and fpfh_restated.

One cloud is x float32 [3,N] with its rows as (idx int [total or more], row_start int64 [N+1]); max_nn = 0 takes whole rows.
`padded` lays the USED entries of every row into a rectangle and says which slots are used.  An unused slot holds the row's own
index i and is MASKED wherever it could count: never -1 as a stand-in for "nothing", because an entry outside [0, N) reads as i
and IS a neighbour by the header (a pair at distance 0: counted in the first pass, one more row in the normals' m).
  normals   plane_restated.covariances on the first L entries, one call per distinct L (m = L + 1 is the call's k + 1), then
            `jacobi_normal`: the device's cyclic Jacobi, sign rule and curvature operation by operation in IEEE doubles, so the
            comparison with the device is bit for bit.  plane_restated.normal (numpy's eigh) is what it is held to in turn.
  spfh      fpfh_restated.pairs on the rectangle, `counted` masked, the counts as the header's uint32 [3][12].
  fpfh      fpfh_restated.fpfh's chain on the wide counts.  An unused slot reads as i: d2 = 0, skipped -- the chain's own rule."""
import math

import numpy as np

import fpfh_restated as fr
import plane_restated as pr

F32 = np.float32
BINS = 11
SWEEPS = 16


def lengths(row_start, max_nn=0):
    n = np.diff(np.asarray(row_start, np.int64))
    return np.minimum(n, max_nn) if max_nn > 0 else n


def padded(idx, row_start, max_nn=0):
    """-> (j int64 [N,W], used bool [N,W], L int64 [N]): row i's first L_i entries AS THEY ARE, its own index behind them."""
    idx = np.asarray(idx).astype(np.int64)
    row_start = np.asarray(row_start, np.int64)
    L = lengths(row_start, max_nn)
    N, W = len(L), int(L.max()) if len(L) and L.max() > 0 else 0
    j = np.broadcast_to(np.arange(N)[:, None], (N, W)).copy()
    used = np.arange(W)[None, :] < L[:, None]
    for i in range(N):
        j[i, :L[i]] = idx[row_start[i]:row_start[i] + L[i]]
    return j, used, L


def dense_csr(idx):
    """idx [N,k] -> (flat [N k], row_start = i k): a fixed-width list written as rows."""
    idx = np.asarray(idx)
    N, k = idx.shape
    return idx.reshape(-1).copy(), np.arange(N + 1, dtype=np.int64) * k


def widen(sp):
    """fpfh_restated's bytes uint8 [N,48] -> the header's words int64 [N,3,12]."""
    return np.asarray(sp, np.uint8).reshape(-1, 3, 16)[:, :, :12].astype(np.int64)


# ---------------------------------------------------------------------------------------------------------------------- normals

def covariances(x, idx, row_start, max_nn=0):
    """-> (C float64 [N,3,3], L): the header's C over {i} U row[0..L_i); rows with L_i < 2 hold zeros (they are not asked)."""
    j, _, L = padded(idx, row_start, max_nn)
    N = len(L)
    C = np.zeros((N, 3, 3))
    for length in np.unique(L[L >= 2]):
        rows = L == length
        C[rows] = pr.covariances(x, j[:, :length])[rows]    # (the other rows' columns are cut or their own index: not taken)
    return C, L


def _rotate(a, v, p, q, r):
    """nm_rotate on the symmetric a (dict of the six entries by sorted index pair) and the columns p, q of v."""
    key = lambda s, t: (s, t) if s < t else (t, s)          # noqa: E731
    apq = a[key(p, q)]
    if apq == 0.0:
        return
    app, aqq = a[(p, p)], a[(q, q)]
    theta = (aqq - app) / (2.0 * apq)
    th2 = theta * theta
    t = 0.5 / theta if math.isinf(th2) else (1.0 if theta >= 0.0 else -1.0) / (abs(theta) + math.sqrt(th2 + 1.0))
    c = 1.0 / math.sqrt(t * t + 1.0)
    s = t * c
    a[(p, p)], a[(q, q)], a[key(p, q)] = app - t * apq, aqq + t * apq, 0.0
    xx, yy = a[key(r, p)], a[key(r, q)]
    a[key(r, p)], a[key(r, q)] = c * xx - s * yy, s * xx + c * yy
    for row in range(3):
        aa, bb = v[row][p], v[row][q]
        v[row][p], v[row][q] = c * aa - s * bb, s * aa + c * bb


def jacobi_normal(C, x_i=None, viewpoint=None):
    """C [3,3] float64 -> (n fp32 [3], curvature fp32): the device's solve step by step (csrc/normals_point.h)."""
    if not np.isfinite(C).all():
        return np.asarray([0, 0, 1], F32), F32(np.nan)
    if not C.any():
        return np.asarray([0, 0, 1], F32), F32(0)
    a = {(0, 0): float(C[0, 0]), (0, 1): float(C[0, 1]), (0, 2): float(C[0, 2]), (1, 1): float(C[1, 1]), (1, 2): float(C[1, 2]),
         (2, 2): float(C[2, 2])}
    v = [[1.0, 0.0, 0.0], [0.0, 1.0, 0.0], [0.0, 0.0, 1.0]]
    for _ in range(SWEEPS):
        if a[(0, 1)] == 0.0 and a[(0, 2)] == 0.0 and a[(1, 2)] == 0.0:
            break
        _rotate(a, v, 0, 1, 2)
        _rotate(a, v, 0, 2, 1)
        _rotate(a, v, 1, 2, 0)
    d = [a[(0, 0)], a[(1, 1)], a[(2, 2)]]
    c = 0 if (d[0] <= d[1] and d[0] <= d[2]) else (1 if d[1] <= d[2] else 2)
    l0 = d[c]
    o1, o2 = (d[1] if c == 0 else d[0]), (d[1] if c == 2 else d[2])
    l1, l2 = (o1, o2) if o1 <= o2 else (o2, o1)
    e = [v[0][c], v[1][c], v[2][c]]
    ln = math.sqrt((e[0] * e[0] + e[1] * e[1]) + e[2] * e[2])
    n = np.asarray([e[0] / ln, e[1] / ln, e[2] / ln]).astype(F32)
    tr = (l0 + l1) + l2
    return pr.orient(n, x_i, viewpoint), F32(0) if tr == 0.0 else F32(l0 / tr)


def normals(x, idx, row_start, max_nn=0, viewpoint=None, solve=jacobi_normal):
    """vcr_rows_normals_f32 for one cloud -> (normals fp32 [3,N], curvature fp32 [N], C, L)."""
    x = np.asarray(x, F32)
    C, L = covariances(x, idx, row_start, max_nn)
    N = len(L)
    n, cv = np.zeros((3, N), F32), np.zeros(N, F32)
    n[2] = 1                                                # L < 2: (0, 0, 1), curvature 0
    for i in np.flatnonzero(L >= 2):
        got = solve(C[i], x[:, i], viewpoint)
        n[:, i], cv[i] = got[0], got[-1]
    return n, cv, C, L


# ------------------------------------------------------------------------------------------------------------------------- fpfh

def pairs(x, nrm, idx, row_start, max_nn=0):
    """fpfh_restated.pairs over the rows' rectangle, `counted` (and `tie`) false in the unused slots; plus used and L."""
    j, used, L = padded(idx, row_start, max_nn)
    p = fr.pairs(x, nrm, j, 0.0)
    p["counted"] = p["counted"] & used
    p["tie"] = p["tie"] & used
    p["used"], p["L"] = used, L
    return p


def pack(p):
    """The pairs' bins as the header's words: int64 [N,3,12]."""
    N, W = p["counted"].shape
    h = np.zeros((N, 3, 12), np.int64)
    rows = np.arange(N)
    for jj in range(W):
        m = p["counted"][:, jj]
        for g in range(3):
            np.add.at(h[:, g, :], (rows[m], p["bins"][m, jj, g]), 1)
    h[:, :, BINS] = p["counted"].sum(1)[:, None]
    return h


def spfh(x, nrm, idx, row_start, max_nn=0):
    """vcr_rows_spfh_f32 for one cloud: int64 [N,3,12]."""
    return pack(pairs(x, nrm, idx, row_start, max_nn))


def fpfh(x, idx, row_start, sp, max_nn=0):
    """vcr_rows_fpfh_f32 for one cloud from the words sp [N,3,12]: float32 [33,N] -- fpfh_restated.fpfh's chain, no radius."""
    j, _, _ = padded(idx, row_start, max_nn)               # (an unused slot reads as i: d2 = 0, the chain skips it)
    j, _, d2 = fr.geometry(x, j)
    N, W = j.shape
    sp = np.asarray(sp).astype(np.int64).reshape(N, 3, 12)
    out = np.zeros((3 * BINS, N), F32)
    with np.errstate(all="ignore"):
        for g in range(3):
            acc, s = np.zeros((N, BINS)), np.zeros(N)
            for jj in range(W):
                r, dd = j[:, jj], d2[:, jj]
                cj = sp[r, g, BINS].astype(np.float64)
                ok = (dd > 0) & np.isfinite(dd) & (cj != 0)
                sc = 100.0 / cj
                for b in range(BINS):
                    val = (sp[r, g, b].astype(np.float64) * sc) / dd
                    acc[:, b] = np.where(ok, acc[:, b] + val, acc[:, b])
                    s = np.where(ok, s + val, s)
            acc = np.where((s != 0)[:, None], acc * (100.0 / s)[:, None], acc)
            ci = sp[:, g, BINS].astype(np.float64)
            mine = np.where((ci != 0)[:, None], sp[:, g, :BINS].astype(np.float64) * (100.0 / ci)[:, None], 0.0)
            out[g * BINS:(g + 1) * BINS] = (acc + mine).T.astype(F32)
    return out


# ---------------------------------------------------------------------------------------------------------------- the recipes

RAGGED = (2, 300)                                           # fpfh_restated.cloud(B, N): the jittered torus of the GPU test
# radii on that cloud: rows of 0, 1, 2 entries (the longest 17); of 63, 64, 65 and 129; of 129 and of more than 255 (the longest
# 261); the last spans the cloud, 299 entries in every row (tests/test_rows_cpu.py asserts all of it)
RAGGED_RADII = (0.1, 0.335, 0.53, 4.0)
WANTED_LENGTHS = (0, 1, 2, 63, 64, 65, 129)


def exact_cloud(B=2, N=300, seed=5):
    """[B,3,N] fp32, coordinates multiples of 2^-6 in (-4, 4), no two points alike: every difference, and d2 = dx^2 + dy^2 +
    dz^2 in any order, fused or not, in fp32 or fp64, is exact (below 3 * 2^18 units of 2^-12)."""
    rs = np.random.RandomState(seed)
    out = []
    for _ in range(B):
        while True:
            q = rs.randint(-255, 256, (3, N))
            if len({tuple(c) for c in q.T}) == N:
                break
        out.append((q * 2.0 ** -6).astype(F32))
    return np.stack(out)
