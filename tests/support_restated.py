"""CPU restatement of include/support/vcr_hip_support.h in numpy -- what the tests compare the support
kernels with.  Two parts.

The used-entries rule (``used``): walk a centre's row in order; an entry outside [0, N) is skipped, an entry equal to the centre's
self index is a self entry, any other a neighbour entry; the walk ends behind the max_nn-th neighbour entry.

The four definitions, built ON rows_restated, fpfh_restated and plane_restated: the support cloud and the centres are laid into
ONE cloud of N + M points (``joined``), centre i at index N + i, and the centres' used neighbour entries into CSR rows over it (the
support's rows empty), so that rows_restated's spfh (fpfh_restated's pairs and pack) and fpfh (the weighted sum) run as they are
and their last M rows are the answer.  The normals take plane_restated's sign rule and rows_restated's Jacobi solve; only the
nine sums over the m used entries with the divisor m -- the one thing that differs from "the point and its k neighbours" -- are
written here.

One cloud is x float32 [3,N] with centres c float32 [3,M] and rows (idx int [total or more], row_start int64 [M+1]); self_index
int [M] or None; max_nn = 0 takes whole rows."""
import numpy as np

import rows_restated as wr

F32 = np.float32
BINS = 11


def finite(c):
    return np.isfinite(np.asarray(c, F32)).all(0)


def used(idx, row_start, N, self_index=None, max_nn=0):
    """-> a list over the centres of (entries int64 [m], is_self bool [m]): the USED entries of each row, in order."""
    idx = np.asarray(idx).astype(np.int64)
    row_start = np.asarray(row_start, np.int64)
    out = []
    for i in range(len(row_start) - 1):
        s = -1 if self_index is None else int(self_index[i])
        ent, own, taken = [], [], 0
        for e in idx[row_start[i]:row_start[i + 1]]:
            if e < 0 or e >= N:
                continue                                    # skipped: it counts as nothing
            ent.append(int(e))
            own.append(e == s)
            if e != s:
                taken += 1
                if taken == max_nn:                         # (max_nn == 0: never)
                    break
        out.append((np.asarray(ent, np.int64), np.asarray(own, bool)))
    return out


def neighbour_rows(idx, row_start, N, self_index=None, max_nn=0, keep=None):
    """The used NEIGHBOUR entries as CSR (flat int64, row_start int64 [M+1]); keep bool [M]: the other centres' rows are empty."""
    rows = [e[~o] for e, o in used(idx, row_start, N, self_index, max_nn)]
    if keep is not None:
        rows = [r if k else r[:0] for r, k in zip(rows, keep)]
    rs = np.zeros(len(rows) + 1, np.int64)
    rs[1:] = np.cumsum([len(r) for r in rows])
    return (np.concatenate(rows) if rows else np.zeros(0, np.int64)).astype(np.int64), rs


def joined(x, c, rows):
    """-> (X float32 [3,N+M], idx, row_start int64 [N+M+1]): the support then the centres as one cloud, the support's rows empty
    and centre i's row that of point N + i."""
    x, c = np.asarray(x, F32), np.asarray(c, F32)
    N = x.shape[1]
    idx, rs = rows
    return np.concatenate([x, c], axis=1), idx, np.concatenate([np.zeros(N, np.int64), rs])


# ---------------------------------------------------------------------------------------------------------------------- normals

def covariance(x, c_i, entries):
    """C float64 [3,3] over the m entries: d = x_j - c_i in fp32, widened; nine fp64 sums in the entries' order; divisor m."""
    d = (np.asarray(x, F32)[:, entries] - np.asarray(c_i, F32)[:, None]).astype(np.float64).T
    if len(d) == 0:
        return np.full((3, 3), np.nan)
    Sd = np.cumsum(d, axis=0)[-1]                           # (cumsum adds in the entries' order; 0 + d_0 is d_0)
    Sdd = np.cumsum(d[:, :, None] * d[:, None, :], axis=0)[-1]    # products of two fp32 values: exact
    m = np.float64(len(entries))
    mean = Sd / m
    with np.errstate(invalid="ignore", over="ignore"):
        return Sdd / m - mean[:, None] * mean[None, :]


def normals(x, c, idx, row_start, self_index=None, max_nn=0, viewpoint=None):
    """vcr_support_normals_f32 for one cloud -> (normals fp32 [3,M], curvature fp32 [M])."""
    x, c = np.asarray(x, F32), np.asarray(c, F32)
    M = c.shape[1]
    n, cv = np.zeros((3, M), F32), np.zeros(M, F32)
    n[2] = 1                                                # m < 3: (0, 0, 1), curvature 0
    ok = finite(c)
    for i, (ent, _) in enumerate(used(idx, row_start, x.shape[1], self_index, max_nn)):
        if not ok[i]:
            n[:, i], cv[i] = np.nan, np.nan
        elif len(ent) >= 3:
            n[:, i], cv[i] = wr.jacobi_normal(covariance(x, c[:, i], ent), c[:, i], viewpoint)
    return n, cv


# ------------------------------------------------------------------------------------------------------------------------- fpfh

def pairs(x, nrm, c, cn, idx, row_start, self_index=None, max_nn=0):
    """rows_restated.pairs for the centres' used neighbour entries: the dict's arrays hold N + M rows, the last M the centres'."""
    N = np.asarray(x).shape[1]
    X, j, rs = joined(x, c, neighbour_rows(idx, row_start, N, self_index, max_nn, keep=finite(c)))
    return wr.pairs(X, np.concatenate([np.asarray(nrm, F32), np.asarray(cn, F32)], axis=1), j, rs)


def spfh(x, nrm, c, cn, idx, row_start, self_index=None, max_nn=0):
    """vcr_support_spfh_f32 for one cloud: int64 [M,3,12] (a centre that is not finite: zero words)."""
    N = np.asarray(x).shape[1]
    return wr.pack(pairs(x, nrm, c, cn, idx, row_start, self_index, max_nn))[N:]


def needed(x, c, idx, row_start, self_index=None, max_nn=0):
    """vcr_support_needed_f32 for one cloud -> dict of points fp32 [3,N], count, index int32 [N], slot int32 [N]."""
    x = np.asarray(x, F32)
    N = x.shape[1]
    flat, _ = neighbour_rows(idx, row_start, N, self_index, max_nn, keep=finite(c))
    need = np.zeros(N, bool)
    need[flat] = True
    at = np.flatnonzero(need)
    points, index, slot = np.full((3, N), np.nan, F32), np.full(N, -1, np.int32), np.full(N, -1, np.int32)
    points[:, :len(at)], index[:len(at)], slot[at] = x[:, at], at, np.arange(len(at))
    return {"points": points, "count": len(at), "index": index, "slot": slot}


def fpfh(x, c, idx, row_start, support_spfh, centre_spfh, self_index=None, slot=None, max_nn=0):
    """vcr_support_fpfh_f32 for one cloud from support_spfh [R,3,12] and centre_spfh [M,3,12]: float32 [33,M].  A neighbour
    whose slot is outside [0, R) is given a row of zeros: c == 0, which rows_restated.fpfh's chain skips."""
    x = np.asarray(x, F32)
    N = x.shape[1]
    support_spfh = np.asarray(support_spfh).astype(np.int64).reshape(-1, 3, 12)
    R = len(support_spfh)
    slot = np.arange(N) if slot is None else np.asarray(slot).astype(np.int64)
    ok = (slot >= 0) & (slot < R)
    per_point = np.where(ok[:, None, None], support_spfh[np.where(ok, slot, 0)], 0)
    X, j, rs = joined(x, c, neighbour_rows(idx, row_start, N, self_index, max_nn))
    sp = np.concatenate([per_point, np.asarray(centre_spfh).astype(np.int64).reshape(-1, 3, 12)])
    out = wr.fpfh(X, j, rs, sp)[:, N:]
    out[:, ~finite(c)] = np.nan
    return out


def feature(x, nrm, c, q_rows, s_rows, self_index=None, query_normals=None, max_nn=0, support_spfh=None):
    """compute_fpfh_feature(queries=c, query_index=self_index) for one cloud, the "all" plan written out: q_rows the centres'
    rows in the support, s_rows the support's own rows (a self search).  nrm None estimates the support's normals from s_rows
    (rows_restated.normals).  -> (fpfh float32 [33,M], the centres' normals, the centres' spfh)."""
    x, c = np.asarray(x, F32), np.asarray(c, F32)
    N = x.shape[1]
    if nrm is None:
        nrm = wr.normals(x, s_rows[0], s_rows[1], max_nn)[0]
    nrm = np.asarray(nrm, F32)
    if support_spfh is None:                                # (given: the same histograms, computed once for several calls)
        support_spfh = wr.spfh(x, nrm, s_rows[0], s_rows[1], max_nn)
    if query_normals is None:
        query_normals = normals(x, c, q_rows[0], q_rows[1], self_index, max_nn)[0]
        if self_index is not None:
            has = (np.asarray(self_index) >= 0) & (np.asarray(self_index) < N)
            query_normals[:, has] = nrm[:, np.asarray(self_index)[has]]
    mine = spfh(x, nrm, c, query_normals, q_rows[0], q_rows[1], self_index, max_nn)
    return fpfh(x, c, q_rows[0], q_rows[1], support_spfh, mine, self_index, None, max_nn), query_normals, mine


def with_self_at_head(idx, row_start):
    """Self rows (no row holds its own index) -> the same rows with i inserted at the head of row i."""
    idx, row_start = np.asarray(idx).astype(np.int64), np.asarray(row_start, np.int64)
    N = len(row_start) - 1
    rows = [np.concatenate([[i], idx[row_start[i]:row_start[i + 1]]]) for i in range(N)]
    return np.concatenate(rows), row_start + np.arange(N + 1)


# ---------------------------------------------------------------------------------------------------------------- the recipes

RADII = wr.RAGGED_RADII[:3]                                 # 0.1: rows of 0 to a few entries; 0.335: around the form threshold and
SIZES = (1, 37, 300, 333)                                   # the wave's chunk of 64; 0.53: long rows.  M: one, few, N, more than N
CENTRES = ("jitter", "outside", "nonfinite")                # query_restated's recipes for positions that are not points


def centres(x, name, M, seed=0):
    """query_restated's recipe `name` on the cloud x [3,N] -> float32 [3,M]."""
    import query_restated as qr
    return qr.QUERIES[name](np.asarray(x, F32), M, seed=seed)


def subset(N, M=37, seed=11):
    """M indices into [0, N): one repeated, one -1."""
    at = np.random.RandomState(seed).choice(N, M, replace=False).astype(np.int32)
    at[5], at[9] = at[2], -1
    return at
