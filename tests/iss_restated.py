"""CPU restatement of include/keypoint/vcr_hip_iss.h in numpy -- what the tests compare the ISS kernels
with -- and the clouds the CPU and GPU tests share.

One cloud is x float32 [3,N] with its rows as (idx int [total or more], row_start int64 [N+1]).
  definition        the header read literally: the 64-chain sums vectorised over the padded rows (rows_restated.padded: an unused
                    slot adds +0.0, which changes no chain, because a chain that starts at +0.0 never holds -0.0), C by
                    vcr_normals_f32's expressions, the cyclic Jacobi by rows_restated._rotate operation by operation in IEEE
                    doubles, the ratio tests, the prefix rule, the suppression and the selection.  Bit for bit the device's.
  float64_reading   Open3D's own arithmetic on the SAME neighbourhoods (radius_restated.radius_rows' hits): cumulants of the raw
                    coordinates over {i} U hits in float64, numpy.linalg.eigvalsh, the two ratio tests, IsLocalMaxima.  What the
                    definition is held to, except where one of its comparisons is a near tie."""
import numpy as np

import dbscan_restated as dr
import plane_restated as pr
import radius_restated as rr
import rows_restated as wr

F32 = np.float32
I32 = np.int32
NOT_SERVED = -2
NEAR = 2.0 ** -16                                           # a comparison of the float64 reading this close (relative) may fall
#                                                             either way: the fp32 differences move l0 by about 2e-6 relative
XOR_STEPS = (32, 16, 8, 4, 2, 1)


# ---------------------------------------------------------------------------------------------------------------- the 64 chains

def chain_sums(terms, used):
    """terms float64 [N,W,T], used bool [N,W] -> [N,T]: chain p adds the used entries e = p, p + 64, ... in ascending e from +0.0,
    then v[p] = v[p] + v[p ^ s] for s = 32 ... 1; every chain ends alike (asserted), chain 0 is returned."""
    N, W, T = terms.shape
    steps = (W + 63) // 64
    t = np.zeros((N, steps * 64, T))
    t[:, :W] = np.where(used[:, :, None], terms, 0.0)
    t = t.reshape(N, steps, 64, T)
    v = np.zeros((N, 64, T))
    with np.errstate(all="ignore"):
        for c in range(steps):
            v = v + t[:, c]
        lanes = np.arange(64)
        for s in XOR_STEPS:
            v = v + v[:, lanes ^ s]
    assert (v.view(np.uint64) == v[:, :1].view(np.uint64)).all() or np.isnan(v).any()
    return v[:, 0]


def chain_loop(values):
    """One row's one term by a plain loop over the chains (tests hold chain_sums to it): values float64 [L] -> the sum."""
    v = [0.0] * 64
    for p in range(64):
        for e in range(p, len(values), 64):
            v[p] = v[p] + float(values[e])
    for s in XOR_STEPS:
        v = [v[p] + v[p ^ s] for p in range(64)]
    assert all(np.float64(a).view(np.uint64) == np.float64(v[0]).view(np.uint64) for a in v)
    return v[0]


def sums(x, idx, row_start):
    """-> (S float64 [N,9]: dx, dy, dz, xx, xy, xz, yy, yz, zz in the 64-chain order, L int64 [N])."""
    x = np.asarray(x, F32)
    N = x.shape[1]
    j, used, L = wr.padded(idx, row_start)
    j = np.where((j >= 0) & (j < N), j, np.arange(N)[:, None])               # an entry outside [0, N) reads as i
    with np.errstate(all="ignore"):
        d = (x[:, j] - x[:, :, None]).astype(np.float64)                       # [3,N,W]: the fp32 difference, widened
        terms = np.stack([d[0], d[1], d[2], d[0] * d[0], d[0] * d[1], d[0] * d[2], d[1] * d[1], d[1] * d[2], d[2] * d[2]], axis=2)
    return chain_sums(terms, used), L


def covariance_of(S, m):
    """vcr_normals_f32's expressions on the nine sums: C float64 [N,3,3]."""
    m = np.asarray(m, np.float64)[:, None]
    with np.errstate(all="ignore"):
        mean = S[:, :3] / m
        q = S[:, 3:] / m
        C = np.empty((len(S), 3, 3))
        for k, (a, b) in enumerate(((0, 0), (0, 1), (0, 2), (1, 1), (1, 2), (2, 2))):
            C[:, a, b] = C[:, b, a] = q[:, k] - mean[:, a] * mean[:, b]
    return C


def jacobi_eigenvalues(C):
    """C [3,3] float64, finite and not all zero -> (l0, l1, l2): the device's sweeps and sort (csrc/iss_point.h)."""
    a = {(0, 0): float(C[0, 0]), (0, 1): float(C[0, 1]), (0, 2): float(C[0, 2]), (1, 1): float(C[1, 1]), (1, 2): float(C[1, 2]),
         (2, 2): float(C[2, 2])}
    v = [[1.0, 0.0, 0.0], [0.0, 1.0, 0.0], [0.0, 0.0, 1.0]]
    for _ in range(wr.SWEEPS):
        if a[(0, 1)] == 0.0 and a[(0, 2)] == 0.0 and a[(1, 2)] == 0.0:
            break
        wr._rotate(a, v, 0, 1, 2)
        wr._rotate(a, v, 0, 2, 1)
        wr._rotate(a, v, 1, 2, 0)
    d = [a[(0, 0)], a[(1, 1)], a[(2, 2)]]
    c = 0 if (d[0] <= d[1] and d[0] <= d[2]) else (1 if d[1] <= d[2] else 2)
    o1, o2 = (d[1] if c == 0 else d[0]), (d[1] if c == 2 else d[2])
    return (d[c], o1, o2) if o1 <= o2 else (d[c], o2, o1)


def saliency(x, idx, row_start, gamma_21=0.975, gamma_32=0.975, min_neighbors=5):
    """vcr_rows_iss_saliency_f32 for one served cloud -> (saliency float64 [N], eigen float64 [N,3])."""
    S, L = sums(x, idx, row_start)
    m = L + 1
    C = covariance_of(S, m)
    N = len(L)
    sal, eig = np.zeros(N), np.zeros((N, 3))
    for i in range(N):
        if m[i] < min_neighbors:
            continue
        if not np.isfinite(C[i]).all():
            eig[i] = np.nan
            continue
        if not C[i].any():
            continue
        l0, l1, l2 = jacobi_eigenvalues(C[i])
        eig[i] = l0, l1, l2
        with np.errstate(all="ignore"):
            if np.float64(l1) / np.float64(l2) < gamma_21 and np.float64(l0) / np.float64(l1) < gamma_32:
                sal[i] = l0
    return sal, eig


# ------------------------------------------------------------------------------------------------------------- the suppression

def used_lengths(row_start, d2=None, r2_nm=None):
    """u_i: the whole row without d2; with it the leading entries with d2 <= r2_nm (fp32), ended by the first that fails."""
    row_start = np.asarray(row_start, np.int64)
    n = np.diff(row_start)
    if d2 is None:
        return n
    r2 = F32(r2_nm)
    u = np.zeros(len(n), np.int64)
    for i in range(len(n)):
        ok = np.asarray(d2[row_start[i]:row_start[i + 1]], F32) <= r2
        u[i] = len(ok) if ok.all() else int(np.argmin(ok))
    return u


def nms(sal, idx, row_start, min_neighbors=5, d2=None, r2_nm=None):
    """vcr_rows_iss_nms_f32 for one served cloud -> keypoint int32 [N] (all -2 where a saliency is NaN)."""
    sal = np.asarray(sal, np.float64)
    N = len(sal)
    if np.isnan(sal).any():
        return np.full(N, NOT_SERVED, I32)
    idx = np.asarray(idx).astype(np.int64)
    u = used_lengths(row_start, d2, r2_nm)
    out = np.zeros(N, I32)
    for i in range(N):
        if not (sal[i] > 0 and u[i] + 1 >= min_neighbors):
            continue
        j = idx[row_start[i]:row_start[i] + u[i]]
        j = np.where((j >= 0) & (j < N), j, i)
        out[i] = not (sal[i] < sal[j]).any()
    return out


def select(x, keypoint):
    """vcr_iss_select_f32 for one cloud -> (points [3,N] with NaN behind the kept, count, index [N] with -1 behind them)."""
    N = x.shape[1]
    at = np.flatnonzero(np.asarray(keypoint) > 0)
    points = np.full((3, N), np.nan, F32)
    points[:, :len(at)] = np.asarray(x, F32)[:, at]
    index = np.full(N, -1, I32)
    index[:len(at)] = at
    return points, len(at), index


def definition(x, rows, nms_rows=None, d2=None, r2_nm=None, gamma_21=0.975, gamma_32=0.975, min_neighbors=5, capacity=None,
               nms_capacity=None):
    """The whole header for one cloud.  rows = (idx, row_start[, total]): the saliency's; nms_rows likewise (None: the same rows,
    cut to the d2 prefix where d2 and r2_nm are given).  capacity, and nms_capacity for nms_rows (None: whatever total is),
    enter "served" alone.  -> dict of saliency, eigen, keypoint, points, count, index."""
    x = np.asarray(x, F32)
    N = x.shape[1]

    def is_served(r, cap):
        total = int(r[2]) if len(r) > 2 else int(np.asarray(r[1])[-1])
        return dr.served(r[1], total, total if cap is None else cap)
    if is_served(rows, capacity):
        sal, eig = saliency(x, rows[0], rows[1], gamma_21, gamma_32, min_neighbors)
    else:
        sal, eig = np.full(N, np.nan), np.full((N, 3), np.nan)
    nr, ncap = (rows, capacity) if nms_rows is None else (nms_rows, nms_capacity)
    flag = nms(sal, nr[0], nr[1], min_neighbors, d2, r2_nm) if is_served(nr, ncap) else np.full(N, NOT_SERVED, I32)
    points, count, index = select(x, flag)
    return {"saliency": sal, "eigen": eig, "keypoint": flag, "points": points, "count": count, "index": index}


# ------------------------------------------------------------------------------------------------------------ Open3D's reading

def model_resolution(x):
    """ComputeModelResolution: the mean over the finite points of sqrt((double) d2) to the nearest other point (fp32 d2)."""
    x = np.ascontiguousarray(x, F32)
    d2 = rr.d2_all(x).astype(np.float64)
    ok = np.isfinite(x).all(0)
    d2[:, ~ok] = np.inf
    np.fill_diagonal(d2, np.inf)
    return float(np.sqrt(d2.min(1))[ok].mean())


def default_radii(x):
    """Open3D's defaults as the library takes them: fp32(6 res), fp32(4 res)."""
    res = model_resolution(x)
    return float(F32(6.0 * res)), float(F32(4.0 * res))


def float64_reading(x, salient_radius, non_max_radius, gamma_21=0.975, gamma_32=0.975, min_neighbors=5):
    """-> dict: keypoint bool [N], saliency [N], near bool [N] (a ratio of the point within NEAR of its gamma, or its saliency
    within NEAR of one of its non-max row's where that comparison decides), and the two searches' rows."""
    x = np.ascontiguousarray(x, F32)
    N = x.shape[1]
    d2 = rr.d2_all(x)
    big, small = rr.radius_rows(x, salient_radius, d2=d2), rr.radius_rows(x, non_max_radius, d2=d2)
    xd = x.astype(np.float64)
    sal, near = np.zeros(N), np.zeros(N, bool)
    for i in range(N):
        hits = np.concatenate([[i], big["idx"][big["row_start"][i]:big["row_start"][i + 1]]])
        if len(hits) < min_neighbors:
            continue
        p = xd[:, hits]
        mean = p.mean(1)
        C = (p[:, None, :] * p[None, :, :]).mean(2) - mean[:, None] * mean[None, :]
        if not np.isfinite(C).all():
            continue
        e3, e2, e1 = np.linalg.eigvalsh(C)
        with np.errstate(all="ignore"):
            r21, r32 = e2 / e1, e3 / e2
        near[i] = abs(r21 - gamma_21) <= NEAR * gamma_21 or abs(r32 - gamma_32) <= NEAR * gamma_32
        if r21 < gamma_21 and r32 < gamma_32:
            sal[i] = e3
    key = np.zeros(N, bool)
    for i in range(N):
        j = small["idx"][small["row_start"][i]:small["row_start"][i + 1]]
        # a near comparison of saliencies counts where it DECIDES: the point is a candidate and no entry beats it clearly.  (Two
        # points with the same neighbourhood tie exactly in this reading -- a few per cent of a surface's points do -- and
        # nearly all of them lose to a third point anyway.)
        tie = np.abs(sal[i] - sal[j]) <= NEAR * np.maximum(np.abs(sal[i]), np.abs(sal[j]))
        near[i] |= bool(sal[i] > 0 and tie.any() and not (sal[i] < sal[j][~tie]).any())
        if sal[i] > 0 and len(j) + 1 >= min_neighbors:
            key[i] = not (sal[i] < sal[j]).any()
    return {"keypoint": key, "saliency": sal, "near": near, "rows": big, "nms_rows": small}


def of_cloud(x, salient_radius, non_max_radius, **kw):
    """The definition on the definition's rows (radius_restated.radius_rows): one search and the prefix where non_max_radius <=
    salient_radius, two searches otherwise -- what compute_iss_keypoints returns for an explicit pair of radii."""
    x = np.ascontiguousarray(x, F32)
    big = rr.radius_rows(x, salient_radius)
    rows = (big["idx"], big["row_start"])
    if non_max_radius <= salient_radius:
        return definition(x, rows, d2=big["bits"].view(F32), r2_nm=rr.r2_of(non_max_radius), **kw)
    small = rr.radius_rows(x, non_max_radius)
    return definition(x, rows, nms_rows=(small["idx"], small["row_start"]), **kw)


# -------------------------------------------------------------------------------------------------------------------- the clouds

def torus(N=600, seed=3):
    return pr.jittered_torus(seed, N)


def bumpy(N, seed=1):
    """A height field over the unit square with bumps of several widths: corners and saddles for the detector to find."""
    rs = np.random.RandomState(seed)
    u, v = rs.uniform(0, 1, N), rs.uniform(0, 1, N)
    z = 0.1 * np.sin(9 * u) * np.cos(7 * v) + 0.15 * np.exp(-((u - .3) ** 2 + (v - .6) ** 2) / 0.01) \
        - 0.12 * np.exp(-((u - .7) ** 2 + (v - .3) ** 2) / 0.006) + 0.05 * u * v
    return np.stack([u, v, z]).astype(F32)


def cube(N=700, seed=2):
    """Uniform in the unit cube: a volume, about 107 entries a row at Open3D's default radius."""
    return np.random.RandomState(seed).uniform(0, 1, (3, N)).astype(F32)


CLOUDS = {"torus": lambda: torus(600), "bumpy600": lambda: bumpy(600), "bumpy1500": lambda: bumpy(1500), "cube": lambda: cube(700)}
GAMMAS = ((0.975, 0.975), (0.6, 0.6))                       # Open3D's, and a pair at which the ratio tests reject


def hand_cloud():
    """Two stars of six arms, every value exact.  Centre 0 at the origin with arms at (+-4,0,0), (0,+-2,0), (0,0,+-1); centre 7 at
    (10,0,0) with arms at +-4, +-2, +-0.5.  A centre's row is its six arms: S_d = 0, S_dd = diag(32, 8, 2) and diag(32, 8, 0.5),
    m = 7, C is diagonal and the Jacobi has nothing to rotate: eigen = (2/7, 8/7, 32/7) and (0.5/7, 8/7, 32/7), both ratios
    0.25 and 0.0625.  An arm's row is its centre alone: m = 2.
    -> (x [3,14], rows of the saliency, rows of the suppression with their d2): a centre's non-max row is its arms IN ORDER OF
    DISTANCE and then the other centre at d2 = 100."""
    arms = lambda c, z: [(c + 4, 0, 0), (c - 4, 0, 0), (c, 2, 0), (c, -2, 0), (c, 0, z), (c, 0, -z)]     # noqa: E731
    pts = [(0, 0, 0)] + arms(0, 1) + [(10, 0, 0)] + arms(10, 0.5)
    x = np.asarray(pts, F32).T.copy()
    sal_rows = [[1, 2, 3, 4, 5, 6]] + [[0]] * 6 + [[8, 9, 10, 11, 12, 13]] + [[7]] * 6
    nms_rows = [[5, 6, 3, 4, 1, 2, 7]] + [[0]] * 6 + [[12, 13, 10, 11, 8, 9, 0]] + [[7]] * 6
    d2 = [[1, 1, 4, 4, 16, 16, 100]] + [[16], [16], [4], [4], [1], [1]] + [[.25, .25, 4, 4, 16, 16, 100]] + [[16], [16], [4], [4], [.25], [.25]]
    return x, flat(sal_rows), flat(nms_rows), np.asarray([v for r in d2 for v in r], F32)


def flat(rows):
    """A list of rows -> (idx int32 [total], row_start int64 [N+1])."""
    row_start = np.zeros(len(rows) + 1, np.int64)
    np.cumsum([len(r) for r in rows], out=row_start[1:])
    return np.asarray([e for r in rows for e in r], I32), row_start


def batch(rows_list, slack=0):
    """Per-cloud (idx, row_start) -> (idx int32 [B,capacity] with 12345 behind each total, row_start int64 [B,N+1], total [B])."""
    cap = max(len(r[0]) for r in rows_list) + slack
    idx = np.full((len(rows_list), cap), 12345, I32)
    for b, r in enumerate(rows_list):
        idx[b, :len(r[0])] = r[0]
    row_start = np.stack([r[1] for r in rows_list])
    return idx, row_start, row_start[:, -1].copy()


LENGTHS = (0, 1, 2, 63, 64, 65, 128, 129)


def rows_of_lengths(N, lengths=LENGTHS, seed=4):
    """Caller-built rows on N points: row i has lengths[i % len] random entries, some outside [0, N) -> (idx, row_start)."""
    rs = np.random.RandomState(seed)
    rows = []
    for i in range(N):
        r = rs.randint(0, N, lengths[i % len(lengths)])
        if len(r) > 3 and i % 5 == 0:
            r[1], r[3] = -1, N + 7                          # read as i
        rows.append(r.tolist())
    return flat(rows)
