"""include/smooth/vcr_hip_mls.h restated in numpy: the frame of a point, the mean and the origin of its fit,
every entry's weight (np.exp: the one library call), the 27 weighted sums in the 64-chain order, the 6 x 6 Cholesky and the
projection -- every expression in the header's order, in IEEE doubles, one operation a numpy call so nothing is fused.

One cloud is x float32 [3,N] with normals float32 [3,N] and its rows as (idx int [total or more], row_start int64 [N+1]).  The
recipes the CPU and the GPU tests share (the noisy sphere, the jittered lattice in a plane, the hand-built rows) are at the end."""
import numpy as np

import dbscan_restated as dr
import iss_restated as ir
import radius_restated as rr
import rows_restated as wr

F32, I32, F64 = np.float32, np.int32, np.float64
NOT_SERVED = -2
TERMS = 6
SUMS = 27
XOR_STEPS = (32, 16, 8, 4, 2, 1)
TINY = 2.0 ** -40
LANES = np.arange(64)


def frame(x_i, n):
    """-> (nh, u, uh, v) as float64 [3] each (u before it is normalised: the boundary pass's), or None where there is no frame."""
    n = np.asarray(n, F32).astype(F64)
    with np.errstate(all="ignore"):
        s = (n[0] * n[0] + n[1] * n[1]) + n[2] * n[2]
        if not (np.isfinite(np.asarray(x_i, F64)).all() and np.isfinite(n).all() and s > 0.0 and np.isfinite(s)):
            return None
        h = n * (1.0 / np.sqrt(s))
    a, am = 0, abs(h[0])
    if abs(h[1]) < am:
        a, am = 1, abs(h[1])
    if abs(h[2]) < am:
        a = 2
    e = np.zeros(3)
    e[a] = 1.0
    cross = lambda p, q: np.asarray([p[1] * q[2] - p[2] * q[1], p[2] * q[0] - p[0] * q[2], p[0] * q[1] - p[1] * q[0]])  # noqa: E731
    u = cross(h, e)
    uh = u * (1.0 / np.sqrt((u[0] * u[0] + u[1] * u[1]) + u[2] * u[2]))
    return h, u, uh, cross(h, uh)


def chains(terms):
    """terms float64 [L,T] -> [T]: chain p adds the entries p, p + 64, ... in ascending order from +0.0, then v[p] = v[p] + v[p ^ s]
    for s = 32 ... 1.  (A slot without an entry adds +0.0, which changes no chain: none is ever -0.0.)"""
    L, T = terms.shape
    steps = (L + 63) // 64
    t = np.zeros((max(steps, 1) * 64, T))
    t[:L] = terms
    t = t.reshape(-1, 64, T)
    v = np.zeros((64, T))
    with np.errstate(all="ignore"):
        for c in range(steps):
            v = v + t[c]
        for s in XOR_STEPS:
            v = v + v[LANES ^ s]
    return v[0].copy()


def differences(x, i, j):
    """The fp32 differences x_j - x_i widened, [3,L], and which entries are not skipped."""
    N = x.shape[1]
    j = np.asarray(j).astype(np.int64)
    j = np.where((j >= 0) & (j < N), j, i)
    with np.errstate(all="ignore"):
        d = (x[:, j] - x[:, i:i + 1]).astype(F64)
    return d, np.isfinite(d).all(0)


def weights(x, normals, idx, row_start, h2, capacity=None, exp=np.exp):
    """vcr_mls_weights_f32 for one served cloud -> (weight float64 [capacity], origin float64 [N,3], w_self float64 [N], frame
    int32 [N])."""
    x, normals = np.asarray(x, F32), np.asarray(normals, F32)
    N = x.shape[1]
    row_start = np.asarray(row_start, np.int64)
    total = int(row_start[-1])
    h2 = F64(h2)
    weight = np.full(total if capacity is None else capacity, np.nan)
    origin, w_self, fr = np.full((N, 3), np.nan), np.full(N, np.nan), np.zeros(N, I32)
    with np.errstate(all="ignore"):
        for i in range(N):
            fm = frame(x[:, i], normals[:, i])
            if fm is None:
                continue
            fr[i] = 1
            h = fm[0]
            s, e = int(row_start[i]), int(row_start[i + 1])
            d, fin = differences(x, i, idx[s:e])
            S = chains(np.where(fin, d, 0.0).T)
            mu = S / F64(e - s + 1)
            t = (mu[0] * h[0] + mu[1] * h[1]) + mu[2] * h[2]
            o = t * h
            q = d - o[:, None]
            weight[s:e] = np.where(fin, exp(-(((q[0] * q[0] + q[1] * q[1]) + q[2] * q[2]) / h2)), 0.0)
            origin[i] = o
            w_self[i] = exp(-(((o[0] * o[0] + o[1] * o[1]) + o[2] * o[2]) / h2))
    return weight, origin, w_self, fr


def arguments(x, normals, idx, row_start, h2):
    """The argument of every exp of ``weights`` (the rows' and the points' own), for the allowance's measurement: the device's
    weights are held to np.exp of these."""
    got = []
    weights(x, normals, idx, row_start, h2, exp=lambda a: (got.append(np.atleast_1d(a).copy()), np.exp(a))[1])
    return np.concatenate(got) if got else np.zeros(0)


def terms_of(w, uu, vv, f):
    """The 27 terms of entries -> float64 [L,27]: A_ab row by row (a <= b), then r_a."""
    p = [np.ones_like(uu), vv, vv * vv, uu, uu * vv, uu * uu]
    wp = [w * pa for pa in p]
    return np.stack([wp[a] * p[b] for a in range(6) for b in range(a, 6)] + [wp[a] * f for a in range(6)], axis=1)


def at(a, b):
    """Where A_ab (a <= b) sits among the sums."""
    return a * 6 - a * (a - 1) // 2 + (b - a)


def sums(x, i, j, w, o, w_self, uh, v, h):
    """The 27 sums of row i: the entries in the 64 chains, then the point's own term by one addition."""
    dot = lambda q, a: (q[0] * a[0] + q[1] * a[1]) + q[2] * a[2]                 # noqa: E731
    with np.errstate(all="ignore"):
        d, fin = differences(x, i, j)
        q = d - o[:, None]
        z = lambda t: np.where(fin, t, 0.0)                                       # noqa: E731
        S = chains(terms_of(z(np.asarray(w, F64)), z(dot(q, uh)), z(dot(q, v)), z(dot(q, h))))
        q = (-o)[:, None]
        return S + terms_of(np.asarray([w_self], F64), dot(q, uh), dot(q, v), dot(q, h))[0]


def cholesky_solve(S):
    """The header's solve on the 27 sums -> (c float64 [6], failed)."""
    A = lambda a, b: F64(S[at(min(a, b), max(a, b))])                            # noqa: E731
    Lm = np.zeros((6, 6))
    failed = False
    with np.errstate(all="ignore"):
        for k in range(6):
            t = A(k, k)
            for j in range(k):
                t = t - Lm[k, j] * Lm[k, j]
            failed = failed or not (np.isfinite(t) and t > A(k, k) * TINY)
            Lm[k, k] = np.sqrt(t)
            for r in range(k + 1, 6):
                s = A(k, r)
                for j in range(k):
                    s = s - Lm[r, j] * Lm[k, j]
                Lm[r, k] = s / Lm[k, k]
        y, c = np.zeros(6), np.zeros(6)
        for k in range(6):
            t = F64(S[21 + k])
            for j in range(k):
                t = t - Lm[k, j] * y[j]
            y[k] = t / Lm[k, k]
        for k in range(5, -1, -1):
            t = y[k]
            for j in range(k + 1, 6):
                t = t - Lm[j, k] * c[j]
            c[k] = t / Lm[k, k]
    return c, failed


def fit(x, normals, idx, row_start, weight, origin, w_self, fr, order=2, min_neighbors=3, want_sums=False):
    """vcr_mls_fit_f32 for one served cloud, reading weight, origin, w_self and frame AS GIVEN -> dict of points float32 [3,N], fit
    int32 [N], normals float32 [3,N], coeffs float64 [N,6] (and sums float64 [N,27], NaN where no quadratic was asked)."""
    x, normals = np.asarray(x, F32), np.asarray(normals, F32)
    N = x.shape[1]
    row_start = np.asarray(row_start, np.int64)
    points, nout = x.copy(), np.full((3, N), np.nan, F32)
    how, coeffs, allsums = np.zeros(N, I32), np.zeros((N, 6)), np.full((N, SUMS), np.nan)
    with np.errstate(all="ignore"):
        for i in range(N):
            fm = frame(x[:, i], normals[:, i])
            s, e = int(row_start[i]), int(row_start[i + 1])
            m = e - s + 1
            if fm is None:
                continue
            h, _, uh, v = fm
            nout[:, i] = h.astype(F32)
            if fr[i] == 0 or m < min_neighbors:
                continue
            how[i] = 1
            c = np.zeros(6)
            o = np.asarray(origin[i], F64)
            if order == 2 and m >= TERMS:
                S = sums(x, i, idx[s:e], weight[s:e], o, w_self[i], uh, v, h)
                allsums[i] = S
                got, failed = cholesky_solve(S)
                if not failed:
                    how[i], c = 2, got
            coeffs[i] = c
            points[:, i] = (x[:, i].astype(F64) + (o + c[0] * h)).astype(F32)
            g = (h - c[3] * uh) - c[1] * v
            nout[:, i] = (g * (1.0 / np.sqrt((g[0] * g[0] + g[1] * g[1]) + g[2] * g[2]))).astype(F32)
    out = {"points": points, "fit": how, "normals": nout, "coeffs": coeffs}
    if want_sums:
        out["sums"] = allsums
    return out


def not_served(N):
    return {"points": np.full((3, N), np.nan, F32), "fit": np.full(N, NOT_SERVED, I32), "normals": np.full((3, N), np.nan, F32),
            "coeffs": np.full((N, 6), np.nan)}


def definition(x, normals, rows, h2, order=2, min_neighbors=3, capacity=None, exp=np.exp):
    """The two stages for one cloud.  rows = (idx, row_start[, total]); capacity enters "served" alone."""
    x = np.asarray(x, F32)
    N = x.shape[1]
    total = int(rows[2]) if len(rows) > 2 else int(np.asarray(rows[1])[-1])
    cap = total if capacity is None else capacity
    if not dr.served(rows[1], total, cap):
        return dict(not_served(N), weight=np.full(cap, np.nan), origin=np.full((N, 3), np.nan), w_self=np.full(N, np.nan),
                    frame=np.full(N, NOT_SERVED, I32))
    w, o, ws, fr = weights(x, normals, rows[0], rows[1], h2, cap, exp)
    return dict(fit(x, normals, rows[0], rows[1], w, o, ws, fr, order, min_neighbors), weight=w, origin=o, w_self=ws, frame=fr)


def hybrid_rows(x, radius, max_nn=None):
    """The definition's rows of the public call: all points within radius, cut to the nearest max_nn (None: all)."""
    res = rr.radius_rows(np.ascontiguousarray(x, F32), radius)
    return res if max_nn is None else rr.cut(res, max_nn)


def of_cloud(x, normals, radius, order=2, max_nn=None, sqr_gauss_param=None, min_neighbors=3, rows=None):
    """smooth_mls for one cloud with given normals, on the definition's rows."""
    res = hybrid_rows(x, radius, max_nn) if rows is None else rows
    h2 = float(radius) * float(radius) if sqr_gauss_param is None else sqr_gauss_param
    return definition(x, normals, (res["idx"], res["row_start"]), h2, order, min_neighbors)


def ulps(got, want):
    """The largest |got - want| in units in the last place of want (float64 arrays, finite and of one sign pattern)."""
    got, want = np.asarray(got, F64), np.asarray(want, F64)
    if got.size == 0:
        return 0.0
    return float(np.max(np.abs(got - want) / np.spacing(np.abs(want))))


def ulps32(got, want):
    """Per element: how many fp32 values lie between got and want (0 = the same bits; NaN against NaN counts 0)."""
    key = lambda a: np.where(a.view(np.int32) < 0, np.int64(-2 ** 31) - a.view(np.int32).astype(np.int64),  # noqa: E731
                             a.view(np.int32).astype(np.int64))
    got, want = np.ascontiguousarray(got, F32), np.ascontiguousarray(want, F32)
    d = np.abs(key(got) - key(want))
    both = np.isnan(got) & np.isnan(want)
    one = np.isnan(got) ^ np.isnan(want)
    return np.where(both, 0, np.where(one, 2 ** 40, d))


# ------------------------------------------------------------------------------------------------------------------- the recipes

SPHERE_N, SPHERE_SIGMA, SPHERE_RADIUS = 1200, 0.01, 0.3
SEEDS = (0, 1, 2)


def noisy_sphere(seed, N=SPHERE_N, sigma=SPHERE_SIGMA):
    """N uniform directions on the unit sphere, every point moved along its direction by a normal deviate of sigma -> x [3,N]."""
    rs = np.random.RandomState(seed)
    dirs = rs.normal(size=(3, N))
    dirs /= np.sqrt((dirs * dirs).sum(0))
    return (dirs * (1.0 + sigma * rs.normal(size=N))).astype(F32)


def outward(x, nrm):
    """nrm with every normal on the side of its point's direction from the origin."""
    flip = (np.asarray(x, F64) * np.asarray(nrm, F64)).sum(0) < 0
    return np.where(flip[None, :], -nrm, nrm).astype(F32)


def sphere_normals(x, radius=SPHERE_RADIUS, rows=None):
    """The input normals of the sphere tests: the rows' own estimate (rows_restated.normals), turned outward."""
    res = hybrid_rows(x, radius) if rows is None else rows
    return outward(x, wr.normals(x, res["idx"], res["row_start"])[0])


def radial_rms(points):
    r = np.sqrt((np.asarray(points, F64) ** 2).sum(0))
    return float(np.sqrt(np.mean((r - 1.0) ** 2)))


def radial_angle(points, nrm):
    """The mean angle (degrees) of the normals to their points' directions from the origin."""
    p, n = np.asarray(points, F64), np.asarray(nrm, F64)
    cos = (p * n).sum(0) / (np.sqrt((p * p).sum(0)) * np.sqrt((n * n).sum(0)))
    return float(np.degrees(np.arccos(np.clip(cos, -1, 1))).mean())


def smoothing(x, nrm, got):
    """The figures of the smoothing condition -> (rms in, rms out, angle in, angle out)."""
    return radial_rms(x), radial_rms(got["points"]), radial_angle(x, nrm), radial_angle(got["points"], got["normals"])


def plane_lattice(n=20, seed=7):
    """An n x n lattice of spacing 1 in the plane z = 0.25, jittered IN the plane by up to 0.2 -> (x [3,n n], normals (0, 0, 1)).
    Every height over the plane is exactly zero, so every fit's right-hand side is, and every point comes back with its bits."""
    rs = np.random.RandomState(seed)
    gx, gy = np.meshgrid(np.arange(n), np.arange(n), indexing="ij")
    x = np.stack([gx.ravel() + rs.uniform(-0.2, 0.2, n * n), gy.ravel() + rs.uniform(-0.2, 0.2, n * n),
                  np.full(n * n, 0.25)]).astype(F32)
    nrm = np.zeros((3, n * n), F32)
    nrm[2] = 1
    return x, nrm


LENGTHS = (0, 1, 2, 4, 5, 6, 63, 64, 65, 128, 129)
HAND_N = 200
NAN_POINT, NAN_OWNER, ZERO_NORMAL, COPY_OF, COLLINEAR, EQUAL = 150, 151, 152, 153, 154, 155


def hand_cloud(seed=0, N=HAND_N):
    """A bumpy sheet of N points with rough normals and caller-built rows: row i has LENGTHS[i % 11] entries (so every length
    occurs about 18 times), among them entries outside [0, N), the point itself and a copy of it; point NAN_POINT is NaN and sits
    in many rows, NAN_OWNER is NaN and owns a row, ZERO_NORMAL has the normal 0; COLLINEAR's row lies on one line through it and
    EQUAL's row is copies of one point -> (x, normals, idx, row_start)."""
    rs = np.random.RandomState(100 + seed)
    x = rs.uniform(-1, 1, (3, N))
    x[2] = 0.2 * np.sin(2 * x[0]) * np.cos(1.5 * x[1]) + 0.01 * rs.normal(size=N)
    x = x.astype(F32)
    nrm = np.stack([-0.4 * np.cos(2 * x[0]), 0.3 * np.sin(1.5 * x[1]), np.ones(N)]) + 0.05 * rs.normal(size=(3, N))
    nrm = (nrm * rs.uniform(0.5, 2.0, N)).astype(F32)
    nrm[:, 7] = [0, 0, -3]                                  # equal smallest |nh_a|: the lowest index
    x[:, COPY_OF] = x[:, 3]
    x[:, [NAN_POINT, NAN_OWNER]] = np.nan
    nrm[:, ZERO_NORMAL] = 0
    line = [160, 161, 162, 163, 164, 165, 166]
    for k, j in enumerate(line):
        x[:, j] = x[:, COLLINEAR] + F32(0.1 * (k + 1)) * np.asarray([1, 2, 0], F32)
    nrm[:, COLLINEAR] = [0, 0, 1]
    rows = []
    for i in range(N):
        r = rs.randint(0, N, LENGTHS[i % len(LENGTHS)])
        r = np.where(np.isin(r, [NAN_POINT, NAN_OWNER]) & (rs.uniform(size=len(r)) < 0.7), (r + 17) % 140, r)
        if len(r) > 3:
            r[1] = NAN_POINT if i % 4 == 0 else r[1]
            r[2] = (-1, N + 7, i, 3, COPY_OF)[i % 5]
        rows.append(r.tolist())
    rows[COLLINEAR] = line
    rows[EQUAL] = [170] * 8
    rows[3] = rows[3] + [COPY_OF]
    return (x, nrm) + ir.flat(rows)
