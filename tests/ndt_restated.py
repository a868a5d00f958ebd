"""CPU restatement of include/ndt/vcr_hip_ndt.h in numpy fp64 -- what the GPU tests compare the kernels
with: the map to the bit (the voxels are tests/voxel_restated.py's, the Jacobi is tests/rows_restated.py's, the lookup is a dict),
the derivative sums to the bit but for the one exp per (point, voxel) -- `e=` feeds the device's, and then they are --, and the
Levenberg-Marquardt loop decision by decision.  numpy's elementwise fp64 +, -, *, / are IEEE's, so a vectorised expression that
keeps the header's parentheses keeps its bits."""
import math

import numpy as np

import nnscore_restated as nr
import rows_restated as rr
import voxel_restated as vr
import voxel_sort_restated as vsr

F32 = np.float32
VALUES = 29
MAX_CELLS = 1 << 21
DIAG = (8, 14, 19, 23, 26, 28)                              # H_aa among the 29 values
STATUS = ("converged", "max iterations", "max trials", "no hits", "not finite")
CELLS = ((0, 0, 0), (-1, 0, 0), (1, 0, 0), (0, -1, 0), (0, 1, 0), (0, 0, -1), (0, 0, 1))
PIVOT = 1e-12


def constants(o, h):
    h = float(F32(h))
    c1 = 10.0 * (1.0 - o)
    c2 = o / (h * h * h)
    d3 = -math.log(c2)
    d1 = -math.log(c1 + c2) - d3
    d2 = -2.0 * math.log((-math.log(c1 * math.exp(-0.5) + c2) - d3) / d1)
    return d1, d2


# ----------------------------------------------------------------------------------------------------------------------- the map

def gaussian(x64, min_points=6, min_eig_ratio=0.01):
    """x64 [3, n] float64, a voxel's members in ascending order -> (mu [3], A [6] or NaNs, valid)."""
    n = x64.shape[1]
    s = [float(x64[c, 0]) for c in range(3)]
    for k in range(1, n):
        for c in range(3):
            s[c] = s[c] + float(x64[c, k])
    mu = [s[c] / float(n) for c in range(3)]
    nan6 = [math.nan] * 6
    if n < min_points:
        return mu, nan6, 0
    acc = [0.0] * 6
    for k in range(n):
        d = [float(x64[c, k]) - mu[c] for c in range(3)]
        e = 0
        for r in range(3):
            for c in range(r, 3):
                acc[e] = acc[e] + d[r] * d[c]
                e += 1
    C = [v / float(n - 1) for v in acc]
    if not all(math.isfinite(v) for v in C) or not any(C):
        return mu, nan6, 0
    a = {(0, 0): C[0], (0, 1): C[1], (0, 2): C[2], (1, 1): C[3], (1, 2): C[4], (2, 2): C[5]}
    v = [[1.0, 0.0, 0.0], [0.0, 1.0, 0.0], [0.0, 0.0, 1.0]]
    for _ in range(rr.SWEEPS):
        if a[(0, 1)] == 0.0 and a[(0, 2)] == 0.0 and a[(1, 2)] == 0.0:
            break
        rr._rotate(a, v, 0, 1, 2)
        rr._rotate(a, v, 0, 2, 1)
        rr._rotate(a, v, 1, 2, 0)
    l = [a[(0, 0)], a[(1, 1)], a[(2, 2)]]
    lmax = l[0] if l[0] > l[1] else l[1]
    lmax = lmax if lmax > l[2] else l[2]
    if not lmax > 0.0:
        return mu, nan6, 0
    fl = min_eig_ratio * lmax
    with np.errstate(divide="ignore", over="ignore", invalid="ignore"):
        inv = [float(np.float64(1.0) / np.float64(fl if x < fl else x)) for x in l]
        A = [float(np.float64(((v[r][0] * inv[0]) * v[c][0] + (v[r][1] * inv[1]) * v[c][1]) + (v[r][2] * inv[2]) * v[c][2]))
             for r in range(3) for c in range(r, 3)]
    if not all(math.isfinite(x) for x in A):
        return mu, nan6, 0
    return mu, A, 1


def ndt_map(xyz, h, min_points=6, min_eig_ratio=0.01):
    """xyz [3, N] fp32, h -> dict of mean float64 [3,N], inv_cov float64 [6,N], valid, voxel_points int32 [N], count, origin
    float64 [3], h (the fp32 edge as fp64) and lookup: {(cx, cy, cz): voxel number}."""
    xyz = np.ascontiguousarray(xyz, dtype=F32)
    N = xyz.shape[1]
    hd = np.float64(F32(h))
    g = vr.voxel_fast(xyz, h)
    finite = np.isfinite(xyz).all(axis=0)
    origin = xyz[:, finite].min(axis=1).astype(np.float64) - 0.5 * hd if finite.any() else np.full(3, np.nan)
    out = {"mean": np.full((3, N), np.nan), "inv_cov": np.full((6, N), np.nan), "valid": np.zeros(N, np.int32),
           "voxel_points": g["voxel_points"], "count": np.int32(g["count"]), "origin": origin, "h": hd, "lookup": {}}
    M = int(g["count"])
    if M <= 0:
        return out
    members, start = vsr.member_lists(g["point_voxel"], M)
    x64 = xyz.astype(np.float64)
    for v in range(M):
        mem = members[start[v]:start[v] + g["voxel_points"][v]]
        mu, A, ok = gaussian(x64[:, mem], min_points, min_eig_ratio)
        out["mean"][:, v], out["inv_cov"][:, v], out["valid"][v] = mu, A, ok
        cell = np.floor((x64[:, mem[0]] - origin) / hd)
        out["lookup"][(int(cell[0]), int(cell[1]), int(cell[2]))] = v
    return out


def map_batch(xyz, h, min_points=6, min_eig_ratio=0.01):
    return [ndt_map(c, h, min_points, min_eig_ratio) for c in xyz]


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a.view(np.uint8), b.view(np.uint8))


# ----------------------------------------------------------------------------------------------------------------- the derivatives

def voxels_read(P, m, neighbors=7):
    """P [3, n] float64 (the moved points) -> int32 [n, 7]: the valid voxel read per cell, -1 where none."""
    n = P.shape[1]
    out = np.full((n, 7), -1, np.int32)
    if int(m["count"]) <= 0:
        return out
    with np.errstate(invalid="ignore", over="ignore"):
        cell = np.floor((P - m["origin"][:, None]) / m["h"])
    inside = ((cell >= 0) & (cell < MAX_CELLS)).all(axis=0)      # (a NaN fails)
    for i in np.flatnonzero(inside):
        c = (int(cell[0, i]), int(cell[1, i]), int(cell[2, i]))
        for k in range(neighbors):
            q = (c[0] + CELLS[k][0], c[1] + CELLS[k][1], c[2] + CELLS[k][2])
            if min(q) < 0 or max(q) >= MAX_CELLS:
                continue
            v = m["lookup"].get(q, -1)
            if v >= 0 and m["valid"][v]:
                out[i, k] = v
    return out


def _jdot(a, v, P):
    if a == 0:
        return v[2] * P[1] - v[1] * P[2]
    if a == 1:
        return v[0] * P[2] - v[2] * P[0]
    if a == 2:
        return v[1] * P[0] - v[0] * P[1]
    return v[a - 3]


def terms(P, mu, A6, d2, e=None):
    """The 28 fp64 terms of the header for n (point, voxel) pairs: P, mu [3, n], A6 [6, n] -> (e [n], T [28, n]): T[0] = e (f takes
    it with a minus), T[1:7] = w u_a, T[7:28] = the Hessian's terms, the upper triangle by rows."""
    nd2, nd2h = -d2, -(d2 * 0.5)
    A = [[A6[0], A6[1], A6[2]], [A6[1], A6[3], A6[4]], [A6[2], A6[4], A6[5]]]
    r = [P[c] - mu[c] for c in range(3)]
    Ar = [(A[i][0] * r[0] + A[i][1] * r[1]) + A[i][2] * r[2] for i in range(3)]
    q = (r[0] * Ar[0] + r[1] * Ar[1]) + r[2] * Ar[2]
    if e is None:
        e = np.exp(nd2h * q)
    w = d2 * e
    u = [_jdot(a, Ar, P) for a in range(6)]
    AJ = [[_jdot(a, A[i], P) for i in range(3)] for a in range(6)]
    rAS = {(0, 0): -(Ar[1] * P[1] + Ar[2] * P[2]), (0, 1): Ar[0] * P[1], (0, 2): Ar[0] * P[2],
           (1, 1): -(Ar[0] * P[0] + Ar[2] * P[2]), (1, 2): Ar[1] * P[2], (2, 2): -(Ar[0] * P[0] + Ar[1] * P[1])}
    T = [e] + [w * u[a] for a in range(6)]
    for a in range(6):
        for b in range(a, 6):
            inner = nd2 * (u[a] * u[b]) + _jdot(b, AJ[a], P)
            if b < 3:
                inner = inner + rAS[(a, b)]
            T.append(w * inner)
    return e, np.stack([np.broadcast_to(x, e.shape) for x in T])


def reduce_points(vals):
    """vals [29, Ns] -> [29]: per 256 points the butterfly 32 ... 1, the four waves ascending, the partials ascending from +0."""
    Ns = vals.shape[1]
    nblk = (Ns + 255) // 256
    pad = np.zeros((VALUES, nblk * 256))
    pad[:, :Ns] = vals
    v = pad.reshape(VALUES, nblk, 4, 64)
    lane = np.arange(64)
    for o in (32, 16, 8, 4, 2, 1):
        v = v + v[..., lane ^ o]
    w = v[..., 0]                                           # [29, nblk, 4]
    part = ((w[..., 0] + w[..., 1]) + w[..., 2]) + w[..., 3]
    tot = np.zeros(VALUES)
    for i in range(nblk):
        tot = tot + part[:, i]
    return tot


def derivatives_at(P, m, d2, neighbors=7, e=None, voxel=None):
    """The sums at the moved points P [3, Ns] float64.  voxel [Ns, 7]: a frozen assignment instead of the lookup; e [Ns, 7]:
    the exp per (point, cell) to use instead of numpy's.  -> dict: values [29] (f, hits, g, H), abs [29] (the sums of the
    absolute terms, for a tolerance), f, hits, g [6], H [21], e [Ns, 7], voxel [Ns, 7]."""
    Ns = P.shape[1]
    if voxel is None:
        voxel = voxels_read(P, m, neighbors)
    acc, mag = np.zeros((VALUES, Ns)), np.zeros((VALUES, Ns))
    e_out = np.full((Ns, 7), np.nan)
    for k in range(7):
        at = np.flatnonzero(voxel[:, k] >= 0)
        if not len(at):
            continue
        v = voxel[at, k]
        ek, T = terms(P[:, at], m["mean"][:, v], m["inv_cov"][:, v], d2, None if e is None else e[at, k])
        e_out[at, k] = ek
        acc[0, at] = acc[0, at] - T[0]
        acc[2:, at] = acc[2:, at] + T[1:]
        mag[0, at] = mag[0, at] + np.abs(T[0])
        mag[2:, at] = mag[2:, at] + np.abs(T[1:])
    acc[1] = (voxel >= 0).any(axis=1).astype(np.float64)
    with np.errstate(invalid="ignore", over="ignore"):
        tot, mtot = reduce_points(acc), mag.sum(axis=1)
    return {"values": tot, "abs": mtot, "f": tot[0], "hits": int(tot[1]) if math.isfinite(tot[1]) else 0, "g": tot[2:8], "H": tot[8:],
            "e": e_out, "voxel": voxel}


def moved64(src, R, t):
    """The device's fp32 moved points, widened."""
    R = np.eye(3, dtype=F32) if R is None else R
    t = np.zeros(3, F32) if t is None else t
    with np.errstate(invalid="ignore", over="ignore"):
        return nr.moved(src, R, t).astype(np.float64)


def derivatives(src, m, R=None, t=None, neighbors=7, outlier_ratio=0.55, e=None):
    """src [3, Ns] fp32 at the fp32 pose (R, t) against the map m -> derivatives_at's dict."""
    _, d2 = constants(outlier_ratio, m["h"])
    return derivatives_at(moved64(src, R, t), m, d2, neighbors, e)


def full(tri):
    """The upper triangle by rows (21 or 6 entries) -> the symmetric matrix."""
    n = 6 if len(tri) == 21 else 3
    H = np.zeros((n, n))
    H[np.triu_indices(n)] = tri
    return H + np.triu(H, 1).T


# ------------------------------------------------------------------------------------------------------------------------ the loop

def euler(x):
    """pl_euler: R = Rz(x2) Ry(x1) Rx(x0), t = x[3:6]."""
    s0, c0, s1, c1, s2, c2 = math.sin(x[0]), math.cos(x[0]), math.sin(x[1]), math.cos(x[1]), math.sin(x[2]), math.cos(x[2])
    return np.array([[c2 * c1, (c2 * s1) * s0 - s2 * c0, (c2 * s1) * c0 + s2 * s0],
                     [s2 * c1, (s2 * s1) * s0 + c2 * c0, (s2 * s1) * c0 - c2 * s0],
                     [-s1, c1 * s0, c1 * c0]]), np.array([x[3], x[4], x[5]])


def solve6(H21, g, lam):
    """pl_solve on H + lam I: (x, ok) by the Cholesky with the pivot rule of csrc/refine_solve6.h."""
    A = full(H21)
    A[np.diag_indices(6)] += lam
    L = np.zeros((6, 6))
    ok = True
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        for j in range(6):
            s = A[j, j] - float(np.dot(L[j, :j], L[j, :j]))
            ok = ok and math.isfinite(s) and s > PIVOT * A[j, j]
            d = math.sqrt(s) if s > 0 else math.nan
            L[j, j] = d
            for i in range(j + 1, 6):
                L[i, j] = (A[i, j] - float(np.dot(L[i, :j], L[j, :j]))) / d
        if not ok:
            return np.full(6, np.nan), False
        y = np.linalg.solve(L, -np.asarray(g))
        x = np.linalg.solve(L.T, y)
    return x, bool(np.isfinite(x).all())


def compose(x, R, t):
    Ri, ti = euler(x)
    return Ri @ R, Ri @ t + ti


def ndt(src, m, R=None, t=None, neighbors=7, outlier_ratio=0.55, max_iterations=30, rot_epsilon=1e-6, trans_epsilon=None,
        max_trials=None):
    """vcr_ndt_f32 decision by decision -> dict of R, t (fp32), score, hits, g, H, iterations, trials, converged, status, trace."""
    d1, d2 = constants(outlier_ratio, m["h"])
    trans_epsilon = 1e-6 * float(m["h"]) if trans_epsilon is None else trans_epsilon
    max_trials = 4 * max_iterations if max_trials is None else max_trials
    R64 = np.eye(3) if R is None else np.asarray(R, F32).astype(np.float64)
    t64 = np.zeros(3) if t is None else np.asarray(t, F32).astype(np.float64)

    def evaluate(Rd, td):
        return derivatives_at(moved64(src, Rd.astype(F32), td.astype(F32)), m, d2, neighbors)["values"]

    v = evaluate(R64, t64)
    trace = np.full(max_trials + 1, np.nan)
    trace[0] = v[0]
    st = {"iterations": 0, "trials": 0, "converged": 0, "status": 2}
    lam, nu = 1e-5 * max(abs(v[i]) for i in DIAG), 2.0
    live = True
    if not np.isfinite(v).all() or v[1] < 3.0:
        st["status"], live = (4 if not np.isfinite(v).all() else 3), False
    rnd = 0
    while live:
        if st["iterations"] >= max_iterations:
            st["status"] = 1
            break
        if rnd >= max_trials:
            st["status"] = 2
            break
        rnd += 1
        st["trials"] += 1
        x, ok = solve6(v[8:], v[2:8], lam)
        if not ok:
            with np.errstate(over="ignore"):
                lam, nu = lam * nu, nu * 2.0
            continue
        Rt, tt = compose(x, R64, t64)
        vt = evaluate(Rt, tt)
        if not np.isfinite(vt).all() or vt[1] < 3.0:
            st["status"] = 4 if not np.isfinite(vt).all() else 3
            break
        if vt[0] < v[0]:
            R64, t64, v = Rt, tt, vt
            st["iterations"] += 1
            lam, nu = lam * (1.0 / 3.0), 2.0
            trace[rnd] = v[0]
            if np.abs(x[:3]).max() < rot_epsilon and np.abs(x[3:]).max() < trans_epsilon:
                st["converged"], st["status"] = 1, 0
                break
        else:
            with np.errstate(over="ignore"):
                lam, nu = lam * nu, nu * 2.0
    Ns = src.shape[1]
    return dict(st, R=R64.astype(F32), t=t64.astype(F32), score=v[0], hits=int(v[1]), g=v[2:8], H=v[8:], trace=trace,
                probability=((-d1) * (-v[0])) / float(Ns))


# ---- the recipes the CPU and GPU tests share ----

def torus(seed, n, r0=0.35, noise=0.0):
    """n points of a bent, flattened torus' surface, [3, n] fp32: no axis of symmetry, so every pose coordinate is held."""
    rs = np.random.RandomState(seed)
    a, b = rs.uniform(0, 2 * np.pi, n), rs.uniform(0, 2 * np.pi, n)
    x = np.stack([(1.0 + r0 * np.cos(b)) * np.cos(a), 0.7 * (1.0 + r0 * np.cos(b)) * np.sin(a) + 0.2 * np.cos(2 * a),
                  r0 * np.sin(b) + 0.3 * np.cos(a)])
    return (x + noise * rs.standard_normal(x.shape)).astype(F32)


def pose(angle, shift, seed=0):
    """A rotation by `angle` about a seeded axis and a translation of length `shift`: (R [3,3], t [3]) float64."""
    rs = np.random.RandomState(1000 + seed)
    ax = rs.standard_normal(3)
    ax /= np.linalg.norm(ax)
    K = np.array([[0, -ax[2], ax[1]], [ax[2], 0, -ax[0]], [-ax[1], ax[0], 0]])
    R = np.eye(3) + math.sin(angle) * K + (1 - math.cos(angle)) * (K @ K)
    d = rs.standard_normal(3)
    return R, shift * d / np.linalg.norm(d)


RECOVERY = ((0.05, 0.03), (0.2, 0.1))                       # the start offsets of the recovery recipe (rad, length)
RECOVERY_H = 0.3


def recovery_case(i):
    """-> (src [3,500], tgt [3,700] fp32, R0, t0 fp32: the start pose, Rg, tg: the truth src -> tgt).  Two samplings of one torus;
    the source is the target's surface moved by the INVERSE of the offset, so the truth is the offset and the start the identity."""
    angle, shift = RECOVERY[i]
    tgt = torus(11, 700)
    Rg, tg = pose(angle, shift, seed=i)
    s = torus(12, 500).astype(np.float64)
    src = (Rg.T @ (s - tg[:, None])).astype(F32)
    return src, tgt, np.eye(3, dtype=F32), np.zeros(3, F32), Rg, tg


def pose_error(R, t, Rg, tg):
    """(angle of R Rg^T in rad, |t - tg|)."""
    c = (np.trace(np.asarray(R, np.float64) @ Rg.T) - 1.0) / 2.0
    return math.acos(max(-1.0, min(1.0, c))), float(np.linalg.norm(np.asarray(t, np.float64) - tg))
