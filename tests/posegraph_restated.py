"""include/posegraph/vcr_hip_posegraph.h restated in numpy float64: the residual and Jacobians of an
edge, the line process, the system in ascending edge order, the Levenberg-Marquardt loop with its stops, the pruning pass.
The edge terms repeat the kernel operation by operation (no fma on either side), vectorised over the edges; every sum over edges
runs in edge order.  The solve is a block Cholesky with the kernel's pivot rule whose sums numpy orders as it likes: that is
where the two differ by rounding (and in sin, cos and atan2).  Also the recipes the tests rest on."""
import functools

import numpy as np

PL_PIVOT = 1e-12
CRITERIA = {"max_iteration": 100, "max_iteration_lm": 20, "min_relative_increment": 1e-6, "min_relative_residual_increment": 1e-6,
            "min_right_term": 1e-6, "min_residual": 1e-6, "lower_scale_factor": 1.0 / 3.0, "upper_scale_factor": 2.0 / 3.0}


# ------------------------------------------------------------------------------------------------------------------ poses

def euler(x):
    """refine_solve6.h's pl_euler: R = Rz(x2) Ry(x1) Rx(x0), t = x[3:]."""
    x = np.asarray(x, np.float64)
    s0, c0, s1, c1, s2, c2 = np.sin(x[0]), np.cos(x[0]), np.sin(x[1]), np.cos(x[1]), np.sin(x[2]), np.cos(x[2])
    R = np.array([[c2 * c1, (c2 * s1) * s0 - s2 * c0, (c2 * s1) * c0 + s2 * s0],
                  [s2 * c1, (s2 * s1) * s0 + c2 * c0, (s2 * s1) * c0 - c2 * s0],
                  [-s1, c1 * s0, c1 * c0]], np.float64)
    return R, x[3:6].copy()


def vec6(R, t):
    """The inverse of euler, for arrays [..., 3, 3], [..., 3] -> [..., 6]."""
    R, t = np.asarray(R, np.float64), np.asarray(t, np.float64)
    sy = np.sqrt(R[..., 0, 0] * R[..., 0, 0] + R[..., 1, 0] * R[..., 1, 0])
    big = sy > 1e-6
    x0 = np.where(big, np.arctan2(R[..., 2, 1], R[..., 2, 2]), np.arctan2(-R[..., 1, 2], R[..., 1, 1]))
    x1 = np.arctan2(-R[..., 2, 0], sy)
    x2 = np.where(big, np.arctan2(R[..., 1, 0], R[..., 0, 0]), 0.0)
    return np.stack([x0, x1, x2, t[..., 0], t[..., 1], t[..., 2]], -1)


def _dot3(a0, b0, a1, b1, a2, b2):
    return (a0 * b0 + a1 * b1) + a2 * b2


def _dot6(a, b):
    """sum_p a[p] b[p], left to right; a, b lists of six arrays."""
    return ((((a[0] * b[0] + a[1] * b[1]) + a[2] * b[2]) + a[3] * b[3]) + a[4] * b[4]) + a[5] * b[5]


def step(x, R, t):
    """euler(x) (R, t): the update of one node."""
    Ri, ti = euler(x)
    Rn, tn = np.empty((3, 3)), np.empty(3)
    for r in range(3):
        for c in range(3):
            Rn[r, c] = _dot3(Ri[r, 0], R[0, c], Ri[r, 1], R[1, c], Ri[r, 2], R[2, c])
        tn[r] = _dot3(Ri[r, 0], t[0], Ri[r, 1], t[1], Ri[r, 2], t[2]) + ti[r]
    return Rn, tn


def inverse(R, t):
    return R.T.copy(), -R.T @ t


def compose(Ra, ta, Rb, tb):
    """(Ra, ta) after (Rb, tb)."""
    return Ra @ Rb, Ra @ tb + ta


# ------------------------------------------------------------------------------------------------------------------ edges

def valid_edges(src, dst, K):
    src, dst = np.asarray(src), np.asarray(dst)
    return (src >= 0) & (src < K) & (dst >= 0) & (dst < K) & (src != dst)


def edge_m(R, t, s, d, Re, te):
    """M = X^-1 T_dst^-1 T_src of every edge: (RP [E,3,3] = R_e^T R_d^T, RM [E,3,3], tM [E,3]), the kernel's products."""
    Rs, ts, Rd, td = R[s], t[s], R[d], t[d]
    E = len(s)
    RP, RM, tM, v = np.empty((E, 3, 3)), np.empty((E, 3, 3)), np.empty((E, 3)), np.empty((E, 3))
    for i in range(3):
        for j in range(3):
            RP[:, i, j] = _dot3(Re[:, 0, i], Rd[:, j, 0], Re[:, 1, i], Rd[:, j, 1], Re[:, 2, i], Rd[:, j, 2])
    w = ts - td
    for k in range(3):
        v[:, k] = _dot3(Rd[:, 0, k], w[:, 0], Rd[:, 1, k], w[:, 1], Rd[:, 2, k], w[:, 2]) - te[:, k]
    for i in range(3):
        tM[:, i] = _dot3(Re[:, 0, i], v[:, 0], Re[:, 1, i], v[:, 1], Re[:, 2, i], v[:, 2])
    for i in range(3):
        for j in range(3):
            RM[:, i, j] = _dot3(RP[:, i, 0], Rs[:, 0, j], RP[:, i, 1], Rs[:, 1, j], RP[:, i, 2], Rs[:, 2, j])
    return RP, RM, tM


def residuals(R, t, s, d, Re, te):
    """r_e [E,6] (indices must be valid: give blanks any valid pair and mask them afterwards)."""
    _, RM, tM = edge_m(R, t, s, d, Re, te)
    return vec6(RM, tM)


def jacobians(R, t, s, d, Re, te):
    """J_src [E,6,6] (J[e, p, k]: component p, generator k); J_dst = -J_src."""
    RP, _, _ = edge_m(R, t, s, d, Re, te)
    Rs, ts = R[s], t[s]
    J = np.zeros((len(s), 6, 6))
    for k in range(3):
        k1, k2 = (k + 1) % 3, (k + 2) % 3
        N = np.empty((len(s), 3, 3))
        for i in range(3):
            for j in range(3):
                N[:, i, j] = RP[:, i, k2] * Rs[:, k1, j] - RP[:, i, k1] * Rs[:, k2, j]
        J[:, 0, k] = (N[:, 2, 1] - N[:, 1, 2]) * 0.5
        J[:, 1, k] = (N[:, 0, 2] - N[:, 2, 0]) * 0.5
        J[:, 2, k] = (N[:, 1, 0] - N[:, 0, 1]) * 0.5
        for i in range(3):
            J[:, 3 + i, k] = RP[:, i, k2] * ts[:, k1] - RP[:, i, k1] * ts[:, k2]
            J[:, 3 + i, 3 + k] = RP[:, i, k]
    return J


def quad(r, info):
    """q_e = r^T info r and u = info r, the kernel's order."""
    u = [_dot6([info[:, p, c] for c in range(6)], [r[:, c] for c in range(6)]) for p in range(6)]
    return _dot6([r[:, p] for p in range(6)], u), u


def edge_terms(R, t, s, d, Re, te, info):
    """-> (q [E], W [E,6,6] = J^T info J (symmetric by construction), g [E,6] = J^T info r, r, J)."""
    r = residuals(R, t, s, d, Re, te)
    J = jacobians(R, t, s, d, Re, te)
    q, u = quad(r, info)
    E = len(s)
    W, g = np.empty((E, 6, 6)), np.empty((E, 6))
    for k in range(6):
        col = [J[:, p, k] for p in range(6)]
        g[:, k] = _dot6(col, u)
        c = [_dot6([info[:, p, m] for m in range(6)], col) for p in range(6)]
        for k0 in range(k + 1):
            W[:, k0, k] = _dot6([J[:, p, k0] for p in range(6)], c)
            W[:, k, k0] = W[:, k0, k]
    return q, W, g, r, J


def edge_sum(terms):
    """One term an edge, added in edge order (a blank's is 0)."""
    a = 0.0
    for v in np.asarray(terms, np.float64).tolist():
        a += v
    return a


class Graph:
    """A pose graph as the kernel takes it: K, src, dst [E], Re [E,3,3], te [E,3], info [E,6,6], uncertain [E]."""

    def __init__(self, src, dst, Re, te, info, uncertain, K):
        self.K = int(K)
        self.src, self.dst = np.asarray(src, np.int64), np.asarray(dst, np.int64)
        self.Re, self.te = np.asarray(Re, np.float64).reshape(-1, 3, 3), np.asarray(te, np.float64).reshape(-1, 3)
        self.info = np.asarray(info, np.float64).reshape(-1, 6, 6)
        self.unc = np.asarray(uncertain).astype(bool)
        self.valid = valid_edges(self.src, self.dst, self.K)
        self.s, self.d = np.where(self.valid, self.src, 0), np.where(self.valid, self.dst, 0)
        self.E = len(self.src)


def mu_of(g, alive, mcd):
    """max_correspondence_distance^2 times the mean of info[5][5] over the live uncertain edges, added in edge order."""
    a, n = 0.0, 0
    for e in range(g.E):
        if alive[e] and g.unc[e]:
            a += g.info[e, 5, 5]
            n += 1
    return (mcd * mcd) * (a / n) if n else 0.0


def line_process(q, unc, mu):
    """s = sqrt(l): 1 on a certain edge, mu / (mu + q) on an uncertain one."""
    with np.errstate(invalid="ignore", divide="ignore"):
        return np.where(unc, mu / (mu + q), 1.0)


def residual_terms(q, s, unc, alive, mu):
    with np.errstate(invalid="ignore", over="ignore"):
        return np.where(alive, (s * s) * q + np.where(unc, mu * ((s - 1.0) * (s - 1.0)), 0.0), 0.0)


def linearise(g, R, t, alive, mu, anchor=0, want_abs=False):
    """l, H, b and the residual at the poses (R, t).  -> dict(s, q, H [6K,6K], b [6K], res); want_abs: also "Habs", "babs", the
    sums of the absolute values of every elementary product l J info J / l J info r that enters an entry, and "nterms", their
    number an entry -- what the tests' allowances are made of."""
    K = g.K
    q, W, gg, r, J = edge_terms(R, t, g.s, g.d, g.Re, g.te, g.info)
    s = line_process(q, g.unc, mu)
    res = edge_sum(residual_terms(q, s, g.unc, alive, mu))
    H, b = np.zeros((6 * K, 6 * K)), np.zeros(6 * K)
    if want_abs:
        aJ, aI = np.abs(J), np.abs(g.info)
        Wabs = np.einsum("epk,epq,eqm->ekm", aJ, aI, aJ)
        gabs = np.einsum("epk,epq,eq->ek", aJ, aI, np.abs(r))
        Habs, babs, Hn, bn = np.zeros_like(H), np.zeros_like(b), np.zeros_like(H), np.zeros_like(b)
    for e in range(g.E):                                    # ascending edge index
        if not alive[e]:
            continue
        a, c = 6 * g.s[e], 6 * g.d[e]
        l = s[e] * s[e]
        term, gt = l * W[e], l * gg[e]
        H[a:a + 6, a:a + 6] += term
        H[c:c + 6, c:c + 6] += term
        H[a:a + 6, c:c + 6] -= term
        H[c:c + 6, a:a + 6] -= term
        b[a:a + 6] -= gt
        b[c:c + 6] += gt
        if want_abs:
            for (x, y) in ((a, a), (c, c), (a, c), (c, a)):
                Habs[x:x + 6, y:y + 6] += l * Wabs[e]
                Hn[x:x + 6, y:y + 6] += 36
            for x in (a, c):
                babs[x:x + 6] += l * gabs[e]
                bn[x:x + 6] += 36
    A = 6 * anchor
    H[A:A + 6, :] = 0.0
    H[:, A:A + 6] = 0.0
    H[A:A + 6, A:A + 6] = np.eye(6)
    b[A:A + 6] = 0.0
    out = dict(s=s, q=q, H=H, b=b, res=res)
    if want_abs:
        for M in (Habs, Hn):
            M[A:A + 6, :] = 0.0
            M[:, A:A + 6] = 0.0
        babs[A:A + 6] = 0.0
        bn[A:A + 6] = 0.0
        out.update(Habs=Habs, babs=babs, Hn=Hn, bn=bn)
    return out


def solve(H, lam, b):
    """(H + lambda I) d = b by a right-looking block Cholesky on 6 x 6 blocks, the pivot rule applied in the diagonal blocks
    against the diagonal of H + lambda I.  -> (d, ok)."""
    n = len(b)
    A = H + lam * np.eye(n)
    diag0 = np.diag(A).copy()
    L = np.zeros_like(A)
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        for j in range(0, n, 6):
            D, F = A[j:j + 6, j:j + 6], np.zeros((6, 6))
            for c in range(6):
                sv = D[c, c] - np.dot(F[c, :c], F[c, :c])
                if not (np.isfinite(sv) and sv > PL_PIVOT * diag0[j + c]):
                    return np.full(n, np.nan), False
                F[c, c] = np.sqrt(sv)
                for r in range(c + 1, 6):
                    F[r, c] = (D[r, c] - np.dot(F[r, :c], F[c, :c])) / F[c, c]
            L[j:j + 6, j:j + 6] = F
            if j + 6 < n:
                col = np.linalg.solve(F, A[j + 6:, j:j + 6].T).T
                L[j + 6:, j:j + 6] = col
                A[j + 6:, j + 6:] -= col @ col.T
        y = np.linalg.solve(L, b)
        d = np.linalg.solve(L.T, y)
    return d, bool(np.all(np.isfinite(d)))


def optimize(g, R, t, max_correspondence_distance, anchor=0, prune=True, edge_prune_threshold=0.25, criteria=None, trace=None, conds=None):
    """The header's call on one graph.  -> dict(R, t, weight, kept, residual [2], iterations [2], trials [2], converged); trace: a
    list that receives ("take" | "reject", pass) a trial; conds: a list that receives cond(H + lambda I) of every solve."""
    c = dict(CRITERIA, **(criteria or {}))
    K = g.K
    R, t = np.array(R, np.float64), np.array(t, np.float64)
    alive = g.valid.copy()
    s_last = np.full(g.E, np.nan)
    residual, iterations, trials, conv = [0.0, 0.0], [0, 0], [0, 0], 0
    res = 0.0
    for ps in range(2 if prune and c["max_iteration"] > 0 else 1):
        mu = mu_of(g, alive, max_correspondence_distance)
        lin = linearise(g, R, t, alive, mu, anchor)
        s_last = np.where(alive, lin["s"], s_last)
        res = lin["res"]
        if ps == 0:
            residual[0] = res
        lam, nu = 1e-5 * np.max(np.diag(lin["H"])), 2.0
        outer = ntr = 0
        stop, conv = 0, 0
        while not stop and outer < c["max_iteration"]:
            outer += 1
            taken = False
            for _ in range(c["max_iteration_lm"]):
                ntr += 1
                d, ok = solve(lin["H"], lam, lin["b"])
                if conds is not None and ok:
                    conds.append(float(np.linalg.cond(lin["H"] + lam * np.eye(6 * K))))
                if not ok:
                    stop = 2
                    break
                x = vec6(R, t).reshape(-1)
                nd2 = nx2 = den = 0.0
                for i in range(6 * K):
                    nd2 += d[i] * d[i]
                    den += d[i] * (lam * d[i] + lin["b"][i])
                for i in range(K):
                    nx2 += _dot6(list(x[6 * i:6 * i + 6]), list(x[6 * i:6 * i + 6]))
                if np.sqrt(nd2) <= c["min_relative_increment"] * (np.sqrt(nx2) + c["min_relative_increment"]):
                    stop, conv = 1, 1
                    break
                Rn, tn = np.empty_like(R), np.empty_like(t)
                for i in range(K):
                    Rn[i], tn[i] = step(d[6 * i:6 * i + 6], R[i], t[i])
                qn, _ = quad(residuals(Rn, tn, g.s, g.d, g.Re, g.te), g.info)
                res_new = edge_sum(residual_terms(qn, lin["s"], g.unc, alive, mu))
                with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
                    rho = (res - res_new) / (den + 1e-3)
                if rho > 0:
                    taken = True
                    if trace is not None:
                        trace.append(("take", ps))
                    R, t = Rn, tn
                    small = np.sqrt(res) - np.sqrt(res_new) < c["min_relative_residual_increment"] * np.sqrt(res)
                    res = res_new
                    if small:
                        stop, conv = 1, 1
                        break
                    cc = 2.0 * rho - 1.0
                    lam, nu = lam * max(c["lower_scale_factor"], 1.0 - (cc * cc) * cc), 2.0
                    lin = linearise(g, R, t, alive, mu, anchor)
                    s_last = np.where(alive, lin["s"], s_last)
                    if np.max(np.abs(lin["b"])) <= c["min_right_term"]:
                        stop, conv = 1, 1
                    break
                if trace is not None:
                    trace.append(("reject", ps))
                lam, nu = lam * nu, nu * 2.0
            if not stop and res < c["min_residual"]:
                stop, conv = 1, 1
        iterations[ps], trials[ps] = outer, ntr
        if stop == 2:
            break
        if prune and ps == 0:
            with np.errstate(invalid="ignore"):
                alive = alive & ~(g.unc & (s_last * s_last < edge_prune_threshold))
    residual[1] = res
    with np.errstate(invalid="ignore"):
        weight = np.where(g.valid, s_last * s_last, np.nan)
    return dict(R=R, t=t, weight=weight, kept=alive.astype(np.int32), residual=np.array(residual), iterations=np.array(iterations, np.int32),
                trials=np.array(trials, np.int32), converged=int(conv))


# ------------------------------------------------------------------------------------------------------------------ recipes

def pose_error(R, t, R_true, t_true):
    """Mean over the nodes of the rotation angle (rad) and of the translation distance between two sets of poses."""
    ang = [np.arccos(np.clip((np.trace(R[i].T @ R_true[i]) - 1.0) / 2.0, -1.0, 1.0)) for i in range(len(R))]
    return float(np.mean(ang)), float(np.mean(np.linalg.norm(np.asarray(t) - np.asarray(t_true), axis=1)))


def small_info(rs, n=60, spread=0.5):
    """An information matrix with a real count: robust_restated.information on a cloud of n points every one an inlier."""
    import robust_restated as ro
    tgt = rs.uniform(-spread, spread, (3, n)).astype(np.float32)
    return ro.information(tgt, np.arange(n), np.zeros(n, np.float32), 0.05)


MCD = 0.05                                                   # the recipes' max_correspondence_distance


@functools.lru_cache(maxsize=None)
def ring(seed=3, K=8, odo_noise=0.01, wrong=0.5):
    """K nodes on a ring with planted poses (node 0 the identity); K - 1 odometry edges (i, i + 1), each with a small planted
    error; uncertain edges (i, i + 2) and the closing edge (K - 1, 0), true but for ONE, (1, 3), whose X is wrong by about
    `wrong` rad; information matrices from small clouds.  -> dict(graph, R0, t0 (the chained odometry), R_true, t_true,
    wrong_edge).  Shared between the tests: read only."""
    rs = np.random.RandomState(seed)
    R_true, t_true = [np.eye(3)], [np.zeros(3)]
    for i in range(1, K):
        a = 2 * np.pi * i / K
        Ri, _ = euler([rs.uniform(-0.2, 0.2), rs.uniform(-0.2, 0.2), a, 0, 0, 0])
        R_true.append(Ri)
        t_true.append(np.array([np.cos(a) - 1.0, np.sin(a), rs.uniform(-0.1, 0.1)]))
    R_true, t_true = np.array(R_true), np.array(t_true)

    def rel(i, j):                                          # X: frame i -> frame j = T_j^-1 T_i
        Rj, tj = inverse(R_true[j], t_true[j])
        return compose(Rj, tj, R_true[i], t_true[i])

    src, dst, Re, te, info, unc = [], [], [], [], [], []
    for i in range(K - 1):                                  # odometry, with its planted error
        Rx, tx = rel(i, i + 1)
        Rn, tn = euler(rs.normal(0, odo_noise, 6))
        Rx, tx = compose(Rn, tn, Rx, tx)
        src.append(i); dst.append(i + 1); Re.append(Rx); te.append(tx); info.append(small_info(rs)); unc.append(0)
    wrong_edge = None
    for i, j in [(i, i + 2) for i in range(K - 2)] + [(K - 1, 0)]:
        Rx, tx = rel(i, j)
        if (i, j) == (1, 3):
            Rn, tn = euler([0.3, -0.25, wrong * 0.6, 0.2, -0.15, 0.1])
            Rx, tx = compose(Rn, tn, Rx, tx)
            wrong_edge = len(src)
        src.append(i); dst.append(j); Re.append(Rx); te.append(tx); info.append(small_info(rs)); unc.append(1)
    g = Graph(src, dst, Re, te, info, unc, K)
    R0, t0 = [np.eye(3)], [np.zeros(3)]
    for i in range(K - 1):                                  # T_{i+1} = T_i X^-1
        Ri, ti = inverse(g.Re[i], g.te[i])
        Rn, tn = compose(R0[-1], t0[-1], Ri, ti)
        R0.append(Rn); t0.append(tn)
    out = dict(graph=g, R0=np.array(R0), t0=np.array(t0), R_true=R_true, t_true=t_true, wrong_edge=wrong_edge)
    for v in list(out.values()) + [g.src, g.dst, g.Re, g.te, g.info, g.unc, g.valid, g.s, g.d]:
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def triangle(seed=11):
    """K = 3, the three edges plus a DUPLICATE of (0, 1) (slightly different), one of them uncertain; poses a little off."""
    rs = np.random.RandomState(seed)
    R_true, t_true = [np.eye(3)], [np.zeros(3)]
    for i in range(1, 3):
        Ri, ti = euler(rs.uniform(-0.5, 0.5, 6))
        R_true.append(Ri); t_true.append(ti)
    src, dst, Re, te, info, unc = [], [], [], [], [], []
    for (i, j), u in (((0, 1), 0), ((1, 2), 0), ((2, 0), 1), ((0, 1), 1)):
        Rj, tj = inverse(R_true[j], t_true[j])
        Rx, tx = compose(Rj, tj, R_true[i], t_true[i])
        Rn, tn = euler(rs.normal(0, 0.02, 6))
        Rx, tx = compose(Rn, tn, Rx, tx)
        src.append(i); dst.append(j); Re.append(Rx); te.append(tx); info.append(small_info(rs)); unc.append(u)
    g = Graph(src, dst, Re, te, info, unc, 3)
    R0 = np.array([step(rs.normal(0, 0.03, 6), R_true[i], t_true[i])[0] if i else np.eye(3) for i in range(3)])
    t0 = np.array([step(rs.normal(0, 0.03, 6), R_true[i], t_true[i])[1] if i else np.zeros(3) for i in range(3)])
    return dict(graph=g, R0=R0, t0=t0, R_true=np.array(R_true), t_true=np.array(t_true))


@functools.lru_cache(maxsize=None)
def chain(K=128, closures=13, seed=5):
    """A chain of K nodes with `closures` true uncertain closures (i, i + 10 ...): the largest graph the kernel takes."""
    rs = np.random.RandomState(seed)
    R_true, t_true = [np.eye(3)], [np.zeros(3)]
    for i in range(1, K):
        Ri, ti = step(np.concatenate([rs.uniform(-0.1, 0.1, 3), rs.uniform(-0.2, 0.2, 3) + [0.3, 0, 0]]), R_true[-1], t_true[-1])
        R_true.append(Ri); t_true.append(ti)
    src, dst, Re, te, info, unc = [], [], [], [], [], []
    pairs = [(i, i + 1, 0) for i in range(K - 1)] + [(int(i), int(i) + 10, 1) for i in rs.choice(K - 10, closures, replace=False)]
    for i, j, u in pairs:
        Rj, tj = inverse(R_true[j], t_true[j])
        Rx, tx = compose(Rj, tj, R_true[i], t_true[i])
        Rn, tn = euler(rs.normal(0, 0.003, 6))
        Rx, tx = compose(Rn, tn, Rx, tx)
        src.append(i); dst.append(j); Re.append(Rx); te.append(tx); info.append(small_info(rs)); unc.append(u)
    g = Graph(src, dst, Re, te, info, unc, K)
    R0, t0 = [np.eye(3)], [np.zeros(3)]
    for i in range(K - 1):
        Ri, ti = inverse(g.Re[i], g.te[i])
        Rn, tn = compose(R0[-1], t0[-1], Ri, ti)
        R0.append(Rn); t0.append(tn)
    return dict(graph=g, R0=np.array(R0), t0=np.array(t0), R_true=np.array(R_true), t_true=np.array(t_true))
